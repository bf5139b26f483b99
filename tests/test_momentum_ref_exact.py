"""tests/momentum_ref.py over its number type, without a GPU.

  * Ref(p, num=float) is the restatement the STRICT kernels are compared with bit for bit.  Making the number type a parameter must not
    change one bit of it: tests/golden/momentum_ref/float_restatement.npz holds what the restatement gave before it had the parameter (a viscous
    sub-cycle, an explicit tendency and step for both rheologies, on two cases of test_gpu_momentum_variants.CASES).
  * Ref(p, num=fast_math_ref.CTX) evaluates the same expressions in 80-digit decimal arithmetic.  Rounded to double it must lie within a
    few ulp of max|Q| of the double evaluation -- were a term missing, a sign wrong or an operand not converted exactly, the two would
    differ in the leading digits -- and the exact path refuses a case with free drift.
"""
import os

import numpy as np
import pytest

import cases
import momentum_variant_shapes as mv
import test_gpu_momentum_variants as variants          # (for its CASES; importing it needs no GPU)
from fast_math_ref import CTX, U
from momentum_ref import Ref, rel_error

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "momentum_ref", "float_restatement.npz")
GOLDEN_CASES = {
    "periodic_fplane": dict(Nx=24, Ny=20, random_uv=0.03),
    "channel_wind_arrays": dict(Nx=22, Ny=18, topo=("periodic", "bounded"), wind_drag="arrays", bottom="arrays", random_uv=0.03),
}


def float_record(kw):
    """what the golden file records of one case (whole parents)"""
    out = {}
    c = cases.make_case(substeps=3, **kw)
    p = cases.oracle_problem(c)
    Ref(p, nu=mv.NU).time_step_momentum(c["dt"], 3)
    out["split_u"], out["split_v"] = p.f["u"].copy(), p.f["v"].copy()
    for rheology in ("viscous", "evp"):
        p = cases.oracle_problem(c)
        if rheology == "evp":
            mv.seed_sigma(p)
        r = Ref(p, nu=mv.NU, viscous=rheology == "viscous")
        r.compute_tendencies(60.0)
        r.explicit_step(60.0)
        out[f"{rheology}_Gu"], out[f"{rheology}_Gv"] = r.Gu.copy(), r.Gv.copy()
        out[f"{rheology}_u"], out[f"{rheology}_v"] = p.f["u"].copy(), p.f["v"].copy()
    return out


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_float_restatement_unchanged_bit_for_bit(name, oracle_lib):
    assert dict(variants.CASES)[name] == GOLDEN_CASES[name]                  # two of the existing cases, as they are there
    want = np.load(GOLDEN)
    got = float_record(GOLDEN_CASES[name])
    assert sorted(f"{name}/{k}" for k in got) == sorted(k for k in want.files if k.startswith(name + "/"))
    for k, a in got.items():
        b = want[f"{name}/{k}"]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, k, float(np.abs(a - b).max()))
        assert np.abs(a).max() > 0


# The bound of the sanity check.  A quantity is a sum of at most six terms (Coriolis, two stresses, divergence, immersed flux, forcing),
# each a chain of at most a dozen correctly rounded operations, so the double evaluation is within about 12 u of the sum of the terms'
# magnitudes; the terms of the stress divergence cancel (differences of neighbouring stresses), which makes that sum a small multiple
# of max|Q|.  64 u = 32 ulp allows a factor five for it; a wrong term is off by 1e-2 and more.
SANITY_U = 64


@pytest.mark.parametrize("name", [n for n, kw in mv.EXACT_CASES if (kw["Nx"], kw["Ny"]) == (65, 5)])
def test_exact_path_agrees_with_the_double_one(name, oracle_lib):
    ref = mv.exact_references(name)
    assert len(ref) == 10
    for quantity, (Qf, Qx) in ref.items():
        assert Qf.shape == Qx.shape == (5, 65)
        e = rel_error(Qf, Qx, CTX)
        print(f"[momentum-ref-exact] {name} | {quantity} | e_ref = {e:.3e} = {e / U:.2f} u")
        assert 0 < e <= SANITY_U * U, (name, quantity, e / U)
        # the exact value rounded once is the double evaluation up to that error, and it has the same zeros (open water, land)
        rounded = np.array([float(x) for x in Qx.ravel()]).reshape(Qx.shape)
        assert np.array_equal(rounded == 0.0, Qf == 0.0), (name, quantity)


def test_exact_path_refuses_free_drift(oracle_lib):
    c = cases.make_case(Nx=12, Ny=10, random_uv=0.03, free_drift=True)
    with pytest.raises(AssertionError, match="free drift"):
        Ref(cases.oracle_problem(c), num=CTX)
