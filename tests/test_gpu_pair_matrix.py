"""GPU tests of every instantiation of the two-sub-steps kernel (csrc/evp_fused2.hip, k_pair) a configuration can select.

tests/pair_matrix.py crosses the ingredients the launch code selects an instantiation by -- kernel family, coefficient kind,
compile-time forcing kinds -- and states the selection rule once (expected_key); this file runs every case of that matrix on both
orders of the first sub-step and on the three transports:

  a. untiled, against the CPU oracle, two sub-steps from first = 1 and from first = 2, on the bounds of
     test_even_start_two_substeps_vs_oracle (u, v within 1e-13 max|u, v|, sigma on owned cells within 1e-10 max|sigma|, identical
     zero-velocity sets, everything finite).  scripts/order_sensitivity.py shows for every case that the oracle's other order, and the
     oracle's answer without the case's distinguishing ingredient, lie orders of magnitude outside those bounds
     (profiles/r12_pair_matrix.md);
  b. untiled, bit for bit against the three-kernel path, n = 2 and 3 sub-steps (3: a pair and a trailing single sub-step);
  c. PEER1 DLD0: one tile connected to itself on the peer transport, against the untiled run and the three-kernel run;
  d. PEER1 DLD1: two peer-connected tiles of a Bounded x direction (unequal row strides), one host thread each, against the
     untiled run.

Everything goes through csi_evp_initialize / csi_evp_subcycle(dt, n, first) / csi_evp_finalize, and every test asserts fusion level 2,
the launch count and, on tiles, the peer transport: a silent fall-back to the three kernels or to the message exchange fails.  Which
kernel names the launches carry is measured, not asserted (scripts/pair_instantiation_coverage.py).
"""
import ctypes as C

import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import pair_matrix as pm
from test_gpu_evp import DIAG, EVP_FIELDS, cmp_region
from test_gpu_local_tiles import run_tile_threads
from test_gpu_pair_ufirst import STATE, assert_close_to_oracle, assert_pair_path, pair_launches, subcycle

pytestmark = pytest.mark.gpu

NAMES = list(pm.MATRIX)
TILED = sorted(pm.COMBOS)
DLD_NAMES = [n for n in TILED if pm.dld_case(n) is not None]


# ---- a: against the oracle, both parities ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_matrix_two_substeps_vs_oracle(name, first, oracle_lib):
    """Sub-steps first, first + 1 in one launch, from the state set! leaves, with the oracle's ice strength copied in: the bounds of
    test_even_start_two_substeps_vs_oracle, for every case of the matrix and both orders."""
    c = cases.make_case(substeps=2, **pm.MATRIX[name])
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="fast")
    m.set_fusion(2)
    for k in ("u", "v"):
        assert np.array_equal(EVP_FIELDS[k](m).numpy(), p.f[k]), f"{k} after update_state!"
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    m.copy_to_field(m.dynamics.auxiliaries.fields.P, p.f["P"])
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], first, first + 1)
    subcycle(m, c, 2, first)
    assert_pair_path(m, c, 2, (name, first))
    assert_close_to_oracle(m, p, f"{name} first = {first}:")


# ---- b: bit for bit against the three-kernel path ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [1, 2])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_matrix_bitwise_equal_three_kernel_path(name, n, first):
    """set_fusion(2) equals set_fusion(0) on the fields and regions of test_even_start_bitwise_equal_three_kernel_path: u, v, s11, s22 on
    whole parents, s12 too without walls and on the interior with them, the diagnostics' interiors after csi_evp_finalize."""
    c = cases.make_case(substeps=n, **pm.MATRIX[name])
    walls = "bounded" in c["topo"]
    out = {}
    for fusion in (0, 2):
        m = cases.csi_model(c, mode="fast")
        m.set_fusion(fusion)
        m.ctx.call("csi_evp_initialize")
        subcycle(m, c, n, first)
        if fusion == 2:
            assert_pair_path(m, c, n, (name, n, first))
        else:
            assert m.ctx.last_path()["level"] == 0 and m.ctx.launches_per_substep() == 3
        m.ctx.call("csi_evp_finalize")
        m.synchronize()
        out[fusion] = {k: EVP_FIELDS[k](m).numpy().copy() for k in ("u", "v", "s11", "s22") + (() if walls else ("s12",))}
        out[fusion].update({k: EVP_FIELDS[k](m).interior_numpy().copy() for k in DIAG + (("s12",) if walls else ())})
    for k in out[0]:
        a, b = out[0][k], out[2][k]
        assert np.all(np.isfinite(b)), (name, k)
        assert np.array_equal(a, b), (name, n, first, k, np.abs(a - b).max(), np.argwhere(a != b)[:5])


# ---- c, d: the peer transport ---------------------------------------------------------------------------------------------------------

def exchange_forcing_halos(m, c):
    """what csi_time_step_momentum does before its sub-cycle and csi_evp_subcycle leaves to the caller (include/csi.h): the halos of the
    stress and forcing arrays beyond connected sides"""
    on = {"TOP": c.get("field_forcing") or c.get("wind_drag") == "arrays", "BOT": c.get("field_forcing") or c.get("bottom") == "arrays",
          "FORCING": c.get("user_forcing")}
    names = [f"{slot}_{comp}" for slot in ("TOP", "BOT", "FORCING") if on[slot] for comp in ("U", "V")]
    if names:
        ids = (C.c_int32 * len(names))(*[csi._lib.F[x] for x in names])
        m.ctx.call("csi_halo_exchange", ids, len(names), int(c["H"]))


def both_parities(m, c, n):
    """initialize, csi_evp_subcycle of n sub-steps from first = 1, then of n sub-steps from first = 2, finalize"""
    m.ctx.call("csi_evp_initialize")
    subcycle(m, c, n, 1)
    subcycle(m, c, n, 2)
    m.ctx.call("csi_evp_finalize")


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", TILED)
def test_matrix_peer_self_connected_bitwise(name, n):
    """One tile connected to itself (test_peer_halo_transport_self_connected_bitwise), every family x coefficient kind x forcing kind at
    128 .. 160 columns: two calls in a row on one context, v-first then u-first, so the launch numbers of the flag protocol carry on.
    Whole parents of u, v, sigma equal the untiled fusion-2 run for n = 2, interiors for n = 3 (the untiled run's trailing launch may be
    another kernel); interiors, the diagnostics' included, equal the three-kernel run."""
    kw, connected = pm.peer_case(name)
    c = cases.make_case(substeps=n, **kw)
    three = cases.csi_model(c, mode="fast")
    three.set_fusion(0)
    ref = cases.csi_model(c, mode="fast")
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, connected))
    exchange_forcing_halos(til, c)
    for m in (three, ref, til):
        both_parities(m, c, n)
    three.synchronize(); ref.synchronize(); til.synchronize()
    path = til.ctx.last_path()
    assert til.ctx.halo_transport() == "peer" and path["exchanges"] == 1, path
    assert_pair_path(til, c, n, "tile")
    assert_pair_path(ref, c, n, "untiled")
    assert three.ctx.last_path()["level"] == 0
    for f in STATE:
        get = (lambda m: EVP_FIELDS[f](m).numpy()) if n % 2 == 0 else (lambda m: EVP_FIELDS[f](m).interior_numpy())
        a, b = get(ref), get(til)
        assert np.all(np.isfinite(b)), (name, f)
        assert np.array_equal(a, b), (name, f, "against the untiled run", np.abs(a - b).max(), np.argwhere(a != b)[:5])
    for f in STATE + DIAG:
        a, b = EVP_FIELDS[f](three).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (name, f, "against the three kernels", np.abs(a - b).max(), np.argwhere(a != b)[:5])


@pytest.mark.parametrize("first", [1, 2])
@pytest.mark.parametrize("name", DLD_NAMES)
def test_matrix_bounded_x_tiles_bitwise(name, first):
    """Two 128-column tiles of a Bounded x direction on the peer transport (exchange interval 0), one host thread per tile: the eastern
    tile's Face fields are one column wider, so each tile's neighbour has another row stride (the DLD instantiations).  Two sub-steps
    from `first`; the owned cells of every tile equal the untiled run bit for bit."""
    n = 2
    c = cases.make_case(substeps=n, **pm.dld_case(name))
    ref = cases.csi_model(c, mode="fast")
    ref.ctx.call("csi_evp_initialize")
    subcycle(ref, c, n, first)
    assert_pair_path(ref, c, n, "untiled")
    ref.ctx.call("csi_evp_finalize")
    ref.synchronize()
    want = {f: EVP_FIELDS[f](ref).interior_numpy().copy() for f in STATE}

    def tile(rank, group):
        m = cases.csi_model(c, mode="fast", tile=(2, 1, rank), local_group=group)
        m.set_exchange_interval(0)
        exchange_forcing_halos(m, c)
        m.ctx.call("csi_evp_initialize")
        subcycle(m, c, n, first)
        path = dict(m.ctx.last_path(), transport=m.ctx.halo_transport(), launches=m.ctx.last_launches())
        m.ctx.call("csi_evp_finalize")
        m.synchronize()
        g = m.grid
        res = dict(path=path, offsets=(g.i_off, g.j_off, g.Nx, g.Ny), **{f: EVP_FIELDS[f](m).interior_numpy().copy() for f in STATE})
        del m
        return res

    for rank, d in enumerate(run_tile_threads(2, tile)):
        assert d["path"]["transport"] == "peer" and d["path"]["level"] == 2, (name, rank, d["path"])
        assert d["path"]["launches"] == (pair_launches(c, n), n), (name, rank, d["path"])
        i0, j0, nx, ny = d["offsets"]
        for f in STATE:
            got, w = d[f][:ny, :nx], want[f][j0:j0 + ny, i0:i0 + nx]
            assert np.all(np.isfinite(got)), (name, rank, f)
            assert np.array_equal(got, w), (name, first, "rank", rank, f, np.abs(got - w).max(), np.argwhere(got != w)[:4].tolist())


def test_refused_configurations_are_refused_by_name():
    """pair_matrix.UNREACHABLE lists the tiled instantiations that stay unreachable because the library refuses their configuration on
    tiles; each listed refusal is asserted here (REFUSALS: key -> a callable that must raise csi.CsiError)."""
    assert set(REFUSALS) == set(pm.UNREACHABLE)
    for key, attempt in REFUSALS.items():
        with pytest.raises(csi.CsiError):
            attempt()


REFUSALS = {}
