"""The cases of tests/test_gpu_momentum_variant_shapes.py, stated once (no GPU needed to read them; tests/test_momentum_variant_shapes_table.py
checks the coverage they claim).

The five kernels of csrc/momentum_viscous.hip and csrc/momentum_explicit.hip launch 64 x 4 threads, one velocity point per thread, over
the interior range.  tests/test_gpu_momentum_variants.py checks their values on grids of at most 24 x 20 cells with halo (4, 4): one
block in x, equal halos.  This table takes the same physics to the smallest grids at which such a launch has a seam or a ragged edge in
each direction, under every halo pair the entry point accepts in kind (the minimum, equal, wider in x, wider in y), on every topology
and metric kind.

A case is a `cases.make_case` keyword set.  The table is not the full product (4 shapes x 4 halos x 4 topologies x 3 metric kinds x 9
physics sets = 1728): the shape and the topology run through their 16 pairs four times, and the halo, the metric kind and the physics
rotate with the case index, with strides chosen so that the coverage conditions of the table test hold.  64 cases.

Nothing had to be omitted: `make_case` builds bounded x periodic on all three metric kinds (the latitude-longitude grid is then
periodic in latitude as far as the halo images go; the metrics stay per row), so that topology is in the table for each of them.
Two rules adapt a physics set to the geometry it lands on; both are stated in `case_kw`:
  * `noslip` puts a ValueBoundaryCondition on the tangential velocity at every wall: it is kept on bounded x bounded only (where the
    existing case has it); on the other topologies that set keeps its BetaPlane and loses the walls' condition.
  * the curvilinear metric kind comes with per-point Coriolis planes (`coriolis_points`), except under a physics set that has no
    Coriolis force (`coriolis=None`): that set stays without one.  The library takes per-point planes on grids with full 2-D metrics
    only (csi_coriolis_points_set refuses the others), so the `points` set keeps them on the curvilinear kind and is an f-plane on the
    uniform and latitude-longitude kinds.
"""
SHAPES = [(63, 3), (64, 4), (65, 5), (130, 9)]         # one thread short of a 64 x 4 block both ways; exact; one point over; third block, partial
MULTI_BLOCK = [(65, 5), (130, 9)]
HALOS = [(2, 2), (4, 4), (5, 3), (3, 5)]               # the smallest the momentum step accepts; the usual; unequal both ways
TOPOLOGIES = [("periodic", "periodic"), ("bounded", "bounded"), ("periodic", "bounded"), ("bounded", "periodic")]
METRICS = {"uniform": {}, "latlon": dict(grid="latlon"), "curvilinear": dict(curvilinear=0.15, coriolis_points=True)}
BLOCK = (64, 4)

IBC = ((0.02, -0.03, 0.01, 0.04), (0.03, 0.01, -0.02, 0.02))
# the nine keyword sets of test_gpu_momentum_variants.CASES without their sizes, topologies and metric kinds (the table test compares)
PHYSICS = [
    ("fplane", dict(random_uv=0.03)),
    ("none_forcing", dict(random_uv=0.03, coriolis=None, user_forcing=True, free_drift=True)),
    ("noslip_beta", dict(noslip=True, beta=2e-11, random_uv=0.03)),
    ("wind_arrays", dict(wind_drag="arrays", bottom="arrays", random_uv=0.03)),
    ("rows_forcing", dict(random_uv=0.03, user_forcing=True)),
    ("fields_free_drift", dict(field_forcing=True, free_drift=True, random_uv=0.03)),
    ("points", dict(coriolis_points=True, random_uv=0.03)),
    ("masked_immersed", dict(land=0.15, immersed_bc=IBC, random_uv=0.03, wind_drag="numbers", coriolis=None)),
    ("masked_forcing", dict(land=0.12, immersed_bc=IBC, user_forcing=True, free_drift=True, beta=2e-11, random_uv=0.03)),
]

CONFIGURATIONS = ["viscous_split", "viscous_explicit", "evp_explicit"]
NU = 1000.0
SPLIT_SUBSTEPS = 3


def halos_for(shape):
    """the halo pairs a grid of this shape is not refused with (need_dynamics_common: Nx >= Hx, Ny >= Hy, both >= 2)"""
    return [h for h in HALOS if h[0] <= shape[0] and h[1] <= shape[1] and min(h) >= 2]


def case_kw(shape, halo, topo, metric, physics):
    kw = dict(Nx=shape[0], Ny=shape[1], H=halo, topo=topo)
    kw.update(dict(PHYSICS)[physics])
    kw.update(METRICS[metric])
    if kw.get("noslip") and topo != ("bounded", "bounded"):
        del kw["noslip"]
    if metric != "curvilinear":
        kw.pop("coriolis_points", None)
    elif "coriolis" in kw and kw["coriolis"] is None:
        del kw["coriolis_points"]
    return kw


def _table():
    out = []
    names = list(METRICS)
    for k in range(64):
        r = k // 16
        shape, topo = SHAPES[(k // 4) % 4], TOPOLOGIES[k % 4]
        allowed = halos_for(shape)
        halo = allowed[(k + r) % len(allowed)]
        metric = names[k % 3]
        physics = PHYSICS[(k + r) % 9][0]
        name = f"{k:02d}_{shape[0]}x{shape[1]}_H{halo[0]}x{halo[1]}_{topo[0][0]}{topo[1][0]}_{metric}_{physics}"
        out.append(dict(name=name, shape=shape, halo=halo, topo=topo, metric=metric, physics=physics,
                        kw=case_kw(shape, halo, topo, metric, physics)))
    return out


TABLE = _table()


def cases_for(configuration):
    """Every configuration runs the whole table (the stored sigma, u^n and v^n of evp_explicit are seeded by the test)."""
    assert configuration in CONFIGURATIONS
    return TABLE


# ---- the cases of the exact-arithmetic comparison: no free drift (that value comes from the C oracle, in double) ------------------------
EXACT_PHYSICS = {
    "uniform_periodic_fplane": dict(topo=("periodic", "periodic"), random_uv=0.03),
    "latlon_channel_forcing": dict(topo=("periodic", "bounded"), grid="latlon", random_uv=0.03, user_forcing=True),
    "curvilinear_points": dict(topo=("bounded", "bounded"), curvilinear=0.15, coriolis_points=True, random_uv=0.03),
    "masked_immersed_wind": dict(topo=("periodic", "bounded"), land=0.15, immersed_bc=IBC, random_uv=0.03, wind_drag="numbers", coriolis=None),
}
EXACT_SHAPES = {(65, 5): (2, 2), (130, 9): (5, 3)}      # shape -> halo
EXACT_CASES = [(f"{n}_{s[0]}x{s[1]}", dict(Nx=s[0], Ny=s[1], H=h, **kw)) for n, kw in EXACT_PHYSICS.items() for s, h in EXACT_SHAPES.items()]
K_FAST = 4.0           # the asserted margin of FAST's error over the reference order's own (see test_gpu_momentum_variant_shapes.py)
EXACT_DT = 60.0
SIGMA_SEED = 5


def seed_sigma(p, seed=SIGMA_SEED):
    """Stored stresses and u^n, v^n that are not zero, drawn as test_gpu_momentum_variants._set_sigma draws them, into the oracle
    problem's arrays; returns them by name (the GPU tests copy the same arrays into the model's fields)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = {}
    for k in ("s11", "s22", "s12", "un", "vn"):
        a = 50.0 * rng.standard_normal(p.f[k].shape) if k.startswith("s") else 0.02 * rng.standard_normal(p.f[k].shape)
        p.f[k][...] = a
        out[k] = a
    return out


_EXACT = {}


def exact_references(name):
    """The quantities of the exact-arithmetic comparison for EXACT_CASES[name], computed once: {quantity: (Q_float, Q_exact)} over the
    interior, Q_float the restatement in doubles (what STRICT must equal bit for bit), Q_exact the same expressions in the 80-digit
    context of tests/fast_math_ref.py.
      visc_v, visc_u                    one viscous sub-step (the first of a sub-cycle: v, then u from the new v), dt = the case's
      G<r>_u, G<r>_v, step<r>_u, _v     one explicit tendency launch and one explicit step of EXACT_DT, r = viscous / evp (stored sigma
                                        and u^n, v^n from seed_sigma)
    Each path steps its own state: what a launch reads of an earlier one is that path's result rounded once to double."""
    if name in _EXACT:
        return _EXACT[name]
    import numpy as np
    import cases
    from fast_math_ref import CTX
    from momentum_ref import Ref
    kw = dict(EXACT_CASES)[name]
    got = {}
    for num in (float, CTX):
        q = {}
        c = cases.make_case(substeps=1, **kw)
        r = Ref(cases.oracle_problem(c), nu=NU, viscous=True, num=num)
        r.time_step_momentum(c["dt"], 1)
        q["visc_v"], q["visc_u"] = r.q["v"].copy(), r.q["u"].copy()
        for rheology in ("viscous", "evp"):
            p = cases.oracle_problem(c)
            if rheology == "evp":
                seed_sigma(p)
            r = Ref(p, nu=NU, viscous=rheology == "viscous", num=num)
            r.compute_tendencies(EXACT_DT)
            q[f"G{rheology}_u"], q[f"G{rheology}_v"] = r.q["Gu"].copy(), r.q["Gv"].copy()
            r.explicit_step(EXACT_DT)
            q[f"step{rheology}_u"], q[f"step{rheology}_v"] = r.q["u"].copy(), r.q["v"].copy()
        got[num] = q
    _EXACT[name] = {k: (got[float][k].astype(np.float64), got[CTX][k]) for k in got[float]}
    return _EXACT[name]
