"""The advection kernels (csrc/advect.hip) face by face against exact WENO arithmetic, and the tracer update branch by branch.

A comb velocity (tests/advect_ref.py: u = +-1 on the faces of one parity, v = 0, spacing 1) makes every single reconstruction of the
SHIPPED kernels observable as a tendency value without a rounding of its own; eight launches per direction observe every face under
both biases.  Each observed value is compared with the 80-digit evaluation of the same reconstruction under the derived,
condition-scaled bound of advect_ref.py (STRICT: also bit for bit with the oracle, which proves the extraction), in every layout a
launch can take.  The tracer update (k_tracer_step and the STEP tail of k_tendencies) is compared bit for bit with a NumPy restatement
of the reference's statements on cells that enumerate its branches.  Every worst ratio is printed before it is asserted (pytest -s);
profiles/r25_advection_faces.md keeps them."""
import numpy as np
import pytest

import advect_layouts as al
import advect_ref as A
import cases
import climaseaice_jl_amd as csi
import fast_math_ref as R
from test_advect_ref import NX, NY, branch_table, comb_case, fields, lines_of
from test_gpu_advect_layouts import ADVECTION, advection_only_model, force, layout_of
from test_gpu_fast_math import primitives, probe          # noqa: F401  (probe: the fixture)

pytestmark = pytest.mark.gpu

MODES = ("strict", "fast")
SHIFT = 5                   # aice = h rolled by five lines across the comb's direction: another value in every cell, the same stencils


def test_rcp_of_one_is_one(probe):       # noqa: F811
    """G = -(rV (fx + fy)) with V = 1: FAST takes rV = fm::rcp(1.0), which must be 1.0 for the comb to observe a face without rounding"""
    assert primitives(probe, np.array([1.0, 1.0]))[2, 0] == 1.0


# ---- one comb sweep -----------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_of(key, c):
    """the oracle problem of a case, made once; its two mode switches are reset on every hand-out (tests set them through sweep)"""
    if key not in _ORACLE:
        _ORACLE[key] = cases.oracle_problem(c)
    p = _ORACLE[key]
    p.s.weno_weights_f32 = 0
    p.s.has_snow = 0
    return p


def tracer_fields(F, along_y, snow=False):
    out = dict(h=F, aice=np.roll(F, SHIFT, axis=1 if along_y else 0))
    if snow:
        out["hs"] = np.roll(F, 2 * SHIFT + 1, axis=1 if along_y else 0)
    return out


def sweep(m, p, L, state, scheme, mode, tend, what, w32=False, snow=False, poison=None):
    """Both directions x two parities x two sign patterns: every face of every tracer, both biases.  state(along_y) -> {name: interior};
    tend(m) launches the kernels and returns {oracle field name: G interior}.  Asserts the harness checks, prints the worst error / bound
    with the face where it occurs, then asserts that no face is outside its bound; returns that worst ratio and its place."""
    worst, outside = (0.0, None), []
    p.s.weno_weights_f32 = int(w32)
    p.s.has_snow = int(snow)
    for along_y in (False, True):
        fld = state(along_y)
        for k, v in fld.items():
            p.interior(k)[...] = v
        for parity in (0, 1):
            for flip in (False, True):
                u, v, sign = A.comb(L, along_y, parity, flip)
                p.interior("u")[...] = u
                p.interior("v")[...] = v
                p.update_state()
                csi.set_(m, u=u, v=v, **fld)
                if poison is not None:           # land cells hold 1e300: no wet face may read them
                    for f, fid in ((m.ice_thickness, "H"), (m.ice_concentration, "A")):
                        a = f.interior_numpy().copy()
                        a[~poison] = 1e300
                        f.set(a)
                        m.ctx.call("csi_fill_halo_local", csi._lib.F[fid])
                G = tend(m)
                faces = A.faces_of(L, sign, along_y)
                for name, g in G.items():
                    tag = what + (name, "y" if along_y else "x", parity, flip)
                    hi, lo, untouched = A.observed(L, g, faces, along_y)
                    assert np.all(np.isfinite(g)), tag
                    assert np.all(g[untouched] == 0.0), tag + ("a cell without a live face",)
                    assert np.array_equal(hi, lo), tag + ("the two cells of a face are not negated", np.argwhere(hi != lo)[:4])
                    if mode == "strict":
                        fn = p.L.ora_weno_flux_y if along_y else p.L.ora_weno_flux_x
                        fs = p.field_struct(name)
                        want = np.array([s * fn(p.ptr, scheme, fs, i, j) for i, j, s in faces])
                        assert A.same_bits(hi + 0.0, want + 0.0), tag + ("oracle", [f for f, a, b in zip(faces, hi, want) if a != b][:4])
                    val, bnd, _ = A.reference_faces(L, p.f[name], scheme, faces, along_y, w32)
                    assert np.array_equal(hi == 0.0, np.array([x == 0 for x in val])), tag + ("zero set",)
                    ratio, at = R.worst_ratio(hi, val, bnd[mode])
                    if ratio > worst[0]:
                        worst = (ratio, (name, "y" if along_y else "x") + faces[at])
                    if ratio > 1.0:
                        outside.append(tag + (ratio, faces[at], float(hi[at]), float(val[at]), float(bnd[mode][at])))
    print(f"faces {' '.join(str(w) for w in what)}: worst error / bound {worst[0]:.4f} at {worst[1]}")
    assert not outside, outside[:4]
    return worst


def tendencies_of(scheme, snow=False):
    def tend(m):
        m.ctx.call("csi_compute_tracer_tendencies", scheme)
        m.synchronize()
        G = m.timestepper.Gn
        out = {"h": G.h.interior_numpy(), "aice": G.aice.interior_numpy()}
        if snow:
            out["hs"] = G.hs.interior_numpy()
        return out
    return tend


def plain_state(f32=False, snow=False):
    FX, FY, _, _ = fields(f32)
    return lambda along_y: tracer_fields(FY if along_y else FX, along_y, snow)



# ---- plain grids ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("topo", ["pp", "bb", "pb"])
@pytest.mark.parametrize("scheme", A.SCHEMES)
def test_every_face_on_plain_grids(scheme, topo, mode, oracle_lib, monkeypatch):
    """130 x 26 (full tiles, a remainder and a seam for every tile shape), halo 4, h and aice of every input family: every face, both
    biases.  STRICT: bit for bit the oracle and within the STRICT bound of the exact value; FAST: within the FAST bound, same zero set."""
    force(monkeypatch)
    c = comb_case(topo)
    p = oracle_of((topo, False), c)
    m = cases.csi_model(c, mode=mode)
    sweep(m, p, lines_of(c, p), plain_state(), scheme, mode, tendencies_of(scheme), (scheme, topo, mode))
    assert layout_of(m) == (al.expected_layout(NX, NY), 0)


# ---- immersed grids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("topo", ["bb", "pp"])
@pytest.mark.parametrize("scheme", A.SCHEMES)
def test_every_face_next_to_land(scheme, topo, mode, oracle_lib, monkeypatch):
    """Hand-placed land (test_advect_ref.immersed_mask): faces at every distance 1 .. 4 from land on either side, alone and next to a
    wall; closed faces carry exactly 0.  Land cells then hold 1e300 and every wet face must give the same bits."""
    force(monkeypatch)
    c = comb_case(topo, land=True)
    p = oracle_of((topo, True), c)
    L = lines_of(c, p)
    m = cases.csi_model(c, mode=mode)

    def keep(store):
        def tend(m_):
            G = tendencies_of(scheme)(m_)
            store.append({k: v.copy() for k, v in G.items()})
            return G
        return tend
    runs = {False: [], True: []}
    sweep(m, p, L, plain_state(), scheme, mode, keep(runs[False]), (scheme, topo, mode, "land"))
    wet = c["mask"].astype(bool)

    def poisoned(m_):
        G = tendencies_of(scheme)(m_)
        runs[True].append({k: v.copy() for k, v in G.items()})
        return {k: np.where(wet, v, 0.0) for k, v in G.items()}       # (what a land cell itself holds is not a face of the sea)
    sweep(m, p, L, plain_state(), scheme, mode, poisoned, (scheme, topo, mode, "land at 1e300"), poison=wet)
    for a, b in zip(runs[False], runs[True]):
        for k in a:
            assert np.array_equal(a[k][wet], b[k][wet]), (scheme, topo, mode, k, "a wet face moved with the land value")


# ---- every layout a launch can take ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", al.FORCED_SHAPES)
def test_every_face_in_the_two_tracer_shapes(shape, mode, oracle_lib, monkeypatch):
    """Two tracers per thread in tiles of 64 x 8, 63 x 7 and 63 x 11 cells (CSI_ADV_NT = 2, CSI_ADV_SHAPE), all six schemes."""
    force(monkeypatch, nt=2, shape=shape)
    c = comb_case("pb")
    p = oracle_of(("pb", False), c)
    m = cases.csi_model(c, mode=mode)
    for scheme in A.SCHEMES:
        sweep(m, p, lines_of(c, p), plain_state(), scheme, mode, tendencies_of(scheme), (scheme, "shape", al.SHAPES[shape], mode))
        assert layout_of(m) == (al.expected_layout(NX, NY, nt=2, shape=shape), 0)


@pytest.mark.parametrize("mode", MODES)
def test_every_face_in_the_snow_layout(mode, oracle_lib, monkeypatch):
    """Three tracers, one per thread, 64 x 4 tiles: the third tracer's faces through Ghs."""
    force(monkeypatch)
    c = comb_case("pb")
    p = oracle_of(("pb", False), c)
    ice = csi.SlabThermodynamics(top_heat_flux=-80.0, bottom_heat_flux=6.0, bottom_salinity=30.0,
                                 top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    m = cases.csi_model(c, mode=mode, timestepper="SplitRungeKutta3", ice_thermodynamics=ice,
                        snow_thermodynamics=csi.snow_slab_thermodynamics(), snowfall=3e-5)
    try:
        for scheme in A.SCHEMES:
            sweep(m, p, lines_of(c, p), plain_state(snow=True), scheme, mode, tendencies_of(scheme, snow=True),
                          (scheme, "snow", mode), snow=True)
            assert layout_of(m) == (al.expected_layout(NX, NY, has_snow=True), 0)
    finally:
        p.s.has_snow = 0


def settled(F, along_y):
    """a state the tracer update leaves alone (h >= 0, 0 <= aice <= 1, h == 0 <=> aice == 0): the update with a zero tendency applied to
    the family fields"""
    t = tracer_fields(F, along_y)
    z = np.zeros_like(F)
    h, a, _ = A.tracer_update(t["h"], t["aice"], z, z, 0.0)
    h2, a2, _ = A.tracer_update(h, a, z, z, 0.0)
    assert A.same_bits(h, h2) and A.same_bits(a, a2)
    return dict(h=h, aice=a)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", list(al.STAGE_LAYOUTS))
def test_every_face_in_the_stage_launch(layout, mode, oracle_lib, monkeypatch):
    """k_tendencies<..., STEP>: an advection-only RK3 step of length 0 on a state the update leaves alone -- every stage reads that
    state, so the Gh / Ga the last stage stored are its faces; h, aice come back bit for bit."""
    nt, shape = al.STAGE_LAYOUTS[layout]
    force(monkeypatch, nt=nt, shape=shape)
    c = comb_case("pb")
    p = oracle_of(("pb", False), c)
    FX, FY, _, _ = fields()
    states = {False: settled(FX, False), True: settled(FY, True)}
    for scheme in A.SCHEMES:
        m = advection_only_model(c, scheme, mode)

        def tend(m_):
            before = {"h": m_.ice_thickness.numpy().copy(), "aice": m_.ice_concentration.numpy().copy()}
            csi.time_step(m_, 0.0)
            m_.synchronize()
            assert layout_of(m_) == (al.expected_layout(NX, NY, nt=nt, shape=shape), 1)
            assert A.same_bits(m_.ice_thickness.numpy(), before["h"]) and A.same_bits(m_.ice_concentration.numpy(), before["aice"])
            G = m_.timestepper.Gn
            return {"h": G.h.interior_numpy(), "aice": G.aice.interior_numpy()}
        sweep(m, p, lines_of(c, p), lambda along_y: states[along_y], scheme, mode, tend, (scheme, layout, mode, "stage"))


# ---- f32 weights ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scheme", al.WENO)
def test_every_face_with_f32_weights(scheme, mode, oracle_lib, monkeypatch):
    """weight_dtype f32: the float part restated in numpy.float32 (bit for bit the oracle's, test_advect_ref.py), its weights exact
    inputs of the 80-digit combination.  Inputs within |c| <= 1e3 plus the 1e-30 family, whose float squares underflow."""
    force(monkeypatch)
    c = comb_case("pb")
    p = oracle_of(("pb", False), c)
    m = cases.csi_model(c, mode=mode, advection=csi.WENO(order=scheme, weight_dtype="f32"))
    try:
        sweep(m, p, lines_of(c, p), plain_state(f32=True), scheme, mode, tendencies_of(scheme), (scheme, "f32", mode), w32=True)
    finally:
        p.s.weno_weights_f32 = 0


# ---- the tracer update ----------------------------------------------------------------------------------------------------------------
def snow_model(c, mode):
    ice = csi.SlabThermodynamics(top_heat_flux=-80.0, bottom_heat_flux=6.0, bottom_salinity=30.0,
                                 top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    return cases.csi_model(c, mode=mode, timestepper="SplitRungeKutta3", ice_thermodynamics=ice,
                           snow_thermodynamics=csi.snow_slab_thermodynamics(), snowfall=3e-5)


@pytest.mark.parametrize("snow", [False, True])
@pytest.mark.parametrize("from_cache", [0, 1])
def test_tracer_update_branch_table(from_cache, snow, oracle_lib):
    """k_tracer_step on cells that enumerate the branches of _dynamic_step_tracers! / dynamic_step_snow! (h+ < 0, a+ < 0, h+ == 0 with
    a+ > 0 and the reverse, a+ > 1, -0.0, NaN and +-Inf tendencies and states, snow over a <= 0), G^n set through the field interface,
    from the fields and from Psi^-: bit for bit the NumPy restatement (signs of zero included, NaN for NaN), the oracle as a second
    opinion, every branch taken by at least one cell.  (The fused image stores of this kernel need a whole step, in which G^n cannot be
    set: test_step_tail_applies_the_stored_tendencies, in both forms.  Snow never meets them: a model with snow has a thermodynamic
    step, and then the stores do not write the images.)"""
    Nx, Ny = 12, 8
    c = cases.make_case(Nx=Nx, Ny=Ny, H=4, spacing=1.0, substeps=2, patches=False, noise=0.0)
    hn, an, Gh, Ga, sn, Ghs = [r.reshape(Ny, Nx) for r in branch_table(Nx * Ny)]
    m = snow_model(c, "strict") if snow else cases.csi_model(c, mode="strict", timestepper="SplitRungeKutta3")
    base = dict(h=hn, aice=an, **({"hs": sn} if snow else {}))
    csi.set_(m, **base)
    if from_cache:
        m.ctx.call("csi_cache_current_fields")
        m.synchronize()
        csi.set_(m, **{k: np.full_like(v, 123.0) for k, v in base.items()})        # the fields themselves must not be read
    G = m.timestepper.Gn
    G.h.set(Gh); G.aice.set(Ga)
    if snow:
        G.hs.set(Ghs)
    m.ctx.call("csi_dynamic_step_tracers", 1.0, from_cache)
    m.synchronize()
    want = A.tracer_update(hn, an, Gh, Ga, 1.0, *((sn, Ghs) if snow else ()))
    taken = want[-1]
    got = [m.ice_thickness.interior_numpy(), m.ice_concentration.interior_numpy()] + ([m.snow_thickness.interior_numpy()] if snow else [])
    p = cases.oracle_problem(c)
    p.s.has_snow = int(snow)
    names = ("hm", "am", "hsm") if from_cache else ("h", "aice", "hs")
    for name, val in zip(names + ("Gh", "Ga", "Ghs"), (hn, an, sn, Gh, Ga, Ghs)):
        p.interior(name)[...] = val
    p.dynamic_step_tracers(1.0, bool(from_cache))
    for k, (g, w) in enumerate(zip(got, want[:-1])):
        name = ("h", "aice", "hs")[k]
        assert A.same_bits(g, w), (name, from_cache, snow, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:4])
        assert A.same_bits(g, p.interior(name)), (name, "oracle")
    for b in A.BRANCHES:
        if snow or b != "snow over a <= 0":
            assert taken[b].any(), b


def tail_state(FX):
    """base state of the step tests: the family fields (negative values, 1e6, zero rows under nonzero aice and the reverse) with -0.0 in
    the zero rows, one NaN cell (the tendencies around it are NaN) and a run of four cells at 1.26e308, whose first-order upwind
    tendency stays finite through the stages and whose last update overflows to Inf"""
    t = tracer_fields(FX, False)
    h, a = t["h"].copy(), t["aice"].copy()
    h[(h == 0) & (np.arange(h.shape[1])[None, :] % 2 == 0)] = -0.0
    a[(a == 0) & (np.arange(a.shape[1])[None, :] % 3 == 0)] = -0.0
    h[5, 40] = np.nan
    h[5, 88:92] = 1.26e308         # x 1.25, x 1.375 after the first two stages (finite), x 1.469 > DBL_MAX / 1.26e308 after the third
    return h, a


# the three ways a whole step reaches the update: (time stepper, fusion) -> (kernel, base state, stores)
STEPS = {"rk3 one launch per stage": ("SplitRungeKutta3", 2),       # k_tendencies<STEP> from Psi^-, its own image stores
         "rk3 separate kernels": ("SplitRungeKutta3", 0),           # k_tracer_step from Psi^- (from_cache = 1), fused image stores
         "forward euler": ("ForwardEuler", 2)}                      # k_tracer_step in place (from_cache = 0), fused image stores


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("step", list(STEPS))
@pytest.mark.parametrize("layout", list(al.STAGE_LAYOUTS))
def test_step_tail_applies_the_stored_tendencies(layout, step, mode, oracle_lib, monkeypatch):
    """One advection-only step on the comb inputs with dt = 0.75: its output must be the reference's update applied to (the step's base
    state, the Gh / Ga its last tendency launch stored), bit for bit in both modes, whole parents with their halo images.  RK3: the
    base state is Psi^-, the update is the last stage's -- in the one-launch stage (k_tendencies<STEP>) and in the separate kernels
    (k_tracer_step with from_cache = 1 and fused image stores).  ForwardEuler: the base state is the state itself, updated IN PLACE by
    k_tracer_step with from_cache = 0 while it writes the images (csi_time_step_fe: no mask, no thermodynamics).  G^n cannot be set
    for a whole step, so the branches are those the comb inputs produce, pooled over the schemes 7, -5 and 1 (first-order upwind keeps
    1.26e308 finite until the update overflows): every branch of the update but the snow one is taken by at least one cell."""
    nt, shape = al.STAGE_LAYOUTS[layout]
    kind, fusion = STEPS[step]
    rk3 = kind == "SplitRungeKutta3"
    force(monkeypatch, nt=nt, shape=shape)
    c = comb_case("pb")
    p = oracle_of(("pb", False), c)
    L = lines_of(c, p)
    FX, _, _, _ = fields()
    h0, a0 = tail_state(FX)
    u, v, _ = A.comb(L, False, 1, False)
    dt = 0.75
    seen = {b: False for b in A.BRANCHES if b != "snow over a <= 0"}
    for scheme in (7, -5, 1):
        m = csi.SeaIceModel(c["g"], dynamics=None, advection=ADVECTION[scheme], timestepper=kind, mode=mode)
        m.set_fusion(fusion)
        csi.set_(m, h=h0, aice=a0, u=u, v=v)
        csi.time_step(m, dt)
        m.synchronize()
        assert layout_of(m) == (al.expected_layout(NX, NY, nt=nt, shape=shape), 1 if (rk3 and fusion) else 0)
        ts = m.timestepper
        if rk3:
            assert A.same_bits(ts.Psi_minus.h.interior_numpy(), h0) and A.same_bits(ts.Psi_minus.aice.interior_numpy(), a0)
        h1, a1, taken = A.tracer_update(h0, a0, ts.Gn.h.interior_numpy(), ts.Gn.aice.interior_numpy(), dt)
        for name, f, want in (("h", m.ice_thickness, h1), ("aice", m.ice_concentration, a1)):
            assert A.same_bits(f.interior_numpy(), want), (name, scheme, layout, step, mode)
            p.interior(name)[...] = want
        p.update_state()
        for name, f in (("h", m.ice_thickness), ("aice", m.ice_concentration)):
            assert A.same_bits(f.numpy(), p.f[name]), (name, scheme, layout, step, mode, "halo images")
        for b in seen:
            seen[b] |= bool(taken[b].any())
    assert all(seen.values()), seen
