"""The tracer kernels (csrc/tracers.hip, csrc/csi_tracers.hip) on the grids of tests/tracer_cases.py: halos that are unequal or odd, grids
between H and 2H + 1 cells wide (a cell has an image on both sides and k_tracer_finish must never take its wide store), the edges of
the 63 x 7 stencil tile and of the 128 x 4 finish block, every alignment class of a pair of c and of the source-free copy, the
("bounded", "periodic") topology and the north fold with Hx != Hy.  tests/test_tracer_cases_table.py proves what the table covers.

STRICT: G and whole parents of c bit for bit (signs of zero included) against tests/tracers_ref.py.  FAST: G within G_TOL
(tests/test_gpu_steps.py), c bit for bit given the device's own G and aice tendency; whole steps within the bounds of
tests/test_gpu_tracers.py.  Beside the matrix: a tracer bound one double behind a 16-byte boundary, G[k] == NULL, the weighted path
pinned bit for bit in FAST to a plain tracer that holds fl(aice * c) and that one to the snow thickness' tendency, layout independence
on the new shapes, and the refusals and host paths nothing reached.  Every test asserts the launch counts before it looks at values."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import climaseaice_jl_amd as csi
import tracer_cases as tc
import tracers_ref as tr
from test_gpu_steps import G_TOL
from test_gpu_tracers import POISON, SPECS8, UNSUPPORTED, G_of, expected_layout, inactive_parent, model_of, ref_of, specs_of, sync_oracle_to_device

pytestmark = pytest.mark.gpu
_L = csi._lib
IDS = [c.id for c in tc.CASES]
SCHEMES6 = ((7, "f64"), (5, "f64"), (3, "f64"), (-5, "f64"), (-3, "f64"), (1, "f64"), (7, "f32"), (5, "f32"), (3, "f32"))


@functools.lru_cache(maxsize=None)
def built(cid):
    """the inputs of a row, built once and shared (nothing writes into them)"""
    return tc.build(tc.BY_ID[cid])


def test_the_table_speaks_of_these_tracers():
    assert tuple(s[3] != 0.0 for s in SPECS8) == tc.SOURCED8


def bits_differ(a, b):
    """where two parents differ by bits (for the message of a failed comparison)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.argwhere((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b)))[:4]


def check_G(mode, got, want, what):
    """STRICT: bit for bit.  FAST: within G_TOL of the restatement's maximum -- and exactly zero where that maximum is zero."""
    assert np.all(np.isfinite(got)), what
    if np.abs(want).max() == 0.0:
        assert np.all(got == 0.0), what
    elif mode == "strict":
        assert tr.same_bits(got, want), (what, np.abs(got - want).max(), bits_differ(got, want))
    else:
        assert np.abs(got - want).max() <= G_TOL * np.abs(want).max(), (what, np.abs(got - want).max() / np.abs(want).max())


# ---- the two halves, stand-alone, on every row ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_halves_on_every_row(cid, oracle_lib):
    """The protocol of test_gpu_tracers.test_halves_against_the_restatement in STRICT and in FAST: three tracers of mixed weighting in
    one launch, the row's scheme and scheme 1, everything no stencil may read poisoned with 1e300"""
    for mode in ("strict", "fast"):
        halves_on_a_row(cid, mode)


def halves_on_a_row(cid, mode):
    case = tc.BY_ID[cid]
    c = built(cid)
    specs = specs_of(3)
    m = model_of(c, specs, mode=mode, stepper="ForwardEuler", scheme=case.scheme)
    p, ts = ref_of(c, specs)
    assert (p.s.Hx, p.s.Hy) == case.halo == (c["g"].Hx, c["g"].Hy)
    assert m.ctx.tracers_stats() == (0, 0) and m.ctx.tracers_last()["tracers_per_thread"] == 0
    bad = inactive_parent(p)
    for t, s in zip(ts, specs):
        t["c"][bad] = POISON
        m.copy_to_field(m.tracer(s.name), t["c"])
    start = {k: p.f[k].copy() for k in ("h", "aice")}
    start_c = [t["c"].copy() for t in ts]
    dt = c["dt"]
    for n, scheme in enumerate(dict.fromkeys((case.scheme, 1))):
        for k in ("h", "aice"):
            p.f[k][...] = start[k]
        m.copy_to_field(m.ice_thickness, start["h"]); m.copy_to_field(m.ice_concentration, start["aice"])
        for t, s, c0 in zip(ts, specs, start_c):
            t["c"][...] = c0
            m.copy_to_field(m.tracer(s.name), c0)
        p.compute_tracer_tendencies(scheme)
        m.ctx.call("csi_compute_tracer_tendencies", scheme)
        m.ctx.tracers_tendencies(scheme, dt, False)
        m.synchronize()
        assert m.ctx.tracers_stats() == (n + 1, n) and m.ctx.tracers_last() == expected_layout(3)
        want = [tr.tendency(p, scheme, t["c"], t["weighted"]) for t in ts]
        got = [G_of(m, s) for s in specs]
        for s, g_, w_ in zip(specs, got, want):
            assert (np.abs(w_).max() > 0) == (case.Nx * case.Ny > 1), (cid, scheme, s.name)
            check_G(mode, g_, w_, (cid, mode, scheme, "G", s.name))
        if mode == "fast":
            sync_oracle_to_device(p, m, ("Gh", "Ga"))
        tr.stage_first(p, ts, scheme, dt, G_given=got)
        p.dynamic_step_tracers(dt, False)
        m.ctx.call("csi_dynamic_step_tracers", dt, 0)
        if mode == "fast":
            sync_oracle_to_device(p, m, ("h", "aice"))
        tr.stage_second(p, ts, dt)
        m.ctx.tracers_update(dt)
        m.synchronize()
        assert m.ctx.tracers_stats() == (n + 1, n + 1)
        for t, s in zip(ts, specs):
            got_c = m.tracer(s.name).numpy()
            assert tr.same_bits(got_c, t["c"]), (cid, mode, scheme, s.name, bits_differ(got_c, t["c"]))      # whole parents: images included
            inner = tr.interior(p, got_c)
            assert np.all(inner[~tr.active(p)] == 0.0) and np.all(inner[p.interior("aice") <= 0] == 0.0)
            assert np.abs(inner).max() < 1e6          # the poison reached nothing


# ---- whole steps on every row ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_whole_steps_on_every_row(cid, oracle_lib):
    """Two SplitRungeKutta3 steps and one ForwardEuler step with five tracers, three of them with a source (from the second stage on
    their stencils read the source-free copy: both forms of the wide store run), against tr.step_rk3 / tr.step_fe -- computed once for
    both modes -- with the bounds of test_gpu_tracers.test_rk3_steps_of_tracers_with_sources_against_the_restatement; STRICT: whole
    parents, on the fold rows those beyond the fold included (tracer 1 is weighted and has a source)"""
    case = tc.BY_ID[cid]
    c = built(cid)
    specs = specs_of(5)
    assert specs[1].weighting == "concentration" and specs[1].source != 0.0
    for stepper, steps in (("SplitRungeKutta3", 2), ("ForwardEuler", 1)):
        p, ts = ref_of(c, specs)
        for n in range(steps):
            tr.step_rk3(p, ts, c["dt"], case.scheme) if stepper == "SplitRungeKutta3" else tr.step_fe(p, ts, c["dt"], case.scheme, n == 0)
        for mode in ("strict", "fast"):
            m = model_of(c, specs, mode=mode, stepper=stepper, scheme=case.scheme)
            for n in range(steps):
                csi.time_step(m, c["dt"])
            m.synchronize()
            stages = 6 if stepper == "SplitRungeKutta3" else 1
            assert m.ctx.tracers_stats() == (stages, stages) and m.ctx.tracers_last() == expected_layout(5)
            for t, s in zip(ts, specs):
                got = m.tracer(s.name).numpy()
                what = (cid, mode, stepper, s.name)
                assert np.all(np.isfinite(got)), what
                check_G(mode, G_of(m, s), t["G"], what)
                if mode == "strict":
                    assert tr.same_bits(got, t["c"]), (what, np.abs(got - t["c"]).max(), bits_differ(got, t["c"]))
                else:
                    assert np.abs(got - t["c"]).max() <= 1e-13 * max(np.abs(t["c"]).max(), 2 * c["dt"] * abs(s.source)), what
                    assert np.array_equal(got == 0.0, t["c"] == 0.0), what


# ---- a tracer bound by hand one double behind a 16-byte boundary; G[k] == NULL ------------------------------------------------------------------
def variant_of(good, **kw):
    t = _L.Tracers.from_buffer_copy(good)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(t, k)[v[0]] = v[1]
        else:
            setattr(t, k, v)
    return t


def offset_parent(m, like):
    """a device array of `like`'s parent shape whose first element lies 8 bytes behind a 16-byte boundary, inside an allocation one
    double longer"""
    nj, ni = like.data.shape
    buf = torch.zeros(nj * ni + 2, dtype=torch.float64, device=m.device)
    first = 1 if buf.data_ptr() % 16 == 0 else 2
    view = buf[first:first + nj * ni].view(nj, ni)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return buf, view


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
def test_a_tracer_bound_one_double_behind_a_boundary(stepper):
    """Even Nx, even Hx: every pair of an ordinary tracer is aligned, every pair of this one is not -- aice is still loaded as a pair and
    c stored cell by cell.  The sourced, weighted tracer 1 and its G are bound by hand; the results equal those of the ordinary binding."""
    Nx, Ny, halo = 40, 28, (4, 4)
    f0 = tc.finish_path(Nx, Ny, *halo, tc.TOPOS["pp"], c_offset_doubles=1, k=1, sourced=True, rk=stepper != "ForwardEuler")
    assert all(p == tc.SCALAR_C for row in f0.paths for p in row) and all(all(r) for r in f0.aice_pair)
    assert tc.path_counts(Nx, Ny, *halo, tc.TOPOS["pp"], k=1, sourced=True, rk=True)[tc.WIDE_C_FREE] > 0
    c = tc.build(tc.Case("offset", Nx, Ny, halo, "pp", 7, 0, True, "offset"))
    specs = specs_of(3)
    out = {}
    for bound in ("ordinary", "by hand"):
        m = model_of(c, specs, mode="fast", stepper=stepper, scheme=7)
        keep = None
        if bound == "by hand":
            cb, cv = offset_parent(m, m.tracer("age"))
            gb, gv = offset_parent(m, m.tracer("age"))
            m.synchronize()
            cv.copy_(m.tracer("age").data)               # the filled parent set_ left
            torch.cuda.synchronize()
            keep = (cb, gb, variant_of(m._tracers_struct, c=(1, cv.data_ptr()), G=(1, gv.data_ptr())))
            m.ctx.tracers_set(keep[2])
        for _ in range(2):
            csi.time_step(m, c["dt"])
        m.synchronize()
        stages = 2 * (1 if stepper == "ForwardEuler" else 3)
        assert m.ctx.tracers_stats() == (stages, stages) and m.ctx.tracers_last() == expected_layout(3)
        age = cv.cpu().numpy() if keep else m.tracer("age").numpy().copy()
        Gage = gv.cpu().numpy()[halo[1]:halo[1] + Ny, halo[0]:halo[0] + Nx] if keep else G_of(m, specs[1])
        out[bound] = dict(plain=m.tracer("plain").numpy().copy(), age=age, signed=m.tracer("signed").numpy().copy(), G=Gage.copy())
        if keep:
            assert np.all(m.tracer("age").interior_numpy() == c["values"][1])          # the model's own array was left alone
    assert np.abs(out["ordinary"]["age"]).max() > 0 and np.abs(out["ordinary"]["G"]).max() > 0
    for k in out["ordinary"]:
        assert tr.same_bits(out["by hand"][k], out["ordinary"][k]), (stepper, k, bits_differ(out["by hand"][k], out["ordinary"][k]))


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
def test_tracers_without_a_tendency_array(stepper):
    """G[k] == NULL (include/csi.h allows it; the Python front end always binds one): c as with G bound, the former G arrays untouched"""
    c = built("tile-63x7-H54-bb-s7")
    specs = specs_of(5)
    out = {}
    for bound in (True, False):
        m = model_of(c, specs, mode="fast", stepper=stepper, scheme=7)
        if not bound:
            for s in specs:
                getattr(m.timestepper.Gn, s.name).data.fill_(-77.0)
            torch.cuda.synchronize()
            t = variant_of(m._tracers_struct)
            for k in range(len(specs)):
                t.G[k] = None
            m.ctx.tracers_set(t)
        for _ in range(2):
            csi.time_step(m, c["dt"])
        m.synchronize()
        stages = 2 * (1 if stepper == "ForwardEuler" else 3)
        assert m.ctx.tracers_stats() == (stages, stages)
        out[bound] = [m.tracer(s.name).numpy().copy() for s in specs]
        G = [getattr(m.timestepper.Gn, s.name).numpy() for s in specs]
        if bound:
            assert all(np.abs(g).max() > 0 for g in G)
        else:
            assert all(np.all(g == -77.0) for g in G)
    for s, a, b in zip(specs, out[True], out[False]):
        assert tr.same_bits(a, b), (stepper, s.name, bits_differ(a, b))


# ---- the weighted path, pinned exactly in both modes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("cid", ["tile-127x22-H44-pp-s-5", "tile-63x7-H54-bb-s7", "narrow_xy-5x9-H44-bp-s7"])
def test_weighted_tendency_is_the_plain_tendency_of_the_rounded_product(cid, mode):
    """include/csi.h: q = aice * c is ONE rounded product per stencil point and a tracer's operations do not depend on its place in the
    group.  So G of a BY_CONCENTRATION tracer equals, bit for bit and in both modes, G of a PLAIN tracer of the same launch whose whole
    parent holds fl(aice * c); and that one equals Ghs of csi_compute_tracer_tendencies with hs bound to the same parent -- the snow path
    of k_tendencies, which tests/test_gpu_advect_faces.py holds face by face.  Six schemes, f32 weights for the three WENO orders."""
    case = tc.BY_ID[cid]
    assert min(case.halo) >= 4
    if cid.startswith("tile-127"):
        case = case._replace(Ny=23)                   # 127 x 23: fewer rows than four tiles, a one-column last block
    c = tc.build(case)
    specs = [csi.Tracer("dyew", weighting="concentration"), csi.Tracer("dyep")]
    m = model_of(c, specs, mode=mode, stepper="ForwardEuler", scheme=7, values=[c["values"][0], c["values"][0]])
    g, dev = c["g"], m.device
    hs, Ghs = csi.CenterField(g, dev, "hs"), csi.CenterField(g, dev, "Ghs")
    torch.cuda.synchronize()
    m._bind("HS", hs); m._bind("GHS", Ghs)
    m.synchronize()
    cw, a = m.tracer("dyew").numpy().copy(), m.ice_concentration.numpy().copy()
    q = a * cw                                        # one rounded product per parent element, halos included
    assert np.abs(q - cw).max() > 0.05
    m.copy_to_field(m.tracer("dyep"), q)
    m.copy_to_field(hs, q)
    dt = c["dt"]
    for n, (scheme, wd) in enumerate(SCHEMES6):
        m.ctx.call("csi_set_weno_weight_dtype", 1 if wd == "f32" else 0)
        for f in (m.timestepper.Gn.dyew, m.timestepper.Gn.dyep, Ghs):
            f.data.fill_(-77.0)
        torch.cuda.synchronize()
        m.ctx.call("csi_compute_tracer_tendencies", scheme)
        m.ctx.tracers_tendencies(scheme, dt, False)
        m.synchronize()
        assert m.ctx.tracers_stats() == (n + 1, 0) and m.ctx.tracers_last() == expected_layout(2)
        Gw, Gp, Gs = G_of(m, specs[0]), G_of(m, specs[1]), Ghs.interior_numpy().copy()
        what = (cid, mode, scheme, wd)
        assert np.all(np.isfinite(Gw)) and np.abs(Gw).max() > 0 and not np.any(Gw == -77.0), what
        assert tr.same_bits(Gw, Gp), (what, "weighted vs plain of the product", np.abs(Gw - Gp).max(), bits_differ(Gw, Gp))
        assert tr.same_bits(Gp, Gs), (what, "plain vs Ghs", np.abs(Gp - Gs).max(), bits_differ(Gp, Gs))


# ---- layout independence on the new shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["tile-63x7-H54-bb-s7", "tile-64x8-H44-pb-s5", "narrow_xy-5x9-H44-bp-s7"])
def test_results_do_not_depend_on_the_layout_on_the_new_shapes(cid, monkeypatch):
    case = tc.BY_ID[cid]
    c = built(cid)
    specs = specs_of(5)

    def run(force):
        if force:
            monkeypatch.setenv("CSI_TRACERS_NTR", str(force))
        else:
            monkeypatch.delenv("CSI_TRACERS_NTR", raising=False)
        m = model_of(c, specs, mode="fast", stepper="SplitRungeKutta3", scheme=case.scheme)
        csi.time_step(m, c["dt"])
        m.synchronize()
        assert m.ctx.tracers_stats() == (3, 3) and m.ctx.tracers_last() == expected_layout(5, force)
        return [(m.tracer(s.name).numpy().copy(), G_of(m, s)) for s in specs]
    free = run(0)
    assert all(np.abs(G).max() > 0 for _, G in free)
    for force in (1, 2, 4):
        for s, (c0, G0), (c1, G1) in zip(specs, free, run(force)):
            assert tr.same_bits(c0, c1) and tr.same_bits(G0, G1), (cid, force, s.name)


# ---- refusals and host paths ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_nothing_reached_by_name():
    from test_gpu_tracers import flow_case
    c = flow_case(37, 29, tc.TOPOS["pp"], 0, land=False)
    dt = c["dt"]
    m = model_of(c, specs_of(2), mode="fast", stepper="SplitRungeKutta3", scheme=7)
    ctx, good = m.ctx, m._tracers_struct
    nj, ni = m.ice_thickness.data.shape
    # from_cache before any csi_cache_current_fields since csi_tracers_set
    with pytest.raises(csi.CsiError, match="from_cache needs csi_cache_current_fields after csi_tracers_set"):
        ctx.tracers_tendencies(7, dt, True)
    # Ga, then aice^-, bound with another leading dimension
    wide = torch.zeros(nj * (ni + 1), dtype=torch.float64, device=m.device)
    torch.cuda.synchronize()
    for slot, own in (("GA", m.timestepper.Gn.aice), ("AM", m.timestepper.Psi_minus.aice)):
        ctx.call("csi_field_bind", _L.slot_id(slot), ctypes.c_void_p(wide.data_ptr()), ni + 1, ni, nj)
        with pytest.raises(csi.CsiError, match="tracers: parent shape mismatch: .* vs h"):
            ctx.tracers_tendencies(7, dt, False)
        m._bind(slot, own)
    # h re-bound with another leading dimension after csi_tracers_set
    ctx.call("csi_field_bind", _L.slot_id("H"), ctypes.c_void_p(wide.data_ptr()), ni + 1, ni, nj)
    for call in (lambda: ctx.tracers_tendencies(7, dt, False), lambda: ctx.tracers_update(dt)):
        with pytest.raises(csi.CsiError, match="the grid or the binding of h changed after csi_tracers_set"):
            call()
    m._bind("H", m.ice_thickness)
    ctx.tracers_tendencies(7, dt, False)          # the same binding again: accepted
    ctx.tracers_update(dt)
    # a new csi_grid_set (the same grid) after csi_tracers_set
    m._configure()
    with pytest.raises(csi.CsiError, match="the grid or the binding of h changed after csi_tracers_set"):
        ctx.tracers_tendencies(7, dt, False)
    ctx.tracers_set(good)
    # a host pointer as c
    host = np.zeros((nj, ni))
    with pytest.raises(csi.CsiError, match="tracer 0: c is not a device array"):
        ctx.tracers_set(variant_of(good, c=(0, host.ctypes.data)))
    with pytest.raises(csi.CsiError, match="tracer 1: G is not a device array"):
        ctx.tracers_set(variant_of(good, G=(1, host.ctypes.data)))
    ctx.tracers_set(good)                          # the refusals changed nothing: the model still steps
    csi.set_(m, h=c["h"], aice=c["a"], u=c["u"], v=c["v"], plain=c["values"][0], age=c["values"][1])
    before = ctx.tracers_stats()
    csi.time_step(m, dt)
    m.synchronize()
    assert ctx.tracers_stats() == (before[0] + 3, before[1] + 3)
    fresh = model_of(c, specs_of(2), mode="fast", stepper="SplitRungeKutta3", scheme=7)
    csi.time_step(fresh, dt)
    fresh.synchronize()
    for name in ("plain", "age"):
        assert tr.same_bits(m.tracer(name).numpy(), fresh.tracer(name).numpy()), name
    # csi_tracers_set(NULL) twice
    ctx.tracers_set(None)
    ctx.tracers_set(None)
    with pytest.raises(csi.CsiError, match="csi_tracers_set has not been called"):
        ctx.tracers_update(dt)
    # a halo too small for the scheme, through csi_tracers_tendencies
    c3 = flow_case(37, 29, tc.TOPOS["pp"], 0, land=False, H=3)
    m3 = model_of(c3, specs_of(2), mode="fast", stepper="ForwardEuler", scheme=5)
    with pytest.raises(csi.CsiError, match="halo too small for the advection scheme"):
        m3.ctx.tracers_tendencies(7, dt, False)
    assert m3.ctx.tracers_stats() == (0, 0)
    m3.ctx.tracers_tendencies(5, dt, False)
    assert m3.ctx.tracers_stats() == (1, 0)
    # a grid narrower than its halo: the second half would store more than one image per side
    g = csi.RectilinearGrid((3, 8), x=(0, 3e3), y=(0, 8e3), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    mn = csi.SeaIceModel(g, advection=csi.WENO(order=7), timestepper="ForwardEuler", mode="fast", tracers=("dye",))
    mn.ctx.tracers_tendencies(0, dt, False)          # (point-wise, no image)
    with pytest.raises(csi.CsiError, match="tile smaller than its halo: local halo fill of") as e:
        mn.ctx.tracers_update(dt)
    assert e.value.code == UNSUPPORTED and mn.ctx.tracers_stats() == (0, 1)


def test_set_again_with_another_count_and_with_sources_on_and_off():
    """csi_tracers_set with n = 2, 8, 1 on ONE context, stepping in between, and sources all zero / one non-zero / all zero (the library's
    source-free copies are allocated, kept and released): every configuration equals a fresh context's result bit for bit, under RK3"""
    c = built("baseline-37x29-H44-pp-s7")
    dt = c["dt"]
    specs8 = specs_of(8)
    m = model_of(c, specs8, mode="fast", stepper="SplitRungeKutta3", scheme=7)
    good = m._tracers_struct
    state = dict(h=c["h"], aice=c["a"], u=c["u"], v=c["v"], **{s.name: c["values"][k] for k, s in enumerate(specs8)})

    def fresh(specs):
        f = model_of(c, specs, mode="fast", stepper="SplitRungeKutta3", scheme=7)
        for _ in range(2):
            csi.time_step(f, dt)
        f.synchronize()
        return [f.tracer(s.name).numpy().copy() for s in specs]

    def again(t, names):
        m.ctx.tracers_set(t)
        csi.set_(m, **state)
        before = m.ctx.tracers_stats()
        for _ in range(2):
            csi.time_step(m, dt)
        m.synchronize()
        assert m.ctx.tracers_stats() == (before[0] + 6, before[1] + 6) and m.ctx.tracers_last() == expected_layout(t.n)
        return [m.tracer(nm).numpy().copy() for nm in names]
    for n in (2, 8, 1):
        names = [s.name for s in specs8[:n]]
        for nm, a, b in zip(names, again(variant_of(good, n=n), names), fresh(specs8[:n])):
            assert tr.same_bits(a, b), ("n", n, nm, bits_differ(a, b))
    for sources in ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (-2e-3, 0.0, 5e-4)):
        t = variant_of(good, n=3)
        for k, v in enumerate(sources):
            t.source[k] = v
        specs = [csi.Tracer(nm, weighting=w, nonnegative=nn, source=v) for (nm, w, nn, _), v in zip(SPECS8[:3], sources)]
        names = [s.name for s in specs]
        for nm, a, b in zip(names, again(t, names), fresh(specs)):
            assert tr.same_bits(a, b), ("sources", sources, nm, bits_differ(a, b))
