"""The point-wise halves of the tracer kernels (csrc/tracers.hip star_value, finish_values, k_tracer_star_noadv, k_tracer_finish) on edge
values, bit for bit against tests/tracers_ref.py in both modes: the branch table of tests/tracer_cases.py -- base values 1.5, -1.5, +0.0,
-0.0, 5e-324, 1e300, +Inf, -Inf, NaN; aice* ordinary, above 1, +0.0, -0.0, negative, subnormal, NaN; the second half's aice 0.5, +0.0,
-0.0, 5e-324, -0.1, NaN; active and immersed cells; nonnegative 0 and 1; sources 0, 2, -2e-3 -- on a 37 x 5 periodic grid at rest.

With zero velocities every face flux of the first-order upwind stencil is a zero with the sign of the value it carries, and G = -0.0
wherever the four faces of a cell see finite values -- except +0.0 where both the east and the north flux are -0.0 (clean_cells states
the rule; the test asserts it by bits before it compares).  0 * Inf is NaN: a non-finite value makes G of its own cell and of its west
and south neighbours NaN; those cells stay in the comparison, as NaN sets.  Where G = -0.0 the plain first half is
c* = c^- + dt * (-0.0) = c^-, -0.0 included, and the weighted one ((aice^- c^-) + (-0.0)) / (aice^- + dt Ga) with Ga written by hand.  Scheme 0 (k_tracer_star_noadv) runs the same table with G = +0.0.  Under RK3 (from_cache) a second stage runs,
whose stencil reads the source-free copy the first stage left: where a clipped -0.0 must have become +0.0 (Julia's max)."""
import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import tracer_cases as tc
import tracers_ref as tr

pytestmark = pytest.mark.gpu
NEG_ZERO = np.float64(-0.0).view(np.uint64)
DT = tc.BRANCH_DT


def branch_case():
    Nx, Ny = tc.BRANCH_GRID
    c = cases.make_case(Nx=Nx, Ny=Ny, H=4, topo=("periodic", "periodic"), spacing=1000.0, patches=False, noise=0.0, top=None, bottom=None,
                        coriolis=None, u0=0.0, v0=0.0)
    c["mask"] = tc.branch_round(0)[4]
    assert not np.any(c["u"]) and not np.any(c["v"])
    return c


def parent_of(p, interior, fill=True):
    a = np.zeros_like(p.f["h"])
    tr.interior(p, a)[...] = interior
    if fill:
        tr.fill_halo(p, a)
    return a


def tracers_of(p, weighted, c_interior):
    """the six tracers of a model: (nonnegative, source) over tc.BRANCH_TRACERS, all plain or all weighted, all with the same base
    values -- immersed cells keep theirs (update_state! is not called: the halves are)"""
    return [dict(c=parent_of(p, c_interior), weighted=weighted, nonneg=bool(nn), source=float(src), G=None, star=None, free=None)
            for nn, src in tc.BRANCH_TRACERS]


def model_for(c, weighted, mode, stepper):
    specs = [csi.Tracer(f"t{k}", weighting="concentration" if weighted else None, nonnegative=bool(nn), source=src)
             for k, (nn, src) in enumerate(tc.BRANCH_TRACERS)]
    m = csi.SeaIceModel(c["g"], advection=csi.UpwindBiased(order=1), timestepper=stepper, mode=mode, tracers=specs)
    m.set_mask(c["mask"])
    csi.set_(m, h=np.where(c["mask"], 0.3, 0.0), aice=np.where(c["mask"], 0.5, 0.0), u=c["u"], v=c["v"])
    return m, specs


def clean_cells(p, cin, weighted):
    """(clean, minus): interior cells whose four faces see finite stencil values -- the cell itself, its east and its north neighbour
    (u = v = 0: the upwind cell of a face is the one on its high side) --, and among them those where G must be -0.0.  A face's flux is
    dy * 0 * q = +-0.0 with the sign of q (+0.0 where the mask closes it), a difference of two zeros is -0.0 only as (-0.0) - (+0.0), and
    G = -(V^-1 (fx + fy)): +0.0 only where BOTH the east and the north flux are -0.0 (and the west and south ones +0.0), -0.0 elsewhere."""
    with np.errstate(invalid="ignore"):
        q = p.f["aice"] * cin if weighted else cin
    s = p.s
    own, east, north = (slice(s.Hy, s.Hy + s.Ny), slice(s.Hx, s.Hx + s.Nx)), (slice(s.Hy, s.Hy + s.Ny), slice(s.Hx + 1, s.Hx + s.Nx + 1)), \
        (slice(s.Hy + 1, s.Hy + s.Ny + 1), slice(s.Hx, s.Hx + s.Nx))
    fin, neg = np.isfinite(q), np.signbit(q)
    clean = fin[own] & fin[east] & fin[north]
    return clean, clean & ~(neg[east] & neg[north])


def same(got, want, what):
    ok = tr.same_bits(got, want)
    if not ok:
        g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
        bad = np.argwhere((g.view(np.uint64) != w.view(np.uint64)) & ~(np.isnan(g) & np.isnan(w)))
        raise AssertionError((what, len(bad), [(tuple(b), float(g[tuple(b)]), float(w[tuple(b)])) for b in bad[:4]]))


def test_every_combination_is_in_the_table():
    assert len(tc.branch_combinations()) == tc.BRANCH_C_DISTINCT * len(tc.BRANCH_ASTAR) * len(tc.BRANCH_ANOW) * 2 == 864
    assert {(nn, s) for nn, s in tc.BRANCH_TRACERS} == {(nn, s) for nn in (0, 1) for s in (0.0, 2.0, -2e-3)}


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_halves_on_the_branch_table(weighted, mode, oracle_lib):
    """ForwardEuler halves through the ABI: aice^- and Ga written by hand, csi_tracers_tendencies with scheme 1 and with scheme 0, the
    second half's aice written by hand, csi_tracers_update; c over whole parents by bits"""
    assert len(tc.branch_combinations()) == 864
    c = branch_case()
    m, specs = model_for(c, weighted, mode, "ForwardEuler")
    p = cases.oracle_problem(c)
    assert m.ctx.tracers_stats() == (0, 0)
    stencil = point = 0
    clean_seen = 0
    for scheme in (1, 0):
        for r in range(tc.BRANCH_ROUNDS):
            cm, ab, Ga, an, act = tc.branch_round(r)
            assert np.array_equal(act, tr.active(p))
            ts = tracers_of(p, weighted, cm)
            p.f["aice"][...] = parent_of(p, ab)
            p.f["Ga"][...] = parent_of(p, Ga, fill=False)
            m.copy_to_field(m.ice_concentration, p.f["aice"])
            m.copy_to_field(m.timestepper.Gn.aice, p.f["Ga"])
            for t, s in zip(ts, specs):
                m.copy_to_field(m.tracer(s.name), t["c"])
                getattr(m.timestepper.Gn, s.name).data.fill_(-77.0)
            torch.cuda.synchronize()
            m.ctx.tracers_tendencies(scheme, DT, False)
            m.synchronize()
            stencil, point = stencil + (scheme != 0), point + (scheme == 0)
            assert m.ctx.tracers_stats() == (stencil, point)
            got = [getattr(m.timestepper.Gn, s.name).interior_numpy().copy() for s in specs]
            Ga_keep = p.f["Ga"].copy()
            for t, s, g_ in zip(ts, specs, got):
                want = tr.tendency(p, scheme, t["c"], weighted)
                if scheme:
                    clean, minus = clean_cells(p, t["c"], weighted)
                    assert minus.sum() > 60 and np.all(want[minus].view(np.uint64) == NEG_ZERO), (r, s.name)      # G == -0.0, by bits
                    assert np.all(want[clean] == 0.0) and np.all(np.isnan(want[~clean]) | (want[~clean] == 0.0))
                    clean_seen += int(minus.sum())
                else:
                    assert np.all(want.view(np.uint64) == 0)
                same(g_, want, (mode, scheme, r, "G", s.name))
            p.f["Ga"][...] = Ga_keep
            tr.stage_first(p, ts, scheme, DT, G_given=got)
            p.f["aice"][...] = parent_of(p, an)
            m.copy_to_field(m.ice_concentration, p.f["aice"])
            tr.stage_second(p, ts, DT)
            m.ctx.tracers_update(DT)
            m.synchronize()
            point += 1
            assert m.ctx.tracers_stats() == (stencil, point)
            for t, s in zip(ts, specs):
                same(m.tracer(s.name).numpy(), t["c"], (mode, scheme, r, "c", s.name))
                inner = tr.interior(p, t["c"])
                assert np.all(inner[~act] == 0.0) and np.all(inner[~(an > 0)] == 0.0)
    assert clean_seen > 0


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_two_rk3_stages_on_the_branch_table(weighted, mode, oracle_lib):
    """from_cache = 1 through the ABI: csi_cache_current_fields, then two stages.  The second stage's stencil reads the source-free copy
    the first one left (tracers with a source) or the tracer itself, and the product aice * c with the first stage's final aice: a -0.0
    where +0.0 belongs, in either, changes the sign of a zero flux and shows in G and c of the second stage, compared by bits."""
    c = branch_case()
    m, specs = model_for(c, weighted, mode, "SplitRungeKutta3")
    p = cases.oracle_problem(c)
    stencil = point = 0
    signs = set()
    for r in range(tc.BRANCH_ROUNDS):
        cm, ab, Ga, an, act = tc.branch_round(r)
        ts = tracers_of(p, weighted, cm)
        p.f["aice"][...] = parent_of(p, ab)
        m.copy_to_field(m.ice_concentration, p.f["aice"])
        for t, s in zip(ts, specs):
            m.copy_to_field(m.tracer(s.name), t["c"])
        m.ctx.call("csi_cache_current_fields")
        p.f["am"][...] = p.f["aice"]
        base = [t["c"].copy() for t in ts]
        for stage, (dtau, shift) in enumerate(((DT / 2, 0), (DT, 40))):
            _, _, Ga, an, _ = tc.branch_round(r, shift)
            p.f["Ga"][...] = parent_of(p, Ga, fill=False)
            m.copy_to_field(m.timestepper.Gn.aice, p.f["Ga"])
            m.ctx.tracers_tendencies(1, dtau, True)
            m.synchronize()
            stencil += 1
            assert m.ctx.tracers_stats() == (stencil, point)
            got = [getattr(m.timestepper.Gn, s.name).interior_numpy().copy() for s in specs]
            Ga_keep = p.f["Ga"].copy()
            for t, s, g_ in zip(ts, specs, got):
                assert (t["free"] is not None) == (stage == 1 and t["source"] != 0.0)
                cin = t["c"] if t["free"] is None else t["free"]
                want = tr.tendency(p, 1, cin, weighted)
                same(g_, want, (mode, r, stage, "G", s.name))
                signs |= {int(v) for v in np.unique(want[~np.isnan(want)].view(np.uint64))}
            p.f["Ga"][...] = Ga_keep
            tr.stage_first(p, ts, 1, dtau, base=base, a_base=p.f["am"], G_given=got)
            p.f["aice"][...] = parent_of(p, an)
            m.copy_to_field(m.ice_concentration, p.f["aice"])
            tr.stage_second(p, ts, dtau, rk=True)
            m.ctx.tracers_update(dtau)
            m.synchronize()
            point += 1
            assert m.ctx.tracers_stats() == (stencil, point)
            for t, s in zip(ts, specs):
                same(m.tracer(s.name).numpy(), t["c"], (mode, r, stage, "c", s.name))
    assert int(NEG_ZERO) in signs          # (and whatever other zero or value the restatement gives: compared by bits above)
