"""GPU tests of the u-first order of the two-sub-steps kernel (csrc/evp_fused2.hip, k_pair with AUF = 1).

The launch loop takes the order of a pair from the parity of its first sub-step (csi_launch.hip: ufirst = s % 2 == 0).
csi_time_step_momentum always starts on sub-step 1, so every pair it launches starts on an odd sub-step and runs a v-first (AUF = 0)
instantiation; the u-first half of the instantiations is reached only by a caller of csi_evp_subcycle who passes an even
first_substep -- anybody who cuts a sub-cycle into chunks of odd length.  Everything here therefore goes through

    csi_evp_initialize,  csi_evp_subcycle(dt, n, first) with an EVEN first,  csi_evp_finalize (where diagnostics are compared)

on the case tables of the other GPU tests (which is how the library selects a kernel family), and every test asserts the level the
sub-cycle ran on and its launch count: a silent fall-back to the three kernels fails.

References:
  * the CPU oracle, which takes the same first sub-step (tests 1 and 2; scripts/order_sensitivity.py shows that its two orders are
    3.5 to 10 orders of magnitude further apart than the bounds asserted here -- its table is in profiles/r11_pair_coverage.md --, so an order mix-up
    cannot pass; the one case that is blind to the order is named below);
  * the three-kernel FAST path started on the same even sub-step, bit for bit (tests 3, 5, 6, 7);
  * the same kernels in one uncut call (test 4: chunk invariance, the property an ABI caller relies on).

The tile count is whatever the library chooses (no CSI_PAIR_TILES); every configuration is one the library selects by itself.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
from test_gpu_evp import (CASES, DIAG, EVP_FIELDS, FOLD_BAND_CASES, FUSED_CASES, MASKED, PAIR_CASES, PEER_CASES, THREE_KERNEL_ONLY, cmp_region,
                          fuzz_config, fuzz_unfused, gpu_fields)
from test_gpu_activity import ROWC_CASES, SKIP_CASES, assert_bitwise, parents

pytestmark = pytest.mark.gpu

STATE = ("u", "v", "s11", "s22", "s12")
# The oracle comparisons run every case of PAIR_CASES / the six cases of the odd-start cycle test, and one more: without Coriolis force
# and with a uniform initial velocity the two orders of `ice_strength_nocoriolis` give nearly the same answer (7e-13 of max|u| apart
# after two sub-steps, scripts/order_sensitivity.py), so that case alone could not tell a u-first launch from a v-first one on the
# velocities; the same configuration with seeded velocity noise can.
ORDER_CASES = dict(CASES, ice_strength_nocoriolis_noisy=dict(CASES["ice_strength_nocoriolis"], random_uv=0.05))
ORACLE_CASES = sorted(PAIR_CASES) + ["ice_strength_nocoriolis_noisy"]
CYCLE_CASES = ["periodic_full_ice", "ice_strength_nocoriolis", "latlon_channel", "periodic_patches", "masked_latlon", "curvilinear_bounded",
               "ice_strength_nocoriolis_noisy"]


def subcycle(m, c, n, first):
    m.ctx.call("csi_evp_subcycle", float(c["dt"]), int(n), int(first))


def folded(c):
    return c["topo"][1] == "folded"


def pair_launches(c, n):
    """launches of n sub-steps at level 2: one per pair and one for a trailing sub-step; next to a north fold the band's three per
    sub-step beside them (csi_fold.hip band_launches)"""
    return (n + 1) // 2 + (3 * n if folded(c) else 0)


def assert_pair_path(m, c, n, what=""):
    """the last csi_evp_subcycle of n >= 2 sub-steps ran on the two-sub-steps kernel, in the launches that takes"""
    assert m.ctx.last_path()["level"] == 2, (what, m.ctx.last_path())
    assert m.ctx.last_launches() == (pair_launches(c, n), n), (what, m.ctx.last_launches())


# ---- 1, 2: against the oracle -----------------------------------------------------------------------------------------------------

def assert_close_to_oracle(m, p, what):
    """the bounds of test_fast_two_substeps_from_every_state_of_the_oracle_cycle; returns the relative differences"""
    g = gpu_fields(m)
    vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max(), 1e-30)
    smax = max(np.abs(p.f["s11"]).max(), np.abs(p.f["s22"]).max(), np.abs(p.f["s12"]).max(), 1e-30)
    rel = {}
    for k in ("u", "v"):
        d = np.abs(g[k] - p.f[k]).max()
        print(what, k, "max difference", d, "of", vmax)
        assert np.all(np.isfinite(g[k])) and d <= 1e-13 * vmax, (what, k, d, vmax, np.argwhere(np.abs(g[k] - p.f[k]) > 1e-13 * vmax)[:5])
        assert np.array_equal(g[k] == 0.0, p.f[k] == 0.0), (what, k, "zero set", np.argwhere((g[k] == 0.0) != (p.f[k] == 0.0))[:5])
        rel[k] = d / vmax
    rel["sig"] = 0.0
    for k in ("s11", "s22", "s12"):
        # (owned cells / corners: without finalize_rheology! the oracle's halo layers of sigma are whatever its kernels computed there)
        a, b = EVP_FIELDS[k](m).interior_numpy(), p.interior(k)
        d = np.abs(a - b).max()
        print(what, k, "max difference", d, "of", smax)
        assert np.all(np.isfinite(a)) and d <= 1e-10 * smax, (what, k, d, smax, np.argwhere(np.abs(a - b) > 1e-10 * smax)[:5])
        rel["sig"] = max(rel["sig"], d / smax)
    return rel


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_even_start_two_substeps_vs_oracle(name, oracle_lib):
    """Sub-steps 2 and 3 (u before v, then v before u) in one launch of a u-first instantiation, from the state set! leaves, with the
    oracle's ice strength: u, v within 1e-13 max|u, v| of the oracle's sub-steps 2 and 3, sigma on owned cells within 1e-10 max|sigma|,
    zero-velocity sets identical, everything finite.  (How far away the oracle's own answer for sub-steps 1 and 2 lies, case by case:
    scripts/order_sensitivity.py, tabulated in profiles/r11_pair_coverage.md -- 3e-9 of max|u, v| at the least, on the rigid pack of
    periodic_full_ice, up to 2e-3; ice_strength_nocoriolis alone is blind, see ORDER_CASES.)"""
    c = cases.make_case(substeps=2, **ORDER_CASES[name])
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="fast")
    m.set_fusion(2)
    for k in ("u", "v"):
        assert np.array_equal(EVP_FIELDS[k](m).numpy(), p.f[k]), f"{k} after update_state!"
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    m.copy_to_field(m.dynamics.auxiliaries.fields.P, p.f["P"])
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], 2, 3)
    subcycle(m, c, 2, 2)
    assert_pair_path(m, c, 2, name)
    assert_close_to_oracle(m, p, name)


@pytest.mark.parametrize("name", CYCLE_CASES)
def test_even_start_along_the_oracle_cycle(name, oracle_lib):
    """test_fast_two_substeps_from_every_state_of_the_oracle_cycle on the other parity: the oracle runs sub-step 1, then the pair kernel
    is restarted from the ORACLE's state -- u, v, sigma, P, u^n, v^n, parents with their halos -- at every even s = 2, 4, .. 118 and
    advanced by sub-steps s, s + 1 beside it: 59 comparisons per case on the tight bounds, through the rigid pack of the first two
    cases included.  Along the cycle the oracle's two orders stay at least 1e-8 of max|u, v| and 3e-7 of max|sigma| apart on every
    case but ice_strength_nocoriolis (1e-11 and 2e-9 at the least: one to two orders above the bounds, below the 1e-10 at which a case
    counts as able to tell the orders apart).  Its 59 comparisons check agreement with the oracle at rounding level, hardly the
    order: that is what its noisy variant is in the list for (3e-7 at the least)."""
    c = cases.make_case(substeps=120, **ORDER_CASES[name])
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="fast")
    m.set_fusion(2)
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    m.synchronize()
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], 1, 1)
    worst = {"u": 0.0, "v": 0.0, "sig": 0.0}
    for s in range(2, 120, 2):
        for k in ("u", "v", "s11", "s22", "s12", "P", "un", "vn"):
            EVP_FIELDS[k](m).data.copy_(torch.from_numpy(np.ascontiguousarray(p.f[k])))
        torch.cuda.synchronize()
        p.subcycle(c["dt"], s, s + 1)
        subcycle(m, c, 2, s)
        assert_pair_path(m, c, 2, (name, s))
        rel = assert_close_to_oracle(m, p, f"{name} sub-steps {s}, {s + 1}:")
        worst = {k: max(worst[k], rel[k]) for k in worst}
    print(name, "worst two-sub-step differences along the cycle from even sub-steps (relative):", worst)


# ---- 3: bit for bit against the three-kernel path ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 8, 9])
@pytest.mark.parametrize("name", FUSED_CASES)
def test_even_start_bitwise_equal_three_kernel_path(name, n):
    """test_fused_kernels_bitwise_equal_three_kernel_path with both paths started on sub-step 2.  n = 1: the u-first `single` mode of the
    two-sub-steps kernel where only that kernel takes the configuration (the one-sub-step kernel elsewhere); 3: a pair and a trailing
    u-first single; 8, 9: long enough for the tile-activity test.  Same fields and regions: u, v, s11, s22 on whole parents, s12 too
    without walls and on the interior with them, the diagnostics' interiors after csi_evp_finalize.  The fold cases run the pair
    kernel below the band."""
    c = cases.make_case(substeps=n, **CASES[name])
    walls = "bounded" in c["topo"] or folded(c)
    out, level = {}, {}
    for fusion in (0, 2):
        m = cases.csi_model(c, mode="fast")
        m.set_fusion(fusion)
        m.ctx.call("csi_evp_initialize")
        subcycle(m, c, n, 2)
        level[fusion] = m.ctx.last_path()["level"]
        assert m.ctx.launches_per_substep() == (1 if level[fusion] else 3)
        if fusion == 2:
            launches = m.ctx.last_launches()
        m.ctx.call("csi_evp_finalize")
        m.synchronize()
        out[fusion] = {k: EVP_FIELDS[k](m).numpy().copy() for k in ("u", "v", "s11", "s22") + (() if walls else ("s12",))}
        out[fusion].update({k: (EVP_FIELDS[k](m).numpy().copy(), EVP_FIELDS[k](m).interior_numpy().copy()) for k in DIAG + (("s12",) if walls else ())})
    single = 0 if (name in MASKED or name in THREE_KERNEL_ONLY) else 1      # the one-sub-step kernel takes neither masks nor array-valued forcing
    assert level[0] == 0
    assert level[2] == (2 if ((name in PAIR_CASES or name in THREE_KERNEL_ONLY) and n >= 2) else single), level
    if level[2] == 2:
        assert launches == (pair_launches(c, n), n), launches
    elif level[2] == 1:
        assert launches == (n, n), launches
    for k in out[0]:
        a, b = out[0][k], out[2][k]
        if isinstance(a, tuple):        # (level 2 leaves the diagnostics' halo cells to the second sub-step's range: interiors)
            a, b = (a[1], b[1]) if level[2] == 2 else (a[0], b[0])
        assert np.all(np.isfinite(b)), k
        assert np.array_equal(a, b), (name, n, k, np.abs(a - b).max(), np.argwhere(a != b)[:5])


# ---- 4: chunk invariance -------------------------------------------------------------------------------------------------------------

CHUNK_CASES = ["periodic_patches",                 # plain
               "bounded", "noslip_channel",        # walls
               "latlon_channel", "beta_bounded",   # per-row coefficients
               "masked_channel",                   # immersed mask
               "coupled_channel",                  # array forcing
               "free_drift_omip",                  # free drift
               "user_forcing_latlon", "immersed_flux_bc", "immersed_flux_bc_curvilinear",      # model.forcing arrays, immersed fluxes
               "wind_drag_arrays_coupled",         # wind-drag arrays
               "curvilinear_masked",               # per-point coefficients
               "folded_uniform", "folded_tripolar"]                                            # the north fold


@pytest.mark.parametrize("n,a", [(7, 3), (12, 5), (120, 61)])
@pytest.mark.parametrize("name", CHUNK_CASES)
def test_chunked_subcycle_equals_the_whole_one(name, n, a):
    """csi_evp_subcycle(dt, a, 1) followed by csi_evp_subcycle(dt, n - a, a + 1) is csi_evp_subcycle(dt, n, 1), bit for bit: u, v, sigma
    wherever every path defines them (cmp_region), the diagnostics' interiors after csi_evp_finalize.  a is odd, so the second chunk
    starts on an even sub-step and its pairs run the other order than the uncut call's pairs over the same sub-steps."""
    c = cases.make_case(substeps=n, **CASES[name])
    whole = cases.csi_model(c, mode="fast")
    whole.ctx.call("csi_evp_initialize")
    subcycle(whole, c, n, 1)
    assert_pair_path(whole, c, n, "whole")
    whole.ctx.call("csi_evp_finalize")
    cut = cases.csi_model(c, mode="fast")
    cut.ctx.call("csi_evp_initialize")
    subcycle(cut, c, a, 1)
    assert_pair_path(cut, c, a, "first chunk")
    subcycle(cut, c, n - a, a + 1)
    assert_pair_path(cut, c, n - a, "second chunk")
    cut.ctx.call("csi_evp_finalize")
    whole.synchronize(); cut.synchronize()
    for k in STATE:
        x, y = cmp_region(c, k, EVP_FIELDS[k](whole).numpy()), cmp_region(c, k, EVP_FIELDS[k](cut).numpy())
        assert np.all(np.isfinite(y)), k
        assert np.array_equal(x, y), (name, n, a, k, np.abs(x - y).max(), np.argwhere(x != y)[:5])
    for k in DIAG:
        x, y = EVP_FIELDS[k](whole).interior_numpy(), EVP_FIELDS[k](cut).interior_numpy()
        assert np.array_equal(x, y), (name, n, a, k, np.abs(x - y).max(), np.argwhere(x != y)[:5])


# ---- 5: the peer halo transport --------------------------------------------------------------------------------------------------------

def exchange_forcing_halos(m, c):
    """what csi_time_step_momentum does before its sub-cycle and csi_evp_subcycle leaves to the caller (include/csi.h): the halos of the
    stress arrays beyond connected sides"""
    names = [f"{slot}_{comp}" for slot, on in (("TOP", c.get("field_forcing") or c.get("wind_drag") == "arrays"), ("BOT", c.get("field_forcing")))
             if on for comp in ("U", "V")]
    if names:
        ids = (C.c_int32 * len(names))(*[csi._lib.F[x] for x in names])
        m.ctx.call("csi_halo_exchange", ids, len(names), int(c["H"]))


def two_calls(m, c, n, first):
    """initialize, two csi_evp_subcycle calls of n sub-steps -- the second continues where the first ended --, finalize"""
    m.ctx.call("csi_evp_initialize")
    subcycle(m, c, n, first)
    subcycle(m, c, n, first + n)
    m.ctx.call("csi_evp_finalize")


@pytest.mark.parametrize("n", [2, 7, 12])
@pytest.mark.parametrize("name", sorted(PEER_CASES))
def test_even_start_peer_transport_self_connected_bitwise(name, n):
    """test_peer_halo_transport_self_connected_bitwise from sub-step 2: two calls in a row on one context, the second continuing where
    the first ended (with n = 7 on the odd sub-step 9), so the launch numbers of the flag protocol carry on and both (buffer, order)
    tables of a position are used.  Whole parents of u, v, sigma equal the untiled fusion-2 run for even n, interiors for odd n (the
    trailing launch of the untiled run may be another kernel); interiors, the diagnostics' included, equal the three-kernel run."""
    kw, fc = PEER_CASES[name]
    c = cases.make_case(substeps=n, patches=True, random_uv=0.05, **kw)
    three = cases.csi_model(c, mode="fast")
    three.set_fusion(0)
    ref = cases.csi_model(c, mode="fast")
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, fc))
    exchange_forcing_halos(til, c)
    for m in (three, ref, til):
        two_calls(m, c, n, 2)
    three.synchronize(); ref.synchronize(); til.synchronize()
    path = til.ctx.last_path()
    assert til.ctx.halo_transport() == "peer" and path["exchanges"] == 1, path
    assert_pair_path(til, c, n, "tile")
    assert_pair_path(ref, c, n, "untiled")
    assert three.ctx.last_path()["level"] == 0
    for f in STATE:
        get = (lambda m: EVP_FIELDS[f](m).numpy()) if n % 2 == 0 else (lambda m: EVP_FIELDS[f](m).interior_numpy())
        a, b = get(ref), get(til)
        assert np.array_equal(a, b), (f, "parents incl. halos", np.abs(a - b).max(), np.argwhere(a != b)[:5])
    for f in STATE + DIAG:
        a, b = EVP_FIELDS[f](three).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])


@pytest.mark.parametrize("tier", [1, 2])
@pytest.mark.parametrize("name", ["periodic_xy", "channel_land", "coupled_arrays"])
def test_even_start_peer_protocol_tiers_bitwise(name, tier):
    """the fences of tiers 1 and 2 sit in the u-first instantiations too: 13 sub-steps from sub-step 2, twice, equal the untiled run"""
    kw, fc = PEER_CASES[name]
    n = 13
    c = cases.make_case(substeps=n, patches=True, random_uv=0.05, **kw)
    ref = cases.csi_model(c, mode="fast")
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, fc))
    til.set_peer_tier(tier)
    exchange_forcing_halos(til, c)
    for m in (ref, til):
        two_calls(m, c, n, 2)
    ref.synchronize(); til.synchronize()
    assert til.ctx.halo_transport() == "peer" and til.ctx.peer_tier() == tier
    assert_pair_path(til, c, n, "tile")
    assert_pair_path(ref, c, n, "untiled")
    for f in STATE:
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, tier, np.abs(a - b).max(), np.argwhere(a != b)[:5])


# ---- 6: structure cuts and the fold band ------------------------------------------------------------------------------------------------

def even_start_run(c, n, steps=2, skipping=True, row_constant=True, fusion=2):
    """`steps` times initialize / n sub-steps from sub-step 2 / finalize on one model: (parents, tile activity per step, model)"""
    m = cases.csi_model(c, mode="fast")
    m.set_fusion(fusion)
    m.set_tile_skipping(skipping)
    m.set_row_constant(row_constant)
    acts = []
    for _ in range(steps):
        m.ctx.call("csi_evp_initialize")
        subcycle(m, c, n, 2)
        if fusion:
            assert_pair_path(m, c, n)
        else:
            assert m.ctx.last_path()["level"] == 0
        m.ctx.call("csi_evp_finalize")
        m.synchronize()
        acts.append(m.tile_activity())
    return parents(m), acts, m


def assert_equals_three_kernel_path(c, got, three, what):
    """two synchronised models: u, v, sigma where every path defines them, the diagnostics' interiors"""
    for k in STATE:
        a, b = cmp_region(c, k, EVP_FIELDS[k](three).numpy()), cmp_region(c, k, EVP_FIELDS[k](got).numpy())
        assert np.all(np.isfinite(b)), (what, k)
        assert np.array_equal(a, b), (what, k, np.abs(a - b).max(), np.argwhere(a != b)[:5])
    for k in DIAG:
        a, b = EVP_FIELDS[k](three).interior_numpy(), EVP_FIELDS[k](got).interior_numpy()
        assert np.array_equal(a, b), (what, k, np.abs(a - b).max(), np.argwhere(a != b)[:5])


@pytest.mark.parametrize("name", list(SKIP_CASES))
def test_even_start_skipping_is_bit_identical(name):
    """test_skipping_is_bit_identical from sub-step 2, two sub-cycles in a row (the second launches from the first one's sample): tile
    skipping on = off on every parent cell, = the three-kernel path where every path defines the fields."""
    c = cases.make_case(**SKIP_CASES[name])
    n = c["substeps"]
    assert n >= 8
    on, acts, m = even_start_run(c, n, skipping=True)
    off, acts_off, _ = even_start_run(c, n, skipping=False)
    _, _, m3 = even_start_run(c, n, fusion=0)
    assert_bitwise(on, off, name)
    tiles, live, used = acts[0]
    assert used >= 1 and 0 < live < tiles, (name, acts)           # the first sub-cycle always tests: something was skipped, something ran
    if 10 * live < 9 * tiles:
        assert acts[-1][2] >= 1 and 0 < acts[-1][1] < acts[-1][0], (name, acts)
    assert acts_off[-1][2] == 0
    assert_equals_three_kernel_path(c, m, m3, name)


@pytest.mark.parametrize("name", list(ROWC_CASES))
def test_even_start_row_constant_tiles_are_bit_identical(name):
    """test_row_constant_tiles_are_bit_identical from sub-step 2, two sub-cycles in a row: row-constant rows on = off on every parent
    cell, = the three-kernel path where every path defines the fields; the rows are found (all of them outside a fold band) with the
    cut on and none with it off."""
    c = cases.make_case(**ROWC_CASES[name])
    n = c["substeps"]
    assert n >= 8
    on, _, m = even_start_run(c, n, row_constant=True, skipping=False)
    off, _, m0 = even_start_run(c, n, row_constant=False, skipping=False)
    _, _, m3 = even_start_run(c, n, fusion=0)
    assert_bitwise(on, off, name)
    rows = c["Ny"] + 2 * c["H"] + 1
    assert m.row_constant_rows() >= rows - (2 * c["H"] + 2 if folded(c) else 0)
    assert m0.row_constant_rows() == 0
    assert_equals_three_kernel_path(c, m, m3, name)


@pytest.mark.parametrize("n", [8, 11])
@pytest.mark.parametrize("name", sorted(FOLD_BAND_CASES))
def test_even_start_north_fold_band_bitwise(name, n):
    """test_north_fold_band_bitwise from sub-step 2, two sub-cycles in a row: the pair kernel below the band starts u first, and so do
    the band's own launches beside it; cuts on = cuts off = the three kernels on the whole grid."""
    kw = dict(topo=("periodic", "folded"), patches=True, random_uv=0.04)
    kw.update(FOLD_BAND_CASES[name])
    c = cases.make_case(substeps=n, **kw)
    on, _, m = even_start_run(c, n)
    off, _, _ = even_start_run(c, n, skipping=False, row_constant=False)
    _, _, m3 = even_start_run(c, n, fusion=0)
    assert_bitwise(on, off, name)
    assert_equals_three_kernel_path(c, m, m3, name)


# ---- 7: fuzz -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(24))
def test_even_start_fuzz_bitwise(seed):
    """The generator of test_fused_paths_fuzz_bitwise on seeds of its own (every family of round 3 switched on), first sub-step drawn
    from {2, 4, 6}, 1 .. 12 sub-steps: fusion 2 equals the three kernels bit for bit."""
    kw, _ = fuzz_config(50000 + seed)
    rng = np.random.default_rng(77000 + seed)
    first, n = int(rng.choice([2, 4, 6])), int(rng.integers(1, 13))
    c = cases.make_case(substeps=n, **kw)
    out, lvl = {}, {}
    for fusion in (0, 2):
        m = cases.csi_model(c, mode="fast")
        m.set_fusion(fusion)
        m.ctx.call("csi_evp_initialize")
        subcycle(m, c, n, first)
        lvl[fusion] = m.ctx.last_path()["level"]
        launches = m.ctx.last_launches()
        m.ctx.call("csi_evp_finalize")
        m.synchronize()
        out[fusion] = {k: cmp_region(c, k, EVP_FIELDS[k](m).numpy()).copy() for k in STATE}
        out[fusion]["alpha"] = EVP_FIELDS["alpha"](m).interior_numpy().copy()
    # one sub-step: the two-sub-steps kernel is not used; the one-sub-step kernel takes neither masks nor arrays nor free drift
    pair_only = bool(kw["land"] or kw["field_forcing"] or kw.get("free_drift") or kw.get("user_forcing") or kw.get("immersed_bc")
                     or kw.get("wind_drag") == "arrays" or kw.get("bottom") == "arrays")
    expect = 0 if fuzz_unfused(kw) else (2 if n >= 2 else (0 if pair_only else 1))
    assert lvl[0] == 0 and lvl[2] == expect, (kw, first, n, lvl)
    if expect:
        assert launches == ((n + 1) // 2 if expect == 2 else n, n), (kw, first, n, launches)
    for k in out[0]:
        a, b = out[0][k], out[2][k]
        assert np.all(np.isfinite(b)), (k, kw)
        assert np.array_equal(a, b), (seed, kw, first, n, k, np.abs(a - b).max(), np.argwhere(a != b)[:4])
