"""The halo fill kernels as operations (csrc/halo.hip k_fill_halo, k_fill_halo_batch, k_mask, k_copy_batch), BIT FOR BIT against
tests/halo_ref.py (pinned to the C oracle on every cell by tests/test_halo_ref.py): index arithmetic only, nothing has a tolerance.

Parents start with their halos holding distinct finite sentinels.  After a fill
  * INTERIOR and SPECIFIED cells equal the reference;
  * UNTOUCHED and CORNER_UNSPECIFIED cells still hold their sentinels -- the library's rule is "no image, no store" (DESIGN.md).
Matrix: the four locations; (P,P), (P,B), (B,P), (B,B), (P,RightFolded); halos (4,4), (3,5), (5,2); Nx and Ny each from
{H, H+1, 2H-1, 2H, 2H+1} of their own direction plus one size above 64.  On the fold, Ny == Hy leaves a Center-in-y field's row
Ny + Hy without a source among the points: there the library must refuse the fill and leave the parent alone, like any grid narrower
than its halo."""
import ctypes as C

import numpy as np
import pytest
import torch

import climaseaice_jl_amd as csi
import halo_ref as R
import oracle as O

pytestmark = pytest.mark.gpu
L = csi._lib
DEV = "cuda:0"
UNSUPPORTED = -4

TOPOS = {"PP": (L.PERIODIC, L.PERIODIC), "PB": (L.PERIODIC, L.BOUNDED), "BP": (L.BOUNDED, L.PERIODIC), "BB": (L.BOUNDED, L.BOUNDED),
         "PF": (L.PERIODIC, L.RIGHT_FOLDED),
         "CC": (L.FULLY_CONNECTED, L.FULLY_CONNECTED), "PC": (L.PERIODIC, L.FULLY_CONNECTED), "CP": (L.FULLY_CONNECTED, L.PERIODIC),
         "CB": (L.FULLY_CONNECTED, L.BOUNDED), "BC": (L.BOUNDED, L.FULLY_CONNECTED)}
ORA_TOPO = {"P": O.PERIODIC, "B": O.BOUNDED, "F": O.RIGHT_FOLDED}
MATRIX = ["PP", "PB", "BP", "BB", "PF"]
HALOS = [(4, 4), (3, 5), (5, 2)]
VALUES = [(0.375, None), (None, -1.25), (0.375, -1.25)]
CC, FC, CF, FF = (R.CENTER, R.CENTER), (R.FACE, R.CENTER), (R.CENTER, R.FACE), (R.FACE, R.FACE)
# every slot csi_fill_halo_local accepts (csi_field_id and the two prescribed free-drift fields), by location
SLOT_LOC = {n: CC for n in L.FIELD_IDS}
SLOT_LOC.update({n: FC for n in ("U", "UN", "UM", "TOP_U", "BOT_U", "FORCING_U", "GU", "FREE_DRIFT_U")})
SLOT_LOC.update({n: CF for n in ("V", "VN", "VM", "TOP_V", "BOT_V", "FORCING_V", "GV", "FREE_DRIFT_V")})
SLOT_LOC.update({n: FF for n in ("S12", "ZETA_F")})
SLOTS = {loc: [n for n, l in SLOT_LOC.items() if l == loc] for loc in (CC, FC, CF, FF)}


def sizes(H, big):
    return sorted({H, H + 1, 2 * H - 1, 2 * H, 2 * H + 1, big})


def fold_sign(loc):
    return -1 if loc[0] != loc[1] else 1          # the library's rule: (f,c) and (c,f) fields are vector components


class Raw:
    """A context with a grid and slots bound to slices of torch tensors, without a model."""

    def __init__(self):
        self.ctx = L.Context(0)
        self.keep = []

    def grid(self, Nx, Ny, Hx, Hy, topo):
        self.ctx.call("csi_sync")
        met = L.Metrics()
        met.dx = met.dy = 1000.0
        self.ctx.call("csi_grid_set", Nx, Ny, Hx, Hy, TOPOS[topo][0], TOPOS[topo][1], L.METRIC_UNIFORM, C.byref(met))
        for q in ("U", "V"):
            for side in (0, 1):
                self.ctx.call("csi_velocity_bc_set", L.F[q], side, 0, 0.0)
        self.keep = []

    def value_bc(self, vals):
        for q in ("U", "V"):
            for side in (0, 1):
                self.ctx.call("csi_velocity_bc_set", L.F[q], side, 0 if vals[side] is None else 1, 0.0 if vals[side] is None else vals[side])

    def stack(self, parent, names):
        """One device array holding a guard slice, a copy of `parent` per name, and a guard slice; every name bound to its own."""
        t = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(parent, (len(names) + 2,) + parent.shape))).to(DEV)
        nj, ni = parent.shape
        for k, n in enumerate(names):
            self.ctx.call("csi_field_bind", L.F[n], C.c_void_p(t[k + 1].data_ptr()), ni, ni, nj)
        self.keep.append(t)
        return t

    def rc(self, name, *args):
        return getattr(self.ctx.L, name)(self.ctx.h, *args)

    def error(self):
        return self.ctx.L.csi_last_error(self.ctx.h).decode()


@pytest.fixture(scope="module")
def raw():
    r = Raw()
    yield r
    r.ctx.call("csi_sync")
    r.ctx.close()


def seeded(shape, Hx, Hy, seed):
    rng = np.random.default_rng(seed)
    return R.sentinel_parent(shape, Hx, Hy, 0.5 + rng.random((shape[0] - 2 * Hy, shape[1] - 2 * Hx)), seed=seed)


def check(got, before, exp, cls, what):
    """INTERIOR and SPECIFIED cells equal the reference; every other cell still holds what it held."""
    want = np.where((cls == R.INTERIOR) | (cls == R.SPECIFIED), exp, before)
    bad = ~R.same_bits(got, want)
    if bad.any():
        j, i = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {bad.sum()} cells differ, first at array [{j}, {i}] ({R.CLASS_NAMES[int(cls[j, i])]}): "
                             f"{got[j, i]!r}, expected {want[j, i]!r}")


def check_stack(raw, t, names, before, exp, cls, what):
    raw.ctx.call("csi_sync")
    got = t.cpu().numpy()
    assert np.all(R.same_bits(got[0], before)) and np.all(R.same_bits(got[-1], before)), what + ": a store landed outside its parent"
    for k, n in enumerate(names):
        check(got[k + 1], before, exp, cls, f"{n} {what}")


@pytest.mark.parametrize("halo", HALOS, ids=lambda h: f"H{h[0]}x{h[1]}")
@pytest.mark.parametrize("topo", MATRIX)
def test_fill_halo_local_every_slot(raw, topo, halo):
    Hx, Hy = halo
    seed = 0
    for Nx in sizes(Hx, 70):
        for Ny in sizes(Hy, 67):
            raw.grid(Nx, Ny, Hx, Hy, topo)
            what = f"{topo} N=({Nx},{Ny}) H={halo}"
            for loc, names in SLOTS.items():
                seed += 1
                before = seeded(R.parent_shape(Nx, Ny, Hx, Hy, loc, topo), Hx, Hy, seed)
                t = raw.stack(before, names)
                if not R.supported(Nx, Ny, Hx, Hy, loc, topo):
                    assert topo == "PF" and Ny == Hy and loc[1] == R.CENTER          # the only such case of this matrix
                    for n in names:
                        assert raw.rc("csi_fill_halo_local", L.F[n]) == UNSUPPORTED and "tile smaller than its halo" in raw.error()
                    raw.ctx.call("csi_sync")
                    assert np.all(R.same_bits(t.cpu().numpy(), before)), what + ": a refused fill wrote"
                    continue
                exp, cls = R.fill(before, Nx, Ny, Hx, Hy, loc, topo, fold_sign=fold_sign(loc))
                for n in names:
                    raw.ctx.call("csi_fill_halo_local", L.F[n])
                check_stack(raw, t, names, before, exp, cls, what)
                if loc in (FC, CF) and R.supported(Nx, Ny, Hx, Hy, loc, topo):
                    # u, v with ValueBoundaryConditions (u: the y walls, v: the x walls), low and high separately; the other slots of the
                    # location keep the no-flux default
                    q = "U" if loc == FC else "V"
                    for vals in VALUES:
                        raw.value_bc(vals)
                        t = raw.stack(before, names)
                        kw = dict(value_y=vals) if q == "U" else dict(value_x=vals)
                        expv, clsv = R.fill(before, Nx, Ny, Hx, Hy, loc, topo, fold_sign=-1, **kw)
                        for n in names:
                            raw.ctx.call("csi_fill_halo_local", L.F[n])
                        raw.ctx.call("csi_sync")
                        got = t.cpu().numpy()
                        for k, n in enumerate(names):
                            e, c = (expv, clsv) if n == q else (exp, cls)
                            check(got[k + 1], before, e, c, f"{n} {what} values {vals}")
                    raw.value_bc((None, None))


def edge_mask(Nx, Ny, Hx, Hy, topo, seed):
    """(wet interior, mask parent): about a quarter land, with land ON the grid edges so that wrapped and mirrored images of masked
    cells exist; halo entries image their cells (Periodic, fold), as a model's mask does."""
    rng = np.random.default_rng(seed)
    wet = rng.random((Ny, Nx)) > 0.25
    wet[0, 0] = wet[-1, -1] = wet[0, Nx // 2] = wet[Ny // 2, 0] = wet[Ny // 2, -1] = False
    wet[-1, Nx // 2] = False
    if topo[1] == "F":
        wet[-1, :] &= wet[-1, ::-1]
    full = np.zeros((Ny + 2 * Hy, Nx + 2 * Hx), dtype=np.uint8)
    full[Hy:Hy + Ny, Hx:Hx + Nx] = wet
    if topo[0] == "P":
        full[:, :Hx] = full[:, Nx:Nx + Hx]
        full[:, Nx + Hx:] = full[:, Hx:2 * Hx]
    if topo[1] == "P":
        full[:Hy, :] = full[Ny:Ny + Hy, :]
        full[Ny + Hy:, :] = full[Hy:2 * Hy, :]
    if topo[1] == "F":
        full = csi.fold_north(full, Nx, Ny, Hx, Hy, False, False, 1).astype(np.uint8)
    return wet, full


STATE = [("H", "h", CC), ("A", "aice", CC), ("HS", "hs", CC), ("U", "u", FC), ("V", "v", CF)]


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("halo", HALOS, ids=lambda h: f"H{h[0]}x{h[1]}")
@pytest.mark.parametrize("topo", MATRIX)
def test_update_state_fills_and_masks(raw, topo, halo, masked):
    """csi_update_state on h, aice, hs, u, v together (k_mask, k_fill_halo_batch) against ora_update_state from the same parents, exact
    zeros included; the velocities once with the no-flux default and once with ValueBoundaryConditions."""
    Hx, Hy = halo
    seed = 1000
    for Nx in sizes(Hx, 70):
        for Ny in sizes(Hy, 67):
            for vals in ((None, None), (0.375, -1.25)):
                what = f"{topo} N=({Nx},{Ny}) H={halo} values {vals} {'masked' if masked else ''}"
                raw.grid(Nx, Ny, Hx, Hy, topo)
                raw.value_bc(vals)
                p = O.Problem(Nx, Ny, Hx, Hy, (ORA_TOPO[topo[0]], ORA_TOPO[topo[1]]))
                p.s.has_snow = 1
                for side in (0, 1):
                    p.set_value_bc("u", side, vals[side])
                    p.set_value_bc("v", side, vals[side])
                if masked:
                    wet, full = edge_mask(Nx, Ny, Hx, Hy, topo, seed)
                    p.set_mask(full)
                    dm = torch.from_numpy(full).to(DEV)
                    raw.ctx.call("csi_mask_set", C.c_void_p(dm.data_ptr()), full.shape[1])
                before, dev = {}, {}
                for slot, name, loc in STATE:
                    seed += 1
                    before[slot] = seeded(p.f[name].shape, Hx, Hy, seed)
                    p.f[name][...] = before[slot]
                    dev[slot] = raw.stack(before[slot], [slot])
                ok = all(R.supported(Nx, Ny, Hx, Hy, loc, topo) for _, _, loc in STATE)
                if not ok:
                    assert topo == "PF" and Ny == Hy
                    assert raw.rc("csi_update_state") == UNSUPPORTED and "tile smaller than its halo" in raw.error()
                    raw.ctx.call("csi_sync")
                    for slot, _, _ in STATE:
                        assert np.all(R.same_bits(dev[slot].cpu().numpy(), before[slot])), f"{slot} {what}: a refused update_state wrote"
                    continue
                p.update_state()
                raw.ctx.call("csi_update_state")
                raw.ctx.call("csi_sync")
                for slot, name, loc in STATE:
                    kw = dict(value_y=vals) if slot == "U" else (dict(value_x=vals) if slot == "V" else {})
                    exp = p.f[name]
                    # the oracle's result is the reference's fill of the masked points (checked here, on the host) ...
                    masked_in = before[slot].copy()
                    sl = (slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
                    masked_in[sl] = exp[sl]
                    ref, cls = R.fill(masked_in, Nx, Ny, Hx, Hy, loc, topo, fold_sign=fold_sign(loc), **kw)
                    assert np.all(R.same_bits(ref, exp)), f"{slot} {what}: halo_ref and ora_update_state disagree"
                    if masked:
                        assert (exp[sl] == 0.0).any() and not np.signbit(exp[sl][exp[sl] == 0.0]).any()
                    # ... and the library's equals it wherever a cell has a source
                    got = dev[slot].cpu().numpy()
                    assert np.all(R.same_bits(got[0], before[slot])) and np.all(R.same_bits(got[2], before[slot]))
                    check(got[1], masked_in, exp, cls, f"{slot} {what}")
    raw.ctx.call("csi_mask_set", None, 0)


@pytest.mark.parametrize("topo", ["CC", "PC", "CP", "CB", "BC"])
def test_connected_sides_are_left_alone(raw, topo):
    """A context with connected sides and no communicator: csi_fill_halo_local fills the local sides and leaves every cell beyond a
    connected side -- the halo exchange's -- holding its sentinel."""
    seed = 5000
    for Hx, Hy in HALOS:
        for Nx, Ny in ((Hx, 2 * Hy + 1), (2 * Hx - 1, Hy), (2 * Hx + 1, 2 * Hy), (70, Hy + 1), (1, 1) if topo == "CC" else (Hx + 1, 67)):
            raw.grid(Nx, Ny, Hx, Hy, topo)
            for loc, names in SLOTS.items():
                seed += 1
                before = seeded(R.parent_shape(Nx, Ny, Hx, Hy, loc, topo), Hx, Hy, seed)
                exp, cls = R.fill(before, Nx, Ny, Hx, Hy, loc, topo, fold_sign=fold_sign(loc))
                # (halo_ref gives a connected side no image: every cell beyond it is UNTOUCHED or, in the corners, CORNER_UNSPECIFIED)
                if topo[0] == "C":
                    assert not np.any(cls[:, :Hx] == R.SPECIFIED) and not np.any(cls[:, Hx + Nx + R.extra_point(topo[0], loc[0]):] == R.SPECIFIED)
                if topo[1] == "C":
                    assert not np.any(cls[:Hy, :] == R.SPECIFIED) and not np.any(cls[Hy + Ny:, :] == R.SPECIFIED)
                names = names[:2]
                t = raw.stack(before, names)
                for n in names:
                    raw.ctx.call("csi_fill_halo_local", L.F[n])
                check_stack(raw, t, names, before, exp, cls, f"{topo} N=({Nx},{Ny}) H=({Hx},{Hy})")
                if topo == "CC":
                    assert np.all((cls == R.INTERIOR) | (cls == R.UNTOUCHED))


NARROW = [("PP", (3, 9), (4, 4)), ("PP", (9, 3), (4, 4)), ("BB", (2, 11), (3, 5)), ("BB", (7, 4), (3, 5)), ("PB", (4, 9), (5, 2)),
          ("BP", (11, 1), (5, 2)), ("PF", (2, 9), (3, 5)), ("PF", (9, 5), (3, 5)), ("PF", (9, 4), (3, 5))]


@pytest.mark.parametrize("topo,N,halo", NARROW, ids=[f"{t}-{n[0]}x{n[1]}-H{h[0]}x{h[1]}" for t, n, h in NARROW])
def test_narrower_than_the_halo_is_refused(raw, topo, N, halo):
    """N < H in a direction whose sides wrap or mirror: csi_fill_halo_local and csi_update_state return CSI_ERR_UNSUPPORTED and leave the
    parents bit-unchanged.  A field whose sides in that direction have no image (Face on walls) is still filled, at any N >= 1."""
    (Nx, Ny), (Hx, Hy) = N, halo
    raw.grid(Nx, Ny, Hx, Hy, topo)
    refused = 0
    for k, (loc, names) in enumerate(SLOTS.items()):
        before = seeded(R.parent_shape(Nx, Ny, Hx, Hy, loc, topo), Hx, Hy, 7000 + k)
        t = raw.stack(before, names)
        if R.supported(Nx, Ny, Hx, Hy, loc, topo):
            exp, cls = R.fill(before, Nx, Ny, Hx, Hy, loc, topo, fold_sign=fold_sign(loc))
            for n in names:
                raw.ctx.call("csi_fill_halo_local", L.F[n])
            check_stack(raw, t, names, before, exp, cls, f"{topo} N={N} H={halo}")
        else:
            refused += 1
            for n in names:
                assert raw.rc("csi_fill_halo_local", L.F[n]) == UNSUPPORTED and "tile smaller than its halo" in raw.error()
            raw.ctx.call("csi_sync")
            assert np.all(R.same_bits(t.cpu().numpy(), before))
    assert refused >= 1                                 # (h is Center in both directions: always among them)
    # update_state: h, aice and the velocities together -- refused as a whole, before the mask or any fill has written
    wet, full = edge_mask(Nx, Ny, Hx, Hy, topo, 1)
    dm = torch.from_numpy(full).to(DEV)
    raw.ctx.call("csi_mask_set", C.c_void_p(dm.data_ptr()), full.shape[1])
    held = {}
    for k, (slot, _, loc) in enumerate(STATE):
        b = seeded(R.parent_shape(Nx, Ny, Hx, Hy, loc, topo), Hx, Hy, 7100 + k)
        held[slot] = (b, raw.stack(b, [slot]))
    assert raw.rc("csi_update_state") == UNSUPPORTED and "tile smaller than its halo" in raw.error()
    raw.ctx.call("csi_sync")
    for slot, (b, t) in held.items():
        assert np.all(R.same_bits(t.cpu().numpy(), b)), slot
    raw.ctx.call("csi_mask_set", None, 0)


STEP_SLOTS = [("H", CC), ("A", CC), ("U", FC), ("V", CF), ("GH", CC), ("GA", CC), ("HM", CC), ("AM", CC)]
NARROW_STEPS = [("PP", (3, 9), (4, 4)), ("BB", (9, 2), (3, 5)), ("PB", (2, 11), (5, 3))]


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("entry", ["fe", "fe_first", "rk3"])
@pytest.mark.parametrize("topo,N,halo", NARROW_STEPS, ids=[f"{t}-{n[0]}x{n[1]}-H{h[0]}x{h[1]}" for t, n, h in NARROW_STEPS])
def test_whole_steps_on_a_grid_narrower_than_the_halo_are_refused(raw, topo, N, halo, entry, masked):
    """csi_time_step_fe / csi_time_step_rk3 of an advection-only model end by imaging h and aice -- through update_state!, or, without a
    mask, through the tracer update's own stores, which never reach update_state!'s check.  Both must be refused at the ENTRY of the
    step: CSI_ERR_UNSUPPORTED and every bound parent (state, tendencies, Psi^-) bit-unchanged, not an error after a half-advanced step."""
    (Nx, Ny), (Hx, Hy) = N, halo
    raw.grid(Nx, Ny, Hx, Hy, topo)
    if masked:
        wet, full = edge_mask(Nx, Ny, Hx, Hy, topo, 2)
        dm = torch.from_numpy(full).to(DEV)
        raw.ctx.call("csi_mask_set", C.c_void_p(dm.data_ptr()), full.shape[1])
    held = {}
    for k, (slot, loc) in enumerate(STEP_SLOTS):
        b = seeded(R.parent_shape(Nx, Ny, Hx, Hy, loc, topo), Hx, Hy, 7300 + k)
        held[slot] = (b, raw.stack(b, [slot]))
    assert not R.supported(Nx, Ny, Hx, Hy, CC, topo)
    scheme = 5                                          # WENO5: three halo layers, which every halo here has
    if entry == "rk3":
        rc = raw.rc("csi_time_step_rk3", 60.0, 0, scheme)
    else:
        rc = raw.rc("csi_time_step_fe", 60.0, 0, scheme, int(entry == "fe_first"))
    assert rc == UNSUPPORTED and "tile smaller than its halo" in raw.error(), (rc, raw.error())
    raw.ctx.call("csi_sync")
    for slot, (b, t) in held.items():
        assert np.all(R.same_bits(t.cpu().numpy(), b)), f"{slot}: a refused step wrote"
    raw.ctx.call("csi_mask_set", None, 0)


# ---- cache_current_fields! (k_copy_batch): the 16-byte path, the 8-byte path, the odd tail, the grid-stride loop ---------------------
PAIRS = [("H", "HM", CC), ("A", "AM", CC), ("HS", "HSM", CC), ("U", "UM", FC), ("V", "VM", CF)]
GUARD = 4


def _carve(n, offset, fill):
    """A float64 view of n elements starting `offset` elements into an allocation of its own (torch allocations are at least 16-byte
    aligned: offset even -> a 16-byte-aligned address, odd -> 8 bytes beyond one), with guard words on both sides."""
    whole = torch.full((n + 2 * GUARD,), -7.0e7, dtype=torch.float64, device=DEV)
    assert whole.data_ptr() % 16 == 0
    view = whole[offset:offset + n]
    view.copy_(torch.from_numpy(fill))
    return whole, view


@pytest.mark.parametrize("offsets", [(2, 2), (1, 1), (1, 2), (2, 3)], ids=["aligned16", "both+8", "src+8", "dst+8"])
@pytest.mark.parametrize("N", [(5, 5), (6, 5), (5, 6), (1, 1), (1030, 1031)], ids=lambda n: f"{n[0]}x{n[1]}")
def test_cache_current_fields_copies_whole_parents(raw, N, offsets):
    """(Bounded, Bounded) with H = (3, 2): h's parent has (Nx + 6)(Ny + 4) elements, u's one column more, v's one row more -- odd and
    even counts in one batch; 1030 x 1031 is beyond the 2048 blocks x 256 threads x 2 elements of one sweep, so the stride loop runs."""
    (Nx, Ny), (Hx, Hy) = N, (3, 2)
    raw.grid(Nx, Ny, Hx, Hy, "BB")
    rng = np.random.default_rng(Nx + 7 * Ny)
    held = []
    counts = set()
    for src, dst, loc in PAIRS:
        nj, ni = R.parent_shape(Nx, Ny, Hx, Hy, loc, "BB")
        n = nj * ni
        counts.add(n % 2)
        a = rng.standard_normal(n)
        a[:3] = (np.nan, -0.0, np.inf)                      # bits, not values
        ws, vs = _carve(n, offsets[0], a)
        wd, vd = _carve(n, offsets[1], np.full(n, 3.25))
        assert vs.data_ptr() % 16 == (8 if offsets[0] % 2 else 0) and vd.data_ptr() % 16 == (8 if offsets[1] % 2 else 0)
        raw.ctx.call("csi_field_bind", L.F[src], C.c_void_p(vs.data_ptr()), ni, ni, nj)
        raw.ctx.call("csi_field_bind", L.F[dst], C.c_void_p(vd.data_ptr()), ni, ni, nj)
        held.append((src, a, ws, wd, n))
    assert counts == {0, 1}                               # odd and even element counts in one batch
    raw.ctx.call("csi_cache_current_fields")
    raw.ctx.call("csi_sync")
    for src, a, ws, wd, n in held:
        s, d = ws.cpu().numpy(), wd.cpu().numpy()
        o0, o1 = offsets
        assert np.all(R.same_bits(d[o1:o1 + n], a)), f"{src}: the copy differs from the source"
        assert np.all(R.same_bits(s[o0:o0 + n], a)), f"{src}: the source changed"
        for w, o in ((s, o0), (d, o1)):
            assert np.all(w[:o] == -7.0e7) and np.all(w[o + n:] == -7.0e7), f"{src}: a guard word changed"
    for src, dst, _ in PAIRS:
        raw.ctx.call("csi_field_bind", L.F[src], None, 0, 0, 0)
        raw.ctx.call("csi_field_bind", L.F[dst], None, 0, 0, 0)
