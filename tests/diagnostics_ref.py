"""NumPy restatement of csi_diagnostics_compute (include/csi.h, "device diagnostics"): the quantities in the DOCUMENTED order of
operations, from the fields' interiors, the metrics and the mask.  Nothing here is taken from the library.

    blocks of 64 x 64 cells; thread (tx, ty) adds rows ty, ty + 4, ..., ty + 60 of column tx from +0.0; the 64 lanes of a wave
    combine over offsets 32, 16, 8, 4, 2, 1 (xor butterfly); the block adds its four waves in wave order -> one record per block,
    r = by * nbx + bx; the finishing block's thread t adds records t, t + 256, ... from +0.0, then the same butterfly and wave order.
    Cells beyond the grid and inactive cells contribute +0.0.
"""
import math

import numpy as np

BX, BY, WAVES, LANES, FIN = 64, 64, 4, 64, 256


def butterfly(x):
    """x[..., 64] -> the value every lane holds after s[lane] = s[lane] + s[lane ^ off], off = 32 .. 1."""
    lane = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ off]
    assert np.all((x == x[..., :1]) | np.isnan(x))
    return x[..., 0]


def wave_order(w):
    """w[..., 4] -> ((w0 + w1) + w2) + w3"""
    s = w[..., 0]
    for k in range(1, WAVES):
        s = s + w[..., k]
    return s


def ordered_sum(terms):
    """Sum of an (Ny, Nx) array of terms (inactive cells already +0.0) in the documented order."""
    ny, nx = terms.shape
    nbx, nby = -(-nx // BX), -(-ny // BY)
    T = np.zeros((nby * BY, nbx * BX))
    T[:ny, :nx] = terms
    T = T.reshape(nby, BY // WAVES, WAVES, nbx, BX)          # [by, r, ty, bx, tx]: row = 64 by + 4 r + ty
    s = np.zeros((nby, WAVES, nbx, BX))
    for r in range(BY // WAVES):
        s = s + T[:, r]
    rec = wave_order(np.moveaxis(butterfly(s), 1, -1)).reshape(-1)      # [by, bx] -> r = by * nbx + bx
    pad = np.zeros(-(-rec.size // FIN) * FIN)
    pad[:rec.size] = rec
    s = np.zeros(FIN)
    for chunk in pad.reshape(-1, FIN):
        s = s + chunk
    return float(wave_order(butterfly(s.reshape(WAVES, LANES))))


def metrics_of(grid):
    """(dx^fc, dy^cf, Az^cc) over i = 1 .. Nx, j = 1 .. Ny as (Ny, Nx) arrays, from grid.metrics() (any of the three kinds)."""
    m = grid.metrics()
    Nx, Ny, Hx, Hy = grid.Nx, grid.Ny, grid.Hx, grid.Hy
    one = np.ones((Ny, Nx))
    if m["kind"] == "uniform":
        return m["dx"] * one, m["dy"] * one, (m["dx"] * m["dy"]) * one
    if m["kind"] == "per_j":
        rows = slice(Hy, Hy + Ny)
        return np.asarray(m["dxc"])[rows, None] * one, m["dy"] * one, np.asarray(m["azc"])[rows, None] * one
    cut = (slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    return m["dxfc"][cut].copy(), m["dycf"][cut].copy(), m["azcc"][cut].copy()


def _count(bad):
    return int(np.count_nonzero(bad))


def velocity_group(u, v, dxfc, dycf):
    """u: (Ny, Nx [+ 1]) interior, v: (Ny [+ 1], Nx) interior (the + 1: the last faces of a Bounded direction)."""
    ny, nx = dxfc.shape
    with np.errstate(all="ignore"):
        inv = (np.abs(u[:ny, :nx]) / dxfc) + (np.abs(v[:ny, :nx]) / dycf)
        inv_max = float(np.fmax.reduce(inv, axis=None, initial=-np.inf))
        out = dict(inv_timescale_max=inv_max,
                   max_abs_u=float(np.fmax.reduce(np.abs(u), axis=None, initial=-np.inf)),
                   max_abs_v=float(np.fmax.reduce(np.abs(v), axis=None, initial=-np.inf)),
                   nonfinite_u=_count(~np.isfinite(u)), nonfinite_v=_count(~np.isfinite(v)),
                   nan_u=_count(np.isnan(u)), nan_v=_count(np.isnan(v)))
        if out["nan_u"] + out["nan_v"] > 0:
            out["advection_timescale"] = math.nan
        else:
            out["advection_timescale"] = float(np.float64(1.0) / np.float64(inv_max))
    return out


def tracer_terms(h, a, hs, az, mask, threshold):
    """The five (Ny, Nx) term arrays, +0.0 at inactive cells; products in the documented order."""
    act = np.ones(h.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    hs_ = np.zeros_like(h) if hs is None else hs
    with np.errstate(all="ignore"):
        return act, dict(ice_volume=np.where(act, (h * a) * az, 0.0), ice_area=np.where(act, a * az, 0.0),
                         ice_extent=np.where(act & (a >= threshold), az, 0.0), snow_volume=np.where(act, (hs_ * a) * az, 0.0),
                         active_area=np.where(act, az, 0.0))


def tracer_group(h, a, hs, az, mask, threshold=0.15):
    act, terms = tracer_terms(h, a, hs, az, mask, threshold)
    out = {k: ordered_sum(t) for k, t in terms.items()}
    hs_ = np.zeros_like(h) if hs is None else hs
    for name, f, arr in (("min_h", np.fmin, h), ("max_h", np.fmax, h), ("min_aice", np.fmin, a), ("max_aice", np.fmax, a),
                         ("max_hs", np.fmax, hs_)):
        out[name] = float(f.reduce(arr[act], axis=None, initial=np.inf if f is np.fmin else -np.inf))
    out.update(nonfinite_h=_count(~np.isfinite(h)), nonfinite_aice=_count(~np.isfinite(a)), nonfinite_hs=_count(~np.isfinite(hs_)),
               active_cells=_count(act))
    if hs is None:
        out.update(snow_volume=None, max_hs=None, nonfinite_hs=None)
    return out


def of_model(model, mask=None, threshold=0.15, what="all"):
    """The restatement on copies of a model's fields (Field.numpy(): a host copy of each parent)."""
    g = model.grid
    model.synchronize()
    dxfc, dycf, az = metrics_of(g)
    out = {}
    if what in ("all", "velocity"):
        out.update(velocity_group(model.velocities.u.interior_numpy(), model.velocities.v.interior_numpy(), dxfc, dycf))
    if what in ("all", "tracers"):
        hs = model.snow_thickness.interior_numpy() if model.snow_thickness is not None else None
        out.update(tracer_group(model.ice_thickness.interior_numpy(), model.ice_concentration.interior_numpy(), hs, az, mask, threshold))
    return out


SUMS = ("ice_volume", "ice_area", "ice_extent", "snow_volume", "active_area")
EXACT = ("inv_timescale_max", "advection_timescale", "max_abs_u", "max_abs_v", "nonfinite_u", "nonfinite_v", "nan_u", "nan_v",
         "min_h", "max_h", "min_aice", "max_aice", "max_hs", "nonfinite_h", "nonfinite_aice", "nonfinite_hs", "active_cells")


def same_bits(a, b):
    """Equal as bit patterns (-0.0 != +0.0; any NaN equals any NaN); None == None; ints compared as ints."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    if isinstance(a, int) and isinstance(b, int):
        return a == b
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def compare(record, want, keys=None):
    """Names whose value in a csi Diagnostics record differs by a bit from the restatement's."""
    bad = []
    for k in keys or want:
        got = record.nonfinite.get(k[10:]) if k.startswith("nonfinite_") else record.nan.get(k[4:]) if k.startswith("nan_") else getattr(record, k)
        if not same_bits(got, want[k]):
            bad.append((k, got, want[k]))
    return bad


def fsum_bound(terms):
    """(exact sum by math.fsum, the order-independent worst-case bound (n - 1) 2^-53 sum |x_i| of recursive summation in any order)."""
    x = np.asarray(terms, dtype=np.float64).ravel()
    return math.fsum(x), (x.size - 1) * 2.0 ** -53 * math.fsum(np.abs(x))
