"""NumPy restatement of the advected tracers (include/csi.h, "advected ice tracers and ice age"): both halves of a stage, and FE / RK3
steps composed from the oracle's verbs.  The tendency G = -horizontal_div_Uc(.) is TAKEN FROM THE ORACLE: the snow thickness is the
reference's one generic third tracer, so hs := c (PLAIN) or hs := aice * c (BY_CONCENTRATION, one rounded product per parent element) over
the whole parent, has_snow = 1, and Ghs is the tendency -- no line of new oracle code.

A tracer here is a dict: c (parent array, the oracle's layout), weighted, nonneg, source and, after a first half, G and star (interiors);
free (a parent array or None): under RK3, for a tracer with a source, the stage before without its source -- what the next stage's
stencil reads.
"""
import ctypes as C

import numpy as np

import oracle as O
from advect_ref import same_bits      # noqa: F401  (bit for bit, signs of zero included, a NaN matching any NaN)


def tracer(p, interior, weighted=False, nonneg=True, source=0.0):
    c = np.zeros_like(p.f["h"])
    s = p.s
    c[s.Hy:s.Hy + s.Ny, s.Hx:s.Hx + s.Nx] = interior
    t = dict(c=c, weighted=bool(weighted), nonneg=bool(nonneg), source=float(source), G=None, star=None, free=None)
    update_state(p, [t])
    return t


def interior(p, a):
    s = p.s
    return a[s.Hy:s.Hy + s.Ny, s.Hx:s.Hx + s.Nx]


def active(p):
    """the interior cells that are not immersed"""
    if not p.s.has_mask:
        return np.ones((p.s.Ny, p.s.Nx), dtype=bool)
    return interior(p, p._mask) != 0


def fill_halo(p, a):
    p.L.ora_fill_halo_center(p.ptr, O.Field(a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[1]))


def update_state(p, tracers):
    """update_state! of the tracers: zero in immersed cells, local halo images, as hs gets them"""
    for t in tracers:
        interior(p, t["c"])[~active(p)] = 0.0
        fill_halo(p, t["c"])


def tendency(p, scheme, c, weighted):
    """G over the interior from the oracle's snow tendency; the problem's own hs, Ghs, Gh, Ga and has_snow are put back."""
    if scheme == 0:
        return np.zeros((p.s.Ny, p.s.Nx))
    keep = {k: p.f[k].copy() for k in ("hs", "Ghs", "Gh", "Ga")}
    snow = p.s.has_snow
    with np.errstate(over="ignore", invalid="ignore"):
        p.f["hs"][...] = p.f["aice"] * c if weighted else c
    p.s.has_snow = 1
    p.compute_tracer_tendencies(scheme)
    G = p.interior("Ghs").copy()
    p.s.has_snow = snow
    for k, v in keep.items():
        p.f[k][...] = v
    return G


def first_half(G, cb, ab, Ga, dt, weighted):
    """c* from interiors: the base c^-, aice^-, the aice tendency as just written; every product and sum rounded on its own"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if not weighted:
            return cb + dt * G
        a_star = ab + dt * Ga
        return np.where(a_star > 0, ((ab * cb) + dt * G) / a_star, 0.0)


def jmax(a, b):
    """Julia's max, as csrc/advect_dev.h jmax states it: NaN where either argument is NaN, otherwise b where a < b and a elsewhere --
    so jmax(0.0, -0.0) is +0.0, where numpy's maximum is free to return either zero"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a < b, b, a))


def second_half(star, a, act, dt, nonneg, source):
    with np.errstate(over="ignore", invalid="ignore"):
        x = jmax(0.0, star) if nonneg else star
        return np.where((a > 0) & act, x + dt * source, 0.0)


def free_half(star, a, act, nonneg):
    """the second half without the source: the field the next RK3 stage's stencil reads"""
    with np.errstate(over="ignore", invalid="ignore"):
        x = jmax(0.0, star) if nonneg else star
        return np.where((a > 0) & act, x, 0.0)


def stage_first(p, tracers, scheme, dtau, base=None, a_base=None, G_given=None):
    """The first half for every tracer.  The oracle's Gh, Ga must have been computed for this stage (p.compute_tracer_tendencies).
    base: the c^- parents (None: the current fields); a_base: the aice^- parent; G_given: interiors to use instead of the oracle's."""
    Ga = p.interior("Ga").copy()
    ab = interior(p, p.f["aice"] if a_base is None else a_base).copy()
    for k, t in enumerate(tracers):
        cin = t["c"] if t["free"] is None else t["free"]
        t["G"] = tendency(p, scheme, cin, t["weighted"]) if G_given is None else G_given[k]
        cb = interior(p, t["c"] if base is None else base[k]).copy()
        t["star"] = first_half(t["G"], cb, ab, Ga, dtau, t["weighted"])


def stage_second(p, tracers, dtau, rk=False):
    """rk: an RK3 stage -- a tracer with a source also leaves its source-free copy for the next stage's stencil"""
    a = p.interior("aice").copy()
    for t in tracers:
        if rk and t["source"] != 0.0:
            t["free"] = np.zeros_like(t["c"]) if t["free"] is None else t["free"]
            interior(p, t["free"])[...] = free_half(t["star"], a, active(p), t["nonneg"])
            fill_halo(p, t["free"])
        interior(p, t["c"])[...] = second_half(t["star"], a, active(p), dtau, t["nonneg"], t["source"])
        fill_halo(p, t["c"])
        t["star"] = None


def zero_tendencies(p):
    for k in ("Gh", "Ga", "Ghs"):
        p.f[k][...] = 0.0


def step_fe(p, tracers, dt, scheme, first_iteration=False, dynamics=False):
    """time_step!(::FESeaIceModel) composed from the oracle's verbs, the tracers' halves where include/csi.h places them"""
    if first_iteration:
        p.update_state()
        update_state(p, tracers)
    p.compute_tracer_tendencies(scheme) if scheme else zero_tendencies(p)
    stage_first(p, tracers, scheme, dt)
    if dynamics:
        p.time_step_momentum(dt)
    p.dynamic_step_tracers(dt, False)
    stage_second(p, tracers, dt)
    p.update_state()


def step_rk3(p, tracers, dt, scheme, dynamics=False):
    """the SplitRungeKutta3 step: cache_current_fields!, then stages of dt / 3, dt / 2, dt, each from Psi^-"""
    for m, k in (("hm", "h"), ("am", "aice"), ("hsm", "hs"), ("um", "u"), ("vm", "v")):
        p.f[m][...] = p.f[k]
    base = [t["c"].copy() for t in tracers]
    for t in tracers:
        t["free"] = None                  # the first stage's stencil reads the tracers themselves
    for beta in (3, 2, 1):
        dtau = dt / beta
        p.compute_tracer_tendencies(scheme) if scheme else zero_tendencies(p)
        stage_first(p, tracers, scheme, dtau, base=base, a_base=p.f["am"])
        if dynamics:
            p.time_step_momentum(dtau, rk_reset=True)
        p.dynamic_step_tracers(dtau, True)
        stage_second(p, tracers, dtau, rk=True)
        p.update_state()
    for t in tracers:
        t["free"] = None
