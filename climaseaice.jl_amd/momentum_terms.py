"""Momentum balance terms, interface stresses and their power of a SeaIceModel, computed on the device (include/csi.h,
csi_momentum_terms_compute / csi_momentum_budget_compute).

term fields       every term of u_velocity_tendency / v_velocity_tendency (src/SeaIceDynamics/momentum_tendencies_kernel_functions.jl:
                  11-74) kept as a force per unit area in N m^-2 at its velocity point: coriolis, top (air-ice), bottom (ocean-ice),
                  internal (the stress divergence with its immersed part) and forcing (model.forcing), each with an _x field at the u
                  points and a _y field at the v points that the model allocates and binds on first use; all filled by ONE launch,
                  nothing is copied or waited for.  The ocean receives -bottom.
interface_stress  the reference's x_momentum_stress / y_momentum_stress (sea_ice_external_stress.jl:33-37, 162-174), the stress without
                  the interpolated concentration and the sign: the same launch with a flag, written into the top / bottom fields
momentum_budget   the power of each term, sum u F_x Az^fc + v F_y Az^cf, in the diagnostics' summation order; residual = their sum, the
                  rate of change of kinetic energy the terms imply (no inertia term: an EVP sub-cycle does not close it per step)

The definitions, the halo elements read and the summation order are stated in include/csi.h; tests/momentum_terms_ref.py restates them
in NumPy.  On a tiled model compute_momentum_terms is rank-local; momentum_budget is COLLECTIVE (every rank calls it between the same
two steps).  For coupling: call after the step, before the ocean reads -bottom.
"""
import math
from dataclasses import dataclass

from . import _lib

MOMENTUM_TERMS = ("coriolis", "top", "bottom", "internal", "forcing")
TERM_FIELD_NAMES = tuple(f"{t}_{c}" for t in MOMENTUM_TERMS for c in ("x", "y"))
_SLOT = {n: _lib.slot_of_display_name(n) for n in TERM_FIELD_NAMES}
_BIT = {t: 1 << k for k, t in enumerate(MOMENTUM_TERMS)}
_GROUPS = {"external": _lib.MBUDGET_EXTERNAL, "body": _lib.MBUDGET_BODY, "internal": _lib.MBUDGET_INTERNAL, "all": _lib.MBUDGET_ALL}
_GROUP_MEMBERS = (("external", ("top", "bottom")), ("body", ("coriolis", "forcing")), ("internal", ("internal",)))


def slot_of(name):
    """The csi_field_bind slot ("M_TOP_X", ...) of a term field's name; ValueError naming the ten for anything else."""
    if name not in _SLOT:
        raise ValueError(f"momentum term field: one of {', '.join(TERM_FIELD_NAMES)} is needed, got {name!r}")
    return _SLOT[name]


def location_of(name):
    """(Face, Center) for an _x field, (Center, Face) for an _y field."""
    return _lib.slot_location(slot_of(name))


def name_of_slot(slot):
    """The term field's name for its slot or for the name itself (a stand-in recorder's slots are names); None for any other slot."""
    if slot in _SLOT:
        return slot
    return next((n for n, s in _SLOT.items() if s == slot), None)


def expand(names):
    """The field names of a sequence of names: a term's name ("top") stands for its two components, x before y."""
    out = []
    for n in names:
        if n in MOMENTUM_TERMS:
            out += [f"{n}_x", f"{n}_y"]
        else:
            slot_of(n)
            out.append(n)
    return out


def mask_of(names):
    """The CSI_MTERM_* mask of a sequence of term or field names (at least one): a bit selects both components."""
    if not names:
        raise ValueError(f"compute_momentum_terms: name at least one of {', '.join(MOMENTUM_TERMS)} (or a component, e.g. 'top_x')")
    mask = 0
    for n in expand(names):
        mask |= _BIT[n[:-2]]
    return mask


def terms_of(mask):
    """The term names of a CSI_MTERM_* mask."""
    return tuple(t for t in MOMENTUM_TERMS if mask & _BIT[t])


def interface_stress(model, side):
    if side not in ("top", "bottom"):
        raise ValueError(f"interface_stress: side must be 'top' or 'bottom', got {side!r}")
    fields = (model.momentum_term(f"{side}_x"), model.momentum_term(f"{side}_y"))
    model.ctx.momentum_terms_compute(_BIT[side] | _lib.MTERM_RAW_STRESS)
    return fields


@dataclass(frozen=True)
class MomentumBudget:
    """The result of model.momentum_budget(): immutable; powers in W.  Members of a group that was not requested are None.
    coriolis, forcing   the "body" group (the Coriolis power vanishes to rounding on a uniform doubly periodic f-plane)
    top, bottom         the "external" group: wind input and ocean drag (bottom <= 0 against an ocean at rest)
    internal            the work of the stress divergence, immersed part included
    residual            the sum of the five: the rate of change of kinetic energy the terms imply; None unless all were requested"""
    what: tuple
    coriolis: float = None
    top: float = None
    bottom: float = None
    internal: float = None
    forcing: float = None
    residual: float = None


def _what_mask(what):
    if isinstance(what, str):
        if what not in _GROUPS:
            raise ValueError(f"momentum_budget: what must be 'all', 'external', 'body' or 'internal' (or a tuple of the last three), got {what!r}")
        return _GROUPS[what]
    mask = 0
    for w in what:
        mask |= _what_mask(w)
    return mask


def momentum_budget(model, what="all"):
    """csi_momentum_budget_compute on the model's context: two launches and a 40-byte copy on the library's stream, which it waits for."""
    mask = _what_mask(what)
    b = model.ctx.momentum_budget_compute(mask)
    kw, groups = {}, []
    for group, members in _GROUP_MEMBERS:
        if mask & _GROUPS[group]:
            groups.append(group)
            kw.update({m: getattr(b, m) for m in members})
    if mask == _lib.MBUDGET_ALL:
        kw["residual"] = math.fsum(kw[t] for t in MOMENTUM_TERMS)
    return MomentumBudget(what=tuple(groups), **kw)
