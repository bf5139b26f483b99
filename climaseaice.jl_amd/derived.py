"""Derived fields and energy budget integrals of a SeaIceModel, computed on the device (include/csi.h, csi_derived_compute /
csi_budget_compute).

derived fields   divergence, shear, deformation (the strain-rate invariants _compute_evp_viscosities! forms and drops,
                 src/Rheologies/elasto_visco_plastic_rheology.jl:247-260), speed, and for an EVP model sigma_I, sigma_II (the stress state
                 relative to the strength P of the last momentum step) and stress_power: (Center, Center) fields the model allocates and
                 binds on first use, all filled by ONE launch; nothing is copied or waited for
energy_budget    the three sums of the reference's test/test_rheology_energy_budget.jl:77-88 -- work of the stress divergence, stress
                 power -- and the kinetic energy, in the diagnostics' summation order

The definitions, the halo elements read and the summation order are stated in include/csi.h; tests/derived_ref.py restates them in NumPy.
On a tiled model compute_derived is rank-local; energy_budget is COLLECTIVE (every rank calls it between the same two steps).
"""
import math
from dataclasses import dataclass

from . import _lib

DERIVED_NAMES = ("divergence", "shear", "deformation", "speed", "sigma_I", "sigma_II", "stress_power")
STRESS_GROUP = ("sigma_I", "sigma_II", "stress_power")
_SLOT = {n: _lib.slot_of_display_name(n) for n in DERIVED_NAMES}
_BIT = {n: 1 << k for k, n in enumerate(DERIVED_NAMES)}
_GROUPS = {"stress": _lib.BUDGET_STRESS, "kinetic": _lib.BUDGET_KINETIC, "all": _lib.BUDGET_ALL}


def slot_of(name):
    """The csi_field_bind slot ("D_SHEAR", ...) of a derived field's name; ValueError naming the seven for anything else."""
    if name not in _SLOT:
        raise ValueError(f"derived field: one of {', '.join(DERIVED_NAMES)} is needed, got {name!r}")
    return _SLOT[name]


def name_of_slot(slot):
    """The derived field's name for its slot or for the name itself (a stand-in recorder's slots are names); None for any other slot."""
    if slot in _SLOT:
        return slot
    return next((n for n, s in _SLOT.items() if s == slot), None)


def mask_of(names):
    """The CSI_DERIVED_* mask of a sequence of names (at least one)."""
    if not names:
        raise ValueError(f"compute_derived: name at least one of {', '.join(DERIVED_NAMES)}")
    mask = 0
    for n in names:
        slot_of(n)
        mask |= _BIT[n]
    return mask


@dataclass(frozen=True)
class EnergyBudget:
    """The result of model.energy_budget(): immutable.  Members of a group that was not requested are None.
    internal_work   sum (u d_j sigma_1j) Az^fc + (v d_j sigma_2j) Az^cf       (W)
    stress_power    sum (sigma11 e11) Az^cc + (sigma22 e22) Az^cc + (2 sigma12 e12) Az^ff      (D)
    imbalance       |W + D| / max(|W|, |D|): rounding level on unmasked grids whose fields vanish at the walls (the reference's adjoint
                    identity, asserted < 1e-10 by its own test); not small next to land.  NaN when W = D = 0.
    kinetic_energy  sum (1/2) m_u u^2 Az^fc + (1/2) m_v v^2 Az^cf"""
    what: tuple
    internal_work: float = None
    stress_power: float = None
    imbalance: float = None
    kinetic_energy: float = None


def imbalance(W, D):
    """relative_imbalance of test/test_rheology_energy_budget.jl:93"""
    big = max(abs(W), abs(D))
    return math.nan if big == 0.0 or math.isnan(big) else abs(W + D) / big


def _what_mask(what):
    if isinstance(what, str):
        if what not in _GROUPS:
            raise ValueError(f"energy_budget: what must be 'all', 'stress' or 'kinetic' (or a tuple of the last two), got {what!r}")
        return _GROUPS[what]
    mask = 0
    for w in what:
        mask |= _what_mask(w)
    return mask


def energy_budget(model, what="all"):
    """csi_budget_compute on the model's context: two launches and a 24-byte copy on the library's stream, which it waits for."""
    mask = _what_mask(what)
    b = model.ctx.budget_compute(mask)
    stress, kin = bool(mask & _lib.BUDGET_STRESS), bool(mask & _lib.BUDGET_KINETIC)
    kw = {}
    if stress:
        kw.update(internal_work=b.internal_work, stress_power=b.stress_power, imbalance=imbalance(b.internal_work, b.stress_power))
    if kin:
        kw.update(kinetic_energy=b.kinetic_energy)
    return EnergyBudget(what=tuple(n for n, on in (("stress", stress), ("kinetic", kin)) if on), **kw)
