"""Per-cell heat fluxes and RadiativeEmission without a GPU: the Python API's checks, the C layout of the new structs, and the
restatement tests/thermo_flux_ref.py against itself."""
import json
import os
import subprocess

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import thermo_flux_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid():
    return csi.RectilinearGrid((4, 3), x=(0, 1), y=(0, 1), halo=(3, 3))


def test_radiative_emission_defaults():
    e = csi.RadiativeEmission()
    assert (e.emissivity, e.stefan_boltzmann_constant, e.reference_temperature) == (1.0, 5.67e-8, 273.15)
    e = csi.RadiativeEmission(emissivity=0.97, stefan_boltzmann_constant=5.6704e-8, reference_temperature=273.16)
    assert (e.emissivity, e.stefan_boltzmann_constant, e.reference_temperature) == (0.97, 5.6704e-8, 273.16)


@pytest.mark.parametrize("kw, err, words", [
    (dict(top_heat_flux=lambda i, j, grid, T, clock, fields: 0.0), NotImplementedError, "FluxFunction"),
    (dict(top_heat_flux=(csi.RadiativeEmission(), np.zeros((3, 4)), np.ones((3, 4)))), NotImplementedError, "at most one array"),
    (dict(bottom_heat_flux=(csi.RadiativeEmission(), 1.0)), NotImplementedError, "top heat flux only"),
    (dict(top_heat_flux=np.zeros((4, 4))), ValueError, "shape"),
    (dict(top_heat_flux=(1.0,) * 9), NotImplementedError, "at most 8 terms"),
    (dict(top_heat_flux="abc"), TypeError, "unsupported"),
])
def test_refusals_by_name(kw, err, words):
    with pytest.raises(err, match=words):
        csi.SeaIceModel(grid(), ice_thermodynamics=csi.SlabThermodynamics(), **kw)


def test_refused_flux_function_object():
    class FluxFunction:
        def __call__(self, *args):
            return 0.0
    with pytest.raises(NotImplementedError, match="FluxFunction"):
        csi.SeaIceModel(grid(), ice_thermodynamics=csi.SlabThermodynamics(), top_heat_flux=(1.0, FluxFunction()))


@pytest.mark.parametrize("side", ["top_heat_flux", "bottom_heat_flux"])
def test_fluxes_in_both_places(side):
    with pytest.raises(ValueError, match="both"):
        csi.SeaIceModel(grid(), ice_thermodynamics=csi.SlabThermodynamics(**{side: 1.0}), **{side: np.zeros((3, 4))})


def test_per_cell_shapes_are_checked():
    with pytest.raises(ValueError, match="PrescribedTemperature"):
        csi.SeaIceModel(grid(), ice_thermodynamics=csi.SlabThermodynamics(top_heat_boundary_condition=csi.PrescribedTemperature(np.zeros(5))))
    with pytest.raises(ValueError, match="snowfall"):
        csi.SeaIceModel(grid(), ice_thermodynamics=csi.SlabThermodynamics(), snow_thermodynamics=csi.snow_slab_thermodynamics(),
                        snowfall=np.zeros((2, 2)))
    assert csi.PrescribedTemperature(-3).temperature == -3.0 and not csi.PrescribedTemperature(-3).per_cell
    assert csi.PrescribedTemperature(np.zeros((3, 4))).per_cell


def test_numeric_slab_params_unchanged():
    """The numbers still travel in csi_slab_params as before; terms leave them at 0."""
    ice = csi.SlabThermodynamics(top_heat_flux=100.0, bottom_heat_flux="frazil")
    p = ice.params(900.0)
    assert (p.top_flux_kind, p.bottom_flux_kind, p.top_heat_flux, p.bottom_heat_flux) == (0, 1, 100.0, 1.0)
    p = csi.SlabThermodynamics().params(900.0)
    assert (p.top_flux_kind, p.bottom_flux_kind, p.top_heat_flux, p.bottom_heat_flux) == (1, 0, 0.0, 0.0)
    p = ice.params(900.0, top_heat_flux=(csi.RadiativeEmission(), 1.0), bottom_heat_flux=np.zeros((3, 4)))
    assert (p.top_flux_kind, p.bottom_flux_kind, p.top_heat_flux, p.bottom_heat_flux) == (0, 0, 0.0, 0.0)


def test_c_layout_of_the_new_structs(tmp_path):
    """sizeof / offsetof of csi_heat_flux_term and csi_surface_solve as gcc lays them out == the ctypes mirrors; the new enums."""
    import ctypes as C
    exe = str(tmp_path / "heat_flux_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "heat_flux_layout.c"), "-o", exe])
    lay = json.loads(subprocess.check_output([exe]).decode())
    for cname, T in (("csi_heat_flux_term", csi._lib.HeatFluxTerm), ("csi_surface_solve", csi._lib.SurfaceSolve)):
        assert C.sizeof(T) == lay[cname]["size"], cname
        assert [f[0] for f in T._fields_] == list(lay[cname]["fields"]), cname
        for n in lay[cname]["fields"]:
            assert getattr(T, n).offset == lay[cname]["fields"][n], (cname, n)
    e = lay["enums"]
    assert (e["CSI_FLUX_CONSTANT"], e["CSI_FLUX_ARRAY"], e["CSI_FLUX_RADIATIVE_EMISSION"]) == (
        csi._lib.FLUX_CONSTANT, csi._lib.FLUX_ARRAY, csi._lib.FLUX_RADIATIVE_EMISSION)
    assert (e["CSI_HEAT_TOP"], e["CSI_HEAT_BOTTOM"], e["CSI_MAX_HEAT_FLUX_TERMS"]) == (csi._lib.HEAT_TOP, csi._lib.HEAT_BOTTOM,
                                                                                       csi._lib.MAX_HEAT_FLUX_TERMS)
    for k in ("TOP_HEAT_FLUX", "BOTTOM_HEAT_FLUX", "SNOWFALL"):
        assert e["CSI_F_" + k] == csi._lib.F[k]
    assert e["CSI_F_COUNT"] == len(csi._lib.FIELD_IDS) and e["CSI_F_TOP_HEAT_FLUX"] == e["CSI_F_COUNT"]
    assert e["CSI_F_COUNT_ALL"] == len(csi._lib.FIELD_IDS) + len(csi._lib.THERMO_FIELD_IDS) and e["CSI_VERSION"] == 100


# ---- the restatement against itself -------------------------------------------------------------------------------------------

def cells(n=4000, seed=1):
    rng = np.random.default_rng(seed)
    h = 0.05 + 3.0 * rng.random(n)
    Tu_prev = -30.0 + 30.0 * rng.random(n)
    q = -300.0 + 500.0 * rng.random(n)
    return h, Tu_prev, q


def test_secant_on_linear_fluxes_is_the_closed_form():
    """With a flux that does not depend on T the secant's root equals the closed form Tb - Qx R within 1e-9 K."""
    h, Tu_prev, q = cells()
    k, Tb = 2.0, -1.62
    f = lambda T: q - (-k * (T - Tb) / h)
    root, iters = R.secant(f, Tu_prev, np.ones(h.shape, bool))
    assert np.abs(root - (Tb - q * h / k)).max() <= 1e-9
    assert iters.max() <= 3


def test_emission_root_balances_the_fluxes():
    """At a converged emission root |Qx - Qi| <= 2 f'(root) tol: the secant's last step is below tol and the error shrinks."""
    h, Tu_prev, q = cells(seed=2)
    k, Tb, tol = 2.0, -1.62, 1e-3
    top = [R.EMISSION, q]
    f = lambda T: R.getflux(top, T) - (-k * (T - Tb) / h)
    root, iters = R.secant(f, Tu_prev, np.ones(h.shape, bool), tol=tol)
    assert iters.max() < 1000
    fprime = 4 * 5.67e-8 * (root + 273.15) ** 3 + k / h
    assert np.all(np.abs(f(root)) <= 2 * fprime * tol)
    # a tighter tolerance moves the root by less than tol
    tight, _ = R.secant(f, Tu_prev, np.ones(h.shape, bool), tol=1e-10)
    assert np.abs(root - tight).max() < tol


def test_cap_at_the_melting_temperature():
    h, Tu_prev, q = cells(seed=3)
    a = np.full_like(h, 0.9)
    for top in ([R.EMISSION, q - 400.0], [q - 400.0]):
        _, _, Tu, _ = R.slab_step(h, a, Tu_prev, 600.0, top, [0.0], ice_salinity=5.0)
        Tm = -0.054 * 5.0
        assert np.all(Tu <= Tm) and (Tu == Tm).any()
    _, _, Tu, _ = R.slab_step(np.full(4, 0.01), np.full(4, 0.5), np.zeros(4), 600.0, [R.EMISSION], [0.0], S=30.0)
    assert np.all(Tu == -0.054 * 30.0)            # unconsolidated: the bottom temperature


def test_three_numbers_sum_right_nested():
    T = np.zeros(3)
    assert np.all(R.getflux([1e16, -1e16, 1.0], T) == 1e16 + (-1e16 + 1.0))
    assert np.all(R.getflux([1e16, -1e16, 1.0], T) == 0.0) and (1e16 + -1e16) + 1.0 == 1.0
    assert np.all(R.getflux([1.0, 1e16, -1e16, 1.0], T) == 1.0 + (1e16 + (-1e16 + 1.0)))
    assert np.all(R.getflux([-0.0], T) == 0.0) and np.signbit(R.getflux([-0.0], T)).all()
