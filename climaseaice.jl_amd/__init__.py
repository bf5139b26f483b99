"""climaseaice.jl_amd -- MI355X-native drop-in for the hot path of CliMA/ClimaSeaIce.jl.

The split-explicit EVP momentum sub-cycle, the WENO advection of h / aice and their launch loop
as hand-written gfx950 HIP kernels behind a C ABI (include/csi.h, libcsi_hip.so), plus this thin
host-side mirror of the reference's `SeaIceModel` / `time_step!` surface.  The directory name
contains a dot, so import it through the repo-root shim: `import climaseaice_jl_amd as csi`.
"""
from . import _lib
from ._lib import Context, CsiError, LocalGroup, plan_exchange, plan_ranges
from .dynamics import (Auxiliaries, BetaPlane, FreeDriftVelocities, PointwiseCoriolis, ElastoViscoPlasticRheology, ExplicitSolver, FPlane, IceStrength,
                       ReplacementPressure, SeaIceMomentumEquation, SemiImplicitStress, SplitExplicitSolver, StressBalanceFreeDrift,
                       ViscousRheology)
from .fields import CenterField, CornerField, Field, XFaceField, YFaceField
from .grids import (Bounded, Center, Face, Flat, FullyConnected, LatitudeLongitudeGrid, LeftConnected,
                    OrthogonalCurvilinearGrid, Periodic, LeftConnectedRightFolded, RightFolded, fold_north,
                    RectilinearGrid, RightConnected, TileGrid, TripolarGrid)
from .diagnostics import Diagnostics, TimeStepWizard, assert_finite, cell_advection_timescale, new_time_step
from .derived import DERIVED_NAMES, EnergyBudget
from .momentum_terms import MOMENTUM_TERMS, TERM_FIELD_NAMES, MomentumBudget
from .output import (AveragedTimeInterval, IterationInterval, OutputWriter, TimeInterval, aligned_time_step, bound_fields,
                     load_output)
from .ocean import SlabOceanMixedLayer
from .time_series import (Clamp, Cyclical, FieldTimeSeries, InMemory, Linear, RegriddedTimeSeries, RegriddedVectorTimeSeries, SourceGrid,
                          fill_missing)
from .model import (FieldBoundaryConditions, FluxBoundaryCondition, ImmersedBoundaryCondition, MeltingConstrainedFluxBalance, ValueBoundaryCondition, PrescribedTemperature, RadiativeEmission, LinearHeatFlux, bulk_sensible_heat_flux, SteppedAlbedo, ShortwaveRadiation, SeaIceModel, SlabThermodynamics, SnowSlabThermodynamics,
                    snow_slab_thermodynamics, UpwindBiased, WENO, set_, time_step, time_step_momentum, compute_momentum_tendencies, update_state,
                    prognostic_state, restore_prognostic_state)
from .enthalpy import ColumnField, ColumnGrid, ColumnTimeSeries, EnthalpyMethodSeaIceModel, MolecularDiffusivity
from .drifters import Drifters, DrifterWriter, load_tracks
from .regions import RegionalDiagnostics, RegionalSeriesWriter, Regions, load_regional_series
from .tracers import IceAge, Tracer

__all__ = [n for n in dir() if not n.startswith("_")]
