"""EnthalpyMethodSeaIceModel: the reference's enthalpy-method column model (src/EnthalpyMethodSeaIceModel.jl) on the device.

ColumnGrid(size, z, topology)          RectilinearGrid(size=Nz, z=..., topology=(Flat, Flat, Bounded)) of the reference's example, or
                                       (Nx, Ny, Nz) independent columns
ColumnField                            a (Nz + 2, Ny, Nx) device array, levels 0 and Nz + 1 the z halos
MolecularDiffusivity(kappa_ice, kappa_water)
ColumnTimeSeries(grid, times, data)    a FieldTimeSeries whose slices are numbers, (Nt,), or (Ny, Nx) planes, (Nt, Ny, Nx)
EnthalpyMethodSeaIceModel(grid, ...)   set / update_state / time_step / time_steps / ice_thickness / last_launch

The semantics -- set! updates neither porosity nor diffusivity, update_state! ignores latent heat, frozen cells take kappa_water, the
boundary values of a step are those of its start time -- are the reference's, stated in include/csi.h ("enthalpy-method column
model").  time_steps(dt, n) is the call the fused kernel exists for: n sub-steps with the columns' state held on chip.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .grids import Bounded, Center, Flat
from .model import FieldBoundaryConditions, FluxBoundaryCondition, ValueBoundaryCondition
from .time_series import FieldTimeSeries, RegriddedTimeSeries

REFERENCE_DENSITY = 999.8       # kg m^-3 (EnthalpyMethodSeaIceModel.jl:38)


class ColumnGrid:
    """ColumnGrid(size, z, topology=(Flat, Flat, Bounded)).  size: Nz (horizontally Flat, one column) or (Nx, Ny, Nz) independent
    columns.  z: (bottom, top) -- faces bottom + k * ((top - bottom) / Nz), the last one `top` itself -- or the Nz + 1 faces."""

    def __init__(self, size, z, topology=(Flat, Flat, Bounded)):
        if np.isscalar(size):
            self.Nx, self.Ny, self.Nz = 1, 1, int(size)
        else:
            if len(size) != 3:
                raise ValueError("ColumnGrid: size is Nz or (Nx, Ny, Nz)")
            self.Nx, self.Ny, self.Nz = (int(s) for s in size)
        if min(self.Nx, self.Ny, self.Nz) < 1:
            raise ValueError("ColumnGrid: Nx, Ny, Nz >= 1")
        topology = tuple(topology)
        if len(topology) != 3 or topology[2] is not Bounded:
            raise NotImplementedError("ColumnGrid: the vertical topology is Bounded (topology=(Flat, Flat, Bounded))")
        self.topology = topology
        z = np.asarray(z, dtype=np.float64)
        if z.shape == (2,) and self.Nz != 1:
            dz = (z[1] - z[0]) / self.Nz
            faces = z[0] + np.arange(self.Nz + 1) * dz
            faces[-1] = z[1]
        else:
            faces = z.copy()
        if faces.shape != (self.Nz + 1,) or not np.all(np.isfinite(faces)) or not np.all(np.diff(faces) > 0):
            raise ValueError("ColumnGrid: z is (bottom, top) or Nz + 1 finite, strictly increasing faces")
        self.z_faces = np.ascontiguousarray(faces)
        self.z_centers = (self.z_faces[:-1] + self.z_faces[1:]) / 2.0

    def interior_size(self, LX=Center, LY=Center):
        """(nx, ny) of a horizontal plane: what a FieldTimeSeries of planes has per slice."""
        return self.Nx, self.Ny

    def minimum_zspacing(self):
        return float(np.min(self.z_faces[1:] - self.z_faces[:-1]))


class ColumnField:
    """A (Nz + 2, Ny, Nx) array in device memory: level k = 1 .. Nz the interior, 0 and Nz + 1 the z halos."""

    def __init__(self, grid, device=None, name=""):
        self.grid, self.name = grid, name
        self.data = torch.zeros((grid.Nz + 2, grid.Ny, grid.Nx), dtype=torch.float64, device=device)

    def parent(self):
        return self.data

    def interior(self):
        return self.data[1:-1]

    def numpy(self):
        return self.data.detach().cpu().numpy()

    def interior_numpy(self):
        return self.interior().detach().cpu().numpy()

    def set(self, value):
        """A number, an array that broadcasts against (Nz, Ny, Nx) -- (Nz,) is a profile for every column --, or a function f(z) of
        the level centres."""
        g = self.grid
        if isinstance(value, FieldTimeSeries):
            raise NotImplementedError(f"set!({self.name or 'field'}): a FieldTimeSeries cannot be set into a field")
        if callable(value):
            value = np.asarray(value(g.z_centers), dtype=np.float64)
        if np.isscalar(value):
            arr = np.full((g.Nz, g.Ny, g.Nx), float(value))
        else:
            arr = np.asarray(value, dtype=np.float64)
            if arr.ndim == 1:
                arr = arr[:, None, None]
            arr = np.array(np.broadcast_to(arr, (g.Nz, g.Ny, g.Nx)))      # (a copy: a broadcast view is read-only)
        self.interior().copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(self.data.device))
        self._settle()
        return self

    def set_parent(self, arr):
        """The whole array, halo levels included."""
        self.data.copy_(torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).to(self.data.device))
        self._settle()
        return self

    def _settle(self):
        # torch wrote on ITS stream, the library works on its own: a library call right after a set must not overtake the copy
        if self.data.is_cuda:
            torch.cuda.current_stream(self.data.device).synchronize()


class MolecularDiffusivity:
    """MolecularDiffusivity(kappa_ice=1e-5, kappa_water=1e-6) (EnthalpyMethodSeaIceModel.jl:204-213); `.kappa` is the model's."""

    def __init__(self, kappa_ice=1e-5, kappa_water=1e-6):
        self.kappa_ice, self.kappa_water = float(kappa_ice), float(kappa_water)
        self.kappa = None


class ColumnTimeSeries(FieldTimeSeries):
    """ColumnTimeSeries(grid, times, data, time_indexing=Linear()): a boundary temperature given at a list of times.  data of shape
    (Nt,): one number per time, for every column; (Nt, Ny, Nx): a plane per time.  All slices live in device memory."""

    def __init__(self, grid, times, data, time_indexing=None, backend=None):
        if not isinstance(grid, ColumnGrid):
            raise TypeError("ColumnTimeSeries: grid is a ColumnGrid")
        self._describe(grid, (Center, Center), times, time_indexing, backend)
        if self.backend.chunk_size is not None:
            raise NotImplementedError("ColumnTimeSeries: InMemory(n), the host-resident backend, is not supported for boundary temperatures; "
                                      "InMemory() keeps every slice on the device")
        arr = np.ascontiguousarray(data, dtype=np.float64)
        nt = self.times.size
        if arr.shape not in ((nt,), (nt, grid.Ny, grid.Nx)):
            raise ValueError(f"ColumnTimeSeries: data of shape (Nt,) = {(nt,)} or (Nt, Ny, Nx) = {(nt, grid.Ny, grid.Nx)} is needed, got {arr.shape}")
        self.data = arr

    @property
    def scalar(self):
        return self.data.ndim == 1


_FORMS = {0: None, _lib.ENTH_PER_STEP: "per_step", _lib.ENTH_ON_CHIP: "on_chip"}


class EnthalpyMethodSeaIceModel:
    """EnthalpyMethodSeaIceModel(grid, closure=MolecularDiffusivity(), ice_heat_capacity=2090 / 999.8, water_heat_capacity=3991 / 999.8,
    fusion_enthalpy=3.3e5 / 999.8, boundary_conditions=dict(T=FieldBoundaryConditions(top=ValueBoundaryCondition(...), bottom=...))).

    A boundary temperature is a number, an (Ny, Nx) array (NumPy or a device tensor, e.g. a plane of a ColumnField), or a
    ColumnTimeSeries; None keeps the default, no flux."""

    def __init__(self, grid, closure=None, ice_heat_capacity=2090.0 / REFERENCE_DENSITY, water_heat_capacity=3991.0 / REFERENCE_DENSITY,
                 fusion_enthalpy=3.3e5 / REFERENCE_DENSITY, boundary_conditions=None, device="cuda:0", stream=None):
        if not isinstance(grid, ColumnGrid):
            raise TypeError("EnthalpyMethodSeaIceModel: grid is a ColumnGrid (the model has no horizontal operator; couple columns "
                            "horizontally is not built)")
        closure = closure if closure is not None else MolecularDiffusivity()
        if not isinstance(closure, MolecularDiffusivity):
            raise NotImplementedError("EnthalpyMethodSeaIceModel: closure is a MolecularDiffusivity")
        sides = self._check_boundary_conditions(grid, boundary_conditions)
        self.grid, self.closure = grid, closure
        self.ice_heat_capacity, self.water_heat_capacity = float(ice_heat_capacity), float(water_heat_capacity)
        self.fusion_enthalpy = float(fusion_enthalpy)
        self.boundary_conditions = boundary_conditions or {}
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("EnthalpyMethodSeaIceModel needs a HIP device (torch 'cuda' device); there is no CPU path")
        self.clock = SimpleNamespace(time=0.0, iteration=0)
        self.ctx = _lib.Context(self.device.index or 0, stream)
        mk = lambda name: ColumnField(grid, self.device, name)      # noqa: E731
        self.state = SimpleNamespace(T=mk("T"), H=mk("H"), phi=mk("phi"))
        closure.kappa = mk("kappa")
        self.tendencies = None          # G.H lives in registers: the step kernel never writes it to memory
        torch.cuda.synchronize(self.device)
        p = _lib.EnthalpyParams(grid.Nx, grid.Ny, grid.Nz, 0, grid.z_faces.ctypes.data_as(C.POINTER(C.c_double)), self.ice_heat_capacity,
                                self.water_heat_capacity, self.fusion_enthalpy, closure.kappa_ice, closure.kappa_water)
        self.h = C.c_void_p()
        self._call("csi_enthalpy_create", self.ctx.h, C.byref(p), C.byref(self.h), on_model=False)
        for which, f in ((_lib.ENTH_H, self.state.H), (_lib.ENTH_T, self.state.T), (_lib.ENTH_PHI, self.state.phi),
                         (_lib.ENTH_KAPPA, closure.kappa)):
            self._call("csi_enthalpy_bind", which, C.c_void_p(f.data.data_ptr()))
        self._keep = []
        for side, value in sides:
            self._set_boundary(side, value)
        torch.cuda.synchronize(self.device)

    # ---- argument checks: before a device is touched -------------------------------------------------------------------------------
    @staticmethod
    def _check_boundary_conditions(grid, bcs):
        bcs = bcs or {}
        unknown = set(bcs) - {"T", "H", "phi"}
        if unknown:
            raise ValueError(f"EnthalpyMethodSeaIceModel: boundary_conditions for unknown fields {sorted(unknown)}")
        for name in ("H", "phi"):
            f = bcs.get(name)
            if f is not None and any(getattr(f, s, None) is not None for s in ("top", "bottom")):
                raise NotImplementedError(f"EnthalpyMethodSeaIceModel: a boundary condition on {name} is not supported; give value conditions on T")
        out = []
        f = bcs.get("T")
        if f is not None and not isinstance(f, FieldBoundaryConditions):
            raise TypeError("EnthalpyMethodSeaIceModel: boundary_conditions['T'] is a FieldBoundaryConditions(top=, bottom=)")
        for side, name in ((_lib.ENTH_T_BOTTOM, "bottom"), (_lib.ENTH_T_TOP, "top")):
            bc = getattr(f, name, None) if f is not None else None
            if bc is None:
                out.append((side, None))
                continue
            if isinstance(bc, FluxBoundaryCondition) or not isinstance(bc, ValueBoundaryCondition):
                raise NotImplementedError(f"EnthalpyMethodSeaIceModel: the {name} condition on T is a ValueBoundaryCondition or the default; "
                                          "flux and gradient conditions are not supported")
            v = bc.value
            if isinstance(v, RegriddedTimeSeries) or (isinstance(v, FieldTimeSeries) and not isinstance(v, ColumnTimeSeries)):
                raise NotImplementedError(f"EnthalpyMethodSeaIceModel: the {name} temperature series is a ColumnTimeSeries (numbers or (Ny, Nx) "
                                          "planes on the column grid)")
            if isinstance(v, ColumnTimeSeries):
                if v.grid.Nx != grid.Nx or v.grid.Ny != grid.Ny:
                    raise ValueError(f"EnthalpyMethodSeaIceModel: the {name} temperature series was made for another grid")
            elif callable(v):
                raise NotImplementedError(f"EnthalpyMethodSeaIceModel: a function-valued {name} temperature is not supported; sample it into a "
                                          "ColumnTimeSeries at the step times")
            elif not isinstance(v, float):
                shape = tuple(v.shape) if hasattr(v, "shape") else None
                if shape != (grid.Ny, grid.Nx):
                    raise ValueError(f"EnthalpyMethodSeaIceModel: the {name} temperature array has shape {shape}, (Ny, Nx) = {(grid.Ny, grid.Nx)} is needed")
            out.append((side, v))
        return out

    def _call(self, name, *args, on_model=True):
        fn = getattr(self.ctx.L, name)
        rc = fn(self.h, *args) if on_model else fn(*args)
        if rc != _lib.OK:
            raise _lib.CsiError(rc, self.ctx.L.csi_last_error(self.ctx.h).decode())

    def _set_boundary(self, side, value):
        if value is None:
            self._call("csi_enthalpy_boundary_set", side, _lib.ENTH_BC_NONE, 0.0, None, None)
        elif isinstance(value, float):
            self._call("csi_enthalpy_boundary_set", side, _lib.ENTH_BC_NUMBER, value, None, None)
        elif isinstance(value, ColumnTimeSeries):
            dev = torch.from_numpy(value.data).to(self.device)
            self._keep.append((dev, value.times))
            g = self.grid
            ts = _lib.TimeSeries(value.times.size, value.time_indexing.kind, _lib.SERIES_DEVICE, 0, value.time_indexing.period,
                                 value.times.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(dev.data_ptr()),
                                 1 if value.scalar else g.Nx, 1 if value.scalar else g.Nx * g.Ny)
            kind = _lib.ENTH_BC_SERIES_SCALAR if value.scalar else _lib.ENTH_BC_SERIES_PLANE
            self._call("csi_enthalpy_boundary_set", side, kind, 0.0, None, C.byref(ts))
        else:
            if isinstance(value, torch.Tensor):
                dev = value.to(device=self.device, dtype=torch.float64).contiguous()
            else:
                dev = torch.from_numpy(np.ascontiguousarray(value, dtype=np.float64)).to(self.device)
            self._keep.append(dev)
            self._call("csi_enthalpy_boundary_set", side, _lib.ENTH_BC_ARRAY, 0.0, C.c_void_p(dev.data_ptr()), None)

    # ---- the reference's surface ------------------------------------------------------------------------------------------------------
    def set(self, T=None, H=None):
        """set!(model; T) / set!(model; H): writes the field, then H = c T + L phi with the porosity held now / T = H / c and T's
        halos.  Neither updates porosity or diffusivity."""
        if T is not None and H is not None:
            raise ValueError("Cannot set both temperature and enthalpy!")
        if T is not None:
            self.state.T.set(T)
            self._call("csi_enthalpy_set", _lib.ENTH_T, self.clock.time)
        if H is not None:
            self.state.H.set(H)
            self._call("csi_enthalpy_set", _lib.ENTH_H, self.clock.time)

    def update_state(self):
        self._call("csi_enthalpy_update_state", self.clock.time)

    def time_step(self, dt):
        self.time_steps(dt, 1)

    def time_steps(self, dt, n):
        """n steps of dt: on chip, min(n, 64) sub-steps per launch with the state of 64 columns per wave held in LDS."""
        t = C.c_double()
        self._call("csi_enthalpy_time_step", float(dt), int(n), self.clock.time, C.byref(t))
        self.clock.time = t.value
        self.clock.iteration += int(n)

    def ice_thickness(self, melting_temperature=-0.1):
        """The example's diagnostic, made total (include/csi.h): an (Ny, Nx) NumPy array.  Waits for the device."""
        out = torch.empty((self.grid.Ny, self.grid.Nx), dtype=torch.float64, device=self.device)
        torch.cuda.synchronize(self.device)
        self._call("csi_enthalpy_ice_thickness", float(melting_temperature), C.c_void_p(out.data_ptr()))
        self.synchronize()
        return out.cpu().numpy()

    def last_launch(self):
        """What the last time_step / time_steps launched: form ("on_chip" / "per_step"), launches, sub-steps per launch, LDS bytes."""
        r = _lib.EnthalpyLaunch()
        self._call("csi_enthalpy_last_launch", C.byref(r))
        return dict(form=_FORMS[r.form], launches=r.launches, substeps_per_launch=r.substeps_per_launch, lds_bytes=r.lds_bytes)

    def synchronize(self):
        self.ctx.call("csi_sync")

    def fields(self):
        return dict(T=self.state.T, H=self.state.H, phi=self.state.phi, kappa=self.closure.kappa)

    def prognostic_state(self):
        """Host copies of H, T, phi, kappa (halo levels included) and the clock.  All four: T and kappa are not functions of H before
        the first update_state."""
        self.synchronize()
        out = {k: f.numpy().copy() for k, f in self.fields().items()}
        out["clock"] = (self.clock.time, self.clock.iteration)
        return out

    def restore_prognostic_state(self, state):
        self.synchronize()
        for k, f in self.fields().items():
            f.set_parent(state[k])
        self.clock.time, self.clock.iteration = state["clock"]

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.csi_enthalpy_destroy(self.h)
            self.h = C.c_void_p()
        self.ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
