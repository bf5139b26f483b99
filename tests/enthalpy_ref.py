"""NumPy restatement of the enthalpy-method column model, written from the statement in include/csi.h ("enthalpy-method column
model"): set, update_state, one step, n steps, the ice thickness and the clock.  Plain double arithmetic in the header's operation
order on whole (Nz + 2, Ny, Nx) arrays, so the library has to agree BIT FOR BIT.  Series-valued boundary temperatures go through
tests/time_series_ref.py.  The oracle of tests/test_enthalpy_ref.py and tests/test_gpu_enthalpy.py.

`mistake` builds a deliberately WRONG model, for the tests that show a mistake is visible: "late_boundary" (boundary values at the
time a step ends), "swap_kappa" (frozen cells take kappa_ice), "dzc_for_dzf" (cell spacings where face spacings belong)."""
import numpy as np

import time_series_ref as tsr

REFERENCE_DENSITY = 999.8
DEFAULTS = dict(c=2090.0 / REFERENCE_DENSITY, L=3.3e5 / REFERENCE_DENSITY, kappa_ice=1e-5, kappa_water=1e-6)


class Series:
    """A boundary temperature at a list of times: data (Nt,) numbers or (Nt, Ny, Nx) planes."""

    def __init__(self, times, data, indexing=tsr.LINEAR, period=0.0):
        self.times, self.data = np.asarray(times, dtype=np.float64), np.asarray(data, dtype=np.float64)
        self.indexing, self.period = indexing, period

    def at(self, t):
        return tsr.at(self.times, self.data, self.indexing, self.period, t)


def uniform_faces(bottom, top, Nz):
    """ColumnGrid's faces for z = (bottom, top)."""
    if Nz == 1:
        return np.array([bottom, top], dtype=np.float64)
    dz = (np.float64(top) - np.float64(bottom)) / Nz
    f = np.float64(bottom) + np.arange(Nz + 1) * dz
    f[-1] = top
    return f


def metrics(zf):
    """(zc[Nz], dzc[Nz], dzf[Nz + 1]) of the header's OPERATORS paragraph."""
    zf = np.asarray(zf, dtype=np.float64)
    zc = (zf[:-1] + zf[1:]) / 2.0
    dzc = zf[1:] - zf[:-1]
    dzf = np.empty(zf.size)
    dzf[1:-1] = zc[1:] - zc[:-1]
    dzf[0], dzf[-1] = dzc[0], dzc[-1]
    return zc, dzc, dzf


class Model:
    def __init__(self, Nx, Ny, zf, bottom=None, top=None, c=DEFAULTS["c"], L=DEFAULTS["L"], kappa_ice=DEFAULTS["kappa_ice"],
                 kappa_water=DEFAULTS["kappa_water"], mistake=None):
        self.Nx, self.Ny, self.zf = Nx, Ny, np.asarray(zf, dtype=np.float64)
        self.Nz = self.zf.size - 1
        self.zc, self.dzc, self.dzf = metrics(self.zf)
        self.c, self.L, self.kappa_ice, self.kappa_water = (np.float64(v) for v in (c, L, kappa_ice, kappa_water))
        self.sides = (bottom, top)          # None | number | (Ny, Nx) array | Series
        self.mistake = mistake
        if mistake == "swap_kappa":
            self.kappa_ice, self.kappa_water = self.kappa_water, self.kappa_ice
        if mistake == "dzc_for_dzf":
            self.dzf = np.concatenate([self.dzc, self.dzc[-1:]])
        shape = (self.Nz + 2, Ny, Nx)
        self.H, self.T, self.phi, self.kappa = (np.zeros(shape) for _ in range(4))
        self.time, self.iteration = np.float64(0.0), 0

    def copy_state_from(self, other):
        for k in ("H", "T", "phi", "kappa"):
            getattr(self, k)[...] = getattr(other, k)
        self.time, self.iteration = other.time, other.iteration

    # ---- boundary temperatures --------------------------------------------------------------------------------------------------------
    def side_value(self, s, t):
        b = self.sides[s]
        if b is None:
            return None
        if isinstance(b, Series):
            return np.broadcast_to(b.at(t), (self.Ny, self.Nx))
        return np.broadcast_to(np.asarray(b, dtype=np.float64), (self.Ny, self.Nx))

    def fill_T_halos(self, t):
        T = self.T
        for s, (halo, nb) in enumerate(((0, 1), (self.Nz + 1, self.Nz))):
            v = self.side_value(s, t)
            T[halo] = T[nb] if v is None else 2.0 * v - T[nb]

    # ---- set!, update_state!, time_step! ----------------------------------------------------------------------------------------------
    def set_T(self, T):
        self.T[1:-1] = np.broadcast_to(_profile(T), self.T[1:-1].shape)
        self.H[1:-1] = self.c * self.T[1:-1] + self.L * self.phi[1:-1]

    def set_H(self, H):
        self.H[1:-1] = np.broadcast_to(_profile(H), self.H[1:-1].shape)
        self.T[1:-1] = self.H[1:-1] / self.c
        self.fill_T_halos(self.time)

    def update_state(self, t=None):
        t = self.time if t is None else t
        self.T[1:-1] = self.H[1:-1] / self.c
        self.fill_T_halos(t)
        self.phi[1:-1] = np.where(self.T[1:-1] < 0.0, 1.0, 0.0)
        self.kappa[1:-1] = self.kappa_ice * (1.0 - self.phi[1:-1]) + self.kappa_water * self.phi[1:-1]
        self.kappa[0], self.kappa[-1] = self.kappa[1], self.kappa[-2]

    def tendency(self):
        T, kap = self.T, self.kappa
        flux = ((kap[1:] + kap[:-1]) / 2.0) * ((T[1:] - T[:-1]) / self.dzf[:, None, None])
        return (flux[1:] - flux[:-1]) / self.dzc[:, None, None]

    def time_step(self, dt):
        dt = np.float64(dt)
        self.H[1:-1] = self.H[1:-1] + dt * self.tendency()
        self.update_state(self.time + dt if self.mistake == "late_boundary" else self.time)
        self.time = self.time + dt
        self.iteration += 1

    def time_steps(self, dt, n):
        for _ in range(n):
            self.time_step(dt)

    # ---- the ice thickness --------------------------------------------------------------------------------------------------------------
    def ice_thickness(self, Tm=-0.1):
        out = np.empty((self.Ny, self.Nx))
        Tm = np.float64(Tm)
        for j in range(self.Ny):
            for i in range(self.Nx):
                T = self.T[1:-1, j, i]
                kw = 0
                while kw < self.Nz and T[kw] >= Tm:
                    kw += 1
                if kw == 0:
                    out[j, i] = -self.zf[0]
                elif kw == self.Nz:
                    out[j, i] = 0.0
                else:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        dTdz = (T[kw] - T[kw - 1]) / self.dzf[kw]
                        z = self.zc[kw - 1] + (Tm - T[kw - 1]) / dTdz
                    out[j, i] = -z
        return out


def _profile(v):
    v = np.asarray(v, dtype=np.float64)
    return v[:, None, None] if v.ndim == 1 else v


def example_thickness_binary_search(T, zc, dzf, Tm):
    """examples/diffusive_ice_column_model.jl:115-127 as written: searchsortedlast(Ti, Tm, rev = true) on a profile that decreases
    upward (1-based kw), then the linear interpolation."""
    lo, hi = 0, T.size + 1                     # Julia's searchsortedlast on a reverse-sorted vector
    while lo < hi - 1:
        m = (lo + hi) // 2
        if Tm > T[m - 1]:                      # lt(rev, Tm, T[m]): Tm sorts before T[m]
            hi = m
        else:
            lo = m
    kw = lo
    ki = kw + 1
    dTdz = (T[ki - 1] - T[kw - 1]) / dzf[ki - 1]
    return -(zc[kw - 1] + (Tm - T[kw - 1]) / dTdz)


# ---- the reference's example (examples/diffusive_ice_column_model.jl) -------------------------------------------------------------------
DAY = 86400.0


def example_air_ice_temperature(t):
    return (-0.5 / DAY) * t + 5 * np.sin(2 * np.pi * t / DAY) + -5


def example_ice_ocean_temperature(t):
    return (-0.1 / DAY) * t + 1.1


def step_times(dt, n, t0=0.0):
    """The clock's own times: t0, then one addition of dt per step (NOT k * dt), so that a series sampled there has its nodes exactly
    on the step times."""
    t = np.empty(n)
    t[0] = t0
    for k in range(1, n):
        t[k] = t[k - 1] + np.float64(dt)
    return t


def example_model(nsteps, mistake=None, Nx=1, Ny=1):
    """The example's column (20 levels, z = (-1, 0), dt = 0.1 dz^2 / kappa), its two boundary functions sampled at the step times,
    T = 1.1 set and update_state called, as run! does.  Returns (model, dt)."""
    zf = uniform_faces(-1.0, 0.0, 20)
    dt = 0.1 * float(np.min(zf[1:] - zf[:-1])) ** 2 / 1e-5
    times = step_times(dt, nsteps + 2)
    m = Model(Nx, Ny, zf, bottom=Series(times, example_ice_ocean_temperature(times)), top=Series(times, example_air_ice_temperature(times)),
              mistake=mistake)
    m.set_T(1.1)
    m.update_state()
    return m, dt
