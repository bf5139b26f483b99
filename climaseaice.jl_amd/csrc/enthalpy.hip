// enthalpy.hip -- the enthalpy-method column model (include/csi.h, "enthalpy-method column model"): the reference's
// EnthalpyMethodSeaIceModel (src/EnthalpyMethodSeaIceModel.jl) with MolecularDiffusivity, stepped explicitly.
//
//   k_enthalpy_steps<ON_CHIP>   n sub-steps of time_step! (:168-185) in one launch; per column and sub-step, k = 1 .. Nz upward:
//                                   flux[k] = ((kappa[k] + kappa[k-1]) / 2) * ((T[k] - T[k-1]) / dzf[k])        k = 1 .. Nz + 1
//                                   G[k]    = (flux[k+1] - flux[k]) / dzc[k]
//                                   H[k]    = H[k] + dt * G[k]
//                               then update_state! (:161-166) at the time the sub-step STARTED from:
//                                   T[k]    = H[k] / c ;  T[0] = 2 Tb - T[1] | T[1] ;  T[Nz+1] = 2 Tt - T[Nz] | T[Nz]
//                                   phi[k]  = T[k] < 0 ? 1 : 0
//                                   kappa[k] = k_ice * (1 - phi[k]) + k_water * phi[k] ;  kappa[0] = kappa[1], kappa[Nz+1] = kappa[Nz]
//                               (frozen cells, phi = 1, take k_water: the reference's assignment, mirrored.)
//   k_enthalpy_state<MODE>      set!(model; T), set!(model; H) and update_state! on their own
//   k_enthalpy_thickness        the example's ice-thickness diagnostic, made total
//
// One thread per column, lanes along x, level k of every array one coalesced plane.  A thread marches upward and updates in place: it
// carries the lower face's flux and the old T[k], kappa[k] in registers and reads the old level k + 1 before that level's turn, so
// no second copy of the column exists.  Columns never exchange data: no barrier, no cross-lane operation.
//
// Two storage forms share substep():
//   on chip    H[1 .. Nz] and T[0 .. Nz + 1] of the wave's 64 columns live in LDS as [level][lane] (8-byte accesses of consecutive
//              lanes: conflict-free), (2 Nz + 2) * 512 bytes; the launch runs n sub-steps.  The first reads kappa from memory (the
//              held kappa need not be the one T implies: set! updates neither phi nor kappa), the later ones derive it from T; after
//              the last, H, T, phi, kappa are stored once, the halo levels of T and kappa included.
//   per step   the same body on the caller's arrays, one launch per step, for columns too deep for LDS.
// Compiled with -ffp-contract=off: the operations above in that order, IEEE division (three per cell and step: by dzf, by dzc, by c;
// the division by 2 is exact), STRICT and FAST alike.  No scratch.
#include "enthalpy_dev.h"

namespace csi {

namespace {

__device__ __forceinline__ double kappa_of(const EnthDev& E, double T) {
    const double phi = T < 0.0 ? 1.0 : 0.0;
    return E.k_ice * (1.0 - phi) + E.k_water * phi;
}

// the boundary temperature of a side for this column (boff: the column's offset in a plane), sub-step q of the table
__device__ __forceinline__ double side_value(const EnthSide& s, const EnthSteps& S, int side, int q, long boff) {
    if (s.kind == ENTH_BC_NONE) return 0.0;              // (unused: halo_of takes the neighbour)
    if (s.kind == ENTH_BC_NUMBER) return s.number;
    if (s.kind == ENTH_BC_ARRAY) return s.data[boff];
    const int n1 = S.n1[side][q], n2 = S.n2[side][q];
    const double p1 = s.data[(long)n1 * s.slice_stride + boff];
    if (n1 == n2) return p1;
    const double frac = S.frac[side][q];
    const double p2 = s.data[(long)n2 * s.slice_stride + boff];
    return p2 * frac + p1 * (1.0 - frac);
}

__device__ __forceinline__ long side_offset(const EnthSide& s, int i, int j) {
    return (s.kind == ENTH_BC_ARRAY || s.kind == ENTH_BC_SERIES_PLANE) ? (long)j * s.ld + i : 0;
}

__device__ __forceinline__ double halo_of(const EnthSide& s, double Tb, double Tn) { return s.kind == ENTH_BC_NONE ? Tn : 2.0 * Tb - Tn; }

// H and T of one column in the caller's arrays / in the wave's LDS image
struct GlobalColumn {
    double *H, *T;
    long plane;
    __device__ __forceinline__ double getT(int k) const { return T[k * plane]; }
    __device__ __forceinline__ double getH(int k) const { return H[k * plane]; }
    __device__ __forceinline__ void setT(int k, double v) { T[k * plane] = v; }
    __device__ __forceinline__ void setH(int k, double v) { H[k * plane] = v; }
};
struct LdsColumn {
    double *T, *H;           // T: level 0 of this lane; H: level 0 (never touched) of this lane
    __device__ __forceinline__ double getT(int k) const { return T[k * kEnthLanes]; }
    __device__ __forceinline__ double getH(int k) const { return H[k * kEnthLanes]; }
    __device__ __forceinline__ void setT(int k, double v) { T[k * kEnthLanes] = v; }
    __device__ __forceinline__ void setH(int k, double v) { H[k * kEnthLanes] = v; }
};

// One sub-step of one column.  kappa_mem: kappa is read from memory (else derived from T); store_aux: phi and kappa are stored.
// kap / phi: level 0 of this column in the caller's arrays.
template <class Column>
__device__ __forceinline__ void substep(const EnthDev& E, Column& C, const double* kap_in, double* kap_out, double* phi_out, bool kappa_mem,
                                        bool store_aux, double Tb, double Tt) {
    const int Nz = E.nz;
    const long P = E.plane;
    const double Tm = C.getT(0);
    double Tk = C.getT(1);
    double kk = kappa_mem ? kap_in[P] : kappa_of(E, Tk);
    const double km = kappa_mem ? kap_in[0] : kk;
    double flo = ((kk + km) / 2.0) * ((Tk - Tm) / E.dzf[0]);
    double T1 = 0.0, Tn = 0.0, k1 = 0.0, kn = 0.0;
    for (int k = 1; k <= Nz; ++k) {
        const double Tp = C.getT(k + 1);
        const double kp = kappa_mem ? kap_in[(k + 1) * P] : (k < Nz ? kappa_of(E, Tp) : kk);
        const double fhi = ((kp + kk) / 2.0) * ((Tp - Tk) / E.dzf[k]);
        const double G = (fhi - flo) / E.dzc[k - 1];
        const double Hn = C.getH(k) + E.dt * G;
        Tn = Hn / E.c;
        C.setH(k, Hn);
        C.setT(k, Tn);
        if (store_aux) {
            const double ph = Tn < 0.0 ? 1.0 : 0.0;
            kn = E.k_ice * (1.0 - ph) + E.k_water * ph;
            phi_out[k * P] = ph;
            kap_out[k * P] = kn;
            if (k == 1) k1 = kn;
        }
        if (k == 1) T1 = Tn;
        flo = fhi; Tk = Tp; kk = kp;
    }
    C.setT(0, halo_of(E.side[0], Tb, T1));
    C.setT(Nz + 1, halo_of(E.side[1], Tt, Tn));
    if (store_aux) {
        kap_out[0] = k1;
        kap_out[(Nz + 1) * P] = kn;
    }
}

}  // namespace

template <bool ON_CHIP>
__global__ void __launch_bounds__(ON_CHIP ? kEnthLanes : 256) k_enthalpy_steps(EnthDev E, EnthSteps S) {
    extern __shared__ double lds[];
    const long col = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= E.plane) return;
    const int j = (int)(col / E.nx), i = (int)(col - (long)j * E.nx);
    const long off[2] = {side_offset(E.side[0], i, j), side_offset(E.side[1], i, j)};
    const int Nz = E.nz;
    const long P = E.plane;
    if (ON_CHIP) {
        LdsColumn C{lds + threadIdx.x, lds + (Nz + 2) * kEnthLanes - kEnthLanes + threadIdx.x};
        for (int k = 0; k <= Nz + 1; ++k) C.setT(k, E.T[k * P + col]);
        for (int k = 1; k <= Nz; ++k) C.setH(k, E.H[k * P + col]);
        for (int q = 0; q < S.n; ++q) {
            const double Tb = side_value(E.side[0], S, 0, q, off[0]), Tt = side_value(E.side[1], S, 1, q, off[1]);
            substep(E, C, E.kappa + col, E.kappa + col, E.phi + col, q == 0, q == S.n - 1, Tb, Tt);
        }
        for (int k = 0; k <= Nz + 1; ++k) E.T[k * P + col] = C.getT(k);
        for (int k = 1; k <= Nz; ++k) E.H[k * P + col] = C.getH(k);
    } else {
        GlobalColumn C{E.H + col, E.T + col, P};
        const double Tb = side_value(E.side[0], S, 0, 0, off[0]), Tt = side_value(E.side[1], S, 1, 0, off[1]);
        substep(E, C, E.kappa + col, E.kappa + col, E.phi + col, true, true, Tb, Tt);
    }
}

// set!(model; T): H = c T + L phi (the phi held now).  set!(model; H): T = H / c and T's halos.  update_state!: that, then phi and
// kappa with its no-flux halos.  H's and phi's halo levels are neither read nor written.
template <int MODE>
__global__ void __launch_bounds__(256) k_enthalpy_state(EnthDev E, EnthSteps S) {
    const long col = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= E.plane) return;
    const int Nz = E.nz;
    const long P = E.plane;
    if (MODE == ENTH_SET_T) {
        for (int k = 1; k <= Nz; ++k) E.H[k * P + col] = E.c * E.T[k * P + col] + E.L * E.phi[k * P + col];
        return;
    }
    const int j = (int)(col / E.nx), i = (int)(col - (long)j * E.nx);
    const double Tb = side_value(E.side[0], S, 0, 0, side_offset(E.side[0], i, j));
    const double Tt = side_value(E.side[1], S, 1, 0, side_offset(E.side[1], i, j));
    double T1 = 0.0, Tn = 0.0, k1 = 0.0, kn = 0.0;
    for (int k = 1; k <= Nz; ++k) {
        Tn = E.H[k * P + col] / E.c;
        E.T[k * P + col] = Tn;
        if (k == 1) T1 = Tn;
        if (MODE == ENTH_UPDATE_STATE) {
            const double ph = Tn < 0.0 ? 1.0 : 0.0;
            kn = E.k_ice * (1.0 - ph) + E.k_water * ph;
            E.phi[k * P + col] = ph;
            E.kappa[k * P + col] = kn;
            if (k == 1) k1 = kn;
        }
    }
    E.T[col] = halo_of(E.side[0], Tb, T1);
    E.T[(Nz + 1) * P + col] = halo_of(E.side[1], Tt, Tn);
    if (MODE == ENTH_UPDATE_STATE) {
        E.kappa[col] = k1;
        E.kappa[(Nz + 1) * P + col] = kn;
    }
}

// kw: the levels from the bottom up whose T >= Tm, stopping at the first that is not.  0: -zf[1]; Nz: 0; else the example's linear
// interpolation between zc[kw] and zc[kw + 1] (examples/diffusive_ice_column_model.jl:115-127)
__global__ void __launch_bounds__(256) k_enthalpy_thickness(EnthDev E, double Tm, double z_bottom, double* out) {
    const long col = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= E.plane) return;
    const int Nz = E.nz;
    const long P = E.plane;
    int kw = 0;
    double Tw = 0.0, Ti = 0.0;
    for (int k = 1; k <= Nz; ++k) {
        Ti = E.T[k * P + col];
        if (!(Ti >= Tm)) break;
        Tw = Ti;
        kw = k;
    }
    double h;
    if (kw == 0) {
        h = -z_bottom;
    } else if (kw == Nz) {
        h = 0.0;
    } else {
        const double dTdz = (Ti - Tw) / E.dzf[kw];
        const double z = E.zc[kw - 1] + (Tm - Tw) / dTdz;
        h = -z;
    }
    out[col] = h;
}

hipError_t enthalpy_allow_lds(size_t lds_bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_enthalpy_steps<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

void launch_enthalpy_steps(const EnthDev& E, const EnthSteps& S, bool on_chip, size_t lds_bytes, hipStream_t st) {
    if (E.plane <= 0) return;
    if (on_chip) {
        const unsigned g = (unsigned)((E.plane + kEnthLanes - 1) / kEnthLanes);
        hipLaunchKernelGGL(k_enthalpy_steps<true>, dim3(g), dim3(kEnthLanes), lds_bytes, st, E, S);
    } else {
        const unsigned g = (unsigned)((E.plane + 255) / 256);
        hipLaunchKernelGGL(k_enthalpy_steps<false>, dim3(g), dim3(256), 0, st, E, S);
    }
}

void launch_enthalpy_state(const EnthDev& E, const EnthSteps& S, int mode, hipStream_t st) {
    if (E.plane <= 0) return;
    const dim3 g((unsigned)((E.plane + 255) / 256)), b(256);
    if (mode == ENTH_SET_T) hipLaunchKernelGGL(k_enthalpy_state<ENTH_SET_T>, g, b, 0, st, E, S);
    else if (mode == ENTH_SET_H) hipLaunchKernelGGL(k_enthalpy_state<ENTH_SET_H>, g, b, 0, st, E, S);
    else hipLaunchKernelGGL(k_enthalpy_state<ENTH_UPDATE_STATE>, g, b, 0, st, E, S);
}

void launch_enthalpy_thickness(const EnthDev& E, double Tm, double z_bottom, double* out, hipStream_t st) {
    if (E.plane <= 0) return;
    hipLaunchKernelGGL(k_enthalpy_thickness, dim3((unsigned)((E.plane + 255) / 256)), dim3(256), 0, st, E, Tm, z_bottom, out);
}

}  // namespace csi
