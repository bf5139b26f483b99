// enthalpy_dev.h -- what enthalpy.hip (kernels) and csi_enthalpy.hip (host) share: the descriptors of the enthalpy-method column model
// (include/csi.h, "enthalpy-method column model").
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace csi {

constexpr int kEnthMaxSubsteps = 64;             // CSI_ENTH_MAX_SUBSTEPS: sub-steps of one on-chip launch (the size of EnthSteps)
constexpr int kEnthLanes = 64;                   // columns of a wave: one block of the on-chip form

// csi_enthalpy_bc_kind
enum { ENTH_BC_NONE = 0, ENTH_BC_NUMBER = 1, ENTH_BC_ARRAY = 2, ENTH_BC_SERIES_SCALAR = 3, ENTH_BC_SERIES_PLANE = 4 };

// the boundary temperature of one side (0 bottom, 1 top)
struct EnthSide {
    int kind, pad;
    double number;
    const double* data;      // ARRAY: (Ny, Nx) values; SERIES_*: all slices
    long ld;                 // doubles between the rows of a plane
    long slice_stride;       // doubles between slices
};

struct EnthDev {
    int nx, ny, nz, pad;
    long plane;              // Ny * Nx: doubles between levels
    double *H, *T, *phi, *kappa;      // (Nz + 2, Ny, Nx), levels 0 and Nz + 1 the z halos
    const double* dzc;       // [Nz]      dzc[k - 1] = zf[k + 1] - zf[k]
    const double* dzf;       // [Nz + 1]  dzf[k - 1] = the spacing of face k
    const double* zc;        // [Nz]      zc[k - 1]: the midpoint of the faces of level k
    double c, L, k_ice, k_water, dt;
    EnthSide side[2];
};

// per sub-step and side: the two slices and the weight of csi_time_series_plan at the time the sub-step starts from
struct EnthSteps {
    int n, pad;
    int n1[2][kEnthMaxSubsteps], n2[2][kEnthMaxSubsteps];
    double frac[2][kEnthMaxSubsteps];
};

// mode of k_enthalpy_state
enum { ENTH_SET_T = 0, ENTH_SET_H = 1, ENTH_UPDATE_STATE = 2 };

void launch_enthalpy_steps(const EnthDev& E, const EnthSteps& S, bool on_chip, size_t lds_bytes, hipStream_t st);
void launch_enthalpy_state(const EnthDev& E, const EnthSteps& S, int mode, hipStream_t st);
void launch_enthalpy_thickness(const EnthDev& E, double Tm, double z_bottom, double* out, hipStream_t st);
hipError_t enthalpy_allow_lds(size_t lds_bytes);      // once per process and size class: lets a block of the on-chip form take lds_bytes

}  // namespace csi
