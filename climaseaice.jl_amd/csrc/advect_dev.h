// advect_dev.h -- the advection reconstructions as device code, shared by advect.hip (h, aice, snow thickness) and tracers.hip
// (advected tracers): WENO(3 | 5 | 7) in the WENO-Z form, UpwindBiased(3 | 5), their FAST and f32-weight forms, the order reduction
// next to walls and immersed cells (buffer_at) and reconstruct<>.  Moved out of advect.hip unchanged; both units are compiled with
// -ffp-contract=off, so a tracer reconstructed here gets the operations h gets.
#pragma once
#include "csi_dev.h"
#include "evp_fast_math.h"

namespace csi {
// Julia's max(a, b) for floats: NaN if either is NaN
__device__ __forceinline__ double jmax(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? b : a); }

namespace adv {

#define WENO_EPS 1e-8

__device__ __forceinline__ double weno5(const double* p) {
    double q0 = (2 * p[2] + 5 * p[3] - p[4]) / 6;
    double q1 = (-p[1] + 5 * p[2] + 2 * p[3]) / 6;
    double q2 = (2 * p[0] - 7 * p[1] + 11 * p[2]) / 6;
    double b0 = (p[2] * (10 * p[2] - 31 * p[3] + 11 * p[4]) + p[3] * (25 * p[3] - 19 * p[4]) + p[4] * (4 * p[4])) / 3;
    double b1 = (p[1] * (4 * p[1] - 13 * p[2] + 5 * p[3]) + p[2] * (13 * p[2] - 13 * p[3]) + p[3] * (4 * p[3])) / 3;
    double b2 = (p[0] * (4 * p[0] - 19 * p[1] + 11 * p[2]) + p[1] * (25 * p[1] - 31 * p[2]) + p[2] * (10 * p[2])) / 3;
    double tau = fabs(b0 - b2);
    double r0 = tau / (b0 + WENO_EPS), r1 = tau / (b1 + WENO_EPS), r2 = tau / (b2 + WENO_EPS);
    double a0 = (3.0 / 10) * (1 + r0 * r0);
    double a1 = (3.0 / 5) * (1 + r1 * r1);
    double a2 = (1.0 / 10) * (1 + r2 * r2);
    double s = a0 + a1 + a2;
    return (a0 * q0 + a1 * q1 + a2 * q2) / s;
}
__device__ __forceinline__ double upwind5(const double* p) {
    return (2 * p[0] - 13 * p[1] + 47 * p[2] + 27 * p[3] - 3 * p[4]) / 60;
}
__device__ __forceinline__ double weno7(const double* p) {
    double q0 = (3 * p[3] + 13 * p[4] - 5 * p[5] + p[6]) / 12;
    double q1 = (-p[2] + 7 * p[3] + 7 * p[4] - p[5]) / 12;
    double q2 = (p[1] - 5 * p[2] + 13 * p[3] + 3 * p[4]) / 12;
    double q3 = (-3 * p[0] + 13 * p[1] - 23 * p[2] + 25 * p[3]) / 12;
    double b0 = p[3] * (2.107 * p[3] - 9.402 * p[4] + 7.042 * p[5] - 1.854 * p[6]) +
                p[4] * (11.003 * p[4] - 17.246 * p[5] + 4.642 * p[6]) + p[5] * (7.043 * p[5] - 3.882 * p[6]) + p[6] * (0.547 * p[6]);
    double b1 = p[2] * (0.547 * p[2] - 2.522 * p[3] + 1.922 * p[4] - 0.494 * p[5]) +
                p[3] * (3.443 * p[3] - 5.966 * p[4] + 1.602 * p[5]) + p[4] * (2.843 * p[4] - 1.642 * p[5]) + p[5] * (0.267 * p[5]);
    double b2 = p[1] * (0.267 * p[1] - 1.642 * p[2] + 1.602 * p[3] - 0.494 * p[4]) +
                p[2] * (2.843 * p[2] - 5.966 * p[3] + 1.922 * p[4]) + p[3] * (3.443 * p[3] - 2.522 * p[4]) + p[4] * (0.547 * p[4]);
    double b3 = p[0] * (0.547 * p[0] - 3.882 * p[1] + 4.642 * p[2] - 1.854 * p[3]) +
                p[1] * (7.043 * p[1] - 17.246 * p[2] + 7.042 * p[3]) + p[2] * (11.003 * p[2] - 9.402 * p[3]) + p[3] * (2.107 * p[3]);
    double tau = fabs(b0 + 3 * b1 - 3 * b2 - b3);
    double r0 = tau / (b0 + WENO_EPS), r1 = tau / (b1 + WENO_EPS), r2 = tau / (b2 + WENO_EPS), r3 = tau / (b3 + WENO_EPS);
    double a0 = (4.0 / 35) * (1 + r0 * r0);
    double a1 = (18.0 / 35) * (1 + r1 * r1);
    double a2 = (12.0 / 35) * (1 + r2 * r2);
    double a3 = (1.0 / 35) * (1 + r3 * r3);
    double s = a0 + a1 + a2 + a3;
    return (a0 * q0 + a1 * q1 + a2 * q2 + a3 * q3) / s;
}

__device__ __forceinline__ double weno3(const double* p) {
    double q0 = (p[1] + p[2]) / 2;
    double q1 = (-p[0] + 3 * p[1]) / 2;
    double b0 = p[1] * (p[1] - 2 * p[2]) + p[2] * p[2];
    double b1 = p[0] * (p[0] - 2 * p[1]) + p[1] * p[1];
    double tau = fabs(b0 - b1);
    double r0 = tau / (b0 + WENO_EPS), r1 = tau / (b1 + WENO_EPS);
    double a0 = (2.0 / 3) * (1 + r0 * r0);
    double a1 = (1.0 / 3) * (1 + r1 * r1);
    double s = a0 + a1;
    return (a0 * q0 + a1 * q1) / s;
}
__device__ __forceinline__ double upwind3(const double* p) { return (-p[0] + 5 * p[1] + 2 * p[2]) / 6; }

// ---- FAST-mode reconstructions (see the header).  Candidate polynomials, weights and the final combination are contracted; divisions
// are reciprocals (fm::rcp: hardware seed + one Newton step) or multiplications by constants.  The smoothness indicators and tau:
// rounds 3 - 4 evaluated them EXACTLY as in STRICT mode (no contraction) -- they are small differences of O(c^2) terms, and a
// rounding-level change of their evaluation moves the nonlinear weights by ~1e-9 relative and the tendencies by 7e-13 of max|G|
// (measured), over the 1e-13 then stated for the tendencies.  Round 5 (CSI_ADV_FAST_BETA = 1, the default): they are contracted too --
// the uncontracted quadratic forms were 92 of a WENO7 reconstruction's ~150 FP64 instructions (56 contracted) -- and the FAST
// tolerance on the TENDENCIES is stated as 1e-12 of max|G|; the tolerance on what the north star names, h and aice after an update,
// stays 1e-13 relative (dt |dG| = 120 s x 1e-12 x 1e-6 m/s against h ~ 0.3 m: four orders inside it).  STRICT is untouched.
#ifndef CSI_ADV_FAST_BETA
#define CSI_ADV_FAST_BETA 1
#endif
#if CSI_ADV_FAST_BETA
#define CSI_BETA_CONTRACT _Pragma("clang fp contract(fast)")
#else
#define CSI_BETA_CONTRACT
#endif
__device__ __forceinline__ double weno3_fast(const double* p) {
    double b0, b1;
    {
        CSI_BETA_CONTRACT
        b0 = p[1] * (p[1] - 2 * p[2]) + p[2] * p[2];
        b1 = p[0] * (p[0] - 2 * p[1]) + p[1] * p[1];
    }
    const double tau = fabs(b0 - b1);
    {
#pragma clang fp contract(fast)
        const double q0 = 0.5 * (p[1] + p[2]);
        const double q1 = 0.5 * (3 * p[1] - p[0]);
        const double r0 = tau * fm::rcp(b0 + WENO_EPS), r1 = tau * fm::rcp(b1 + WENO_EPS);
        const double a0 = (2.0 / 3) * (1 + r0 * r0);
        const double a1 = (1.0 / 3) * (1 + r1 * r1);
        return (a0 * q0 + a1 * q1) * fm::rcp(a0 + a1);
    }
}
__device__ __forceinline__ double upwind3_fast(const double* p) {
#pragma clang fp contract(fast)
    return (5 * p[1] + 2 * p[2] - p[0]) * (1.0 / 6);
}
__device__ __forceinline__ double weno5_fast(const double* p) {
    double b0, b1, b2;
    {
        CSI_BETA_CONTRACT
#if CSI_ADV_FAST_BETA
        constexpr double third = 1.0 / 3;
        b0 = (p[2] * (10 * p[2] - 31 * p[3] + 11 * p[4]) + p[3] * (25 * p[3] - 19 * p[4]) + p[4] * (4 * p[4])) * third;
        b1 = (p[1] * (4 * p[1] - 13 * p[2] + 5 * p[3]) + p[2] * (13 * p[2] - 13 * p[3]) + p[3] * (4 * p[3])) * third;
        b2 = (p[0] * (4 * p[0] - 19 * p[1] + 11 * p[2]) + p[1] * (25 * p[1] - 31 * p[2]) + p[2] * (10 * p[2])) * third;
#else
        b0 = (p[2] * (10 * p[2] - 31 * p[3] + 11 * p[4]) + p[3] * (25 * p[3] - 19 * p[4]) + p[4] * (4 * p[4])) / 3;
        b1 = (p[1] * (4 * p[1] - 13 * p[2] + 5 * p[3]) + p[2] * (13 * p[2] - 13 * p[3]) + p[3] * (4 * p[3])) / 3;
        b2 = (p[0] * (4 * p[0] - 19 * p[1] + 11 * p[2]) + p[1] * (25 * p[1] - 31 * p[2]) + p[2] * (10 * p[2])) / 3;
#endif
    }
    const double tau = fabs(b0 - b2);
    {
#pragma clang fp contract(fast)
        const double q0 = (2 * p[2] + 5 * p[3] - p[4]) * (1.0 / 6);
        const double q1 = (5 * p[2] + 2 * p[3] - p[1]) * (1.0 / 6);
        const double q2 = (2 * p[0] - 7 * p[1] + 11 * p[2]) * (1.0 / 6);
        const double r0 = tau * fm::rcp(b0 + WENO_EPS), r1 = tau * fm::rcp(b1 + WENO_EPS), r2 = tau * fm::rcp(b2 + WENO_EPS);
        const double a0 = (3.0 / 10) * (1 + r0 * r0);
        const double a1 = (3.0 / 5) * (1 + r1 * r1);
        const double a2 = (1.0 / 10) * (1 + r2 * r2);
        return (a0 * q0 + a1 * q1 + a2 * q2) * fm::rcp(a0 + a1 + a2);
    }
}
__device__ __forceinline__ double upwind5_fast(const double* p) {
#pragma clang fp contract(fast)
    return (2 * p[0] - 13 * p[1] + 47 * p[2] + 27 * p[3] - 3 * p[4]) * (1.0 / 60);
}
__device__ __forceinline__ double weno7_fast(const double* p) {
    double b0, b1, b2, b3;
    {
        CSI_BETA_CONTRACT
        b0 = p[3] * (2.107 * p[3] - 9.402 * p[4] + 7.042 * p[5] - 1.854 * p[6]) +
             p[4] * (11.003 * p[4] - 17.246 * p[5] + 4.642 * p[6]) + p[5] * (7.043 * p[5] - 3.882 * p[6]) + p[6] * (0.547 * p[6]);
        b1 = p[2] * (0.547 * p[2] - 2.522 * p[3] + 1.922 * p[4] - 0.494 * p[5]) +
             p[3] * (3.443 * p[3] - 5.966 * p[4] + 1.602 * p[5]) + p[4] * (2.843 * p[4] - 1.642 * p[5]) + p[5] * (0.267 * p[5]);
        b2 = p[1] * (0.267 * p[1] - 1.642 * p[2] + 1.602 * p[3] - 0.494 * p[4]) +
             p[2] * (2.843 * p[2] - 5.966 * p[3] + 1.922 * p[4]) + p[3] * (3.443 * p[3] - 2.522 * p[4]) + p[4] * (0.547 * p[4]);
        b3 = p[0] * (0.547 * p[0] - 3.882 * p[1] + 4.642 * p[2] - 1.854 * p[3]) +
             p[1] * (7.043 * p[1] - 17.246 * p[2] + 7.042 * p[3]) + p[2] * (11.003 * p[2] - 9.402 * p[3]) + p[3] * (2.107 * p[3]);
    }
    const double tau = fabs(b0 + 3 * b1 - 3 * b2 - b3);
    {
#pragma clang fp contract(fast)
        const double q0 = (3 * p[3] + 13 * p[4] - 5 * p[5] + p[6]) * (1.0 / 12);
        const double q1 = (7 * p[3] + 7 * p[4] - p[2] - p[5]) * (1.0 / 12);
        const double q2 = (p[1] - 5 * p[2] + 13 * p[3] + 3 * p[4]) * (1.0 / 12);
        const double q3 = (13 * p[1] - 3 * p[0] - 23 * p[2] + 25 * p[3]) * (1.0 / 12);
        const double r0 = tau * fm::rcp(b0 + WENO_EPS), r1 = tau * fm::rcp(b1 + WENO_EPS), r2 = tau * fm::rcp(b2 + WENO_EPS), r3 = tau * fm::rcp(b3 + WENO_EPS);
        const double a0 = (4.0 / 35) * (1 + r0 * r0);
        const double a1 = (18.0 / 35) * (1 + r1 * r1);
        const double a2 = (12.0 / 35) * (1 + r2 * r2);
        const double a3 = (1.0 / 35) * (1 + r3 * r3);
        return (a0 * q0 + a1 * q1 + a2 * q2 + a3 * q3) * fm::rcp(a0 + a1 + a2 + a3);
    }
}

// ---- weight_dtype f32 (csi_set_weno_weight_dtype; oracle/csi_oracle.c weno*_f32, whose statement of the ASSUMED upstream semantics
// -- newer Oceananigans versions carry a second float type FT2 = Float32 for a WENO scheme's smoothness / weight arithmetic -- this
// follows): stencil values converted to float, indicators, tau, ratios, unnormalised weights and their sum in float (same
// expressions, same order, this unit is compiled without contraction; fp32 division is correctly rounded by default), candidates in
// double, result (sum alpha_s q_s) / (sum alpha_s) in double.  STRICT: that, bit for bit.  FAST: the same float weights -- they are
// a dozen full-rate instructions, nothing to gain -- with the double part contracted and the last division a reciprocal.
#define WENO_EPS_F 1e-8f
template <bool FAST>
__device__ __forceinline__ double weno3_w32(const double* p) {
    float f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = (float)p[k];
    const float b0 = f[1] * (f[1] - 2 * f[2]) + f[2] * f[2];
    const float b1 = f[0] * (f[0] - 2 * f[1]) + f[1] * f[1];
    const float tau = fabsf(b0 - b1);
    const float r0 = tau / (b0 + WENO_EPS_F), r1 = tau / (b1 + WENO_EPS_F);
    const float a0 = (float)(2.0 / 3) * (1 + r0 * r0);
    const float a1 = (float)(1.0 / 3) * (1 + r1 * r1);
    const float s = a0 + a1;
    if (FAST) {
#pragma clang fp contract(fast)
        const double q0 = 0.5 * (p[1] + p[2]);
        const double q1 = 0.5 * (3 * p[1] - p[0]);
        return ((double)a0 * q0 + (double)a1 * q1) * fm::rcp((double)s);
    }
    const double q0 = (p[1] + p[2]) / 2;
    const double q1 = (-p[0] + 3 * p[1]) / 2;
    return ((double)a0 * q0 + (double)a1 * q1) / (double)s;
}
template <bool FAST>
__device__ __forceinline__ double weno5_w32(const double* p) {
    float f[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) f[k] = (float)p[k];
    const float b0 = (f[2] * (10 * f[2] - 31 * f[3] + 11 * f[4]) + f[3] * (25 * f[3] - 19 * f[4]) + f[4] * (4 * f[4])) / 3;
    const float b1 = (f[1] * (4 * f[1] - 13 * f[2] + 5 * f[3]) + f[2] * (13 * f[2] - 13 * f[3]) + f[3] * (4 * f[3])) / 3;
    const float b2 = (f[0] * (4 * f[0] - 19 * f[1] + 11 * f[2]) + f[1] * (25 * f[1] - 31 * f[2]) + f[2] * (10 * f[2])) / 3;
    const float tau = fabsf(b0 - b2);
    const float r0 = tau / (b0 + WENO_EPS_F), r1 = tau / (b1 + WENO_EPS_F), r2 = tau / (b2 + WENO_EPS_F);
    const float a0 = (float)(3.0 / 10) * (1 + r0 * r0);
    const float a1 = (float)(3.0 / 5) * (1 + r1 * r1);
    const float a2 = (float)(1.0 / 10) * (1 + r2 * r2);
    const float s = a0 + a1 + a2;
    if (FAST) {
#pragma clang fp contract(fast)
        const double q0 = (2 * p[2] + 5 * p[3] - p[4]) * (1.0 / 6);
        const double q1 = (5 * p[2] + 2 * p[3] - p[1]) * (1.0 / 6);
        const double q2 = (2 * p[0] - 7 * p[1] + 11 * p[2]) * (1.0 / 6);
        return ((double)a0 * q0 + (double)a1 * q1 + (double)a2 * q2) * fm::rcp((double)s);
    }
    const double q0 = (2 * p[2] + 5 * p[3] - p[4]) / 6;
    const double q1 = (-p[1] + 5 * p[2] + 2 * p[3]) / 6;
    const double q2 = (2 * p[0] - 7 * p[1] + 11 * p[2]) / 6;
    return ((double)a0 * q0 + (double)a1 * q1 + (double)a2 * q2) / (double)s;
}
template <bool FAST>
__device__ __forceinline__ double weno7_w32(const double* p) {
    float f[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) f[k] = (float)p[k];
    const float b0 = f[3] * (2.107f * f[3] - 9.402f * f[4] + 7.042f * f[5] - 1.854f * f[6]) +
                     f[4] * (11.003f * f[4] - 17.246f * f[5] + 4.642f * f[6]) + f[5] * (7.043f * f[5] - 3.882f * f[6]) + f[6] * (0.547f * f[6]);
    const float b1 = f[2] * (0.547f * f[2] - 2.522f * f[3] + 1.922f * f[4] - 0.494f * f[5]) +
                     f[3] * (3.443f * f[3] - 5.966f * f[4] + 1.602f * f[5]) + f[4] * (2.843f * f[4] - 1.642f * f[5]) + f[5] * (0.267f * f[5]);
    const float b2 = f[1] * (0.267f * f[1] - 1.642f * f[2] + 1.602f * f[3] - 0.494f * f[4]) +
                     f[2] * (2.843f * f[2] - 5.966f * f[3] + 1.922f * f[4]) + f[3] * (3.443f * f[3] - 2.522f * f[4]) + f[4] * (0.547f * f[4]);
    const float b3 = f[0] * (0.547f * f[0] - 3.882f * f[1] + 4.642f * f[2] - 1.854f * f[3]) +
                     f[1] * (7.043f * f[1] - 17.246f * f[2] + 7.042f * f[3]) + f[2] * (11.003f * f[2] - 9.402f * f[3]) + f[3] * (2.107f * f[3]);
    const float tau = fabsf(b0 + 3 * b1 - 3 * b2 - b3);
    const float r0 = tau / (b0 + WENO_EPS_F), r1 = tau / (b1 + WENO_EPS_F), r2 = tau / (b2 + WENO_EPS_F), r3 = tau / (b3 + WENO_EPS_F);
    const float a0 = (float)(4.0 / 35) * (1 + r0 * r0);
    const float a1 = (float)(18.0 / 35) * (1 + r1 * r1);
    const float a2 = (float)(12.0 / 35) * (1 + r2 * r2);
    const float a3 = (float)(1.0 / 35) * (1 + r3 * r3);
    const float s = a0 + a1 + a2 + a3;
    if (FAST) {
#pragma clang fp contract(fast)
        const double q0 = (3 * p[3] + 13 * p[4] - 5 * p[5] + p[6]) * (1.0 / 12);
        const double q1 = (7 * p[3] + 7 * p[4] - p[2] - p[5]) * (1.0 / 12);
        const double q2 = (p[1] - 5 * p[2] + 13 * p[3] + 3 * p[4]) * (1.0 / 12);
        const double q3 = (13 * p[1] - 3 * p[0] - 23 * p[2] + 25 * p[3]) * (1.0 / 12);
        return ((double)a0 * q0 + (double)a1 * q1 + (double)a2 * q2 + (double)a3 * q3) * fm::rcp((double)s);
    }
    const double q0 = (3 * p[3] + 13 * p[4] - 5 * p[5] + p[6]) / 12;
    const double q1 = (-p[2] + 7 * p[3] + 7 * p[4] - p[5]) / 12;
    const double q2 = (p[1] - 5 * p[2] + 13 * p[3] + 3 * p[4]) / 12;
    const double q3 = (-3 * p[0] + 13 * p[1] - 23 * p[2] + 25 * p[3]) / 12;
    return ((double)a0 * q0 + (double)a1 * q1 + (double)a2 * q2 + (double)a3 * q3) / (double)s;
}

// Boundary-order reduction next to walls (upstream topologically_conditional_interpolation, recalled -- SURVEY.md
// App. B; same rule as oracle/csi_oracle.c::reduced_buffer): the scheme with buffer B (order 2B-1) is used at face
// idx only if its biased stencil stays inside the domain, else the buffer scheme of order 2B-3, down to upwind 1.
__device__ __forceinline__ int reduced_buffer(int B, int idx, int N, bool left, bool wall_lo, bool wall_hi) {
    while (B > 1) {
        const bool lo_ok = !wall_lo || idx >= (left ? B + 1 : B);
        const bool hi_ok = !wall_hi || idx <= (left ? N + 2 - B : N + 1 - B);
        if (lo_ok && hi_ok) break;
        --B;
    }
    return B;
}

// Immersed boundaries (upstream immersed reconstruction, recalled; oracle/csi_oracle.c::reduced_buffer_immersed):
// the scheme with buffer B needs the 2B cells idx-B .. idx+B-1 around the face to be active (not immersed, not
// beyond a wall); here as distances: dl = cells below the face up to the first inactive one, dr likewise above.
__device__ __forceinline__ int reduced_buffer_immersed(const GridDev& g, int B, int i, int j, bool along_y) {
    int dl = B, dr = B;
    for (int k = B; k >= 1; --k) {
        if (along_y ? inactive_cell(g, i, j - k) : inactive_cell(g, i - k, j)) dl = k - 1;
        if (along_y ? inactive_cell(g, i, j + k - 1) : inactive_cell(g, i + k - 1, j)) dr = k - 1;
    }
    const int b = dl < dr ? dl : dr;
    return b < 1 ? 1 : b;
}

// reconstruct at a face from the line of values through `base` (cell on the high side of the
// face); st = element stride of the line; left bias (vel > 0): upwind cell is base - st.
// B: buffer of the scheme to use at this face (after the boundary-order reduction).
template <int SCHEME, bool FAST = false, bool W32 = false>
__device__ __forceinline__ double reconstruct(const double* base, long st, bool left, int B) {
    const double* up = left ? base - st : base;
    const long s = left ? st : -st;
    if (SCHEME == 1) return up[0];
    constexpr bool WENO = SCHEME > 0;
    if (B == 1) return up[0];
    if (B == 2) {
        double p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = up[(k - 1) * s];
        return WENO ? (W32 ? weno3_w32<FAST>(p) : (FAST ? weno3_fast(p) : weno3(p))) : (FAST ? upwind3_fast(p) : upwind3(p));
    }
    if (B == 3 || SCHEME != 7) {
        double p[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) p[k] = up[(k - 2) * s];
        return WENO ? (W32 ? weno5_w32<FAST>(p) : (FAST ? weno5_fast(p) : weno5(p))) : (FAST ? upwind5_fast(p) : upwind5(p));
    }
    double p[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) p[k] = up[(k - 3) * s];
    return W32 ? weno7_w32<FAST>(p) : (FAST ? weno7_fast(p) : weno7(p));
}
// buffer at face (i, j) of the x / y direction: immersed grid -> the immersed rule (it covers the walls: cells beyond
// them are inactive); else the topological rule next to walls; else the full scheme
template <int SCHEME>
__device__ __forceinline__ int buffer_at(const GridDev& g, int i, int j, bool along_y, bool left) {
    constexpr int B0 = SCHEME == 7 ? 4 : (SCHEME == 1 ? 1 : ((SCHEME == 3 || SCHEME == -3) ? 2 : 3));   // order 2B - 1
    if (SCHEME == 1) return 1;
    if (g.has_mask) return reduced_buffer_immersed(g, B0, i, j, along_y);
    const bool wl = (along_y ? g.ylo : g.xlo) == SIDE_WALL, wh = (along_y ? g.yhi : g.xhi) == SIDE_WALL;
    if (!(wl | wh)) return B0;
    return reduced_buffer(B0, along_y ? j : i, along_y ? g.Ny : g.Nx, left, wl, wh);
}

}  // namespace adv
}  // namespace csi
