// fast_math_probe.hip -- TEST INFRASTRUCTURE, not part of libcsi_hip.so.
//
// Runs every function of csrc/evp_fast_math.h element-wise over arrays so that tests/test_gpu_fast_math.py can compare each one with a
// high-precision evaluation of the reference's formulas (tests/fast_math_ref.py) and the "same bits" forms with each other.  The header
// is included unchanged and this file is built by the `probe` target of csrc/Makefile with exactly the flags of evp_fast.o
// ($(COMMON) $(STRICT): no contraction), so the arithmetic here is the arithmetic of the FAST kernels.
//
// Layout: structure of arrays.  Input k of element i is in[k * n + i], output k is out[k * n + i]; every thread handles one element
// and checks i < n; no shared memory, no atomics.  The host entry points take device pointers, n and a stream and return the
// hipError_t of the launch.
#include "evp_fast_math.h"

namespace fm = csi::fm;

namespace {

constexpr int BLOCK = 256;
inline dim3 blocks_for(long n) { return dim3((unsigned)((n + BLOCK - 1) / BLOCK)); }

// x -> raw seeds v_rcp_f64 / v_rsq_f64, rcp, rsqrt, sqrt_fast, sqrt_rsqrt's (s, rs)
__global__ void __launch_bounds__(BLOCK) k_primitives(const double* __restrict__ x, double* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double s, rs;
    fm::sqrt_rsqrt(v, s, rs);
    out[0 * n + i] = __builtin_amdgcn_rcp(v);
    out[1 * n + i] = __builtin_amdgcn_rsq(v);
    out[2 * n + i] = fm::rcp(v);
    out[3 * n + i] = fm::rsqrt(v);
    out[4 * n + i] = fm::sqrt_fast(v);
    out[5 * n + i] = s;
    out[6 * n + i] = rs;
}

// inputs in the argument order of stress_update_r (17 rows): e11c e22c e12f e11f e22f e12c Pc Pf mc mf rmc rmf hkc hkf s11 s22 s12
// (stress_update_s reads the same rows as e11c e22c E12f S11f S22f y2 Pc XP mc M4 rmc rM4 hkc hkf4 s11 s22 s12; stress_update ignores
// rmc, rmf).  which: 0 stress_update_r, 1 stress_update_s, 2 stress_update.  Outputs: s11 s22 s12 alpha zc2 zf2 xc rDc.
__global__ void __launch_bounds__(BLOCK) k_stress(int which, fm::StressConst k, const double* __restrict__ in, double* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double a[17];
    for (int q = 0; q < 17; ++q) a[q] = in[q * n + i];
    fm::StressOut o;
    if (which == 0)
        o = fm::stress_update_r(k, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15], a[16]);
    else if (which == 1)
        o = fm::stress_update_s(k, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15], a[16]);
    else
        o = fm::stress_update(k, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[12], a[13], a[14], a[15], a[16]);
    out[0 * n + i] = o.s11; out[1 * n + i] = o.s22; out[2 * n + i] = o.s12; out[3 * n + i] = o.alpha;
    out[4 * n + i] = o.zc2; out[5 * n + i] = o.zf2; out[6 * n + i] = o.xc; out[7 * n + i] = o.rDc;
}

// inputs (6 rows): tau rhoCd we webar w wbar.  Outputs: ex, im of ext_stress(kind, ...) and ex, im of ext_stress_rest(rhoCd, w, wbar).
__global__ void __launch_bounds__(BLOCK) k_ext_stress(int kind, const double* __restrict__ in, double* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double ex, im, exr, imr;
    fm::ext_stress(kind, in[0 * n + i], in[1 * n + i], in[2 * n + i], in[3 * n + i], in[4 * n + i], in[5 * n + i], ex, im);
    fm::ext_stress_rest(in[1 * n + i], in[4 * n + i], in[5 * n + i], exr, imr);
    out[0 * n + i] = ex; out[1 * n + i] = im; out[2 * n + i] = exr; out[3 * n + i] = imr;
}

// inputs (16 rows): w wn m_a m_b a_a a_b al_a al_b div cor ext imt exb imb peripheral(!= 0) wf.  The forms that take averages or sums
// read them from m_a, a_a, al_a.  which: 0 vel_update_avg, 1 vel_update_avg_fd, 2 vel_update_sum, 3 vel_update_sum_fd, 4 vel_update,
// 5 vel_update_fd.  One output.
__global__ void __launch_bounds__(BLOCK) k_vel(int which, fm::VelConst k, const double* __restrict__ in, double* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double a[16];
    for (int q = 0; q < 16; ++q) a[q] = in[q * n + i];
    const bool per = a[14] != 0.0;
    double r;
    switch (which) {
        case 0: r = fm::vel_update_avg(k, a[0], a[1], a[2], a[4], a[6], a[8], a[9], a[10], a[11], a[12], a[13], per); break;
        case 1: r = fm::vel_update_avg_fd(k, a[0], a[1], a[2], a[4], a[6], a[8], a[9], a[10], a[11], a[12], a[13], per, a[15]); break;
        case 2: r = fm::vel_update_sum(k, a[0], a[1], a[2], a[4], a[6], a[8], a[9], a[10], a[11], a[12], a[13], per); break;
        case 3: r = fm::vel_update_sum_fd(k, a[0], a[1], a[2], a[4], a[6], a[8], a[9], a[10], a[11], a[12], a[13], per, a[15]); break;
        case 4: r = fm::vel_update(k, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], per); break;
        default: r = fm::vel_update_fd(k, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], per, a[15]); break;
    }
    out[i] = r;
}

// inputs (4 rows) a b c d.  Outputs: avg4(a, b, c, d); quarter(sum2(a, b), sum2(c, d)); the nested halvings avg2(avg2(a, b), avg2(c, d)).
__global__ void __launch_bounds__(BLOCK) k_avg(const double* __restrict__ in, double* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double a = in[0 * n + i], b = in[1 * n + i], c = in[2 * n + i], d = in[3 * n + i];
    out[0 * n + i] = fm::avg4(a, b, c, d);
    out[1 * n + i] = fm::quarter(fm::sum2(a, b), fm::sum2(c, d));
    out[2 * n + i] = fm::avg2(fm::avg2(a, b), fm::avg2(c, d));
}

// inputs (10 rows) p0 .. p9, handed to the functions in their own argument order (full_strain_corner* read p0 .. p6).
// Outputs: full_strain_corner, full_strain_corner8, full_div1, full_div1_x2, full_div2, full_div2_x2.
__global__ void __launch_bounds__(BLOCK) k_full(const double* __restrict__ in, double* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double p[10];
    for (int q = 0; q < 10; ++q) p[q] = in[q * n + i];
    out[0 * n + i] = fm::full_strain_corner(p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
    out[1 * n + i] = fm::full_strain_corner8(p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
    out[2 * n + i] = fm::full_div1(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]);
    out[3 * n + i] = fm::full_div1_x2(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]);
    out[4 * n + i] = fm::full_div2(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]);
    out[5 * n + i] = fm::full_div2_x2(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]);
}

fm::StressConst stress_const(const double* c) {
    // c: em2 Dmin amin amax hk1 pressure_kind -- everything else is derived the way csi_launch.hip's fast_coef derives it
    fm::StressConst k;
    k.em2 = c[0]; k.Dmin = c[1]; k.Dmin2 = c[1] * c[1]; k.rDmin = 1.0 / c[1];
    k.amin = c[2]; k.amax = c[3]; k.amin2 = c[2] * c[2]; k.amax2 = c[3] * c[3]; k.ramin = 1.0 / c[2]; k.ramax = 1.0 / c[3];
    k.hk1 = c[4];
    k.pressure_kind = (int)c[5];
    k.em2_8 = 0.125 * c[0]; k.Dmin2_16 = 16.0 * k.Dmin2;
    return k;
}

int launched() { return (int)hipGetLastError(); }

}  // namespace

extern "C" {

int fmp_primitives(const double* x, double* out, long n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_primitives, blocks_for(n), dim3(BLOCK), 0, (hipStream_t)stream, x, out, n);
    return launched();
}
int fmp_stress(int which, const double* consts, const double* in, double* out, long n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_stress, blocks_for(n), dim3(BLOCK), 0, (hipStream_t)stream, which, stress_const(consts), in, out, n);
    return launched();
}
int fmp_ext_stress(int kind, const double* in, double* out, long n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_ext_stress, blocks_for(n), dim3(BLOCK), 0, (hipStream_t)stream, kind, in, out, n);
    return launched();
}
// consts: dt rdt min_mass min_conc (fcor, has_cor are not read by the functions)
int fmp_vel(int which, const double* consts, const double* in, double* out, long n, void* stream) {
    if (n <= 0) return 0;
    fm::VelConst k;
    k.dt = consts[0]; k.rdt = consts[1]; k.fcor = 0.0; k.min_mass = consts[2]; k.min_conc = consts[3]; k.has_cor = 0;
    hipLaunchKernelGGL(k_vel, blocks_for(n), dim3(BLOCK), 0, (hipStream_t)stream, which, k, in, out, n);
    return launched();
}
int fmp_avg(const double* in, double* out, long n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_avg, blocks_for(n), dim3(BLOCK), 0, (hipStream_t)stream, in, out, n);
    return launched();
}
int fmp_full(const double* in, double* out, long n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_full, blocks_for(n), dim3(BLOCK), 0, (hipStream_t)stream, in, out, n);
    return launched();
}

}  // extern "C"
