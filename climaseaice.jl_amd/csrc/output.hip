// output.hip -- device-side output: time averages and packed records (include/csi.h: csi_output_accumulate / csi_output_snapshot).
//
//   k_output_accumulate   acc = acc + (x * w) for every AVERAGED field of an output set, one launch: the product first, then the sum
//   k_output_pack         the record of every field of the set, one launch, into a device staging slot: x (snapshot) or acc / W (one
//                         IEEE division; acc is then set to +0.0), fill_value in inactive cells of a masked (Center, Center) field,
//                         converted to fp32 (round to nearest even) where the field asks for it
// The table of descriptors (at most sixteen) travels by value as the kernel argument; the grid runs over (column block, row block,
// field), fields smaller than the largest leave their surplus blocks at once.  Only the INTERIOR of a bound array is read: element
// e of row j of a field is src[e + j * lds], src the first interior element -- halo elements are never touched.  acc and the
// record are dense row-major (ny, nx) arrays.
//
// Streaming kernels: per element 8 B in and 4 or 8 B out (pack), 16 B in and 8 B out (accumulate), no reuse.  A thread owns four
// consecutive elements in each of kRows rows, kBy rows apart; the four start at a multiple of four counted from the 16-byte boundary
// at or below the start of the row it READS (the bound array's row, or acc's for an averaged field), so the loads are two 16-byte
// accesses; the stores are 16-byte accesses -- two for fp64, one for fp32 -- wherever the destination address of the four is
// 16-byte aligned as well (interior start, leading dimension and record row all aligned: even halos and row lengths), and single
// elements otherwise (odd halos, the wider Face rows of a Bounded side).  The first / last four of a row that starts / ends
// inside them are single elements, each guarded by its own bounds test.  All loads of a thread's rows are issued before the first
// value is used.  No LDS, no atomics, no scratch.  Compiled without contraction; STRICT and FAST run this one code.
#include "csi_dev.h"
#include "csi_kernels.h"
#include <cstdint>

namespace csi {

namespace {

constexpr int kRows = 2;                 // rows per thread
constexpr int kBx = 64, kBy = 4;         // threads of a block: 256 columns x (4 * kRows) rows

typedef double d2_t __attribute__((ext_vector_type(2)));      // (native vectors: ONE 16-byte access each)
typedef float f4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// 0 / 1: elements between the 16-byte boundary at or below p and p
__device__ __forceinline__ int head_of(const double* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 3) & 1); }

// elements [e0, e0 + 3] of a row of n (on: the row exists); two 16-byte loads where all four exist and the address allows it
__device__ __forceinline__ void load4(const double* row, int e0, int n, bool on, double (&v)[4]) {
    const double* p = row + e0;
    if (on & (e0 >= 0) & (e0 + 3 < n) & aligned16(p)) {
        const d2_t a = *reinterpret_cast<const d2_t*>(p), b = *reinterpret_cast<const d2_t*>(p + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = 0.0;
            if (on & (e0 + k >= 0) & (e0 + k < n)) v[k] = p[k];
        }
    }
}

__device__ __forceinline__ void store4(double* row, int e0, int n, bool on, const double (&v)[4]) {
    double* p = row + e0;
    if (on & (e0 >= 0) & (e0 + 3 < n) & aligned16(p)) {
        const d2_t a = {v[0], v[1]}, b = {v[2], v[3]};
        *reinterpret_cast<d2_t*>(p) = a;
        *reinterpret_cast<d2_t*>(p + 2) = b;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (on & (e0 + k >= 0) & (e0 + k < n)) p[k] = v[k];
    }
}

__device__ __forceinline__ void store4(float* row, int e0, int n, bool on, const double (&v)[4]) {
    float* p = row + e0;
    // (a plain conversion: round to nearest even, overflow to +-Inf, subnormal results kept)
    const f4_t o = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    if (on & (e0 >= 0) & (e0 + 3 < n) & aligned16(p)) {
        *reinterpret_cast<f4_t*>(p) = o;
    } else {
        if (on & (e0 >= 0) & (e0 < n)) p[0] = o.x;
        if (on & (e0 + 1 >= 0) & (e0 + 1 < n)) p[1] = o.y;
        if (on & (e0 + 2 >= 0) & (e0 + 2 < n)) p[2] = o.z;
        if (on & (e0 + 3 >= 0) & (e0 + 3 < n)) p[3] = o.w;
    }
}

}  // namespace

__global__ void __launch_bounds__(kBx * kBy) k_output_accumulate(OutputTable T) {
    const OutputDesc& D = T.d[blockIdx.z];
    const int quad = (int)(blockIdx.x * kBx + threadIdx.x);
    const int jb = (int)(blockIdx.y * (kBy * kRows) + threadIdx.y);
    if (4 * quad - 1 >= D.nx || jb >= D.ny) return;
    double x[kRows][4], a[kRows][4];
    int e0[kRows];
    bool on[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int j = jb + r * kBy;
        on[r] = j < D.ny;
        const long jj = on[r] ? j : 0;
        const double* row = D.src + jj * D.lds;
        e0[r] = 4 * quad - head_of(row);
        load4(row, e0[r], D.nx, on[r], x[r]);
        load4(D.acc + jj * D.nx, e0[r], D.nx, on[r], a[r]);
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const long jj = on[r] ? jb + r * kBy : 0;
        double o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = a[r][k] + (x[r][k] * T.w);
        store4(D.acc + jj * D.nx, e0[r], D.nx, on[r], o);
    }
}

__global__ void __launch_bounds__(kBx * kBy) k_output_pack(OutputTable T) {
    const OutputDesc& D = T.d[blockIdx.z];
    const int quad = (int)(blockIdx.x * kBx + threadIdx.x);
    const int jb = (int)(blockIdx.y * (kBy * kRows) + threadIdx.y);
    if (4 * quad - 1 >= D.nx || jb >= D.ny) return;
    // an averaged field reads (and clears) its accumulator, a snapshot field the bound array
    const double* in = D.averaged ? D.acc : D.src;
    const long ldin = D.averaged ? (long)D.nx : D.lds;
    const bool masked = D.masked && T.mask != nullptr;
    double x[kRows][4];
    unsigned char m[kRows][4];
    int e0[kRows];
    bool on[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int j = jb + r * kBy;
        on[r] = j < D.ny;
        const long jj = on[r] ? j : 0;
        const double* row = in + jj * ldin;
        e0[r] = 4 * quad - head_of(row);
        load4(row, e0[r], D.nx, on[r], x[r]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m[r][k] = 1;
            if (masked & on[r] & (e0[r] + k >= 0) & (e0[r] + k < D.nx)) m[r][k] = T.mask[(e0[r] + k) + jj * T.mask_ld];
        }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const long jj = on[r] ? jb + r * kBy : 0;
        double o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double v = D.averaged ? x[r][k] / T.w : x[r][k];
            o[k] = m[r][k] ? v : D.fill;
        }
        if (D.f32) store4(reinterpret_cast<float*>(D.dst) + jj * D.nx, e0[r], D.nx, on[r], o);
        else store4(reinterpret_cast<double*>(D.dst) + jj * D.nx, e0[r], D.nx, on[r], o);
        if (D.averaged) {
            const double z[4] = {0.0, 0.0, 0.0, 0.0};
            store4(D.acc + jj * D.nx, e0[r], D.nx, on[r], z);
        }
    }
}

static dim3 output_grid(const OutputTable& T) {
    int nx = 0, ny = 0;
    for (int k = 0; k < T.n; ++k) {
        nx = T.d[k].nx > nx ? T.d[k].nx : nx;
        ny = T.d[k].ny > ny ? T.d[k].ny : ny;
    }
    const int quads = nx / 4 + 1;                        // a row that starts odd has one more
    return dim3((unsigned)((quads + kBx - 1) / kBx), (unsigned)((ny + kBy * kRows - 1) / (kBy * kRows)), (unsigned)T.n);
}

void launch_output_accumulate(const OutputTable& T, hipStream_t s) {
    if (T.n <= 0) return;
    hipLaunchKernelGGL(k_output_accumulate, output_grid(T), dim3(kBx, kBy), 0, s, T);
}

void launch_output_pack(const OutputTable& T, hipStream_t s) {
    if (T.n <= 0) return;
    hipLaunchKernelGGL(k_output_pack, output_grid(T), dim3(kBx, kBy), 0, s, T);
}

}  // namespace csi
