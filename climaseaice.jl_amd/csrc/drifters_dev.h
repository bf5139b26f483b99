// drifters_dev.h -- the rule of the Lagrangian ice drifters (include/csi.h, "Lagrangian ice drifters"): locate, weights, norm, rate,
// one sub-step.  A host-and-device header without a HIP type in it: drifters.hip instantiates it on the device over the bound fields
// and the grid's metrics, csi_drifters.hip calls locate() on the host (csi_drifters_locate), and tests/drifters_host.cpp compiles the
// whole sub-step with g++ over plain arrays, so that the CPU suite holds this one C statement against tests/drifters_ref.py.
//
// The fields are reached through a Source type F with
//     void F::load_u(int i, int j, double* num, double* den) const      the four u values and dx^fc at (i, j), (i + 1, j), (i, j + 1),
//                                                                       (i + 1, j + 1), in this order
//     void F::load_v(int i, int j, double* num, double* den) const      the same of v and dy^cf
//     bool F::land(int i, int j) const                                  the containing cell is inactive (false without a mask)
// so that every load of one rate evaluation is issued before the first value is used (the idiom of momentum_dev.h): sixteen loads
// (eight on a uniform grid), then eight divisions, then the two bilinear forms on registers.
// Every expression is in the header's order; the units that include this file are compiled without contraction.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DRIFT_FN __host__ __device__ __forceinline__
#else
#define DRIFT_FN inline
#endif

namespace csi {
namespace drift {

enum : int { CLAMPED_X = 1, CLAMPED_Y = 2, HELD = 4, LOST = 8, INACTIVE = 16 };

struct Dom {
    int Nx, Ny;
    int periodic_x, periodic_y;   // 1: Periodic, 0: Bounded
};

// the stencils of one point: A (u / dx^fc) at columns ia, ia + 1 and rows ja, ja + 1 with weights sx, sy; B (v / dy^cf) at ib, jb with
// rx, ry; the containing cell (ic, jc)
struct Stencil {
    int ia, ja, ib, jb, ic, jc;
    double sx, sy, rx, ry;
};

// fmin(fmax(floor(x), lo), hi): clamped as a double, BEFORE the conversion, so that no x -- NaN, +-Inf -- can form an index outside
// [lo, hi] (fmax / fmin return the other argument for a NaN)
DRIFT_FN double floor_clamped(double x, double lo, double hi) { return fmin(fmax(floor(x), lo), hi); }

DRIFT_FN bool finite_(double x) { return x - x == 0.0; }      // (false for NaN and +-Inf; no library call on either side)

DRIFT_FN Stencil locate(int Nx, int Ny, double xi, double eta) {
    Stencil s;
    const double fx = floor_clamped(xi, 0.0, (double)(Nx - 1));
    const double t = eta - 0.5;
    const double fy = floor_clamped(t, -1.0, (double)(Ny - 1));
    s.sx = xi - fx;
    s.sy = t - fy;
    s.ia = (int)fx + 1;
    s.ja = (int)fy + 1;
    const double gy = floor_clamped(eta, 0.0, (double)(Ny - 1));
    const double q = xi - 0.5;
    const double gx = floor_clamped(q, -1.0, (double)(Nx - 1));
    s.ry = eta - gy;
    s.rx = q - gx;
    s.ib = (int)gx + 1;
    s.jb = (int)gy + 1;
    s.ic = (int)fx + 1;
    s.jc = (int)gy + 1;
    return s;
}

// (1 - wb) * ((1 - wa) * f00 + wa * f10) + wb * ((1 - wa) * f01 + wa * f11): wa the weight along the direction in which f00 -> f10
DRIFT_FN double bilinear(double wa, double wb, double f00, double f10, double f01, double f11) {
    return (1 - wb) * ((1 - wa) * f00 + wa * f10) + wb * ((1 - wa) * f01 + wa * f11);
}

DRIFT_FN double norm(double x, int N, int periodic, int bit, int& status) {
    const double n = (double)N;
    if (periodic) {
        double r = x - n * floor(x / n);
        if (r >= n || r < 0) r = 0.0;
        return r;
    }
    const double r = x < 0 ? 0.0 : (x > n ? n : x);
    if (r != x && x == x) status |= bit;
    return r;
}

template <class F>
DRIFT_FN void rate(const F& f, const Dom& d, double xi, double eta, double& a, double& b) {
    const Stencil s = locate(d.Nx, d.Ny, xi, eta);
    double un[4], ud[4], vn[4], vd[4];
    f.load_u(s.ia, s.ja, un, ud);
    f.load_v(s.ib, s.jb, vn, vd);
    const double A00 = un[0] / ud[0], A10 = un[1] / ud[1], A01 = un[2] / ud[2], A11 = un[3] / ud[3];
    const double B00 = vn[0] / vd[0], B10 = vn[1] / vd[1], B01 = vn[2] / vd[2], B11 = vn[3] / vd[3];
    a = bilinear(s.sx, s.sy, A00, A10, A01, A11);
    b = bilinear(s.ry, s.rx, B00, B01, B10, B11);
}

// One sub-step of an ACTIVE drifter (finite xi, eta).  Returns false when the drifter is lost: (xi, eta) = (NaN, NaN), nothing more
// is to be done for it.
template <class F>
DRIFT_FN bool substep(const F& f, const Dom& d, double tau, double& xi, double& eta, int& status) {
    double a1, b1, a2, b2;
    rate(f, d, xi, eta, a1, b1);
    const double half = tau / 2;
    const double xm = norm(xi + half * a1, d.Nx, d.periodic_x, CLAMPED_X, status);
    const double ym = norm(eta + half * b1, d.Ny, d.periodic_y, CLAMPED_Y, status);
    rate(f, d, xm, ym, a2, b2);
    const double X = xi + tau * a2, Y = eta + tau * b2;
    const double xn = norm(X, d.Nx, d.periodic_x, CLAMPED_X, status);
    const double yn = norm(Y, d.Ny, d.periodic_y, CLAMPED_Y, status);
    if (!(finite_(X) && finite_(Y) && finite_(xn) && finite_(yn))) {
        xi = eta = NAN;
        status |= LOST;
        return false;
    }
    const int ic = (int)floor_clamped(xn, 0.0, (double)(d.Nx - 1)) + 1, jc = (int)floor_clamped(yn, 0.0, (double)(d.Ny - 1)) + 1;
    if (f.land(ic, jc)) {
        status |= HELD;
        return true;
    }
    xi = xn;
    eta = yn;
    return true;
}

}  // namespace drift
}  // namespace csi
