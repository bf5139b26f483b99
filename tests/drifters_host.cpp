// drifters_host.cpp -- csrc/drifters_dev.h compiled for the host (g++, no contraction) over plain arrays; test infrastructure, not part
// of libcsi_hip.so.  Two uses:
//   a shared library (tests/test_drifters_ref.py loads it with ctypes): drifters_host_advance runs the header's sub-step, so that the
//   CPU suite holds the one C statement of the rule against tests/drifters_ref.py bit for bit;
//   with -DDRIFTERS_HOST_MAIN a stand-alone program that runs a table of edge positions -- on and beyond every boundary, NaN, +-Inf,
//   1e300 -- on 37 x 29 in the three topologies, built with -fsanitize=address,undefined,float-cast-overflow: an index outside the
//   parents, or a conversion of an out-of-range double, ends it with a report and a non-zero status.
// Arrays as in the library: element (i, j) of a parent with row stride ld at parent[(i + Hx - 1) + (j + Hy - 1) * ld]; the metric planes
// dxfc, dycf likewise with stride ldm; the mask: Ny x Nx bytes of the interior (NULL: none).
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <limits>
#include <vector>

#include "drifters_dev.h"

namespace {

struct HostSource {
    const double *u, *v, *dxfc, *dycf;      // element (0, 0)
    long ldu, ldv, ldm;
    const uint8_t* mask;                    // cell (1, 1)
    int Nx;
    static void four(const double* p, long ld, int i, int j, double* out) {
        for (int k = 0; k < 4; ++k) out[k] = p[(i + (k & 1)) + (long)(j + (k >> 1)) * ld];
    }
    void load_u(int i, int j, double* num, double* den) const { four(u, ldu, i, j, num); four(dxfc, ldm, i, j, den); }
    void load_v(int i, int j, double* num, double* den) const { four(v, ldv, i, j, num); four(dycf, ldm, i, j, den); }
    bool land(int i, int j) const { return mask && mask[(i - 1) + (long)(j - 1) * Nx] == 0; }
};

}  // namespace

extern "C" int drifters_host_advance(int Nx, int Ny, int Hx, int Hy, int periodic_x, int periodic_y, const double* u, long ldu, const double* v,
                                     long ldv, const double* dxfc, const double* dycf, long ldm, const uint8_t* mask, long n, double* xi,
                                     double* eta, int32_t* status, double tau, int m) {
    using namespace csi::drift;
    const long o = Hx - 1;
    const HostSource src{u + o + (long)(Hy - 1) * ldu, v + o + (long)(Hy - 1) * ldv, dxfc + o + (long)(Hy - 1) * ldm, dycf + o + (long)(Hy - 1) * ldm,
                         ldu, ldv, ldm, mask, Nx};
    const Dom dom{Nx, Ny, periodic_x, periodic_y};
    for (long q = 0; q < n; ++q) {
        double x = xi[q], y = eta[q];
        if (!(finite_(x) && finite_(y))) {
            status[q] = INACTIVE;
            continue;
        }
        int st = 0;
        for (int s = 0; s < m; ++s)
            if (!substep(src, dom, tau, x, y, st)) break;
        xi[q] = x;
        eta[q] = y;
        status[q] = st;
    }
    return 0;
}

#ifdef DRIFTERS_HOST_MAIN
int main() {
    const int Nx = 37, Ny = 29, Hx = 3, Hy = 3;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const double ex[] = {0.0, 1.0, 12.0, 0.5, 7.25, Nx - std::ldexp((double)Nx, -52), (double)Nx, Nx - 0.5, Nx - 1.0, -1e-17, Nx + 1e-13, nan, inf, -inf, 1e300, -1e300};
    const double ey[] = {0.0, 0.25, 0.4999999999999999, 0.5, 3.75, Ny - 0.5, Ny - 0.25, (double)Ny, Ny - std::ldexp((double)Ny, -52), -1e-17, Ny + 1e-13, nan, inf, -inf, 1e300, -1e300};
    long checked = 0;
    int seen = 0;
    for (int topo = 0; topo < 3; ++topo) {
        const int px = topo != 1, py = topo == 0;      // pp, bb, pb
        // parents of exactly the library's extents: one more column / row for a Face field on a Bounded side, so that the sanitizer sees
        // every address beyond what a model would have allocated
        const long niu = Nx + 2 * Hx + (px ? 0 : 1), nju = Ny + 2 * Hy;
        const long niv = Nx + 2 * Hx, njv = Ny + 2 * Hy + (py ? 0 : 1);
        const long nim = Nx + 2 * Hx + 1, njm = Ny + 2 * Hy + 1;
        std::vector<double> u(niu * nju), v(niv * njv), dxfc(nim * njm), dycf(nim * njm);
        for (long k = 0; k < (long)u.size(); ++k) u[k] = 0.3 * std::sin(0.37 * k) + 0.1;
        for (long k = 0; k < (long)v.size(); ++k) v[k] = 0.2 * std::cos(0.23 * k) - 0.05;
        for (long k = 0; k < (long)dxfc.size(); ++k) { dxfc[k] = 1000.0 + 50.0 * std::sin(0.11 * k); dycf[k] = 900.0 + 40.0 * std::cos(0.07 * k); }
        std::vector<uint8_t> mask((long)Nx * Ny, 1);
        for (long k = 0; k < (long)mask.size(); k += 7) mask[k] = 0;
        for (int with_mask = 0; with_mask < 2; ++with_mask)
            for (double tau : {0.0, 600.0, -2500.0, 1e7, inf})
                for (double x0 : ex)
                    for (double y0 : ey) {
                        double x = x0, y = y0;
                        int32_t st = -1;
                        drifters_host_advance(Nx, Ny, Hx, Hy, px, py, u.data(), niu, v.data(), niv, dxfc.data(), dycf.data(), nim,
                                              with_mask ? mask.data() : nullptr, 1, &x, &y, &st, tau, 3);
                        const bool in_range = x >= 0 && x <= Nx && y >= 0 && y <= Ny;
                        const bool both_nan = x != x && y != y;
                        const bool was_inactive = !(csi::drift::finite_(x0) && csi::drift::finite_(y0));
                        // an active drifter ends inside the domain, or lost as (NaN, NaN), or held where it was (wherever that was)
                        if (was_inactive ? st != csi::drift::INACTIVE : !(in_range || ((st & csi::drift::LOST) && both_nan) || (st & csi::drift::HELD))) {
                            printf("FAIL topo %d tau %g (%g, %g) -> (%g, %g) status %d\n", topo, tau, x0, y0, x, y, (int)st);
                            return 1;
                        }
                        seen |= st;
                        ++checked;
                    }
    }
    printf("drifters_host: %ld edge cases, status bits seen %d\n", checked, seen);
    return seen == 31 ? 0 : 2;
}
#endif
