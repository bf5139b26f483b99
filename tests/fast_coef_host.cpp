// fast_coef_host.cpp -- TEST INFRASTRUCTURE: a thin extern "C" wrapper around the host functions of csrc/csi_fast_coef.h (g++, no GPU),
// loaded with ctypes by tests/test_fast_math_ref.py and tests/test_host_logic.py.
#include "csi_fast_coef.h"

#include <cstring>

extern "C" {

int fch_fc_count(void) { return csi::FC_COUNT; }
int fch_c2_count(void) { return csi::C2_COUNT; }
double fch_pair_coef_scale(int which) { return csi::pair_coef_scale(which); }

// uni: FC_COUNT doubles
void fch_uniform(double dx, double dy, double* uni) {
    std::memset(uni, 0, sizeof(double) * csi::FC_COUNT);
    csi::build_fast_coef_uniform(dx, dy, uni);
}
// out: FC_COUNT * n doubles, coefficient w of table row t at out[w * n + t]
void fch_per_j(int n, double dy, const double* dxc, const double* dxf, const double* azc, const double* azf, double* out) {
    std::vector<double> v;
    csi::build_fast_coef_per_j(n, dy, dxc, dxf, azc, azf, v);
    std::memcpy(out, v.data(), sizeof(double) * v.size());
}
// m: the twelve dense (nj, ni) metric planes in csi_metrics.full order; out: C2_COUNT * ni * nj doubles
void fch_full(int ni, int nj, const double* const* m, double* out) {
    std::vector<double> v;
    csi::build_fast_coef_full(ni, nj, m, v);
    std::memcpy(out, v.data(), sizeof(double) * v.size());
}
int fch_fast_params_supported(double min_mass, double Dmin) { return csi::fast_params_supported(min_mass, Dmin) ? 1 : 0; }

}  // extern "C"
