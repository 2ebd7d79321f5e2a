// tv2_vjp_host.cpp -- TEST-ONLY: compiles the per-fibre arithmetic of the TV-L2 prox derivative (proxtv_amd/csrc/tv2vjpcore.hpp) with
// g++ and runs it over one fibre the way tv2_vjp.hip does on the device.  Never linked into libproxtv_amd.so; built on demand by
// tests/test_tv2_vjp_host.py into a temp directory.
#define PTV_HOST_TEST 1
#include <vector>

#include "../proxtv_amd/csrc/tv2vjpcore.hpp"

using namespace ptv;

namespace {

struct Edges {
    double *p;
    double get(int i) const { return p[i]; }
    void put(int i, double v) const { p[i] = v; }
};

}  // namespace

extern "C" {

// gx (may be g) = J g for one fibre of n samples; returns glam
double tv2_vjp_host_run(const double *y, double mu, const double *g, int n, double lam, double *gx) {
    std::vector<double> r((size_t)(n > 0 ? n : 1), -1.0), zh(r.size()), zq(r.size());
    return tv2vjp::fibre(n, mu, lam, [&](int i) { return y[i]; }, [&](int i) { return g[i]; }, Edges{r.data()}, Edges{zh.data()},
                         Edges{zq.data()}, [&](int i, double v) { gx[i] = v; });
}

// the edge from which the forward elimination stops storing pivots (n - 1: it stored them all); n >= 2
int tv2_vjp_host_kfix(const double *y, double mu, const double *g, int n) {
    std::vector<double> r((size_t)n), zh((size_t)n), zq((size_t)n);
    return tv2vjp::eliminate(n, 2.0 + mu, [&](int i) { return y[i]; }, [&](int i) { return g[i]; }, Edges{r.data()}, Edges{zh.data()},
                             Edges{zq.data()})
        .kfix;
}

}
