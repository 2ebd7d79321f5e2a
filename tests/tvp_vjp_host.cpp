// tvp_vjp_host.cpp -- TEST-ONLY: compiles the per-fibre derivative of the general-p TV-Lp prox (proxtv_amd/csrc/tvpvjpcore.hpp) and the
// forward it differentiates (tvpcore.hpp) with g++, one fibre per call.  Never linked into libproxtv_amd.so; built on demand by
// tests/test_tvp_vjp_host.py into a temp directory.
#include <vector>

#include "../proxtv_amd/csrc/tvpcore.hpp"
#include "../proxtv_amd/csrc/tvpvjpcore.hpp"

extern "C" {

// x = prox(y); returns 1 if a cap stopped the iteration.  outer: the forward's outer iterations (0: a closed form)
int host_tvp_forward(const double *y, double *x, int n, double lam, double p, double *gap, int *outer) {
    std::vector<double> v((size_t)n + 1), dl((size_t)n + 1), ll((size_t)n + 1), zz((size_t)n + 1);
    const ptv::tvp::Fibre F{y, x, v.data(), dl.data(), ll.data(), zz.data(), 0, 1, n, lam, p};
    const ptv::tvp::Result r = ptv::tvp::solve(F);
    if (gap) *gap = r.gap;
    if (outer) *outer = r.outer;
    return r.capped;
}

// gx (may be g) = J g for one fibre of n samples whose prox is x; returns glam.  inc: the stride the fibre is laid out with (the
// arrays passed in are dense; the harness spreads them out and gathers the result, as a lane of the kernel sees them)
double host_tvp_vjp(const double *x, const double *g, double *gx, int n, double lam, double p, int inc) {
    const size_t len = (size_t)(n > 0 ? n : 1) * (size_t)inc;
    const bool inplace = gx == g;
    std::vector<double> xs(len, -7.0), gs(len, -7.0), os(len, -7.0), ll(len, -7.0), z1(len, -7.0), z2(len, -7.0);
    for (int i = 0; i < n; i++) {
        xs[(size_t)i * inc] = x[i];
        gs[(size_t)i * inc] = g[i];
    }
    double *out = inplace ? gs.data() : os.data();
    const ptv::tvpvjp::Fibre F{xs.data(), gs.data(), out, ll.data(), z1.data(), z2.data(), 0, inc, n, lam, p};
    const double glam = ptv::tvpvjp::solve(F);
    for (int i = 0; i < n; i++) gx[i] = out[(size_t)i * inc];
    return glam;
}

}
