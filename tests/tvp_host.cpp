// Host build of the general-p TV-Lp fibre solver (proxtv_amd/csrc/tvpcore.hpp), one fibre per call: tests/test_tvp_host.py.
#include <vector>

#include "../proxtv_amd/csrc/tvpcore.hpp"

extern "C" int host_tvp_fibre(const double *y, double *x, int n, double lam, double p, double *gap, int *outer, int *sweeps) {
    std::vector<double> v((size_t)n + 1), dl((size_t)n + 1), ll((size_t)n + 1), zz((size_t)n + 1);
    const ptv::tvp::Fibre F{y, x, v.data(), dl.data(), ll.data(), zz.data(), 0, 1, n, lam, p};
    const ptv::tvp::Result r = ptv::tvp::solve(F);
    if (gap) *gap = r.gap;
    if (outer) *outer = r.outer;
    if (sweeps) *sweeps = r.sweeps;
    return r.capped;
}
