// vjp_host.cpp -- TEST-ONLY: compiles the chunk-level functions of the prox derivative (proxtv_amd/csrc/vjpcore.hpp) with g++ and
// drives phases A, B and C over one fibre the way vjp.hip does on the device, for any chunk length.  Never linked into
// libproxtv_amd.so; built on demand by tests/test_vjp_host.py into a temp directory.
#define PTV_HOST_TEST 1
#define __device__
#define __host__
#define __forceinline__ inline
#include <vector>

#include "../proxtv_amd/csrc/vjpcore.hpp"

using namespace ptv;

namespace {

template <int L>
int run(const double *y, const double *g, int n, double *gx, double *gw) {
    const int nch = (n + L - 1) / L;
    std::vector<vjp::Summary> S((size_t)nch);
    std::vector<vjp::Resolved> R((size_t)nch);
    auto load = [&](vjp::Chunk<L> &ch, int c) {
        const int k0 = c * L, len = n - k0 < L ? n - k0 : L;
        vjp::chunk_load(ch, len, k0 + len < n, [&](int k) { return y[k0 + k]; }, [&](int k) { return g[k0 + k]; });
        vjp::chunk_prefix(ch);
    };
    for (int c = 0; c < nch; c++) {
        vjp::Chunk<L> ch;
        load(ch, c);
        S[(size_t)c] = vjp::chunk_summary(ch);
    }
    const int nseg = vjp::resolve_fibre(S.data(), R.data(), nch, 1);
    for (int c = 0; c < nch; c++) {
        vjp::Chunk<L> ch;
        load(ch, c);
        const int k0 = c * L;
        vjp::chunk_means(ch, R[(size_t)c], gw != nullptr, [&](int k, double v) { gw[k0 + k] = v; });
        for (int k = 0; k < ch.len; k++) gx[k0 + k] = ch.g[k];
    }
    return nseg;
}

}  // namespace

extern "C" {

// gx = P g, gw (or null: n - 1 entries), returns the number of segments; -1 for a chunk length this harness was not built for.
// gx may be g.
int vjp_host_run(const double *y, const double *g, int n, int chunk, double *gx, double *gw) {
    if (n <= 0) return 0;
    switch (chunk) {
    case 1: return run<1>(y, g, n, gx, gw);
    case 2: return run<2>(y, g, n, gx, gw);
    case 7: return run<7>(y, g, n, gx, gw);
    case 16: return run<16>(y, g, n, gx, gw);
    case 64: return run<64>(y, g, n, gx, gw);
    }
    return -1;
}

// the step rule's constants as the library has them: {relative factor (in units of the sample), absolute slack}
void vjp_host_step_rule(double *out) {
    out[0] = swp::kCertifyStep * swp::kCertifyUlp;
    out[1] = swp::kCertifySlack;
}

int vjp_host_is_step(double a, double b) { return vjp::is_step(a, b) ? 1 : 0; }

}
