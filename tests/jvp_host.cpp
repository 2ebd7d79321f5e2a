// jvp_host.cpp -- TEST-ONLY: compiles the tangent load of the prox's forward-mode derivative (proxtv_amd/csrc/jvpcore.hpp, on top of
// vjpcore.hpp) with g++ and drives phases A, B and C over one fibre the way jvp.hip does on the device, for any chunk length, in both
// forms of the edge-injection term: per chunk from the masks (the strided kernel's lanes) and per sample from the neighbouring values
// of y (the contiguous kernel's staging loop).  Never linked into libproxtv_amd.so; built on demand by tests/test_jvp_host.py.
#define PTV_HOST_TEST 1
#define __device__
#define __host__
#define __forceinline__ inline
#include <vector>

#include "../proxtv_amd/csrc/jvpcore.hpp"

using namespace ptv;

namespace {

struct Tangent {
    const double *a, *b, *c;   // up to three arrays, null = skipped
    double ca, cb, cc;
    const double *dw;          // per edge, or null
    double dlam;
    int inject;
};

template <int L>
void run(const double *y, const Tangent &t, int n, int staged, double *dy) {
    const int nch = (n + L - 1) / L;
    std::vector<vjp::Summary> S((size_t)nch);
    std::vector<vjp::Resolved> R((size_t)nch);
    jvp::Comb q;
    q.a = t.a, q.b = t.b, q.c = t.c, q.ca = t.ca, q.cb = t.cb, q.cc = t.cc;
    auto dr = [&](int e) { return (t.dw ? t.dw[e] : 0.0) + t.dlam; };
    // staged: v of the whole fibre first, sample by sample (any order would do), then the plain chunk_load on it
    std::vector<double> v;
    if (staged) {
        v.resize((size_t)n);
        for (int i = n - 1; i >= 0; i--) {
            double x = jvp::comb_at(q, i);
            if (t.inject) {
                const bool hp = i > 0, hn = i < n - 1;
                x += jvp::sample_term(hp, hp ? y[i - 1] : 0.0, y[i], hn, hn ? y[i + 1] : 0.0, hp ? dr(i - 1) : 0.0, hn ? dr(i) : 0.0);
            }
            v[(size_t)i] = x;
        }
    }
    auto load = [&](vjp::Chunk<L> &ch, int c) {
        const int k0 = c * L, len = n - k0 < L ? n - k0 : L;
        const bool has_next = k0 + len < n, has_prev = k0 > 0;
        auto Y = [&](int k) { return y[k0 + k]; };
        if (staged) vjp::chunk_load(ch, len, has_next, Y, [&](int k) { return v[(size_t)(k0 + k)]; });
        else jvp::chunk_load_tangent(ch, len, has_next, has_prev, has_prev ? y[k0 - 1] : 0.0, t.inject != 0, Y,
                                     [&](int k) { return jvp::comb_at(q, k0 + k); }, [&](int k) { return dr(k0 + k); });
        vjp::chunk_prefix(ch);
    };
    for (int c = 0; c < nch; c++) {
        vjp::Chunk<L> ch;
        load(ch, c);
        S[(size_t)c] = vjp::chunk_summary(ch);
    }
    vjp::resolve_fibre(S.data(), R.data(), nch, 1);
    std::vector<double> out((size_t)n);   // (dy may be one of the tangent arrays: nothing is written before every chunk has loaded)
    for (int c = 0; c < nch; c++) {
        vjp::Chunk<L> ch;
        load(ch, c);
        vjp::chunk_means(ch, R[(size_t)c], false, [](int, double) {});
        for (int k = 0; k < ch.len; k++) out[(size_t)(c * L + k)] = ch.g[k];
    }
    for (int i = 0; i < n; i++) dy[i] = out[(size_t)i];
}

}  // namespace

extern "C" {

// dy = P (ca a + cb b + cc c + E(sigma, dw + dlam)) along one fibre of n samples at the prox output y; staged: the per-sample form of E.
// Returns 0, or -1 for a chunk length this harness was not built for.
int jvp_host_run(const double *y, const double *a, double ca, const double *b, double cb, const double *c, double cc, const double *dw,
                 double dlam, int inject, int n, int chunk, int staged, double *dy) {
    if (n <= 0) return 0;
    const Tangent t{a, b, c, ca, cb, cc, dw, dlam, inject};
    switch (chunk) {
    case 1: run<1>(y, t, n, staged, dy); return 0;
    case 2: run<2>(y, t, n, staged, dy); return 0;
    case 7: run<7>(y, t, n, staged, dy); return 0;
    case 16: run<16>(y, t, n, staged, dy); return 0;
    }
    return -1;
}

}
