// vjp_steps_host.cpp -- TEST-ONLY: the step codes of the prox derivative (proxtv_amd/csrc/vjpcore.hpp: chunk_codes, chunk_load_steps)
// compiled with g++ and driven over one fibre the way vjp.hip does on the device, for chunks of 1, 2, 7 and 16 samples.  Never linked
// into libproxtv_amd.so; built on demand by tests/test_vjp_steps_host.py into a temp directory -- as a shared object for ctypes, and,
// with -DVJP_STEPS_MAIN, as a program of its own that checks the same things on fibres it draws itself (the sanitizer build).
#define PTV_HOST_TEST 1
#define __device__
#define __host__
#define __forceinline__ inline
#include <cstdio>
#include <cstring>
#include <vector>

#include "../proxtv_amd/csrc/vjpcore.hpp"

using namespace ptv;

namespace {

template <int L>
unsigned codes_of(const double *y, int n, int c) {
    const int k0 = c * L, len = n - k0 < L ? n - k0 : L;
    return vjp::chunk_codes<L>(len, k0 + len < n, [&](int k) { return y[k0 + k]; });
}

// phases A, B, C over one fibre; the chunks are filled from y (words == null) or from the words
template <int L>
int run(const double *y, const unsigned *words, const double *g, int n, double *gx, double *gw) {
    const int nch = (n + L - 1) / L;
    std::vector<vjp::Summary> S((size_t)nch);
    std::vector<vjp::Resolved> R((size_t)nch);
    auto load = [&](vjp::Chunk<L> &ch, int c) {
        const int k0 = c * L, len = n - k0 < L ? n - k0 : L;
        if (words) vjp::chunk_load_steps(ch, len, k0 + len < n, words[c], [&](int k) { return g[k0 + k]; });
        else       vjp::chunk_load(ch, len, k0 + len < n, [&](int k) { return y[k0 + k]; }, [&](int k) { return g[k0 + k]; });
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

// 0: every chunk filled from its word is the chunk filled from y, the bits beyond the edges it owns are 0, up is inside step.
// Otherwise 1 + the first chunk that differs.
template <int L>
int compare(const double *y, const double *g, int n) {
    const int nch = (n + L - 1) / L;
    for (int c = 0; c < nch; c++) {
        const int k0 = c * L, len = n - k0 < L ? n - k0 : L;
        const bool has_next = k0 + len < n;
        vjp::Chunk<L> a, b;
        vjp::chunk_load(a, len, has_next, [&](int k) { return y[k0 + k]; }, [&](int k) { return g[k0 + k]; });
        const unsigned w = codes_of<L>(y, n, c);
        vjp::chunk_load_steps(b, len, has_next, w, [&](int k) { return g[k0 + k]; });
        const int owned = has_next ? len : len - 1;
        const unsigned mask = owned >= 16 ? 0xffffu : (1u << owned) - 1u;
        bool ok = a.step == b.step && a.up == b.up && a.len == b.len && a.has_next == b.has_next;
        ok = ok && std::memcmp(a.g, b.g, sizeof(double) * (size_t)len) == 0;
        ok = ok && (w & 0xffffu & ~mask) == 0 && ((w >> 16) & ~w & 0xffffu) == 0 && ((w >> 16) & ~mask) == 0;
        if (!ok) return 1 + c;
    }
    return 0;
}

}  // namespace

extern "C" {

// 0: equal everywhere; 1 + chunk number of the first difference; -1: a chunk length this harness was not built for
int vjp_steps_host_compare(const double *y, const double *g, int n, int chunk) {
    switch (chunk) {
    case 1: return compare<1>(y, g, n);
    case 2: return compare<2>(y, g, n);
    case 7: return compare<7>(y, g, n);
    case 16: return compare<16>(y, g, n);
    }
    return -1;
}

// words[ceil(n / chunk)] <- the codes of the fibre; returns their number, -1 as above
int vjp_steps_host_words(const double *y, int n, int chunk, unsigned *words) {
    const int nch = (n + chunk - 1) / chunk;
    for (int c = 0; c < nch; c++) {
        switch (chunk) {
        case 1: words[c] = codes_of<1>(y, n, c); break;
        case 2: words[c] = codes_of<2>(y, n, c); break;
        case 7: words[c] = codes_of<7>(y, n, c); break;
        case 16: words[c] = codes_of<16>(y, n, c); break;
        default: return -1;
        }
    }
    return nch;
}

// gx = P g, gw (or null: n - 1 entries) from y (words == null) or from the words; returns the number of segments, -1 as above
int vjp_steps_host_run(const double *y, const unsigned *words, const double *g, int n, int chunk, double *gx, double *gw) {
    if (n <= 0) return 0;
    switch (chunk) {
    case 1: return run<1>(y, words, g, n, gx, gw);
    case 2: return run<2>(y, words, g, n, gx, gw);
    case 7: return run<7>(y, words, g, n, gx, gw);
    case 16: return run<16>(y, words, g, n, gx, gw);
    }
    return -1;
}

}

#ifdef VJP_STEPS_MAIN
namespace {

unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
double uniform() {   // (0, 1), a 64-bit LCG's high bits
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(rng_state >> 11) + 0.5) / 9007199254740992.0;
}

int check(const char *name, const std::vector<double> &y) {
    const int n = (int)y.size();
    std::vector<double> g((size_t)n), gx1((size_t)n), gx2((size_t)n), gw1((size_t)(n > 1 ? n - 1 : 1)), gw2(gw1.size());
    for (double &v : g) v = uniform() - 0.5;
    const int chunks[4] = {1, 2, 7, 16};
    for (int chunk : chunks) {
        if (vjp_steps_host_compare(y.data(), g.data(), n, chunk) != 0) {
            std::printf("FAILED compare: %s n %d chunk %d\n", name, n, chunk);
            return 1;
        }
        std::vector<unsigned> words((size_t)((n + chunk - 1) / chunk));
        vjp_steps_host_words(y.data(), n, chunk, words.data());
        const int s1 = vjp_steps_host_run(y.data(), nullptr, g.data(), n, chunk, gx1.data(), gw1.data());
        const int s2 = vjp_steps_host_run(nullptr, words.data(), g.data(), n, chunk, gx2.data(), gw2.data());
        if (s1 != s2 || std::memcmp(gx1.data(), gx2.data(), sizeof(double) * (size_t)n) != 0 ||
            (n > 1 && std::memcmp(gw1.data(), gw2.data(), sizeof(double) * (size_t)(n - 1)) != 0)) {
            std::printf("FAILED pipeline: %s n %d chunk %d\n", name, n, chunk);
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main() {
    int bad = 0;
    const int sizes[] = {1, 2, 3, 7, 15, 16, 17, 33, 112, 113, 200};
    for (int n : sizes) {
        std::vector<double> y((size_t)n);
        for (double &v : y) v = 4 * uniform() - 2;
        bad += check("random", y);
        double level = uniform();
        for (double &v : y) {
            if (uniform() < 0.2) level = 4 * uniform() - 2;
            v = level;
        }
        bad += check("piecewise constant", y);
        for (double &v : y) v = 0.75;
        bad += check("all equal", y);
        double acc = 0.0;
        for (double &v : y) v = acc += 0.1 + uniform();
        bad += check("strictly monotone", y);
        for (double &v : y) v = -v;
        bad += check("monotone down", y);
    }
    std::printf(bad ? "VJP_STEPS_HOST_FAILED\n" : "VJP_STEPS_HOST_OK\n");
    return bad ? 1 : 0;
}
#endif
