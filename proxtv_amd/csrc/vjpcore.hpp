// vjpcore.hpp -- the derivative of the 1-D TV-L1 prox, chunk by chunk.  Plain C++ on registers and small arrays:
// vjp.hip runs it one lane per chunk, tests/vjp_host.cpp runs the same functions with g++.
//
// y = prox(x) along one fibre.  Edge k (between samples k and k+1) is a STEP iff
//     |y[k+1] - y[k]| > kCertifyStep * 2^-52 * max(|y[k]|, |y[k+1]|) + kCertifySlack
// (the certifier's rule, certify_rule.hpp, with the scale taken at the edge itself so that no pass over the fibre is needed).
// Segments are the maximal runs of samples between steps; where the prox is differentiable its Jacobian P = dy/dx replaces
// every sample by the mean over its segment (symmetric: the same product serves as VJP and JVP), so for a cotangent g
//     gx = P g ,   gw[k] = sigma_k (gx[k] - gx[k+1])   (sigma_k = sign of the step, 0 on an edge that is none) ,   trace P = #segments.
// Limits of the rule, inherited and not repaired here: at a kink (a jump that is zero up to the rule) the prox is not
// differentiable and the merged segment is what comes out; and the absolute slack turns data far below 1e-9 in magnitude into one
// segment per fibre.
//
// A fibre is cut into chunks of at most L samples.  A chunk owns the edges behind its samples, the one into the next chunk included.
//   phase A  chunk_load + chunk_prefix + chunk_summary   what the chunk knows alone: has it a step, (sum, count) of its open head
//                                                        (up to its first step) and of its open tail (behind its last step)
//   phase B  resolve_fibre (or, in parallel, vjp_combine) the segments that span chunks, over the monoid (flag, sum, count): a forward
//                                                        pass sums each open run ONCE, left to right, a backward pass hands the mean
//                                                        to every chunk the run touches -- so a segment has one value, bit for bit
//   phase C  chunk_load + chunk_prefix + chunk_means      the chunk again, with those means for its head and tail
// Sums run left to right inside a chunk and across chunks: nothing depends on timing, the result is the same bits every run.
// chunk_load is the only reader of y, and keeps of it two masks; chunk_codes packs those into a word per chunk and chunk_load_steps
// fills a chunk from the word, so that phases A and C can run without y (the tape of step codes).
#pragma once

#include "certify_rule.hpp"

#ifdef PTV_HOST_TEST
#include <cmath>
#define PTV_VJP_HD inline
#else
#define PTV_VJP_HD __host__ __device__ __forceinline__
#endif

namespace ptv {
namespace vjp {

PTV_VJP_HD bool is_step(double a, double b) {
    return fabs(b - a) > swp::kCertifyStep * swp::kCertifyUlp * fmax(fabs(a), fabs(b)) + swp::kCertifySlack;
}

// bits below k / the lowest and the highest set bit (x != 0): masks are at most 64 bits wide
PTV_VJP_HD unsigned long long below(int k) { return k >= 64 ? ~0ull : (1ull << k) - 1ull; }
PTV_VJP_HD int lowest(unsigned long long x) { return __builtin_ctzll(x); }
PTV_VJP_HD int highest(unsigned long long x) { return 63 - __builtin_clzll(x); }

// one chunk in registers: its cotangent samples (overwritten in place by prefix sums, then by means), which of its edges step
template <int L>
struct Chunk {
    static_assert(L >= 1 && L <= 64, "edge masks are 64 bits wide");
    double g[L];
    unsigned long long step = 0, up = 0;   // bit k: the edge behind sample k is a step / a step upwards
    int len = 0;                           // samples in this chunk (the fibre's last chunk may be short)
    bool has_next = false;                 // a sample follows in the fibre: the chunk owns the edge into it
};

// what a chunk knows alone (phase A -> B)
struct Summary {
    double hs, ts;    // sums of the open head (samples up to the first step; the whole chunk when there is none) and the open tail
    int hc, tc;       // their counts; tc == 0: the edge into the next chunk is a step
    int flag, nsteps; // the chunk holds a step ; how many
};
// what phase B hands back (B -> C): the means of the segments the chunk's first and last samples lie in, and of the one the next
// chunk starts with (for gw on the edge between them)
struct Resolved {
    double head, tail, next, spare;
};

// Y(k): y of sample k of the chunk, k = 0 .. len (len itself only when has_next) ; G(k): the cotangent
template <int L, class Y, class G>
PTV_VJP_HD void chunk_load(Chunk<L> &c, int len, bool has_next, Y y, G g) {
    c.len = len;
    c.has_next = has_next;
    c.step = c.up = 0;
    double a = y(0);
#pragma unroll
    for (int k = 0; k < L; k++) {
        if (k < len) {
            c.g[k] = g(k);
            if (k < len - 1 || has_next) {
                const double b = y(k + 1);
                if (is_step(a, b)) {
                    c.step |= 1ull << k;
                    if (b > a) c.up |= 1ull << k;
                }
                a = b;
            }
        }
    }
}

// ---- step codes: all that chunk_load keeps of y ----------------------------------------------------------------------------------
// One 32-bit word per chunk of at most 16 samples: bit k = the edge behind sample k is a step, bit 16 + k = that step goes up; the
// bits of edges the chunk does not own (beyond a short last chunk, behind the fibre's last sample) are 0.  chunk_codes walks y the
// way chunk_load does, so chunk_load_steps(chunk_codes(y), g) leaves the Chunk chunk_load(y, g) leaves, bit for bit.
constexpr int kCodeEdges = 16;

template <int L, class Y>
PTV_VJP_HD unsigned chunk_codes(int len, bool has_next, Y y) {
    static_assert(L >= 1 && L <= kCodeEdges, "a code word holds 16 edges");
    unsigned word = 0;
    double a = y(0);
#pragma unroll
    for (int k = 0; k < L; k++) {
        if (k < len && (k < len - 1 || has_next)) {
            const double b = y(k + 1);
            if (is_step(a, b)) word |= (b > a ? 0x10001u : 1u) << k;
            a = b;
        }
    }
    return word;
}

template <int L, class G>
PTV_VJP_HD void chunk_load_steps(Chunk<L> &c, int len, bool has_next, unsigned word, G g) {
    static_assert(L <= kCodeEdges, "a code word holds 16 edges");
    c.len = len;
    c.has_next = has_next;
    c.step = word & 0xffffu;
    c.up = word >> kCodeEdges;
#pragma unroll
    for (int k = 0; k < L; k++)
        if (k < len) c.g[k] = g(k);
}

// g[k] <- the sum of g over the samples of k's segment up to k, inside the chunk, left to right
template <int L>
PTV_VJP_HD void chunk_prefix(Chunk<L> &c) {
#pragma unroll
    for (int k = 1; k < L; k++)
        if (k < c.len && !((c.step >> (k - 1)) & 1ull)) c.g[k] += c.g[k - 1];
}

// first sample of the segment sample k lies in (inside the chunk)
template <int L>
PTV_VJP_HD int segment_start(const Chunk<L> &c, int k) {
    const unsigned long long b = c.step & below(k);
    return b ? highest(b) + 1 : 0;
}

// after chunk_prefix
template <int L>
PTV_VJP_HD Summary chunk_summary(const Chunk<L> &c) {
    Summary s;
    s.flag = c.step != 0ull;
    s.nsteps = 0;
    const int last = c.len - 1, first_step = s.flag ? lowest(c.step) : last;
    s.hs = s.ts = 0.0;
#pragma unroll
    for (int k = 0; k < L; k++) {
        if (k == first_step) s.hs = c.g[k];
        if (k == last) s.ts = c.g[k];
        s.nsteps += (int)((c.step >> k) & 1ull);
    }
    s.hc = first_step + 1;
    if ((c.step >> last) & 1ull) {
        s.ts = 0.0;
        s.tc = 0;
    } else {
        s.tc = c.len - segment_start(c, last);
    }
    return s;
}

// ---- phase B: the monoid (flag, sum, count) ------------------------------------------------------------------------------------
// An element stands for a stretch of chunks: `flag` = it holds a step, (s, n) = sum and count of the run that is open at its right
// end.  combine(a, b) is the stretch a followed by b; {0, 0, 0} is the identity.
struct Run {
    double s;
    int n, flag;
};
PTV_VJP_HD Run vjp_combine(const Run &a, const Run &b) {
    if (b.flag) return b;
    return Run{a.s + b.s, a.n + b.n, a.flag};
}
PTV_VJP_HD Run run_of(const Summary &s) { return s.flag ? Run{s.ts, s.tc, 1} : Run{s.hs, s.hc, 0}; }
// the mean of the segment chunk c's first sample lies in, should it close inside c (or c be the fibre's last chunk): `open` is the
// run that reaches c from the left
PTV_VJP_HD double head_mean(const Run &open, const Summary &s) { return (open.s + s.hs) / (double)(open.n + s.hc); }
// `mine`: head_mean of this chunk ; `right`: the resolved head of the next chunk (anything for the fibre's last chunk)
PTV_VJP_HD Resolved resolve_chunk(const Summary &s, double mine, double right, bool last) {
    Resolved r;
    r.head = (s.flag || last) ? mine : right;
    r.tail = !s.flag ? r.head : (s.tc == 0 ? 0.0 : (last ? s.ts / (double)s.tc : right));
    r.next = last ? 0.0 : right;
    r.spare = 0.0;
    return r;
}

// one fibre, sequentially: S[c * stride], R[c * stride] for its chunks c = 0 .. nch-1.  Returns the fibre's number of segments.
PTV_VJP_HD int resolve_fibre(const Summary *S, Resolved *R, int nch, long stride) {
    Run open{0.0, 0, 0};
    int steps = 0;
    for (int c = 0; c < nch; c++) {
        const Summary s = S[c * stride];
        R[c * stride].head = head_mean(open, s);
        open = vjp_combine(open, run_of(s));
        steps += s.nsteps;
    }
    double right = 0.0;
    for (int c = nch - 1; c >= 0; c--) {
        const Resolved r = resolve_chunk(S[c * stride], R[c * stride].head, right, c == nch - 1);
        R[c * stride] = r;
        right = r.head;
    }
    return steps + 1;
}

// ---- phase C -------------------------------------------------------------------------------------------------------------------
// after chunk_prefix: g[k] <- the mean of k's segment ; GW(k, v) receives gw of every edge the chunk owns (pass want_gw = false to
// skip them)
template <int L, class GW>
PTV_VJP_HD void chunk_means(Chunk<L> &c, const Resolved &r, bool want_gw, GW gw) {
    const int last = c.len - 1;
    double m = 0.0, right = r.next;   // the mean of the segment being written ; the mean of sample k + 1
#pragma unroll
    for (int k = L - 1; k >= 0; k--) {
        if (k <= last) {
            const bool ends = ((c.step >> k) & 1ull) != 0ull;
            if (ends || k == last) {
                const int s0 = segment_start(c, k);
                m = s0 == 0 ? r.head : ((k == last && !ends) ? r.tail : c.g[k] / (double)(k - s0 + 1));
            }
            if (want_gw && (k < last || c.has_next)) gw(k, ends ? (((c.up >> k) & 1ull) ? m - right : right - m) : 0.0);
            c.g[k] = m;
            right = m;
        }
    }
}

}  // namespace vjp
}  // namespace ptv
