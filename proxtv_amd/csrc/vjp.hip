// vjp.hip -- the derivative of the batched 1-D TV-L1 prox (proxtv_tv1_fibres_vjp_dev): a segmented mean along every fibre.
//
// The arithmetic is vjpcore.hpp's, one lane per chunk of kVjpL samples, in the three phases described there:
//   A  vjp_*_kernel<VJP_SUMMARY> reads y and g, leaves one Summary per chunk
//   B  vjp_resolve_*_kernel      per fibre over its summaries: the means of the segments that span chunks, the fibre's segment count
//   C  vjp_*_kernel<VJP_PLAIN>   reads y and g again, writes gx (and gw)
// in the certifier's two geometries: strided fibres, 64 adjacent fibres per wave so that every access is a 512-byte row and a lane
// walks its chunk straight from global memory; contiguous fibres, where a wave stages 64 consecutive chunks through LDS (rows
// padded to an odd stride) so that global accesses stay coalesced while each lane walks its own row.  Summaries live in HBM scratch
// from the pool; there are no atomics: every sum has one order, so two calls give the same bits.  An output may be its input g:
// a chunk reads all it needs of g before anything of gx is written, and no chunk reads another's g.
//
// The second half of the file is the derivative of the 2-D Douglas-Rachford solve (proxtv_DR2_TV_vjp_dev): the unfused
// forward recurrence with its sweep outputs kept, then the same three phases once per sweep, last sweep first.  The pointwise work of
// the reverse recurrence rides in phase C as epilogue variants of the two kernels (VJP_DR_ROW / VJP_DR_COL below), the way ops.hpp
// folds the forward's into the sweeps: a reverse iteration is two fibre VJPs and no other pass over the arrays.
#include "solvers.hpp"
#include "vjpcore.hpp"

#include <algorithm>
#include <memory>
#include <vector>

#include "pointwise.hpp"
#include "sweep.hpp"

namespace ptv {

namespace {

using vjp::Chunk;
using vjp::Resolved;
using vjp::Run;
using vjp::Summary;

constexpr int kVjpL = 16;             // samples per chunk: sixteen cotangents in registers per lane
constexpr int kVjpRow = kVjpL + 1;    // LDS row of the contiguous kernel: the chunk plus the next sample's y; odd, so conflict-free
static_assert((kVjpL & (kVjpL - 1)) == 0, "the staging loops split an element index by shifts");

// What a launch of the chunk kernels does: phase A, or phase C with one of three write-outs of the means a = P g.
//   VJP_PLAIN    gx = a                                                    (proxtv_tv1_fibres_vjp_dev)
//   VJP_DR_ROW   the row sweep of a reverse Douglas-Rachford iteration, g = gbar in place:   gU += a ;  c = 2 a - g ;  gx = g - a
//                ... of the final sweep, g = the caller's cotangent:                          gU  = a ;  c = a       ;  gx = -a
//   VJP_DR_COL   the column sweep behind it, g = c, gx = what the row sweep left:             gx += a
// and gw = or += the per-edge gradient.  Every element is read and written by the one lane that owns it.
enum { VJP_SUMMARY = 0, VJP_PLAIN = 1, VJP_DR_ROW = 2, VJP_DR_COL = 3 };
struct VjpEpi {
    double *gU = nullptr, *c = nullptr;   // VJP_DR_ROW
    int final = 0;                        // VJP_DR_ROW: the final sweep's form
    int add_gw = 0;                       // gw accumulates
};

// g0: the cotangent the sample came in with (VJP_DR_ROW, not final; anything otherwise)
template <int MODE>
__device__ __forceinline__ void vjp_store(const VjpEpi &e, double *gx, long i, double a, double g0) {
    if constexpr (MODE == VJP_DR_ROW) {
        if (e.final) {
            e.gU[i] = a;
            e.c[i] = a;
            gx[i] = -a;
        } else {
            e.gU[i] += a;
            e.c[i] = 2.0 * a - g0;
            gx[i] = g0 - a;
        }
    } else if constexpr (MODE == VJP_DR_COL) {
        gx[i] += a;
    } else {
        gx[i] = a;
    }
}
template <int MODE>
__device__ __forceinline__ void vjp_store_gw(const VjpEpi &e, double *gw, long i, double v) {
    if (MODE != VJP_PLAIN && e.add_gw) gw[i] += v;
    else gw[i] = v;
}

// ---- strided fibres: wave = 64 adjacent fibres x one chunk ---------------------------------------------------------------------
// S and R are indexed chunk * count + fibre (adjacent lanes, adjacent records)
template <int MODE>
__global__ __launch_bounds__(256) void vjp_strided_kernel(const double *y, const double *g, double *gx, double *gw, FibreGeom geo, int nch,
                                                          Summary *S, const Resolved *R, VjpEpi epi) {
    constexpr bool WRITE = MODE != VJP_SUMMARY;
    const long unit = (long)blockIdx.x * 4 + (threadIdx.x >> 6), groups = (geo.count + 63) / 64;
    if (unit >= groups * nch) return;
    long grp, c;
    divmod_nonneg(unit, (long)nch, grp, c);
    const long j = grp * 64 + (threadIdx.x & 63);
    if (j >= geo.count) return;
    long blk, off;
    divmod_nonneg(j, geo.inc, blk, off);
    const int k0 = (int)c * kVjpL, clen = min(kVjpL, geo.len - k0);
    const bool has_next = k0 + clen < geo.len;
    const long base = blk * geo.inc * geo.len + off + (long)k0 * geo.inc, inc = geo.inc;
    Chunk<kVjpL> ch;
    vjp::chunk_load(ch, clen, has_next, [&](int k) { return y[base + (long)k * inc]; }, [&](int k) { return g[base + (long)k * inc]; });
    double g0[MODE == VJP_DR_ROW ? kVjpL : 1] = {};   // the cotangents as they came in: the row epilogue wants them next to the means
    if constexpr (MODE == VJP_DR_ROW) {
#pragma unroll
        for (int k = 0; k < kVjpL; k++)
            if (k < clen) g0[k] = ch.g[k];
    }
    vjp::chunk_prefix(ch);
    const long idx = c * geo.count + j;
    if (!WRITE) {
        S[idx] = vjp::chunk_summary(ch);
        return;
    }
    const long wbase = blk * geo.inc * (geo.len - 1) + off + (long)k0 * geo.inc;
    vjp::chunk_means(ch, R[idx], gw != nullptr, [&](int k, double v) { vjp_store_gw<MODE>(epi, gw, wbase + (long)k * inc, v); });
#pragma unroll
    for (int k = 0; k < kVjpL; k++)
        if (k < clen) vjp_store<MODE>(epi, gx, base + (long)k * inc, ch.g[k], g0[MODE == VJP_DR_ROW ? k : 0]);
}

// one lane per fibre, over its chunks in order
__global__ __launch_bounds__(64) void vjp_resolve_strided_kernel(const Summary *S, Resolved *R, int nch, long count, int *nseg) {
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= count) return;
    const int n = vjp::resolve_fibre(S + j, R + j, nch, count);
    if (nseg) nseg[j] = n;
}

// ---- contiguous fibres: wave = 64 consecutive chunks (of one fibre or of several), staged through LDS -------------------------------
// S and R are indexed fibre * nch + chunk
template <int MODE>
__global__ __launch_bounds__(64) void vjp_contig_kernel(const double *y, const double *g, double *gx, double *gw, int len, long count, int nch,
                                                        Summary *S, const Resolved *R, VjpEpi epi) {
    constexpr bool WRITE = MODE != VJP_SUMMARY;
    __shared__ double ty[64 * kVjpRow], tg[64 * kVjpRow];
    const int lane = threadIdx.x;
    const long unit = (long)blockIdx.x * 64 + lane;
    const bool valid = unit < count * nch;
    long j = 0, c = 0;
    if (valid) divmod_nonneg(unit, (long)nch, j, c);
    const int k0 = (int)c * kVjpL, clen = valid ? min(kVjpL, len - k0) : 0;
    const bool has_next = valid && k0 + clen < len;
    const long base = j * len + k0;
    // rows in: element e of the tile is sample e % L of the chunk of lane e / L
#pragma unroll
    for (int i = 0; i < kVjpL; i++) {
        const int e = i * 64 + lane, src = e / kVjpL, k = e % kVjpL;
        const long b = __shfl(base, src);
        if (k < __shfl(clen, src)) {
            ty[src * kVjpRow + k] = y[b + k];
            tg[src * kVjpRow + k] = g[b + k];
        }
    }
    if (has_next) ty[lane * kVjpRow + clen] = y[base + clen];
    __syncthreads();
    Chunk<kVjpL> ch;
    if (valid) {
        const double *my = ty + lane * kVjpRow, *mg = tg + lane * kVjpRow;
        vjp::chunk_load(ch, clen, has_next, [&](int k) { return my[k]; }, [&](int k) { return mg[k]; });
        vjp::chunk_prefix(ch);
    }
    if (!WRITE) {
        if (valid) S[unit] = vjp::chunk_summary(ch);
        return;
    }
    // rows out: gx through the tile g came in by, gw through y's (the lane is done with its row of y).  The epilogues' other operands
    // meet the means in the coalesced loop below, straight from and to global memory: no third tile (the row epilogue reads its sample of
    // g a second time there -- the lane that reads it is the one that overwrites it)
    const bool want_gw = gw != nullptr;
    if (valid) {
        double *my = ty + lane * kVjpRow, *mg = tg + lane * kVjpRow;
        vjp::chunk_means(ch, R[unit], want_gw, [&](int k, double v) { my[k] = v; });
#pragma unroll
        for (int k = 0; k < kVjpL; k++)
            if (k < clen) mg[k] = ch.g[k];
    }
    __syncthreads();
    const long wbase = j * (len - 1) + k0;
    const int wlen = has_next ? clen : clen - 1;   // edges this chunk owns
#pragma unroll
    for (int i = 0; i < kVjpL; i++) {
        const int e = i * 64 + lane, src = e / kVjpL, k = e % kVjpL;
        const long b = __shfl(base, src), wb = __shfl(wbase, src);
        const int n = __shfl(clen, src), nw = __shfl(wlen, src);
        if (k < n) {
            double g0 = 0.0;
            if constexpr (MODE == VJP_DR_ROW)
                if (!epi.final) g0 = g[b + k];
            vjp_store<MODE>(epi, gx, b + k, tg[src * kVjpRow + k], g0);
        }
        if (want_gw && k < nw) vjp_store_gw<MODE>(epi, gw, wb + k, ty[src * kVjpRow + k]);
    }
}

// one wave per fibre, 64 chunks per trip: a scan with vjp_combine across the lanes forwards, a ballot backwards
__global__ __launch_bounds__(256) void vjp_resolve_contig_kernel(const Summary *S, Resolved *R, int nch, long count, int *nseg) {
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= count) return;   // (the whole wave)
    const Summary *Sj = S + j * nch;
    Resolved *Rj = R + j * nch;
    const Summary none{0.0, 0.0, 0, 0, 0, 0};
    Run carry{0.0, 0, 0};
    int steps = 0;
    for (int c0 = 0; c0 < nch; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < nch;
        const Summary s = in ? Sj[c] : none;
        Run e = in ? vjp::run_of(s) : Run{0.0, 0, 0};
        for (int o = 1; o < 64; o <<= 1) {
            const Run t{__shfl_up(e.s, o), __shfl_up(e.n, o), __shfl_up(e.flag, o)};
            if (lane >= o) e = vjp::vjp_combine(t, e);
        }
        e = vjp::vjp_combine(carry, e);
        Run open{__shfl_up(e.s, 1), __shfl_up(e.n, 1), __shfl_up(e.flag, 1)};
        if (lane == 0) open = carry;
        if (in) Rj[c].head = vjp::head_mean(open, s);
        carry = Run{__shfl(e.s, 63), __shfl(e.n, 63), __shfl(e.flag, 63)};
        steps += s.nsteps;
    }
    for (int o = 32; o > 0; o >>= 1) steps += __shfl_xor(steps, o);
    if (nseg && lane == 0) nseg[j] = steps + 1;
    double beyond = 0.0;   // the resolved head of the first chunk of the trip to the right
    for (int c0 = ((nch - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
        const int c = c0 + lane;
        const bool in = c < nch, last = c == nch - 1;
        const Summary s = in ? Sj[c] : none;
        const double mine = in ? Rj[c].head : 0.0;
        // the head of chunk c is that of the first chunk at or behind it whose head segment closes
        const unsigned long long closes = __ballot(in && (s.flag || last)) >> lane;
        double head = __shfl(mine, closes ? lane + __builtin_ctzll(closes) : lane);
        if (!closes) head = beyond;
        double right = __shfl_down(head, 1);
        if (lane == 63) right = beyond;
        if (in) Rj[c] = vjp::resolve_chunk(s, mine, right, last);
        beyond = __shfl(head, 0);
    }
}

}  // namespace

namespace {

// phases A, B and C<MODE> of one sweep's derivative on the stream; S and R hold geo.count * ceil(geo.len / kVjpL) records.  gx == null: no phase C.
template <int MODE>
void vjp_launch(const double *y, const double *g, double *gx, double *gw, int *nseg, const FibreGeom &geo, Summary *S, Resolved *R,
                const VjpEpi &epi, hipStream_t s) {
    const int nch = (geo.len + kVjpL - 1) / kVjpL;
    const long units = geo.count * nch;
    if (geo.inc == 1) {
        const unsigned blocks = (unsigned)((units + 63) / 64), fibres4 = (unsigned)((geo.count + 3) / 4);
        hipLaunchKernelGGL(vjp_contig_kernel<VJP_SUMMARY>, dim3(blocks), dim3(64), 0, s, y, g, gx, gw, geo.len, geo.count, nch, S, R, VjpEpi{});
        hipLaunchKernelGGL(vjp_resolve_contig_kernel, dim3(fibres4), dim3(256), 0, s, S, R, nch, geo.count, nseg);
        if (gx) hipLaunchKernelGGL(vjp_contig_kernel<MODE>, dim3(blocks), dim3(64), 0, s, y, g, gx, gw, geo.len, geo.count, nch, S, R, epi);
    } else {
        const long waves = ((geo.count + 63) / 64) * nch;
        const unsigned blocks = (unsigned)((waves + 3) / 4), fibres64 = (unsigned)((geo.count + 63) / 64);
        hipLaunchKernelGGL(vjp_strided_kernel<VJP_SUMMARY>, dim3(blocks), dim3(256), 0, s, y, g, gx, gw, geo, nch, S, R, VjpEpi{});
        hipLaunchKernelGGL(vjp_resolve_strided_kernel, dim3(fibres64), dim3(64), 0, s, S, R, nch, geo.count, nseg);
        if (gx) hipLaunchKernelGGL(vjp_strided_kernel<MODE>, dim3(blocks), dim3(256), 0, s, y, g, gx, gw, geo, nch, S, R, epi);
    }
    PTV_HIP(hipGetLastError());
}

long vjp_units(const FibreGeom &geo) { return geo.count * ((geo.len + kVjpL - 1) / kVjpL); }

}  // namespace

void tv1_fibres_vjp(const double *y, const double *g, double *gx, double *gw, int *nseg, const int *ns, int nds, int dim, hipStream_t s) {
    const FibreGeom geo = fibres_along(ns, nds, dim);
    if (geo.count <= 0 || geo.len <= 0) return;
    const long units = vjp_units(geo);
    Scratch S(sizeof(Summary) * (size_t)units), R(sizeof(Resolved) * (size_t)units);
    if (geo.len == 1) gw = nullptr;   // no edges
    if (!g) g = y;                    // (segment counts alone: phase A sums something, phase C does not run)
    vjp_launch<VJP_PLAIN>(y, g, gx, gw, nseg, geo, S.as<Summary>(), R.as<Resolved>(), VjpEpi{}, s);
    PTV_HIP(hipStreamSynchronize(s));   // (the scratch goes back to the pool behind this)
}

// ---- the derivative of the 2-D Douglas-Rachford solve ------------------------------------------------------------------------------
namespace {

// gU[b * n + i] += 2 sums[b] / n : what the cotangent of t0 = 2 mean(U) hands every sample of image b
__global__ __launch_bounds__(256) void dr_vjp_mean_term_kernel(double *gU, long n, const double *sums) {
    const double v = 2 * sums[blockIdx.y] / n;
    double *seg = gU + (long)blockIdx.y * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) seg[i] += v;
}

}  // namespace

size_t dr2_vjp_tape_bytes(size_t M, size_t N, size_t B, int maxit) {
    if (maxit <= 0) maxit = MAX_ITERS_DR;
    return 2 * ((size_t)maxit + 1) * sizeof(double) * M * N * B;
}

// Forward: the recurrence of dr2_norms (solvers.hip) on B stacked images with the sweep outputs x1_k, x2_k kept, k = 0 .. maxit (the last
// pair: the final sweeps); nothing else is needed afterwards, where P_c / P_r are read off those outputs.
//   t = 2 mean(U) ; repeat: x1 = prox_c(t), x2 = prox_r(U - t + 2 x1), t <- t - x1 + x2 ; x1 = prox_c(t), out = x2 = prox_r(U - t + x1)
// Reverse, for the cotangent g of out (gbar: the cotangent of t; every line one launch of three phases):
//   final  a = P_r g : gU = a, c = a, gbar = -a, gW2 = gw    |  d = P_c c : gbar += d, gW1 = gw
//   k = maxit-1 .. 0
//          a = P_r gbar : gU += a, c = 2 a - gbar, gbar -= a, gW2 += gw   |  d = P_c c : gbar += d, gW1 += gw
//   end    gU += 2 sum(gbar) / (M N) per image
void dr2_vjp(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, const double *W1m, const double *W2m, const double *g,
             double *out, double *gU, double *gW1, double *gW2, double *glam, int maxit, hipStream_t s) {
    const long n1 = (long)(M * N), n = n1 * (long)B;
    if (maxit <= 0) maxit = MAX_ITERS_DR;
    if (n == 0) return;
    const int ns[3] = {(int)M, (int)N, (int)B};
    const FibreGeom cols = fibres_along(ns, 3, 0), rows = fibres_along(ns, 3, 1);
    const long e1 = (long)((M - 1) * N), e2 = (long)(M * (N - 1));   // edges per image
    const size_t bytes = sizeof(double) * (size_t)n;

    Scratch tape(dr2_vjp_tape_bytes(M, N, B, maxit)), t(bytes), v(bytes);
    Scratch partials(sizeof(double) * kReduceBlocks * B), sums(sizeof(double) * 2 * B);
    auto x1 = [&](int k) { return tape.d() + (size_t)(2 * k) * (size_t)n; };
    auto x2 = [&](int k) { return tape.d() + (size_t)(2 * k + 1) * (size_t)n; };
    {   // seed of the geometry policy, like dr2: the image's edge statistics (the first array a sweep sees here is the constant t0)
        const int both[2] = {0, 1};
        const double *const wts[2] = {W1m, W2m};
        policy_probe(unary, wts, ns, 3, both, 2, s);
    }
    sum_to(unary, n1, (long)B, partials.d(), sums.d(), s);
    dr_fill(t.d(), n1, (long)B, sums.d(), 1.0, s);
    for (int k = 0; k <= maxit; k++) {
        const bool last = k == maxit;
        tv1_fibres(t.d(), x1(k), ns, 3, 0, W1, W1m, s);
        lincomb(v.d(), unary, 1.0, t.d(), -1.0, x1(k), last ? 1.0 : 2.0, nullptr, 0, n, s);
        tv1_fibres(v.d(), x2(k), ns, 3, 1, W2, W2m, s);
        if (!last) lincomb(t.d(), t.d(), 1.0, x1(k), -1.0, x2(k), 1.0, nullptr, 0, n, s);
    }
    if (out) PTV_HIP(hipMemcpyAsync(out, x2(maxit), bytes, hipMemcpyDeviceToDevice, s));

    // t and v are free again: gbar and c
    double *gbar = t.d(), *c = v.d();
    const bool want_gw = gW1 || gW2 || glam;
    std::unique_ptr<Scratch> own1, own2;   // (the per-edge sums are what glam is summed from: kept here when the caller does not want them)
    if (want_gw && !gW1 && e1 > 0) { own1.reset(new Scratch(sizeof(double) * (size_t)e1 * B)); gW1 = own1->d(); }
    if (want_gw && !gW2 && e2 > 0) { own2.reset(new Scratch(sizeof(double) * (size_t)e2 * B)); gW2 = own2->d(); }
    double *w1 = (want_gw && e1 > 0) ? gW1 : nullptr, *w2 = (want_gw && e2 > 0) ? gW2 : nullptr;
    const long units = std::max(vjp_units(cols), vjp_units(rows));
    Scratch S(sizeof(Summary) * (size_t)units), R(sizeof(Resolved) * (size_t)units);
    for (int k = maxit; k >= 0; k--) {
        VjpEpi row, col;
        row.gU = gU;
        row.c = c;
        row.final = k == maxit;
        row.add_gw = col.add_gw = k != maxit;
        vjp_launch<VJP_DR_ROW>(x2(k), row.final ? g : gbar, gbar, w2, nullptr, rows, S.as<Summary>(), R.as<Resolved>(), row, s);
        vjp_launch<VJP_DR_COL>(x1(k), c, gbar, w1, nullptr, cols, S.as<Summary>(), R.as<Resolved>(), col, s);
    }
    sum_to(gbar, n1, (long)B, partials.d(), sums.d(), s);
    {
        const long blocks = (n1 + 255) / 256;
        hipLaunchKernelGGL(dr_vjp_mean_term_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024), (unsigned)B), dim3(256), 0, s, gU, n1, sums.d());
        PTV_HIP(hipGetLastError());
    }
    if (glam) {
        std::vector<double> h(2 * B, 0.0);
        for (int which = 0; which < 2; which++) {
            const long e = which ? e2 : e1;
            if (e <= 0) continue;   // no edges that way: the sums stay 0
            sum_to(which ? gW2 : gW1, e, (long)B, partials.d(), sums.d() + which * B, s);
            PTV_HIP(hipMemcpyAsync(h.data() + which * B, sums.d() + which * B, sizeof(double) * B, hipMemcpyDeviceToHost, s));
        }
        PTV_HIP(hipStreamSynchronize(s));
        for (size_t b = 0; b < B; b++) {
            glam[2 * b] = h[b];
            glam[2 * b + 1] = h[B + b];
        }
    }
    PTV_HIP(hipStreamSynchronize(s));   // (the scratch goes back to the pool behind this)
}

}  // namespace ptv
