// vjp.hip -- the derivative of the batched 1-D TV-L1 prox (proxtv_tv1_fibres_vjp_dev): a segmented mean along every fibre.
//
// The arithmetic is vjpcore.hpp's, one lane per chunk of kVjpL samples, in the three phases described there:
//   A  vjp_*_kernel<false>       reads y and g, leaves one Summary per chunk
//   B  vjp_resolve_*_kernel      per fibre over its summaries: the means of the segments that span chunks, the fibre's segment count
//   C  vjp_*_kernel<true>        reads y and g again, writes gx (and gw)
// in the certifier's two geometries: strided fibres, 64 adjacent fibres per wave so that every access is a 512-byte row and a lane
// walks its chunk straight from global memory; contiguous fibres, where a wave stages 64 consecutive chunks through LDS (rows
// padded to an odd stride) so that global accesses stay coalesced while each lane walks its own row.  Summaries live in HBM scratch
// from the pool; there are no atomics: every sum has one order, so two calls give the same bits.  An output may be its input g:
// a chunk reads all it needs of g before anything of gx is written, and no chunk reads another's g.
#include "solvers.hpp"
#include "vjpcore.hpp"

namespace ptv {

namespace {

using vjp::Chunk;
using vjp::Resolved;
using vjp::Run;
using vjp::Summary;

constexpr int kVjpL = 16;             // samples per chunk: sixteen cotangents in registers per lane
constexpr int kVjpRow = kVjpL + 1;    // LDS row of the contiguous kernel: the chunk plus the next sample's y; odd, so conflict-free
static_assert((kVjpL & (kVjpL - 1)) == 0, "the staging loops split an element index by shifts");

// ---- strided fibres: wave = 64 adjacent fibres x one chunk ---------------------------------------------------------------------
// S and R are indexed chunk * count + fibre (adjacent lanes, adjacent records)
template <bool WRITE>
__global__ __launch_bounds__(256) void vjp_strided_kernel(const double *y, const double *g, double *gx, double *gw, FibreGeom geo, int nch,
                                                          Summary *S, const Resolved *R) {
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
    vjp::chunk_prefix(ch);
    const long idx = c * geo.count + j;
    if (!WRITE) {
        S[idx] = vjp::chunk_summary(ch);
        return;
    }
    const long wbase = blk * geo.inc * (geo.len - 1) + off + (long)k0 * geo.inc;
    vjp::chunk_means(ch, R[idx], gw != nullptr, [&](int k, double v) { gw[wbase + (long)k * inc] = v; });
#pragma unroll
    for (int k = 0; k < kVjpL; k++)
        if (k < clen) gx[base + (long)k * inc] = ch.g[k];
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
template <bool WRITE>
__global__ __launch_bounds__(64) void vjp_contig_kernel(const double *y, const double *g, double *gx, double *gw, int len, long count, int nch,
                                                        Summary *S, const Resolved *R) {
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
    // rows out: gx through the tile g came in by, gw through y's (the lane is done with its row of y)
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
        if (k < n) gx[b + k] = tg[src * kVjpRow + k];
        if (want_gw && k < nw) gw[wb + k] = ty[src * kVjpRow + k];
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

void tv1_fibres_vjp(const double *y, const double *g, double *gx, double *gw, int *nseg, const int *ns, int nds, int dim, hipStream_t s) {
    const FibreGeom geo = fibres_along(ns, nds, dim);
    if (geo.count <= 0 || geo.len <= 0) return;
    const int nch = (geo.len + kVjpL - 1) / kVjpL;
    const long units = geo.count * nch;
    Scratch S(sizeof(Summary) * (size_t)units), R(sizeof(Resolved) * (size_t)units);
    if (geo.len == 1) gw = nullptr;   // no edges
    if (!g) g = y;                    // (segment counts alone: phase A sums something, phase C does not run)
    if (geo.inc == 1) {
        const unsigned blocks = (unsigned)((units + 63) / 64), fibres4 = (unsigned)((geo.count + 3) / 4);
        hipLaunchKernelGGL(vjp_contig_kernel<false>, dim3(blocks), dim3(64), 0, s, y, g, gx, gw, geo.len, geo.count, nch, S.as<Summary>(),
                           R.as<Resolved>());
        hipLaunchKernelGGL(vjp_resolve_contig_kernel, dim3(fibres4), dim3(256), 0, s, S.as<Summary>(), R.as<Resolved>(), nch, geo.count, nseg);
        if (gx) hipLaunchKernelGGL(vjp_contig_kernel<true>, dim3(blocks), dim3(64), 0, s, y, g, gx, gw, geo.len, geo.count, nch, S.as<Summary>(),
                           R.as<Resolved>());
    } else {
        const long waves = ((geo.count + 63) / 64) * nch;
        const unsigned blocks = (unsigned)((waves + 3) / 4), fibres64 = (unsigned)((geo.count + 63) / 64);
        hipLaunchKernelGGL(vjp_strided_kernel<false>, dim3(blocks), dim3(256), 0, s, y, g, gx, gw, geo, nch, S.as<Summary>(), R.as<Resolved>());
        hipLaunchKernelGGL(vjp_resolve_strided_kernel, dim3(fibres64), dim3(64), 0, s, S.as<Summary>(), R.as<Resolved>(), nch, geo.count, nseg);
        if (gx) hipLaunchKernelGGL(vjp_strided_kernel<true>, dim3(blocks), dim3(256), 0, s, y, g, gx, gw, geo, nch, S.as<Summary>(), R.as<Resolved>());
    }
    PTV_HIP(hipGetLastError());
    PTV_HIP(hipStreamSynchronize(s));   // (the scratch goes back to the pool behind this)
}

}  // namespace ptv
