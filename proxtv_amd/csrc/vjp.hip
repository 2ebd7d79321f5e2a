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
// Phases A and C take of y only which edges step and which way (vjpcore.hpp: chunk_load), so both kernels have a second source, chosen
// at compile time beside MODE: the 2-bit step codes of y, one 32-bit word per chunk (vjp_encode_*_kernel writes them, in the order of
// the Summary / Resolved records, so a lane's word is one coalesced load).  The word instantiations load no y -- 0.25 B a sample in
// place of 8 -- and give the same bits (proxtv_tv1_fibres_steps_dev, proxtv_tv1_fibres_vjp_steps_dev).
//
// The second half of the file is the derivative of the 2-D Douglas-Rachford solve (proxtv_DR2_TV_vjp_dev): the unfused
// forward recurrence with its sweep outputs kept (tape = 0) or their step codes (tape = 1: the sweeps write into arrays the next
// iteration reuses and each output is encoded behind its sweep), then the same three phases once per sweep, last sweep first.  The pointwise work of
// the reverse recurrence rides in phase C as epilogue variants of the two kernels (VJP_DR_ROW / VJP_DR_COL below), the way ops.hpp
// folds the forward's into the sweeps: a reverse iteration is two fibre VJPs and no other pass over the arrays.
//
// The third part is the derivative of the two Dykstra loops behind tvgen (proxtv_PD_TV_vjp_dev), built the same way:
// VJP_PD2 for the two-term loop, VJP_PD_SUMMARY / VJP_PD for the parallel one, whose cotangent is formed on load in phases A and C.
//
// All three loops take a norm in {1, 2} per direction / term (proxtv_DR2_TVp_vjp_dev, proxtv_PD_TVp_vjp_dev): every
// reverse recurrence is linear in a = J g, whichever prox J belongs to.  A TV-L1 sweep keeps the launches described above; a TV-L2
// sweep is tv2_fibres with its multipliers forward and tv2_vjp.hip's kernel with the same write-out mode in reverse (tape_prox /
// tape_vjp), and SweepTape says what each keeps.  With option general_p_vjp a norm may also be a general p: tvp_fibres
// forward, tvp_vjp.hip's kernel in reverse, from the sweep's output alone.
#include "solvers.hpp"
#include "vjpcore.hpp"
#include "jvp.hpp"

#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

#include "pointwise.hpp"
#include "sweep.hpp"
#include "tv2.hpp"
#include "tvp.hpp"
#include "tvp_vjp.hpp"

namespace ptv {

namespace {

using vjp::Chunk;
using vjp::Resolved;
using vjp::Run;
using vjp::Summary;

constexpr int kVjpL = 16;             // samples per chunk: sixteen cotangents in registers per lane
constexpr int kVjpRow = kVjpL + 1;    // LDS row of the contiguous kernel: the chunk plus the next sample's y; odd, so conflict-free
static_assert((kVjpL & (kVjpL - 1)) == 0, "the staging loops split an element index by shifts");
static_assert(kVjpL == kVjpChunk, "jvp.hip lays out its records for the same chunks (jvp.hpp)");

// What a launch of the chunk kernels does: phase A, or phase C with one of three write-outs of the means a = P g.
//   VJP_PLAIN    gx = a                                                    (proxtv_tv1_fibres_vjp_dev)
//   VJP_DR_ROW   the row sweep of a reverse Douglas-Rachford iteration, g = gbar in place:   gU += a ;  c = 2 a - g ;  gx = g - a
//                ... of the final sweep, g = the caller's cotangent:                          gU  = a ;  c = a       ;  gx = -a
//   VJP_DR_COL   the column sweep behind it, g = c, gx = what the row sweep left:             gx += a
// and gw = or += the per-edge gradient.  Every element is read and written by the one lane that owns it.
// The Dykstra loops (pd_vjp below):
//   VJP_PD2      a sweep of the two-term loop, g = the running difference D, in place:       gx = a - g   (and, with gU: gU += a)
//                ... of the last iteration, where the state is still empty:                   gx = a (no gU) ;  gx = a - g, gU = a
//   VJP_PD       term i of the parallel loop: the cotangent is pi = scale g - zeta, formed on load (g = chi, shared by the terms; phase
//                A is VJP_PD_SUMMARY, the same load), gx = zeta_i in place:                   gx = zeta + a ;  gU += gx (final: gU = gx)
//                (zeta == null: the last iteration's form, every zeta_i still 0)
enum { VJP_SUMMARY = 0, VJP_PLAIN = 1, VJP_DR_ROW = 2, VJP_DR_COL = 3, VJP_PD2 = 4, VJP_PD_SUMMARY = 5, VJP_PD = 6 };
struct VjpEpi {
    double *gU = nullptr, *c = nullptr;   // VJP_DR_ROW ; gU: VJP_PD2 (gy) and VJP_PD (the running sum of the zeta_i)
    int final = 0;                        // VJP_DR_ROW: the final sweep's form ; VJP_PD2: the last iteration's ; VJP_PD: the iteration's first term
    int add_gw = 0;                       // gw accumulates
    const double *zeta = nullptr;         // VJP_PD
    double scale = 0.0;                   // VJP_PD: 1 / P
};

// what the chunk kernels read the steps from: y itself (SRC = double) or the code words vjp_encode left of it (SRC = unsigned)
template <class SRC>
constexpr bool vjp_from_words() {
    static_assert(std::is_same<SRC, double>::value || std::is_same<SRC, unsigned>::value, "the source is y or its code words");
    return std::is_same<SRC, unsigned>::value;
}

constexpr bool vjp_writes(int mode) { return mode != VJP_SUMMARY && mode != VJP_PD_SUMMARY; }
constexpr bool vjp_forms_cotangent(int mode) { return mode == VJP_PD_SUMMARY || mode == VJP_PD; }
// modes whose write-out wants a second value per sample next to the mean: the cotangent as it came in, or (VJP_PD) zeta
constexpr bool vjp_keeps(int mode) { return mode == VJP_DR_ROW || mode == VJP_PD2 || mode == VJP_PD; }

// the cotangent of sample i the way phases A and C of VJP_PD both form it: one fused multiply-add, so both see the same bits
__device__ __forceinline__ double vjp_pd_cotangent(const VjpEpi &e, const double *g, long i, double zeta) {
    return __builtin_fma(g[i], e.scale, -zeta);
}

// g0: the cotangent the sample came in with (VJP_DR_ROW, not final; VJP_PD2), zeta (VJP_PD); anything otherwise
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
    } else if constexpr (MODE == VJP_PD2) {
        if (e.gU) {
            e.gU[i] = e.final ? a : e.gU[i] + a;
            gx[i] = a - g0;
        } else {
            gx[i] = e.final ? a : a - g0;
        }
    } else if constexpr (MODE == VJP_PD) {
        const double z = g0 + a;
        gx[i] = z;
        e.gU[i] = e.final ? z : e.gU[i] + z;
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
// S and R are indexed chunk * count + fibre (adjacent lanes, adjacent records), and so are the code words when y is those
template <int MODE, class SRC>
__global__ __launch_bounds__(256) void vjp_strided_kernel(const SRC *y, const double *g, double *gx, double *gw, FibreGeom geo, int nch,
                                                          Summary *S, const Resolved *R, VjpEpi epi) {
    constexpr bool WRITE = vjp_writes(MODE), KEEP = vjp_keeps(MODE), WORDS = vjp_from_words<SRC>();
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
    const long idx = c * geo.count + j;
    Chunk<kVjpL> ch;
    double g0[KEEP ? kVjpL : 1] = {};   // the cotangents as they came in (VJP_PD: zeta): the epilogue wants them next to the means
    // (y: the chunk's samples, walked by chunk_load; or its code word, one coalesced load)
    auto load = [&](auto cot) {
        if constexpr (WORDS) vjp::chunk_load_steps(ch, clen, has_next, y[idx], cot);
        else vjp::chunk_load(ch, clen, has_next, [&](int k) { return y[base + (long)k * inc]; }, cot);
    };
    if constexpr (vjp_forms_cotangent(MODE)) {
        load([&](int k) {
            const long i = base + (long)k * inc;
            const double z = epi.zeta ? epi.zeta[i] : 0.0;
            if constexpr (MODE == VJP_PD) g0[k] = z;
            return vjp_pd_cotangent(epi, g, i, z);
        });
    } else {
        load([&](int k) { return g[base + (long)k * inc]; });
    }
    if constexpr (MODE == VJP_DR_ROW || MODE == VJP_PD2) {
#pragma unroll
        for (int k = 0; k < kVjpL; k++)
            if (k < clen) g0[k] = ch.g[k];
    }
    vjp::chunk_prefix(ch);
    if (!WRITE) {
        S[idx] = vjp::chunk_summary(ch);
        return;
    }
    const long wbase = blk * geo.inc * (geo.len - 1) + off + (long)k0 * geo.inc;
    vjp::chunk_means(ch, R[idx], gw != nullptr, [&](int k, double v) { vjp_store_gw<MODE>(epi, gw, wbase + (long)k * inc, v); });
#pragma unroll
    for (int k = 0; k < kVjpL; k++)
        if (k < clen) vjp_store<MODE>(epi, gx, base + (long)k * inc, ch.g[k], g0[KEEP ? k : 0]);
}

// one lane per fibre, over its chunks in order
__global__ __launch_bounds__(64) void vjp_resolve_strided_kernel(const Summary *S, Resolved *R, int nch, long count, int *nseg) {
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= count) return;
    const int n = vjp::resolve_fibre(S + j, R + j, nch, count);
    if (nseg) nseg[j] = n;
}

// ---- contiguous fibres: wave = 64 consecutive chunks (of one fibre or of several), staged through LDS -------------------------------
// S and R are indexed fibre * nch + chunk, and so are the code words when y is those: they are not staged (a lane's word is one
// coalesced load), the ty tile then only carries gw out
template <int MODE, class SRC>
__global__ __launch_bounds__(64) void vjp_contig_kernel(const SRC *y, const double *g, double *gx, double *gw, int len, long count, int nch,
                                                        Summary *S, const Resolved *R, VjpEpi epi) {
    constexpr bool WRITE = vjp_writes(MODE), WORDS = vjp_from_words<SRC>();
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
            if constexpr (!WORDS) ty[src * kVjpRow + k] = y[b + k];
            if constexpr (vjp_forms_cotangent(MODE)) tg[src * kVjpRow + k] = vjp_pd_cotangent(epi, g, b + k, epi.zeta ? epi.zeta[b + k] : 0.0);
            else tg[src * kVjpRow + k] = g[b + k];
        }
    }
    if constexpr (!WORDS)
        if (has_next) ty[lane * kVjpRow + clen] = y[base + clen];
    __syncthreads();
    Chunk<kVjpL> ch;
    if (valid) {
        const double *mg = tg + lane * kVjpRow;
        if constexpr (WORDS) {
            vjp::chunk_load_steps(ch, clen, has_next, y[unit], [&](int k) { return mg[k]; });
        } else {
            const double *my = ty + lane * kVjpRow;
            vjp::chunk_load(ch, clen, has_next, [&](int k) { return my[k]; }, [&](int k) { return mg[k]; });
        }
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
            if constexpr (MODE == VJP_PD2)
                if (epi.gU || !epi.final) g0 = g[b + k];
            if constexpr (MODE == VJP_PD)
                if (epi.zeta) g0 = epi.zeta[b + k];
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

// ---- step codes: y -> one word per chunk (vjpcore.hpp: chunk_codes), in the geometries and the record order of the kernels above --------
// Each reads y once plus every chunk's next sample and writes its own word: no atomics, the same words every time.
__global__ __launch_bounds__(256) void vjp_encode_strided_kernel(const double *y, unsigned *W, FibreGeom geo, int nch) {
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
    W[c * geo.count + j] = vjp::chunk_codes<kVjpL>(clen, has_next, [&](int k) { return y[base + (long)k * inc]; });
}

__global__ __launch_bounds__(64) void vjp_encode_contig_kernel(const double *y, unsigned *W, int len, long count, int nch) {
    __shared__ double ty[64 * kVjpRow];
    const int lane = threadIdx.x;
    const long unit = (long)blockIdx.x * 64 + lane;
    const bool valid = unit < count * nch;
    long j = 0, c = 0;
    if (valid) divmod_nonneg(unit, (long)nch, j, c);
    const int k0 = (int)c * kVjpL, clen = valid ? min(kVjpL, len - k0) : 0;
    const bool has_next = valid && k0 + clen < len;
    const long base = j * len + k0;
#pragma unroll
    for (int i = 0; i < kVjpL; i++) {
        const int e = i * 64 + lane, src = e / kVjpL, k = e % kVjpL;
        const long b = __shfl(base, src);
        if (k < __shfl(clen, src)) ty[src * kVjpRow + k] = y[b + k];
    }
    if (has_next) ty[lane * kVjpRow + clen] = y[base + clen];
    __syncthreads();
    if (!valid) return;
    const double *my = ty + lane * kVjpRow;
    W[unit] = vjp::chunk_codes<kVjpL>(clen, has_next, [&](int k) { return my[k]; });
}

// the segment counts from the words alone: 1 + the steps of the fibre.  One lane per strided fibre, one wave per contiguous one.
__global__ __launch_bounds__(64) void vjp_count_strided_kernel(const unsigned *W, int nch, long count, int *nseg) {
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= count) return;
    int steps = 0;
    for (int c = 0; c < nch; c++) steps += __popc(W[c * count + j] & 0xffffu);
    nseg[j] = steps + 1;
}
__global__ __launch_bounds__(256) void vjp_count_contig_kernel(const unsigned *W, int nch, long count, int *nseg) {
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= count) return;   // (the whole wave)
    int steps = 0;
    for (int c = lane; c < nch; c += 64) steps += __popc(W[j * nch + c] & 0xffffu);
    for (int o = 32; o > 0; o >>= 1) steps += __shfl_xor(steps, o);
    if (lane == 0) nseg[j] = steps + 1;
}

}  // namespace

namespace {

// phases A, B and C<MODE> of one sweep's derivative on the stream; S and R hold geo.count * ceil(geo.len / kVjpL) records.  gx == null: no phase C.
// y: the sweep's output, or (SRC = unsigned) its code words in the layout of S and R.
template <int MODE, class SRC>
void vjp_launch(const SRC *y, const double *g, double *gx, double *gw, int *nseg, const FibreGeom &geo, Summary *S, Resolved *R,
                const VjpEpi &epi, hipStream_t s) {
    constexpr int A = MODE == VJP_PD ? VJP_PD_SUMMARY : VJP_SUMMARY;   // (phase A forms the cotangent the way phase C will)
    const VjpEpi epa = MODE == VJP_PD ? epi : VjpEpi{};
    const int nch = (geo.len + kVjpL - 1) / kVjpL;
    const long units = geo.count * nch;
    if (geo.inc == 1) {
        const unsigned blocks = (unsigned)((units + 63) / 64), fibres4 = (unsigned)((geo.count + 3) / 4);
        hipLaunchKernelGGL((vjp_contig_kernel<A, SRC>), dim3(blocks), dim3(64), 0, s, y, g, gx, gw, geo.len, geo.count, nch, S, R, epa);
        hipLaunchKernelGGL(vjp_resolve_contig_kernel, dim3(fibres4), dim3(256), 0, s, S, R, nch, geo.count, nseg);
        if (gx) hipLaunchKernelGGL((vjp_contig_kernel<MODE, SRC>), dim3(blocks), dim3(64), 0, s, y, g, gx, gw, geo.len, geo.count, nch, S, R, epi);
    } else {
        const long waves = ((geo.count + 63) / 64) * nch;
        const unsigned blocks = (unsigned)((waves + 3) / 4), fibres64 = (unsigned)((geo.count + 63) / 64);
        hipLaunchKernelGGL((vjp_strided_kernel<A, SRC>), dim3(blocks), dim3(256), 0, s, y, g, gx, gw, geo, nch, S, R, epa);
        hipLaunchKernelGGL(vjp_resolve_strided_kernel, dim3(fibres64), dim3(64), 0, s, S, R, nch, geo.count, nseg);
        if (gx) hipLaunchKernelGGL((vjp_strided_kernel<MODE, SRC>), dim3(blocks), dim3(256), 0, s, y, g, gx, gw, geo, nch, S, R, epi);
    }
    PTV_HIP(hipGetLastError());
}

long vjp_units(const FibreGeom &geo) { return geo.count * ((geo.len + kVjpL - 1) / kVjpL); }

// the same from whichever the tape kept: the code words when there are any, else the sweep's output
template <int MODE>
void vjp_launch_taped(const double *y, const unsigned *words, const double *g, double *gx, double *gw, const FibreGeom &geo, Summary *S, Resolved *R,
                const VjpEpi &epi, hipStream_t s) {
    if (words) vjp_launch<MODE>(words, g, gx, gw, nullptr, geo, S, R, epi, s);
    else       vjp_launch<MODE>(y, g, gx, gw, nullptr, geo, S, R, epi, s);
}

// W[vjp_units(geo)] <- the step codes of y
void vjp_encode(const double *y, unsigned *W, const FibreGeom &geo, hipStream_t s) {
    const int nch = (geo.len + kVjpL - 1) / kVjpL;
    if (geo.inc == 1) {
        const unsigned blocks = (unsigned)((geo.count * nch + 63) / 64);
        hipLaunchKernelGGL(vjp_encode_contig_kernel, dim3(blocks), dim3(64), 0, s, y, W, geo.len, geo.count, nch);
    } else {
        const long waves = ((geo.count + 63) / 64) * nch;
        hipLaunchKernelGGL(vjp_encode_strided_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, y, W, geo, nch);
    }
    PTV_HIP(hipGetLastError());
}

}  // namespace

// phase B alone, for the forward-mode kernels of jvp.hip: the launches vjp_launch makes between its phases A and C
void vjp_resolve(vjp::Summary *S, vjp::Resolved *R, const FibreGeom &geo, int *nseg, hipStream_t s) {
    const int nch = (geo.len + kVjpL - 1) / kVjpL;
    if (geo.inc == 1) hipLaunchKernelGGL(vjp_resolve_contig_kernel, dim3((unsigned)((geo.count + 3) / 4)), dim3(256), 0, s, S, R, nch, geo.count, nseg);
    else              hipLaunchKernelGGL(vjp_resolve_strided_kernel, dim3((unsigned)((geo.count + 63) / 64)), dim3(64), 0, s, S, R, nch, geo.count, nseg);
    PTV_HIP(hipGetLastError());
}

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

long tv1_steps_words(const int *ns, int nds, int dim) {
    const FibreGeom geo = fibres_along(ns, nds, dim);
    return (geo.count <= 0 || geo.len <= 0) ? 0 : vjp_units(geo);
}

void tv1_fibres_steps(const double *y, unsigned *steps, const int *ns, int nds, int dim, hipStream_t s) {
    const FibreGeom geo = fibres_along(ns, nds, dim);
    if (geo.count <= 0 || geo.len <= 0) return;
    vjp_encode(y, steps, geo, s);
    PTV_HIP(hipStreamSynchronize(s));
}

void tv1_fibres_vjp_steps(const unsigned *steps, const double *g, double *gx, double *gw, int *nseg, const int *ns, int nds, int dim,
                          hipStream_t s) {
    const FibreGeom geo = fibres_along(ns, nds, dim);
    if (geo.count <= 0 || geo.len <= 0) return;
    const int nch = (geo.len + kVjpL - 1) / kVjpL;
    if (!gx) {   // the segment counts alone: the words hold them
        if (!nseg) return;
        if (geo.inc == 1) hipLaunchKernelGGL(vjp_count_contig_kernel, dim3((unsigned)((geo.count + 3) / 4)), dim3(256), 0, s, steps, nch, geo.count, nseg);
        else              hipLaunchKernelGGL(vjp_count_strided_kernel, dim3((unsigned)((geo.count + 63) / 64)), dim3(64), 0, s, steps, nch, geo.count, nseg);
        PTV_HIP(hipGetLastError());
        PTV_HIP(hipStreamSynchronize(s));
        return;
    }
    const long units = vjp_units(geo);
    Scratch S(sizeof(Summary) * (size_t)units), R(sizeof(Resolved) * (size_t)units);
    if (geo.len == 1) gw = nullptr;   // no edges
    vjp_launch<VJP_PLAIN>(steps, g, gx, gw, nseg, geo, S.as<Summary>(), R.as<Resolved>(), VjpEpi{}, s);
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

// ---- what the forward keeps of one term's K sweeps ------------------------------------------------------------------------
//   TV-L1, tape = 0   K outputs                                          8 K n bytes
//   TV-L1, tape = 1   one array the sweeps reuse, K word arrays          8 n + 4 K words
//   TV-L2, any tape   K outputs and K multiplier arrays (one double per fibre): the derivative reads D y itself     8 K (n + fibres)
//   TV-Lp, any tape   K outputs, nothing else: the derivative needs the output, lambda and p alone                   8 K n
// Inside the one scratch block: every term's doubles, in the order of the terms, then every term's words.
struct SweepTape {
    bool l2 = false, gen = false;   // TV-L2 ; a general p (neither: TV-L1)
    double p = 1.0;
    int K = 0, tape = 0;
    size_t n = 0, fibres = 0, units = 0;   // samples ; fibres along the term's dimension ; step-code words of one output
    double *out = nullptr, *mus = nullptr;
    unsigned *words = nullptr;
    size_t doubles() const { return l2 ? (size_t)K * (n + fibres) : ((tape && !gen) ? n : (size_t)K * n); }
    size_t nwords() const { return (!l2 && !gen && tape) ? (size_t)K * units : 0; }
    double *y(int k) const { return out + ((l2 || gen || !tape) ? (size_t)k * n : 0); }
    double *mu(int k) const { return l2 ? mus + (size_t)k * fibres : nullptr; }
    unsigned *w(int k) const { return words ? words + (size_t)k * units : nullptr; }
    bool per_fibre() const { return l2 || gen; }   // one penalty gradient per fibre (TV-L1: per edge)
};

SweepTape sweep_tape(const int *ns, int nds, int dim, double norm, int K, int tape) {
    SweepTape t;
    const FibreGeom geo = fibres_along(ns, nds, dim);
    t.l2 = norm == 2;
    t.gen = norm != 1 && norm != 2;
    t.p = norm;
    t.K = K;
    t.tape = tape;
    if (geo.count <= 0 || geo.len <= 0) return t;
    t.n = (size_t)geo.count * (size_t)geo.len;
    t.fibres = (size_t)geo.count;
    t.units = (size_t)vjp_units(geo);
    return t;
}

size_t tape_bytes(const std::vector<SweepTape> &terms) {
    size_t d = 0, w = 0;
    for (const SweepTape &t : terms) {
        d += t.doubles();
        w += t.nwords();
    }
    return d * sizeof(double) + w * sizeof(unsigned);
}

void tape_carve(std::vector<SweepTape> &terms, double *block) {
    double *d = block;
    for (SweepTape &t : terms) {
        t.out = d;
        t.mus = t.l2 ? d + (size_t)t.K * t.n : nullptr;
        d += t.doubles();
    }
    unsigned *w = reinterpret_cast<unsigned *>(d);
    for (SweepTape &t : terms) {
        t.words = t.nwords() ? w : nullptr;
        w += t.nwords();
    }
}

// sweep k of a term, forward: its output (and, TV-L2, its multipliers) where the tape keeps them
void tape_prox(const double *in, const SweepTape &t, int k, const int *ns, int nds, int dim, double lam, const double *weights, hipStream_t s) {
    if (t.l2)       tv2_fibres(in, t.y(k), ns, nds, dim, lam, s, t.mu(k));
    else if (t.gen) tvp_fibres(in, t.y(k), nullptr, ns, nds, dim, lam, t.p, s);
    else            tv1_fibres(in, t.y(k), ns, nds, dim, lam, weights, s);
}

constexpr int tv2_mode_of(int mode) {
    return mode == VJP_DR_ROW ? TV2_VJP_DR_ROW : mode == VJP_DR_COL ? TV2_VJP_DR_COL : mode == VJP_PD2 ? TV2_VJP_PD2
         : mode == VJP_PD ? TV2_VJP_PD : TV2_VJP_PLAIN;
}

// ... and in reverse, a = J g with J that sweep's Jacobian and the write-out MODE: the segmented mean from the output or its words
// (gw: per edge), the TV-L2 derivative from the output and its multipliers, or the general-p one from the output alone (gw: per fibre)
template <int MODE>
void tape_vjp(const SweepTape &t, int k, const double *g, double *gx, double *gw, const int *ns, int nds, int dim, double lam, const FibreGeom &geo,
              Summary *S, Resolved *R, const VjpEpi &epi, hipStream_t s) {
    if (!t.per_fibre()) {
        vjp_launch_taped<MODE>(t.y(k), t.w(k), g, gx, gw, geo, S, R, epi, s);
        return;
    }
    Tv2VjpEpi e;
    e.mode = tv2_mode_of(MODE);
    e.gU = epi.gU;
    e.c = epi.c;
    e.final = epi.final;
    e.add_glam = epi.add_gw;
    e.zeta = epi.zeta;
    e.scale = epi.scale;
    if (t.l2) tv2_fibres_vjp_epi(t.y(k), t.mu(k), g, gx, gw, ns, nds, dim, lam, e, s);
    else      tvp_fibres_vjp_epi(t.y(k), g, gx, gw, ns, nds, dim, lam, t.p, e, s);
}

}  // namespace

// bytes = sum over the two directions d (n = M N B, K = maxit + 1):  TV-L1, tape 0: 8 K n ;  TV-L1, tape 1: 8 n + 4 K words_d ;
// TV-L2: 8 K (n + fibres_d), fibres_0 = N B, fibres_1 = M B ;  a general p: 8 K n
size_t dr2_vjp_tape_bytes(size_t M, size_t N, size_t B, int maxit, int tape, double norm1, double norm2) {
    if (maxit <= 0) maxit = MAX_ITERS_DR;
    const int ns[3] = {(int)M, (int)N, (int)B};
    return tape_bytes({sweep_tape(ns, 3, 0, norm1, maxit + 1, tape), sweep_tape(ns, 3, 1, norm2, maxit + 1, tape)});
}

// Forward: the recurrence of dr2_norms (solvers.hip) on B stacked images with the sweep outputs x1_k, x2_k kept, k = 0 .. maxit (the last
// pair: the final sweeps); nothing else is needed afterwards, where P_c / P_r are read off those outputs.
//   t = 2 mean(U) ; repeat: x1 = prox_c(t), x2 = prox_r(U - t + 2 x1), t <- t - x1 + x2 ; x1 = prox_c(t), out = x2 = prox_r(U - t + x1)
// Reverse, for the cotangent g of out (gbar: the cotangent of t; every line one launch of three phases):
//   final  a = P_r g : gU = a, c = a, gbar = -a, gW2 = gw    |  d = P_c c : gbar += d, gW1 = gw
//   k = maxit-1 .. 0
//          a = P_r gbar : gU += a, c = 2 a - gbar, gbar -= a, gW2 += gw   |  d = P_c c : gbar += d, gW1 += gw
//   end    gU += 2 sum(gbar) / (M N) per image
// tape = 1: x1_k and x2_k are written into two arrays that every iteration reuses and encoded behind their sweep (vjp_encode); the
// reverse loop is the same with the words of sweep k where y was.
void dr2_vjp(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, const double *W1m, const double *W2m, const double *g,
             double *out, double *gU, double *gW1, double *gW2, double *glam, int maxit, int tape, hipStream_t s, double norm1, double norm2) {
    const long n1 = (long)(M * N), n = n1 * (long)B;
    const bool l2c = norm1 != 1, l2r = norm2 != 1;   // (a TV-L2 or general-p direction: one uniform image, no per-edge gradients)
    if (l2c) gW1 = nullptr;
    if (l2r) gW2 = nullptr;
    if (maxit <= 0) maxit = MAX_ITERS_DR;
    if (n == 0) return;
    const int ns[3] = {(int)M, (int)N, (int)B};
    const FibreGeom cols = fibres_along(ns, 3, 0), rows = fibres_along(ns, 3, 1);
    // what a direction's penalty gradient is summed from, per image: its edges (TV-L1) or its fibres (TV-L2)
    const long e1 = l2c ? cols.count : (long)((M - 1) * N), e2 = l2r ? rows.count : (long)(M * (N - 1));
    const size_t bytes = sizeof(double) * (size_t)n;

    std::vector<SweepTape> kept_of{sweep_tape(ns, 3, 0, norm1, maxit + 1, tape), sweep_tape(ns, 3, 1, norm2, maxit + 1, tape)};
    Scratch kept(tape_bytes(kept_of)), t(bytes), v(bytes);
    Scratch partials(sizeof(double) * kReduceBlocks * B), sums(sizeof(double) * 2 * B);
    tape_carve(kept_of, kept.d());
    const SweepTape &tc = kept_of[0], &tr = kept_of[1];
    auto x1 = [&](int k) { return tc.y(k); };
    auto x2 = [&](int k) { return tr.y(k); };
    {   // seed of the geometry policy, like dr2: the image's edge statistics (the first array a sweep sees here is the constant t0)
        const int both[2] = {0, 1};
        const double *const wts[2] = {W1m, W2m};
        policy_probe(unary, wts, ns, 3, both, 2, s);
    }
    sum_to(unary, n1, (long)B, partials.d(), sums.d(), s);
    dr_fill(t.d(), n1, (long)B, sums.d(), 1.0, s);
    for (int k = 0; k <= maxit; k++) {
        const bool last = k == maxit;
        tape_prox(t.d(), tc, k, ns, 3, 0, W1, W1m, s);
        lincomb(v.d(), unary, 1.0, t.d(), -1.0, x1(k), last ? 1.0 : 2.0, nullptr, 0, n, s);
        tape_prox(v.d(), tr, k, ns, 3, 1, W2, W2m, s);
        if (!last) lincomb(t.d(), t.d(), 1.0, x1(k), -1.0, x2(k), 1.0, nullptr, 0, n, s);
        if (tc.w(k)) vjp_encode(x1(k), tc.w(k), cols, s);
        if (tr.w(k)) vjp_encode(x2(k), tr.w(k), rows, s);
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
        tape_vjp<VJP_DR_ROW>(tr, k, row.final ? g : gbar, gbar, w2, ns, 3, 1, W2, rows, S.as<Summary>(), R.as<Resolved>(), row, s);
        tape_vjp<VJP_DR_COL>(tc, k, c, gbar, w1, ns, 3, 0, W1, cols, S.as<Summary>(), R.as<Resolved>(), col, s);
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

// ---- the derivative of the Dykstra loops behind tvgen ------------------------------------------------------------------------------
namespace {

long total(const int *ns, int nds) {
    long n = 1;
    for (int i = 0; i < nds; i++) n *= ns[i];
    return n;
}

}  // namespace

namespace {

std::vector<SweepTape> pd_tapes(int which, const double *dims, const double *norms, const int *ns, int nds, int npen, int iters, int tape) {
    const int K = (which == 0 && npen == 1) ? 1 : iters;   // (one term: every iteration repeats the first)
    std::vector<SweepTape> terms;
    for (int i = 0; i < npen; i++) terms.push_back(sweep_tape(ns, nds, (int)(dims[i] - 1), norms ? norms[i] : 1.0, K, tape));
    return terms;
}

}  // namespace

// bytes = sum over the terms i (n the array's size, K = iters, or 1 for which = 0 with one term):  TV-L1, tape 0: 8 K n ;
// TV-L1, tape 1: 8 n + 4 K words_i ;  TV-L2: 8 K (n + fibres_i), fibres_i = n / ns[dims[i] - 1] ;  a general p: 8 K n
size_t pd_vjp_tape_bytes(int which, const double *dims, const int *ns, int nds, int npen, int iters, int tape, const double *norms) {
    return tape_bytes(pd_tapes(which, dims, norms, ns, nds, npen, iters, tape));
}

namespace {

// the edges along a term's dimension, and what gw of a sweep along it is handed (null: nobody asks, or there are none)
struct TermGw {
    long edges = 0;
    std::unique_ptr<Scratch> buf;
    double *d() const { return buf ? buf->d() : nullptr; }
};
void term_gw(TermGw &t, const FibreGeom &geo, bool wanted, bool l2 = false) {
    t.edges = l2 ? geo.count : geo.count * (long)(geo.len - 1);   // (a TV-L2 or general-p sweep hands out one value per fibre)
    if (wanted && t.edges > 0) t.buf.reset(new Scratch(sizeof(double) * (size_t)t.edges));
}
// glam[i] = the sum of term i's per-edge gradients, in sum_to's fixed layout (0 where there are no edges)
void sum_terms(const std::vector<TermGw> &gw, double *glam, hipStream_t s) {
    const size_t P = gw.size();
    Scratch partials(sizeof(double) * kReduceBlocks), sums(sizeof(double) * P);
    std::vector<double> h(P, 0.0);
    for (size_t i = 0; i < P; i++) {
        if (!gw[i].d()) continue;
        sum_to(gw[i].d(), gw[i].edges, 1, partials.d(), sums.d() + i, s);
        PTV_HIP(hipMemcpyAsync(&h[i], sums.d() + i, sizeof(double), hipMemcpyDeviceToHost, s));
    }
    PTV_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < P; i++) glam[i] = h[i];
}

// Two-term proximal Dykstra (pd2 of solvers.hip, TV-L1 terms), K iterations with the sweep outputs z_k, x'_k kept:
//   x = y, p = q = 0 ; repeat: z = prox_0(x + p), p += x - z ; x' = prox_1(z + q), q += z - x' ; x = x'
// Reverse.  With X, Pb, Qb the cotangents of x, p, q (X = g, Pb = Qb = 0 behind the last iteration), an iteration is
//   a = P_1 (X - Qb) ; Zc = a + Qb - Pb ; Qb += a ; b = P_0 Zc ; X = Pb = Pb + b
// X and Pb are one array from the first reverse iteration on, so the state is X and the difference D = X - Qb, and in those
//   a = P_1 D ; Zc = a - D  (last iteration: Zc = a) ; b = P_0 Zc ; X += b  (last: X = b) ; D = b - Zc
// two launches of three phases, D rewritten in place by both, X = gy touched by the second alone.  One term: a single sweep.
// tape = 1: z and x' are two arrays that every iteration reuses, encoded behind their sweep (x' is still read by the next iteration's
// first two steps, which is before its sweep rewrites it).
void pd2_vjp(const double *y, const double *lambdas, const double *dims, const int *ns, int nds, int npen, int K, const double *g, double *x,
             double *gy, double *glam, int tape, hipStream_t s, const double *norms) {
    const long n = total(ns, nds);
    const size_t bytes = sizeof(double) * (size_t)n;
    const int d0 = (int)(dims[0] - 1), d1 = npen >= 2 ? (int)(dims[1] - 1) : d0;
    const FibreGeom g0 = fibres_along(ns, nds, d0), g1 = fibres_along(ns, nds, d1);
    std::vector<SweepTape> kept_of = pd_tapes(0, dims, norms, ns, nds, npen, K, tape);
    Scratch kept(tape_bytes(kept_of));
    tape_carve(kept_of, kept.d());
    const SweepTape &t0 = kept_of[0], &t1 = kept_of[npen >= 2 ? 1 : 0];
    std::vector<TermGw> gw((size_t)npen);
    term_gw(gw[0], g0, glam != nullptr, t0.per_fibre());
    if (npen >= 2) term_gw(gw[1], g1, glam != nullptr, t1.per_fibre());
    const long units = std::max(vjp_units(g0), vjp_units(g1));
    Scratch S(sizeof(Summary) * (size_t)units), R(sizeof(Resolved) * (size_t)units);
    if (npen == 1) {   // (x + p stays y: every iteration repeats the first)
        tape_prox(y, t0, 0, ns, nds, d0, lambdas[0], nullptr, s);
        if (t0.w(0)) vjp_encode(t0.y(0), t0.w(0), g0, s);
        if (x) PTV_HIP(hipMemcpyAsync(x, t0.y(0), bytes, hipMemcpyDeviceToDevice, s));
        tape_vjp<VJP_PLAIN>(t0, 0, g, gy, gw[0].d(), ns, nds, d0, lambdas[0], g0, S.as<Summary>(), R.as<Resolved>(), VjpEpi{}, s);
    } else {
        Scratch t(bytes), p(bytes), q(bytes);
        auto zk = [&](int k) { return t0.y(k); };
        auto xk = [&](int k) { return t1.y(k); };
        const double *xc = y;
        for (int k = 0; k < K; k++) {
            if (k == 0) {   // p = q = 0
                tape_prox(y, t0, 0, ns, nds, d0, lambdas[0], nullptr, s);
                lincomb(p.d(), y, 1.0, zk(0), -1.0, nullptr, 0, nullptr, 0, n, s);
                tape_prox(zk(0), t1, 0, ns, nds, d1, lambdas[1], nullptr, s);
                lincomb(q.d(), zk(0), 1.0, xk(0), -1.0, nullptr, 0, nullptr, 0, n, s);
            } else {
                lincomb(t.d(), xc, 1.0, p.d(), 1.0, nullptr, 0, nullptr, 0, n, s);
                tape_prox(t.d(), t0, k, ns, nds, d0, lambdas[0], nullptr, s);
                lincomb(p.d(), p.d(), 1.0, xc, 1.0, zk(k), -1.0, nullptr, 0, n, s);
                lincomb(t.d(), zk(k), 1.0, q.d(), 1.0, nullptr, 0, nullptr, 0, n, s);
                tape_prox(t.d(), t1, k, ns, nds, d1, lambdas[1], nullptr, s);
                lincomb(q.d(), q.d(), 1.0, zk(k), 1.0, xk(k), -1.0, nullptr, 0, n, s);
            }
            if (t0.w(k)) vjp_encode(zk(k), t0.w(k), g0, s);
            if (t1.w(k)) vjp_encode(xk(k), t1.w(k), g1, s);
            xc = xk(k);
        }
        if (x) PTV_HIP(hipMemcpyAsync(x, xc, bytes, hipMemcpyDeviceToDevice, s));
        double *D = t.d();   // t is free again
        for (int k = K - 1; k >= 0; k--) {
            VjpEpi second, first;
            second.final = first.final = k == K - 1;
            second.add_gw = first.add_gw = k != K - 1;
            first.gU = gy;
            tape_vjp<VJP_PD2>(t1, k, second.final ? g : D, D, gw[1].d(), ns, nds, d1, lambdas[1], g1, S.as<Summary>(), R.as<Resolved>(), second, s);
            tape_vjp<VJP_PD2>(t0, k, D, D, gw[0].d(), ns, nds, d0, lambdas[0], g0, S.as<Summary>(), R.as<Resolved>(), first, s);
        }
    }
    if (glam) sum_terms(gw, glam, s);
    PTV_HIP(hipStreamSynchronize(s));   // (the scratch goes back to the pool behind this)
}

// Parallel proximal Dykstra (pd_like(false, ...) of solvers.hip, TV-L1 terms), K iterations with the P sweep outputs p_i^k kept:
//   z_i = y ; repeat: p_i = prox_i(z_i) ; x = sum_i p_i / P ; z_i += x - p_i          (the combine is the fused loop's own kernel)
// Reverse, zeta_i the cotangent of z_i (0 behind the last iteration) and chi = [g, the last iteration] + sum_i zeta_i:
//   for every i:  pi = chi / P - zeta_i ; a = P_i pi ; zeta_i += a ; chi' (+)= zeta_i             end: gy = chi'
// one launch of three phases per term: pi is formed on load in phases A and C (chi is read by every term, so the sum for the next
// iteration grows in a second array; the two change places), zeta_i is rewritten in place in the arrays the forward kept z_i in.
// tape = 1: the p_i of an iteration live in P arrays that every iteration reuses (the combine needs all of them), each encoded behind
// its sweep.
void pdp_vjp(const double *y, const double *lambdas, const double *dims, const int *ns, int nds, int P, int K, const double *g, double *x,
             double *gy, double *glam, int tape, hipStream_t s, const double *norms) {
    const long n = total(ns, nds);
    const size_t bytes = sizeof(double) * (size_t)n;
    std::vector<SweepTape> kept_of = pd_tapes(1, dims, norms, ns, nds, P, K, tape);
    Scratch kept(tape_bytes(kept_of));
    tape_carve(kept_of, kept.d());
    auto pk = [&](int k, int i) { return kept_of[(size_t)i].y(k); };
    auto ck = [&](int k, int i) { return kept_of[(size_t)i].w(k); };
    std::vector<std::unique_ptr<Scratch>> z;
    std::vector<FibreGeom> geo;
    std::vector<TermGw> gw((size_t)P);
    long units = 0;
    for (int i = 0; i < P; i++) {
        z.emplace_back(new Scratch(bytes));
        geo.push_back(fibres_along(ns, nds, (int)(dims[i] - 1)));
        term_gw(gw[(size_t)i], geo.back(), glam != nullptr, kept_of[(size_t)i].per_fibre());
        units = std::max(units, vjp_units(geo.back()));
        PTV_HIP(hipMemcpyAsync(z.back()->d(), y, bytes, hipMemcpyDeviceToDevice, s));
    }
    Scratch xa(bytes), xb(bytes), partials(sizeof(double) * kReduceBlocks), acc(sizeof(double));
    // more terms than a kernel-argument pack holds: the combine reads its addresses from a table in HBM, [P] p_i^k then [P] z_i per iteration
    std::unique_ptr<Scratch> table;
    if (P > kMaxTerms) {
        std::vector<double *> host;
        for (int k = 0; k < K; k++) {
            for (int i = 0; i < P; i++) host.push_back(pk(k, i));
            for (int i = 0; i < P; i++) host.push_back(z[(size_t)i]->d());
        }
        table.reset(new Scratch(sizeof(double *) * host.size()));
        PTV_HIP(hipMemcpyAsync(table->as<double *>(), host.data(), sizeof(double *) * host.size(), hipMemcpyHostToDevice, s));
        PTV_HIP(hipStreamSynchronize(s));   // (`host` lives on this frame)
    }
    PTV_HIP(hipMemsetAsync(xa.d(), 0, bytes, s));
    for (int k = 0; k < K; k++) {
        PtrPack pp{}, zp{};
        for (int i = 0; i < P; i++) {
            tape_prox(z[(size_t)i]->d(), kept_of[(size_t)i], k, ns, nds, (int)(dims[i] - 1), lambdas[i], nullptr, s);
            if (ck(k, i)) vjp_encode(pk(k, i), ck(k, i), geo[(size_t)i], s);
            if (i < kMaxTerms) {
                pp.v[i] = pk(k, i);
                zp.v[i] = z[(size_t)i]->d();
            }
        }
        if (table) pd_combine_many(table->as<double *>() + (size_t)k * 2 * (size_t)P, xa.d(), xa.d(), P, n, partials.d(), acc.d(), false, s);
        else       pd_combine(pp, zp, xa.d(), xa.d(), P, n, partials.d(), acc.d(), s);
    }
    if (x) PTV_HIP(hipMemcpyAsync(x, xa.d(), bytes, hipMemcpyDeviceToDevice, s));

    Scratch S(sizeof(Summary) * (size_t)units), R(sizeof(Resolved) * (size_t)units);
    const double *chi = g;
    double *next = nullptr;
    for (int k = K - 1; k >= 0; k--) {
        // the last sum is gy itself, unless gy is the g that a single iteration is still reading
        if (k == 0) next = (gy == g && K == 1) ? xa.d() : gy;
        else        next = chi == xa.d() ? xb.d() : xa.d();
        for (int i = 0; i < P; i++) {
            VjpEpi e;
            e.zeta = k == K - 1 ? nullptr : z[(size_t)i]->d();
            e.scale = 1.0 / P;
            e.gU = next;
            e.final = i == 0;
            e.add_gw = k != K - 1;
            tape_vjp<VJP_PD>(kept_of[(size_t)i], k, chi, z[(size_t)i]->d(), gw[(size_t)i].d(), ns, nds, (int)(dims[i] - 1), lambdas[i], geo[(size_t)i],
                             S.as<Summary>(), R.as<Resolved>(), e, s);
        }
        chi = next;
    }
    if (next != gy) PTV_HIP(hipMemcpyAsync(gy, next, bytes, hipMemcpyDeviceToDevice, s));
    if (glam) sum_terms(gw, glam, s);
    PTV_HIP(hipStreamSynchronize(s));   // (the scratch goes back to the pool behind this)
}

}  // namespace

void pd_vjp(int which, const double *y, const double *lambdas, const double *dims, const int *ns, int nds, int npen, int iters, const double *g,
            double *x, double *gy, double *glam, int tape, hipStream_t s, const double *norms) {
    if (total(ns, nds) == 0) return;
    if (which == 0) pd2_vjp(y, lambdas, dims, ns, nds, npen, iters, g, x, gy, glam, tape, s, norms);
    else            pdp_vjp(y, lambdas, dims, ns, nds, npen, iters, g, x, gy, glam, tape, s, norms);
}

}  // namespace ptv
