// jvp.hip -- forward-mode derivatives: the tangent of the batched 1-D TV-L1 prox (proxtv_tv1_fibres_jvp_dev) and of the
// 2-D Douglas-Rachford solve (proxtv_DR2_TV_jvp_dev).
//
// The fibre tangent is dy = P (dx + E(sigma, dr)) (jvpcore.hpp): the segmented mean of vjp.hip applied to a vector that is formed on
// load.  So the three phases are vjp.hip's -- A: a Summary per chunk of kVjpChunk samples, B: vjp_resolve, shared and unchanged, C: the
// means written out -- in the same two geometries, with kernels of their own for A and C whose load is jvpcore.hpp's:
//   strided fibres      64 adjacent fibres per wave, a lane walks its chunk from global memory (chunk_load_tangent: E from the chunk's
//                       masks; the sigma of the edge before the chunk from the sample in front of it, y[first - inc])
//   contiguous fibres   a wave stages 64 consecutive chunks through LDS rows of kVjpChunk + 1 doubles; the staging loop meets every sample
//                       once, coalesced, and forms E there (sample_term, from y[i - 1], y[i], y[i + 1]: the neighbours are the same
//                       cache lines), so the tile holds v and the lanes run the plain chunk_load on it
// dr is dlam on every edge plus, when given, a per-edge array laid out as the prox's weights (gw of the VJP).  The tangent dx may be a
// combination of up to three arrays (jvpcore.hpp: Comb), formed inside the loads or by one pointwise pass in front (jvp_comb_kernel, the
// same expression: the same bits).  No atomics: every element is written by one lane and every sum has one order.
//
// The Douglas-Rachford tangent runs next to the unfused forward recurrence, sweep by sweep (dr2_jvp below): nothing is taped.
#include "jvp.hpp"
#include "jvpcore.hpp"

#include <algorithm>
#include <memory>

#include "pointwise.hpp"
#include "policy.hpp"
#include "solvers.hpp"
#include "sweep.hpp"

namespace ptv {

namespace {

using vjp::Chunk;
using vjp::Resolved;
using vjp::Summary;

constexpr int kJvpL = kVjpChunk;
constexpr int kJvpRow = kJvpL + 1;   // LDS row of the contiguous kernel: the chunk plus the next sample's y; odd, so conflict-free
static_assert((kJvpL & (kJvpL - 1)) == 0, "the staging loops split an element index by shifts");

// What a launch does: phase A, or phase C with one of two write-outs of a = P v.
//   JVP_PLAIN    dy = a                         (the fibre call; the column sweeps of a Douglas-Rachford iteration: dx1; its final row sweep)
//   JVP_DR_ROW   dt <- dt - dx1 + a             (the row sweep of an iteration: a is dx2, which nothing else reads and which is not stored)
enum { JVP_SUMMARY = 0, JVP_PLAIN = 1, JVP_DR_ROW = 2 };
struct JvpIn {
    jvp::Comb v;                  // the tangent in x
    const double *dw = nullptr;   // per-edge penalty tangent, or null
    double dlam = 0.0;            // ... plus this on every edge
    int inject = 0;               // 0: every dr is zero, E is left out
};
struct JvpEpi {
    double *dt = nullptr;
    const double *dx1 = nullptr;
};

template <int MODE>
__device__ __forceinline__ void jvp_store(const JvpEpi &e, double *dy, long i, double a) {
    if constexpr (MODE == JVP_DR_ROW) e.dt[i] = e.dt[i] - e.dx1[i] + a;
    else dy[i] = a;
}

// ---- strided fibres: wave = 64 adjacent fibres x one chunk; S and R at chunk * count + fibre ------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void jvp_strided_kernel(const double *y, JvpIn in, double *dy, FibreGeom geo, int nch, Summary *S,
                                                          const Resolved *R, JvpEpi epi) {
    const long unit = (long)blockIdx.x * 4 + (threadIdx.x >> 6), groups = (geo.count + 63) / 64;
    if (unit >= groups * nch) return;
    long grp, c;
    divmod_nonneg(unit, (long)nch, grp, c);
    const long j = grp * 64 + (threadIdx.x & 63);
    if (j >= geo.count) return;
    long blk, off;
    divmod_nonneg(j, geo.inc, blk, off);
    const int k0 = (int)c * kJvpL, clen = min(kJvpL, geo.len - k0);
    const bool has_next = k0 + clen < geo.len, has_prev = k0 > 0;
    const long inc = geo.inc, base = blk * inc * geo.len + off + (long)k0 * inc;
    const long wbase = blk * inc * (geo.len - 1) + off + (long)k0 * inc;   // the edge behind the chunk's first sample
    const long idx = c * geo.count + j;
    Chunk<kJvpL> ch;
    const double yprev = has_prev ? y[base - inc] : 0.0;
    jvp::chunk_load_tangent(
        ch, clen, has_next, has_prev, yprev, in.inject != 0, [&](int k) { return y[base + (long)k * inc]; },
        [&](int k) { return jvp::comb_at(in.v, base + (long)k * inc); },
        [&](int k) { return (in.dw ? in.dw[wbase + (long)k * inc] : 0.0) + in.dlam; });
    vjp::chunk_prefix(ch);
    if (MODE == JVP_SUMMARY) {
        S[idx] = vjp::chunk_summary(ch);
        return;
    }
    vjp::chunk_means(ch, R[idx], false, [](int, double) {});
#pragma unroll
    for (int k = 0; k < kJvpL; k++)
        if (k < clen) jvp_store<MODE>(epi, dy, base + (long)k * inc, ch.g[k]);
}

// ---- contiguous fibres: wave = 64 consecutive chunks staged through LDS; S and R at fibre * nch + chunk ---------------------------------
template <int MODE>
__global__ __launch_bounds__(64) void jvp_contig_kernel(const double *y, JvpIn in, double *dy, int len, long count, int nch, Summary *S,
                                                        const Resolved *R, JvpEpi epi) {
    __shared__ double ty[64 * kJvpRow], tg[64 * kJvpRow];
    const int lane = threadIdx.x;
    const long unit = (long)blockIdx.x * 64 + lane;
    const bool valid = unit < count * nch;
    long j = 0, c = 0;
    if (valid) divmod_nonneg(unit, (long)nch, j, c);
    const int k0 = (int)c * kJvpL, clen = valid ? min(kJvpL, len - k0) : 0;
    const bool has_next = valid && k0 + clen < len;
    const long base = j * len + k0, wbase = j * (len - 1) + k0;
    // rows in: element e of the tile is sample e % L of the chunk of lane e / L; v = the tangent in x plus E of that sample
#pragma unroll
    for (int i = 0; i < kJvpL; i++) {
        const int e = i * 64 + lane, src = e / kJvpL, k = e % kJvpL;
        const long b = __shfl(base, src), wb = __shfl(wbase, src);
        const int n = __shfl(clen, src), p = __shfl(k0, src) + k;   // p: the sample's place in its fibre
        if (k < n) {
            const long g = b + k;
            const double yi = y[g];
            double v = jvp::comb_at(in.v, g);
            if (in.inject) {
                const bool hp = p > 0, hn = p < len - 1;
                const double dp = hp ? (in.dw ? in.dw[wb + k - 1] : 0.0) + in.dlam : 0.0;
                const double dh = hn ? (in.dw ? in.dw[wb + k] : 0.0) + in.dlam : 0.0;
                v += jvp::sample_term(hp, hp ? y[g - 1] : 0.0, yi, hn, hn ? y[g + 1] : 0.0, dp, dh);
            }
            ty[src * kJvpRow + k] = yi;
            tg[src * kJvpRow + k] = v;
        }
    }
    if (has_next) ty[lane * kJvpRow + clen] = y[base + clen];
    __syncthreads();
    Chunk<kJvpL> ch;
    if (valid) {
        const double *my = ty + lane * kJvpRow, *mg = tg + lane * kJvpRow;
        vjp::chunk_load(ch, clen, has_next, [&](int k) { return my[k]; }, [&](int k) { return mg[k]; });
        vjp::chunk_prefix(ch);
    }
    if (MODE == JVP_SUMMARY) {
        if (valid) S[unit] = vjp::chunk_summary(ch);
        return;
    }
    // rows out, through the tile v came in by; the row epilogue's operands meet the means in the coalesced loop below
    if (valid) {
        double *mg = tg + lane * kJvpRow;
        vjp::chunk_means(ch, R[unit], false, [](int, double) {});
#pragma unroll
        for (int k = 0; k < kJvpL; k++)
            if (k < clen) mg[k] = ch.g[k];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kJvpL; i++) {
        const int e = i * 64 + lane, src = e / kJvpL, k = e % kJvpL;
        const long b = __shfl(base, src);
        if (k < __shfl(clen, src)) jvp_store<MODE>(epi, dy, b + k, tg[src * kJvpRow + k]);
    }
}

// out = the combination, one element per lane: the pointwise pass of the second route
__global__ __launch_bounds__(256) void jvp_comb_kernel(double *out, jvp::Comb q, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = jvp::comb_at(q, i);
}

void jvp_comb(double *out, const jvp::Comb &q, long n, hipStream_t s) {
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(jvp_comb_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, out, q, n);
    PTV_HIP(hipGetLastError());
}

long jvp_units(const FibreGeom &geo) { return geo.count * ((geo.len + kJvpL - 1) / kJvpL); }

// phases A, B and C<MODE> of one sweep's tangent on the stream; S and R hold jvp_units(geo) records
template <int MODE>
void jvp_launch(const double *y, const JvpIn &in, double *dy, const FibreGeom &geo, Summary *S, Resolved *R, const JvpEpi &epi, hipStream_t s) {
    const int nch = (geo.len + kJvpL - 1) / kJvpL;
    const long units = geo.count * nch;
    if (geo.inc == 1) {
        const unsigned blocks = (unsigned)((units + 63) / 64);
        hipLaunchKernelGGL((jvp_contig_kernel<JVP_SUMMARY>), dim3(blocks), dim3(64), 0, s, y, in, dy, geo.len, geo.count, nch, S, R, JvpEpi{});
        vjp_resolve(S, R, geo, nullptr, s);
        hipLaunchKernelGGL((jvp_contig_kernel<MODE>), dim3(blocks), dim3(64), 0, s, y, in, dy, geo.len, geo.count, nch, S, R, epi);
    } else {
        const long waves = ((geo.count + 63) / 64) * nch;
        const unsigned blocks = (unsigned)((waves + 3) / 4);
        hipLaunchKernelGGL((jvp_strided_kernel<JVP_SUMMARY>), dim3(blocks), dim3(256), 0, s, y, in, dy, geo, nch, S, R, JvpEpi{});
        vjp_resolve(S, R, geo, nullptr, s);
        hipLaunchKernelGGL((jvp_strided_kernel<MODE>), dim3(blocks), dim3(256), 0, s, y, in, dy, geo, nch, S, R, epi);
    }
    PTV_HIP(hipGetLastError());
}

JvpIn jvp_in(const jvp::Comb &v, const double *dw, double dlam, const FibreGeom &geo) {
    JvpIn in;
    in.v = v;
    in.dw = geo.len > 1 ? dw : nullptr;   // (no edges: nothing to read)
    in.dlam = dlam;
    in.inject = geo.len > 1 && (in.dw != nullptr || dlam != 0.0);
    return in;
}

jvp::Comb comb1(const double *a) {
    jvp::Comb q;
    q.a = a;
    q.ca = 1.0;
    return q;
}

}  // namespace

void tv1_fibres_jvp(const double *y, const double *dx, const double *dw, double dlam, double *dy, const int *ns, int nds, int dim,
                    hipStream_t s) {
    const FibreGeom geo = fibres_along(ns, nds, dim);
    if (geo.count <= 0 || geo.len <= 0) return;
    const long units = jvp_units(geo);
    Scratch S(sizeof(Summary) * (size_t)units), R(sizeof(Resolved) * (size_t)units);
    jvp_launch<JVP_PLAIN>(y, jvp_in(comb1(dx), dw, dlam, geo), dy, geo, S.as<Summary>(), R.as<Resolved>(), JvpEpi{}, s);
    PTV_HIP(hipStreamSynchronize(s));   // (the scratch goes back to the pool behind this)
}

// ---- the tangent of the 2-D Douglas-Rachford solve ---------------------------------------------------------------------------------
// six arrays of the data's size (t, v, x1, x2, dt, dx1; x2 is the caller's `out` when there is one), the chunk records of the longer
// direction, the reduction's partial sums.  (The forward sweeps' own persistent state -- link codes, flags -- is theirs, as in dr2.)
size_t dr2_jvp_scratch_bytes(size_t M, size_t N, size_t B) {
    const size_t n = M * N * B;
    if (n == 0) return 0;
    const int ns[3] = {(int)M, (int)N, (int)B};
    const long units = std::max(jvp_units(fibres_along(ns, 3, 0)), jvp_units(fibres_along(ns, 3, 1)));
    return 6 * sizeof(double) * n + (sizeof(Summary) + sizeof(Resolved)) * (size_t)units + sizeof(double) * (kReduceBlocks + 2) * B;
}

// The recurrence of dr2_vjp's forward (vjp.hip) with the tangent of every sweep formed behind it, from that sweep's output:
//   t = 2 mean(U), dt = 2 mean(dU) ;
//   repeat: x1 = prox_c(t), dx1 = P_c(x1)[dt + E(dW1)] ; x2 = prox_r(U - t + 2 x1), dx2 = P_r(x2)[dU - dt + 2 dx1 + E(dW2)] ;
//           t <- t - x1 + x2, dt <- dt - dx1 + dx2                                  (the dt update rides in the row sweep's phase C)
//   x1, dx1 as above ; out = x2 = prox_r(U - t + x1), ds = P_r(x2)[dU - dt + dx1 + E(dW2)]
// The row sweeps' three-array combination is formed inside the loads of phases A and C or by one pointwise pass into v, which is free
// once x2 is there (option dr_jvp_route; policy.hpp has the default and its measurement): the same bits either way.
void dr2_jvp(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, const double *W1m, const double *W2m, const double *dU,
             const double *dW1m, const double *dW2m, double dW1, double dW2, double *out, double *ds, int maxit, hipStream_t s) {
    const long n1 = (long)(M * N), n = n1 * (long)B;
    if (maxit <= 0) maxit = MAX_ITERS_DR;
    if (n == 0) return;
    const int ns[3] = {(int)M, (int)N, (int)B};
    const FibreGeom cols = fibres_along(ns, 3, 0), rows = fibres_along(ns, 3, 1);
    const size_t bytes = sizeof(double) * (size_t)n;
    Scratch t(bytes), v(bytes), x1(bytes), dt(bytes), dx1(bytes);
    std::unique_ptr<Scratch> own;
    if (!out) own.reset(new Scratch(bytes));
    double *x2 = out ? out : own->d();
    Scratch partials(sizeof(double) * kReduceBlocks * B), sums(sizeof(double) * 2 * B);
    const long units = std::max(jvp_units(cols), jvp_units(rows));
    Scratch S(sizeof(Summary) * (size_t)units), R(sizeof(Resolved) * (size_t)units);
    {   // seed of the geometry policy, as dr2_vjp's forward has it
        const int both[2] = {0, 1};
        const double *const wts[2] = {W1m, W2m};
        policy_probe(unary, wts, ns, 3, both, 2, s);
    }
    sum_to(unary, n1, (long)B, partials.d(), sums.d(), s);
    dr_fill(t.d(), n1, (long)B, sums.d(), 1.0, s);
    if (dU) {
        sum_to(dU, n1, (long)B, partials.d(), sums.d(), s);
        dr_fill(dt.d(), n1, (long)B, sums.d(), 1.0, s);
    } else {
        PTV_HIP(hipMemsetAsync(dt.d(), 0, bytes, s));
    }
    const int route = options().dr_jvp_route;
    const bool in_loads = route == 1 || (route != 2 && kDrJvpCombineInLoads);
    const JvpIn col_in = jvp_in(comb1(dt.d()), dW1m, dW1, cols);
    for (int k = 0; k <= maxit; k++) {
        const bool last = k == maxit;
        tv1_fibres(t.d(), x1.d(), ns, 3, 0, W1, W1m, s);
        jvp_launch<JVP_PLAIN>(x1.d(), col_in, dx1.d(), cols, S.as<Summary>(), R.as<Resolved>(), JvpEpi{}, s);
        lincomb(v.d(), unary, 1.0, t.d(), -1.0, x1.d(), last ? 1.0 : 2.0, nullptr, 0, n, s);
        tv1_fibres(v.d(), x2, ns, 3, 1, W2, W2m, s);
        jvp::Comb q;
        q.a = dU;
        q.ca = 1.0;
        q.b = dt.d();
        q.cb = -1.0;
        q.c = dx1.d();
        q.cc = last ? 1.0 : 2.0;
        if (!in_loads) {
            jvp_comb(v.d(), q, n, s);
            q = comb1(v.d());
        }
        const JvpIn row_in = jvp_in(q, dW2m, dW2, rows);
        if (last) {
            jvp_launch<JVP_PLAIN>(x2, row_in, ds, rows, S.as<Summary>(), R.as<Resolved>(), JvpEpi{}, s);
        } else {
            JvpEpi epi;
            epi.dt = dt.d();
            epi.dx1 = dx1.d();
            jvp_launch<JVP_DR_ROW>(x2, row_in, nullptr, rows, S.as<Summary>(), R.as<Resolved>(), epi, s);
            lincomb(t.d(), t.d(), 1.0, x1.d(), -1.0, x2, 1.0, nullptr, 0, n, s);
        }
    }
    PTV_HIP(hipStreamSynchronize(s));   // (the scratch goes back to the pool behind this)
}

}  // namespace ptv
