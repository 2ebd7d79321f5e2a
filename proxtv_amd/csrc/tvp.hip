// tvp.hip -- batched 1-D TV-Lp prox over the fibres of an N-D array for general p (the reference's GP_TVp / FW_TVp / GPFW_TVp arm of
// TV(), src/TVLPopt.cpp; dispatch src/TVgenopt.cpp:46-48).
//
//     prox(y) = argmin_x 1/2 ||x - y||^2 + lambda ||Dx||_p ,   1.002 < p < 100, p != 2
//
// The method is tvpcore.hpp's (nested Newton iterations on the KKT system of the dual, every step a tridiagonal LDL' sweep; DESIGN.md
// 6h), not the reference's gradient-projection / Frank-Wolfe scheme: it stops on the fibre's own duality gap at 1e-8 where the
// reference stops at 1e-5, and a hard cap bounds every fibre's sweeps.
//
// Mapping: tv2_fibres_kernel's -- one lane per fibre, 64 adjacent fibres per wave (every access of the wave is a coalesced 512-byte
// row); dimension-0 sweeps go through the tiled transpose so that they, too, are strided.  Four scratch arrays of the data's size
// (iterate, Newton direction, the two vectors the forward elimination leaves).  Every lane runs its own iteration counts: a wave
// takes as long as its slowest fibre.  No warm start across fibres, no atomics: a fibre's result depends on the fibre alone.
// Single long fibres run on the same kernel (no parallel-inside-the-fibre route; DESIGN.md 6h states the bound).
#include "tvp.hpp"

#include "pointwise.hpp"
#include "tvpcore.hpp"

namespace ptv {

namespace {

struct TvpArgs {
    const double *y;
    double *x;
    double *v, *dl, *ll, *zz;   // scratch, laid out like the data
    double lam, p;
    double *gap;                // one per fibre
    int *stat;                  // one per fibre: outer iterations | capped << 30
};

__global__ __launch_bounds__(64) void tvp_fibres_kernel(TvpArgs a, FibreGeom g) {
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= g.count || g.len <= 0) return;
    long blk, off;
    divmod_nonneg(j, g.inc, blk, off);
    const tvp::Fibre F{a.y, a.x, a.v, a.dl, a.ll, a.zz, blk * g.inc * g.len + off, g.inc, g.len, a.lam, a.p};
    const tvp::Result r = tvp::solve(F);
    a.gap[j] = r.gap;
    a.stat[j] = r.outer | (r.capped << 30);
}

// one workgroup, fixed order: out = {fibres solved iteratively, fibres capped, largest iteration count, largest gap}
constexpr int kStatThreads = 256;
__global__ __launch_bounds__(kStatThreads) void tvp_stats_kernel(const double *gap, const int *stat, long count, double *out) {
    __shared__ double sc[4][kStatThreads];
    double solved = 0.0, capped = 0.0, iters = 0.0, worst = 0.0;
    for (long j = threadIdx.x; j < count; j += kStatThreads) {
        const int st = stat[j], it = st & 0x3fffffff;
        solved += it > 0 ? 1.0 : 0.0;
        capped += (st >> 30) & 1 ? 1.0 : 0.0;
        iters = it > iters ? (double)it : iters;
        worst = gap[j] > worst ? gap[j] : worst;
    }
    sc[0][threadIdx.x] = solved;
    sc[1][threadIdx.x] = capped;
    sc[2][threadIdx.x] = iters;
    sc[3][threadIdx.x] = worst;
    __syncthreads();
    for (int d = kStatThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            const int o = threadIdx.x + d;
            sc[0][threadIdx.x] += sc[0][o];
            sc[1][threadIdx.x] += sc[1][o];
            sc[2][threadIdx.x] = sc[2][o] > sc[2][threadIdx.x] ? sc[2][o] : sc[2][threadIdx.x];
            sc[3][threadIdx.x] = sc[3][o] > sc[3][threadIdx.x] ? sc[3][o] : sc[3][threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) out[threadIdx.x] = sc[threadIdx.x][0];
}

}  // namespace

size_t tvp_scratch_bytes(const int *ns, int nds, int dim) {
    size_t n = 1;
    for (int i = 0; i < nds; i++) n *= (size_t)ns[i];
    if (n == 0) return 0;
    const FibreGeom g = fibres_along(ns, nds, dim);
    const bool transposed = g.inc == 1 && g.count > 1;
    return sizeof(double) * n * (transposed ? 6 : 4) + (sizeof(double) + sizeof(int)) * (size_t)g.count + 4 * sizeof(double);
}

TvpStats tvp_fibres(const double *in, double *out, double *gap, const int *ns, int nds, int dim, double lam, double p, hipStream_t s) {
    TvpStats stats;
    long n = 1;
    for (int i = 0; i < nds; i++) n *= ns[i];
    if (n <= 0) return stats;
    if (!tvp_general_norm(p)) {
        set_error("the general-p solver takes 1.002 < p < 100, p != 2 (got %g)", p);
        throw HipFailure{hipErrorInvalidValue};
    }
    const size_t need = tvp_scratch_bytes(ns, nds, dim);
    if (need > pool_cap_bytes()) {
        set_error("the general-p fibre prox needs %zu bytes of scratch, the scratch pool is capped at %zu (PROXTV_POOL_CAP_MB)", need,
                  pool_cap_bytes());
        throw HipFailure{hipErrorOutOfMemory};
    }
    const size_t bytes = sizeof(double) * (size_t)n;
    FibreGeom g = fibres_along(ns, nds, dim);
    Scratch v(bytes), dl(bytes), ll(bytes), zz(bytes);
    Scratch gaps(sizeof(double) * (size_t)g.count), stat(sizeof(int) * (size_t)g.count), red(4 * sizeof(double));
    double *gp = gap ? gap : gaps.d();
    if (g.inc == 1 && g.count > 1) {
        // dimension 0: fibres are contiguous, so lanes would stride by the fibre length -- transpose (len x count ->
        // count x len), solve along dimension 1 of the transposed array, transpose back (fibre j of the transposed array is fibre j)
        Scratch tin(bytes), tout(bytes);
        slab_transpose(in, tin.d(), g.len, g.count, 1, s);
        const FibreGeom gt{g.count, g.len, g.count};
        const TvpArgs a{tin.d(), tout.d(), v.d(), dl.d(), ll.d(), zz.d(), lam, p, gp, stat.as<int>()};
        hipLaunchKernelGGL(tvp_fibres_kernel, dim3((unsigned)((gt.count + 63) / 64)), dim3(64), 0, s, a, gt);
        PTV_HIP(hipGetLastError());
        slab_transpose(tout.d(), out, g.count, g.len, 1, s);
    } else {
        const TvpArgs a{in, out, v.d(), dl.d(), ll.d(), zz.d(), lam, p, gp, stat.as<int>()};
        hipLaunchKernelGGL(tvp_fibres_kernel, dim3((unsigned)((g.count + 63) / 64)), dim3(64), 0, s, a, g);
        PTV_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(tvp_stats_kernel, dim3(1), dim3(kStatThreads), 0, s, gp, stat.as<int>(), g.count, red.d());
    PTV_HIP(hipGetLastError());
    double h[4] = {0, 0, 0, 0};
    PTV_HIP(hipMemcpyAsync(h, red.d(), sizeof(h), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    stats.solved = (long)h[0];
    stats.capped = (long)h[1];
    stats.iters = (int)h[2];
    stats.gap = h[3];
    count_event(CNT_TVP_FIBRES, stats.solved);
    count_event(CNT_TVP_CAPPED, stats.capped);
    return stats;
}

void warm_tvp() {
    hipFuncAttributes attr;
    PTV_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(tvp_fibres_kernel)));
}

}  // namespace ptv
