// tvp_vjp.hip -- the derivative of the batched general-p TV-Lp fibre prox of tvp.hip.
//
// Per fibre, from the prox's output, lambda and p alone: two solves with one tridiagonal matrix -- n x n for p > 2, (n-1) x (n-1) for
// p < 2, the arm in which every power has an exponent >= 0 -- that share one LDL' factorisation: a forward elimination on two right-hand
// sides, which also yields both scalar products of the rank-one correction, and one backward substitution on the combined vector that
// writes gx as it goes; before them a pass for the largest jump and one for ||Dy||_p (tvpvjpcore.hpp has the formulas and the arithmetic).
//
// Mapping: tvp_fibres_kernel's -- one lane per fibre, 64 adjacent fibres per wave (every access of the wave is a coalesced 512-byte
// row); dimension-0 fibres go through the tiled transpose so that they, too, are strided.  Three scratch arrays of the data's size from
// the pool (l_i and the two z_i / d_i of the elimination).  No atomics: glam is one value per fibre.  Single long fibres run on the same
// kernel, one lane (no parallel-inside-the-fibre route, as in the forward).
#include "tvp_vjp.hpp"

#include "pointwise.hpp"
#include "tvp.hpp"
#include "tvpvjpcore.hpp"

namespace ptv {

namespace {

struct TvpVjpArgs {
    const double *y, *g;
    double *gx, *glam;      // glam or null
    double *ll, *z1, *z2;   // scratch, laid out like the data
    double lam, p;
};

__global__ __launch_bounds__(64) void tvp_vjp_fibres_kernel(TvpVjpArgs a, FibreGeom g) {
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= g.count || g.len <= 0) return;
    long blk, off;
    divmod_nonneg(j, g.inc, blk, off);
    const tvpvjp::Fibre F{a.y, a.g, a.gx, a.ll, a.z1, a.z2, blk * g.inc * g.len + off, g.inc, g.len, a.lam, a.p};
    const double glam = tvpvjp::solve(F);
    if (a.glam) a.glam[j] = glam;
}

}  // namespace

size_t tvp_vjp_scratch_bytes(const int *ns, int nds, int dim) {
    size_t n = 1;
    for (int i = 0; i < nds; i++) n *= (size_t)ns[i];
    if (n == 0) return 0;
    const FibreGeom g = fibres_along(ns, nds, dim);
    const bool transposed = g.inc == 1 && g.count > 1;
    return sizeof(double) * n * (transposed ? 5 : 3);
}

void tvp_fibres_vjp(const double *y, const double *g, double *gx, double *glam, const int *ns, int nds, int dim, double lam, double p,
                    hipStream_t s) {
    long n = 1;
    for (int i = 0; i < nds; i++) n *= ns[i];
    if (n <= 0) return;
    if (!tvp_general_norm(p)) {
        set_error("the general-p derivative takes 1.002 < p < 100, p != 2 (got %g)", p);
        throw HipFailure{hipErrorInvalidValue};
    }
    const size_t need = tvp_vjp_scratch_bytes(ns, nds, dim);
    if (need > pool_cap_bytes()) {
        set_error("the general-p fibre derivative needs %zu bytes of scratch, the scratch pool is capped at %zu (PROXTV_POOL_CAP_MB)", need,
                  pool_cap_bytes());
        throw HipFailure{hipErrorOutOfMemory};
    }
    const size_t bytes = sizeof(double) * (size_t)n;
    const FibreGeom geo = fibres_along(ns, nds, dim);
    Scratch ll(bytes), z1(bytes), z2(bytes);
    if (geo.inc == 1 && geo.count > 1) {
        // dimension 0: transpose y and g (len x count -> count x len), work along dimension 1 in place on the transposed g, transpose back
        // (fibre j of the transposed array is fibre j)
        Scratch ty(bytes), tg(bytes);
        slab_transpose(y, ty.d(), geo.len, geo.count, 1, s);
        slab_transpose(g, tg.d(), geo.len, geo.count, 1, s);
        const FibreGeom gt{geo.count, geo.len, geo.count};
        const TvpVjpArgs a{ty.d(), tg.d(), tg.d(), glam, ll.d(), z1.d(), z2.d(), lam, p};
        hipLaunchKernelGGL(tvp_vjp_fibres_kernel, dim3((unsigned)((gt.count + 63) / 64)), dim3(64), 0, s, a, gt);
        PTV_HIP(hipGetLastError());
        slab_transpose(tg.d(), gx, geo.count, geo.len, 1, s);
        return;
    }
    const TvpVjpArgs a{y, g, gx, glam, ll.d(), z1.d(), z2.d(), lam, p};
    hipLaunchKernelGGL(tvp_vjp_fibres_kernel, dim3((unsigned)((geo.count + 63) / 64)), dim3(64), 0, s, a, geo);
    PTV_HIP(hipGetLastError());
}

void warm_tvp_vjp() {
    hipFuncAttributes attr;
    PTV_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(tvp_vjp_fibres_kernel)));
}

}  // namespace ptv
