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
//
// The kernel takes a compile-time MODE (tv2.hpp: Tv2VjpEpi, the modes of vjp.hip's reverse recurrences): what the load of
// the cotangent and the store of a = J g do.  The core hands out a_i after its last read of sample i of the cotangent, so a store may
// rewrite the cotangent's own array (g == gx; gU == g; zeta rewritten in place), and a write-out that wants the incoming value beside
// a_i reads it again there: the same lane, the line still in cache.  Two routes give the same bits: the MODE kernel on the arrays as they
// lie (fused), or the plain kernel into scratch and tv2_vjp.hip's pointwise write-out behind it (epilogue: dimension-0 fibres always).
// The write-out's additions are compiled without contraction, so that none of them can fuse with a product inside the core in the one
// route and not in the other.
#include "tvp_vjp.hpp"

#include "pointwise.hpp"
#include "policy.hpp"
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

// the cotangent of element i (an offset into the arrays) as every pass loads it: VJP_PD forms pi by the one fma the pre-pass of the
// epilogue route uses
template <int MODE>
__device__ __forceinline__ double tvp_vjp_load(const Tv2VjpEpi &e, const double *g, long i) {
    if constexpr (MODE == TV2_VJP_PD) return __builtin_fma(g[i], e.scale, -(e.zeta ? e.zeta[i] : 0.0));
    else return g[i];
}

// what becomes of a = (J g)_i ; g: the array the cotangent was loaded from.  tv2_vjp.hip's write-out, every operation one rounding
// (2 a as a + a: exact either way)
template <int MODE>
__device__ __forceinline__ void tvp_vjp_store(const Tv2VjpEpi &e, const double *g, double *gx, long i, double a) {
#pragma clang fp contract(off)
    if constexpr (MODE == TV2_VJP_DR_ROW) {
        if (e.final) {
            e.gU[i] = a;
            e.c[i] = a;
            gx[i] = -a;
        } else {
            const double g0 = g[i];
            e.gU[i] = e.gU[i] + a;
            e.c[i] = (a + a) - g0;
            gx[i] = g0 - a;
        }
    } else if constexpr (MODE == TV2_VJP_DR_COL) {
        gx[i] = gx[i] + a;
    } else if constexpr (MODE == TV2_VJP_PD2) {
        if (e.gU) {
            const double g0 = g[i];
            e.gU[i] = e.final ? a : e.gU[i] + a;
            gx[i] = a - g0;
        } else {
            gx[i] = e.final ? a : a - g[i];
        }
    } else if constexpr (MODE == TV2_VJP_PD) {
        const double z = (e.zeta ? e.zeta[i] : 0.0) + a;
        gx[i] = z;
        e.gU[i] = e.final ? z : e.gU[i] + z;
    } else {
        gx[i] = a;
    }
}

__device__ __forceinline__ double tvp_vjp_glam_sum(double have, double glam) {
#pragma clang fp contract(off)
    return have + glam;
}

template <int MODE>
__global__ __launch_bounds__(64) void tvp_vjp_fibres_kernel(TvpVjpArgs a, FibreGeom g, Tv2VjpEpi e) {
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= g.count || g.len <= 0) return;
    long blk, off;
    divmod_nonneg(j, g.inc, blk, off);
    const long base = blk * g.inc * g.len + off, inc = g.inc;
    const tvpvjp::Fibre F{a.y, a.g, a.gx, a.ll, a.z1, a.z2, base, inc, g.len, a.lam, a.p};
    double glam;
    if constexpr (MODE == TV2_VJP_PLAIN) {
        glam = tvpvjp::solve(F);
    } else {
        glam = tvpvjp::solve(
            F, [&](int i) { return tvp_vjp_load<MODE>(e, a.g, base + (long)i * inc); },
            [&](int i, double v) { tvp_vjp_store<MODE>(e, a.g, a.gx, base + (long)i * inc, v); });
    }
    if (a.glam) a.glam[j] = (MODE != TV2_VJP_PLAIN && e.add_glam) ? tvp_vjp_glam_sum(a.glam[j], glam) : glam;
}

template <int MODE>
void launch_fibres(const TvpVjpArgs &a, const FibreGeom &geo, const Tv2VjpEpi &e, hipStream_t s) {
    hipLaunchKernelGGL((tvp_vjp_fibres_kernel<MODE>), dim3((unsigned)((geo.count + 63) / 64)), dim3(64), 0, s, a, geo, e);
    PTV_HIP(hipGetLastError());
}

long total_of(const int *ns, int nds) {
    long n = 1;
    for (int i = 0; i < nds; i++) n *= ns[i];
    return n;
}

// whether the fused kernel may run on the arrays as they lie: not on dimension-0 fibres (they are transposed first)
bool tvp_vjp_fused_legal(const FibreGeom &geo) { return !(geo.inc == 1 && geo.count > 1); }

// option tvp_vjp_route: 0 = the rule of policy.hpp, 1 = fused wherever legal, 2 = the epilogue everywhere
bool tvp_vjp_fused(const FibreGeom &geo) {
    if (!tvp_vjp_fused_legal(geo)) return false;
    const int route = options().tvp_vjp_route;
    if (route == 1) return true;
    if (route == 2) return false;
    return tvp_vjp_fused_auto(geo.count);
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

size_t tvp_vjp_epi_scratch_bytes(const int *ns, int nds, int dim, int mode, bool add_glam) {
    const size_t plain = tvp_vjp_scratch_bytes(ns, nds, dim);
    if (plain == 0 || mode == TV2_VJP_PLAIN) return plain;
    const FibreGeom g = fibres_along(ns, nds, dim);
    if (tvp_vjp_fused(g)) return plain;
    const size_t n = (size_t)g.count * (size_t)g.len;
    return plain + sizeof(double) * (n * (mode == TV2_VJP_PD ? 2 : 1) + (add_glam ? (size_t)g.count : 0));
}

void tvp_fibres_vjp(const double *y, const double *g, double *gx, double *glam, const int *ns, int nds, int dim, double lam, double p,
                    hipStream_t s) {
    const long n = total_of(ns, nds);
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
        launch_fibres<TV2_VJP_PLAIN>(a, gt, Tv2VjpEpi{}, s);
        slab_transpose(tg.d(), gx, geo.count, geo.len, 1, s);
        return;
    }
    const TvpVjpArgs a{y, g, gx, glam, ll.d(), z1.d(), z2.d(), lam, p};
    launch_fibres<TV2_VJP_PLAIN>(a, geo, Tv2VjpEpi{}, s);
}

void tvp_fibres_vjp_epi(const double *y, const double *g, double *gx, double *glam, const int *ns, int nds, int dim, double lam, double p,
                        const Tv2VjpEpi &epi, hipStream_t s) {
    if (epi.mode == TV2_VJP_PLAIN) {
        tvp_fibres_vjp(y, g, gx, glam, ns, nds, dim, lam, p, s);
        return;
    }
    const long n = total_of(ns, nds);
    if (n <= 0) return;
    if (!tvp_general_norm(p)) {
        set_error("the general-p derivative takes 1.002 < p < 100, p != 2 (got %g)", p);
        throw HipFailure{hipErrorInvalidValue};
    }
    const size_t bytes = sizeof(double) * (size_t)n;
    const FibreGeom geo = fibres_along(ns, nds, dim);
    if (tvp_vjp_fused(geo)) {
        Scratch ll(bytes), z1(bytes), z2(bytes);
        const TvpVjpArgs a{y, g, gx, glam, ll.d(), z1.d(), z2.d(), lam, p};
        switch (epi.mode) {
            case TV2_VJP_DR_ROW: launch_fibres<TV2_VJP_DR_ROW>(a, geo, epi, s); break;
            case TV2_VJP_DR_COL: launch_fibres<TV2_VJP_DR_COL>(a, geo, epi, s); break;
            case TV2_VJP_PD2:    launch_fibres<TV2_VJP_PD2>(a, geo, epi, s); break;
            default:             launch_fibres<TV2_VJP_PD>(a, geo, epi, s); break;
        }
        return;
    }
    // a = J g (J pi) into scratch by the plain call; then the write-out, one element per thread
    fibre_vjp_epilogue_route(epi, g, gx, glam, n, geo.count, s, [&](const double *cot, double *a, double *gl) {
        tvp_fibres_vjp(y, cot, a, gl, ns, nds, dim, lam, p, s);
    });
}

void warm_tvp_vjp() {
    hipFuncAttributes attr;
    // (one code object holds every MODE: touching one uploads it; the others are asked for so that none is resolved inside a solve)
    PTV_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(tvp_vjp_fibres_kernel<TV2_VJP_PLAIN>)));
    PTV_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(tvp_vjp_fibres_kernel<TV2_VJP_DR_ROW>)));
    PTV_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(tvp_vjp_fibres_kernel<TV2_VJP_DR_COL>)));
    PTV_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(tvp_vjp_fibres_kernel<TV2_VJP_PD2>)));
    PTV_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(tvp_vjp_fibres_kernel<TV2_VJP_PD>)));
}

}  // namespace ptv
