// tv2_vjp.hip -- the derivative of the batched 1-D TV-L2 prox of tv2.hip, alone and as a sweep of a solver's reverse
// recurrence.
//
// Per fibre: two solves with tridiag(-1, 2 + mu, -1), the matrix one Newton iteration of the forward factors, with the multiplier mu the
// forward hands out -- one forward elimination on two right-hand sides (D g and D y) that also yields both dot products of kappa, one
// backward substitution on the combined vector that forms gx = g - D'w as it goes (tv2vjpcore.hpp has the formulas and the arithmetic).
//
// Mapping, as the forward's: one lane per fibre, 64 adjacent fibres per wave, so every access of the wave is a coalesced 512-byte row;
// dimension-0 fibres go through the tiled transpose.  Three scratch arrays of the data's size from the pool (zh, zq and the reciprocal
// pivots; of the last only the stretch before the pivots' fixed point is written and read).  A few long contiguous fibres take the
// parallel-inside-the-fibre route of tv2.hip under the forward's own condition.  No atomics: glam is one value per fibre.
//
// The kernel takes a compile-time MODE (tv2.hpp: Tv2VjpEpi): what the load of the cotangent and the store of a = J g do.  The core reads
// sample i of the cotangent in both passes before it hands out a_i, and never afterwards, so a store may rewrite the cotangent's own
// array (g == gx; zeta rewritten in place), and a write-out that wants the incoming value beside a_i reads it again there: the same lane,
// the line still in cache.
#include "tv2.hpp"

#include <algorithm>
#include <memory>

#include "pointwise.hpp"
#include "tv2vjpcore.hpp"

namespace ptv {

namespace {

struct Tv2VjpArgs {
    const double *y, *mu, *g;
    double *gx, *glam;     // glam or null
    double *r, *zh, *zq;   // scratch, laid out like the data
    double lam;
};

// one fibre of a scratch array: edge i at p[i * inc] (p already points at the fibre's first element)
struct FibreIo {
    double *p;
    long inc;
    __device__ __forceinline__ double get(int i) const { return p[(long)i * inc]; }
    __device__ __forceinline__ void put(int i, double v) const { p[(long)i * inc] = v; }
};

// the cotangent of element i (an offset into the arrays) as both passes load it
template <int MODE>
__device__ __forceinline__ double tv2_vjp_load(const Tv2VjpEpi &e, const double *g, long i) {
    if constexpr (MODE == TV2_VJP_PD) return __builtin_fma(g[i], e.scale, -(e.zeta ? e.zeta[i] : 0.0));
    else return g[i];
}

// what becomes of a = (J g)_i ; g: the array the cotangent was loaded from
template <int MODE>
__device__ __forceinline__ void tv2_vjp_store(const Tv2VjpEpi &e, const double *g, double *gx, long i, double a) {
    if constexpr (MODE == TV2_VJP_DR_ROW) {
        if (e.final) {
            e.gU[i] = a;
            e.c[i] = a;
            gx[i] = -a;
        } else {
            const double g0 = g[i];
            e.gU[i] += a;
            e.c[i] = 2.0 * a - g0;
            gx[i] = g0 - a;
        }
    } else if constexpr (MODE == TV2_VJP_DR_COL) {
        gx[i] += a;
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

template <int MODE>
__global__ __launch_bounds__(64) void tv2_vjp_fibres_kernel(Tv2VjpArgs p, FibreGeom g, Tv2VjpEpi e) {
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= g.count || g.len <= 0) return;
    long blk, off;
    divmod_nonneg(j, g.inc, blk, off);
    const long base = blk * g.inc * g.len + off, inc = g.inc;
    const double *y = p.y + base;
    const double glam = tv2vjp::fibre(
        g.len, p.mu[j], p.lam, [=](int i) { return y[(long)i * inc]; }, [=](int i) { return tv2_vjp_load<MODE>(e, p.g, base + (long)i * inc); },
        FibreIo{p.r + base, inc}, FibreIo{p.zh + base, inc}, FibreIo{p.zq + base, inc},
        [=](int i, double v) { tv2_vjp_store<MODE>(e, p.g, p.gx, base + (long)i * inc, v); });
    if (p.glam) p.glam[j] = (MODE != TV2_VJP_PLAIN && e.add_glam) ? p.glam[j] + glam : glam;
}

// ---- the routes without a fused write-out: pointwise kernels around a TV2_VJP_PLAIN call ------------------------------------------------
__global__ __launch_bounds__(256) void tv2_vjp_cotangent_kernel(Tv2VjpEpi e, const double *g, double *pi, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) pi[i] = tv2_vjp_load<TV2_VJP_PD>(e, g, i);
}
template <int MODE>
__global__ __launch_bounds__(256) void tv2_vjp_epilogue_kernel(Tv2VjpEpi e, const double *a, const double *g, double *gx, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) tv2_vjp_store<MODE>(e, g, gx, i, a[i]);
}
__global__ __launch_bounds__(256) void tv2_vjp_glam_add_kernel(double *glam, const double *part, long count) {
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < count; j += (long)gridDim.x * 256) glam[j] += part[j];
}
unsigned pointwise_blocks(long n) { return (unsigned)std::min<long>((n + 255) / 256, 4096); }

template <int MODE>
void launch_fibres(const Tv2VjpArgs &a, const FibreGeom &geo, const Tv2VjpEpi &e, hipStream_t s) {
    hipLaunchKernelGGL((tv2_vjp_fibres_kernel<MODE>), dim3((unsigned)((geo.count + 63) / 64)), dim3(64), 0, s, a, geo, e);
    PTV_HIP(hipGetLastError());
}

template <int MODE>
void launch_epilogue(const Tv2VjpEpi &e, const double *a, const double *g, double *gx, long n, hipStream_t s) {
    hipLaunchKernelGGL((tv2_vjp_epilogue_kernel<MODE>), dim3(pointwise_blocks(n)), dim3(256), 0, s, e, a, g, gx, n);
    PTV_HIP(hipGetLastError());
}

// whether fibres of this geometry run the lane-per-fibre kernel on the arrays as they lie
bool tv2_vjp_direct(const FibreGeom &geo, double lam) { return !tv2_long_route(geo, lam) && !(geo.inc == 1 && geo.count > 1); }

}  // namespace

void fibre_vjp_cotangent(const Tv2VjpEpi &epi, const double *g, double *pi, long n, hipStream_t s) {
    hipLaunchKernelGGL(tv2_vjp_cotangent_kernel, dim3(pointwise_blocks(n)), dim3(256), 0, s, epi, g, pi, n);
    PTV_HIP(hipGetLastError());
}

void fibre_vjp_glam_add(double *glam, const double *part, long count, hipStream_t s) {
    hipLaunchKernelGGL(tv2_vjp_glam_add_kernel, dim3(pointwise_blocks(count)), dim3(256), 0, s, glam, part, count);
    PTV_HIP(hipGetLastError());
}

void fibre_vjp_write_out(const Tv2VjpEpi &epi, const double *a, const double *g, double *gx, long n, hipStream_t s) {
    switch (epi.mode) {
        case TV2_VJP_DR_ROW: launch_epilogue<TV2_VJP_DR_ROW>(epi, a, g, gx, n, s); break;
        case TV2_VJP_DR_COL: launch_epilogue<TV2_VJP_DR_COL>(epi, a, g, gx, n, s); break;
        case TV2_VJP_PD2:    launch_epilogue<TV2_VJP_PD2>(epi, a, g, gx, n, s); break;
        case TV2_VJP_PD:     launch_epilogue<TV2_VJP_PD>(epi, a, g, gx, n, s); break;
        default:             launch_epilogue<TV2_VJP_PLAIN>(epi, a, g, gx, n, s); break;
    }
}

void tv2_fibres_vjp(const double *y, const double *mu, const double *g, double *gx, double *glam, const int *ns, int nds, int dim,
                    double lam, hipStream_t s) {
    long n = 1;
    for (int i = 0; i < nds; i++) n *= ns[i];
    if (n <= 0) return;
    const size_t bytes = sizeof(double) * (size_t)n;
    const FibreGeom geo = fibres_along(ns, nds, dim);
    if (tv2_long_route(geo, lam)) {
        tv2_long_fibres_vjp(y, mu, g, gx, glam, geo, lam, s);
        return;
    }
    Scratch r(bytes), zh(bytes), zq(bytes);
    if (geo.inc == 1 && geo.count > 1) {
        // dimension 0: transpose y and g (len x count -> count x len), work along dimension 1 in place on the transposed g, transpose back
        Scratch ty(bytes), tg(bytes);
        slab_transpose(y, ty.d(), geo.len, geo.count, 1, s);
        slab_transpose(g, tg.d(), geo.len, geo.count, 1, s);
        const FibreGeom gt{geo.count, geo.len, geo.count};
        const Tv2VjpArgs a{ty.d(), mu, tg.d(), tg.d(), glam, r.d(), zh.d(), zq.d(), lam};   // (fibre j of the transposed array is fibre j)
        launch_fibres<TV2_VJP_PLAIN>(a, gt, Tv2VjpEpi{}, s);
        slab_transpose(tg.d(), gx, geo.count, geo.len, 1, s);
        return;
    }
    const Tv2VjpArgs a{y, mu, g, gx, glam, r.d(), zh.d(), zq.d(), lam};
    launch_fibres<TV2_VJP_PLAIN>(a, geo, Tv2VjpEpi{}, s);
}

void tv2_fibres_vjp_epi(const double *y, const double *mu, const double *g, double *gx, double *glam, const int *ns, int nds, int dim,
                        double lam, const Tv2VjpEpi &epi, hipStream_t s) {
    if (epi.mode == TV2_VJP_PLAIN) {
        tv2_fibres_vjp(y, mu, g, gx, glam, ns, nds, dim, lam, s);
        return;
    }
    long n = 1;
    for (int i = 0; i < nds; i++) n *= ns[i];
    if (n <= 0) return;
    const size_t bytes = sizeof(double) * (size_t)n;
    const FibreGeom geo = fibres_along(ns, nds, dim);
    if (tv2_vjp_direct(geo, lam)) {
        Scratch r(bytes), zh(bytes), zq(bytes);
        const Tv2VjpArgs a{y, mu, g, gx, glam, r.d(), zh.d(), zq.d(), lam};
        switch (epi.mode) {
            case TV2_VJP_DR_ROW: launch_fibres<TV2_VJP_DR_ROW>(a, geo, epi, s); break;
            case TV2_VJP_DR_COL: launch_fibres<TV2_VJP_DR_COL>(a, geo, epi, s); break;
            case TV2_VJP_PD2:    launch_fibres<TV2_VJP_PD2>(a, geo, epi, s); break;
            default:             launch_fibres<TV2_VJP_PD>(a, geo, epi, s); break;
        }
        return;
    }
    // a = J g (J pi) into scratch by the plain call, whichever route it takes; then the write-out, one element per thread
    fibre_vjp_epilogue_route(epi, g, gx, glam, n, geo.count, s, [&](const double *cot, double *a, double *gl) {
        tv2_fibres_vjp(y, mu, cot, a, gl, ns, nds, dim, lam, s);
    });
}

}  // namespace ptv
