// tv2_vjp.hip -- the derivative of the batched 1-D TV-L2 prox of tv2.hip.
//
// Per fibre: two solves with tridiag(-1, 2 + mu, -1), the matrix one Newton iteration of the forward factors, with the multiplier mu the
// forward hands out -- one forward elimination on two right-hand sides (D g and D y) that also yields both dot products of kappa, one
// backward substitution on the combined vector that forms gx = g - D'w as it goes (tv2vjpcore.hpp has the formulas and the arithmetic).
//
// Mapping, as the forward's: one lane per fibre, 64 adjacent fibres per wave, so every access of the wave is a coalesced 512-byte row;
// dimension-0 fibres go through the tiled transpose.  Three scratch arrays of the data's size from the pool (zh, zq and the reciprocal
// pivots; of the last only the stretch before the pivots' fixed point is written and read).  A few long contiguous fibres take the
// parallel-inside-the-fibre route of tv2.hip under the forward's own condition.  No atomics: glam is one value per fibre.
#include "tv2.hpp"

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

__global__ __launch_bounds__(64) void tv2_vjp_fibres_kernel(Tv2VjpArgs p, FibreGeom g) {
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= g.count || g.len <= 0) return;
    long blk, off;
    divmod_nonneg(j, g.inc, blk, off);
    const long base = blk * g.inc * g.len + off, inc = g.inc;
    const double *y = p.y + base, *gg = p.g + base;
    double *gx = p.gx + base;
    const double glam = tv2vjp::fibre(
        g.len, p.mu[j], p.lam, [=](int i) { return y[(long)i * inc]; }, [=](int i) { return gg[(long)i * inc]; }, FibreIo{p.r + base, inc},
        FibreIo{p.zh + base, inc}, FibreIo{p.zq + base, inc}, [=](int i, double v) { gx[(long)i * inc] = v; });
    if (p.glam) p.glam[j] = glam;
}

}  // namespace

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
        hipLaunchKernelGGL(tv2_vjp_fibres_kernel, dim3((unsigned)((gt.count + 63) / 64)), dim3(64), 0, s, a, gt);
        PTV_HIP(hipGetLastError());
        slab_transpose(tg.d(), gx, geo.count, geo.len, 1, s);
        return;
    }
    const Tv2VjpArgs a{y, mu, g, gx, glam, r.d(), zh.d(), zq.d(), lam};
    hipLaunchKernelGGL(tv2_vjp_fibres_kernel, dim3((unsigned)((geo.count + 63) / 64)), dim3(64), 0, s, a, geo);
    PTV_HIP(hipGetLastError());
}

}  // namespace ptv
