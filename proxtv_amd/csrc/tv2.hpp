// tv2.hpp -- batched exact 1-D TV-L2 prox over fibres (tv2.hip) and its derivative (tv2_vjp.hip).
#pragma once

#include <memory>

#include "common.hpp"

namespace ptv {

// out = argmin 1/2 ||x - in||^2 + lam ||Dx||_2 along dimension `dim` of every fibre of the N-D column-major array.
// `in` and `out` must be distinct arrays.  mu (device, or null): the multiplier of every fibre, one value per fibre in the column-major
// order of the array with `dim` removed -- exactly 0.0 where the dual lies inside the ball (out is the mean), for ns[dim] == 1 and for
// lam <= 0 (and where the first Newton step from mu = 0 is rejected: active by a rounding margin, the kink).  With mu == nullptr the
// call is what it was without the argument, bit for bit.
void tv2_fibres(const double *in, double *out, const int *ns, int nds, int dim, double lam, hipStream_t s, double *mu = nullptr);

// The derivative of that prox applied to g: y and mu are what tv2_fibres returned for the same ns / dim / lam.
// gx (may be g itself; otherwise no array may overlap another) = J g with J = dy/dx, symmetric; glam (device, one per fibre, or null)
// the gradient in lam.  No atomics.
void tv2_fibres_vjp(const double *y, const double *mu, const double *g, double *gx, double *glam, const int *ns, int nds, int dim,
                    double lam, hipStream_t s);

// The same derivative as one sweep of a solver's reverse recurrence (vjp.hip: dr2_vjp, pd_vjp).  With a = J g the modes are
// vjp.hip's, a standing where the segmented mean stands there:
//   TV2_VJP_PLAIN    gx = a                                                              (tv2_fibres_vjp, bit for bit)
//   TV2_VJP_DR_ROW   g = gbar in place:  gU += a ;  c = 2 a - g ;  gx = g - a            (final: gU = a ;  c = a ;  gx = -a)
//   TV2_VJP_DR_COL   gx += a
//   TV2_VJP_PD2      g = D in place:     gx = a - g  (with gU: gU += a)                  (final: gx = a without gU ;  gU = a with it)
//   TV2_VJP_PD       the cotangent is pi = fma(g, scale, -zeta), formed on load in both passes by that one fma (zeta == null: 0);
//                    gx = zeta in place:  gx = zeta + a ;  gU += gx                       (final: gU = gx)
// glam: one value per fibre, written, or accumulated with add_glam.  Every element is read and written by the lane that owns it.
enum { TV2_VJP_PLAIN = 0, TV2_VJP_DR_ROW = 1, TV2_VJP_DR_COL = 2, TV2_VJP_PD2 = 3, TV2_VJP_PD = 4 };
struct Tv2VjpEpi {
    int mode = TV2_VJP_PLAIN;
    double *gU = nullptr, *c = nullptr;
    int final = 0;
    int add_glam = 0;
    const double *zeta = nullptr;
    double scale = 0.0;
};
// Strided fibres (dim >= 1, and a single dimension-0 fibre) run the write-out inside the lane-per-fibre kernel.  Dimension-0 fibres (the
// transposed route) and the long-fibre route run TV2_VJP_PLAIN into scratch and one pointwise kernel behind it (TV2_VJP_PD: one more in
// front, which forms pi with the same fma).
void tv2_fibres_vjp_epi(const double *y, const double *mu, const double *g, double *gx, double *glam, const int *ns, int nds, int dim,
                        double lam, const Tv2VjpEpi &epi, hipStream_t s);

// The pointwise kernels of that second route, generic in a: they serve the general-p derivative's epilogue route too (tvp_vjp.hip;
// DESIGN.md 6j).  pi[i] = fma(g[i], scale, -zeta[i]) (TV2_VJP_PD's load) ; the write-out of epi.mode on a = J g, one element per thread ;
// glam[j] += part[j].
void fibre_vjp_cotangent(const Tv2VjpEpi &epi, const double *g, double *pi, long n, hipStream_t s);
void fibre_vjp_write_out(const Tv2VjpEpi &epi, const double *a, const double *g, double *gx, long n, hipStream_t s);
void fibre_vjp_glam_add(double *glam, const double *part, long count, hipStream_t s);

// The epilogue route, whichever prox J belongs to: `plain(cot, a, glam)` enqueues a = J cot (and the per-fibre glam, where the pointer
// is not null) by the plain call; around it the pre-pass of TV2_VJP_PD, the glam accumulation and the write-out of epi.mode.
template <class Plain>
void fibre_vjp_epilogue_route(const Tv2VjpEpi &epi, const double *g, double *gx, double *glam, long n, long fibres, hipStream_t s,
                              const Plain &plain) {
    const size_t bytes = sizeof(double) * (size_t)n;
    Scratch a(bytes);
    std::unique_ptr<Scratch> pi, part;
    const double *cot = g;
    if (epi.mode == TV2_VJP_PD) {
        pi.reset(new Scratch(bytes));
        fibre_vjp_cotangent(epi, g, pi->d(), n, s);
        cot = pi->d();
    }
    const bool add = glam && epi.add_glam;
    if (add) part.reset(new Scratch(sizeof(double) * (size_t)fibres));
    plain(cot, a.d(), add ? part->d() : glam);
    if (add) fibre_vjp_glam_add(glam, part->d(), fibres, s);
    fibre_vjp_write_out(epi, a.d(), g, gx, n, s);
}

// ---- shared by the two units ----
// whether fibres of this geometry go through the parallel-inside-the-fibre path (tv2_long_*) -- the forward and the derivative agree
bool tv2_long_route(const FibreGeom &g, double lam);
// the derivative along that path (tv2.hip: it reuses the forward's reduce / scan / apply kernels); contiguous fibres only
void tv2_long_fibres_vjp(const double *y, const double *mu, const double *g, double *gx, double *glam, const FibreGeom &geo, double lam,
                         hipStream_t s);

}  // namespace ptv
