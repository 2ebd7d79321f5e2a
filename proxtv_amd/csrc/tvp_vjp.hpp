// tvp_vjp.hpp -- the derivative of the batched general-p TV-Lp fibre prox (tvp_vjp.hip; the method: tvpvjpcore.hpp).
#pragma once

#include "common.hpp"
#include "tv2.hpp"

namespace ptv {

// gx = J g along dimension `dim` of every fibre of the N-D column-major array, J the Jacobian of tvp_fibres (tvp.hpp) at the point whose
// OUTPUT is y, p as tvp_general_norm accepts; glam (device, or null): -gx'D'phi of every fibre, one value per fibre in the column-major
// order of the array with `dim` removed (as tvp_fibres lays out gap).  gx may be g; no other pair of arrays may overlap.  Scratch (three
// arrays of the data's size, two more for dimension 0) comes from the pool; beyond the pool's cap the call throws with last_error naming
// the bytes and nothing written.  Enqueues on s and returns.  No atomics: a fibre's bits depend on that fibre alone.
void tvp_fibres_vjp(const double *y, const double *g, double *gx, double *glam, const int *ns, int nds, int dim, double lam, double p,
                    hipStream_t s);
size_t tvp_vjp_scratch_bytes(const int *ns, int nds, int dim);

// The same derivative as one sweep of a solver's reverse recurrence (vjp.hip: dr2_vjp, pd_vjp): a = J g with the write-out
// of epi.mode -- tv2.hpp's Tv2VjpEpi, the modes and their formulas as listed there (glam: one value per fibre, written, or accumulated
// with add_glam).  TV2_VJP_PLAIN is tvp_fibres_vjp, bit for bit.  Two routes, the same bits: fused -- the write-out inside the
// lane-per-fibre kernel, on the arrays as they lie (dimension >= 1, or a single dimension-0 fibre); epilogue -- the plain call into
// scratch and tv2_vjp.hip's pointwise write-out behind it (TV2_VJP_PD: one more in front, which forms pi with the same fma), always for
// dimension-0 fibres.  Where both are legal option tvp_vjp_route chooses (0: policy.hpp's rule on the fibre count).
void tvp_fibres_vjp_epi(const double *y, const double *g, double *gx, double *glam, const int *ns, int nds, int dim, double lam, double p,
                        const Tv2VjpEpi &epi, hipStream_t s);
// the scratch of that call by the route it will take: tvp_vjp_scratch_bytes, and on the epilogue route one more array of the data's size
// (two for TV2_VJP_PD) and, where glam accumulates, one double per fibre
size_t tvp_vjp_epi_scratch_bytes(const int *ns, int nds, int dim, int mode, bool add_glam);

}  // namespace ptv
