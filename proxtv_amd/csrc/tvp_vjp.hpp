// tvp_vjp.hpp -- the derivative of the batched general-p TV-Lp fibre prox (tvp_vjp.hip; the method: tvpvjpcore.hpp).
#pragma once

#include "common.hpp"

namespace ptv {

// gx = J g along dimension `dim` of every fibre of the N-D column-major array, J the Jacobian of tvp_fibres (tvp.hpp) at the point whose
// OUTPUT is y, p as tvp_general_norm accepts; glam (device, or null): -gx'D'phi of every fibre, one value per fibre in the column-major
// order of the array with `dim` removed (as tvp_fibres lays out gap).  gx may be g; no other pair of arrays may overlap.  Scratch (three
// arrays of the data's size, two more for dimension 0) comes from the pool; beyond the pool's cap the call throws with last_error naming
// the bytes and nothing written.  Enqueues on s and returns.  No atomics: a fibre's bits depend on that fibre alone.
void tvp_fibres_vjp(const double *y, const double *g, double *gx, double *glam, const int *ns, int nds, int dim, double lam, double p,
                    hipStream_t s);
size_t tvp_vjp_scratch_bytes(const int *ns, int nds, int dim);

}  // namespace ptv
