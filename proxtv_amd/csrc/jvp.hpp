// jvp.hpp -- host interface of the forward-mode derivatives (jvp.hip; the method: jvpcore.hpp).
#pragma once

#include "common.hpp"

namespace ptv {

namespace vjp {
struct Summary;
struct Resolved;
}  // namespace vjp

// samples per chunk of the derivative kernels, reverse and forward mode alike (vjp.hip checks its own constant against this one): the
// scratch records S and R hold fibres * ceil(len / kVjpChunk) entries
constexpr int kVjpChunk = 16;

// phase B of vjp.hip on the stream, shared by both modes: R <- the means of the segments that span chunks, from the summaries S
// (strided fibres: records at chunk * count + fibre; contiguous ones: fibre * nch + chunk).  nseg (or null): every fibre's segments.
void vjp_resolve(vjp::Summary *S, vjp::Resolved *R, const FibreGeom &geo, int *nseg, hipStream_t s);

// dy = P (dx + E(sigma, dw + dlam)) at the prox output y (jvpcore.hpp): dx null = zero, dw (per edge, the shape of the prox's weights)
// null = zero, dlam added on every edge.  dy may be dx.  Returns with the stream drained.
void tv1_fibres_jvp(const double *y, const double *dx, const double *dw, double dlam, double *dy, const int *ns, int nds, int dim,
                    hipStream_t s);

// the tangent of dr2's unfused recurrence (the one dr2_vjp replays), formed sweep by sweep next to the forward: nothing is kept between
// iterations but t and dt, so the scratch -- dr2_jvp_scratch_bytes, which the caller checks against pool_cap_bytes -- does not depend on
// maxit.  dU / dW1m / dW2m may be null (zero); out (the forward result) may be null.  No overlaps.  Returns with the stream drained.
size_t dr2_jvp_scratch_bytes(size_t M, size_t N, size_t B);
void dr2_jvp(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, const double *W1m, const double *W2m, const double *dU,
             const double *dW1m, const double *dW2m, double dW1, double dW2, double *out, double *ds, int maxit, hipStream_t s);

}  // namespace ptv
