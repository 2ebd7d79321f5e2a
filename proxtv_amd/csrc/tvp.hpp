// tvp.hpp -- batched 1-D TV-Lp prox over fibres for general p (tvp.hip; the method: tvpcore.hpp).
#pragma once

#include "common.hpp"

namespace ptv {

// the norms the general-p solver takes: the reference's own LPPROJ_PSMALL / LPPROJ_PLARGE, beyond which it stops treating p as general
constexpr double kTvpPMin = 1.002, kTvpPMax = 100.0;
inline bool tvp_general_norm(double p) { return p > kTvpPMin && p < kTvpPMax && p != 2.0; }

struct TvpStats {
    long solved = 0;      // fibres solved iteratively (the others were closed forms: a copy, or the mean)
    long capped = 0;      // ... of which a cap stopped the iteration above its target gap
    int iters = 0;        // the largest outer iteration count of a fibre
    double gap = 0.0;     // the largest achieved duality gap of a fibre
};

// out = argmin 1/2 ||x - in||^2 + lam ||Dx||_p along dimension `dim` of every fibre of the N-D column-major array, p as tvp_general_norm
// accepts.  `in` and `out` must be distinct arrays.  gap (device, or null): the achieved duality gap of every fibre, one value per fibre
// in the column-major order of the array with `dim` removed (as tv2_fibres lays out mu) -- 0 where the answer is a closed form.
// Scratch (four arrays of the data's size, two more for dimension 0, 12 bytes per fibre) comes from the pool; beyond the pool's cap the
// call throws with last_error naming the bytes.  Reads the fibres' statistics back: synchronises the stream.  No atomics.
TvpStats tvp_fibres(const double *in, double *out, double *gap, const int *ns, int nds, int dim, double lam, double p, hipStream_t s);
size_t tvp_scratch_bytes(const int *ns, int nds, int dim);

void warm_tvp();

}  // namespace ptv
