// jvpcore.hpp -- the forward-mode derivative of the 1-D TV-L1 prox, chunk by chunk.  Plain C++ on registers and small
// arrays, on top of vjpcore.hpp: jvp.hip runs it one lane per chunk, tests/jvp_host.cpp runs the same functions with g++.
//
// y = prox(x; r) along one fibre, r_k the penalty of edge k (between samples k and k+1), sigma_k = +1 / -1 / 0 for a step up / a step
// down / no step (vjpcore.hpp's rule).  On a segment S between the steps l and r:  y_S = mean(x_S) + (sigma_r r_r - sigma_l r_l) / |S|,
// so for tangents dx and dr
//     dy = P (dx + E(sigma, dr)) ,   E(sigma, dr)[i] = sigma_i dr_i - sigma_{i-1} dr_{i-1}      (an edge outside the fibre: 0)
// with P the segmented mean of vjpcore.hpp: the transpose of gx = P g, gw[k] = sigma_k (gx[k] - gx[k+1]).  All this file adds is the
// LOAD of v = dx + E: phases A, B and C then run on v as they run on a cotangent.  dx itself may be a combination of up to three arrays
// (Comb), which is how the sweeps of a Douglas-Rachford solve take their tangent without a pass in front of them.
//
// A chunk owns the edges BEHIND its samples, so chunk_load's masks hold sigma_k for its own samples; the edge before its first sample
// belongs to the previous chunk and is decided here from the sample in front of the chunk (`yprev`), by the same is_step.
// Two forms of E, the same bits: per chunk from the masks (chunk_load_tangent: a lane that walks its chunk), and per sample from the
// three values of y around it (sample_term: a staging loop that meets every sample once, in any order).
#pragma once

#include "vjpcore.hpp"

namespace ptv {
namespace jvp {

// v[i] = ca a[i] + cb b[i] + cc c[i], null arrays skipped (all null: 0).  One expression, left to right, wherever it is formed.
struct Comb {
    const double *a = nullptr, *b = nullptr, *c = nullptr;
    double ca = 0.0, cb = 0.0, cc = 0.0;
};
PTV_VJP_HD double comb_at(const Comb &q, long i) {
    double v = q.a ? q.ca * q.a[i] : 0.0;
    if (q.b) v += q.cb * q.b[i];
    if (q.c) v += q.cc * q.c[i];
    return v;
}

// sigma dr of the edge between the samples a and b
PTV_VJP_HD double edge_term(double a, double b, double dr) { return vjp::is_step(a, b) ? (b > a ? dr : -dr) : 0.0; }

// E of one sample from its neighbours: has_prev / has_next say whether the fibre has a sample before / behind it (yprev / ynext and
// dr_prev / dr_here -- the tangents of the edges before and behind the sample -- are read only then)
PTV_VJP_HD double sample_term(bool has_prev, double yprev, double y, bool has_next, double ynext, double dr_prev, double dr_here) {
    const double behind = has_next ? edge_term(y, ynext, dr_here) : 0.0;
    const double before = has_prev ? edge_term(yprev, y, dr_prev) : 0.0;
    return behind - before;
}

// chunk_load with the tangent: g[k] = V(k) + E[k].  Y(k), k = 0 .. len (len itself only when has_next), as chunk_load takes it;
// DR(k), k = -1 .. len - 1: the tangent of the edge behind sample k of the chunk (-1: the edge before the chunk, asked for only when
// has_prev and that edge steps; an edge is asked for only where it steps).  inject = false: E is left out (every dr is zero).
template <int L, class Y, class V, class DR>
PTV_VJP_HD void chunk_load_tangent(vjp::Chunk<L> &c, int len, bool has_next, bool has_prev, double yprev, bool inject, Y y, V v, DR dr) {
    vjp::chunk_load(c, len, has_next, y, v);
    if (!inject) return;
    double before = 0.0;
    if (has_prev) {
        const double y0 = y(0);
        if (vjp::is_step(yprev, y0)) before = y0 > yprev ? dr(-1) : -dr(-1);
    }
#pragma unroll
    for (int k = 0; k < L; k++) {
        if (k < len) {
            double behind = 0.0;
            if ((c.step >> k) & 1ull) behind = ((c.up >> k) & 1ull) ? dr(k) : -dr(k);
            c.g[k] += behind - before;
            before = behind;
        }
    }
}

}  // namespace jvp
}  // namespace ptv
