// solvers.hpp -- device-resident splitting loops (solvers.hip).  All pointers are HBM pointers.
#pragma once

#include "common.hpp"

namespace ptv {

struct SolveInfo {
    double iters = 0;
    double gap = 0;
    bool gap_set = false;  // DR / Yang leave info[INFO_GAP] untouched, like the reference
    int rc = RC_OK;
};

// out = prox along dimension `dim` of every fibre of `in` (uniform lam, or per-edge `weights`)
void tv1_fibres(const double *in, double *out, const int *ns, int nds, int dim, double lam, const double *weights,
                hipStream_t s);

// the certificate of such a sweep: fibres of `out` that are NOT the prox of the same fibre of `in` (-1: cannot be checked: lam <= 0, in == out)
long certify_fibres(const double *in, const double *out, const int *ns, int nds, int dim, double lam, const double *weights, hipStream_t s);

// the derivative of that prox at its output y (vjp.hip; formulas: vjpcore.hpp): gx = P g, gw (or null) the gradient in the edge
// penalties, nseg (or null) the segments of every fibre = trace P.  gx may be g.  Returns with the stream drained.
void tv1_fibres_vjp(const double *y, const double *g, double *gx, double *gw, int *nseg, const int *ns, int nds, int dim,
                    hipStream_t s);

// the step codes of y (vjpcore.hpp: one 32-bit word per chunk of 16 samples, all the derivative reads of y): tv1_steps_words of them, in
// the library's own order for this ns / dim; and the derivative above from those words.  gx == null: nseg alone.  Both drain the stream.
long tv1_steps_words(const int *ns, int nds, int dim);
void tv1_fibres_steps(const double *y, unsigned *steps, const int *ns, int nds, int dim, hipStream_t s);
void tv1_fibres_vjp_steps(const unsigned *steps, const double *g, double *gx, double *gw, int *nseg, const int *ns, int nds, int dim,
                          hipStream_t s);

// the derivative of dr2 (vjp.hip): runs the unfused recurrence with its 2 (maxit + 1) sweep outputs kept in pool scratch
// (dr2_vjp_tape_bytes; the caller checks it against pool_cap_bytes), then the reverse sweeps.  out / gW1 / gW2 / glam may be null; gU may
// be g, no other overlap.  glam: HOST double[2 B], (sum gW1, sum gW2) per image.  Returns with the stream drained.
// tape = 1: the sweeps write into two reused arrays and only the step codes of every output are kept (32 times less per output).
// norm1 / norm2 in {1, 2}: a TV-L2 direction's sweeps keep their output and multipliers under either tape and are
// differentiated by tv2_vjp.hip's write-out modes; it has no per-edge gradient (gW of that direction is ignored) and wants B == 1 and no
// weight maps.  Both 1: the launches, and so the bits, of the call without the arguments.
size_t dr2_vjp_tape_bytes(size_t M, size_t N, size_t B, int maxit, int tape, double norm1 = 1.0, double norm2 = 1.0);
void dr2_vjp(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, const double *W1m, const double *W2m, const double *g,
             double *out, double *gU, double *gW1, double *gW2, double *glam, int maxit, int tape, hipStream_t s, double norm1 = 1.0,
             double norm2 = 1.0);

// the derivative of pd2 (which == 0; npen <= 2) / pd (which == 1) with TV-L1 terms (vjp.hip): runs `iters` iterations of the
// unfused recurrence -- no stopping test, nothing read back -- with every sweep output kept in pool scratch (pd_vjp_tape_bytes; the caller
// checks it against pool_cap_bytes), then the reverse sweeps.  lambdas / dims: host, as pd2 / pd take them.  x / glam may be null; gy may be
// g, no other overlap.  glam: HOST double[npen], the gradient in `lambdas` as passed.  Returns with the stream drained.
// tape = 1: step codes of every output, and one reused array per term.
// norms (host, one of {1, 2} per term, or null = all 1): TV-L2 terms as for dr2_vjp; all 1: the launches of the call without the argument.
size_t pd_vjp_tape_bytes(int which, const double *dims, const int *ns, int nds, int npen, int iters, int tape, const double *norms = nullptr);
void pd_vjp(int which, const double *y, const double *lambdas, const double *dims, const int *ns, int nds, int npen, int iters, const double *g,
            double *x, double *gy, double *glam, int tape, hipStream_t s, const double *norms = nullptr);

// out = prox along `dim` with the TV-L1 (norm 1: the sweep kernels) or TV-L2 (norm 2: tv2.hip) penalty; in != out
void prox_fibres(const double *in, double *out, const int *ns, int nds, int dim, double lam, double norm, hipStream_t s);

// Douglas-Rachford on B stacked MxN images (B = 1: DR2_TV / DR2L1W_TV).  W1m/W2m != nullptr selects the weighted
// solver (per-edge penalties, (M-1)xN and Mx(N-1) per image); otherwise scalars W1 (columns) / W2 (rows).
SolveInfo dr2(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, const double *W1m,
              const double *W2m, double *out, int maxit, hipStream_t s);
// the same loop with a TV-L2 penalty in at least one direction (norms in {1, 2}): unfused steps
SolveInfo dr2_norms(size_t M, size_t N, const double *unary, double W1, double W2, double norm1, double norm2, double *out,
                    int maxit, hipStream_t s);

// `norms` (may be null = all 1): one of {1, 2} per penalty term
SolveInfo pd2(const double *y, const double *lambdas, const double *dims, double *x, const int *ns, int nds, int npen,
              int maxIters, hipStream_t s, const double *norms = nullptr);
// lambdas already scaled by npen (the C-ABI wrapper does the in-place scaling the reference does)
SolveInfo pd(const double *y, const double *lambdas, const double *dims, double *x, const int *ns, int nds, int npen,
             int maxIters, hipStream_t s, const double *norms = nullptr);
SolveInfo pdr(const double *y, const double *lambdas, const double *dims, double *x, const int *ns, int nds, int npen,
              int maxIters, hipStream_t s, const double *norms = nullptr);
// order[k] = 0-based dimension of the k-th (Z_k, U_k) pair, lambdas[k] its penalty
SolveInfo yang(const int *ns, int nds, const int *order, const double *lambdas, const double *Y, double *X, int maxit,
               hipStream_t s);

// Kolmogorov et al.'s primal-dual splitting, 2-D (src/TV2Dopt.cpp:907-1024)
SolveInfo kolmogorov2(size_t M, size_t N, const double *Y, double lambda, double *X, int maxit, hipStream_t s);
// Condat / Chambolle-Pock / accelerated Chambolle-Pock, 2-D (src/TV2Dopt.cpp:587-760); alg = 0 / 1 / 2
SolveInfo ccp2(size_t M, size_t N, const double *Y, double lambda, double *X, int alg, int maxit, hipStream_t s);

}  // namespace ptv
