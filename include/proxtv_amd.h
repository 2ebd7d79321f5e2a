/*
 * proxtv_amd.h -- C-ABI of libproxtv_amd.so, the MI355X (gfx950) TV-proximity library.
 *
 * PART 1 is the drop-in boundary: the same unmangled symbols, argument meaning, ownership and
 * return/info conventions as the reference's `extern "C"` block (reference: src/TVopt.h:88-141,
 * src/condat_fast_tv.h:76-81).  All pointers in part 1 are HOST pointers; the library stages them
 * to HBM, runs the HIP path and copies the result back.  Arrays are column-major (dimension 0
 * fastest), float64.  `info` is caller-owned double[3] or NULL: {iterations, gap/stop, return code}
 * (reference: src/general.h:58-73).  Functions never throw; a HIP failure or an unsupported
 * argument prints "<fn>: <reason>" to stdout like the reference's CANCEL macros, sets
 * info[2]=RC_ERROR and returns 0.  THERE IS NO CPU FALLBACK: without a usable gfx950 device every
 * entry point fails that way.
 *
 * PART 2 is new API (not in the reference): device-pointer entry points used by bench.py and by
 * callers that already hold data in HBM, plus the batch solver that shards independent images.
 *
 * Norms: p = 1 (TV-L1, the hot path of BASELINE.json) and p = 2 (TV-L2) have exact device solvers.  Every function
 * the reference's cffi cdef declares (prox_tv/prox_tv_build.py:13-76) is exported, so that cdef links against this
 * library unmodified: the alternative 1-D TV-L1 algorithms (projected Newton, Kolmogorov's and Johnson's solvers,
 * Condat's taut string) are entry points of the one exact solver -- the minimiser is unique -- and the general-p
 * TV-Lp schemes report RC_ERROR for p outside {1, 2} unless option general_p is set (below: then 1.002 < p < 100 is
 * served by the general-p fibre prox, proxtv_tvpg_fibres_dev).
 */
#ifndef PROXTV_AMD_H
#define PROXTV_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants shared with the reference ------------------------------------------------------ */
#define N_INFO 3              /* src/general.h:58 */
#define INFO_ITERS 0
#define INFO_GAP 1
#define INFO_RC 2
#define RC_OK 0               /* src/general.h:70-73 */
#define RC_ITERS 1
#define RC_STUCK 2
#define RC_ERROR 3
#define STOP_PD 1e-6          /* src/TVopt.h:71 */
#define MAX_ITERS_PD 35       /* src/TVopt.h:73 */
#define MAX_ITERS_DR 35       /* src/TVopt.h:83 */
#define MAX_ITERS_YANG 35     /* src/TVopt.h:85 */
#define MAX_ITERS_CONDAT 2500      /* src/TVopt.h:75 ; STOP_CONDAT = 0 (:77) */
#define MAX_ITERS_KOLMOGOROV 2500  /* src/TVopt.h:79 ; STOP_KOLMOGOROV = 0 (:81) */
#define ALG_CONDAT 0               /* src/TVopt.h: algorithm selector of CondatChambollePock2_TV */
#define ALG_CHAMBOLLE_POCK 1
#define ALG_CHAMBOLLE_POCK_ACC 2

/* Opaque, ABI-only (reference: src/utils.h:20-34).  The HIP path keeps its scratch in HBM and
   ignores workspaces; callers (like the reference's Python layer) pass NULL. */
typedef struct Workspace Workspace;

/* =============================== PART 1: drop-in entry points ================================== */

/* replaces src/TVgenopt.cpp:30 `TV` -- p == 1 (TV-L1, the hot path) and p == 2 (TV-L2); p < 1 or any other p ->
   RC_ERROR, returns 0 */
int TV(double *y, double lambda, double *x, double *info, int n, double p, Workspace *ws);
/* replace src/TVL2opt.cpp:35, :190, :446 -- the TV-L2 prox  min 1/2 ||x-y||^2 + lambda ||Dx||_2.  The three reference
   entry points are three iteration schemes for the same minimiser (which they reach to a duality gap of 1e-5, the
   hybrid one warm-started from its workspace); all are served by one exact device solve that depends on (y, lambda)
   only (tv2.hip).  info: iterations 0, gap 0, RC_OK. */
int more_TV2(double *y, double lambda, double *x, double *info, int n);
int morePG_TV2(double *y, double lambda, double *x, double *info, int n, Workspace *ws);
int PG_TV2(double *y, double lambda, double *x, double *info, int n);

/* replace src/TVL1opt.cpp:37 and src/TVL1Wopt.cpp:37 (projected Newton; `sigma`, its sufficient-descent tolerance, has no
   counterpart in an exact solve), src/TVL1opt_kolmogorov.cpp:133 and :38 (Kolmogorov et al.'s message passing; n <= 1
   handled like the reference), src/condat_fast_tv.cpp:133 (Condat's taut string) and src/johnsonRyanTV.cpp:9 (Johnson's
   dynamic programme; n == 0 / n == 1 / lam == 0 like the reference): the same unique minimiser as the entry points below,
   served by the same exact HIP solver.  info (where present): iterations 0, gap 0, RC_OK. */
int PN_TV1(double *y, double lambda, double *x, double *info, int n, double sigma, Workspace *ws);
int PN_TV1_Weighted(double *Y, double *W, double *X, double *info, int n, double sigma, Workspace *ws);
void SolveTVConvexQuadratic_a1_nw(int n, double *b, double w, double *solution);
void SolveTVConvexQuadratic_a1(int n, double *b, double *w, double *solution);
void TV1D_denoise_tautstring(double *input, double *output, int width, const double lambda);
void dp(int n, double *y, double lam, double *beta);
/* replace src/TVLPopt.cpp:37, :295, :583, :871, :1111 -- TV-Lp first-order schemes.  p == 1 and p == 2 are served by the
   exact solvers (like TV); any other p -> prints the reason, info[2] = RC_ERROR, returns 0. */
int GP_TVp(double *y, double lambda, double *x, double *info, int n, double p, Workspace *ws);
int OGP_TVp(double *y, double lambda, double *x, double *info, int n, double p, Workspace *ws);
int FISTA_TVp(double *y, double lambda, double *x, double *info, int n, double p, Workspace *ws);
int FW_TVp(double *y, double lambda, double *x, double *info, int n, double p, Workspace *ws);
int GPFW_TVp(double *y, double lambda, double *x, double *info, int n, double p, Workspace *ws);

/* replaces src/TVL1opt.cpp:359 */
int linearizedTautString_TV1(double *y, double lambda, double *x, int n);
/* replaces src/TVL1opt_tautstring.cpp:355 and :256 */
int classicTautString_TV1(double *signal, int n, double lam, double *prox);
int classicTautString_TV1_offset(double *signal, int n, double lam, double *prox, double offset);
/* replaces src/TVL1opt_hybridtautstring.cpp:237 and :56.  The 1-D TV-L1 prox is unique, so all
   five unweighted entry points run the same exact HIP solver; `backtracksexp` is accepted and has
   no observable effect on the result. */
void hybridTautString_TV1(double *y, int n, double lambda, double *x);
void hybridTautString_TV1_custom(double *y, int n, double lambda, double *x, double backtracksexp);
/* replaces src/TVL1Wopt.cpp:364 -- lambda has n-1 entries */
int tautString_TV1_Weighted(double *y, double *lambda, double *x, int n);
/* replaces src/condat_fast_tv.cpp:78 -- no-op when width <= 0 or lambda < 0; in-place allowed */
void TV1D_denoise(double *input, double *output, const int width, const double lambda);

/* replaces src/TV2Dopt.cpp:352 -- returns 0 on success (sic); norm1 / norm2 in {1, 2} (2: TV-L2 fibres, exact solve) */
int DR2_TV(size_t M, size_t N, double *unary, double W1, double W2, double norm1, double norm2,
           double *s, int nThreads, int maxit, double *info);
/* replaces src/TV2DWopt.cpp:46 -- W1 is (M-1)xN, W2 is Mx(N-1), column-major; returns 0 on success (sic) */
int DR2L1W_TV(size_t M, size_t N, double *unary, double *W1, double *W2, double *s, int nThreads,
              int maxit, double *info);
/* replaces src/TV2Dopt.cpp:59 -- npen in {1,2}; dims are 1-based doubles; norms in {1, 2} (here and below) */
int PD2_TV(double *y, double *lambdas, double *norms, double *dims, double *x, double *info, int *ns,
           int nds, int npen, int ncores, int maxIters);
/* replaces src/TVNDopt.cpp:48 -- multiplies lambdas[] by npen in caller memory, like the reference */
int PD_TV(double *y, double *lambdas, double *norms, double *dims, double *x, double *info, int *ns,
          int nds, int npen, int ncores, int maxIters);
/* replaces src/TVNDopt.cpp:280 -- multiplies lambdas[] by npen in caller memory, like the reference */
int PDR_TV(double *y, double *lambdas, double *norms, double *dims, double *x, double *info, int *ns,
           int nds, int npen, int ncores, int maxIters);
/* replaces src/TV2Dopt.cpp:787 */
int Yang2_TV(size_t M, size_t N, double *Y, double lambda, double *X, int maxit, double *info);
/* replaces src/TVNDopt.cpp:678 */
int Yang3_TV(size_t M, size_t N, size_t O, double *Y, double lambda, double *X, int maxit, double *info);
/* replaces src/TV2Dopt.cpp:907 -- Kolmogorov et al.'s primal-dual splitting of the same 2-D TV-L1 problem; both of
   its steps are 1-D proxes (columns through Moreau's identity, rows directly) and run on the sweep kernels.
   maxit <= 0 -> 2500; stops earlier only when X reaches a bitwise fixed point (STOP = 0); info[0] = iterations + 1 */
int Kolmogorov2_TV(size_t M, size_t N, double *Y, double lambda, double *X, int maxit, double *info);
/* replaces src/TV2Dopt.cpp:587 -- Condat (alg 0) / Chambolle-Pock (1) / accelerated Chambolle-Pock (2) primal-dual
   iterations: pointwise stencils, one fused kernel per iteration.  Images with a single row or column are rejected
   (the reference indexes out of bounds there). */
int CondatChambollePock2_TV(size_t M, size_t N, double *Y, double lambda, double *X, short alg, int maxit,
                            double *info);

/* Workspace allocator shims (reference: src/utils.cpp:79-237).  ABI-only: they return / accept
   small host objects so reference callers that create workspaces keep linking. */
Workspace *newWorkspace(int n);
void resetWorkspace(Workspace *ws);
void freeWorkspace(Workspace *ws);
Workspace **newWorkspaces(int n, int p);
void freeWorkspaces(Workspace **wa, int p);

/* =============================== PART 2: MI355X-native extensions ============================== */

/* Library / device state.  proxtv_init returns 0 when a gfx950 device is usable, else non-zero and
   prints the reason.  device < 0 keeps the current HIP device; device >= 0 makes it current (hipSetDevice).
   Everything the library keeps between calls (stream, scratch pool, chunk-kernel buffers, geometry policy) is
   per host thread AND per device: a thread may move between GPUs freely (hipSetDevice / proxtv_init), every entry
   point works on the device that is current when it is called, and pointers must belong to that device.
   Host threads never share state: concurrent calls from several threads are safe (options below are process-wide:
   set them before the threads start solving -- a change mid-solve takes effect at that solve's next sweep). */
int  proxtv_init(int device);
const char *proxtv_version(void);
const char *proxtv_last_error(void);
/* free every cached HBM scratch block held by the calling thread's pool on the current device (the pool is capped:
   PROXTV_POOL_CAP_MB, default 65536) */
void proxtv_release_scratch(void);

/* Knobs (process-wide; returns the previous value, -1 for an unknown key).  Each also has an environment variable
   PROXTV_<KEY> read at load time.  Twenty in all; none is needed for correct results.
     "runs"           1 (default): on rung 0, dimension-0 sweeps over data most of whose edges are bends known a priori (|dy| > 4 lambda)
                      cut the interior segments of their fibres at those bends and solve them run by run -- runs of one and two samples by
                      rule, longer ones walked one per lane: exact by construction, nothing speculated ; 0: speculative chunks everywhere
     "chunk_mode"     -1: the geometry policy chooses per sweep (default) ; 0..5: pin a rung of the ladder (see proxtv_chunk_mode)
     "deterministic"  1 (default): the rung of a sweep is a function of sampled statistics of its input and of lambda alone --
                      the same call gives the same bits whatever ran before ; 0: hill climb on measured sweep times, seeded by
                      the same statistics (results then agree to ~1e-13 between calls, not bit for bit)
     "chunk_min_len"  fibres shorter than this do not take the multi-block chunk kernels (default 96)
     "whole"          fibres of 16 .. chunk_min_len samples: 1 (default) by length and data, 2 whole fibres in LDS, 0 sequential
     "along"          1 (default): dimension-0 sweeps by chunks along the fibre ; 0: through the transposing 64-fibre tile
     "xlink"          1 (default): chunk kernels check the links across their workgroups themselves ; 0: the repair kernel does
     "dr_form"        DR2_TV / DR2L1W_TV: which sweep does the pointwise work of an iteration.  1 (default): the column sweep leaves
                      the row sweep's input and epilogue operand when the row sweep will run on the robust 64-fibre tile (decided
                      from the same sampled statistics as the rung) ; 2: on the plain tile too ; 0: never (the reference's split).
                      Same iterates either way, to a few ulps
     "pin"            1 (default): rung 3 is the pinning solver ; 0: the global-memory chunk kernel
     "pin_seed"       the pinning solver (rung 3) starts from the knots known a priori: 2 (default) jumps above 4 lambda and the
                      deepest knots of windows of 4 / 16 / 64 knots, 1: the jumps alone, 0: from the fibre ends alone
     "repair_jobs"    failed links across the workgroups of a chunked sweep are first repaired one lane per failure, four to a
                      fibre; what that leaves goes to the sequential repair: 1 (default) where the sampled statistic of the sweep's
                      input says such links fail in numbers (an unsampled input counts as such), 2 always ; 0: the sequential repair
                      alone (same results, bit for bit)
     "tile"           strided sweeps on rungs 0 and 1 (the robust instantiation follows the same knob): 1 (default) tiles of 32 fibres
                      x 8 chunks in 4 waves, four workgroups per CU ; 0: the 64-fibre x 8-wave tile, two per CU
     "optimistic"     1 (default): a DR solve whose every sweep will run on rung 0 launches no repair kernel behind its sweeps; a sweep
                      that leaves anything marks one word, read at the end, and such a solve is run again with the repairs (counters
                      optimistic_solves / optimistic_redone) ; 0: a repair launch behind every chunked sweep.  Same results, bit for bit
     "certify"        1: behind every fibre sweep a second kernel checks the optimality conditions of the prox on what the sweep wrote,
                      fibre by fibre (u = cumsum(y - x): |u_k| <= lambda_k ; u_k = -+lambda_k where x steps up / down ; u_{n-1} = 0),
                      re-solves a fibre that fails with the sequential walk and counts it (proxtv_debug_counter: certify_failures,
                      certify_sweeps, certify_skipped) ; 0 (default): sweeps are exact by their own argument and
                      the check costs a pass over the sweep's arrays
     "verbose"        1: log every decision of the geometry policy to stderr
     "profile"        1: hipEvent pair around every sweep launch (proxtv_last_kernel_ms / _launches)
     "why", "trace"   tuning / profiling aids (proxtv_debug_why, proxtv_debug_trace)
     "ablate"         profiling aid: skips phases of the chunk kernels -- RESULTS ARE WRONG while it is non-zero (a warning is printed)
     "debug_legacy_rebuild"   test aid: 1 plants the rebuild semantics of rounds 1-4 in the along-fibre kernel (an unproven chunk values
                      its first piece from its own first row: the hole of DESIGN.md 6 (ii')) so that the suite can watch the certifier catch
                      it -- RESULTS MAY BE WRONG while it is non-zero (a warning is printed) */
int proxtv_set_option(const char *key, int value);
/* One more key of proxtv_set_option, a feature switch rather than a tuning knob (environment: PROXTV_GENERAL_P):
     general_p      0 (default): every entry point refuses a norm p outside {1, 2} -- RC_ERROR, as it always has ;
                    1: TV, GP_TVp / OGP_TVp / FISTA_TVp / FW_TVp / GPFW_TVp, DR2_TV, PD2_TV, PD_TV and their device forms
                    proxtv_tvp_fibres_dev, proxtv_DR2_TVp_dev, proxtv_PD_TVp_dev (which = 0, 1) take 1.002 < p < 100 (the reference's own
                    LPPROJ_PSMALL / LPPROJ_PLARGE) and serve it with the general-p fibre prox below.  The 1-D host symbols then fill
                    info[0] = outer iterations, info[1] = the achieved duality gap, info[2] = RC_OK, or RC_ITERS where the iteration cap
                    was hit.  PDR_TV and the Yang solvers refuse such a norm whatever the option; the solver derivatives
                    (proxtv_DR2_TVp_vjp_dev, proxtv_PD_TVp_vjp_dev) refuse it unless general_p_vjp, below -- the fibre prox's own
                    derivative, proxtv_tvpg_fibres_vjp_dev, needs no option; p = inf and p >= 100 stay refused.  With 0 every entry
                    point's results are what they were without the key, bit for bit.
     general_p_vjp  (environment: PROXTV_GENERAL_P_VJP) 0 (default): the solver derivatives refuse a norm outside {1, 2}, as they always
                    have ; 1: proxtv_DR2_TVp_vjp_dev and proxtv_PD_TVp_vjp_dev take 1.002 < p < 100 per direction / term (below).  The
                    calls replay the forward themselves: general_p is not asked.  With 1 and every norm in {1, 2} they run the launches
                    and return the bits of 0.
     tvp_vjp_route  debugging aid: where the write-out of a general-p reverse sweep runs -- 0 (default) by the fibre count, 1 inside the
                    fibre kernel wherever legal, 2 as a pointwise pass behind the plain kernel everywhere.  The same bits all three.
     dr_jvp_route   debugging aid: where proxtv_DR2_TV_jvp_dev forms the three-array tangent of a row sweep -- 0 (default) the measured
                    choice, 1 inside the loads of the sweep's two passes, 2 as one pointwise pass in front.  The same bits all three. */

/* Device-pointer solvers: every double* is an HBM pointer valid on the current device, `stream` is
   a hipStream_t (NULL = the library's per-thread stream), `info` is a HOST double[3] or NULL.
   Work is enqueued AND completed (the call synchronises `stream`) unless `info` is NULL and
   PD-type stopping is not involved; see DESIGN.md.  Same return conventions as part 1.
   Aliasing: an output array may overlap an input (in-place use); the solve then runs into a scratch array that is
   copied over the caller's at the end -- one extra pass; distinct arrays cost nothing. */
int proxtv_DR2_TV_dev(size_t M, size_t N, const double *unary, double W1, double W2, double *s,
                      int maxit, double *info, void *stream);
int proxtv_DR2L1W_TV_dev(size_t M, size_t N, const double *unary, const double *W1, const double *W2,
                         double *s, int maxit, double *info, void *stream);
int proxtv_PD2_TV_dev(const double *y, const double *lambdas /*host*/, const double *dims /*host*/,
                      double *x, double *info, const int *ns /*host*/, int nds, int npen, int maxIters,
                      void *stream);
int proxtv_PD_TV_dev(const double *y, const double *lambdas_scaled /*host, already * npen*/,
                     const double *dims /*host*/, double *x, double *info, const int *ns /*host*/,
                     int nds, int npen, int maxIters, void *stream);
int proxtv_PDR_TV_dev(const double *y, const double *lambdas_scaled /*host*/, const double *dims /*host*/,
                      double *x, double *info, const int *ns /*host*/, int nds, int npen, int maxIters,
                      void *stream);
/* Yang ADMM on a 2-D or 3-D array with one lambda per dimension (scalar-lambda reference behaviour
   when all entries are equal).  order follows the reference: 2-D rows then columns, 3-D dims 1,2,3. */
int proxtv_Yang_TV_dev(const int *ns /*host*/, int nds, const double *Y, const double *lambdas /*host, nds*/,
                       double *X, int maxit, double *info, void *stream);
int proxtv_Kolmogorov2_TV_dev(size_t M, size_t N, const double *Y, double lambda, double *X, int maxit, double *info,
                              void *stream);
int proxtv_CondatChambollePock2_TV_dev(size_t M, size_t N, const double *Y, double lambda, double *X, short alg,
                                       int maxit, double *info, void *stream);

/* Batched exact 1-D TV-L1 prox along one dimension of an N-D column-major array (the per-sweep
   kernel of every solver above): out = prox_{lambda}(in) on every fibre along dimension `dim`
   (0-based).  weights == NULL -> uniform lambda; otherwise `weights` has the shape of `in` with
   ns[dim] reduced by one and holds per-edge penalties. */
int proxtv_tv1_fibres_dev(const double *in, double *out, const int *ns /*host*/, int nds, int dim,
                          double lambda, const double *weights, void *stream);

/* The certificate of that prox, on its own: the number of fibres along `dim` for which `out` is NOT the exact TV-L1 prox of `in` --
   the optimality conditions of the 1-D problem checked fibre by fibre (u = cumsum(in - out): |u_k| <= lambda_k, u_k = -+lambda_k where
   out steps up / down, u_{n-1} = 0; reference: what src/TVL1opt.cpp:359-564 solves), within rounding (64 n ulps of the largest sample)
   plus the 4e-10 the reference's own EPSILON tests at a fibre's last sample leave in those sums.
   0 = `out` is the prox; -1 = nothing to check against (lambda <= 0 without weights, in == out); -2 = the call failed
   (proxtv_last_error).  Read-only on both arrays; synchronises the stream.  Option "certify" runs the same check behind every sweep
   of every solver and repairs what fails. */
long proxtv_certify_fibres_dev(const double *in, const double *out, const int *ns /*host*/, int nds, int dim, double lambda,
                               const double *weights, void *stream);

/* The derivative of that prox, at its output: y is what proxtv_tv1_fibres_dev returned for the same ns / dim (no lambda and no weights
   are needed).  Edge k of a fibre is a STEP iff |y[k+1] - y[k]| > 256 * 2^-52 * max(|y[k]|, |y[k+1]|) + 4e-10 (the certifier's constants);
   segments are the maximal runs of samples between steps, and wherever the prox is differentiable its Jacobian P = dy/dx replaces every
   sample by the mean over its segment.  P is symmetric, so this one call is the VJP and the JVP in x:
     gx = P g                                      (shape of y; gx may be g itself)
     gw[k] = sigma_k (gx[k] - gx[k+1])             (gw or NULL: ns[dim] reduced by one, the gradient in the penalty of edge k -- for a uniform
                                                    lambda, d/dlambda is the sum of gw; sigma_k = +1 / -1 on a step up / down, and gw = 0
                                                    exactly on an edge that is no step)
     nseg[j] = segments of fibre j = trace of P    (nseg or NULL: one int per fibre, in the column-major order of the array with `dim`
                                                    removed; the degrees of freedom SURE asks for)
   Two limits of the rule: at a kink -- a jump that is zero up to the rule -- the prox is not differentiable and the merged segment is
   what comes out; and the absolute 4e-10 makes data far below 1e-9 in magnitude one segment per fibre.  ns[dim] == 1: gx = g, nothing is
   written to gw.  gx == NULL (g may then be NULL too): only nseg is computed, in one pass over y.  No atomics: the same call gives the
   same bits.  Synchronises the stream; returns 1, or 0 with proxtv_last_error set. */
int proxtv_tv1_fibres_vjp_dev(const double *y, const double *g, double *gx /*or NULL*/, double *gw /*or NULL*/, int *nseg /*or NULL*/,
                              const int *ns /*host*/, int nds, int dim, void *stream);

/* The derivative of the 2-D Douglas-Rachford solves (DR2_TV / DR2L1W_TV / the batch), on B images stored back to back: for the cotangent
   g of the result,
     gU          the gradient in `unary`                                    (M x N per image; gU may be g itself)
     gW1, gW2    the gradients in the per-edge penalties, or NULL           ((M-1) x N and M x (N-1) per image: the shapes of W1m / W2m.  Also
                                                                             with uniform W1 / W2, where they hold the per-edge terms)
     glam        HOST double[2 B] or NULL: (sum gW1, sum gW2) per image     (the gradients in uniform W1 / W2)
     s           the forward result, or NULL
   W1m and W2m both given: the weighted solve (W1, W2 are ignored); both NULL: the uniform one.  The call is self-contained: it runs the
   UNFUSED forward recurrence (t0 = 2 mean(U); x1 = prox_cols(t), x2 = prox_rows(U - t + 2 x1), t <- t - x1 + x2; a final pair of sweeps),
   keeping the 2 (maxit + 1) sweep outputs in pool scratch -- 2 (maxit + 1) * 8 * M * N * B bytes; beyond the pool's cap
   (PROXTV_POOL_CAP_MB) the call is refused and proxtv_last_error names the bytes -- and then applies proxtv_tv1_fibres_vjp_dev's segmented
   means sweep by sweep, last sweep first, with the pointwise work of the recurrence inside those kernels.  What comes out is the
   derivative of that recurrence: its forward agrees with proxtv_DR2_TV_dev's fused sweeps to rounding, not bit for bit.  The step rule and
   its two limits (kinks; the absolute 4e-10) are proxtv_tv1_fibres_vjp_dev's.  maxit <= 0: 35.  M*N*B == 0: returns 1, nothing is written.
   M == 1 or N == 1 is fine.  No array may overlap another, except gU == g; exactly one weight map, a missing unary / g / gU, an overlap or
   a tape beyond the cap: returns 0 with proxtv_last_error set and nothing written.  No atomics: the same call gives the same bits, and an
   image of a batch the bits of its own call.  Synchronises the stream; returns 1 on success. */
int proxtv_DR2_TV_vjp_dev(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, const double *W1m /*or NULL*/,
                          const double *W2m /*or NULL*/, const double *g, double *s /*or NULL*/, double *gU, double *gW1 /*or NULL*/,
                          double *gW2 /*or NULL*/, double *glam /*host, or NULL*/, int maxit, void *stream);

/* Forward mode.  The tangent of proxtv_tv1_fibres_dev at its output y, for tangents dx of the input and dr of the per-edge
   penalties.  With sigma_k = +1 / -1 on a step up / down of y and 0 on an edge that is none (the rule above),
     E[i] = sigma_i dr_i - sigma_{i-1} dr_{i-1}     (sample i of a fibre; an edge outside the fibre contributes 0)
     dy   = P (dx + E)                              (shape of y; dy may be dx itself)
   where dr_k = dw[k] + dlam: dw (or NULL: zero) has the shape and layout of gw above, dlam is the tangent of a uniform lambda.  dx NULL:
   zero.  This is the exact transpose of proxtv_tv1_fibres_vjp_dev: <g, dy> = <gx, dx> + <gw, dr> for every g.  The limits are that
   call's (kinks; the absolute 4e-10).  ns[dim] == 1: dy = dx.  Every tangent absent or zero: dy is exactly zero.  No array may overlap
   another, except dy == dx; an overlap, a missing y / dy or a dimension out of range: returns 0 with proxtv_last_error set and nothing
   written.  A total size of 0: returns 1.  No atomics: the same call gives the same bits.  Synchronises the stream; returns 1 on success. */
int proxtv_tv1_fibres_jvp_dev(const double *y, const double *dx /*or NULL: zero*/, const double *dw /*per-edge, shape of gw, or NULL*/,
                              double dlam /*uniform tangent, added on every edge*/, double *dy /*may be dx*/, const int *ns /*host*/,
                              int nds, int dim, void *stream);

/* The tangent of the 2-D Douglas-Rachford solves (DR2_TV / DR2L1W_TV / the batch), on B images stored back to back, for tangents
     dU          of `unary`, or NULL (zero)                                 (M x N per image)
     dW1m, dW2m  of the per-edge penalties, or NULL (zero), each on its own ((M-1) x N and M x (N-1) per image; also with uniform W1 / W2)
     dW1, dW2    of uniform penalties, added on every edge of their direction
     ds          the tangent of the result                                  (M x N per image)
     s           the forward result, or NULL
   W1m / W2m as for proxtv_DR2_TV_vjp_dev: both (the weighted solve) or neither.  The call differentiates the UNFUSED recurrence that
   proxtv_DR2_TV_vjp_dev replays, sweep by sweep next to the forward: dt = 2 mean(dU); dx1 = P_c(x1)[dt + E(dW1)],
   dx2 = P_r(x2)[dU - dt + 2 dx1 + E(dW2)], dt <- dt - dx1 + dx2; a final pair, ds = P_r(x2)[dU - dt + dx1 + E(dW2)].  Nothing is kept
   between iterations but t and dt: the scratch is six arrays of the data's size plus 4 bytes a sample of chunk records, whatever maxit
   (beyond the pool's cap, PROXTV_POOL_CAP_MB, the call is refused and proxtv_last_error names the bytes).  <g, ds> equals
   <gU, dU> + <gW1, dW1m + dW1> + <gW2, dW2m + dW2> of proxtv_DR2_TV_vjp_dev up to rounding, and s is that call's s bit for bit.  Limits:
   those of proxtv_DR2_TV_vjp_dev.  maxit <= 0: 35.  M*N*B == 0: returns 1, nothing is written.  M == 1 or N == 1 is fine.  Every tangent
   absent or zero: ds is exactly zero.  Exactly one weight map, a missing unary / ds, any overlap: returns 0 with proxtv_last_error set and
   nothing written.  No atomics: the same call gives the same bits, and an image of a batch the bits of its own call.  Synchronises the
   stream; returns 1 on success. */
int proxtv_DR2_TV_jvp_dev(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, const double *W1m /*or NULL*/,
                          const double *W2m /*or NULL*/, const double *dU /*or NULL*/, const double *dW1m /*or NULL*/,
                          const double *dW2m /*or NULL*/, double dW1, double dW2, double *s /*forward result, or NULL*/, double *ds,
                          int maxit, void *stream);

/* The derivative of the two Dykstra loops tvgen dispatches to, with TV-L1 terms on an N-D array: which = 0, proxtv_PD2_TV_dev (one or two
   terms); which = 1, proxtv_PD_TV_dev (any number of terms, several may share a dimension).  For the cotangent g of the result,
     gy          the gradient in y                                          (shape of y; gy may be g itself)
     glam        HOST double[npen] or NULL: the gradient in `lambdas` AS PASSED -- for which = 1 those are the npen-scaled values the
                 forward entry point takes, so the gradient in the user's penalties is npen times this
     x           the forward result, or NULL
   `iters` is an INPUT: the iteration count the forward solve reported in info[0].  The call is self-contained: it runs exactly `iters`
   iterations of the UNFUSED recurrence -- it tests no stopping value and reads nothing back -- keeping every sweep output in pool scratch
   (which = 1: npen * iters arrays of y's size; which = 0: 2 * iters, or one for a single term, where every iteration repeats the first;
   beyond the pool's cap, PROXTV_POOL_CAP_MB, the call is refused and proxtv_last_error names the bytes), and then applies
   proxtv_tv1_fibres_vjp_dev's segmented means sweep by sweep, last iteration first, with the pointwise work of the reverse recurrence
   inside those kernels.  What comes out is the derivative of the `iters`-step recurrence.  Limits: the dependence of the iteration count
   on the data through the stopping rule is NOT differentiated; the step rule and its two limits (kinks; the absolute 4e-10) are
   proxtv_tv1_fibres_vjp_dev's; the forward agrees with the fused solve to rounding, not bit for bit.  Per-edge weight maps are not
   covered; TV-L2 terms are, by proxtv_PD_TVp_vjp_dev below (this entry has no `norms` argument: every term is TV-L1).  A total size of 0: returns 1, nothing is written.  iters < 1, which = 0 with npen > 2,
   a dimension out of range, a missing y / g / gy, any overlap except gy == g, or a tape beyond the cap: returns 0 with proxtv_last_error
   set and nothing written.  No atomics: the same call gives the same bits.  Synchronises the stream; returns 1 on success. */
int proxtv_PD_TV_vjp_dev(int which /*0: PD2_TV, 1: PD_TV*/, const double *y, const double *lambdas /*host, as the forward takes them*/,
                         const double *dims /*host, 1-based*/, const int *ns /*host*/, int nds, int npen, int iters, const double *g,
                         double *x /*forward result, or NULL*/, double *gy /*may be g*/, double *glam /*host double[npen], or NULL*/,
                         void *stream);

/* Step codes: all that the three derivatives above read of a sweep output y, at 2 bits a sample instead of 64.  One 32-bit word per
   chunk of 16 consecutive samples of a fibre (the last chunk of a fibre may be short):
     bit k      (k < 16)   the edge behind sample k of the chunk -- between it and the fibre's next sample -- is a STEP (the rule above)
     bit 16 + k            that step goes up (y[k+1] > y[k])
   and every bit of an edge the chunk does not own is 0: beyond a short last chunk, and behind the fibre's last sample.  So
   popcount(word & 0xffff) summed over a fibre is its segments less one, and (word >> 16) & ~word & 0xffff is 0.  The bit format is
   public; the ORDER of the words is the library's own (it follows the layout of the kernels' scratch records, so it depends on ns and
   dim) and holds for the same ns and dim on the same build.  A derivative computed from the words is the same bits as the one computed
   from y: the kernels take nothing else from y.
   proxtv_tv1_steps_words: how many words an array has along `dim`: (fibres) * ceil(ns[dim] / 16); 0 for an empty array; -1 with
   proxtv_last_error set for a dimension out of range.  Needs no device.
   proxtv_tv1_fibres_steps_dev: steps[proxtv_tv1_steps_words(...)] <- the codes of y.  One pass over y, no atomics: the same words every
   call.  steps must not overlap y.  Synchronises the stream; returns 1, or 0 with proxtv_last_error set.
   proxtv_tv1_fibres_vjp_steps_dev: proxtv_tv1_fibres_vjp_dev with those words in place of y -- the same arguments, rules and results
   (gx may be g; ns[dim] == 1: gx = g; gx == NULL: nseg alone, read off the words). */
long proxtv_tv1_steps_words(const int *ns /*host*/, int nds, int dim);
int proxtv_tv1_fibres_steps_dev(const double *y, unsigned *steps, const int *ns /*host*/, int nds, int dim, void *stream);
int proxtv_tv1_fibres_vjp_steps_dev(const unsigned *steps, const double *g, double *gx /*or NULL*/, double *gw /*or NULL*/,
                                    int *nseg /*or NULL*/, const int *ns /*host*/, int nds, int dim, void *stream);

/* proxtv_DR2_TV_vjp_dev / proxtv_PD_TV_vjp_dev with the choice of what the forward keeps for the reverse sweeps:
     tape = 0   every sweep output, as float64: the two calls above, bit for bit
     tape = 1   the step codes of every sweep output: each sweep writes into an array that the next iteration reuses (two arrays for
                Douglas-Rachford and PD2, npen for PD) and is encoded behind its sweep.  What is kept, and what is held against the
                pool's cap, is 4 bytes per 16 samples and sweep plus those arrays: for Douglas-Rachford
                (maxit + 1) * 4 * (words along dimension 0 + words along dimension 1) + 2 * 8 * M * N * B bytes.
   Every result is the same bits for both tapes.  Any other value of `tape`: returns 0 with proxtv_last_error set and nothing written.
   All else as documented above. */
int proxtv_DR2_TV_vjp_tape_dev(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, const double *W1m /*or NULL*/,
                               const double *W2m /*or NULL*/, const double *g, double *s /*or NULL*/, double *gU, double *gW1 /*or NULL*/,
                               double *gW2 /*or NULL*/, double *glam /*host, or NULL*/, int maxit, int tape, void *stream);
int proxtv_PD_TV_vjp_tape_dev(int which /*0: PD2_TV, 1: PD_TV*/, const double *y, const double *lambdas /*host*/,
                              const double *dims /*host, 1-based*/, const int *ns /*host*/, int nds, int npen, int iters, const double *g,
                              double *x /*forward result, or NULL*/, double *gy /*may be g*/, double *glam /*host double[npen], or NULL*/,
                              int tape, void *stream);

/* Batch of B independent MxN images stored back to back (image b at unary + b*M*N), each solved
   with DR2_TV semantics (oracle = loop of DR2_TV).  All B images advance together, one
   launch per sweep over B*N (columns) / B*M (rows) fibres. */
int proxtv_DR2_TV_batch_dev(size_t M, size_t N, size_t B, const double *unary, double W1, double W2,
                            double *s, int maxit, double *info, void *stream);

/* Same on HOST pointers (stages through HBM like part 1). */
int proxtv_DR2_TV_batch(size_t M, size_t N, size_t B, const double *unary, double W1, double W2, double *s,
                        int maxit, double *info);

/* The same solvers with a TV-L2 penalty (p = 2: lambda ||Dx||_2 per fibre, exact trust-region solve, tv2.hip) allowed
   per dimension / per term; norms in {1, 2}.  proxtv_PD_TVp_dev: which = 0 PD2_TV, 1 PD_TV, 2 PDR_TV (lambdas already
   scaled by npen for 1 and 2, like proxtv_PD_TV_dev). */
int proxtv_tvp_fibres_dev(const double *in, double *out, const int *ns, int nds, int dim, double lambda, double p,
                          void *stream);
int proxtv_DR2_TVp_dev(size_t M, size_t N, const double *unary, double W1, double W2, double norm1, double norm2,
                       double *s, int maxit, double *info, void *stream);

/* The TV-Lp fibre prox for general p, always available (no option): out = argmin 1/2 ||x - in||^2 + lambda ||Dx||_p along `dim` of every
   fibre, 1.002 < p < 100.  p = 1 and p = 2 go to the exact solvers above and return their bits (gap is then 0); any other p: returns 0 with
   proxtv_last_error set.  Per fibre, with q = p / (p - 1): n == 1 or lambda <= 0 -- a copy; T^-1 D in inside the ball ||u||_q <= lambda --
   the mean; otherwise the dual min 1/2 ||D'u - in||^2 over that ball is solved by nested Newton iterations on its KKT system (every step
   one tridiagonal LDL' sweep) and out = in - D'u, which keeps the fibre's mean.  The iteration stops on the fibre's own
   duality gap, lambda ||D out||_p - u'D out, at max(1e-8, 4e-13 * 1/2 ||in - mean||^2) -- the reference's solvers stop at 1e-5 -- and
   a hard cap of 1500 forward sweeps bounds every fibre's work: a fibre that gets there keeps its best feasible iterate and is counted.
     gap         DEVICE double per fibre, or NULL: the achieved gap, laid out as mu of proxtv_tv2_fibres_dev; 0 for the closed forms
   Counters (proxtv_debug_counter): "tvp_fibres", fibres solved iteratively; "tvp_capped", fibres the cap stopped above their target.
   One lane per fibre: a single long fibre runs on one lane (DESIGN.md 6h gives the bound).  Scratch comes from the pool -- four arrays of
   the data's size, six along dimension 0, 12 bytes per fibre; beyond the pool's cap (PROXTV_POOL_CAP_MB) the call is refused and
   proxtv_last_error names the bytes.  out may overlap in (the solve then goes through scratch); gap may overlap neither.  No atomics, no
   warm start across fibres: a fibre's result depends on that fibre alone and the same call gives the same bits.  Synchronises the stream;
   returns 1, or 0 with proxtv_last_error set. */
int proxtv_tvpg_fibres_dev(const double *in, double *out, double *gap /*or NULL*/, const int *ns /*host*/, int nds, int dim, double lambda,
                           double p, void *stream);

/* The derivative of that prox for a general p (1.002 < p < 100, p != 2): y is what proxtv_tvpg_fibres_dev returned for the same ns / dim /
   lambda / p -- the output, lambda and p are all it needs: no multiplier, no tape.  Per fibre of n samples, D the (n-1) x n difference
   matrix, T = D D', w = D y, N = ||w||_p, s_i = |w_i| / N, q = p / (p - 1), phi_i = sign(w_i) s_i^(p-1), a cotangent g:
     J = (I + lambda D' H D)^-1,  H = (p-1)/N (diag s^(p-2) - phi phi'), applied in the arm where every power has an exponent >= 0
     p > 2       M = I + lambda D' diag((p-1)/N s^(p-2)) D,  b = D' phi,  c = lambda (p-1) / N,  a = M^-1 g,  e = M^-1 b
                 gx = a + c (b'a) / (1 - c b'e) e                           (shape of y; gx may be g itself)
     p < 2       H = T + diag((q-1) N / lambda s^(2-p)),  h = D g,  a = H^-1 h,  e = H^-1 w
                 gx = g - D'(a - (w'a) / (w'e) e)
     both        glam = -gx' D' phi                                         (glam or NULL: DEVICE double per fibre, laid out as gap; for one
                                                                             lambda shared by all fibres d/dlambda is the sum of glam)
     y constant along the fibre (N == 0 exactly):  gx = mean(g) on every sample, glam = 0
     ns[dim] == 1 or lambda <= 0:  gx = g, glam = 0
   The Jacobian is symmetric, so this one call is the VJP and the JVP in x.  The branch the forward took is what is differentiated: where
   it answered with the fibre's mean (the dual inside the ball, or its capped fall-back) it stored the mean itself on every sample, and
   that is what N == 0 recognises.  Four passes per fibre -- the largest |w_i|, N, one forward elimination of the tridiagonal matrix on both
   right-hand sides, which also yields both scalar products, one backward substitution on the combined vector -- against the forward's
   30-100.  One lane per fibre, a single long fibre on one lane, as in the forward.  Scratch comes from the pool -- three arrays of the
   data's size, five along dimension 0; beyond the pool's cap (PROXTV_POOL_CAP_MB) the call is refused and proxtv_last_error names the
   bytes.  A total size of 0: returns 1, nothing is written.  A missing y / g / gx, a dimension out of range, any overlap except gx == g,
   or a p this solver does not take -- p = 1 and p = 2 among them: their derivatives are proxtv_tv1_fibres_vjp_dev and
   proxtv_tv2_fibres_vjp_dev -- returns 0 with proxtv_last_error set and nothing written.  No atomics: a fibre's bits depend on that fibre
   alone and the same call gives the same bits.  Synchronises the stream; returns 1 on success.  A general p inside the solver derivatives
   (proxtv_DR2_TVp_vjp_dev, proxtv_PD_TVp_vjp_dev) is refused unless option general_p_vjp. */
int proxtv_tvpg_fibres_vjp_dev(const double *y, const double *g, double *gx /*may be g*/, double *glam /*device, one per fibre, or NULL*/,
                               const int *ns /*host*/, int nds, int dim, double lambda, double p, void *stream);

/* The TV-L2 fibre prox on its own, with its multiplier: out = argmin 1/2 ||x - in||^2 + lambda ||Dx||_2 along `dim` of every fibre --
   the bits of proxtv_tvp_fibres_dev(p = 2).  Per fibre of n samples, D the (n-1) x n difference matrix and T = D D' = tridiag(-1, 2, -1):
   out = in - D'u, where either u = T^-1 D in lies inside the ball ||u|| <= lambda (out is then the mean of in), or (T + mu I) u = D in
   with ||u|| = lambda and mu > 0 (then D out = mu u, so mu = ||D out|| / lambda).
     mu          DEVICE double per fibre, or NULL: that multiplier, in the column-major order of the array with `dim` removed (as nseg is
                 laid out for TV-L1).  Exactly 0.0 where u lies inside the ball, for ns[dim] == 1 and for lambda <= 0.  The case cannot be
                 read off `out` in floating point (inside the ball D out is ~1e-17, not 0), which is why it is an output.  0.0 can also
                 mean "active by less than one Newton step": where ||T^-1 D in|| exceeds lambda by a rounding margin and the first
                 Newton step does not raise mu, the iteration stops at mu = 0 and `out` is the mean up to that margin -- the kink.
   out may overlap in (the solve then goes through scratch); mu may overlap neither.  A total size of 0: returns 1, nothing is written.
   Synchronises the stream; returns 1, or 0 with proxtv_last_error set. */
int proxtv_tv2_fibres_dev(const double *in, double *out, double *mu /*or NULL*/, const int *ns /*host*/, int nds, int dim, double lambda,
                          void *stream);

/* The derivative of that prox: y and mu are what proxtv_tv2_fibres_dev returned for the same ns / dim / lambda.  With M = T + mu I
   (symmetric positive definite), a cotangent g and h = D g, per fibre:
     mu > 0      p = M^-1 h,  q = M^-1 (D y),  kappa = (h'q) / ((D y)'q)
                 gx = g - D'(p - kappa q)                                   (shape of y; gx may be g itself)
                 glam = -mu lambda kappa                                    (glam or NULL: DEVICE double per fibre, laid out as mu; for one
                                                                             lambda shared by all fibres d/dlambda is the sum of glam)
     mu == 0     gx = mean(g) on every sample, glam = 0
     ns[dim] == 1 or lambda <= 0:  gx = g, glam = 0
   The Jacobian is symmetric, so this one call is the VJP and the JVP in x.  At the kink ||T^-1 D x|| = lambda the prox is not
   differentiable: mu records the branch the forward took and that branch's derivative is what comes out.  Two passes per fibre -- one
   forward elimination on both right-hand sides, which also yields both dot products of kappa, one backward substitution on the combined
   vector -- against the forward's 3-9 Newton iterations of two solves each; a few long contiguous fibres (>= 16384 samples, the forward's
   own condition) are solved parallel inside the fibre.  Scratch comes from the pool.  A total size of 0: returns 1, nothing is written.
   A missing y / mu / g / gx, a dimension out of range, or any overlap except gx == g: returns 0 with proxtv_last_error set and nothing
   written.  No atomics: the same call gives the same bits.  Synchronises the stream; returns 1 on success. */
int proxtv_tv2_fibres_vjp_dev(const double *y, const double *mu, const double *g, double *gx /*may be g*/,
                              double *glam /*device, one per fibre, or NULL*/, const int *ns /*host*/, int nds, int dim, double lambda,
                              void *stream);
int proxtv_PD_TVp_dev(int which, const double *y, const double *lambdas_scaled, const double *norms, const double *dims,
                      double *x, double *info, const int *ns, int nds, int npen, int maxIters, void *stream);

/* The derivatives of proxtv_DR2_TVp_dev and of proxtv_PD_TVp_dev (which = 0 / 1): proxtv_DR2_TV_vjp_tape_dev and proxtv_PD_TV_vjp_tape_dev
   with a norm in {1, 2} per direction / per term.  Arguments, conventions and limits are those two calls': returns 1 on success, 0 with
   proxtv_last_error set and nothing written on a bad argument; overlap only as gU == g / gy == g; an empty array returns 1; glam for
   which = 1 is in the lambdas as passed; `iters` is the forward's reported count.  A norm outside {1, 2}: returns 0 with the error set.
   The recurrences are the same ones; a TV-L1 sweep is differentiated by its segmented mean as before, a TV-L2 sweep by
   proxtv_tv2_fibres_vjp_dev's two solves, with the pointwise work of the reverse recurrence inside that kernel for fibres along a
   dimension >= 1 (dimension-0 fibres and fibres of >= 16384 samples: the plain kernel and one pointwise pass).  With every norm 1, or
   norms == NULL, the result is the bits of the TV-L1 call.
   The Douglas-Rachford entry takes one uniform image: TV-L2 has no per-edge weights and proxtv_DR2_TVp_dev has no batch.
     glam        HOST double[2] (DR: d/dW1, d/dW2) / double[npen], or NULL.  For a TV-L2 term it is the sum over the fibres of
                 proxtv_tv2_fibres_vjp_dev's glam, in sum_to's fixed order.
   The kink: where a TV-L2 fibre's forward sweep took the mu = 0 branch (its dual inside the ball, or active by less than a Newton step),
   that branch is what is differentiated -- the rule of proxtv_tv2_fibres_vjp_dev, sweep by sweep.
   The tape.  A TV-L1 sweep keeps its float64 output (tape = 0) or its step codes (tape = 1) as before.  A TV-L2 sweep keeps its float64
   output AND its multipliers, one double per fibre, under either tape: its derivative reads D y itself.  Bytes held against the pool's
   cap, summed over the directions / terms d, with n the array's size, K the sweeps per term (DR: maxit + 1; PD: iters; PD2 with one
   term: 1), words_d = proxtv_tv1_steps_words along d and fibres_d = n / ns[d]:
       TV-L1, tape = 0:  8 K n          TV-L1, tape = 1:  8 n + 4 K words_d          TV-L2, either tape:  8 K (n + fibres_d)
       a general p, either tape:  8 K n
   Every result is the same bits for both tapes.  No atomics: the same call gives the same bits.
   With option general_p_vjp = 1 a norm may also be any 1.002 < p < 100 (p = inf, p >= 100 and p <= 1.002 stay refused and the error
   names the range; with the option 0 every such norm is refused as before).  Such a sweep is proxtv_tvpg_fibres_dev's forward and
   proxtv_tvpg_fibres_vjp_dev's derivative -- from the sweep's output, lambda and p alone -- with the recurrence's pointwise work inside
   that kernel or in one pointwise pass behind it (always for dimension-0 fibres; the same bits either way).  It keeps its float64 output
   and nothing else, under either tape.  glam for such a term is the sum over the fibres of proxtv_tvpg_fibres_vjp_dev's glam.  The branch
   rule is that call's, sweep by sweep: a constant output fibre differentiates as the mean, ns[d] == 1 or lambda <= 0 as the identity, a
   fibre the forward's iteration cap stopped at the output it returned.  Before anything runs, three sizes are held against the pool's cap
   and a call beyond it is refused with the bytes named and nothing written: the tape (above); per general-p term its forward scratch,
   8 n * 4 (8 n * 6 along dimension 0 of several fibres) + 12 fibres_d + 32; and its reverse scratch, 8 n * 3 (8 n * 5 along dimension 0
   of several fibres), plus, where the write-out is a pass of its own, 8 n (16 n for which = 1) and 8 fibres_d when glam is asked for.
   Not differentiated: the iteration count, p itself, the forward's stopping error. */
int proxtv_DR2_TVp_vjp_dev(size_t M, size_t N, const double *unary, double W1, double W2, double norm1, double norm2, const double *g,
                           double *s /*or NULL*/, double *gU, double *glam /*host double[2], or NULL*/, int maxit, int tape, void *stream);
int proxtv_PD_TVp_vjp_dev(int which, const double *y, const double *lambdas, const double *norms /*host, or NULL*/, const double *dims,
                          const int *ns, int nds, int npen, int iters, const double *g, double *x /*or NULL*/, double *gy /*may be g*/,
                          double *glam /*host, or NULL*/, int tape, void *stream);

/* Timing hook for bench.py: average device time in milliseconds of the `which`-th kernel family
   over the last solve (0 = column sweep, 1 = row sweep, 2 = everything else), measured with
   hipEvents on the solve's own stream when option "profile" is 1. */
double proxtv_last_kernel_ms(int which);
/* Fibres the speculative-chunk kernel could not prove and re-solved sequentially during the last solve on this
   thread's stream (0 for noisy data; large when lambda dwarfs the noise).  Diagnostic only: results are exact
   either way. */
long   proxtv_last_fixups(void);
/* Profiling aid (option "trace" = 1): per-workgroup record of the last speculative-chunk kernel launched by this thread,
   8 words each: [0] = XCC_ID << 32 | HW_ID (where it ran), [1..5] = 100 MHz timestamps at start, window staged, walk
   done, rebuild done, end.  Returns the number of workgroups copied to `dst` (at most max_wgs). */
long   proxtv_debug_trace(unsigned long long *dst, long max_wgs);
/* Tuning aid (option "why" = 1): what left work to the repair kernel since the last call, 8 counters: [0] walks that ran off
   their window, [1] links inside a workgroup / wave that stayed unproven, [2] links across workgroups / segments whose codes
   differ, [3] ... that were not published in time, [4] second chances taken across workgroups.  Returns 8, or <= 0. */
int    proxtv_debug_why(unsigned *dst);
/* What ran (process-wide, cumulative since load; tests and tools take differences): "sweep_launches" (fibre-sweep kernels),
   "repair_launches" (sweep_repair_kernel behind them), "repair_jobs_launches" (option repair_jobs), "pin_sweeps" (sweeps the
   pinning solver took), "pin_cap_next_rung" (sweeps its grid-wide variant handed on after the level cap), "tv2_long_fibres"
   (TV-L2 fibres solved parallel inside the fibre), "optimistic_solves" / "optimistic_redone" (option optimistic), "certify_sweeps" / "certify_failures" / "certify_skipped" (option certify:
   sweeps checked, fibres that failed and were re-solved, sweeps that could not be checked), "tvp_fibres" / "tvp_capped" (general-p fibres
   solved iteratively, and those an iteration cap stopped).  -1 for an unknown name. */
long   proxtv_debug_counter(const char *name);
/* Geometry policy the adaptive chunk kernel currently uses on this thread (the highest over the sweep families):
   0 = 16-sample warm-up zones (noisy data, small lambda), 1 = the same, robust instantiation (walks may run past
   the window, second-chance rounds inside a block: pieces of ~5 samples), 2 = 64-sample zones (pieces of ~10 samples),
   3 = the pinning solver (exact and data-parallel inside the fibre, any piece length; where it does not apply --
   lambda <= 0, fibres beyond what the device holds -- chunks walked from global memory with 256-sample zones),
   4 = chunks walked from global memory with 1024-sample zones, 5 = one sequential walk per fibre. */
int    proxtv_chunk_mode(void);
/* dst = src with the 8-bytes-per-lane access width of the sweep kernels: a known byte count against which the
   rocprofv3 FETCH_SIZE / WRITE_SIZE counters are calibrated (tools/pmc_traffic.py).  Device pointers. */
int    proxtv_calib_copy_dev(const double *src, double *dst, long n, void *stream);
long   proxtv_last_kernel_launches(int which);

#ifdef __cplusplus
}
#endif
#endif /* PROXTV_AMD_H */
