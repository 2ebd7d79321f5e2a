// tvpvjpcore.hpp -- the derivative of the TV-Lp fibre prox for general p, one fibre per caller (a GPU lane in tvp_vjp.hip, a host thread
// in the tests' harness).
//
//     x = prox(y) = argmin 1/2 ||x - y||^2 + lambda ||Dx||_p ,   1 < p < inf, p != 2,   q = p / (p - 1)
//
// Needs only the prox's OUTPUT x (the array called y below, as the forward's result), lambda and p: no multiplier, no tape.  Per fibre of n
// samples, D the (n-1) x n difference matrix, T = D D', w = D x, N = ||w||_p, s_i = |w_i| / N in [0, 1], phi_i = sign(w_i) s_i^(p-1)
// (the gradient of ||.||_p at w; the dual is lambda phi).  The optimality condition x + lambda D' phi(Dx) = y differentiates to
//     J = (I + lambda D' H D)^-1 ,   H = (p-1)/N (diag s^(p-2) - phi phi')      (H w = 0)
// which is symmetric: the same product is the VJP and the JVP.  It is applied in the arm in which its powers have exponents >= 0 -- the
// forward's own choice of variables, so nothing is singular at w_i = 0 and, every power being one of s <= 1, nothing overflows:
//   p > 2, primal   K = I + D' diag(c s^(p-2)) D (n x n), c = lambda (p-1) / N, b = D' phi ;  a = K^-1 g, e = K^-1 b,
//                   kappa = c (b'a) / (1 - c b'e)   (Sherman-Morrison; the denominator is positive: J is positive definite)
//                   gx = a + kappa e = K^-1 (g + kappa b) ,   glam = -gx'b = -(b'a + kappa b'e)
//   p < 2, dual     K = T + diag((q-1) N / lambda s^(2-p)) ((n-1) x (n-1)), h = D g, t = w / N = sign(w) s ;  a = K^-1 h, e = K^-1 t,
//                   kappa = (t'a) / (t'e) ,  v = a - kappa e = K^-1 (h - kappa t) ,  gx = g - D'v ,  glam = -gx'D'phi = -kappa
//                   (the Woodbury form of the same J; the last equality because t'v = 0 and H w = 0)
//   closed forms    n == 1 or lambda <= 0: gx = g ; x constant along the fibre (N == 0 exactly -- the forward stores the mean itself on
//                   that branch and on its capped fall-back): gx = mean(g) ; glam = 0 in all of them.
// The branch the forward took is what is differentiated, as with TV-L2 (tv2vjpcore.hpp).
//
// Four passes over the fibre: the largest |w_i| (and the sum of g); N, summed in powers of |w_i| / max |w|; the LDL' elimination of the
// tridiagonal K on BOTH right-hand sides, whose intermediates give both scalar products of kappa (r1'K^-1 r2 = sum z1_i z2_i / d_i); the
// backward substitution on the ONE combined right-hand side, which writes gx as it goes.  Kept between the last two: l_i = off_i / d_i
// and the two z_i / d_i -- three arrays laid out like the data.  Samples are handled kBlock at a time so that the loads and the pow calls
// of a block do not sit on the recurrence.  gx may be g: the elimination has read all of g before the substitution writes, and the dual's
// substitution reads sample i of g just before it writes it.  Nothing depends on timing: the same call gives the same bits.
//
// solve() takes the load of the cotangent and the store of the result as functors (the contract of tv2vjp::fibre): `cot(i)`
// is called wherever passes 1, 3 and (dual arm) 4 read g_i and must hand out the same bits every time; `put(i, a_i)` receives a = J g
// in the order pass 4 produces it -- last sample first, sample 0 last -- each sample once, and after the last cot(i) of that sample, so
// that it may rewrite the cotangent's own array.  With the defaults (F.g, F.gx) the arithmetic is what it was without them.
#pragma once

#include <cmath>

#ifndef PTV_HD
#if defined(__HIPCC__)
#define PTV_HD __host__ __device__ __forceinline__
#else
#define PTV_HD inline
#endif
#endif

namespace ptv {
namespace tvpvjp {

constexpr int kBlock = 8;   // samples handled per step of a pass (tvpcore.hpp's kBlock)

struct Fibre {
    const double *y;        // the forward's output
    const double *g;        // the cotangent
    double *gx;             // the result (may be g)
    double *ll, *z1, *z2;   // scratch laid out like the data: off_i / d_i and the two z_i / d_i of the elimination
    long base, inc;
    int n;
    double lam, p;
    PTV_HD double ld(const double *a, int i) const { return a[base + (long)i * inc]; }
    PTV_HD void st(double *a, int i, double val) const { a[base + (long)i * inc] = val; }
};

// p > 2: eliminates K = I + D' diag(c s^(p-2)) D on the right-hand sides g and b = D' phi; ba = b'K^-1 g, be = b'K^-1 b
template <class Cot>
PTV_HD void eliminate_primal(const Fibre &F, const Cot &cot, double N, double c, double &ba, double &be) {
    const int n = F.n, nn = n - 1;
    const double pm2 = F.p - 2.0;
    double sa = 0.0, se = 0.0;
    double llprev = 0.0, offprev = 0.0, z1prev = 0.0, z2prev = 0.0;
    for (int i0 = 0; i0 < n; i0 += kBlock) {
        double yy[kBlock + 2], gg[kBlock];   // yy[k]: sample i0 - 1 + k ; gg[k]: cotangent i0 + k
#pragma unroll
        for (int k = 0; k < kBlock + 2; k++) {
            const int i = i0 - 1 + k;
            yy[k] = (i >= 0 && i < n) ? F.ld(F.y, i) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) gg[k] = (i0 + k < n) ? cot(i0 + k) : 0.0;
        double al[kBlock + 1], ph[kBlock + 1];   // edge i0 - 1 + k, between yy[k] and yy[k + 1]: c s^(p-2) and phi
#pragma unroll
        for (int k = 0; k <= kBlock; k++) {
            const int j = i0 - 1 + k;
            al[k] = 0.0; ph[k] = 0.0;
            if (j >= 0 && j < nn) {
                const double w = yy[k + 1] - yy[k], s = fabs(w) / N, pw = pow(s, pm2);
                al[k] = c * pw;
                ph[k] = copysign(s * pw, w);
            }
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i0 + k;
            if (i < n) {
                const double diag = 1.0 + al[k] + al[k + 1], off = -al[k + 1], b = ph[k] - ph[k + 1];
                const double d = diag - offprev * llprev;
                const double z1 = gg[k] - llprev * z1prev, z2 = b - llprev * z2prev;
                const double ll = off / d, zz1 = z1 / d, zz2 = z2 / d;
                F.st(F.ll, i, ll);
                F.st(F.z1, i, zz1);
                F.st(F.z2, i, zz2);
                sa += z1 * zz2;
                se += z2 * zz2;
                llprev = ll;
                offprev = off;
                z1prev = z1;
                z2prev = z2;
            }
        }
    }
    ba = sa;
    be = se;
}

// p > 2: gx = K^-1 (g + kappa b), last sample first
template <class Put>
PTV_HD void substitute_primal(const Fibre &F, const Put &put, double kappa) {
    double next = 0.0;
    for (int i1 = F.n - 1; i1 >= 0; i1 -= kBlock) {
        double ll[kBlock], zz[kBlock];
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i1 - k;
            ll[k] = (i >= 0) ? F.ld(F.ll, i) : 0.0;
            zz[k] = (i >= 0) ? F.ld(F.z1, i) + kappa * F.ld(F.z2, i) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i1 - k;
            if (i >= 0) {
                const double v = zz[k] - ll[k] * next;
                put(i, v);
                next = v;
            }
        }
    }
}

// p < 2: eliminates K = T + diag(cd s^(2-p)) on the right-hand sides h = D g and t = w / N; ta = t'K^-1 h, te = t'K^-1 t
template <class Cot>
PTV_HD void eliminate_dual(const Fibre &F, const Cot &cot, double N, double cd, double &ta, double &te) {
    const int n = F.n, nn = n - 1;
    const double tmp = 2.0 - F.p;
    double sa = 0.0, se = 0.0;
    double llprev = 0.0, offprev = 0.0, z1prev = 0.0, z2prev = 0.0;
    for (int i0 = 0; i0 < nn; i0 += kBlock) {
        double yy[kBlock + 1], gg[kBlock + 1];   // samples i0 + k
#pragma unroll
        for (int k = 0; k <= kBlock; k++) {
            const bool on = i0 + k < n;
            yy[k] = on ? F.ld(F.y, i0 + k) : 0.0;
            gg[k] = on ? cot(i0 + k) : 0.0;
        }
        double dg[kBlock], tt[kBlock];   // edge i0 + k: the diagonal of K and t
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            dg[k] = 1.0; tt[k] = 0.0;
            if (i0 + k < nn) {
                const double t = (yy[k + 1] - yy[k]) / N;
                dg[k] = 2.0 + cd * pow(fabs(t), tmp);
                tt[k] = t;
            }
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i0 + k;
            if (i < nn) {
                const double off = (i < nn - 1) ? -1.0 : 0.0;
                const double d = dg[k] - offprev * llprev;
                const double z1 = (gg[k + 1] - gg[k]) - llprev * z1prev, z2 = tt[k] - llprev * z2prev;
                const double ll = off / d, zz1 = z1 / d, zz2 = z2 / d;
                F.st(F.ll, i, ll);
                F.st(F.z1, i, zz1);
                F.st(F.z2, i, zz2);
                sa += z1 * zz2;
                se += z2 * zz2;
                llprev = ll;
                offprev = off;
                z1prev = z1;
                z2prev = z2;
            }
        }
    }
    ta = sa;
    te = se;
}

// p < 2: v = K^-1 (h - kappa t), last edge first; gx_{i+1} = g_{i+1} - v_i + v_{i+1} as it goes, gx_0 = g_0 + v_0
template <class Cot, class Put>
PTV_HD void substitute_dual(const Fibre &F, const Cot &cot, const Put &put, double kappa) {
    const int nn = F.n - 1;
    double next = 0.0;   // v_{i+1} ; v_{n-1} = 0
    for (int i1 = nn - 1; i1 >= 0; i1 -= kBlock) {
        double ll[kBlock], zz[kBlock], gg[kBlock];
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i1 - k;
            ll[k] = (i >= 0) ? F.ld(F.ll, i) : 0.0;
            zz[k] = (i >= 0) ? F.ld(F.z1, i) - kappa * F.ld(F.z2, i) : 0.0;
            gg[k] = (i >= 0) ? cot(i + 1) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i1 - k;
            if (i >= 0) {
                const double v = zz[k] - ll[k] * next;
                put(i + 1, (gg[k] - v) + next);
                next = v;
            }
        }
    }
    put(0, cot(0) + next);
}

// One fibre: hands a = J g to `put`, returns glam.
template <class Cot, class Put>
PTV_HD double solve(const Fibre &F, const Cot &cot, const Put &put) {
    const int n = F.n, nn = n - 1;
    if (nn <= 0 || !(F.lam > 0.0)) {   // the prox is the identity
        for (int i = n - 1; i >= 0; i--) put(i, cot(i));
        return 0.0;
    }
    // pass 1: the largest jump of the output, the sum of the cotangent
    double wmax = 0.0, gsum = 0.0;
    for (int i0 = 0; i0 < n; i0 += kBlock) {
        double yy[kBlock + 1], gg[kBlock];
#pragma unroll
        for (int k = 0; k <= kBlock; k++) yy[k] = (i0 + k < n) ? F.ld(F.y, i0 + k) : 0.0;
#pragma unroll
        for (int k = 0; k < kBlock; k++) gg[k] = (i0 + k < n) ? cot(i0 + k) : 0.0;
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            if (i0 + k < n) gsum += gg[k];
            if (i0 + k < nn) {
                const double d = fabs(yy[k + 1] - yy[k]);
                if (d > wmax) wmax = d;
            }
        }
    }
    if (!(wmax > 0.0)) {   // the forward answered with the mean
        const double mean = gsum / (double)n;
        for (int i = n - 1; i >= 0; i--) put(i, mean);
        return 0.0;
    }
    // pass 2: N = ||w||_p in powers of |w_i| / max |w| (no power overflows)
    double S = 0.0;
    for (int i0 = 0; i0 < nn; i0 += kBlock) {
        double yy[kBlock + 1];
#pragma unroll
        for (int k = 0; k <= kBlock; k++) yy[k] = (i0 + k < n) ? F.ld(F.y, i0 + k) : 0.0;
#pragma unroll
        for (int k = 0; k < kBlock; k++)
            if (i0 + k < nn) S += pow(fabs(yy[k + 1] - yy[k]) / wmax, F.p);
    }
    const double N = wmax * pow(S, 1.0 / F.p);
    // passes 3 and 4
    if (F.p > 2.0) {
        const double c = F.lam * (F.p - 1.0) / N;
        double ba, be;
        eliminate_primal(F, cot, N, c, ba, be);
        const double kappa = c * ba / (1.0 - c * be);
        substitute_primal(F, put, kappa);
        return -(ba + kappa * be);
    }
    const double cd = N / (F.lam * (F.p - 1.0));   // (q - 1) N / lambda
    double ta, te;
    eliminate_dual(F, cot, N, cd, ta, te);
    const double kappa = ta / te;
    substitute_dual(F, cot, put, kappa);
    return -kappa;
}

// the plain call: the cotangent is F.g, the result goes to F.gx
PTV_HD double solve(const Fibre &F) {
    return solve(F, [&F](int i) { return F.ld(F.g, i); }, [&F](int i, double v) { F.st(F.gx, i, v); });
}

}  // namespace tvpvjp
}  // namespace ptv
