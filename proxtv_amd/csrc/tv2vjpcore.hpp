// tv2vjpcore.hpp -- the derivative of the 1-D TV-L2 prox, one fibre at a time.  Plain C++ on registers and small
// arrays: tv2_vjp.hip runs it one lane per fibre, tests/tv2_vjp_host.cpp runs the same functions with g++.
//
// y = prox(x) = x - D'u along one fibre of n samples, D the (n-1) x n difference matrix, T = D D' = tridiag(-1, 2, -1).  The forward
// (tv2.hip) hands out the fibre's multiplier mu: mu = 0 when u = T^-1 D x lies inside the ball ||u|| <= lambda (y is the mean of x),
// else (T + mu I) u = D x with ||u|| = lambda, and then D y = mu u.  With M = T + mu I, a cotangent g and h = D g:
//     active (mu > 0)   p = M^-1 h ,  q = M^-1 (D y) ,  kappa = (h'q) / ((D y)'q)
//                       gx = g - D'(p - kappa q) ,   glam = -mu lambda kappa
//     inside (mu = 0)   gx = mean(g) on every sample ,  glam = 0
//     n == 1 or lambda <= 0:  gx = g ,  glam = 0
// The Jacobian is symmetric: the same product is the VJP and the JVP in x.  At the kink ||T^-1 D x|| = lambda the prox is not
// differentiable; mu says which branch the forward took and that branch's derivative is what comes out.
//
// Two passes over the fibre.  M = L diag(d) L' with d_0 = a, d_i = a - 1 / d_{i-1}, a = 2 + mu.
//   eliminate   forward on BOTH right-hand sides, zh_i = h_i + zh_{i-1} / d_{i-1} and zq likewise from D y; both dot products of kappa
//               fall out of it: h'M^-1(Dy) = sum zh_i zq_i / d_i, (Dy)'M^-1(Dy) = sum zq_i^2 / d_i.  It also sums g (the inside case).
//   substitute  backward on the ONE vector zh - kappa zq: w_i = (zh_i - kappa zq_i + w_{i+1}) / d_i, writing gx_{i+1} = g_{i+1} - w_i +
//               w_{i+1} as it goes (so gx may be g: a sample is read before it is written, by the same lane).
// What is kept between the passes: zh, zq and r_i = 1 / d_i.  The pivots decrease to a fixed point; once r_i == r_{i-1} bit for bit every
// later one is the same number, so from that edge (kfix) on nothing is stored or loaded.  Samples are handled kBlock at a time so that
// the loads of a block do not sit on the recurrence.  Nothing depends on timing: the same call gives the same bits.
#pragma once

#ifdef PTV_HOST_TEST
#include <cmath>
#define PTV_TV2VJP_HD inline
#else
#define PTV_TV2VJP_HD __host__ __device__ __forceinline__
#endif

namespace ptv {
namespace tv2vjp {

constexpr int kBlock = 8;   // edges handled per step of a pass (tv2.hip's kBlock)

struct Forward {
    double hq = 0.0, qq = 0.0;   // h' M^-1 (D y) ; (D y)' M^-1 (D y)
    double gsum = 0.0;           // sum of g, left to right
    double rfix = 0.0;           // 1 / d at its fixed point
    int kfix = 0;                // edges kfix .. n-2 have r == rfix and are not stored (n - 1: every r is stored)
};

// Y(i), G(i): samples i = 0 .. n-1 (n >= 2).  R, H, Q: scratch with put(i, v) / get(i) for the edges i = 0 .. n-2.
template <class Y, class G, class R, class H, class Q>
PTV_TV2VJP_HD Forward eliminate(int n, double a, Y y, G g, R r, H zh, Q zq) {
    const int nn = n - 1;
    Forward f;
    f.kfix = nn;
    double yprev = y(0), gprev = g(0);
    f.gsum = gprev;
    double rprev = 0.0, hprev = 0.0, qprev = 0.0;   // 1 / d_{i-1}, zh_{i-1}, zq_{i-1}: nothing precedes edge 0
    for (int i0 = 0; i0 < nn; i0 += kBlock) {
        double yv[kBlock], gv[kBlock];
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const bool on = i0 + k < nn;
            yv[k] = on ? y(i0 + k + 1) : 0.0;
            gv[k] = on ? g(i0 + k + 1) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i0 + k;
            if (i < nn) {
                const double ri = 1.0 / (a - rprev);
                const double hi = (gv[k] - gprev) + hprev * rprev;
                const double qi = (yv[k] - yprev) + qprev * rprev;
                f.hq += (hi * qi) * ri;
                f.qq += (qi * qi) * ri;
                f.gsum += gv[k];
                if (f.kfix == nn && ri == rprev) {
                    f.kfix = i;
                    f.rfix = ri;
                }
                if (i < f.kfix) r.put(i, ri);
                zh.put(i, hi);
                zq.put(i, qi);
                rprev = ri;
                hprev = hi;
                qprev = qi;
                yprev = yv[k];
                gprev = gv[k];
            }
        }
    }
    return f;
}

// `active`: gx = g - D'w with w the backward substitution of zh - kappa zq ; else every sample receives `mean`.  The lanes of a wave
// run the same loop either way (an inside lane's w is computed and dropped).  PUT(i, v) receives gx of sample i, last sample first.
template <class G, class R, class H, class Q, class PUT>
PTV_TV2VJP_HD void substitute(int n, bool active, double kappa, double mean, const Forward &f, G g, R r, H zh, Q zq, PUT put) {
    const int nn = n - 1;
    double wnext = 0.0;   // w_{i+1} ; w_{n-1} = 0
    for (int i1 = nn - 1; i1 >= 0; i1 -= kBlock) {
        double rv[kBlock], hv[kBlock], qv[kBlock], gv[kBlock];
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i1 - k;
            const bool on = i >= 0;
            rv[k] = (on && i < f.kfix) ? r.get(i) : f.rfix;
            hv[k] = on ? zh.get(i) : 0.0;
            qv[k] = on ? zq.get(i) : 0.0;
            gv[k] = on ? g(i + 1) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i1 - k;
            if (i >= 0) {
                const double w = ((hv[k] - kappa * qv[k]) + wnext) * rv[k];
                put(i + 1, active ? (gv[k] - w) + wnext : mean);
                wnext = w;
            }
        }
    }
    put(0, active ? g(0) + wnext : mean);   // (w_{-1} = 0)
}

// One fibre: gx through PUT, returns glam.  mu is the forward's multiplier of this fibre.
template <class Y, class G, class R, class H, class Q, class PUT>
PTV_TV2VJP_HD double fibre(int n, double mu, double lam, Y y, G g, R r, H zh, Q zq, PUT put) {
    if (n <= 1 || !(lam > 0.0)) {   // the prox is the identity
        for (int i = 0; i < n; i++) put(i, g(i));
        return 0.0;
    }
    const bool active = mu > 0.0;
    const Forward f = eliminate(n, 2.0 + (active ? mu : 0.0), y, g, r, zh, zq);
    const double kappa = active ? f.hq / f.qq : 0.0;
    substitute(n, active, kappa, f.gsum / (double)n, f, g, r, zh, zq, put);
    return active ? -(mu * lam) * kappa : 0.0;
}

}  // namespace tv2vjp
}  // namespace ptv
