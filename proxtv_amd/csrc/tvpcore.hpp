// tvpcore.hpp -- the TV-Lp fibre prox for general p, one fibre per caller (a GPU lane in tvp.hip, a host thread in the tests' harness).
//
//     prox(y) = argmin_x 1/2 ||x - y||^2 + lambda ||Dx||_p ,   1 < p < inf, p != 2,   q = p / (p - 1)
//
// Dual: min_u 1/2 ||D'u - y||^2 over the ball ||u||_q <= lambda, x = y - D'u; gap(u) = lambda ||Dx||_p - u'Dx for a feasible u.
// Everything below works on y / lambda (the ball has radius 1: no power of a dual value overflows) and scales back on output.
//
// Closed forms: n == 1 or lambda <= 0 -- copy; u0 = T^-1 D y (the running sums of mean - y) inside the ball -- the mean.
// Otherwise the KKT system (T u - D y + mu phi(u) = 0, phi(u) = |u|^(q-1) sign u, ||u||_q = 1) is solved in two nested loops:
//   inner  for a fixed multiplier mu, a smooth strictly convex problem with a tridiagonal Hessian, by Newton's method with a
//          backtracking line search, in the variables in which its power has an exponent above 1 -- so that nothing is singular
//          at zero and nothing needs regularising:
//            p < 2 (q > 2), the dual:    min_u 1/2 u'T u - (Dy)'u + mu/q sum |u_i|^q            Hessian T + mu (q-1) diag |u|^(q-2)
//            p > 2,         the primal:  min_x 1/2 ||x - y||^2 + mu/p sum (|Dx_i| / mu)^p       Hessian I + D' diag((p-1)/mu (|Dx|/mu)^(p-2)) D
//          (the second is the first's dual: u_i = (|Dx_i| / mu)^(p-1) sign Dx_i).  One Newton step is one LDL' sweep (forward
//          elimination, which also assembles gradient and Hessian and sums the objective, the Newton decrement and ||u||_q^q; backward
//          substitution, which also commits the previous step).
//   outer  mu is the root of h(log mu) = log ||u(mu)||_q, decreasing: from mu0 = ||Dy||_p (an upper bound: there ||u|| <= 1) by the
//          fixed point log mu += (q - 1) h (exact where lambda is small), then by the secant rule, kept inside the bracket.
// After every outer iteration the iterate is scaled into the ball and its duality gap evaluated; the output array always holds the
// best feasible iterate so far.  The loops stop at gap <= max(kStop, 4e-13 * 1/2 ||y - mean||^2); kStop is a thousand times
// tighter than the reference's 1e-5.  The work is bounded by kMaxSweeps forward sweeps per fibre: a fibre that gets there keeps its
// best iterate and is reported as capped.
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
namespace tvp {

constexpr int kBlock = 8;          // samples handled per step of a sweep: their loads and powers are independent of the recurrence
constexpr int kMaxOuter = 60;      // multipliers tried
constexpr int kMaxInner = 80;      // Newton steps per multiplier
constexpr int kMaxSweeps = 1500;   // forward sweeps per fibre, in all (a sweep is one pass over the fibre's five arrays)
constexpr double kStop = 1e-8;     // target duality gap, absolute
constexpr double kStopRel = 4e-13; // ... or this fraction of 1/2 ||y - mean||^2, the rounding floor of the gap's own sums

struct Fibre {
    const double *y;            // input
    double *x;                  // output
    double *v, *dl, *ll, *zz;   // scratch laid out like the data: iterate, Newton direction, off_i / d_i, z_i / d_i
    long base, inc;
    int n;
    double lam, p;
};

struct Result {
    double gap;     // the achieved duality gap (0 for the closed forms)
    int outer;      // outer iterations (0 for the closed forms)
    int sweeps;     // forward sweeps
    int capped;     // 1: stopped by a cap above the target gap
};

PTV_HD bool finite_(double a) { return a - a == 0.0; }

struct Work {
    Fibre F;
    double il;         // 1 / lambda
    double q, r;       // r = max(p, q) - 1 > 1: the exponent of the inner problem's gradient
    double yscale;     // max |D y| / lambda
    double escale;     // 1/2 ||y - mean||^2 / lambda^2: the scale of the inner objectives
    PTV_HD double ld(const double *a, int i) const { return a[F.base + (long)i * F.inc]; }
    PTV_HD void st(double *a, int i, double val) const { a[F.base + (long)i * F.inc] = val; }
};

// One forward sweep at the point v + t dl for the multiplier mu: assembles gradient g and Hessian H row by row, eliminates
// (H = L D L', z = L^-1 (-g)) and leaves ll_i = off_i / d_i and zz_i = z_i / d_i for the backward sweep.
// f: the objective there; dec: g' H^-1 g (the Newton decrement squared); S: sum |u_i|^q of the dual point.
template <bool PRIMAL>
PTV_HD void forward(const Work &W, double mu, double t, double &f, double &dec, double &S) {
    const int n = W.F.n, nn = n - 1, m = PRIMAL ? n : nn;
    const double r = W.r, rm1 = r - 1.0, cf = mu / (r + 1.0);
    double fa = 0.0, da = 0.0, Sa = 0.0;
    double llprev = 0.0, offprev = 0.0, zprev = 0.0;
    for (int i0 = 0; i0 < m; i0 += kBlock) {
        double v[kBlock + 2], yy[kBlock + 1];   // v[k]: the iterate at i0 - 1 + k ; yy[k]: y / lambda at i0 + k
#pragma unroll
        for (int k = 0; k < kBlock + 2; k++) {
            const int i = i0 - 1 + k;
            v[k] = (i >= 0 && i < m) ? W.ld(W.F.v, i) + t * W.ld(W.F.dl, i) : 0.0;
        }
#pragma unroll
        for (int k = 0; k <= kBlock; k++) yy[k] = (i0 + k < n) ? W.ld(W.F.y, i0 + k) * W.il : 0.0;
        double diag[kBlock], off[kBlock], g[kBlock];
        if (!PRIMAL) {
#pragma unroll
            for (int k = 0; k < kBlock; k++) {
                const int i = i0 + k;
                diag[k] = 1.0; off[k] = 0.0; g[k] = 0.0;
                if (i < m) {
                    const double v0 = v[k + 1], a = fabs(v0), pw = pow(a, rm1), b = yy[k + 1] - yy[k];
                    diag[k] = 2.0 + mu * r * pw;
                    off[k] = (i < m - 1) ? -1.0 : 0.0;
                    g[k] = 2.0 * v0 - v[k] - v[k + 2] - b + copysign(mu * a * pw, v0);
                    fa += v0 * v0 - v0 * v[k + 2] - b * v0 + cf * (v0 * v0 * pw);
                    Sa += v0 * v0 * pw;
                }
            }
        } else {
            double s[kBlock + 1], gt[kBlock + 1];   // edge i0 - 1 + k, between v[k] and v[k + 1]
#pragma unroll
            for (int k = 0; k <= kBlock; k++) {
                const int j = i0 - 1 + k;
                s[k] = 0.0; gt[k] = 0.0;
                if (j >= 0 && j < nn) {
                    const double w = v[k + 1] - v[k], rho = fabs(w) / mu, pw = pow(rho, rm1);
                    s[k] = (r / mu) * pw;
                    gt[k] = copysign(rho * pw, w);
                    if (k >= 1) {   // (an edge is summed by the block of its left sample)
                        fa += cf * (rho * rho * pw);
                        Sa += rho * rho * pw;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kBlock; k++) {
                const int i = i0 + k;
                diag[k] = 1.0; off[k] = 0.0; g[k] = 0.0;
                if (i < m) {
                    const double d0 = v[k + 1] - yy[k];
                    diag[k] = 1.0 + s[k] + s[k + 1];
                    off[k] = -s[k + 1];
                    g[k] = d0 + gt[k] - gt[k + 1];
                    fa += 0.5 * d0 * d0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i0 + k;
            if (i < m) {
                const double d = diag[k] - offprev * llprev, z = -g[k] - llprev * zprev;
                const double ll = off[k] / d, zz = z / d;
                W.st(W.F.ll, i, ll);
                W.st(W.F.zz, i, zz);
                da += z * zz;
                llprev = ll;
                offprev = off[k];
                zprev = z;
            }
        }
    }
    f = fa;
    dec = da;
    S = Sa;
}

// Backward substitution: dl <- the Newton direction of the last forward sweep; v <- v + t dl with the direction it replaces.
PTV_HD void backward(const Work &W, int m, double t) {
    double dnext = 0.0;
    for (int i1 = m - 1; i1 >= 0; i1 -= kBlock) {
        double ll[kBlock], zz[kBlock], vv[kBlock], dd[kBlock];
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i1 - k;
            ll[k] = (i >= 0) ? W.ld(W.F.ll, i) : 0.0;
            zz[k] = (i >= 0) ? W.ld(W.F.zz, i) : 0.0;
            vv[k] = (i >= 0) ? W.ld(W.F.v, i) : 0.0;
            dd[k] = (i >= 0) ? W.ld(W.F.dl, i) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i1 - k;
            if (i >= 0) {
                const double dn = zz[k] - ll[k] * dnext;
                W.st(W.F.v, i, vv[k] + t * dd[k]);
                W.st(W.F.dl, i, dn);
                dnext = dn;
            }
        }
    }
}

// Newton's method at a fixed mu from the point v + tp dl; on return the point is v + tp dl again (tp updated) and S belongs to it.
// false: no finite point (nothing usable).
template <bool PRIMAL>
PTV_HD bool inner(const Work &W, double mu, double &tp, double tol, int &sweeps, double &S) {
    const int m = PRIMAL ? W.F.n : W.F.n - 1;
    double f, dec;
    forward<PRIMAL>(W, mu, tp, f, dec, S);
    sweeps++;
    if (!finite_(f) || !finite_(dec)) return false;
    for (int it = 0; it < kMaxInner && sweeps < kMaxSweeps; it++) {
        if (dec <= 1e-22 * (fabs(f) + tol)) break;   // (the decrement is the SQUARE of the step's length in the Hessian's norm)
        backward(W, m, tp);
        tp = 0.0;
        double t = 1.0;
        bool took = false;
        while (t >= 1e-9 && sweeps < kMaxSweeps) {
            double f1, dec1, S1;
            forward<PRIMAL>(W, mu, t, f1, dec1, S1);
            sweeps++;
            if (finite_(f1) && finite_(dec1) && f1 <= f - 1e-4 * t * dec + 1e-13 * (fabs(f) + fabs(f1))) {
                tp = t;
                f = f1;
                dec = dec1;
                S = S1;
                took = true;
                break;
            }
            t *= (t > 0.2) ? 0.5 : 0.25;
        }
        if (!took) {   // no descent within rounding: the committed point stands (S: recomputed below by the caller's next sweep)
            forward<PRIMAL>(W, mu, 0.0, f, dec, S);
            sweeps++;
            break;
        }
    }
    return true;
}

// The dual point of v + tp dl, scaled by sc into the ball, as x = y - D'u: returns its gap lambda ||Dx||_p - u'Dx; WRITE: stores x.
template <bool PRIMAL, bool WRITE>
PTV_HD double primal_out(const Work &W, double mu, double tp, double sc) {
    const int n = W.F.n, nn = n - 1, m = PRIMAL ? n : nn;
    const double lam = W.F.lam, rm1 = W.r - 1.0, us = lam * sc, wn = 1.0 / (lam * W.yscale);
    double sp = 0.0, dot = 0.0;
    for (int i0 = 0; i0 < n; i0 += kBlock) {
        double u[kBlock + 2], yy[kBlock + 1];   // u[k]: the dual at edge i0 - 1 + k (0 outside) ; yy[k]: y at i0 + k
        if (!PRIMAL) {
#pragma unroll
            for (int k = 0; k < kBlock + 2; k++) {
                const int j = i0 - 1 + k;
                u[k] = (j >= 0 && j < nn) ? us * (W.ld(W.F.v, j) + tp * W.ld(W.F.dl, j)) : 0.0;
            }
        } else {
            double v[kBlock + 3];   // the iterate at i0 - 1 + k
#pragma unroll
            for (int k = 0; k < kBlock + 3; k++) {
                const int i = i0 - 1 + k;
                v[k] = (i >= 0 && i < m) ? W.ld(W.F.v, i) + tp * W.ld(W.F.dl, i) : 0.0;
            }
#pragma unroll
            for (int k = 0; k < kBlock + 2; k++) {
                const int j = i0 - 1 + k;
                u[k] = 0.0;
                if (j >= 0 && j < nn) {
                    const double w = v[k + 1] - v[k], rho = fabs(w) / mu;
                    u[k] = us * copysign(rho * pow(rho, rm1), w);
                }
            }
        }
#pragma unroll
        for (int k = 0; k <= kBlock; k++) yy[k] = (i0 + k < n) ? W.ld(W.F.y, i0 + k) : 0.0;
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i0 + k;
            if (i < n) {
                const double xi = yy[k] - u[k] + u[k + 1];
                if (WRITE) W.st(W.F.x, i, xi);
                if (i < nn) {
                    const double xn = yy[k + 1] - u[k + 1] + u[k + 2], dx = xn - xi;
                    sp += pow(fabs(dx) * wn, W.F.p);
                    dot += u[k + 1] * dx;
                }
            }
        }
    }
    return lam * (lam * W.yscale) * pow(sp, 1.0 / W.F.p) - dot;
}

template <bool PRIMAL>
PTV_HD void iterate(const Work &W, double mu0, double tp, double tol, Result &res) {
    const double q = W.q;
    double lmu = log(mu0), lo = -INFINITY, hi = INFINITY, lprev = 0.0, hprev = 0.0, best = INFINITY;
    bool have_prev = false;
    int sweeps = 0, outer = 0;
    while (outer < kMaxOuter && sweeps < kMaxSweeps) {
        const double mu = exp(lmu);
        double S;
        if (!inner<PRIMAL>(W, mu, tp, W.escale, sweeps, S)) break;
        outer++;
        double h = log(S) / q;   // log ||u||_q
        if (!(h > -40.0)) h = -40.0;
        if (!(h < 40.0)) h = 40.0;
        const double sc = h > 0.0 ? exp(-h) : 1.0;
        const double gap = primal_out<PRIMAL, false>(W, mu, tp, sc);
        if (gap < best) {
            primal_out<PRIMAL, true>(W, mu, tp, sc);
            best = gap;
        }
        if (best <= tol) break;
        if (h > 0.0) { if (lmu > lo) lo = lmu; } else { if (lmu < hi) hi = lmu; }
        const double fp = lmu + (q - 1.0) * h;
        double cand = have_prev && h != hprev ? lmu - h * (lmu - lprev) / (h - hprev) : fp;
        if (!finite_(cand) || !(cand > lo && cand < hi)) cand = (lo > -INFINITY && hi < INFINITY) ? 0.5 * (lo + hi) : fp;
        if (cand > lmu + 20.0) cand = lmu + 20.0;
        if (cand < lmu - 20.0) cand = lmu - 20.0;
        if (cand == lmu) break;   // the multiplier is settled to the last bit
        lprev = lmu;
        hprev = h;
        have_prev = true;
        lmu = cand;
    }
    res.outer = outer;
    res.sweeps = sweeps;
    res.gap = best;
    res.capped = !(best <= tol);
}

// the whole prox of one fibre
PTV_HD Result solve(const Fibre &F) {
    Work W;
    W.F = F;
    const int n = F.n, nn = n - 1;
    Result res{0.0, 0, 0, 0};
    if (nn <= 0 || !(F.lam > 0.0)) {
        for (int i = 0; i < n; i++) W.st(F.x, i, W.ld(F.y, i));
        return res;
    }
    const bool primal = F.p > 2.0;
    W.il = 1.0 / F.lam;
    W.q = F.p / (F.p - 1.0);
    W.r = (primal ? F.p : W.q) - 1.0;
    // pass 1: the sum and the largest jump
    double sum = 0.0, jump = 0.0;
    for (int i0 = 0; i0 < n; i0 += kBlock) {
        double yy[kBlock + 1];
#pragma unroll
        for (int k = 0; k <= kBlock; k++) yy[k] = (i0 + k < n) ? W.ld(F.y, i0 + k) : 0.0;
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            if (i0 + k < n) sum += yy[k];
            if (i0 + k < nn) {
                const double d = fabs(yy[k + 1] - yy[k]);
                if (d > jump) jump = d;
            }
        }
    }
    const double mean = sum / (double)n, mean_s = mean * W.il;
    W.yscale = jump * W.il;
    // pass 2: u0 = T^-1 D y / lambda (running sums of mean - y), its place against the ball, ||Dy||_p, and the starting point
    double c = 0.0, E = 0.0, Sq = 0.0, Sp = 0.0, umax = 0.0;
    bool outside = false;
    const double ij = jump > 0.0 ? 1.0 / jump : 0.0;
    for (int i0 = 0; i0 < n; i0 += kBlock) {
        double yy[kBlock + 1];
#pragma unroll
        for (int k = 0; k <= kBlock; k++) yy[k] = (i0 + k < n) ? W.ld(F.y, i0 + k) : 0.0;
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int i = i0 + k;
            if (i < n) {
                const double e = yy[k] - mean;
                E += 0.5 * e * e;
                if (primal) {
                    W.st(F.v, i, yy[k] * W.il);
                    W.st(F.dl, i, 0.0);
                }
            }
            if (i < nn) {
                c += mean_s - yy[k] * W.il;
                const double a = fabs(c);
                if (a > umax) umax = a;
                if (a > 1.0) outside = true;
                else if (!outside) Sq += pow(a, W.q);
                Sp += pow(fabs(yy[k + 1] - yy[k]) * ij, F.p);
            }
        }
    }
    if (!outside && Sq <= 1.0) {   // the mean (also every constant fibre: u0 = 0)
        for (int i = 0; i < n; i++) W.st(F.x, i, mean);
        return res;
    }
    const double mu0 = W.yscale * pow(Sp, 1.0 / F.p);
    const double tol = kStop > kStopRel * E ? kStop : kStopRel * E;
    W.escale = E * W.il * W.il;
    if (primal) {   // the primal starts from y
        iterate<true>(W, mu0, 0.0, tol, res);
    } else {
        // pass 3: the dual's two starting points -- v: the solution without the coupling T, sign(b) (|b| / mu0)^(1/r) with b = Dy / lambda
        // (where lambda is small b dwarfs T u); v + dl: u0 scaled to a largest entry of 1 (where lambda is large) -- the lower objective wins
        const double us = umax > 1.0 ? 1.0 / umax : 1.0, ir = 1.0 / W.r;
        c = 0.0;
        for (int i0 = 0; i0 < nn; i0 += kBlock) {
            double yy[kBlock + 1];
#pragma unroll
            for (int k = 0; k <= kBlock; k++) yy[k] = (i0 + k < n) ? W.ld(F.y, i0 + k) * W.il : 0.0;
#pragma unroll
            for (int k = 0; k < kBlock; k++) {
                const int i = i0 + k;
                if (i < nn) {
                    c += mean_s - yy[k];
                    const double b = yy[k + 1] - yy[k], vd = copysign(pow(fabs(b) / mu0, ir), b);
                    W.st(F.v, i, vd);
                    W.st(F.dl, i, c * us - vd);
                }
            }
        }
        double f0, f1, dec, S;
        forward<false>(W, mu0, 0.0, f0, dec, S);
        forward<false>(W, mu0, 1.0, f1, dec, S);
        iterate<false>(W, mu0, (finite_(f1) && !(f0 <= f1)) ? 1.0 : 0.0, tol, res);
        res.sweeps += 2;
    }
    if (!(res.gap <= E)) {   // nothing better than the mean came out (no finite sweep at all, an exponent too stiff for the caps):
        for (int i = 0; i < n; i++) W.st(F.x, i, mean);   // the mean it is, with P(mean) - P* <= P(mean) = 1/2 ||y - mean||^2
        res.gap = E;
        res.capped = 1;
    }
    return res;
}

}  // namespace tvp
}  // namespace ptv
