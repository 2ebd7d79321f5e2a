// tvpg_modes_host.cpp -- TEST-ONLY, a stand-alone program: tvpvjp::solve (proxtv_amd/csrc/tvpvjpcore.hpp) with the load / store functors of
// every write-out MODE of the reverse recurrences against "the plain call, then the write-out in plain C++", bit for bit.
// Lengths around kBlock = 8, both arms (p = 1.5, 3), a constant fibre (the mean branch), strides 1 and 3, and every aliasing the
// solvers use: the result in the cotangent's own array, gU == g, zeta rewritten in place.  Never linked into libproxtv_amd.so; built
// and run by tests/test_tvpg_modes_host.py (g++ -ffp-contract=off, as the library is built).  Prints MODES_HOST_OK and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../proxtv_amd/csrc/tvpcore.hpp"
#include "../proxtv_amd/csrc/tvpvjpcore.hpp"

namespace {

enum { PLAIN = 0, DR_ROW = 1, DR_COL = 2, PD2 = 3, PD = 4 };

struct Rng {
    unsigned long long s;
    double next() {   // uniform in (-1, 1)
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return ((double)(s >> 11) / 9007199254740992.0) * 2.0 - 1.0;
    }
};

using Vec = std::vector<double>;

Vec spread(const Vec &a, int inc) {
    Vec s(a.size() * (size_t)inc + 1, -7.0);
    for (size_t i = 0; i < a.size(); i++) s[i * (size_t)inc] = a[i];
    return s;
}

bool same(const Vec &a, const Vec &b) { return a.size() == b.size() && !memcmp(a.data(), b.data(), a.size() * sizeof(double)); }

int failures = 0;
void expect(bool ok, const char *what, int mode, int n, double p, int inc, int variant) {
    if (ok) return;
    failures++;
    printf("MISMATCH %s: mode %d n %d p %g inc %d variant %d\n", what, mode, n, p, inc, variant);
}

// one case: x the prox's output, g / gu / cc / zeta the arrays of the mode (dense); variant: the mode's flags (final, with / without gU
// or zeta)
void run(int mode, int variant, const Vec &x, const Vec &g, const Vec &gu, const Vec &zeta, double lam, double p, int inc) {
    const int n = (int)x.size();
    const double scale = 1.0 / 3.0;
    const bool final = variant & 1, with = variant & 2;   // with: gU (PD2) / zeta (PD)
    const size_t len = (size_t)n * (size_t)inc + 1;
    // ---- the reference: the cotangent materialised, the plain call into `a`, the write-out in plain C++
    Vec cot(g);
    if (mode == PD)
        for (int i = 0; i < n; i++) cot[i] = std::fma(g[i], scale, -(with ? zeta[i] : 0.0));
    Vec xs = spread(x, inc), cs = spread(cot, inc), as(len, -7.0), ll(len, -7.0), z1(len, -7.0), z2(len, -7.0);
    const ptv::tvpvjp::Fibre R{xs.data(), cs.data(), as.data(), ll.data(), z1.data(), z2.data(), 0, inc, n, lam, p};
    const double glam_ref = ptv::tvpvjp::solve(R);
    Vec gx_ref(g), gu_ref(gu), c_ref(n, -7.0), z_ref(zeta);   // gx_ref: DR_ROW / PD2 rewrite g's array ; DR_COL adds into gu's role below
    for (int i = 0; i < n; i++) {
        const double a = as[(size_t)i * inc];
        if (mode == DR_ROW) {
            if (final) { gu_ref[i] = a; c_ref[i] = a; gx_ref[i] = -a; }
            else { const double g0 = g[i]; gu_ref[i] = gu[i] + a; c_ref[i] = (a + a) - g0; gx_ref[i] = g0 - a; }
        } else if (mode == DR_COL) {
            gu_ref[i] = gu[i] + a;   // (gx is a second array: gu plays it)
        } else if (mode == PD2) {
            if (with) { gu_ref[i] = final ? a : gu[i] + a; gx_ref[i] = a - g[i]; }
            else gx_ref[i] = final ? a : a - g[i];
        } else if (mode == PD) {
            const double z = (with ? zeta[i] : 0.0) + a;
            z_ref[i] = z;
            gu_ref[i] = final ? z : gu[i] + z;
        } else {
            gx_ref[i] = a;
        }
    }
    // ---- the functors, on the arrays as the solvers alias them
    Vec gs = spread(g, inc), us = spread(gu, inc), cc(len, -7.0), zs = spread(zeta, inc);
    std::fill(ll.begin(), ll.end(), -7.0);
    std::fill(z1.begin(), z1.end(), -7.0);
    std::fill(z2.begin(), z2.end(), -7.0);
    double *G = gs.data(), *U = us.data(), *C = cc.data(), *Z = zs.data();
    const ptv::tvpvjp::Fibre F{xs.data(), G, G, ll.data(), z1.data(), z2.data(), 0, inc, n, lam, p};
    const long step = inc;
    double glam;
    if (mode == DR_ROW) {
        glam = ptv::tvpvjp::solve(F, [=](int i) { return G[i * step]; }, [=](int i, double a) {
            const long k = i * step;
            if (final) { U[k] = a; C[k] = a; G[k] = -a; }
            else { const double g0 = G[k]; U[k] = U[k] + a; C[k] = (a + a) - g0; G[k] = g0 - a; }
        });
    } else if (mode == DR_COL) {
        glam = ptv::tvpvjp::solve(F, [=](int i) { return G[i * step]; }, [=](int i, double a) { U[i * step] = U[i * step] + a; });
    } else if (mode == PD2) {
        glam = ptv::tvpvjp::solve(F, [=](int i) { return G[i * step]; }, [=](int i, double a) {
            const long k = i * step;
            if (with) { const double g0 = G[k]; U[k] = final ? a : U[k] + a; G[k] = a - g0; }
            else G[k] = final ? a : a - G[k];
        });
    } else if (mode == PD) {
        glam = ptv::tvpvjp::solve(F, [=](int i) { return std::fma(G[i * step], scale, -(with ? Z[i * step] : 0.0)); }, [=](int i, double a) {
            const long k = i * step;
            const double z = (with ? Z[k] : 0.0) + a;
            Z[k] = z;
            U[k] = final ? z : U[k] + z;
        });
    } else {
        glam = ptv::tvpvjp::solve(F);
    }
    expect(memcmp(&glam, &glam_ref, sizeof(double)) == 0, "glam", mode, n, p, inc, variant);
    Vec got_g(n), got_u(n), got_c(n), got_z(n);
    for (int i = 0; i < n; i++) {
        got_g[i] = gs[(size_t)i * inc];
        got_u[i] = us[(size_t)i * inc];
        got_c[i] = cc[(size_t)i * inc];
        got_z[i] = zs[(size_t)i * inc];
    }
    if (mode == PLAIN || mode == DR_ROW || mode == PD2) expect(same(got_g, gx_ref), "gx", mode, n, p, inc, variant);
    else expect(same(got_g, g), "g untouched", mode, n, p, inc, variant);
    if (mode == DR_ROW) expect(same(got_c, c_ref), "c", mode, n, p, inc, variant);
    if (mode == PD) expect(same(got_z, z_ref), "zeta", mode, n, p, inc, variant);
    if (mode != PLAIN && !(mode == PD2 && !with)) expect(same(got_u, gu_ref), "gU", mode, n, p, inc, variant);
    // the gap elements of a strided layout stay what they were
    for (size_t k = 0; k < len; k++)
        if (inc > 1 && k % (size_t)inc != 0 && (gs[k] != -7.0 || us[k] != -7.0 || cc[k] != -7.0 || zs[k] != -7.0)) {
            expect(false, "a gap element was written", mode, n, p, inc, variant);
            break;
        }
    // gU == g exactly (the final row sweep, the entry points' only aliasing of an output with the cotangent)
    if (mode == DR_ROW && final) {
        Vec g2 = spread(g, inc), c2(len, -7.0), x2(len, -7.0);
        double *A = g2.data(), *C2 = c2.data(), *X2 = x2.data();
        const ptv::tvpvjp::Fibre H{xs.data(), A, X2, ll.data(), z1.data(), z2.data(), 0, inc, n, lam, p};
        const double gl = ptv::tvpvjp::solve(H, [=](int i) { return A[i * step]; }, [=](int i, double a) {
            A[i * step] = a;
            C2[i * step] = a;
            X2[i * step] = -a;
        });
        Vec got(n);
        for (int i = 0; i < n; i++) got[i] = g2[(size_t)i * inc];
        expect(same(got, gu_ref) && memcmp(&gl, &glam_ref, sizeof(double)) == 0, "gU == g", mode, n, p, inc, variant);
    }
}

}  // namespace

int main() {
    const int lengths[] = {1, 2, 7, 8, 9, 17, 129};
    const double ps[] = {1.5, 3.0};
    Rng rng{12345};
    int cases = 0, iterated = 0, flat = 0;
    for (int n : lengths)
        for (double p : ps)
            for (int kind = 0; kind < 3; kind++) {   // 0, 1: the prox of noise at lambda = 0.05 / 0.8 ; 2: a constant output
                const double lam = kind == 1 ? 0.8 : 0.05;
                Vec y(n), x(n), g(n), gu(n), zeta(n);
                for (int i = 0; i < n; i++) { y[i] = 2.0 * rng.next(); g[i] = rng.next(); gu[i] = rng.next(); zeta[i] = rng.next(); }
                if (kind == 2) {
                    for (int i = 0; i < n; i++) x[i] = 0.3;
                } else {
                    Vec v(n + 1), dl(n + 1), l2(n + 1), zz(n + 1);
                    const ptv::tvp::Fibre F{y.data(), x.data(), v.data(), dl.data(), l2.data(), zz.data(), 0, 1, n, lam, p};
                    ptv::tvp::solve(F);
                }
                bool constant = true;
                for (int i = 1; i < n; i++) constant = constant && x[i] == x[0];
                (n > 1 && !constant ? iterated : flat)++;
                for (int inc : {1, 3})
                    for (int mode = PLAIN; mode <= PD; mode++)
                        for (int variant = 0; variant < 4; variant++) {
                            if ((mode == PLAIN || mode == DR_COL) && variant) continue;
                            if (mode == DR_ROW && (variant & 2)) continue;
                            run(mode, variant, x, g, gu, zeta, lam, p, inc);
                            cases++;
                        }
            }
    printf("%d cases, %d fibres iterated, %d closed forms, %d mismatches\n", cases, iterated, flat, failures);
    if (failures || iterated < 10 || flat < 10) return 1;
    printf("MODES_HOST_OK\n");
    return 0;
}
