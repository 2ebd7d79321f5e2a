"""Plain-numpy model of the three differentiated recurrences with ANY norm per term -- 1, 2 or a general p -- and of their derivatives
(what proxtv_DR2_TVp_vjp_dev and proxtv_PD_TVp_vjp_dev compute with option general_p_vjp), shared by
tests/test_tvpg_vjp_model.py and tests/test_gpu_tvpg_vjp.py.  Not a test module.

The recurrences are tvp_vjp_model's.  A term's Jacobian J is the segmented mean (p = 1), the TV-L2 model's two solves (p = 2), or the
dense general-p model of tests/tvp_fibres_vjp_model.py applied to the sweep's output.  Every reverse recurrence is linear in a = J c,
whichever prox J belongs to, and every J is symmetric: the forward-mode linearisation below runs the forward recurrence with J in the
place of the prox, and <g, T v> = <T' g, v> holds to rounding whatever the forward's own accuracy.

`prox(a, dim, lam, p)` is any callable that returns a tvp_vjp_model.Sweep."""
import numpy as np

import tvp_fibres_vjp_model as fm
import tvp_vjp_model as tp

FD_H = 1e-5
# |model - central differences (h = 1e-5)| of the recurrences built from the CPU oracle's exact p = 1 / p = 2 proxes and the host build of
# tvpcore.hpp for a general p: four times the worst figure measured on the cases of tests/test_tvpg_vjp_model.py (DESIGN.md 6j names
# the case: 7.5e-4 in a penalty gradient of DR (9, 7), p = (3, 1.5), lambda = 0.8, eight sweeps; every lambda = 0.05 case stays below
# 1.3e-6).  As in 6i the figure is the derivative of the forward's own stopping error (it stops at a duality gap of 1e-8; 8.7e-5 for
# one primal-arm sweep there), which the differences see and the model does not, carried through the recurrence.
FD_WORST = 7.5e-4
FD_BAR = 4 * FD_WORST
ADJOINT_TOL = 1e-12      # |<g, T v> - <T' g, v>| / (||g|| ||v||): rounding of a few dozen dense solves on arrays of <= 120 entries


def general(p):
    return p not in (1, 2)


def make_prox(oracle, host_forward):
    """prox(a, dim, lam, p): the oracle's exact prox for p in {1, 2}; for a general p `host_forward(x, lam, p)` on every fibre."""
    def prox(a, dim, lam, p):
        if not general(p):
            return tp.prox(oracle, a, dim, lam, p)
        am = np.moveaxis(np.asarray(a, dtype=np.float64), dim, -1)
        out = np.empty(am.shape)
        for idx in np.ndindex(*am.shape[:-1]):
            out[idx] = host_forward(np.ascontiguousarray(am[idx]), lam, p)
        return tp.Sweep(np.moveaxis(out, -1, dim), dim, lam, p)
    return prox


def vjp(sw, c):
    """(J c, d/dlam) of one sweep."""
    if not general(sw.p):
        return tp.vjp(sw, c)
    a, glam = fm.vjp_nd(sw.y, c, sw.lam, sw.p, sw.dim)
    return a, float(glam.sum())


# ---- Douglas-Rachford --------------------------------------------------------------------------------------------------------------------
def dr_forward(prox, U, W1, W2, p1, p2, maxit):
    """(out, tape): tape[k] = (x1_k, x2_k) as Sweeps, k = 0 .. maxit (tvp_vjp_model.dr_forward with any norm)."""
    U = np.asarray(U, dtype=np.float64)
    t = np.full(U.shape, 2.0 * U.mean())
    tape = []
    for _ in range(maxit):
        x1 = prox(t, 0, W1, p1)
        x2 = prox(U - (t - 2.0 * x1.y), 1, W2, p2)
        tape.append((x1, x2))
        t = t - x1.y + x2.y
    x1 = prox(t, 0, W1, p1)
    x2 = prox(U - (t - x1.y), 1, W2, p2)
    tape.append((x1, x2))
    return x2.y, tape


def dr_reverse(tape, g):
    """(gU, glam[2])."""
    glam = np.zeros(2)

    def J(sw, c, which):
        a, gl = vjp(sw, c)
        glam[which] += gl
        return a

    x1, x2 = tape[-1]
    a = J(x2, g, 1)
    gU = a.copy()
    gbar = J(x1, a, 0) - a
    for x1, x2 in reversed(tape[:-1]):
        a = J(x2, gbar, 1)
        gU += a
        gbar = gbar - a + J(x1, 2.0 * a - gbar, 0)
    gU += 2.0 * gbar.sum() / gbar.size
    return gU, glam


def dr_tangent(tape, v):
    """The forward-mode linearisation in U: the recurrence of dr_forward with every prox replaced by its (symmetric) Jacobian."""
    dt = np.full(v.shape, 2.0 * v.mean())
    for x1, x2 in tape[:-1]:
        d1 = vjp(x1, dt)[0]
        d2 = vjp(x2, v - (dt - 2.0 * d1))[0]
        dt = dt - d1 + d2
    x1, x2 = tape[-1]
    d1 = vjp(x1, dt)[0]
    return vjp(x2, v - (dt - d1))[0]


# ---- the Dykstra loops -------------------------------------------------------------------------------------------------------------------
def pd_forward(prox, loop, y, lams, dims, ps, iters):
    """(out, tape) as tvp_vjp_model.pd_forward, with any norm."""
    y = np.asarray(y, dtype=np.float64)
    P = len(lams)
    ds = [int(d) - 1 for d in dims]
    tape = []
    if loop == "pd":
        z = [y.copy() for _ in range(P)]
        x = np.zeros_like(y)
        for _ in range(iters):
            p = [prox(z[i], ds[i], lams[i], ps[i]) for i in range(P)]
            x = sum((s.y for s in p[1:]), p[0].y) / P
            for i in range(P):
                z[i] = z[i] + (x - p[i].y)
            tape.append(tuple(p))
        return x, tape
    assert loop == "pd2" and P in (1, 2)
    if P == 1:
        s = prox(y, ds[0], lams[0], ps[0])
        return s.y, [(s,)]
    x, p, q = y, np.zeros_like(y), np.zeros_like(y)
    for _ in range(iters):
        z = prox(x + p, ds[0], lams[0], ps[0])
        p = p + (x - z.y)
        xn = prox(z.y + q, ds[1], lams[1], ps[1])
        q = q + (z.y - xn.y)
        tape.append((z, xn))
        x = xn.y
    return x, tape


def pd_reverse(loop, tape, g):
    """(gy, glam) as tvp_vjp_model.pd_reverse."""
    P = len(tape[0])
    glam = np.zeros(P)

    def J(i, sw, c):
        a, gl = vjp(sw, c)
        glam[i] += gl
        return a

    if loop == "pd":
        zeta = [np.zeros_like(g) for _ in range(P)]
        xi = g
        for sws in reversed(tape):
            chi = xi + sum(zeta[1:], zeta[0])
            for i in range(P):
                zeta[i] = zeta[i] + J(i, sws[i], chi / P - zeta[i])
            xi = np.zeros_like(g)
        return sum(zeta[1:], zeta[0]), glam
    if P == 1:
        return J(0, tape[0][0], g), glam
    X, Pb, Qb = g, np.zeros_like(g), np.zeros_like(g)
    for z, xn in reversed(tape):
        a = J(1, xn, X - Qb)
        Zc = a + Qb - Pb
        Qb = a + Qb
        X = Pb = Pb + J(0, z, Zc)
    return X, glam


def pd_tangent(loop, tape, v):
    """The forward-mode linearisation in y."""
    P = len(tape[0])
    if loop == "pd":
        dz = [v.copy() for _ in range(P)]
        dx = np.zeros_like(v)
        for sws in tape:
            dp = [vjp(sws[i], dz[i])[0] for i in range(P)]
            dx = sum(dp[1:], dp[0]) / P
            dz = [dz[i] + (dx - dp[i]) for i in range(P)]
        return dx
    if P == 1:
        return vjp(tape[0][0], v)[0]
    dx, dp, dq = v, np.zeros_like(v), np.zeros_like(v)
    for z, xn in tape:
        d0 = vjp(z, dx + dp)[0]
        dp = dp + (dx - d0)
        d1 = vjp(xn, d0 + dq)[0]
        dq = dq + (d0 - d1)
        dx = d1
    return dx


def branches(tape):
    """(mean, iterative): how many general-p fibres of two samples or more answered with the mean (an exactly constant output) and how
    many did not, over all sweeps."""
    mean = iterative = 0
    for sw in tp.sweeps_of(tape):
        if general(sw.p) and sw.n >= 2 and sw.lam > 0:
            flat = np.all(np.diff(sw.y, axis=sw.dim) == 0, axis=sw.dim)
            mean += int(flat.sum())
            iterative += int(flat.size - flat.sum())
    return mean, iterative


# ---- the recurrences composed in torch ------------------------------------------------------------------------------------------------------
def fibres_of(autograd, p):
    """autograd.tvp_fibres hands p = 1 and p = 2 to tv1_fibres / tv2_fibres itself."""
    return lambda x, w, dim: autograd.tvp_fibres(x, w, p, dim)


def dr_compose(torch, autograd, U, W1, W2, p1, p2, maxit):
    cols, rows = fibres_of(autograd, p1), fibres_of(autograd, p2)
    t = 2.0 * U.mean() * torch.ones_like(U)
    for _ in range(maxit):
        x1 = cols(t, W1, 0)
        x2 = rows(U - (t - 2.0 * x1), W2, 1)
        t = t - x1 + x2
    x1 = cols(t, W1, 0)
    return rows(U - (t - x1), W2, 1)


def pd_compose(torch, autograd, loop, y, lams, dims, ps, iters):
    P = len(lams)
    ds = [int(d) - 1 for d in dims]
    f = [fibres_of(autograd, p) for p in ps]
    if loop == "pd":
        z = [y for _ in range(P)]
        x = None
        for _ in range(iters):
            p = [f[i](z[i], lams[i], ds[i]) for i in range(P)]
            x = p[0]
            for t in p[1:]:
                x = x + t
            x = x / P
            z = [z[i] + (x - p[i]) for i in range(P)]
        return x
    if P == 1:
        return f[0](y, lams[0], ds[0])
    x, p, q = y, torch.zeros_like(y), torch.zeros_like(y)
    for _ in range(iters):
        z = f[0](x + p, lams[0], ds[0])
        p = p + (x - z)
        xn = f[1](z + q, lams[1], ds[1])
        q = q + (z - xn)
        x = xn
    return x
