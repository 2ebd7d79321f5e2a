"""Plain-numpy model of the three differentiated recurrences with a norm in {1, 2} per term, and of their derivatives (what
proxtv_DR2_TVp_vjp_dev and proxtv_PD_TVp_vjp_dev compute), shared by tests/test_tvp_vjp_model.py and tests/test_gpu_tvp_vjp.py.  Not a
test module.

The recurrences are dr_vjp_model's and pd_vjp_model's, unchanged; a term's prox is the CPU oracle's exact TV-L1 or TV-L2 prox, and its
Jacobian J the segmented mean of vjp_model (p = 1) or tv2_vjp_model's two solves with the fibre's multiplier (p = 2).  Every reverse
recurrence is linear in a = J c, whichever prox J belongs to."""
import numpy as np

import dr_vjp_model as dm
import tv2_vjp_model as tm
import vjp_model as vm

KINK_CLEAR = 0.2      # every TV-L2 fibre of the CPU cases: | ||T^-1 D x|| - lambda | >= 0.2 lambda
FD_H = 1e-5
FD_TOL = 1e-7         # the project's bar for a composed loop's backward against central differences


class Sweep:
    """One taped sweep: its output y along `dim` with penalty lam and norm p; for p = 2 the multiplier mu and the dual norm un of every
    fibre, in the shape of y without `dim`."""

    def __init__(self, y, dim, lam, p, mu=None, un=None):
        self.y, self.dim, self.lam, self.p, self.mu, self.un = y, dim, lam, p, mu, un

    @property
    def n(self):
        return self.y.shape[self.dim]


def prox(oracle, a, dim, lam, p):
    """The oracle's 1-D prox of norm p on every fibre of `a` along `dim`, as a Sweep."""
    if p == 1:
        return Sweep(dm.prox_along(oracle, a, dim, lam), dim, lam, 1)
    assert p == 2
    am = np.moveaxis(a, dim, -1)
    out, mu, un = np.empty(am.shape), np.zeros(am.shape[:-1]), np.zeros(am.shape[:-1])
    for idx in np.ndindex(*am.shape[:-1]):
        x = np.ascontiguousarray(am[idx])
        if x.size < 2 or not lam > 0:
            out[idx] = x
            continue
        out[idx] = oracle.tv(x, lam, 2)[0]
        mu[idx], un[idx] = tm.mu_of(x, out[idx], lam, banded=x.size > 400)
    return Sweep(np.moveaxis(out, -1, dim), dim, lam, 2, mu, un)


def vjp(sw, c):
    """(J c, d/dlam) of one sweep."""
    if sw.p == 1:
        a, gw, _ = vm.vjp_nd(sw.y, c, sw.dim)
        return a, float(gw.sum())
    if sw.n > 400:
        ym, cm = np.moveaxis(sw.y, sw.dim, -1), np.moveaxis(c, sw.dim, -1)
        a, gl = np.empty(ym.shape), 0.0
        for idx in np.ndindex(*ym.shape[:-1]):
            a[idx], v = tm.vjp_1d(ym[idx], sw.mu[idx], cm[idx], sw.lam, banded=True)
            gl += v
        return np.moveaxis(a, -1, sw.dim), gl
    a, glam = tm.vjp_nd(sw.y, sw.mu.ravel(order="F"), c, sw.lam, sw.dim)
    return a, float(glam.sum())


# ---- Douglas-Rachford --------------------------------------------------------------------------------------------------------------------
def dr_forward(oracle, U, W1, W2, p1, p2, maxit):
    """(out, tape): tape[k] = (x1_k, x2_k) as Sweeps, k = 0 .. maxit, the last pair being the final sweeps'."""
    U = np.asarray(U, dtype=np.float64)
    t = np.full(U.shape, 2.0 * U.mean())
    tape = []
    for _ in range(maxit):
        x1 = prox(oracle, t, 0, W1, p1)
        x2 = prox(oracle, U - (t - 2.0 * x1.y), 1, W2, p2)
        tape.append((x1, x2))
        t = t - x1.y + x2.y
    x1 = prox(oracle, t, 0, W1, p1)
    x2 = prox(oracle, U - (t - x1.y), 1, W2, p2)
    tape.append((x1, x2))
    return x2.y, tape


def dr_reverse(tape, g):
    """(gU, glam[2], sweeps, A): A the largest 2-norm of any cotangent that went into a sweep or came out of one."""
    glam = np.zeros(2)
    norms = [float(np.linalg.norm(g))]

    def J(sw, c, which):
        a, gl = vjp(sw, c)
        glam[which] += gl
        norms.extend((float(np.linalg.norm(c)), float(np.linalg.norm(a))))
        return a

    x1, x2 = tape[-1]
    a = J(x2, g, 1)
    gU = a.copy()
    gbar = J(x1, a, 0) - a
    for x1, x2 in reversed(tape[:-1]):
        a = J(x2, gbar, 1)
        gU += a
        gbar = gbar - a + J(x1, 2.0 * a - gbar, 0)
        norms.append(float(np.linalg.norm(gbar)))
    gU += 2.0 * gbar.sum() / gbar.size
    return gU, glam, 2 * len(tape), max(norms)


# ---- the Dykstra loops -------------------------------------------------------------------------------------------------------------------
def pd_forward(oracle, loop, y, lams, dims, ps, iters):
    """(out, tape): tape[k] holds the Sweeps of iteration k + 1 in the order of the terms (pd_vjp_model.forward with norms)."""
    y = np.asarray(y, dtype=np.float64)
    P = len(lams)
    ds = [int(d) - 1 for d in dims]
    tape = []
    if loop == "pd":
        z = [y.copy() for _ in range(P)]
        x = np.zeros_like(y)
        for _ in range(iters):
            p = [prox(oracle, z[i], ds[i], lams[i], ps[i]) for i in range(P)]
            x = sum((s.y for s in p[1:]), p[0].y) / P
            for i in range(P):
                z[i] = z[i] + (x - p[i].y)
            tape.append(tuple(p))
        return x, tape
    assert loop == "pd2" and P in (1, 2)
    if P == 1:
        s = prox(oracle, y, ds[0], lams[0], ps[0])
        return s.y, [(s,)]
    x, p, q = y, np.zeros_like(y), np.zeros_like(y)
    for _ in range(iters):
        z = prox(oracle, x + p, ds[0], lams[0], ps[0])
        p = p + (x - z.y)
        xn = prox(oracle, z.y + q, ds[1], lams[1], ps[1])
        q = q + (z.y - xn.y)
        tape.append((z, xn))
        x = xn.y
    return x, tape


def pd_reverse(loop, tape, g):
    """(gy, glam, sweeps, A) as pd_vjp_model.reverse."""
    P = len(tape[0])
    glam = np.zeros(P)
    norms = [float(np.linalg.norm(g))]
    sweeps = 0

    def J(i, sw, c):
        nonlocal sweeps
        a, gl = vjp(sw, c)
        glam[i] += gl
        sweeps += 1
        norms.extend((float(np.linalg.norm(c)), float(np.linalg.norm(a))))
        return a

    if loop == "pd":
        zeta = [np.zeros_like(g) for _ in range(P)]
        xi = g
        for sws in reversed(tape):
            chi = xi + sum(zeta[1:], zeta[0])
            for i in range(P):
                zeta[i] = zeta[i] + J(i, sws[i], chi / P - zeta[i])
                norms.append(float(np.linalg.norm(zeta[i])))
            norms.append(float(np.linalg.norm(chi)))
            xi = np.zeros_like(g)
        gy = sum(zeta[1:], zeta[0])
    elif P == 1:
        gy = J(0, tape[0][0], g)
    else:
        X, Pb, Qb = g, np.zeros_like(g), np.zeros_like(g)
        for z, xn in reversed(tape):
            a = J(1, xn, X - Qb)
            Zc = a + Qb - Pb
            Qb = a + Qb
            X = Pb = Pb + J(0, z, Zc)
            norms.extend(float(np.linalg.norm(v)) for v in (Qb, X))
        gy = X
    norms.append(float(np.linalg.norm(gy)))
    return gy, glam, sweeps, max(norms)


# ---- what keeps the derivative well defined, and the bars ----------------------------------------------------------------------------------
def sweeps_of(tape):
    return [sw for step in tape for sw in step]


def kink_clearance(tape):
    """The smallest | ||T^-1 D x|| - lambda | / lambda over every TV-L2 fibre (of two samples or more) of every sweep; inf without one."""
    worst = np.inf
    for sw in sweeps_of(tape):
        if sw.p == 2 and sw.n >= 2 and sw.lam > 0:
            worst = min(worst, float(np.min(np.abs(sw.un - sw.lam))) / sw.lam)
    return worst


def assert_well_defined(tape, clear=KINK_CLEAR, hi=1e-6):
    """Every TV-L2 fibre of every sweep stays `clear` away from the kink, and no jump of a TV-L1 sweep output lies in [1e-12, hi]: the
    step rule has nothing to decide (dr_vjp_model.assert_tape_unambiguous)."""
    assert kink_clearance(tape) >= clear, kink_clearance(tape)
    for k, sw in enumerate(sweeps_of(tape)):
        if sw.p == 1:
            d = np.abs(np.diff(sw.y, axis=sw.dim))
            bad = (d >= 1e-12) & (d <= hi)
            assert not np.any(bad), (k, float(d[bad].min()))


def branches(tape):
    """(inside, active): how many TV-L2 fibres of two samples or more took each branch, over all sweeps."""
    inside = active = 0
    for sw in sweeps_of(tape):
        if sw.p == 2 and sw.n >= 2 and sw.lam > 0:
            inside += int(np.sum(sw.mu == 0))
            active += int(np.sum(sw.mu > 0))
    return inside, active


def worst_cond(tape):
    """The worst cond(T + mu I) = (4 + mu) / (mu + 4 sin^2(pi / 2n)) over the TV-L2 fibres and sweeps (tv2_vjp_model.cond); 1 without one."""
    worst = 1.0
    for sw in sweeps_of(tape):
        if sw.p == 2 and sw.n >= 2 and sw.lam > 0:
            worst = max(worst, float(np.max(tm.cond(sw.n, sw.mu))))
    return worst


def bar(tape, sweeps, A):
    """The TV-L1 recurrence's bar -- 64 S L 2^-52 A, the certifier's rounding rule per sum, once per reverse sweep, L the longest fibre
    swept, A the largest cotangent (pd_vjp_model.bar; dr_vjp_model.sweep_scale is the same with S = 2 maxit + 2) -- times worst_cond."""
    L = max(sw.n for sw in sweeps_of(tape))
    return 64.0 * sweeps * L * 2.0 ** -52 * A * worst_cond(tape)


def glam_bars(tape, sweeps, A):
    """Per penalty.  A TV-L1 term's gradient is a sum over its K sweeps and E edges of differences of two means: 2 K E bars
    (test_gpu_pd_vjp.py).  A TV-L2 term's is a sum over its K sweeps and F fibres of glam = -mu lam (h'q) / ((Dy)'q), linear in the
    fibre's cotangent c with |glam| <= sqrt(4 + mu) ||Dc||_{M^-1} <= 2 sqrt(cond) ||c||_2 (||Dy||_{M^-1} >= mu lam / sqrt(4 + mu)).  The
    cotangent arrives within the bar per entry, sqrt(n) bars in the 2-norm, and the fibre's own rounding is of the same form: 4 sqrt(n
    cond) bars per fibre and sweep."""
    b = bar(tape, sweeps, A)
    c = worst_cond(tape)
    out = []
    for i in range(len(tape[0])):
        sws = [step[i] for step in tape]
        sw = sws[0]
        fibres = sw.y.size // sw.n
        if sw.p == 1:
            out.append(2.0 * len(sws) * max(fibres * (sw.n - 1), 1) * b)
        else:
            out.append(len(sws) * fibres * 4.0 * np.sqrt(sw.n * c) * b)
    return np.array(out)


# ---- the recurrences composed in torch ------------------------------------------------------------------------------------------------------
def fibres_of(autograd, p):
    return autograd.tv1_fibres if p == 1 else autograd.tv2_fibres


def dr_compose(torch, autograd, U, W1, W2, p1, p2, maxit):
    """dr_vjp_model.compose with autograd.tv1_fibres / autograd.tv2_fibres by the direction's norm."""
    cols, rows = fibres_of(autograd, p1), fibres_of(autograd, p2)
    t = 2.0 * U.mean() * torch.ones_like(U)
    for _ in range(maxit):
        x1 = cols(t, W1, 0)
        x2 = rows(U - (t - 2.0 * x1), W2, 1)
        t = t - x1 + x2
    x1 = cols(t, W1, 0)
    return rows(U - (t - x1), W2, 1)


def pd_compose(torch, autograd, loop, y, lams, dims, ps, iters):
    """pd_vjp_model.compose with the term's norm."""
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


# ---- the CPU cases: inputs chosen so that assert_well_defined holds (tests/test_tvp_vjp_model.py asserts it) ---------------------------------
def draw_rows(seed, shape, amps, axis):
    """(data, cotangent): unit-normal data whose slices along `axis` are scaled by amps in turn, so that fibres ACROSS that axis differ in
    size: with the right penalty part of the TV-L2 fibres lies inside the ball and part is active."""
    rng = np.random.default_rng(seed)
    y, g = rng.standard_normal(shape), rng.standard_normal(shape)
    scale = np.array([amps[i % len(amps)] for i in range(shape[axis])])
    return y * scale.reshape([-1 if i == axis else 1 for i in range(len(shape))]), g
