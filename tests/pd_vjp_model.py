"""Plain-numpy model of the two Dykstra loops tvgen dispatches to and of their derivatives (what proxtv_PD_TV_vjp_dev computes), shared by
tests/test_pd_vjp_model.py and tests/test_gpu_pd_vjp.py.  Not a test module.

Parallel proximal Dykstra (PD_TV; any number P of terms, term i along dims[i] with the penalty lams[i] as the C entry point receives it):
    z_i = y ; repeat K: p_i = prox_i(z_i) ; x = sum_i p_i / P ; z_i += x - p_i ; out = x
Two-term proximal Dykstra (PD2_TV; one term: a single sweep):
    x = y, p = q = 0 ; repeat K: z = prox_0(x + p), p += x - z ; x' = prox_1(z + q), q += z - x' ; x = x'
Reverse: the segmented means of vjp_model.vjp_nd at the kept sweep outputs, last iteration first.  The iteration count is
an input of both: the model, like the device call, differentiates the K-step recurrence and tests no stopping value."""
import numpy as np

import dr_vjp_model as dm
import vjp_model as vm

ITERS = 6

# (seed, loop, shape, dims 1-based, lambdas as the C entry point receives them): unit Gaussian y and cotangent, every lambda >= 0.05
CASES = ((1, "pd", (9, 7, 5), (1, 2, 3), (0.3, 0.21, 0.4)),
         (2, "pd", (12, 10), (1, 2), (0.25, 0.4)),
         (3, "pd2", (12, 10), (1, 2), (0.25, 0.4)),
         (4, "pd", (12, 10), (1, 2, 1), (0.3, 0.2, 0.12)),      # three terms, two of them along dimension 1
         (5, "pd", (12, 10), (2,), (0.35,)),                    # npen == 1
         (6, "pd2", (12, 10), (1,), (0.35,)),
         (7, "pd2", (9, 7, 5), (3, 1), (0.3, 0.2)))


def draw(seed, shape):
    """(y, cotangent) of one case."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), rng.standard_normal(shape)


def prox(oracle, a, dim, lam):
    return dm.prox_along(oracle, a, dim, lam)


def forward(oracle, loop, y, lams, dims, iters=ITERS):
    """(out, tape): tape[k] holds the sweep outputs of iteration k + 1 in the order of the terms."""
    y = np.asarray(y, dtype=np.float64)
    P = len(lams)
    ds = [int(d) - 1 for d in dims]
    tape = []
    if loop == "pd":
        z = [y.copy() for _ in range(P)]
        x = np.zeros_like(y)
        for _ in range(iters):
            p = [prox(oracle, z[i], ds[i], lams[i]) for i in range(P)]
            x = sum(p[1:], p[0]) / P
            for i in range(P):
                z[i] = z[i] + (x - p[i])
            tape.append(tuple(p))
        return x, tape
    assert loop == "pd2" and P in (1, 2)
    if P == 1:   # one sweep, whatever iters says: x + p stays y
        out = prox(oracle, y, ds[0], lams[0])
        return out, [(out,)]
    x, p, q = y, np.zeros_like(y), np.zeros_like(y)
    for _ in range(iters):
        z = prox(oracle, x + p, ds[0], lams[0])
        p = p + (x - z)
        xn = prox(oracle, z + q, ds[1], lams[1])
        q = q + (z - xn)
        tape.append((z, xn))
        x = xn
    return x, tape


def reverse(loop, tape, g, dims):
    """(gy, glam, sweeps, A): the gradients in y and in every penalty, the number S of reverse sweeps and the largest 2-norm A of any
    cotangent that went into one or came out of it (the bar of the device tests scales with both)."""
    ds = [int(d) - 1 for d in dims]
    P = len(ds)
    glam = np.zeros(P)
    norms = [float(np.linalg.norm(g))]
    sweeps = 0

    def P_(i, out, c):
        nonlocal sweeps
        a, gw, _ = vm.vjp_nd(out, c, ds[i])
        glam[i] += gw.sum()
        sweeps += 1
        norms.extend((float(np.linalg.norm(c)), float(np.linalg.norm(a))))
        return a

    if loop == "pd":
        zeta = [np.zeros_like(g) for _ in range(P)]
        xi = g
        for ps in reversed(tape):
            chi = xi + sum(zeta[1:], zeta[0])
            for i in range(P):
                zeta[i] = zeta[i] + P_(i, ps[i], chi / P - zeta[i])
                norms.append(float(np.linalg.norm(zeta[i])))
            norms.append(float(np.linalg.norm(chi)))
            xi = np.zeros_like(g)
        gy = sum(zeta[1:], zeta[0])
    elif P == 1:
        gy = P_(0, tape[0][0], g)
    else:
        X, Pb, Qb = g, np.zeros_like(g), np.zeros_like(g)
        for z, xn in reversed(tape):
            a = P_(1, xn, X - Qb)
            Zc = a + Qb - Pb
            Qb = a + Qb
            b = P_(0, z, Zc)
            X = Pb = Pb + b
            norms.extend(float(np.linalg.norm(v)) for v in (Qb, X))
        gy = X
    norms.append(float(np.linalg.norm(gy)))
    return gy, glam, sweeps, max(norms)


def assert_tape_unambiguous(tape, dims, hi=1e-6):
    """Precondition of every test: no jump of any taped prox output lies in [1e-12, hi] -- the step rule has nothing to decide (hi well
    above a difference quotient's h: nor has a perturbation of that size)."""
    for k, outs in enumerate(tape):
        for i, out in enumerate(outs):
            d = np.abs(np.diff(out, axis=int(dims[i]) - 1))
            bad = (d >= 1e-12) & (d <= hi)
            assert not np.any(bad), (k, i, float(d[bad].min()))


def draw_blocks(seed, shape, block=5, amp=3.0):
    """(y, cotangent) for central differences in the penalties on arrays of thousands of samples: y is constant on blocks of `block`
    samples a side, levels amp N(0, 1), so that every jump of every sweep output is either nothing or large.
    assert_tape_unambiguous(hi=...) and step_patterns() are what check that."""
    rng = np.random.default_rng(seed)
    levels = rng.standard_normal(tuple(-(-s // block) for s in shape))
    idx = np.ix_(*[np.arange(s) // block for s in shape])
    return amp * levels[idx], rng.standard_normal(shape)


def step_patterns(tape, dims):
    """The steps (vjp_model's rule) of every taped sweep output along its term's dimension: what the derivative is read off."""
    out = []
    for outs in tape:
        for i, o in enumerate(outs):
            a = np.moveaxis(o, int(dims[i]) - 1, -1)
            lo, hi = a[..., :-1], a[..., 1:]
            out.append(np.abs(hi - lo) > vm.STEP_REL * np.maximum(np.abs(lo), np.abs(hi)) + vm.STEP_ABS)
    return out


def same_patterns(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


def bar(shape, dims, sweeps, A):
    """64 S L 2^-52 A: the certifier's rounding rule per sum (64 n ulps), once per reverse sweep, L the longest fibre swept, A from
    reverse() -- the Dykstra reverse map is not shown non-expansive, so the cotangents' size is computed, not assumed."""
    L = max(shape[int(d) - 1] for d in dims)
    return 64.0 * sweeps * L * 2.0 ** -52 * A


def compose(torch, autograd, loop, y, lams, dims, iters):
    """The same recurrences written the way a user had to before the native derivative: autograd.tv1_fibres and torch's pointwise
    operations on CUDA tensors.  Differentiable in y and in 0-d tensors lams[i]."""
    P = len(lams)
    ds = [int(d) - 1 for d in dims]
    if loop == "pd":
        z = [y for _ in range(P)]
        x = None
        for _ in range(iters):
            p = [autograd.tv1_fibres(z[i], lams[i], ds[i]) for i in range(P)]
            x = p[0]
            for t in p[1:]:
                x = x + t
            x = x / P
            z = [z[i] + (x - p[i]) for i in range(P)]
        return x
    if P == 1:
        return autograd.tv1_fibres(y, lams[0], ds[0])
    x, p, q = y, torch.zeros_like(y), torch.zeros_like(y)
    for _ in range(iters):
        z = autograd.tv1_fibres(x + p, lams[0], ds[0])
        p = p + (x - z)
        xn = autograd.tv1_fibres(z + q, lams[1], ds[1])
        q = q + (z - xn)
        x = xn
    return x
