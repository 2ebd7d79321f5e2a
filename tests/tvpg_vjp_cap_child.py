"""Child process of tests/test_gpu_tvpg_vjp.py (run with PROXTV_POOL_CAP_MB=1 and PROXTV_GENERAL_P_VJP=1; not a test module):
proxtv_DR2_TVp_vjp_dev and proxtv_PD_TVp_vjp_dev calls with a general-p term whose tape, or whose general-p sweeps' scratch forward or in
reverse, does not fit under the scratch pool's cap are refused before anything runs -- return 0, name the bytes of the header's formulas
under both tapes, write nothing -- and calls that fit go through."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from proxtv_amd import _lib, device  # noqa: E402

assert os.environ.get("PROXTV_POOL_CAP_MB") == "1" and os.environ.get("PROXTV_GENERAL_P_VJP") == "1"
lib = _lib.require_device()
assert _lib.option_value("general_p_vjp") == 1 and _lib.option_value("general_p") == 0
rng = np.random.default_rng(0)


def term_bytes(shape, dim, p, K, tape):
    """include/proxtv_amd.h: TV-L1, tape 0: 8 K n ; TV-L1, tape 1: 8 n + 4 K words ; TV-L2: 8 K (n + fibres) ; a general p: 8 K n."""
    n = int(np.prod(shape))
    ns = np.array(shape, dtype=np.int32)
    if p == 2:
        return 8 * K * (n + n // shape[dim])
    if p != 1:
        return 8 * K * n
    return 8 * n + 4 * K * lib.proxtv_tv1_steps_words(ns.ctypes.data, len(shape), dim) if tape else 8 * K * n


def forward_bytes(shape, dim):
    """... a general-p sweep forward: four arrays of the data's size, six along dimension 0 of several fibres, 12 bytes per fibre, 32."""
    n = int(np.prod(shape))
    fibres = n // shape[dim]
    return 8 * n * (6 if dim == 0 and fibres > 1 else 4) + 12 * fibres + 32


def reverse_bytes(shape, dim, pd, glam=True):
    """... and in reverse along dimension 0 of several fibres (always the epilogue route): five arrays, one more for a = J g, one more for
    pi (which = 1), one double per fibre where glam is asked for."""
    n = int(np.prod(shape))
    fibres = n // shape[dim]
    assert dim == 0 and fibres > 1
    return 8 * n * (5 + 1 + (1 if pd else 0)) + (8 * fibres if glam else 0)


def up(shape):
    return device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())


def dr(M, N, ps, tape, maxit=35):
    U, g = up((M, N)), up((M, N))
    gU, s, glam = torch.full_like(g, 7.0), torch.full_like(g, 7.0), np.full(2, 7.0)
    torch.cuda.synchronize()
    rc = lib.proxtv_DR2_TVp_vjp_dev(M, N, U.data_ptr(), 0.3, 0.3, float(ps[0]), float(ps[1]), g.data_ptr(), s.data_ptr(), gU.data_ptr(),
                                    glam.ctypes.data, maxit, tape, 0)
    return rc, gU, s, glam


def pd(which, shape, dims, ps, tape, iters):
    y, g = up(shape), up(shape)
    gy, x, glam = torch.full_like(g, 7.0), torch.full_like(g, 7.0), np.full(len(dims), 7.0)
    lams, dd, norms, ns = np.full(len(dims), 0.3), np.array(dims, dtype=np.float64), np.array(ps, dtype=np.float64), np.array(shape, dtype=np.int32)
    torch.cuda.synchronize()
    rc = lib.proxtv_PD_TVp_vjp_dev(which, y.data_ptr(), lams.ctypes.data, norms.ctypes.data, dd.ctypes.data, ns.ctypes.data, len(shape), len(dims),
                                   iters, g.data_ptr(), x.data_ptr(), gy.data_ptr(), glam.ctypes.data, tape, 0)
    return rc, gy, x, glam


def refused(rc, a, b, glam, need, word):
    msg = lib.proxtv_last_error().decode()
    print("refused:", rc, msg, "expected", need)
    assert need > 2 ** 20 and rc == 0 and str(need) in msg and word in msg and "PROXTV_POOL_CAP_MB" in msg
    assert bool((a == 7.0).all()) and bool((b == 7.0).all()) and np.all(glam == 7.0)


for tape in (0, 1):
    # the tape
    for ps in ((1, 1.5), (3, 2), (1.5, 7)):
        need = sum(term_bytes((100, 100, 1), d, ps[d], 36, tape) for d in (0, 1))
        refused(*dr(100, 100, ps, tape), need, "tape")
    shape, dims, ps, iters = (40, 30, 9), (1, 2, 1, 3), (1, 1.5, 3, 1), 12
    need = sum(term_bytes(shape, d - 1, p, iters, tape) for d, p in zip(dims, ps))
    refused(*pd(1, shape, dims, ps, tape, iters), need, "tape")
    # a general-p sweep's scratch forward: one term, one sweep, a tape of 8 n
    shape = (200, 200)
    assert term_bytes(shape, 1, 1.5, 1, tape) <= 2 ** 20
    refused(*pd(0, shape, (2,), (1.5,), tape, 1), forward_bytes(shape, 1), "forward")
    # ... and in reverse: along dimension 0 the derivative holds more than the forward
    shape = (100, 200)
    assert term_bytes(shape, 0, 3, 1, tape) + term_bytes(shape, 1, 1, 1, tape) <= 2 ** 20 and forward_bytes(shape, 0) <= 2 ** 20
    refused(*pd(1, shape, (1, 2), (3, 1), tape, 1), reverse_bytes(shape, 0, True), "reverse")
    # calls that fit
    rc, gU, s, glam = dr(10, 10, (1.5, 1), tape)
    assert rc == 1 and lib.proxtv_last_error() == b"" and not bool((gU == 7.0).any()) and not np.any(glam == 7.0)
    rc, gy, x, glam = pd(1, (6, 5, 4), (1, 2, 3), (1, 3, 1.5), tape, 3)
    assert rc == 1 and lib.proxtv_last_error() == b"" and not bool((gy == 7.0).any()) and not np.any(glam == 7.0)
print("CAP_CHILD_OK")
