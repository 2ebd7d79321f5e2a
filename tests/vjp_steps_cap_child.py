"""Child process of tests/test_gpu_vjp_steps.py (run with PROXTV_POOL_CAP_MB=1; not a test module): under a 1 MiB cap the solver
derivatives refuse the tape of sweep outputs and go through with the tape of step codes, whose results -- printed here as sha1 -- the
parent compares with its own tape = 0 results at the default cap.  A step tape that does not fit either is refused with its bytes.
The parent imports the cases from here, so both processes draw the same inputs."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from proxtv_amd import _lib, device  # noqa: E402

DR_ITERS, PD_ITERS = 35, 7
PD_CASES = ((1, 3), (0, 2))     # (which, npen), tests/pd_vjp_cap_child.py's


def sha(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def draw(seed, M, N):
    rng = np.random.default_rng(seed)
    up = lambda a: device.to_colmajor(torch.from_numpy(a).cuda())   # noqa: E731
    return up(rng.standard_normal((M, N))), up(rng.standard_normal((M, N)))


def dr(lib, M, N, tape):
    """(rc, gU, s, glam) of proxtv_DR2_TV_vjp_tape_dev on the case of seed 0; the outputs start as 7."""
    U, g = draw(0, M, N)
    gU, s = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    glam = np.full(2, 7.0)
    torch.cuda.synchronize()
    rc = lib.proxtv_DR2_TV_vjp_tape_dev(M, N, 1, U.data_ptr(), 0.3, 0.3, 0, 0, g.data_ptr(), s.data_ptr(), gU.data_ptr(), 0, 0, glam.ctypes.data,
                                        DR_ITERS, tape, 0)
    return rc, gU, s, glam


def pd(lib, which, npen, M, N, tape):
    """(rc, gy, x, glam) of proxtv_PD_TV_vjp_tape_dev on the case of seed 1 + which."""
    y, g = draw(1 + which, M, N)
    gy, x = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    glam = np.full(npen, 7.0)
    lams, dims, ns = np.full(npen, 0.3), np.array([1.0, 2.0, 1.0][:npen]), np.array([M, N], dtype=np.int32)
    torch.cuda.synchronize()
    rc = lib.proxtv_PD_TV_vjp_tape_dev(which, y.data_ptr(), lams.ctypes.data, dims.ctypes.data, ns.ctypes.data, 2, npen, PD_ITERS, g.data_ptr(),
                                       x.data_ptr(), gy.data_ptr(), glam.ctypes.data, tape, 0)
    return rc, gy, x, glam


def untouched(*outs):
    return all(bool((o == 7.0).all()) for o in outs)


def main():
    assert os.environ.get("PROXTV_POOL_CAP_MB") == "1"
    lib = _lib.require_device()
    # Douglas-Rachford, 100 x 100, 35 iterations: 72 outputs are 5.76 MB, their codes and two arrays 361 600 B
    rc, gU, s, glam = dr(lib, 100, 100, 0)
    msg = lib.proxtv_last_error().decode()
    print("refused:", rc, msg)
    assert rc == 0 and str(2 * 36 * 8 * 100 * 100) in msg and "PROXTV_POOL_CAP_MB" in msg and untouched(gU, s, glam)
    rc, gU, s, glam = dr(lib, 100, 100, 1)
    assert rc == 1 and lib.proxtv_last_error() == b"", lib.proxtv_last_error()
    print("DR", sha(gU), sha(s), sha(glam))
    # ... and a step tape that does not fit either: 300 x 300, 36 * (2 * 300 * 19) words and two arrays
    rc, gU, s, glam = dr(lib, 300, 300, 1)
    msg = lib.proxtv_last_error().decode()
    print("refused:", rc, msg)
    assert rc == 0 and str(36 * 2 * 300 * 19 * 4 + 2 * 8 * 300 * 300) in msg and "PROXTV_POOL_CAP_MB" in msg and untouched(gU, s, glam)
    for which, npen in PD_CASES:
        rc, gy, x, glam = pd(lib, which, npen, 100, 100, 0)
        msg = lib.proxtv_last_error().decode()
        print("refused:", rc, msg)
        assert rc == 0 and str(npen * PD_ITERS * 8 * 100 * 100) in msg and untouched(gy, x, glam)
        rc, gy, x, glam = pd(lib, which, npen, 100, 100, 1)
        assert rc == 1 and lib.proxtv_last_error() == b"", lib.proxtv_last_error()
        print(f"PD{which}", sha(gy), sha(x), sha(glam))
        rc, gy, x, glam = pd(lib, which, npen, 300, 300, 1)
        msg = lib.proxtv_last_error().decode()
        print("refused:", rc, msg)
        assert rc == 0 and str(PD_ITERS * npen * 300 * 19 * 4 + npen * 8 * 300 * 300) in msg and untouched(gy, x, glam)
    print("CAP_CHILD_OK")


if __name__ == "__main__":
    main()
