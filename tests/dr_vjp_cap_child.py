"""Child process of tests/test_gpu_dr_vjp.py (run with PROXTV_POOL_CAP_MB=1; not a test module): a proxtv_DR2_TV_vjp_dev call whose tape
does not fit under the scratch pool's cap is refused -- returns 0, names the bytes, writes nothing -- and one that fits goes through."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from proxtv_amd import _lib, device  # noqa: E402

assert os.environ.get("PROXTV_POOL_CAP_MB") == "1"
lib = _lib.require_device()
rng = np.random.default_rng(0)


def run(M, N):
    U = device.to_colmajor(torch.from_numpy(rng.standard_normal((M, N))).cuda())
    g = device.to_colmajor(torch.from_numpy(rng.standard_normal((M, N))).cuda())
    gU, s = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    glam = np.full(2, 7.0)
    torch.cuda.synchronize()
    rc = lib.proxtv_DR2_TV_vjp_dev(M, N, 1, U.data_ptr(), 0.3, 0.3, 0, 0, g.data_ptr(), s.data_ptr(), gU.data_ptr(), 0, 0, glam.ctypes.data, 35, 0)
    return rc, gU, s, glam


rc, gU, s, glam = run(100, 100)
msg = lib.proxtv_last_error().decode()
print("refused:", rc, msg)
assert rc == 0 and str(2 * 36 * 8 * 100 * 100) in msg and "PROXTV_POOL_CAP_MB" in msg
assert bool((gU == 7.0).all()) and bool((s == 7.0).all()) and np.all(glam == 7.0)
rc, gU, s, glam = run(10, 10)
assert rc == 1 and lib.proxtv_last_error() == b"" and not bool((gU == 7.0).any()) and not np.any(glam == 7.0)
print("CAP_CHILD_OK")
