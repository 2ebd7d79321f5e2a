"""Child process of tests/test_gpu_pd_vjp.py (run with PROXTV_POOL_CAP_MB=1; not a test module): a proxtv_PD_TV_vjp_dev call whose tape
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
ITERS = 7


def run(which, M, N, npen):
    y = device.to_colmajor(torch.from_numpy(rng.standard_normal((M, N))).cuda())
    g = device.to_colmajor(torch.from_numpy(rng.standard_normal((M, N))).cuda())
    gy, x = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    glam = np.full(npen, 7.0)
    lams, dims, ns = np.full(npen, 0.3), np.array([1.0, 2.0, 1.0][:npen]), np.array([M, N], dtype=np.int32)
    torch.cuda.synchronize()
    rc = lib.proxtv_PD_TV_vjp_dev(which, y.data_ptr(), lams.ctypes.data, dims.ctypes.data, ns.ctypes.data, 2, npen, ITERS, g.data_ptr(), x.data_ptr(),
                                  gy.data_ptr(), glam.ctypes.data, 0)
    return rc, gy, x, glam


for which, npen in ((1, 3), (0, 2)):
    rc, gy, x, glam = run(which, 100, 100, npen)
    msg = lib.proxtv_last_error().decode()
    print("refused:", rc, msg)
    assert rc == 0 and str(npen * ITERS * 8 * 100 * 100) in msg and "PROXTV_POOL_CAP_MB" in msg
    assert bool((gy == 7.0).all()) and bool((x == 7.0).all()) and np.all(glam == 7.0)
    rc, gy, x, glam = run(which, 10, 10, npen)
    assert rc == 1 and lib.proxtv_last_error() == b"" and not bool((gy == 7.0).any()) and not np.any(glam == 7.0)
print("CAP_CHILD_OK")
