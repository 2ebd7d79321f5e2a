"""Child process of tests/test_gpu_dr_jvp.py (run with PROXTV_POOL_CAP_MB=1; not a test module): the scratch of proxtv_DR2_TV_jvp_dev
does not depend on the iteration count -- a 64 x 64 image goes through at 35 and at 2000 iterations under a 1 MiB cap -- while
proxtv_DR2_TV_vjp_tape_dev at 2000 iterations is refused with either tape."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from proxtv_amd import _lib, device  # noqa: E402

assert os.environ.get("PROXTV_POOL_CAP_MB") == "1"
lib = _lib.require_device()
rng = np.random.default_rng(0)
M = N = 64
U = device.to_colmajor(torch.from_numpy(rng.standard_normal((M, N))).cuda())
dU = device.to_colmajor(torch.from_numpy(rng.standard_normal((M, N))).cuda())

for iters in (35, 2000):
    dy, _ = device.dr2_jvp(U, dU, 0.3, max_iters=iters, dw_col=1.0)
    assert bool(torch.isfinite(dy).all()) and bool((dy != 0).any()), iters
    print("jvp went through at", iters)

for tape in (0, 1):
    gU = torch.full_like(U, 7.0)
    torch.cuda.synchronize()
    rc = lib.proxtv_DR2_TV_vjp_tape_dev(M, N, 1, U.data_ptr(), 0.3, 0.3, 0, 0, dU.data_ptr(), 0, gU.data_ptr(), 0, 0, 0, 2000, tape, 0)
    msg = lib.proxtv_last_error().decode()
    print("vjp tape", tape, "refused:", rc, msg)
    assert rc == 0 and "PROXTV_POOL_CAP_MB" in msg and bool((gU == 7.0).all())
print("JVP_CAP_CHILD_OK")
