"""Child process of tests/test_gpu_tvp_fibres_vjp.py (run with PROXTV_POOL_CAP_MB=1; not a test module): a general-p fibre derivative
whose scratch does not fit under the scratch pool's cap is refused -- an error that names the bytes, nothing written, no fault -- and one
that fits goes through."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from proxtv_amd import ProxTVError, _lib, device  # noqa: E402

assert os.environ.get("PROXTV_POOL_CAP_MB") == "1"
lib = _lib.require_device()
rng = np.random.default_rng(0)

for shape, dim, arrays in (((250, 250), 1, 3), ((250, 250), 0, 5)):
    y = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())      # (any array serves as an output here)
    g = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
    out = torch.full_like(y, 7.0)
    need = 8 * y.numel() * arrays
    assert need > 2 ** 20
    try:
        device.tvp_fibres_vjp(y, g, 0.5, 3.0, dim, out=out)
    except ProxTVError as e:
        print("refused:", e)
        assert str(need) in str(e) and "PROXTV_POOL_CAP_MB" in str(e)
    else:
        raise AssertionError("a call beyond the cap went through")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
x = device.to_colmajor(torch.from_numpy(rng.standard_normal((20, 30))).cuda())
g = device.to_colmajor(torch.from_numpy(rng.standard_normal((20, 30))).cuda())
y = device.tvp_fibres(x, 0.5, 3.0, 1)
gx, glam = device.tvp_fibres_vjp(y, g, 0.5, 3.0, 1, need_glam=True)
assert lib.proxtv_last_error() == b"" and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(glam).all())
print("CAP_CHILD_OK")
