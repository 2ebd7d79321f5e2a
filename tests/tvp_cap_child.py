"""Child process of tests/test_gpu_tvp.py (run with PROXTV_POOL_CAP_MB=1; not a test module): a general-p fibre prox whose scratch
does not fit under the scratch pool's cap is refused -- an error that names the bytes, nothing written, no fault -- and one that fits
goes through."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from proxtv_amd import ProxTVError, _lib, device  # noqa: E402

assert os.environ.get("PROXTV_POOL_CAP_MB") == "1"
lib = _lib.require_device()
rng = np.random.default_rng(0)

for shape, dim, arrays in (((200, 200), 1, 4), ((200, 200), 0, 6)):
    x = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
    out = torch.full_like(x, 7.0)
    need = 8 * x.numel() * arrays + 12 * (x.numel() // shape[dim]) + 32
    assert need > 2 ** 20
    try:
        device.tvp_fibres(x, 0.5, 3.0, dim, out=out)
    except ProxTVError as e:
        print("refused:", e)
        assert str(need) in str(e) and "PROXTV_POOL_CAP_MB" in str(e)
    else:
        raise AssertionError("a call beyond the cap went through")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
x = device.to_colmajor(torch.from_numpy(rng.standard_normal((20, 30))).cuda())
y, gap = device.tvp_fibres(x, 0.5, 3.0, 1, return_gap=True)
assert lib.proxtv_last_error() == b"" and float(gap.max()) <= 1e-5 and bool(torch.isfinite(y).all())
print("CAP_CHILD_OK")
