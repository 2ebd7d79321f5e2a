"""Writes tests/golden/golden_pgen.npz: what the compiled reference (oracle/_ref, one thread) returns for general-p TV-Lp problems.

    python tests/golden/make_golden_pgen.py

1-D: TV(y, lam, p) over tvp_model.GRID (the two corners the reference does not finish -- p = 1.1 at lam = 30, and n = 1000, p = 1.5,
lam = 30 -- are not part of the grid).  Every stored case is ASSERTED to have returned RC_OK with tvp_gap <= 1e-5: a case that does not
fails the generator, none is dropped.  Loops: DR2_TV / PD2_TV on a 24 x 20 image and PD_TV on a 10 x 12 x 6 volume with general norms."""
import os
import sys

os.environ["OMP_NUM_THREADS"] = "1"

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import tvp_model  # noqa: E402
from oracle import cpu  # noqa: E402

SEED = 1
IMG_NORMS = [(1.5, 3.0), (3.0, 1.0), (2.0, 1.5)]
IMG_W = (0.3, 0.3)
VOL_NORMS, VOL_W, VOL_DIMS = [3.0, 1.0, 1.5], [0.2, 0.3, 0.25], [1, 2, 3]


def main():
    ref = cpu.reference()
    out = {"grid": np.array(tvp_model.GRID, dtype=np.float64), "seed": np.array(SEED)}
    worst = 0.0
    for n in sorted({int(c[0]) for c in tvp_model.GRID}):
        out[f"y_{n}"] = tvp_model.signal(n, SEED)
    for k, (n, p, lam) in enumerate(tvp_model.GRID):
        y = out[f"y_{n}"]
        x, info = ref.tv(y, lam, p)
        gap = tvp_model.tvp_gap(x, y, lam, p)
        assert info[2] == 0, f"case {(n, p, lam)}: the reference returned info[2] = {info[2]}"
        assert gap <= 1e-5, f"case {(n, p, lam)}: the reference's gap is {gap}"
        worst = max(worst, gap)
        out[f"x_{k}"], out[f"info_{k}"] = x, info
    rng = np.random.default_rng(SEED)
    img = rng.standard_normal((24, 20))
    img[8:16, 5:12] += 2.0
    vol = rng.standard_normal((10, 12, 6))
    vol[3:7, 4:9, 2:5] += 2.0
    out["img"], out["vol"] = img, vol
    out["img_norms"], out["img_w"] = np.array(IMG_NORMS), np.array(IMG_W)
    out["vol_norms"], out["vol_w"], out["vol_dims"] = np.array(VOL_NORMS), np.array(VOL_W), np.array(VOL_DIMS, dtype=np.float64)
    for j, (p1, p2) in enumerate(IMG_NORMS):
        for tag, iters in (("5", 5), ("0", 0)):
            s, info, rc = ref.dr2(img, IMG_W[0], IMG_W[1], max_iters=iters, norm1=p1, norm2=p2)
            assert info[2] != 3
            out[f"dr2_{tag}_{j}"], out[f"dr2_{tag}_{j}_info"] = s, info
            s, info, rc, _ = ref.pd2(img, list(IMG_W), [1, 2], norms=[p1, p2], max_iters=iters)
            assert info[2] != 3
            out[f"pd2_{tag}_{j}"], out[f"pd2_{tag}_{j}_info"] = s, info
    s, info, rc, _ = ref.pd(vol, VOL_W, VOL_DIMS, norms=VOL_NORMS)
    assert info[2] != 3
    out["pd_vol"], out["pd_vol_info"] = s, info
    path = os.path.join(HERE, "golden_pgen.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(tvp_model.GRID)} 1-D cases, largest reference gap {worst:.3e}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
