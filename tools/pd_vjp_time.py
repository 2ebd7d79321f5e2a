#!/usr/bin/env python3
"""Time of the native derivative of tvgen's two Dykstra loops (device.tvgen_vjp: unfused forward with its tape, then the reverse sweeps)
against (a) the fused forward solve alone (device.tvgen) and (b) the same recurrence composed in torch from autograd.tv1_fibres, forward
and backward -- what a user had to write before, and code that predates the native call: the yardstick.  Same process, torch.cuda.Event
pairs on the stream all of them run on, 3 warm-ups, median of 20 whole calls (each ends in a stream synchronise); native and composed
calls alternate, so that neither has the warmer machine.  The iteration count is what the fused solve reports.  Gradients asked for: x
and every penalty, in (b) as 0-d tensors.  Also: the peak tape bytes, the largest difference between the two gradients, and a sha1 of
the native gy (--compare-with: the file of an earlier run, in another process, to state whether the two gave the same bits).

    python tools/pd_vjp_time.py [--out profiles/pd_vjp_time.txt] [--compare-with earlier.txt]
"""
import argparse
import hashlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import pd_vjp_model as pm  # noqa: E402   (compose: the composition tests/test_gpu_pd_vjp.py checks the native call against)
from proxtv_amd import _lib, autograd, build, device  # noqa: E402

CASES = [("512 x 512 x 64 Gaussian, pd, lambda 0.1", (512, 512, 64), (1, 2, 3), "pd", 0.1),
         ("4096 x 4096 Gaussian, pd2, lambda 0.1", (4096, 4096), (1, 2), "pd2", 0.1)]
WARMUP, REPS = 3, 20


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare-with", default=None)
    args = ap.parse_args()
    _lib.require_device()
    stream = torch.cuda.Stream()
    lines = [f"# tools/pd_vjp_time.py, build {build.build_id()}, {torch.cuda.get_device_name(0)}",
             f"# median (min .. max) of {REPS} calls after {WARMUP} warm-ups, torch.cuda.Event on the calls' stream; native and composed calls alternate",
             "# forward: device.tvgen (fused) | native: device.tvgen_vjp (unfused forward + tape + reverse) | composed: autograd.tv1_fibres + torch, forward + backward",
             f"{'case':40s} {'K':>3s} {'forward ms':>28s} {'native ms':>28s} {'composed ms':>30s} {'comp/native':>11s} {'tape MB':>9s} {'|d gx|':>9s}"]
    prints = []
    with torch.cuda.stream(stream):
        for name, shape, ds, loop, lam in CASES:
            rng = np.random.default_rng(0)
            x = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            g = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            y = device.colmajor_empty(shape)
            P = len(ds)
            ws = [lam] * P
            torch.cuda.synchronize()
            K = int(device.tvgen(x, ws, ds, 0, loop, out=y)[1][0])
            scale = P if loop == "pd" else 1

            def composed():
                xt = x.detach().requires_grad_(True)
                wt = [torch.tensor(lam, dtype=torch.float64, device="cuda", requires_grad=True) for _ in range(P)]
                (g * pm.compose(torch, autograd, loop, xt, [w * scale for w in wt], ds, K)).sum().backward()
                return xt.grad, [float(w.grad) for w in wt]

            native = lambda: device.tvgen_vjp(x, g, ws, ds, K, loop, need_glam=True)   # noqa: E731
            for _ in range(WARMUP):
                device.tvgen(x, ws, ds, 0, loop, out=y)
                native()
                composed()
            fwd = stats([timed(lambda: device.tvgen(x, ws, ds, 0, loop, out=y), stream) for _ in range(REPS)])
            tn, tc = [], []
            for _ in range(REPS):
                tn.append(timed(native, stream))
                tc.append(timed(composed, stream))
            nat, com = stats(tn), stats(tc)
            gx, glam, _ = native()
            cx, cl = composed()
            diff = float((gx - cx).abs().max())
            prints.append(f"# gy sha1 [{name}] {hashlib.sha1(gx.cpu().numpy().tobytes(order='A')).hexdigest()}")
            tape = (P if loop == "pd" else 2) * K * 8 * int(np.prod(shape))
            fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"   # noqa: E731
            lines.append(f"{name:40s} {K:3d} {fmt(fwd):>28s} {fmt(nat):>28s} {fmt(com):>30s} {com[0] / nat[0]:11.2f} {tape / 1e6:9.1f} {diff:9.2e}")
            lines.append("#   d/dlambda native (" + ", ".join(f"{v:.12e}" for v in glam) + "), composed (" + ", ".join(f"{v:.12e}" for v in cl) + ")")
            del cx, gx
            torch.cuda.empty_cache()
    lines += prints
    if args.compare_with:
        with open(args.compare_with) as fh:
            before = [ln.strip() for ln in fh if ln.startswith("# gy sha1")]
        lines.append("# a second run of this tool, in another process, gave " + ("identical gy (same sha1 per case)" if before == prints else "DIFFERENT gy"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
