#!/usr/bin/env python3
"""Time of the native derivative of the 2-D Douglas-Rachford solve (device.dr2_vjp: forward recurrence with its tape, then the reverse
sweeps) against (a) the fused forward solve alone (device.tv1_2d) and (b) the same recurrence composed in torch from
autograd.tv1_fibres, forward and backward -- what a user had to write before, and code that predates the native call.  Same process,
torch.cuda.Event pairs on the stream all of them run on, 3 warm-ups, median of 20, whole calls (each ends in a stream synchronise).
Gradients asked for: x and both uniform penalties, in (b) as 0-d tensors.  Also: the peak tape bytes, the largest difference between
the two gradients, and a fingerprint of the native call's outputs (--compare-with: the file of an earlier run, to state whether two
runs gave the same bits).

    python tools/dr_vjp_time.py [--out profiles/dr_vjp_time.txt] [--compare-with earlier.txt]
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

import dr_vjp_model as dm  # noqa: E402   (compose: the composition tests/test_gpu_dr_vjp.py checks the native call against)
from proxtv_amd import _lib, autograd, build, device  # noqa: E402

CASES = [("1024 x 1024 Gaussian, lambda 0.1", (1024, 1024), 0.1),
         ("4096 x 4096 Gaussian, lambda 0.1", (4096, 4096), 0.1),
         ("4096 x 4096 Gaussian, lambda 1", (4096, 4096), 1.0)]
MAXIT = 35


def median_ms(fn, stream, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare-with", default=None)
    args = ap.parse_args()
    _lib.require_device()
    stream = torch.cuda.Stream()
    lines = [f"# tools/dr_vjp_time.py, build {build.build_id()}, {torch.cuda.get_device_name(0)}",
             f"# median (min .. max) of 20 calls after 3 warm-ups, torch.cuda.Event on the calls' stream; {MAXIT} iterations, gradients in x and both penalties",
             "# forward: device.tv1_2d (fused) | native: device.dr2_vjp (unfused forward + tape + reverse) | composed: autograd.tv1_fibres x 72 + torch, forward + backward",
             f"{'case':34s} {'forward ms':>26s} {'native ms':>26s} {'composed ms':>30s} {'comp/native':>11s} {'tape MB':>9s} {'|d gx|':>9s}"]
    prints = []
    with torch.cuda.stream(stream):
        for name, shape, lam in CASES:
            rng = np.random.default_rng(0)
            x = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            g = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            y = device.colmajor_empty(shape)
            torch.cuda.synchronize()

            def composed():
                xt = x.detach().requires_grad_(True)
                w1, w2 = (torch.tensor(lam, dtype=torch.float64, device="cuda", requires_grad=True) for _ in range(2))
                (g * dm.compose(torch, autograd, xt, w1, w2, MAXIT)).sum().backward()
                return xt.grad, w1.grad, w2.grad

            fwd = median_ms(lambda: device.tv1_2d(x, lam, MAXIT, out=y), stream)
            nat = median_ms(lambda: device.dr2_vjp(x, g, lam, lam, MAXIT, need_gw="sums"), stream)
            com = median_ms(composed, stream)
            gx, _, _, glam, s = device.dr2_vjp(x, g, lam, lam, MAXIT, need_gw="sums", need_y=True)
            cx, c1, c2 = composed()
            diff = float((gx - cx).abs().max())
            h = hashlib.sha1()
            for a in (gx, s):
                h.update(a.cpu().numpy().tobytes(order="A"))
            h.update(glam.tobytes())
            prints.append(f"# outputs sha1 [{name}] {h.hexdigest()}")
            tape = 2 * (MAXIT + 1) * 8 * shape[0] * shape[1]
            fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"   # noqa: E731
            lines.append(f"{name:34s} {fmt(fwd):>26s} {fmt(nat):>26s} {fmt(com):>30s} {com[0] / nat[0]:11.2f} {tape / 1e6:9.1f} {diff:9.2e}")
            lines.append(f"#   d/dlambda native ({glam[0]:.12e}, {glam[1]:.12e}), composed ({float(c1):.12e}, {float(c2):.12e})")
            del cx, gx, s
            torch.cuda.empty_cache()
    lines += prints
    if args.compare_with:
        with open(args.compare_with) as fh:
            before = [ln.strip() for ln in fh if ln.startswith("# outputs sha1")]
        lines.append("# a second run of this tool, in another process, gave " +
                     ("identical outputs (same sha1 per case)" if before == prints else "DIFFERENT outputs"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
