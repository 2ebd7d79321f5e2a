#!/usr/bin/env python3
"""Time of the general-p TV-Lp prox derivative (device.tvp_fibres_vjp) against the forward solve (device.tvp_fibres) on the same array,
dim, penalty and p, in the same process.  torch.cuda.Event pairs on the stream both calls run on, 2 warm-ups, median of 10 (the forward
takes 0.1 - 0.2 s a call).  Both are whole calls: they end in the library's stream synchronise, so launch and synchronise latency is
inside both columns.  The derivative makes four passes over a fibre (largest jump, the p-norm, elimination, substitution), the forward
30 - 100.

    python tools/tvp_fibres_vjp_time.py [--out profiles/tvp_fibres_vjp_time.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from proxtv_amd import _lib, build, device  # noqa: E402

CASES = [(f"4096 x 4096 Gaussian, dim {dim}, lambda 0.1, p {p}", (4096, 4096), dim, 0.1, p) for p in (1.5, 3.0) for dim in (0, 1)]


def median_ms(fn, stream, warmup=2, reps=10):
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
    args = ap.parse_args()
    _lib.require_device()
    stream = torch.cuda.Stream()
    lines = [f"# tools/tvp_fibres_vjp_time.py, build {build.build_id()}, {torch.cuda.get_device_name(0)}",
             "# median (min .. max) of 10 calls after 2 warm-ups, torch.cuda.Event on the calls' stream",
             f"{'case':50s} {'forward ms':>30s} {'vjp ms':>26s} {'vjp+glam ms':>26s} {'vjp/fwd':>8s} {'iterative':>9s}"]
    with torch.cuda.stream(stream):
        for name, shape, dim, lam, p in CASES:
            rng = np.random.default_rng(0)
            x = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            g = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            y, gx = device.colmajor_empty(shape), device.colmajor_empty(shape)
            torch.cuda.synchronize()
            device.tvp_fibres(x, lam, p, dim, out=y)
            fwd = median_ms(lambda: device.tvp_fibres(x, lam, p, dim, out=y), stream)
            vjp = median_ms(lambda: device.tvp_fibres_vjp(y, g, lam, p, dim, out=gx), stream)
            full = median_ms(lambda: device.tvp_fibres_vjp(y, g, lam, p, dim, need_glam=True, out=gx), stream)
            moving = float((torch.diff(y, dim=dim).abs().amax(dim=dim) > 0).double().mean())
            fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"   # noqa: E731
            lines.append(f"{name:50s} {fmt(fwd):>30s} {fmt(vjp):>26s} {fmt(full):>26s} {vjp[0] / fwd[0]:8.4f} {moving:9.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
