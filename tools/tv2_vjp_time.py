#!/usr/bin/env python3
"""Time of the TV-L2 prox derivative (device.tv2_fibres_vjp) against the forward solve (device.tv2_fibres) on the same array, dim and
penalty, in the same process.  torch.cuda.Event pairs on the stream both calls run on, 3 warm-ups, median of 20.  Both are whole calls:
they end in the library's stream synchronise, so launch and synchronise latency is inside both columns.  TB/s counts the 24 bytes per
sample the derivative needs algorithmically (y and g read once, gx written once); the two-pass kernel moves up to 72 (zh, zq and the
reciprocal pivots out and back; of the pivots only the stretch before their fixed point).

    python tools/tv2_vjp_time.py [--out profiles/tv2_vjp_time.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from proxtv_amd import _lib, build, device  # noqa: E402

CASES = [("4096 x 4096 Gaussian, dim 0, lambda 0.1", (4096, 4096), 0, 0.1),
         ("4096 x 4096 Gaussian, dim 0, lambda 10", (4096, 4096), 0, 10.0),
         ("4096 x 4096 Gaussian, dim 1, lambda 0.1", (4096, 4096), 1, 0.1),
         ("4096 x 4096 Gaussian, dim 1, lambda 10", (4096, 4096), 1, 10.0),
         ("512 x 512 x 64 Gaussian, dim 2, lambda 0.1", (512, 512, 64), 2, 0.1),
         ("one fibre of 10^6 samples, lambda 0.5", (1000000,), 0, 0.5)]


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
    args = ap.parse_args()
    _lib.require_device()
    stream = torch.cuda.Stream()
    lines = [f"# tools/tv2_vjp_time.py, build {build.build_id()}, {torch.cuda.get_device_name(0)}",
             "# median (min .. max) of 20 calls after 3 warm-ups, torch.cuda.Event on the calls' stream; TB/s = 24 B/sample over the median",
             f"{'case':44s} {'forward+mu ms':>26s} {'vjp ms':>26s} {'vjp+glam ms':>26s} {'vjp/fwd':>8s} {'TB/s':>6s} {'active':>7s}"]
    with torch.cuda.stream(stream):
        for name, shape, dim, lam in CASES:
            rng = np.random.default_rng(0)
            x = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            g = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            y, gx = device.colmajor_empty(shape), device.colmajor_empty(shape)
            torch.cuda.synchronize()
            _, mu = device.tv2_fibres(x, lam, dim, out=y, return_mu=True)
            fwd = median_ms(lambda: device.tv2_fibres(x, lam, dim, out=y, return_mu=True), stream)
            vjp = median_ms(lambda: device.tv2_fibres_vjp(y, mu, g, lam, dim, out=gx), stream)
            full = median_ms(lambda: device.tv2_fibres_vjp(y, mu, g, lam, dim, need_glam=True, out=gx), stream)
            fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"   # noqa: E731
            lines.append(f"{name:44s} {fmt(fwd):>26s} {fmt(vjp):>26s} {fmt(full):>26s} {vjp[0] / fwd[0]:8.3f} "
                         f"{24.0 * x.numel() / (vjp[0] * 1e-3) / 1e12:6.3f} {float((mu > 0).double().mean()):7.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
