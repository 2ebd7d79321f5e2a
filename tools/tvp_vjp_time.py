#!/usr/bin/env python3
"""Time of the solver derivatives with TV-L2 terms (device.dr2_vjp(p_col=, p_row=), device.tvgen_vjp(ps=)) against the same recurrence
composed in torch from autograd.tv1_fibres / autograd.tv2_fibres (forward and backward of the graph), in the same process.
torch.cuda.Event pairs on the stream both run on, 3 warm-ups, median of 20.  Both columns are whole calls: the native one replays the
forward recurrence itself, so both contain one forward and one reverse pass.

    python tools/tvp_vjp_time.py [--out profiles/tvp_vjp_time.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import torch  # noqa: E402

import tvp_vjp_model as tp  # noqa: E402  (the compositions the tests compare against)
from proxtv_amd import _lib, autograd, build, device  # noqa: E402

MAXIT = 5
DR_CASES = [((1024, 1024), (1, 2)), ((1024, 1024), (2, 2)), ((4096, 4096), (1, 2)), ((4096, 4096), (2, 2))]
PD_CASES = [("pd", (512, 512, 64), (1, 2, 3), (1, 1, 2), 3)]


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
    fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"   # noqa: E731
    lines = [f"# tools/tvp_vjp_time.py, build {build.build_id()}, {torch.cuda.get_device_name(0)}",
             "# median (min .. max) of 20 calls after 3 warm-ups, torch.cuda.Event on the calls' stream; gradients in x and in every penalty",
             f"{'case':58s} {'native ms':>30s} {'native, steps tape ms':>30s} {'composed in torch ms':>30s} {'speed-up':>9s}"]
    with torch.cuda.stream(stream):
        for shape, ps in DR_CASES:
            rng = np.random.default_rng(0)
            x = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            g = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            torch.cuda.synchronize()

            def native(tape="outputs"):
                device.dr2_vjp(x, g, 0.3, 0.25, MAXIT, need_gw="sums", tape=tape, p_col=ps[0], p_row=ps[1])

            def composed():
                xt = x.clone().requires_grad_(True)
                ws = [torch.tensor(w, dtype=torch.float64, device="cuda", requires_grad=True) for w in (0.3, 0.25)]
                (g * tp.dr_compose(torch, autograd, xt, ws[0], ws[1], ps[0], ps[1], MAXIT)).sum().backward()

            a, b, c = median_ms(native, stream), median_ms(lambda: native("steps"), stream), median_ms(composed, stream)
            lines.append(f"{f'DR {shape[0]} x {shape[1]} Gaussian, p = {ps}, {MAXIT} iterations':58s} {fmt(a):>30s} {fmt(b):>30s} {fmt(c):>30s} "
                         f"{c[0] / a[0]:9.2f}")
            print(lines[-1], flush=True)
        for loop, shape, dims, ps, K in PD_CASES:
            rng = np.random.default_rng(0)
            x = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            g = device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())
            ws = tuple(0.3 / len(dims) for _ in dims)
            torch.cuda.synchronize()

            def native(tape="outputs"):
                device.tvgen_vjp(x, g, ws, dims, K, loop, need_glam=True, tape=tape, ps=ps)

            def composed():
                xt = x.clone().requires_grad_(True)
                wt = [torch.tensor(w * len(dims), dtype=torch.float64, device="cuda", requires_grad=True) for w in ws]
                (g * tp.pd_compose(torch, autograd, loop, xt, wt, dims, ps, K)).sum().backward()

            a, b, c = median_ms(native, stream), median_ms(lambda: native("steps"), stream), median_ms(composed, stream)
            name = f"{loop} {' x '.join(map(str, shape))} Gaussian, ps = {list(ps)}, {K} iterations"
            lines.append(f"{name:58s} {fmt(a):>30s} {fmt(b):>30s} {fmt(c):>30s} {c[0] / a[0]:9.2f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
