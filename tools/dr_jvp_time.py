#!/usr/bin/env python3
"""Time and scratch of the forward-mode derivative of the 2-D Douglas-Rachford solve (device.dr2_jvp) against the reverse-mode call on
the same data (device.dr2_vjp, both tapes), and the paired timing that decides where the row sweeps' three-array tangent is formed
(option dr_jvp_route: 1 = inside the loads of phases A and C, 2 = one pointwise pass in front).

Whole calls (each ends in a stream synchronise), torch.cuda.Event pairs on the stream they run on, 3 warm-up rounds, then `reps` rounds in
which the variants take turns on the same arrays, so that drift hits all of them alike; medians, and for the two routes the median and
quartiles of the per-round differences.  Peak pool scratch of a call: the device memory the library's pool took for it, read off
torch.cuda.mem_get_info around the first call after proxtv_release_scratch (the pool keeps what a call used, up to its cap).  The tangent
is in x and in both uniform penalties; the cotangent of the reverse call asks for the same three.

    python tools/dr_jvp_time.py [--out profiles/dr_jvp_time.txt] [--no-batch]
"""
import argparse
import hashlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from proxtv_amd import _lib, build, device  # noqa: E402

# (name, shape, lambda, rounds)
CASES = [("1024 x 1024", (1024, 1024), 0.1, 20), ("4096 x 4096", (4096, 4096), 0.1, 20), ("64 x 2048 x 2048 batch", (2048, 2048, 64), 0.1, 5)]
MAXIT = 35


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def pool_bytes(lib, fn):
    """What the library's scratch pool takes from the device for one call, starting from an empty pool."""
    lib.proxtv_release_scratch()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    out = fn()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    del out
    return before - after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-batch", action="store_true")
    args = ap.parse_args()
    lib = _lib.require_device()
    stream = torch.cuda.Stream()
    fmt = lambda ts: f"{statistics.median(ts):9.3f} ({min(ts):.3f} .. {max(ts):.3f})"   # noqa: E731
    lines = [f"# tools/dr_jvp_time.py, build {build.build_id()}, {torch.cuda.get_device_name(0)}",
             f"# whole calls, {MAXIT} iterations, lambda 0.1, unit Gaussian data; median (min .. max) ms over the rounds, the variants taking turns in every round",
             "# jvp: device.dr2_jvp (tangent in x and both uniform penalties) by route | vjp: device.dr2_vjp(need_gw='sums') by tape | scratch: pool bytes of one call"]
    with torch.cuda.stream(stream):
        for name, shape, lam, reps in CASES:
            if args.no_batch and len(shape) == 3:
                continue
            rng = np.random.default_rng(0)
            x = device.colmajor_empty(shape)
            x.copy_(torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).cuda())
            dx = device.colmajor_empty(shape)
            dx.copy_(torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).cuda())
            torch.cuda.synchronize()

            def jvp(route):
                lib.proxtv_set_option(b"dr_jvp_route", route)
                try:
                    return device.dr2_jvp(x, dx, lam, lam, MAXIT, dw_col=1.0, dw_row=1.0)[0]
                finally:
                    lib.proxtv_set_option(b"dr_jvp_route", 0)

            variants = {"jvp in loads": lambda: jvp(1), "jvp pointwise": lambda: jvp(2),
                        "vjp outputs": lambda: device.dr2_vjp(x, dx, lam, lam, MAXIT, need_gw="sums", tape="outputs")[0],
                        "vjp steps": lambda: device.dr2_vjp(x, dx, lam, lam, MAXIT, need_gw="sums", tape="steps")[0]}
            scratch, times, refused = {}, {}, {}
            for key, fn in variants.items():
                try:
                    scratch[key] = pool_bytes(lib, fn)
                    times[key] = []
                except _lib.ProxTVError as e:
                    refused[key] = str(e)
            lib.proxtv_release_scratch()
            for r in range(3 + reps):
                for key in times:
                    t = timed(variants[key], stream)
                    if r >= 3:
                        times[key].append(t)
            lines.append(f"{name}  ({reps} rounds)")
            for key in variants:
                if key in refused:
                    lines.append(f"  {key:14s} refused: {refused[key]}")
                else:
                    lines.append(f"  {key:14s} {fmt(times[key]):>34s} ms   scratch {scratch[key] / 2**20:10.1f} MiB")
            pairs = sorted(a - b for a, b in zip(times["jvp in loads"], times["jvp pointwise"]))
            q = statistics.quantiles(pairs, n=4) if len(pairs) >= 4 else [pairs[0], statistics.median(pairs), pairs[-1]]
            lines.append(f"  in loads - pointwise, per round: median {q[1]:+.3f} ms, quartiles {q[0]:+.3f} .. {q[2]:+.3f}")
            a, b = jvp(1), jvp(2)
            lines.append(f"  routes bit-identical: {bool(torch.equal(a, b))}; sha1 of ds {hashlib.sha1(a.cpu().numpy().tobytes(order='A')).hexdigest()}")
            del a, b, x, dx
            lib.proxtv_release_scratch()
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
