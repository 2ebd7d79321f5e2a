#!/usr/bin/env python3
"""Time and memory of the two tapes of the solver derivatives: tape = "outputs" (every sweep output kept as float64) against
tape = "steps" (2-bit step codes, each sweep output encoded behind its sweep) for device.dr2_vjp and device.tvgen_vjp, and the fibre
derivative from y (device.tv1_fibres_vjp) against encode + derivative from words (device.tv1_fibres_steps + tv1_fibres_vjp_steps).
Same process, the two tapes ALTERNATING call by call, torch.cuda.Event pairs on the stream they run on, 3 warm-ups each, median of 20,
whole calls (each ends in a stream synchronise).  Also: the tape bytes of both (the figure the C-ABI holds against the pool's cap) and
the sha1 of the gradients of both -- they must be the same bits.

    python tools/vjp_tape_time.py [--out profiles/vjp_tape_time.txt]
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

DR_CASES = [("DR 1024 x 1024, lambda 0.1", (1024, 1024), 0.1), ("DR 4096 x 4096, lambda 0.1", (4096, 4096), 0.1)]
PD_CASES = [("pd 512 x 512 x 64, 3 terms, lambda 0.1", (512, 512, 64), (1, 2, 3), "pd", 0.1),
            ("pd2 4096 x 4096, lambda 0.1", (4096, 4096), (1, 2), "pd2", 0.1)]
FIBRE_CASES = [("fibres 4096 x 4096, dim 0, lambda 0.1", (4096, 4096), 0, 0.1), ("fibres 4096 x 4096, dim 1, lambda 0.1", (4096, 4096), 1, 0.1),
               ("fibres 512 x 512 x 64, dim 2, lambda 0.1", (512, 512, 64), 2, 0.1)]
MAXIT, WARMUP, REPS = 35, 3, 20


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fa, fb, stream):
    """(median, min, max) in ms of each of two calls, run a, b, a, b, ..."""
    for _ in range(WARMUP):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(REPS):
        ta.append(timed(fa, stream))
        tb.append(timed(fb, stream))
    return tuple((statistics.median(t), min(t), max(t)) for t in (ta, tb))


def sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(a.cpu().numpy().tobytes(order="A") if isinstance(a, torch.Tensor) else np.asarray(a).tobytes())
    return h.hexdigest()


def words(lib, shape, dim):
    ns = np.array(shape, dtype=np.int32)
    return lib.proxtv_tv1_steps_words(ns.ctypes.data, len(shape), dim)


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def draw(shape):
    rng = np.random.default_rng(0)
    up = lambda a: device.to_colmajor(torch.from_numpy(a).cuda())   # noqa: E731
    return up(rng.standard_normal(shape)), up(rng.standard_normal(shape))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.require_device()
    stream = torch.cuda.Stream()
    lines = [f"# tools/vjp_tape_time.py, build {build.build_id()}, {torch.cuda.get_device_name(0)}",
             f"# median (min .. max) of {REPS} calls after {WARMUP} warm-ups, torch.cuda.Event on the calls' stream; the two columns alternate call by call",
             "# solvers: whole device.dr2_vjp / device.tvgen_vjp calls (unfused forward + tape + reverse), gradients in x and every penalty",
             f"{'case':40s} {'K':>3s} {'tape=outputs ms':>28s} {'tape=steps ms':>28s} {'steps/outputs':>13s} {'outputs MB':>11s} {'steps MB':>9s} same bits"]
    prints = []
    with torch.cuda.stream(stream):
        for name, shape, lam in DR_CASES:
            x, g = draw(shape)
            torch.cuda.synchronize()
            call = lambda tape: device.dr2_vjp(x, g, lam, lam, MAXIT, need_gw="sums", need_y=True, tape=tape)   # noqa: E731
            t0, t1 = alternate(lambda: call("outputs"), lambda: call("steps"), stream)
            a, b = call("outputs"), call("steps")
            sa, sb = sha(a[0], a[4], a[3]), sha(b[0], b[4], b[3])
            n = shape[0] * shape[1]
            b0 = 2 * (MAXIT + 1) * 8 * n
            b1 = (MAXIT + 1) * 4 * (words(lib, shape, 0) + words(lib, shape, 1)) + 2 * 8 * n
            lines.append(f"{name:40s} {MAXIT:3d} {fmt(t0):>28s} {fmt(t1):>28s} {t1[0] / t0[0]:13.3f} {b0 / 1e6:11.1f} {b1 / 1e6:9.1f} {sa == sb}")
            prints.append(f"# gx, s, glam sha1 [{name}] outputs {sa} steps {sb}")
            del a, b
            torch.cuda.empty_cache()
        for name, shape, ds, loop, lam in PD_CASES:
            x, g = draw(shape)
            P = len(ds)
            ws = [lam] * P
            torch.cuda.synchronize()
            K = int(device.tvgen(x, ws, ds, 0, loop)[1][0])
            call = lambda tape: device.tvgen_vjp(x, g, ws, ds, K, loop, need_glam=True, need_y=True, tape=tape)   # noqa: E731
            t0, t1 = alternate(lambda: call("outputs"), lambda: call("steps"), stream)
            a, b = call("outputs"), call("steps")
            sa, sb = sha(a[0], a[2], a[1]), sha(b[0], b[2], b[1])
            n = int(np.prod(shape))
            b0 = P * K * 8 * n
            b1 = K * 4 * sum(words(lib, shape, d - 1) for d in ds) + P * 8 * n
            lines.append(f"{name:40s} {K:3d} {fmt(t0):>28s} {fmt(t1):>28s} {t1[0] / t0[0]:13.3f} {b0 / 1e6:11.1f} {b1 / 1e6:9.1f} {sa == sb}")
            prints.append(f"# gx, y, glam sha1 [{name}] outputs {sa} steps {sb}")
            del a, b
            torch.cuda.empty_cache()
        lines.append("# the fibre derivative, gx and gw: from y | encode y, then from the words | from the words alone (the encode paid elsewhere)")
        lines.append(f"{'case':40s} {'from y ms':>28s} {'encode + from words ms':>28s} {'from words ms':>28s} {'encode ms':>28s} same bits")
        for name, shape, dim, lam in FIBRE_CASES:
            x, g = draw(shape)
            y = device.tv1_fibres(x, lam, dim)
            gx = device.colmajor_empty(shape)
            steps = device.tv1_fibres_steps(y, dim)
            torch.cuda.synchronize()
            from_y = lambda: device.tv1_fibres_vjp(y, g, dim, need_gw=True, out=gx)                                       # noqa: E731
            from_w = lambda: device.tv1_fibres_vjp_steps(steps, g, shape, dim, need_gw=True, out=gx)                       # noqa: E731
            both = lambda: device.tv1_fibres_vjp_steps(device.tv1_fibres_steps(y, dim), g, shape, dim, need_gw=True, out=gx)   # noqa: E731
            t0, t1 = alternate(from_y, both, stream)
            t2, t3 = alternate(from_w, lambda: device.tv1_fibres_steps(y, dim), stream)
            a = from_y()
            sa = sha(a[0], a[1])
            b = both()
            sb = sha(b[0], b[1])
            lines.append(f"{name:40s} {fmt(t0):>28s} {fmt(t1):>28s} {fmt(t2):>28s} {fmt(t3):>28s} {sa == sb}")
            prints.append(f"# gx, gw sha1 [{name}] from y {sa} from words {sb}")
            torch.cuda.empty_cache()
    lines += prints
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
