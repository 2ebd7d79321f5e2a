#!/usr/bin/env python3
"""Time of the solver derivatives with general-p TV-Lp terms (option general_p_vjp).  Whole calls, torch.cuda.Event pairs on
the stream they run on, 3 warm-ups, median of 10 (min .. max).  Every step runs in a child process of its own under its own time limit;
a step that fails or runs out of time ends the run.

(a) One reverse sweep, fused against epilogue route (option tvp_vjp_route = 1 / 2).  No entry point runs a write-out mode alone, so the
    step times the smallest call that contains one: the parallel Dykstra derivative with one term and one iteration -- one forward
    general-p sweep, one reverse sweep in mode PD, two copies -- under both routes, and beside it the forward sweep alone
    (device.tvp_fibres) and the plain reverse sweep alone (device.tvp_fibres_vjp).  The forward is the same kernel on the same data in
    both columns, but it costs 25 - 100 times a reverse sweep and its run-to-run spread is larger than the difference looked for.  So
    the two routes are timed in PAIRS, one call of each back to back, the order alternating, and the step reports the median of the
    per-pair differences fused - epilogue with its quartiles and its range over PAIRS pairs: slow drift cancels inside a pair, and the
    quartiles say whether the sign can be told.  The resolution stays bounded by the forward's spread.  This sets policy.hpp's threshold.
(b) Whole derivative calls against the same recurrence composed in torch from autograd.tv1_fibres / tv2_fibres / tvp_fibres (forward and
    backward of the graph): both columns hold one forward and one reverse pass.  "one call" runs under the auto rule; its medians with
    the route forced either way stand at the end of the row.

    python tools/tvpg_vjp_time.py [--out profiles/tvpg_vjp_time.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, fibres x samples as an array shape, the dimension swept)
SWEEPS = [("4096 x 4096", (4096, 4096), 1), ("16384 x 1024", (16384, 1024), 1), ("262144 x 64", (512, 512, 64), 2)]
SWEEP_PS = (1.5, 3.0)
DR_CASES = [((1024, 1024), (1, 1.5), 5), ((1024, 1024), (3, 1.5), 5)]
PD_CASES = [("pd", (512, 512, 64), (1, 2, 3), (1, 1, 1.5), 3)]
STEP_LIMIT = 240     # seconds per step
REPS = 10
PAIRS = 40           # (a): pairs of calls, fused and epilogue back to back


def steps():
    out = [f"sweep:{i}:{p}" for i in range(len(SWEEPS)) for p in SWEEP_PS]
    out += [f"dr:{i}" for i in range(len(DR_CASES))] + [f"pd:{i}" for i in range(len(PD_CASES))]
    return out


def run_step(step):
    import numpy as np
    import torch

    import tvpg_vjp_model as gm
    from proxtv_amd import _lib, autograd, device

    lib = _lib.require_device()
    lib.proxtv_set_option(b"general_p_vjp", 1)
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    up = lambda shape: device.to_colmajor(torch.from_numpy(rng.standard_normal(shape)).cuda())   # noqa: E731

    def median_ms(fn, warmup=3, reps=REPS):
        with torch.cuda.stream(stream):
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
        return f"{statistics.median(times):10.3f} ({min(times):.3f} .. {max(times):.3f})", statistics.median(times)

    def by_route(fn):
        """The call under the auto rule, and its medians with the route forced (fused wherever legal / epilogue everywhere)."""
        native, tn = median_ms(fn)
        forced = []
        for route in (1, 2):
            lib.proxtv_set_option(b"tvp_vjp_route", route)
            forced.append(median_ms(fn)[1])
        lib.proxtv_set_option(b"tvp_vjp_route", 0)
        return native, tn, f"one call, fused wherever legal {forced[0]:.3f}, epilogue everywhere {forced[1]:.3f}"

    kind, *rest = step.split(":")
    if kind == "sweep":
        name, shape, dim = SWEEPS[int(rest[0])]
        p, w = float(rest[1]), 0.3
        x, g = up(shape), up(shape)
        y = device.tvp_fibres(x, w, p, dim)
        fwd, _ = median_ms(lambda: device.tvp_fibres(x, w, p, dim))
        plain, _ = median_ms(lambda: device.tvp_fibres_vjp(y, g, w, p, dim))
        call = lambda: device.tvgen_vjp(x, g, (w,), (dim + 1,), 1, "pd", ps=(p,))   # noqa: E731

        def timed(route):
            lib.proxtv_set_option(b"tvp_vjp_route", route)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        times, diffs = {1: [], 2: []}, []
        with torch.cuda.stream(stream):
            for route in (1, 2, 1, 2):      # warm-up
                timed(route)
            for k in range(PAIRS):
                pair = {}
                for route in ((1, 2) if k % 2 == 0 else (2, 1)):
                    pair[route] = timed(route)
                    times[route].append(pair[route])
                diffs.append(pair[1] - pair[2])
        lib.proxtv_set_option(b"tvp_vjp_route", 0)
        q = statistics.quantiles(diffs, n=4)
        col = lambda t: f"{statistics.median(t):9.3f} ({min(t):.3f} .. {max(t):.3f})"   # noqa: E731
        print(f"(a) {name:>13} p {p:3.1f} | forward {fwd} | plain vjp {plain} | call, fused {col(times[1])} | call, epilogue {col(times[2])} | "
              f"fused - epilogue over {PAIRS} pairs: median {q[1]:+7.3f}, quartiles {q[0]:+7.3f} .. {q[2]:+7.3f}, range {min(diffs):+7.3f} .. "
              f"{max(diffs):+7.3f} ms")
        return
    if kind == "dr":
        shape, ps, maxit = DR_CASES[int(rest[0])]
        x, g = up(shape), up(shape)
        native, tn, forced = by_route(lambda: device.dr2_vjp(x, g, 0.3, 0.25, maxit, need_gw="sums", p_col=ps[0], p_row=ps[1]))

        def composed():
            U = x.clone().requires_grad_(True)
            ws = [torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for v in (0.3, 0.25)]
            (g * gm.dr_compose(torch, autograd, U, ws[0], ws[1], ps[0], ps[1], maxit)).sum().backward()

        comp, tc = median_ms(composed)
        print(f"(b) dr {shape} p {ps} maxit {maxit} | one call {native} | composition {comp} | ratio {tn / tc:.3f} | {forced}")
        return
    loop, shape, dims, ps, K = PD_CASES[int(rest[0])]
    P = len(dims)
    ws = tuple(0.3 / P for _ in dims)
    x, g = up(shape), up(shape)
    native, tn, forced = by_route(lambda: device.tvgen_vjp(x, g, ws, dims, K, loop, need_glam=True, ps=ps))

    def composed():
        yc = x.clone().requires_grad_(True)
        wt = [torch.tensor(w * P, dtype=torch.float64, device="cuda", requires_grad=True) for w in ws]
        (g * gm.pd_compose(torch, autograd, loop, yc, wt, dims, ps, K)).sum().backward()

    comp, tc = median_ms(composed)
    print(f"(b) {loop} {shape} dims {dims} p {ps} K {K} | one call {native} | composition {comp} | ratio {tn / tc:.3f} | {forced}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return 0
    from proxtv_amd import build
    lines = [f"# tools/tvpg_vjp_time.py, build {build.build_id()}; ms, median of {REPS} (min .. max), whole calls; (a): the two routes in "
             f"{PAIRS} alternating pairs"]
    rc = 0
    for step in steps():
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            lines.append(f"# step {step}: no result within {STEP_LIMIT} s -- the run ends here")
            rc = 1
            break
        lines.extend(line for line in r.stdout.splitlines() if line.startswith("("))
        print(lines[-1], flush=True)
        if r.returncode != 0:
            lines.append(f"# step {step}: exit status {r.returncode} -- the run ends here\n# " + r.stderr[-600:].replace("\n", "\n# "))
            rc = 1
            break
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
