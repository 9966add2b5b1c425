#!/usr/bin/env python3
"""A sweep over alpha on one observation: (a) the loop the command-line tool ran
before the sweep existed -- one PrimalDualSolver per alpha, persistent kernel
enabled as by default -- against (b) PrimalDualSweep, in the same process,
alternated, warmed, median of 5 with the spread; device events around the whole
sweep including its set-up (uploads, scaling, schedules).

float32 TV-l2, 100 iterations, P in {4, 16, 64} alphas log-spaced in [1e-3, 1] on
256^2, 1024^2, 64^3, 128^3 and 256^3 synth_volume-style inputs.  Prints one JSON
line.  --explore additionally times the stacked form where the constants of
ops.py would choose the sequential one (and the other way round) and several
group budgets: the measurement ops.PD_SWEEP_MAX_VOXELS / PD_SWEEP_GROUP_BYTES are
set from.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from nsol_amd import ops  # noqa: E402
from nsol_amd.application.run_denoising import build_solver, wiring  # noqa: E402
from nsol_amd.parameter_sweep import PrimalDualSweep  # noqa: E402
from nsol_amd.synthetic import synth_volume  # noqa: E402

CASES = [("256^2", (256, 256)), ("1024^2", (1024, 1024)), ("64^3", (64,) * 3),
         ("128^3", (128,) * 3), ("256^3", (256,) * 3)]


def observation(shape, seed=0):
    """synth_volume for cubes; its central slice pattern, tiled, for images."""
    if len(shape) == 3:
        return synth_volume(shape[0], seed=seed)
    n = shape[0]
    q = max(n // 4, 1)
    i = np.arange(n)
    blk = i // q
    v = 100.0 * ((blk[:, None] + blk[None, :]) % 2).astype(np.float64)
    r2 = (i - n / 2.0) ** 2
    v += 50.0 * ((r2[:, None] + r2[None, :]) < (n / 3.0) ** 2)
    rng = np.random.default_rng(seed)
    return v + 0.05 * v.max() * rng.standard_normal(v.shape)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def loop(obs, alphas, iters, L2):
    last = None
    for a in alphas:
        s = build_solver(obs, "TVL2", a, iters, L2=L2, dtype=np.float32)
        s.run()
        last = s
    return last


def sweep(obs, alphas, iters, L2):
    s = PrimalDualSweep(L2=L2, parameters={"alpha": list(alphas)}, iterations=iters,
                        dtype=np.float32, **wiring(obs, "TVL2"))
    s.run()
    return s


def stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1]}


def measure(obs, alphas, iters, L2, reps, variants):
    """variants: {name: callable}; alternated, one warm-up round first."""
    times = {k: [] for k in variants}
    info = {}
    for r in range(reps + 1):
        for name, fn in variants.items():
            before = (ops.pd_sweep_launches(), ops.pd_persist_launches())
            t, out = timed(fn)
            if r:
                times[name].append(t)
            info[name] = {
                "sweep_kernel_launches": ops.pd_sweep_launches() - before[0],
                "persistent_runs": ops.pd_persist_launches() - before[1],
                "execution": out.get_execution()}
            if isinstance(out, PrimalDualSweep):
                info[name]["G"] = out.get_group_size()
            del out
    return {k: dict(stats(v), **info[k]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--members", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--cases", nargs="+", default=[c[0] for c in CASES])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--explore", action="store_true")
    ap.add_argument("--budgets-mb", type=int, nargs="+", default=[256, 1024, 4096])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sweep.py needs a HIP device"
    max_vox, budget = ops.PD_SWEEP_MAX_VOXELS, ops.PD_SWEEP_GROUP_BYTES
    results = []
    for name, shape in CASES:
        if name not in args.cases:
            continue
        obs = observation(shape)
        L2 = 8.0 if len(shape) == 2 else 16.0
        for P in args.members:
            alphas = np.logspace(-3, 0, P)

            def with_constants(mv, gb):
                def run():
                    ops.PD_SWEEP_MAX_VOXELS, ops.PD_SWEEP_GROUP_BYTES = mv, gb
                    try:
                        return sweep(obs, alphas, args.iterations, L2)
                    finally:
                        ops.PD_SWEEP_MAX_VOXELS = max_vox
                        ops.PD_SWEEP_GROUP_BYTES = budget
                return run
            variants = {"loop": lambda: loop(obs, alphas, args.iterations, L2),
                        "sweep": with_constants(max_vox, budget)}
            if args.explore:
                for mb in args.budgets_mb:
                    variants["stacked_%dMB" % mb] = with_constants(1 << 40, mb << 20)
            r = measure(obs, alphas, args.iterations, L2, args.reps, variants)
            spread = max(v["max_s"] - v["min_s"] for v in r.values())
            row = {"case": name, "members": P, "iterations": args.iterations,
                   "loop_launches_if_one_per_iteration": P * args.iterations,
                   "speedup_sweep_over_loop":
                       r["loop"]["median_s"] / r["sweep"]["median_s"],
                   "spread_s": spread}
            row.update(r)
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps({
        "bench": "sweep", "dtype": "float32", "workload": "TV-l2 alpha sweep",
        "PD_SWEEP_MAX_VOXELS": max_vox, "PD_SWEEP_GROUP_BYTES": budget,
        "timing": "device events around the whole sweep incl. set-up, "
                  "alternated, 1 warm-up + median of %d" % args.reps,
        "results": results}))


if __name__ == "__main__":
    main()
