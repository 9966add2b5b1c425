#!/usr/bin/env python3
"""A stack of independent images of one shape: (a) the loop users write today --
one PrimalDualSolver per image, persistent kernel enabled as by default --
against (b) PrimalDualBatch on the same list of solvers, in the same process,
alternated, warmed, median of 5 with the spread; device events around the whole
job including its set-up (building the solvers, uploads, scaling, schedules).

float32 TV-l2 and isotropic TV-l2, 50 iterations, on stacks 256^2 x {16, 64, 256},
1024^2 x 16, 64^3 x {4, 16} and 128^3 x 16 of synth_volume-style inputs, every
image with its own noise, level and hence x_scale.  One JSON line per case.
--explore additionally times the stacked form with several group budgets and
without the size limit: the measurement ops.PD_BATCH_GROUP_BYTES /
PD_BATCH_MAX_VOXELS are set from.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nsol_amd import ops  # noqa: E402
from nsol_amd.application.run_denoising import build_solver  # noqa: E402
from nsol_amd.solver_batch import PrimalDualBatch  # noqa: E402
from bench_sweep import observation, stats, timed  # noqa: E402

CASES = [("256^2", (256, 256), 16), ("256^2", (256, 256), 64),
         ("256^2", (256, 256), 256), ("1024^2", (1024, 1024), 16),
         ("64^3", (64,) * 3, 4), ("64^3", (64,) * 3, 16), ("128^3", (128,) * 3, 16)]


def images(shape, P):
    """P observations of one shape: the pattern of bench_sweep.py at P levels with
    P noise fields."""
    base = observation(shape)
    rng = np.random.default_rng(1)
    return [base * (1.0 + 0.1 * k) +
            0.02 * base.max() * rng.standard_normal(shape) for k in range(P)]


def solvers_of(imgs, iters, L2, iso):
    return [build_solver(o, "TVL2", 0.03, iters, L2=L2, dtype=np.float32,
                         isotropic=iso) for o in imgs]


def loop(imgs, iters, L2, iso):
    out = solvers_of(imgs, iters, L2, iso)
    for s in out:
        s.run()
    return out


def batch(imgs, iters, L2, iso):
    b = PrimalDualBatch(solvers_of(imgs, iters, L2, iso))
    b.run()
    return b


def measure(reps, variants):
    """variants: {name: callable}; alternated, one warm-up round first."""
    times = {k: [] for k in variants}
    info = {}
    for r in range(reps + 1):
        for name, fn in variants.items():
            before = (ops.pd_batch_launches(), ops.pd_persist_launches())
            t, out = timed(fn)
            if r:
                times[name].append(t)
            info[name] = {"batch_kernel_launches": ops.pd_batch_launches() - before[0],
                          "persistent_runs": ops.pd_persist_launches() - before[1]}
            if isinstance(out, PrimalDualBatch):
                ex = out.get_execution()
                info[name]["stacked"] = ex.count("stacked")
                info[name]["G"] = out.get_group_size()
            del out
    return {k: dict(stats(v), **info[k]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--cases", nargs="+", default=None,
                    help="e.g. 256^2x64 128^3x16 (default: all)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--explore", action="store_true")
    ap.add_argument("--budgets-mb", type=int, nargs="+", default=[64, 256, 1024])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_batch.py needs a HIP device"
    max_vox, budget = ops.PD_BATCH_MAX_VOXELS, ops.PD_BATCH_GROUP_BYTES
    for name, shape, P in CASES:
        tag = "%sx%d" % (name, P)
        if args.cases is not None and tag not in args.cases:
            continue
        imgs = images(shape, P)
        L2 = 8.0 if len(shape) == 2 else 16.0
        for iso in (False, True):
            def with_constants(mv, gb):
                def run():
                    ops.PD_BATCH_MAX_VOXELS, ops.PD_BATCH_GROUP_BYTES = mv, gb
                    try:
                        return batch(imgs, args.iterations, L2, iso)
                    finally:
                        ops.PD_BATCH_MAX_VOXELS = max_vox
                        ops.PD_BATCH_GROUP_BYTES = budget
                return run
            variants = {"loop": lambda: loop(imgs, args.iterations, L2, iso),
                        "batch": with_constants(max_vox, budget)}
            if args.explore:
                for mb in args.budgets_mb:
                    variants["stacked_%dMB" % mb] = with_constants(1 << 40, mb << 20)
            r = measure(args.reps, variants)
            spread = max(v["max_s"] - v["min_s"] for v in r.values())
            row = {"bench": "batch", "case": tag, "members": P,
                   "regulariser": "isotropic TV" if iso else "TV",
                   "dtype": "float32", "iterations": args.iterations,
                   "PD_BATCH_MAX_VOXELS": max_vox, "PD_BATCH_GROUP_BYTES": budget,
                   "speedup_batch_over_loop":
                       r["loop"]["median_s"] / r["batch"]["median_s"],
                   "spread_s": spread,
                   "timing": "device events around the whole job incl. set-up, "
                             "alternated, 1 warm-up + median of %d" % args.reps}
            row.update(r)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
