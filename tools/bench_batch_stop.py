#!/usr/bin/env python3
"""A stack of independent images whose solvers have a tolerance: (a)
PrimalDualBatch(solvers) as it is by default -- every solver with a tolerance runs on
its own, one after the other, with one read-back per check -- against (b)
PrimalDualBatch(solvers, stacked_stopping=True), one launch per iteration over the
members still running and one read-back per check for the whole group; in the same
process, alternated, one warm-up, median of 5 with the spread; device events around the
whole job including its set-up.

float32 TV-l2, at most 200 iterations, check_every 10, on stacks 256^2 x {16, 64, 256}
and 128^3 x 16 of the inputs of bench_batch.py.  The members' tolerances are spread
geometrically from 3e-2 to 3e-4 over the stack, so that they stop at different checks;
the iterations every member did are reported (the two forms must agree).  One JSON
line per case.  Nothing gates on it.
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
from bench_batch import images  # noqa: E402
from bench_sweep import stats, timed  # noqa: E402

CASES = [("256^2", (256, 256), 16), ("256^2", (256, 256), 64),
         ("256^2", (256, 256), 256), ("128^3", (128,) * 3, 16)]


def tolerances(P, hi=3e-2, lo=3e-4):
    return [float(t) for t in np.geomspace(hi, lo, P)]


def run(imgs, tols, iters, every, L2, stacked_stopping):
    solvers = [build_solver(o, "TVL2", 0.03, iters, L2=L2, dtype=np.float32,
                            tolerance=t, check_every=every)
               for o, t in zip(imgs, tols)]
    b = PrimalDualBatch(solvers, stacked_stopping=stacked_stopping)
    b.run()
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--check-every", type=int, default=10)
    ap.add_argument("--cases", nargs="+", default=None,
                    help="e.g. 256^2x64 128^3x16 (default: all)")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_batch_stop.py needs a HIP device"
    for name, shape, P in CASES:
        tag = "%sx%d" % (name, P)
        if args.cases is not None and tag not in args.cases:
            continue
        imgs, tols = images(shape, P), tolerances(P)
        L2 = 8.0 if len(shape) == 2 else 16.0
        variants = {"sequential": False, "stacked": True}
        times = {k: [] for k in variants}
        info = {}
        for r in range(args.reps + 1):           # the first round warms up
            for key, flag in variants.items():
                before = (ops.pd_stack_launches(), ops.pd_check_launches())
                t, b = timed(lambda: run(imgs, tols, args.iterations, args.check_every,
                                         L2, flag))
                if r:
                    times[key].append(t)
                done = [s.get_iterations_done() for s in b.get_solvers()]
                info[key] = {
                    "stack_kernel_launches": ops.pd_stack_launches() - before[0],
                    "check_launches": ops.pd_check_launches() - before[1],
                    "stacked": b.get_execution().count("stacked"),
                    "G": b.get_group_size(), "iterations_done": done}
                del b
        res = {k: dict(stats(v), **info[k]) for k, v in times.items()}
        done = res["stacked"]["iterations_done"]
        row = {"bench": "batch_stop", "case": tag, "members": P, "dtype": "float32",
               "iterations": args.iterations, "check_every": args.check_every,
               "tolerances": [tols[0], tols[-1]],
               "same_iterations": done == res["sequential"]["iterations_done"],
               "distinct_stops": len(set(done)), "stops_min_max": [min(done), max(done)],
               "speedup_stacked_over_sequential":
                   res["sequential"]["median_s"] / res["stacked"]["median_s"],
               "timing": "device events around the whole job incl. set-up, "
                         "alternated, 1 warm-up + median of %d" % args.reps}
        for k in res:
            res[k].pop("iterations_done")
        row.update(res)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
