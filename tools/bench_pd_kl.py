#!/usr/bin/env python3
"""The Poisson (Kullback-Leibler) data term against the l2 one, in the launches of
PrimalDualLinearSolver at 256^3 float32 with the sigma = 2 Gaussian of LinearOperators3D:

(a) k_pdl_dual_data_kl (nsol_pdl_dual_data_kl_*) against k_pdl_dual_data (l2), t null as
    behind the blur's epilogue.  Both read q and bt and write q, 12 bytes per voxel; the
    KL form adds one square root and one division.
(b) one whole iteration of the solver with data_loss="kl" against "ell2": runs of ITERS
    iterations alternate inside one process, each under nsol_amd._timing.KernelTimer, so
    the figures are those of the entries as they run inside the solve; an iteration is
    the sum of its entries' durations over ITERS.

3 warm-up rounds, then the median of 5 (min - max).  One JSON line per part."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nsol_amd import _timing, linear_operators  # noqa: E402
from nsol_amd.primal_dual_linear_solver import PrimalDualLinearSolver  # noqa: E402

SHAPE = (256, 256, 256)
ITERS = 20
WARMUP, SAMPLES = 3, 5
ENTRY = {"kl": "pdl_dual_data_kl", "ell2": "pdl_dual_data"}


def summary(ts, nbytes=None):
    med, lo, hi = float(np.median(ts)), min(ts), max(ts)
    out = {"ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)]}
    if nbytes is not None:
        out["GBps"] = round(nbytes / med / 1e6, 1)
    return out


def ratio(a, b):
    """median / median, with (min / max, max / min) as its spread."""
    return {"median": round(float(np.median(a) / np.median(b)), 4),
            "min_max": [round(min(a) / max(b), 4), round(max(a) / min(b), 4)]}


def solvers(shape):
    rng = np.random.default_rng(0)
    A, _ = linear_operators.LinearOperators3D().get_gaussian_blurring_operators(
        np.diag([4.0] * 3))
    counts = rng.poisson(20.0, shape).astype(np.float64)
    A1 = lambda x: A(x.reshape(*shape)).flatten()
    b = torch.from_numpy(counts.reshape(-1)).cuda()
    kw = dict(A=A1, A_adj=A1, b=b, x0=b.to(torch.float32), dimension=3, alpha=0.05,
              iterations=ITERS, x_scale=float(counts.max()), dtype=np.float32,
              bounds=(0.0, np.inf))
    return {"kl": PrimalDualLinearSolver(data_loss="kl", background=1.0, **kw),
            "ell2": PrimalDualLinearSolver(data_loss="ell2", **kw)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--small", action="store_true",
                    help="32^3: a rehearsal of the script, not a measurement")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pd_kl needs a HIP device")
    shape = (32, 32, 32) if args.small else SHAPE
    n = int(np.prod(shape))
    runs = solvers(shape)
    kernel = {k: [] for k in runs}
    iteration = {k: [] for k in runs}
    for r in range(WARMUP + SAMPLES):
        for name, s in runs.items():
            with _timing.KernelTimer() as kt:
                s.run()
            table = kt.summary()
            if r >= WARMUP:
                kernel[name].append(table[ENTRY[name]]["avg_ms"])
                iteration[name].append(sum(e["total_ms"] for e in table.values()) / ITERS)
    common = {"shape": list(shape), "dtype": "float32", "iterations_per_run": ITERS}
    print(json.dumps(dict(common, part="dual_data", kl=summary(kernel["kl"], 12 * n),
                          ell2=summary(kernel["ell2"], 12 * n),
                          kl_over_ell2=ratio(kernel["kl"], kernel["ell2"]))), flush=True)
    print(json.dumps(dict(common, part="iteration", kl=summary(iteration["kl"]),
                          ell2=summary(iteration["ell2"]),
                          kl_over_ell2=ratio(iteration["kl"], iteration["ell2"]))),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
