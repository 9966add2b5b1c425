#!/usr/bin/env python3
"""The two kernels of a TGV iteration (k_tgv_dual, k_tgv_primal; csrc/nsol_tgv.hip)
against k_grad and k_grad_adj, which use the same thread mapping with fewer streams:
time per launch and bytes/s on each kernel's own byte model, at 1024^2, 256^3 and 512^3
float32 and 256^3 float64.  The four kernels alternate inside one process; device
events around REPS launches; 3 warm-up rounds, then the median of 5 (min - max).

Byte model, words per voxel (d = dimension, M = d (d + 1) / 2):
  k_tgv_dual    read xbar, wbar (d), p (d), q (M); write p, q        1 + 3 d + 2 M
  k_tgv_primal  read p (d), q (M), x, w (d), bt; write x, xbar, w, wbar   4 + 4 d + M
  k_grad        read x; write d                                       1 + d
  k_grad_adj    read d; write 1                                       1 + d
(3-D: 22 + 22 = 44 words per iteration, 2-D: 13 + 15 = 28.)

One JSON line per case.  --isotropic / --ell1 time those forms instead."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nsol_amd import ops  # noqa: E402

CASES = [((1024, 1024), torch.float32), ((256, 256, 256), torch.float32),
         ((512, 512, 512), torch.float32), ((256, 256, 256), torch.float64)]
REPS = 10            # launches per timed sample
WARMUP, SAMPLES = 3, 5


def words(d):
    M = d * (d + 1) // 2
    return {"tgv_dual": 1 + 3 * d + 2 * M, "tgv_primal": 4 + 4 * d + M,
            "grad": 1 + d, "grad_adj": 1 + d}


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--isotropic", action="store_true")
    ap.add_argument("--ell1", action="store_true")
    ap.add_argument("--small", action="store_true",
                    help="64^2 and 32^3 only: a rehearsal of the script, not a measurement")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tgv needs a HIP device")
    cases = CASES if not args.small else [((64, 64), torch.float32),
                                          ((32, 32, 32), torch.float64)]
    dflags = ops.PD_REG_ISOTROPIC if args.isotropic else 0
    pflags = ops.PD_DATA_L1 if args.ell1 else 0
    for shape, dt in cases:
        n, d = int(np.prod(shape)), len(shape)
        M = d * (d + 1) // 2
        mk = lambda k: 0.5 * torch.randn(k * n, device="cuda", dtype=dt)
        x, xbar, bt = mk(1), mk(1), mk(1)
        w, wbar, p, q = mk(d), mk(d), mk(d), mk(M)
        g = torch.empty(d * n, device="cuda", dtype=dt)
        div = torch.empty(n, device="cuda", dtype=dt)
        iw = (1.0, 1.0, 1.0)
        L2 = 16.0 if d == 3 else 11.37
        tau = sigma = 1.0 / np.sqrt(L2)
        kernels = {
            "tgv_dual": lambda: ops.tgv_dual(xbar, wbar, p, q, shape, iw, sigma, 2.0,
                                             dflags),
            "tgv_primal": lambda: ops.tgv_primal(p, q, x, xbar, w, wbar, bt, shape, iw,
                                                 tau, tau / 0.05, 1.0, pflags),
            "grad": lambda: ops.grad(x, shape, iw, out=g),
            "grad_adj": lambda: ops.grad_adj(g, shape, iw, out=div),
        }
        ts = {k: [] for k in kernels}
        for r in range(WARMUP + SAMPLES):
            for name, fn in kernels.items():
                t = timed(fn)
                if r >= WARMUP:
                    ts[name].append(t)
        out = {"shape": list(shape), "dtype": str(dt).split(".")[-1],
               "isotropic": bool(args.isotropic), "ell1": bool(args.ell1)}
        wd = words(d)
        for name in kernels:
            med, lo, hi = float(np.median(ts[name])), min(ts[name]), max(ts[name])
            nbytes = wd[name] * n * x.element_size()
            out[name] = {"ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                         "words_per_voxel": wd[name],
                         "GBps": round(nbytes / med / 1e6, 1),
                         "GBps_min_max": [round(nbytes / hi / 1e6, 1),
                                          round(nbytes / lo / 1e6, 1)]}
        out["iteration_ms"] = round(out["tgv_dual"]["ms"] + out["tgv_primal"]["ms"], 4)
        out["iteration_GBps"] = round(
            (wd["tgv_dual"] + wd["tgv_primal"]) * n * x.element_size() /
            out["iteration_ms"] / 1e6, 1)
        print(json.dumps(out), flush=True)
        del x, xbar, bt, w, wbar, p, q, g, div
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
