#!/usr/bin/env python3
"""The forms of k_tgv_primal (csrc/nsol_tgv.hip) against each other, and one iteration of
TGVPrimalDualLinearSolver against one of PrimalDualLinearSolver, launch by launch.  The
method is tools/bench_tgv.py's: the kernels alternate inside one process; device events
around REPS launches; 3 warm-up rounds, then the median of 5 (min - max).

(a) k_tgv_primal plain / WGT / LIN at 256^3 and 512^3 float32 and 256^3 float64.  Byte
    model, words per voxel (d = dimension, M = d (d + 1) / 2):
      plain  read p (d), q (M), x, w (d), bt; write x, xbar, w, wbar      4 + 4 d + M   (22)
      WGT    ... and wt                                                   5 + 4 d + M   (23)
      LIN    g in bt's place                                              4 + 4 d + M   (22)
    The ratios WGT / plain and LIN / plain of the medians are printed with the ratios
    of the extremes.
(b) 256^3 float32, the sigma = 2 Gaussian of LinearOperators3D: the launches of one
    TGVPrimalDualLinearSolver iteration (k_tgv_dual, the blur with its axpby epilogue,
    k_pdl_dual_data, the adjoint blur, k_tgv_primal LIN) and of one PrimalDualLinearSolver
    iteration (the same three for the data term, then k_pd_lin), and their sums.

One JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nsol_amd import linear_operators, ops  # noqa: E402

CASES = [((256, 256, 256), torch.float32), ((512, 512, 512), torch.float32),
         ((256, 256, 256), torch.float64)]
ITERATION_CASE = ((256, 256, 256), torch.float32)
REPS = 10            # launches per timed sample
WARMUP, SAMPLES = 3, 5


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def alternate(kernels):
    """{name: [SAMPLES times in ms]}: the kernels in turn, round after round."""
    ts = {k: [] for k in kernels}
    for r in range(WARMUP + SAMPLES):
        for name, fn in kernels.items():
            t = timed(fn)
            if r >= WARMUP:
                ts[name].append(t)
    return ts


def summary(ts, nbytes=None):
    med, lo, hi = float(np.median(ts)), min(ts), max(ts)
    out = {"ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)]}
    if nbytes is not None:
        out["GBps"] = round(nbytes / med / 1e6, 1)
        out["GBps_min_max"] = [round(nbytes / hi / 1e6, 1), round(nbytes / lo / 1e6, 1)]
    return out


def ratio(ts, name, base):
    """median / median, with (min / max, max / min) as its spread."""
    return {"median": round(float(np.median(ts[name]) / np.median(ts[base])), 4),
            "min_max": [round(min(ts[name]) / max(ts[base]), 4),
                        round(max(ts[name]) / min(ts[base]), 4)]}


def forms(shape, dt):
    n, d = int(np.prod(shape)), len(shape)
    M = d * (d + 1) // 2
    mk = lambda k: 0.5 * torch.randn(k * n, device="cuda", dtype=dt)
    x, xbar, bt, g = mk(1), mk(1), mk(1), mk(1)
    wt = torch.rand(n, device="cuda", dtype=dt) * 2.0
    wt[torch.rand(n, device="cuda") < 0.2] = 0
    w, wbar, p, q = mk(d), mk(d), mk(d), mk(M)
    iw = (1.0, 1.0, 1.0)
    tau = 0.25
    kernels = {
        "plain": lambda: ops.tgv_primal(p, q, x, xbar, w, wbar, bt, shape, iw, tau,
                                        tau / 0.05, 1.0, 0),
        "wgt": lambda: ops.tgv_primal_w(p, q, x, xbar, w, wbar, bt, wt, shape, iw, tau,
                                        tau / 0.05, 1.0, 0),
        "lin": lambda: ops.tgv_primal_lin(p, q, x, xbar, w, wbar, g, shape, iw, tau, 1.0,
                                          0.0, np.inf),
    }
    ts = alternate(kernels)
    base = 4 + 4 * d + M
    wd = {"plain": base, "wgt": base + 1, "lin": base}
    out = {"part": "forms", "shape": list(shape), "dtype": str(dt).split(".")[-1]}
    for name in kernels:
        out[name] = summary(ts[name], wd[name] * n * x.element_size())
        out[name]["words_per_voxel"] = wd[name]
    out["wgt_over_plain"] = ratio(ts, "wgt", "plain")
    out["lin_over_plain"] = ratio(ts, "lin", "plain")
    print(json.dumps(out), flush=True)


def iteration(shape, dt):
    n, d = int(np.prod(shape)), len(shape)
    M = d * (d + 1) // 2
    A, _ = linear_operators.LinearOperators3D().get_gaussian_blurring_operators(
        np.diag([4.0] * 3))
    mk = lambda k: 0.5 * torch.randn(k * n, device="cuda", dtype=dt)
    x, xbar, xbar2, bt, r = mk(1), mk(1), mk(1), mk(1), mk(1)
    w, wbar, p, p2, q = mk(d), mk(d), mk(d), mk(d), mk(M)
    slot = torch.empty(1, dtype=torch.float64, device="cuda")
    iw = (1.0, 1.0, 1.0)
    tau = sigma = 0.24
    held = {"g": A._apply(r, shape)}
    epilogue = A.apply_axpby(xbar, r, shape, sigma, 1.0, result=slot) is not None

    def blur():
        if epilogue:
            A.apply_axpby(xbar, r, shape, sigma, 1.0, result=slot)
        else:
            held["t"] = A._apply(xbar, shape)

    def adjoint():
        held["g"] = A._apply(r, shape)

    kernels = {
        "tgv_dual": lambda: ops.tgv_dual(xbar, wbar, p, q, shape, iw, sigma, 2.0, 0),
        "blur": blur,
        "pdl_dual_data": lambda: ops.pdl_dual_data(
            r, None if epilogue else held["t"], bt, None, sigma, 20.0, False),
        "adjoint_blur": adjoint,
        "tgv_primal_lin": lambda: ops.tgv_primal_lin(p, q, x, xbar, w, wbar, held["g"],
                                                     shape, iw, tau, 1.0, 0.0, np.inf),
        "pdl_iter": lambda: ops.pdl_iter(xbar, xbar2, x, held["g"], p, p2, shape, iw,
                                         sigma, 1.0, tau, 1.0, 0.0, np.inf, ops.PD_REG_TV,
                                         has_p=True),
    }
    if not epilogue:
        blur()
    ts = alternate(kernels)
    out = {"part": "iteration", "shape": list(shape), "dtype": str(dt).split(".")[-1],
           "blur_epilogue": bool(epilogue)}
    for name in kernels:
        out[name] = summary(ts[name])
    data = ("blur", "pdl_dual_data", "adjoint_blur")
    total = lambda names, f: float(sum(f(ts[k]) for k in names))
    for label, names in (("tgv_linear_iteration", ("tgv_dual",) + data + ("tgv_primal_lin",)),
                         ("pd_linear_iteration", data + ("pdl_iter",))):
        out[label] = {"ms": round(total(names, np.median), 4),
                      "ms_min_max": [round(total(names, min), 4),
                                     round(total(names, max), 4)]}
    out["tgv_over_pd_linear"] = round(out["tgv_linear_iteration"]["ms"] /
                                      out["pd_linear_iteration"]["ms"], 3)
    print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--small", action="store_true",
                    help="32^3 only: a rehearsal of the script, not a measurement")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tgv_linear needs a HIP device")
    cases = CASES if not args.small else [((32, 32, 32), torch.float32),
                                          ((32, 32, 32), torch.float64)]
    for shape, dt in cases:
        forms(shape, dt)
        torch.cuda.empty_cache()
    iteration(*(ITERATION_CASE if not args.small else ((32, 32, 32), torch.float32)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
