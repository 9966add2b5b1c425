#!/usr/bin/env python3
"""Cost of observing a fused primal-dual run on the device (observer.py,
keep_iterates=False) against the same run unobserved.

Headline: 512^3 float32 TV-L2, 60 iterations, a float32 reference (exact in
the working dtype).  Arms, alternated round by round in one process so that
drift hits all of them alike:
  plain     no observer;
  every3    {TV, SSD, PSNR, NCC} at iterations 0, 3, ..., 60 (21 points);
  every1    the same at every iteration;
  every3+   {TV, SSD, PSNR, NCC, SSIM, NMI} every 3 iterations.
Each run is timed with HIP events around solver.run() (which ends with the
board read and the finalisation); an observed run pays its set-up inside (the
reference's upload and set-up sums, once per run).  Also reported, each the
median of --rounds: "setup_s", the observer's set-up of such a run on its own,
and "pass_ms", one nsol_observe_* pass of the every3 arm ({TV, SSD, PSNR,
NCC}: pair and gradient groups) on the volume, event-timed.
The host path (keep_iterates=True: a host copy of every iterate, float64, and
the measures evaluated over the history afterwards) is timed at the headline
size too, for --host-iterations iterations only: every copy holds 1 GiB of
host memory at 512^3, the 61 of a whole run would not fit.  It is reported
with the unobserved and device-observed (every = 1) runs of that length.
Prints one JSON line: per arm the median seconds, min / max, and the ratio of
the medians to plain."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import nsol_amd.linear_operators as LO  # noqa: E402
import nsol_amd.primal_dual_solver as pd  # noqa: E402
from nsol_amd.observer import Observer  # noqa: E402
from nsol_amd.prior_measures import PriorMeasures as PM  # noqa: E402
from nsol_amd.proximal_operators import ProximalOperators as prox  # noqa: E402
from nsol_amd.similarity_measures import SimilarityMeasures as SM  # noqa: E402


def make(obs, iters):
    shape = obs.shape
    b = obs.reshape(-1)
    xs = float(obs.max())
    grad, grad_adj = LO.LinearOperators3D().get_gradient_operators()
    Z = (3 * shape[0],) + shape[1:]
    D = lambda x: grad(x.reshape(*shape)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    pf = lambda x, tau: prox.prox_ell2_denoising(x, tau, x0=b, x_scale=xs)
    s = pd.PrimalDualSolver(prox_f=pf, prox_g_conj=prox.prox_tv_conj, B=D,
                            B_conj=Da, L2=16.0, x0=b, alpha=0.05,
                            iterations=iters, x_scale=xs, dtype=np.float32)
    return s, D


def measures(ref, D, shape, extra):
    m = {"TV": lambda x: PM.total_variation(x, D, 3),
         "SSD": lambda x: SM.SSD(x, ref),
         "PSNR": lambda x: SM.PSNR(x, ref),
         "NCC": lambda x: SM.NCC(x, ref)}
    if extra:
        m["SSIM"] = lambda x: SM.SSIM(x.reshape(shape), ref.reshape(shape))
        m["NMI"] = lambda x: SM.NMI(x, ref)
    return m


def timed_run(obs, ref, iters, every, extra, keep=False):
    s, D = make(obs, iters)
    if every is not None:
        o = Observer(keep_iterates=keep, every=every)
        o.set_measures(measures(ref, D, obs.shape, extra))
        s.set_observer(o)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    s.run()
    if every is not None:
        o.compute_measures()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3


def setup_s(obs, ref, iters):
    """The device observer's set-up of a run of the every3 arm on its own:
    classification, board, the reference's upload and its set-up sums."""
    s, D = make(obs, iters)
    o = Observer(keep_iterates=False, every=3)
    o.set_measures(measures(ref, D, obs.shape, False))
    s.set_observer(o)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s._observe_begin(iters)
    for r in list(o._session._refs.values()):
        r.device(torch.float32)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def pass_ms(obs, ref, reps):
    """One observation pass of the every3 arm, event-timed."""
    from nsol_amd import ops
    from nsol_amd.device import to_device
    x = to_device(obs.reshape(-1), np.float32)
    y = to_device(ref, np.float32)
    row = torch.empty(ops.OBS_SUMS, dtype=torch.float64, device=x.device)
    go = lambda: ops.observe(x, 1.0, row, obs.shape, y=y, ybar=100.0,
                             flags=ops.OBS_PAIR | ops.OBS_GRAD)
    go()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        go()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-iterations", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    n = args.n
    obs = (100.0 + 20.0 * rng.standard_normal((n, n, n))).astype(np.float32)
    ref = np.full(n ** 3, 100.0, dtype=np.float32)
    arms = {"plain": (None, False), "every3": (3, False), "every1": (1, False),
            "every3+": (3, True)}
    times = {k: [] for k in arms}
    for k, (ev, ex) in arms.items():                   # warm-up
        timed_run(obs, ref, args.iterations, ev, ex)
    for _ in range(args.rounds):
        for k, (ev, ex) in arms.items():
            times[k].append(timed_run(obs, ref, args.iterations, ev, ex))
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"shape": [n] * 3, "iterations": args.iterations, "dtype": "float32",
           "rounds": args.rounds}
    for k, v in times.items():
        out[k] = {"median_s": med[k], "min_s": float(np.min(v)),
                  "max_s": float(np.max(v)),
                  "ratio": med[k] / med["plain"]}
    su = [setup_s(obs, ref, args.iterations) for _ in range(args.rounds)]
    out["setup_s"] = {"median": float(np.median(su)), "min": float(np.min(su)),
                      "max": float(np.max(su))}
    pm = pass_ms(obs, ref, 20)
    out["pass_ms"] = {"median": float(np.median(pm)), "min": float(np.min(pm)),
                      "max": float(np.max(pm)),
                      "bytes_per_voxel": 8, "voxels": n ** 3}
    hi = args.host_iterations
    out["host_path"] = {
        "shape": [n] * 3, "iterations": hi,
        "plain_s": timed_run(obs, ref, hi, None, False),
        "device_every1_s": timed_run(obs, ref, hi, 1, False),
        "host_every1_s": timed_run(obs, ref, hi, 1, False, keep=True)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
