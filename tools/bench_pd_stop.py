#!/usr/bin/env python3
"""What the stopping rule of the primal-dual solver costs: float32 TV-l2 at 512^3 and
128^3,
  * one launch of the checking kernel (k_pd_check, nsol_pd_check_iter_*, its closing
    workgroup included) against one launch of k_pd_fused (nsol_pd_fused_iter_*) on the
    same arrays, alternating the two in one process, device events, one warm-up then
    the median of 5 (min - max);
  * the public run, PrimalDualSolver.run() of ITERS iterations on a device-resident
    start: plain, and with a tolerance that is never met (1e-300) at check_every = 5,
    10 and 50 -- the stretches between checks keep the multi-iteration kernels, every
    check adds one read-back of four doubles -- wall clock around run(), which ends in
    a synchronisation; one warm-up run each, then the median of 5 (min - max).
Nothing gates on these numbers; DESIGN.md section 4d records them."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nsol_amd import ops
import nsol_amd.linear_operators as LO
import nsol_amd.primal_dual_solver as pd
from nsol_amd.proximal_operators import ProximalOperators as prox

SHAPES = [(128, 128, 128), (512, 512, 512)]
ITERS = 100
REPS = 20           # launches per timed sample


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)


def solver(b, shape, tolerance, check_every):
    grad, grad_adj = LO.LinearOperators3D().get_gradient_operators()
    Z = (3 * shape[0],) + tuple(shape[1:])
    D = lambda x: grad(x.reshape(*shape)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    pf = lambda x, tau: prox.prox_ell2_denoising(x, tau, x0=b, x_scale=1.0)
    return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=prox.prox_tv_conj, B=D, B_conj=Da,
                               L2=16, x0=b, alpha=0.03, iterations=ITERS, x_scale=1.0,
                               dtype=np.float32, tolerance=tolerance,
                               check_every=check_every)


for shape in SHAPES:
    n, dim = int(np.prod(shape)), len(shape)
    bt = torch.rand(n, device="cuda")
    x = bt.clone()
    xb = [bt.clone(), torch.empty_like(bt)]
    p = [torch.zeros(dim * n, device="cuda") for _ in range(2)]
    w = (1.0, 1.0, 1.0)
    ws = ops.pd_check_workspace(x, shape)
    row = torch.zeros(4, dtype=torch.float64, device="cuda")
    out = {"shape": shape, "dtype": "float32"}

    def check():
        for i in range(REPS):
            k = i & 1
            ops.pd_check_iter(xb[k], xb[1 - k], x, bt, None, p[k], p[1 - k], shape, w,
                              0.25, 1.0, 0.25, 0.25 / 0.03, 1.0, ops.PD_DATA_L2, ws, row)

    def plain():
        for i in range(REPS):
            k = i & 1
            ops.pd_fused_iter(xb[k], xb[1 - k], x, bt, p[k], p[1 - k], shape, w, 0.25,
                              1.0, 0.25, 0.25 / 0.03, 1.0, ops.PD_DATA_L2)
    ts = {"check": [], "plain": []}
    for r in range(6):                       # the first round is the warm-up
        for name, fn in (("check", check), ("plain", plain)):
            t = timed(fn) / REPS
            if r:
                ts[name].append(t)
    for name in ("check", "plain"):
        med, lo, hi = stats(ts[name])
        out["%s_launch_ms" % name] = med
        out["%s_launch_min_max" % name] = [lo, hi]
    out["launch_ratio"] = round(out["check_launch_ms"] / out["plain_launch_ms"], 3)
    del x, xb, p, ws
    torch.cuda.empty_cache()

    # the public run
    runs = [("plain", None, 10), ("K5", 1e-300, 5), ("K10", 1e-300, 10),
            ("K50", 1e-300, 50)]
    solvers = {name: solver(bt, shape, tol, k) for name, tol, k in runs}
    for _ in range(12):                      # the headline kernel's online tuner
        solvers["plain"].run()
        if ops.pd_fusedk_tuned(bt, shape) != 0:
            break
    ts = {name: [] for name, _, _ in runs}
    for r in range(6):
        for name, _, _ in runs:
            t0 = time.perf_counter()
            solvers[name].run()
            t = (time.perf_counter() - t0) * 1e3
            if r:
                ts[name].append(t)
    out["run_of"] = ITERS
    for name, _, _ in runs:
        med, lo, hi = stats(ts[name])
        out["%s_run_ms" % name] = med
        out["%s_run_min_max" % name] = [lo, hi]
        if name != "plain":
            assert solvers[name].get_iterations_done() == ITERS
            out["%s_checks" % name] = len(solvers[name].get_changes())
            out["%s_ratio" % name] = round(med / out["plain_run_ms"], 3)
    print(json.dumps(out), flush=True)
    del solvers, bt
    torch.cuda.empty_cache()
