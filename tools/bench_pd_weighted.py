#!/usr/bin/env python3
"""The weighted one-iteration kernel (k_pd_w, nsol_pd_weighted_iter_*) against the
unweighted one (k_pd_fused, nsol_pd_fused_iter_*) on the same arrays, alternating
the two in one process, device events, one warm-up then the median of 5 (min - max);
and the public run of 60 iterations at 512^3, where the unweighted run takes three
iterations per pass and the weighted one a pass per iteration.  Nothing gates on
these numbers; DESIGN.md section 4c records them."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nsol_amd import ops
from nsol_amd.primal_dual_solver import step_schedule

CASES = [((1024, 1024), torch.float32), ((128, 128, 128), torch.float32),
         ((256, 256, 256), torch.float32), ((512, 512, 512), torch.float32),
         ((512, 512, 512), torch.float64)]
REPS = 20           # launches per timed sample


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)


def weights_like(bt):
    """A third zeros, a third ones, the rest in (0, 3]."""
    u = torch.rand_like(bt)
    return torch.where(u < 1 / 3, torch.zeros_like(u),
                       torch.where(u < 2 / 3, torch.ones_like(u), 9 * (1 - u)))


for shape, dt in CASES:
    n, dim = int(np.prod(shape)), len(shape)
    bt = torch.rand(n, device="cuda", dtype=dt)
    wt = weights_like(bt)
    x = bt.clone()
    xb = [bt.clone(), torch.empty_like(bt)]
    p = [torch.zeros(dim * n, device="cuda", dtype=dt) for _ in range(2)]
    w = (1.0, 1.0, 1.0)
    out = {"shape": shape, "dtype": str(dt).split(".")[-1]}
    flags = ops.PD_DATA_L2 | ops.PD_DATA_WEIGHTED
    # the same scalars for every launch: a table of one iteration, p counted as given
    one = np.array([0.25])
    tab = ops.pd_weighted_table(x, 1, [1 / 0.03], one, one, np.array([1.0]), False,
                                0.05, flags)

    def weighted():
        for i in range(REPS):
            k = i & 1
            ops.pd_weighted_iter(xb[k], xb[1 - k], x, bt, wt, p[k], p[1 - k], 1, shape,
                                 w, tab, 0, flags)

    def plain():
        for i in range(REPS):
            k = i & 1
            ops.pd_fused_iter(xb[k], xb[1 - k], x, bt, p[k], p[1 - k], shape, w, 0.25,
                              1.0, 0.25, 0.25 / 0.03, 1.0, ops.PD_DATA_L2)
    ts = {"weighted": [], "plain": []}
    for r in range(6):                       # the first round is the warm-up
        for name, fn in (("weighted", weighted), ("plain", plain)):
            t = timed(fn) / REPS
            if r:
                ts[name].append(t)
    for name, arrays in (("weighted", 6 + 2 * dim), ("plain", 5 + 2 * dim)):
        med, lo, hi = stats(ts[name])
        out["%s_ms" % name] = med
        out["%s_min_max" % name] = [lo, hi]
        out["%s_GBps" % name] = round(arrays * n * bt.element_size() / med / 1e6, 1)
    out["ratio"] = round(out["weighted_ms"] / out["plain_ms"], 3)
    print(json.dumps(out), flush=True)
    del bt, wt, x, xb, p
    torch.cuda.empty_cache()

# the public path: 60 iterations at 512^3 float32
shape = (512, 512, 512)
n = int(np.prod(shape))
bt = torch.rand(n, device="cuda")
wt = weights_like(bt)
x = bt.clone(); xa = torch.empty_like(bt)
xb = [bt.clone(), torch.empty_like(bt)]
p = [torch.zeros(3 * n, device="cuda") for _ in range(2)]
iters = 60
sig, ta, th = step_schedule("ALG2", 16.0, 1 / 0.03, iters)
w = (1.0, 1.0, 1.0)
for _ in range(12):                          # the headline kernel's online tuner
    ops.pd_run(xb[0], xb[1], x, bt, p[0], p[1], shape, w, 1 / 0.03, sig, ta, th, True,
               0.05, ops.PD_DATA_L2, x_alt=xa)
    torch.cuda.synchronize()
    if ops.pd_fusedk_tuned(x, shape) != 0:
        break
ts = {"weighted": [], "plain": []}
for r in range(6):
    for name in ("weighted", "plain"):
        if name == "plain":
            fn = lambda: ops.pd_run(xb[0], xb[1], x, bt, p[0], p[1], shape, w, 1 / 0.03,
                                    sig, ta, th, True, 0.05, ops.PD_DATA_L2, x_alt=xa)
        else:
            fn = lambda: ops.pd_weighted_run(
                xb[0], xb[1], x, bt, wt, p[0], p[1], 1, shape, w, [1 / 0.03], sig, ta,
                th, True, 0.05, ops.PD_DATA_L2 | ops.PD_DATA_WEIGHTED)
        t = timed(fn)
        if r:
            ts[name].append(t / iters)
out = {"shape": shape, "dtype": "float32", "run_of": iters}
for name in ("weighted", "plain"):
    med, lo, hi = stats(ts[name])
    out["%s_ms_per_iteration" % name] = med
    out["%s_min_max" % name] = [lo, hi]
out["ratio"] = round(out["weighted_ms_per_iteration"] / out["plain_ms_per_iteration"], 3)
print(json.dumps(out), flush=True)
