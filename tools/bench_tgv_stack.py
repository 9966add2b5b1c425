#!/usr/bin/env python3
"""The stacked forms of TGVPrimalDualSolver (nsol_amd/tgv_stack.py) against the loop of
TGVPrimalDualSolver objects they replace, in the same process: TGV-l2, float32.

  batch   P 2-D slices through TGVPrimalDualBatch (every member its own observation);
  sweep   P (alpha, beta) members on one 3-D volume through TGVPrimalDualSweep.

Per case two pairs of numbers, the loop first:
  run      wall seconds of the whole run, uploads included, with one synchronisation at the
           end; one warm-up run of each form, then loop and stacked form ALTERNATE and
           the median of 5 is taken of each (the lowest and highest are reported too);
  device   microseconds per iteration on the stream (events around the launches alone, the
           state already on the device): 2 P launches of the single kernels against the
           stacked form's 2 per group, alternating as above.
Nothing gates on these numbers; DESIGN.md section 4k records them.  One JSON line."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nsol_amd import ops, tgv_numpy, tgv_stack
from nsol_amd.tgv_solver import TGVPrimalDualSolver

ALPHAS, BETAS = [0.05, 0.2], [0.5, 1.0, 2.0]
CASES = [("batch", (256, 256), 1, 100), ("batch", (256, 256), 16, 100),
         ("batch", (256, 256), 64, 100), ("batch", (512, 512), 16, 100),
         ("batch", (1024, 1024), 16, 50),
         ("sweep", (64, 64, 64), 6, 50), ("sweep", (128, 128, 128), 6, 50),
         ("sweep", (256, 256, 256), 6, 20)]
if len(sys.argv) > 1:           # e.g. "0 2": the cases by index
    CASES = [CASES[int(a)] for a in sys.argv[1:]]
REPEATS = 5


def observation(shape, seed):
    """A ramp with blocks and noise (the solvers are timed, not judged)."""
    rng = np.random.default_rng(seed)
    t = np.add.outer(np.linspace(20., 60., shape[0]), np.zeros(shape[1:])) \
        .astype(np.float32)
    t[tuple(slice(s // 6, s // 2) for s in shape)] += 40.
    return t + (2.2 * rng.standard_normal(shape)).astype(np.float32)


def members_of(kind, P):
    if kind == "sweep":
        return [(a, b) for a in ALPHAS for b in BETAS][:P]
    return [(0.1, 1.0 + 0.01 * m) for m in range(P)]


def solver(obs, alpha, beta, iters):
    return TGVPrimalDualSolver(b=obs.reshape(-1), x0=obs.reshape(-1), dimension=obs.ndim,
                               shape=obs.shape, alpha=alpha, beta=beta, iterations=iters,
                               x_scale=float(obs.max()), dtype=np.float32)


def wall(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def on_stream(launch, iters):
    """Microseconds per iteration between two events around `iters` calls of launch()."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        launch()
    stop.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(stop) / iters


def alternate(first, second):
    """(median, lowest, highest) of REPEATS measurements of each, taken in turn after one
    warm-up of each."""
    first(), second()
    a, b = [], []
    for _ in range(REPEATS):
        a.append(first())
        b.append(second())
    return tuple((float(np.median(v)), float(min(v)), float(max(v))) for v in (a, b))


def device_pair(shape, P, G, params, iters):
    """(loop, stacked) launch closures on zero-initialised device state."""
    d, n = len(shape), int(np.prod(shape))
    M = tgv_numpy.components(d)
    dev = torch.device("cuda")
    z = lambda k: torch.zeros(k, dtype=torch.float32, device=dev)
    xbar, wbar, p, q = z(P * n), z(P * d * n), z(P * d * n), z(P * M * n)
    x, w, bt = z(P * n), z(P * d * n), z(P * n)
    iw = ops.inv_spacing(np.ones(d), d)
    tau = sigma = 1. / np.sqrt(tgv_numpy.norm_bound(d))
    groups = ops.sweep_groups(P, G)
    tabs = [ops.tgv_stack_table(x, [b for _, b in params[a:e]],
                                [tau / al for al, _ in params[a:e]]) for a, e in groups]

    def loop():
        for m, (alpha, beta) in enumerate(params):
            s = lambda t, k: t[m * k * n:(m + 1) * k * n]
            ops.tgv_dual(s(xbar, 1), s(wbar, d), s(p, d), s(q, M), shape, iw, sigma, beta)
            ops.tgv_primal(s(p, d), s(q, M), s(x, 1), s(xbar, 1), s(w, d), s(wbar, d),
                           s(bt, 1), shape, iw, tau, tau / alpha)

    def stacked():
        for (a, e), tab in zip(groups, tabs):
            s = lambda t, k: t[a * k * n:e * k * n]
            ops.tgv_stack_dual(s(xbar, 1), s(wbar, d), s(p, d), s(q, M), e - a, shape, iw,
                               sigma, tab)
            ops.tgv_stack_primal(s(p, d), s(q, M), s(x, 1), s(xbar, 1), s(w, d),
                                 s(wbar, d), s(bt, 1), e - a, shape, iw, tau, tab)
    return loop, stacked


out = {"dtype": "float32", "repeats": REPEATS, "cases": []}
for kind, shape, P, iters in CASES:
    params = members_of(kind, P)
    P = len(params)
    data = [observation(shape, 1)] * P if kind == "sweep" else \
        [observation(shape, m) for m in range(P)]
    made = []

    def loop():
        ss = [solver(o, a, b, iters) for o, (a, b) in zip(data, params)]
        return wall(lambda: [s.run() for s in ss])

    def stacked():
        if kind == "sweep":
            o = data[0]
            form = tgv_stack.TGVPrimalDualSweep(
                o.reshape(-1), o.reshape(-1), o.ndim, {"alpha": ALPHAS, "beta": BETAS},
                shape=o.shape, iterations=iters, x_scale=float(o.max()), dtype=np.float32)
        else:
            form = tgv_stack.TGVPrimalDualBatch(
                [solver(o, a, b, iters) for o, (a, b) in zip(data, params)])
        made[:] = [form]
        return wall(form.run)

    t_loop, t_stack = alternate(loop, stacked)
    form = made[0]
    execution, G = form.get_execution(), form.get_group_size() or 1
    del made[:], form
    torch.cuda.empty_cache()
    dl, ds = device_pair(shape, P, G, params, iters)
    d_loop, d_stack = alternate(lambda: on_stream(dl, iters), lambda: on_stream(ds, iters))
    out["cases"].append({
        "kind": kind, "shape": list(shape), "members": P, "iterations": iters,
        "execution": execution if isinstance(execution, str) else sorted(set(execution)),
        "group_size": G,
        "run_seconds_loop": round(t_loop[0], 5), "run_seconds_stacked": round(t_stack[0], 5),
        "run_seconds_loop_range": [round(v, 5) for v in t_loop[1:]],
        "run_seconds_stacked_range": [round(v, 5) for v in t_stack[1:]],
        "run_ratio": round(t_loop[0] / t_stack[0], 2),
        "device_us_per_iteration_loop": round(d_loop[0], 1),
        "device_us_per_iteration_stacked": round(d_stack[0], 1),
        "device_us_loop_range": [round(v, 1) for v in d_loop[1:]],
        "device_us_stacked_range": [round(v, 1) for v in d_stack[1:]],
        "device_ratio": round(d_loop[0] / d_stack[0], 2)})
    print(json.dumps(out["cases"][-1]), file=sys.stderr, flush=True)
    del data, dl, ds
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
