#!/usr/bin/env python3
"""The stacked forms of PrimalDualLinearSolver (nsol_amd/linear_stack.py) against the
loop of PrimalDualLinearSolver objects they replace, in the same process: TVL2 with a
sigma = 2 Gaussian blur (13 taps), float32.

  images   256^2 x 64 and 1024^2 x 16 through PrimalDualLinearBatch (the blur over the
           stack is one launch per pass);
  volumes  64^3 x 16 and 128^3 x 8 through PrimalDualLinearBatch (the blur per member);
  sweep    5 alphas at 256^3 through PrimalDualLinearSweep.

Per shape: seconds of both forms -- wall time of run() with a synchronisation at the
end, uploads included, one warm-up run, then the median of 3 --, their ratio, and the
kernel launches per iteration of both.  Nothing gates on these numbers; DESIGN.md
section 4g records them.  One JSON line."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nsol_amd import linear_stack, ops
from nsol_amd.application.run_deconvolution import build_solver, pdl_wiring

BLUR = 2.0
ALPHAS = [0.005, 0.01, 0.02, 0.05, 0.1]
CASES = [("images", (256, 256), 64, 50), ("images", (1024, 1024), 16, 50),
         ("volumes", (64, 64, 64), 16, 50), ("volumes", (128, 128, 128), 8, 50),
         ("sweep", (256, 256, 256), 5, 20)]
if len(sys.argv) > 1:           # e.g. "0 2": the cases by index
    CASES = [CASES[int(a)] for a in sys.argv[1:]]


def observation(shape, seed):
    """Blocks plus noise (the solvers are timed, not judged)."""
    rng = np.random.default_rng(seed)
    t = np.full(shape, 20., dtype=np.float32)
    t[tuple(slice(s // 6, s // 2) for s in shape)] = 80.
    t[tuple(slice(s // 2, (5 * s) // 6) for s in shape)] = 110.
    return t + (2.2 * rng.standard_normal(shape)).astype(np.float32)


def solvers_for(kind, data, iters):
    spacing = np.ones(data[0].ndim)
    alphas = ALPHAS if kind == "sweep" else [0.01] * len(data)
    return [build_solver(d, spacing, BLUR, "TVL2", "PDL", a, iters, dtype=np.float32)
            for d, a in zip(data, alphas)]


def wall(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def median_of_3(make):
    wall(make())                                        # warm-up
    return float(np.median([wall(make()) for _ in range(3)]))


out = {"blur_sigma": BLUR, "dtype": "float32", "cases": []}
for kind, shape, P, iters in CASES:
    if kind == "sweep":
        data = [observation(shape, 1)] * P
    else:
        data = [observation(shape, m) for m in range(P)]

    def loop():
        ss = solvers_for(kind, data, iters)
        return lambda: [s.run() for s in ss]

    def stacked():
        if kind == "sweep":
            kw = pdl_wiring(data[0], np.ones(len(shape)), BLUR, "TVL2",
                            iterations=iters, dtype=np.float32)
            del kw["alpha"]
            form = linear_stack.PrimalDualLinearSweep(parameters={"alpha": ALPHAS}, **kw)
        else:
            form = linear_stack.PrimalDualLinearBatch(solvers_for(kind, data, iters))
        made.append(form)
        return form.run
    made = []
    t_loop, t_stack = median_of_3(loop), median_of_3(stacked)
    form = made[-1]
    execution = form.get_execution()
    G = form.get_group_size()
    template = solvers_for(kind, data[:1], iters)[0]
    # every group makes its own launches
    stacked_launches = sum(linear_stack.launches_per_iteration(template, b - a)[0]
                           for a, b in ops.sweep_groups(P, G or 1))
    out["cases"].append({
        "kind": kind, "shape": list(shape), "members": P, "iterations": iters,
        "execution": execution if isinstance(execution, str) else sorted(set(execution)),
        "group_size": G, "loop_seconds": round(t_loop, 5),
        "stacked_seconds": round(t_stack, 5), "ratio": round(t_loop / t_stack, 2),
        "launches_per_iteration_stacked": stacked_launches,
        "launches_per_iteration_loop":
            linear_stack.launches_per_iteration(template, P)[1]})
    del data, made, form
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
