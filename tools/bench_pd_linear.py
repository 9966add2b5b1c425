#!/usr/bin/env python3
"""PrimalDualLinearSolver (the blur inside the saddle-point problem, no inner solves)
against today's deconvolution path, PrimalDualSolver + prox_linear_least_squares
(iter_max = 10), on the same data: TVL2 with a sigma = 2 Gaussian blur (13 taps),
float32, at 128^3, 256^3 and 512^3.

Per size: iterations per second of the new solver with the blur's epilogue on and off,
iterations per second of the old path, and -- the two iterations are not equivalent --
the objective lambda/2 |A x - b|^2 + TV(x) (scaled variable, anisotropic TV) that each
reaches in equal wall time: 1x, 2x and 4x the time of 10 iterations of the old path.
Wall time with a synchronisation at the end, one warm-up run, then the median of 3.
Nothing gates on these numbers; DESIGN.md section 4f records them.  One JSON line."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nsol_amd import linear_operators as LO, ops
from nsol_amd.application.run_deconvolution import build_solver
from nsol_amd.device import to_device

SIZES = [128, 256, 512]
ALPHA, BLUR = 0.01, 2.0
if len(sys.argv) > 1:
    SIZES = [int(a) for a in sys.argv[1:]]


def observation(n):
    """Blocks under the blur plus 2 % noise."""
    rng = np.random.default_rng(n)
    t = np.full((n, n, n), 20., dtype=np.float32)
    a, b, c = n // 6, n // 2, (5 * n) // 6
    t[a:b, a:c, b:c] = 80.
    t[b:c, a:b, a:c] = 50.
    t[a:c, b:c, a:b] = 110.
    A, _ = LO.LinearOperators3D().get_gaussian_blurring_operators(np.diag([BLUR ** 2] * 3))
    obs = A(t) + (2.2 * rng.standard_normal(t.shape)).astype(np.float32)
    return obs.astype(np.float32), A


def wall(solver):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver.run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def objective(solver, A, obs):
    """lambda/2 |A x - b~|^2 + sum |grad x| of the solver's iterate, scaled variable."""
    shape, scale = obs.shape, float(obs.max())
    x = ops.scale(solver.get_x_device(), scale, divide=True)
    bt = ops.scale(to_device(obs.reshape(-1), np.float32), scale, divide=True)
    r = ops.lincomb2(1.0, A._apply(x, shape), -1.0, bt)
    g = ops.grad(x, shape, (1.0, 1.0, 1.0))
    return 0.5 / ALPHA * ops.dot(r, r) + float(g.double().abs().sum().item())


def solver(obs, kind, iters):
    return build_solver(obs, np.ones(3), BLUR, "TVL2", kind, ALPHA, iters, iter_max=10,
                        L2=12 if kind == "PD" else 8, dtype=np.float32)


def rate(obs, kind, iters):
    wall(solver(obs, kind, iters))                      # warm-up
    ts = [wall(solver(obs, kind, iters)) for _ in range(3)]
    return iters / float(np.median(ts)), float(np.median(ts))


out = {"alpha": ALPHA, "blur_sigma": BLUR, "dtype": "float32", "sizes": []}
for n in SIZES:
    obs, A = observation(n)
    row = {"shape": [n, n, n], "taps": int(A.kernel.shape[0])}
    new_iters = 100 if n <= 256 else 50
    LO.USE_BLUR_EPILOGUE = True
    row["new_ips_epilogue"], _ = rate(obs, "PDL", new_iters)
    LO.USE_BLUR_EPILOGUE = False
    row["new_ips_no_epilogue"], _ = rate(obs, "PDL", new_iters)
    LO.USE_BLUR_EPILOGUE = True
    row["old_ips"], t10 = rate(obs, "PD", 10)
    row["old_seconds_for_10"] = t10
    row["equal_time"] = []
    for mult in (1, 2, 4):
        old = solver(obs, "PD", 10 * mult)
        t_old = wall(old)
        k = max(1, int(row["new_ips_epilogue"] * t10 * mult))
        new = solver(obs, "PDL", k)
        t_new = wall(new)
        row["equal_time"].append({
            "budget": mult, "old_iterations": 10 * mult, "old_seconds": t_old,
            "old_objective": objective(old, A, obs), "new_iterations": k,
            "new_seconds": t_new, "new_objective": objective(new, A, obs)})
        del old, new
    start = solver(obs, "PDL", 0)
    start.run()
    row["start_objective"] = objective(start, A, obs)
    for key in ("new_ips_epilogue", "new_ips_no_epilogue", "old_ips"):
        row[key] = round(row[key], 1)
    out["sizes"].append(row)
    del obs
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
