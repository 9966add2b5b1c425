#!/usr/bin/env python3
"""The stacked forms of TGVPrimalDualLinearSolver (nsol_amd/tgv_linear_stack.py) against
the loop of TGVPrimalDualLinearSolver objects they replace: TGV-l2 behind a sigma = 2
Gaussian blur (13 taps), float32, 100 iterations.

  images   256^2 and 1024^2, P = 4, 16, 64 (the blur over the stack is one launch per pass:
           7 launches per iteration and group against 7 P);
  volumes  64^3 and 128^3, P = 4, 16, with the one-pass blur's epilogue on and off (the blur
           runs member by member: 2 P + 3 launches against 5 P).

Per case, for a batch (every member its own observation) and an (alpha, beta) sweep (one
observation), each against the loop of plain solvers with the same members: milliseconds
between two device events around the whole call -- construction of the stacked form,
uploads, scaling and all iterations; for the loop every solver's run() --, the two forms
ALTERNATING in one process after one warm-up of each, the median of 5 with the lowest and
the highest, and the kernel launches per iteration of both.

Without arguments every case runs in a child process of its own under a time limit, one
after the other, and the first child that fails or runs out of time ends the run: nothing
more is started on the device then.  `--case K` runs case K in this process.  Nothing
gates on these numbers; DESIGN.md section 4l records them.  One JSON line per case."""
import json, os, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

BLUR, ITERS, REPEATS = 2.0, 100, 5
CHILD_SECONDS = 240
ALPHAS = [0.02, 0.05, 0.1, 0.2]
CASES = [("images", s, P, None) for s in ((256, 256), (1024, 1024)) for P in (4, 16, 64)] + \
    [("volumes", s, P, e) for s in ((64, 64, 64), (128, 128, 128)) for P in (4, 16)
     for e in (True, False)]


def members_of(kind, P):
    """(alpha, beta) per member: a grid for the sweep, one alpha and nearby betas for the
    batch."""
    if kind == "sweep":
        return [(a, b) for a in ALPHAS for b in np.linspace(0.5, 3., P // len(ALPHAS))]
    return [(0.05, 1.0 + 0.01 * m) for m in range(P)]


def observation(shape, seed):
    """A ramp with a block and noise (the solvers are timed, not judged)."""
    rng = np.random.default_rng(seed)
    t = np.add.outer(np.linspace(20., 60., shape[0]), np.zeros(shape[1:])) \
        .astype(np.float32)
    t[tuple(slice(s // 6, s // 2) for s in shape)] += 40.
    return t + (2.2 * rng.standard_normal(shape)).astype(np.float32)


def arguments(obs, op):
    shape = obs.shape
    A = lambda x: op(x.reshape(*shape)).flatten()
    return dict(A=A, A_adj=A, b=obs.reshape(-1), x0=obs.reshape(-1), dimension=obs.ndim,
                iterations=ITERS, x_scale=float(obs.max()), dtype=np.float32)


def between_events(run):
    """Milliseconds on the stream around run(), which may upload and synchronise."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    run()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def alternate(first, second):
    """(median, lowest, highest) of REPEATS measurements of each, taken in turn after one
    warm-up of each."""
    first(), second()
    a, b = [], []
    for _ in range(REPEATS):
        a.append(first())
        b.append(second())
    return tuple([round(float(f(v)), 2) for f in (np.median, min, max)] for v in (a, b))


def run_case(k):
    from nsol_amd import linear_operators as LO, ops, tgv_linear_stack as tls
    from nsol_amd.tgv_solver import TGVPrimalDualLinearSolver
    kind, shape, P, epilogue = CASES[k]
    if epilogue is not None:
        LO.USE_BLUR_EPILOGUE = epilogue
    d = len(shape)
    ops_nd = {2: LO.LinearOperators2D, 3: LO.LinearOperators3D}[d]()
    op, _ = ops_nd.get_gaussian_blurring_operators(np.diag([BLUR ** 2] * d))
    out = {"case": k, "kind": kind, "shape": list(shape), "members": P,
           "iterations": ITERS, "epilogue": epilogue, "dtype": "float32"}
    for form in ("batch", "sweep"):
        params = members_of(form, P)
        data = [observation(shape, 1)] * P if form == "sweep" else \
            [observation(shape, m) for m in range(P)]
        made = []

        def solvers():
            return [TGVPrimalDualLinearSolver(alpha=a, beta=b, **arguments(o, op))
                    for o, (a, b) in zip(data, params)]

        def loop():
            return between_events(lambda: [s.run() for s in solvers()])

        def stacked():
            def run():
                if form == "sweep":
                    grid = {"alpha": ALPHAS, "beta": sorted(set(b for _, b in params))}
                    made[:] = [tls.TGVPrimalDualLinearSweep(parameters=grid,
                                                            **arguments(data[0], op))]
                else:
                    made[:] = [tls.TGVPrimalDualLinearBatch(solvers())]
                made[0].run()
            return between_events(run)

        t_loop, t_stack = alternate(loop, stacked)
        execution, G = made[0].get_execution(), made[0].get_group_size() or 1
        template = solvers()[0]
        out[form] = {
            "execution": execution if isinstance(execution, str)
            else sorted(set(execution)),
            "group_size": G, "loop_ms": t_loop, "stacked_ms": t_stack,
            "ratio": round(t_loop[0] / t_stack[0], 2),
            # every group makes its own launches
            "launches_per_iteration_stacked": sum(
                tls.launches_per_iteration(template, b - a)[0]
                for a, b in ops.sweep_groups(P, G)),
            "launches_per_iteration_loop": tls.launches_per_iteration(template, P)[1]}
        del made[:], data, template
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if len(sys.argv) > 2 and sys.argv[1] == "--case":
    import numpy as np, torch
    run_case(int(sys.argv[2]))
else:
    todo = [int(a) for a in sys.argv[1:]] or range(len(CASES))      # e.g. "0 2"
    for k in todo:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case",
                                 str(k)], timeout=CHILD_SECONDS).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            sys.exit("case %d ended with status %d: nothing more is started" % (k, rc))
