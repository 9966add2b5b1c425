#!/usr/bin/env python3
"""Dense-tap correlation: the tiled kernel (nsol_corr_dense_tiled_*) against the plain one
(nsol_corr_dense_*) in one process, alternated round by round, medians with both extremes.

    python tools/bench_conv_dense.py [--rounds R] [--quick]

Cases: float32 and float64; (20, 24, 40), 32^3, 64^3, 128^3 and 256^3 under a 3^3, a 7^3
and the 7 x 13 x 17 oriented Gaussian (R diag(1, 1, 9) R^T, R a 30 degree rotation); 256^2,
512^2 and 2048^2 under 9 x 9 and 31 x 31 (the small shapes are where a launch has fewer
workgroups than the chip has CUs: the planner's workgroup threshold comes from them); then
one PrimalDualLinearSolver iteration on the oriented Gaussian at 256^3 with the switch
linear_operators.USE_TILED_DENSE off and on.  One JSON line per case.

tap_outputs_per_s = voxels * taps / time.  The VALU bound it is held against is one
multiply and one add per tap-output, each a lane-instruction: 256 CUs x 64 lanes x 2.4 GHz
/ 2 = 19.66e12 tap-outputs/s (float32 compiled to packed v_pk_mul_f32 / v_pk_add_f32
does two per lane-instruction pair: 39.3e12)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nsol_amd import ops                                     # noqa: E402
from nsol_amd import kernels as K                            # noqa: E402
import nsol_amd.linear_operators as LO                       # noqa: E402

VALU_PAIRS_PER_S = 256 * 64 * 2.4e9 / 2


def oriented_gaussian():
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    R = np.array([[1., 0., 0.], [0., c, -s], [0., s, c]])
    return K.Kernels3D().get_gaussian(cov=R @ np.diag([1., 1., 9.]) @ R.T)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(float(min(ts)), 4),
            "max": round(float(max(ts)), 4)}


def bench_case(name, shape, kernel, dt, rounds):
    rng = np.random.default_rng(0)
    A = LO.ConvolutionOperator(len(shape), kernel)
    assert not A.separable, name
    n = int(np.prod(shape))
    x = torch.from_numpy(rng.standard_normal(n)).to(dt).cuda()
    taps = torch.from_numpy(A._flipped.reshape(-1)).to(dt).cuda()
    k3, c3 = A._dense3()
    plan = ops.corr_dense_tiled_plan(shape, k3, x.element_size())
    forms = {"plain": lambda: ops.corr_dense(x, shape, taps, k3, c3, "wrap")}
    out = torch.empty_like(x)
    tile = (0, 0, 0)
    if plan is None:          # a class the planner declines: timed on a forced tile
        tile = (32, 64, 16)
        plan = ops.corr_dense_tiled_plan(shape, k3, x.element_size(), tile)
    forms["tiled"] = lambda: ops.corr_dense_tiled(x, shape, taps, k3, c3, "wrap",
                                                  tile=tile, out=out)
    # same bits, at the size that is timed
    ref = forms["plain"]()
    assert forms["tiled"]() is not None
    same = bool(torch.equal(ref.view(torch.int32), out.view(torch.int32)))
    del ref
    work = float(n) * kernel.size
    reps = {}
    for f, fn in forms.items():
        fn()
        torch.cuda.synchronize()
        reps[f] = max(1, min(500, int(60.0 / max(timed(fn, 1), 1e-3))))
    ts = {f: [] for f in forms}
    for _ in range(rounds):
        for f, fn in forms.items():
            ts[f].append(timed(fn, reps[f]))
    res = {f: stats(v) for f, v in ts.items()}
    rate = work / (res["tiled"]["median"] * 1e-3)
    print(json.dumps({
        "case": name, "dtype": str(dt).split(".")[-1], "shape": list(shape),
        "taps": list(kernel.shape), "planner_takes_it": tile == (0, 0, 0),
        "plan": plan, "bits_equal": same, "ms": res,
        "speedup": round(res["plain"]["median"] / res["tiled"]["median"], 2),
        "tiled_tap_outputs_per_s": float("%.4g" % rate),
        "plain_tap_outputs_per_s": float("%.4g" % (work / (res["plain"]["median"] * 1e-3))),
        "tiled_share_of_valu_bound": round(rate / VALU_PAIRS_PER_S, 3)}), flush=True)


def bench_pdl(shape, kernel, rounds, iterations=4):
    import nsol_amd
    rng = np.random.default_rng(1)
    obs = 1. + rng.random(shape)
    lo = LO.LinearOperators3D()
    A, At = lo.get_convolution_and_adjoint_convolution_operators(kernel, exact_adjoint=True)

    def run():
        s = nsol_amd.PrimalDualLinearSolver(
            A=lambda v: A(v.reshape(*shape)).flatten(),
            A_adj=lambda v: At(v.reshape(*shape)).flatten(),
            b=torch.from_numpy(obs.reshape(-1)).cuda(),
            x0=torch.from_numpy(obs.reshape(-1)).cuda(), dimension=3, alpha=0.05,
            iterations=iterations, dtype=np.float32)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.run()
        e1.record()
        torch.cuda.synchronize()
        assert s.get_execution() == "fused"
        return e0.elapsed_time(e1) / iterations, s.get_x()
    ts, xs = {"plain": [], "tiled": []}, {}
    for r in range(rounds + 1):
        for form in ts:
            LO.USE_TILED_DENSE = form == "tiled"
            t, xs[form] = run()
            if r:
                ts[form].append(t)
    LO.USE_TILED_DENSE = True
    res = {f: stats(v) for f, v in ts.items()}
    print(json.dumps({
        "case": "one PDL iteration, oriented Gaussian", "dtype": "float32",
        "shape": list(shape), "taps": list(kernel.shape),
        "bits_equal": bool(np.array_equal(xs["plain"], xs["tiled"])), "ms_per_iteration": res,
        "speedup": round(res["plain"]["median"] / res["tiled"]["median"], 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="without 256^3 and 2048^2")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    rng = np.random.default_rng(2)
    og = oriented_gaussian()
    for dt in (torch.float32, torch.float64):
        shapes = [(20, 24, 40), (32,) * 3, (64,) * 3, (128,) * 3]
        for shape in shapes if args.quick else shapes + [(256,) * 3]:
            for name, k in (("3^3", rng.random((3, 3, 3))), ("7^3", rng.random((7, 7, 7))),
                            ("oriented Gaussian", og)):
                bench_case("%s at %s" % (name, "x".join(map(str, shape))), shape, k, dt,
                           args.rounds)
        for m in (256, 512) if args.quick else (256, 512, 2048):
            for k in (9, 31):
                bench_case("%d x %d at %d^2" % (k, k, m), (m, m), rng.random((k, k)), dt,
                           args.rounds)
    n = 128 if args.quick else 256
    bench_pdl((n, n, n), og, max(2, args.rounds - 2))


if __name__ == "__main__":
    main()
