#!/usr/bin/env python3
"""The shifted block (k_pd_shift3) against the unshifted path in one process on one box.

  python tools/bench_pd_shift.py            run-length sweep at 512^3 and 256^3: ms per run
                                            of N iterations with pdk_shift 0, then 1 (each
                                            after its own plan pass); the curves behind
                                            pdk_shift_min_iters
  python tools/bench_pd_shift.py --plans    bench.py's plan pass (runs of 60 iterations
                                            until nsol_pd_fusedk_tuned says settled) under
                                            the default knobs, then both forms' plans and
                                            the time of 20-iteration runs on them

One JSON line per result on stdout."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from nsol_amd import _lib, ops  # noqa: E402
from nsol_amd.primal_dual_solver import step_schedule  # noqa: E402

NS = [12, 18, 24, 30, 36, 42, 48, 60, 90, 120, 200, 300, 600]


class Volume:
    def __init__(self, n):
        self.shape = (n, n, n)
        dev = torch.device("cuda", 0)
        self.bt = torch.rand(n ** 3, device=dev, dtype=torch.float32)
        self.x = self.bt.clone()
        self.x_alt = torch.empty_like(self.bt)
        self.xbar = [self.bt.clone(), torch.empty_like(self.bt)]
        self.p = [torch.zeros(3 * n ** 3, dtype=torch.float32, device=dev) for _ in range(2)]
        self.lmbda = 1 / 0.03
        self.flags = ops.PD_REG_TV | ops.PD_DATA_L2

    def run(self, iters):
        """ms of one run of `iters` iterations from the initial state"""
        self.x.copy_(self.bt)
        self.xbar[0].copy_(self.bt)
        sig, ta, th = step_schedule("ALG2", 16.0, self.lmbda, iters)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        ops.pd_run(self.xbar[0], self.xbar[1], self.x, self.bt, self.p[0], self.p[1],
                   self.shape, (1.0, 1.0, 1.0), self.lmbda, sig, ta, th, True, 0.05,
                   self.flags, x_alt=self.x_alt, swap_ok=True)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def plan_pass(self, most=8):
        for i in range(most):
            self.run(60)
            if ops.pd_fusedk_tuned(self.x, self.shape) != 0:
                break
        return i + 1


def sweep():
    for n in (512, 256):
        v = Volume(n)
        for shift in (0, 1):
            _lib.set_param("pdk_shift", shift)
            runs = v.plan_pass(10)
            before = ops.pd_shift_launches()
            t = {N: sorted(v.run(N) for _ in range(4)) for N in NS}
            print(json.dumps({
                "size": n, "pdk_shift": shift, "plan": ops.pd_fusedk_plan(v.x, v.shape),
                "plan_runs": runs, "ms_min": {N: round(u[0], 4) for N, u in t.items()},
                "ms_med": {N: round((u[1] + u[2]) / 2, 4) for N, u in t.items()},
                "ms_per_launch_300_600": round((t[600][0] - t[300][0]) / 100, 4),
                "shift_launches": ops.pd_shift_launches() - before}), flush=True)
        del v
        torch.cuda.empty_cache()


def plans():
    for n in (512, 256):
        v = Volume(n)
        runs = v.plan_pass()
        t20 = sorted(v.run(20) for _ in range(5))
        print(json.dumps({
            "size": n, "plan_runs": runs,
            "tuned": ops.pd_fusedk_tuned(v.x, v.shape),
            "plan_shifted": ops.pd_fusedk_plan_form(v.x, v.shape, 1),
            "plan_unshifted": ops.pd_fusedk_plan_form(v.x, v.shape, 0),
            "ms_20_iterations": [round(u, 4) for u in t20]}), flush=True)
        del v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    _lib.load()
    plans() if "--plans" in sys.argv else sweep()
