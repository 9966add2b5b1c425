#!/usr/bin/env python3
"""The blur-and-sample operator pair (SampledConvolutionOperator, nsol_sample.hip)
against the composition it replaces, float32, on the GPU:

  A      new: the operator's passes (ops.corr_axis_down, then ops.corr_axis on the
         reduced grid); composed: ConvolutionOperator, then a strided .contiguous();
  A^T    new: the passes backwards (ops.corr_axis, ops.corr_axis_up); composed: a
         zero-fill of the fine grid, then the adjoint ConvolutionOperator;
  PDL    one PrimalDualLinearSolver iteration, `fused` on the operator pair against
         `device` mode on the composed callables (wall time of run() with a
         synchronisation at its end over the iteration count).

Configurations: a 512^3 fine grid with factors (4,1,1) and (2,2,2), Gaussian taps
13x5x5 and 13x13x13; a 256^2 fine grid with factors (2,2), taps 13x13.

Every configuration runs in a child process of its own under `timeout`; after a child
that fails nothing more is started.  Times come from device events around INNER calls,
after a warm-up, REPS times per form with the two forms alternating; reported are the
median and the spread (min, max) in milliseconds per call.  Bytes are counted from the
shapes (every pass reads its input once and writes its output once) and stated next to
the times; "of_peak" is those bytes over the median time over 8 TB/s -- for an operator
of several passes a whole-operator figure, for the single passes a kernel's.  Nothing
gates on these numbers; DESIGN.md section 4h records them.  One JSON line per
configuration, also appended to FILE with `--out FILE`.

    python tools/bench_sampled_blur.py [--out FILE] [configuration indices]"""
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

PEAK = 8.0e12           # bytes / s, HBM3E of the MI355X
CONFIGS = [
    dict(fine=(512, 512, 512), factors=(4, 1, 1), taps=(13, 5, 5)),
    dict(fine=(512, 512, 512), factors=(4, 1, 1), taps=(13, 13, 13)),
    dict(fine=(512, 512, 512), factors=(2, 2, 2), taps=(13, 5, 5)),
    dict(fine=(512, 512, 512), factors=(2, 2, 2), taps=(13, 13, 13)),
    dict(fine=(256, 256), factors=(2, 2), taps=(13, 13)),
]
CHILD_LIMIT = 240       # seconds per configuration
REPS, INNER, WARM = 7, 10, 3
PDL_ITERS = 20


def gaussian_taps(n):
    import numpy as np
    half = (n - 1) // 2
    t = np.exp(-0.5 * (np.arange(-half, half + 1) / (half / 3.)) ** 2)
    return t / t.sum()


def dense(ks):
    import numpy as np
    out = ks[0]
    for k in ks[1:]:
        out = np.multiply.outer(out, k)
    return out


def timed(forms):
    """{name: (median, min, max) ms per call} of the callables in `forms`, alternating."""
    import numpy as np
    import torch
    for fn in forms.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(REPS):
        for name, fn in forms.items():
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            for _ in range(INNER):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / INNER)
    return {name: (float(np.median(v)), float(min(v)), float(max(v)))
            for name, v in ms.items()}


def row(t, nbytes):
    med, lo, hi = t
    return dict(ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                bytes=int(nbytes), of_peak=round(nbytes / (med * 1e-3) / PEAK, 3))


def blur_bytes(op, n, item):
    """Bytes of ConvolutionOperator on n elements: 8 per element and launch."""
    return 2 * item * n * max(op._launches(None), 1)


def child(index):
    import time
    import numpy as np
    import torch
    from nsol_amd import ops
    from nsol_amd.linear_operators import (ConvolutionOperator,
                                           SampledConvolutionOperator)
    from nsol_amd.primal_dual_linear_solver import PrimalDualLinearSolver
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    cfg = CONFIGS[index]
    fine, factors = cfg["fine"], cfg["factors"]
    d, item = len(fine), 4
    ks = [gaussian_taps(n) for n in cfg["taps"]]
    kernel = dense(ks)
    A = SampledConvolutionOperator(d, kernel, factors)
    At = A.adjoint(fine)
    coarse = A._out_shape(fine)
    blur = ConvolutionOperator(d, kernel)
    blur_adj = ConvolutionOperator(d, kernel[tuple([slice(None, None, -1)] * d)])
    sl = tuple(slice(0, None, f) for f in factors)
    n, m = int(np.prod(fine)), int(np.prod(coarse))
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(n, dtype=torch.float32, device="cuda", generator=gen)
    q = torch.rand(m, dtype=torch.float32, device="cuda", generator=gen)

    def composed_A(t):
        return blur(t.view(*fine))[sl].contiguous().reshape(-1)

    def composed_At(v):
        z = torch.zeros(fine, dtype=v.dtype, device=v.device)
        z[sl] = v.view(*coarse)
        return blur_adj(z).reshape(-1)
    # the two forms compute the same thing (float32, different summation orders)
    ref, got = composed_A(x), A._apply(x, fine)
    err_A = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
    ref, got = composed_At(q), At._apply(q, coarse)
    err_At = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
    assert err_A < 1e-5 and err_At < 1e-5, (err_A, err_At)
    del ref, got

    # ---- bytes from the shapes, pass by pass, and the single passes' own times
    passes, shape, down_bytes = {}, list(fine), 0
    src = x
    for a in A._down:
        out_shape = list(shape)
        out_shape[a] = ops.sampled_extent(shape[a], factors[a], 0)
        nin, nout = int(np.prod(shape)), int(np.prod(out_shape))
        dst = torch.empty(nout, dtype=torch.float32, device="cuda")
        small = torch.rand(nout, dtype=torch.float32, device="cuda", generator=gen)
        big = torch.empty(nin, dtype=torch.float32, device="cuda")
        args = (a + 3 - d, A._taps[a], A._centre[a], "wrap", factors[a], 0)
        t = timed({
            "down": lambda s=src, sh=tuple(shape), o=dst: ops.corr_axis_down(
                s, sh, *args, out=o),
            "up": lambda s=small, sh=tuple(shape), o=big: ops.corr_axis_up(
                s, sh, *args, out=o)})
        nb = item * (nin + nout)
        passes["down axis %d f %d taps %d on %s" % (a, factors[a], A._taps[a].size,
                                                  "x".join(map(str, shape)))] = \
            row(t["down"], nb)
        passes["up axis %d f %d taps %d onto %s" % (a, factors[a], A._taps[a].size,
                                                  "x".join(map(str, shape)))] = \
            row(t["up"], nb)
        down_bytes += nb
        src, shape = dst, out_shape
        del small, big
    plain_bytes = 2 * item * int(np.prod(shape)) * len(A._plain)
    new_bytes = down_bytes + plain_bytes
    copy_bytes = 2 * item * m
    fill_bytes = item * n + 2 * item * m
    out = dict(cfg, coarse=list(coarse), dtype="float32", rel_l2_A=err_A,
               rel_l2_At=err_At, passes=passes)
    t = timed({"new": lambda: A._apply(x, fine), "composed": lambda: composed_A(x)})
    out["A_new"] = row(t["new"], new_bytes)
    out["A_composed"] = row(t["composed"], blur_bytes(blur, n, item) + copy_bytes)
    t = timed({"new": lambda: At._apply(q, coarse), "composed": lambda: composed_At(q)})
    out["At_new"] = row(t["new"], new_bytes)
    out["At_composed"] = row(t["composed"], blur_bytes(blur_adj, n, item) + fill_bytes)
    for k in ("A", "At"):
        out[k + "_speedup"] = round(out[k + "_composed"]["ms"] / out[k + "_new"]["ms"], 2)

    # ---- one PDL iteration, fused against device mode
    b = A._apply(x, fine)

    def solver(fused):
        if fused:
            fa = lambda v: A(v.reshape(*fine)).flatten()
            fb = lambda v: At(v.reshape(*coarse)).flatten()
            extra = {}
        else:
            def fa(v):
                if not isinstance(v, torch.Tensor):
                    raise TypeError("device tensors only")
                return composed_A(v)

            def fb(v):
                if not isinstance(v, torch.Tensor):
                    raise TypeError("device tensors only")
                return composed_At(v)
            extra = dict(A_norm2=1., shape=fine)
        return PrimalDualLinearSolver(fa, fb, b, x, d, alpha=0.05, iterations=PDL_ITERS,
                                      dtype=np.float32, **extra)

    def wall(s):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / PDL_ITERS
    walls = {"fused": [], "device": []}
    for rep in range(4):                      # the first of each is the warm-up
        for name in walls:
            s = solver(name == "fused")
            w = wall(s)
            assert s.get_execution() == name, (name, s.get_execution())
            if rep:
                walls[name].append(w)
            del s
    for name, v in walls.items():
        out["pdl_" + name] = dict(ms_per_iteration=round(float(np.median(v)), 4),
                                  min_ms=round(min(v), 4), max_ms=round(max(v), 4))
    out["pdl_speedup"] = round(out["pdl_device"]["ms_per_iteration"] /
                               out["pdl_fused"]["ms_per_iteration"], 2)
    print(json.dumps(out), flush=True)


def main(argv):
    if argv and argv[0] == "--child":
        return child(int(argv[1]))
    log = None
    if "--out" in argv:
        k = argv.index("--out")
        log = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    indices = [int(a) for a in argv] or range(len(CONFIGS))
    for i in indices:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable,
               os.path.abspath(__file__), "--child", str(i)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:
            print("configuration %d ended with status %d: nothing more is started" %
                  (i, res.returncode), file=sys.stderr)
            return res.returncode
        if log is not None:
            with open(log, "a") as f:
                f.write(res.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
