#!/usr/bin/env python3
"""Device SSIM and MI / NMI histograms (nsol_measures.hip) at 512^3 float32.

SSIM: the volume as 3-D and as the flattened 1-D array the CLIs pass.
Histograms at 100 x 100 bins: the range pass, the joint-histogram pass and the
whole ops.histogram2d(..., marginals=True) call, on random data and on the
zero-background phantom64 tiled to 512^3 (waves that all hit one bin).
Device times: HIP events, median of --reps warm calls.  Effective bandwidth
counts one read of both inputs (2 x 4 bytes per voxel).  Host: the SciPy /
NumPy restatement of the same call, timed once (--no-host skips it).
Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from nsol_amd import ops  # noqa: E402


def dev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def host_s(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def ssim_host(x, y, win=7):
    from scipy.ndimage import uniform_filter
    X, Y = x.astype(np.float64), y.astype(np.float64)
    npix = win ** X.ndim
    cn = npix / (npix - 1.0)
    ux, uy = uniform_filter(X, win), uniform_filter(Y, win)
    uxx, uyy, uxy = (uniform_filter(X * X, win), uniform_filter(Y * Y, win),
                     uniform_filter(X * Y, win))
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    C1, C2 = (0.01 * 2) ** 2, (0.03 * 2) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) *
                                                 (vx + vy + C2))
    p = (win - 1) // 2
    return S[tuple(slice(p, n - p) for n in S.shape)].mean()


def report(case, ms, n, host=None, extra=None):
    out = {"case": case, "device_ms": round(ms, 4),
           "effective_GBps": round(2 * 4 * n / (ms * 1e-3) / 1e9, 1)}
    if host is not None:
        out["host_s"] = round(host, 3)
    out.update(extra or {})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    n = args.n
    shape = (n, n, n)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(shape, device="cuda", generator=g, dtype=torch.float32)
    y = (0.8 * x + 0.2 * torch.randn(shape, device="cuda", generator=g)).contiguous()
    hx = hy = None
    if not args.no_host:
        hx, hy = x.cpu().numpy(), y.cpu().numpy()
    N = x.numel()
    npix3, npix1 = 343.0, 7.0
    C1, C2 = (0.01 * 2) ** 2, (0.03 * 2) ** 2
    xf, yf = x.view(-1), y.view(-1)

    for case, shp, npix in (("ssim_3d", shape, npix3), ("ssim_1d_flat", (N,), npix1)):
        fn = lambda: ops.ssim_sum(xf, yf, shp, 7, C1, C2, npix / (npix - 1))
        ms = dev_ms(fn, args.reps)
        host = None if args.no_host else host_s(lambda: ssim_host(hx.reshape(shp),
                                                                  hy.reshape(shp)))
        report(case, ms, N, host)

    ph = np.load(os.path.join(ROOT, "tests", "golden", "configs.npz"))["phantom64"]
    rep = n // ph.shape[0]
    pt = torch.from_numpy(ph).cuda().repeat(rep, rep, rep).contiguous()
    noise = torch.randn(pt.shape, device="cuda", generator=g)
    pn = torch.where(pt == 0, pt, pt + 0.05 * noise).contiguous()
    for case, a, b in (("hist_random", xf, yf),
                       ("hist_phantom_tiled", pt.view(-1), pn.view(-1))):
        r = ops.pair_range(a, b)
        ex, ey = ops.hist2d_edges(r[0:2], r[2:4], np.float32, np.float32, 100)
        zero_frac = float((a == 0).float().mean().item())
        report(case + "_range_pass", dev_ms(lambda: ops.pair_range(a, b), args.reps),
               a.numel())
        report(case + "_hist_pass",
               dev_ms(lambda: ops.hist2d_counts(a, b, ex, ey), args.reps), a.numel(),
               extra={"zero_fraction_x": round(zero_frac, 3)})
        host = None
        if not args.no_host:
            an, bn = a.cpu().numpy(), b.cpu().numpy()
            host = host_s(lambda: (np.histogram2d(an, bn, 100), np.histogram(an, 100),
                                   np.histogram(bn, 100)))
        report(case + "_histogram2d_marginals",
               dev_ms(lambda: ops.histogram2d(a, b, 100, marginals=True), args.reps),
               a.numel(), host)


if __name__ == "__main__":
    main()
