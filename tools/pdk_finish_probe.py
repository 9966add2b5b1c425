#!/usr/bin/env python3
"""When do the workgroups of one k_pd_shift3 launch finish?  Needs a library built with
-DNSOL_PDK_FINISH_PROBE (nsol_pdk.hip; nsol_pdk_finish_probe answers -2 otherwise).

  python tools/pdk_finish_probe.py [--size 512] [--pdk 12:4:256] [--rows 0] [--map 1]
  python tools/pdk_finish_probe.py --no-probe ...    the same pinned runs and nothing else,
                                                     with any build: what a rocprofv3 --pmc
                                                     pass of a trimmed footprint runs under

Runs float32 TV-L2 at size^3 through the shifted form with the geometry pinned, reads the
table of the LAST launch and prints one JSON line: per XCD (block mod 8) the finish time of
its last workgroup and the spread of finish times inside it, the finish time of the last
tile row's workgroups, and the launch's length -- all in microseconds from the first
workgroup's start (100 MHz wall clock)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from nsol_amd import _lib, ops  # noqa: E402
from nsol_amd.primal_dual_solver import step_schedule  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--pdk", default="12:4:256")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--map", type=int, default=1)
    ap.add_argument("--no-probe", action="store_true")
    args = ap.parse_args()
    lib = _lib.load()
    n = args.size
    nw, ntx, zchunk = (int(t) for t in args.pdk.split(":"))
    # the footprint of the shifted float32 form (make_tiling): 4 voxels per lane, one halo
    # lane on each side of a row, 5 rows of overlap
    lxb = -(-(-(-n // ntx)) // 4) + 2 if ntx > 1 else n // 4
    rows = args.rows or (nw * 64) // lxb
    valid = rows - 5
    nty, nzc = -(-n // valid), -(-n // zchunk)
    for k, v in (("pdk_nw", nw), ("pdk_ntx", ntx), ("pdk_zchunk", zchunk),
                 ("pdk_rows", args.rows), ("pdk_xcd_map", args.map), ("pdk_shift", 1)):
        _lib.set_param(k, v)
    cap = 8192
    out = (ctypes.c_int * (2 * cap))()
    blocks = lib.nsol_pdk_block_map(args.map, ntx, nty, nzc, out, cap)
    assert blocks > 0, "more blocks than the probe's table holds"
    dev = torch.device("cuda", 0)
    bt = torch.rand(n ** 3, device=dev, dtype=torch.float32)
    x, x_alt = bt.clone(), torch.empty_like(bt)
    xbar = [bt.clone(), torch.empty_like(bt)]
    p = [torch.zeros(3 * n ** 3, dtype=torch.float32, device=dev) for _ in range(2)]
    sig, ta, th = step_schedule("ALG2", 16.0, 1 / 0.03, 31)
    table = (ctypes.c_int64 * (2 * blocks))()
    result = []
    for rep in range(4):                 # the first run is cold; every run's last launch
        ops.pd_run(xbar[0], xbar[1], x, bt, p[0], p[1], (n, n, n), (1.0, 1.0, 1.0),
                   1 / 0.03, sig, ta, th, True, 0.05, ops.PD_REG_TV | ops.PD_DATA_L2,
                   x_alt=x_alt)
        if args.no_probe:
            torch.cuda.synchronize()
            continue
        rc = lib.nsol_pdk_finish_probe(table, 2 * blocks)
        assert rc == 0, "nsol_pdk_finish_probe: %d (built without the probe?)" % rc
        live = [b for b in range(blocks) if out[2 * b] >= 0]
        t0 = min(table[2 * b] for b in live)
        us = lambda t: round((t - t0) / 100.0, 1)   # noqa: E731
        fin = {b: us(table[2 * b + 1]) for b in live}
        per_xcd = []
        for xcd in range(8):
            mine = [fin[b] for b in live if b & 7 == xcd]
            rows_cov = sorted({out[2 * b] // ntx for b in live if b & 7 == xcd})
            per_xcd.append({"xcd": xcd, "blocks": len(mine), "tile_rows": len(rows_cov),
                            "volume_rows": sum(min(valid, n - ty * valid) for ty in rows_cov),
                            "first_finish_us": min(mine), "last_finish_us": max(mine)})
        last_row = [fin[b] for b in live if out[2 * b] // ntx == nty - 1]
        result.append({"launch_us": max(fin.values()), "per_xcd": per_xcd,
                       "last_start_us": max(us(table[2 * b]) for b in live),
                       "last_tile_row_finish_us": [min(last_row), max(last_row)]})
    if args.no_probe:
        return
    print(json.dumps({"size": n, "pdk": args.pdk, "rows": rows, "map": args.map,
                      "tiles": [ntx, nty], "zchunks": nzc, "blocks": blocks,
                      "live_blocks": len(live), "runs": result[1:]}))


if __name__ == "__main__":
    main()
