"""Launch geometry of the depth-3 kernels (k_pd_fusedk, k_pd_shift3): forced footprint
rows (pdk_rows: trimmed footprints) under every block -> tile map (pdk_xcd_map 0 / 1 / 2),
and the online tuner's plan with trimmed candidates on its list.

Everything is held to the one-iteration kernel (pdk_enable=0, pd2_enable=0) with
torch.equal on x, xbar[slot] and p[slot]: the geometry decides which workgroup computes a
voxel, never what is computed, so not a bit may differ."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# two x tiles (pdk_ntx=2), a ragged last tile row (45 rows) and a z-chunk seam (two chunks
# of 12 planes)
SHAPES = [((24, 45, 264), np.float32), ((24, 45, 136), np.float64)]
FORCED = dict(pdk_nw=12, pdk_ntx=2, pdk_zchunk=12)
ITERS = (7, 10)

_KNOBS = dict(pdk_enable=1, pdk_nw=0, pdk_zchunk=0, pdk_ntx=0, pdk_rows=0, pdk_xcd_map=1,
              pdk_min_kvox=1024, pdk_shift=-1, pdk_tune_min_mvox=16)


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()                      # fails loudly if the .so is missing
    return nsol_amd


def _run(shape, dtype, iters, knobs, seed=0):
    """One run of `iters` iterations from the initial state; knobs=None: the
    one-iteration kernel.  Returns (x, xbar, p) of the final state."""
    import torch
    from nsol_amd import ops, _lib
    from nsol_amd.primal_dual_solver import step_schedule
    n = int(np.prod(shape))
    td = torch.float32 if dtype == np.float32 else torch.float64
    gen = torch.Generator(device="cuda").manual_seed(seed)
    bt = torch.rand(n, device="cuda", dtype=td, generator=gen)
    x, x_alt = bt.clone(), torch.empty_like(bt)
    xb = [bt.clone(), torch.empty_like(bt)]
    p = [torch.empty(3 * n, device="cuda", dtype=td) for _ in range(2)]
    sig, ta, th = step_schedule("ALG2", 12.0, 1 / 0.05, iters)
    _lib.set_param("pd2_enable", 0)
    for k, v in dict(_KNOBS, **(knobs if knobs is not None else dict(pdk_enable=0))).items():
        _lib.set_param(k, v)
    try:
        slot = ops.pd_run(xb[0], xb[1], x, bt, p[0], p[1], shape, (1.0, 1.0, 1.0), 20.0,
                          sig, ta, th, True, 0.05, ops.PD_REG_TV | ops.PD_DATA_L2,
                          x_alt=x_alt)
        torch.cuda.synchronize()
    finally:
        _lib.set_param("pd2_enable", 1)
        for k, v in _KNOBS.items():
            _lib.set_param(k, v)
    return x, xb[slot], p[slot]


_REF = {}


def _reference(shape, dtype, iters):
    key = (shape, np.dtype(dtype).name, iters)
    if key not in _REF:
        _REF[key] = _run(shape, dtype, iters, None)
    return _REF[key]


def _max_rows(shape, dtype, shift):
    """Footprint rows that fit a 12-wave workgroup with two tiles along x
    (make_tiling in nsol_pdk.hip)."""
    vw = 16 // np.dtype(dtype).itemsize
    halo = 3 if shift else 2
    hx = -(-halo // vw) * vw
    xv = -(-(-(-shape[2] // 2)) // vw) * vw
    return 768 // (xv // vw + 2 * (hx // vw))


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_forced_rows_and_maps_are_bit_identical(nsol, shape, dtype, shift):
    """pdk_rows 0 (the tiling's own), the maximum - 1, 12 and 6 (6 leaves one valid row per
    tile in the shifted form and two in the unshifted: 45 / 23 tile rows, so the whole-row
    map is on and neighbouring tile rows run on different XCDs), each under all three
    maps, after 7 and after 10 iterations."""
    import torch
    from nsol_amd import ops
    rmax = _max_rows(shape, dtype, shift)
    assert 12 < rmax - 1, rmax
    ran = 0
    for iters in ITERS:
        ref = _reference(shape, dtype, iters)
        launches = (iters - 1) // 3 if shift else iters // 3
        for rows in (0, rmax - 1, 12, 6):
            for xcd_map in (0, 1, 2):
                knobs = dict(FORCED, pdk_min_kvox=0, pdk_shift=shift, pdk_rows=rows,
                             pdk_xcd_map=xcd_map)
                before = (ops.pd_shift_launches(), ops.pd_fusedk_launches(3))
                got = _run(shape, dtype, iters, knobs)
                after = (ops.pd_shift_launches(), ops.pd_fusedk_launches(3))
                # (a forced geometry that does not fit takes the old path)
                assert after[0] - before[0] == (after[1] - before[1] if shift else 0)
                assert after[1] - before[1] in (0, launches), (knobs, before, after)
                ran += int(after[1] - before[1] == launches)
                for name, u, v in zip(("x", "xbar", "p"), got, ref):
                    assert torch.equal(u, v), (shape, iters, knobs, name)
    assert ran >= 1, "no forced geometry fitted this shape"


def test_more_rows_than_fit_take_the_old_path(nsol):
    import torch
    from nsol_amd import ops
    shape, dtype = SHAPES[0]
    before = ops.pd_fusedk_launches(3)
    got = _run(shape, dtype, 7, dict(FORCED, pdk_min_kvox=0, pdk_shift=1,
                                     pdk_rows=_max_rows(shape, dtype, 1) + 1))
    assert ops.pd_fusedk_launches(3) == before
    for u, v in zip(got, _reference(shape, dtype, 7)):
        assert torch.equal(u, v)


def test_plan_with_trimmed_candidates_settles_and_is_bit_identical(nsol):
    """The smallest volume the online tuner takes with pdk_tune_min_mvox = 0 (1 Mi voxels,
    the default pdk_min_kvox): runs of 60 iterations as in bench.py's plan pass until
    nsol_pd_fusedk_tuned reports both forms' plans settled; then a long run (the shifted
    form) and a short one (the unshifted form) under the settled plans."""
    import torch
    from nsol_amd import ops, _lib
    shape, dtype = (32, 128, 256), np.float32
    knobs = dict(pdk_tune_min_mvox=0)
    _lib.set_param("pdk_forget", 1)
    try:
        x = None
        for run in range(40):
            x = _run(shape, dtype, 60, knobs)[0]
            # (_run restores pdk_tune_min_mvox; the plans are asked for under the run's knob)
            _lib.set_param("pdk_tune_min_mvox", 0)
            tuned = ops.pd_fusedk_tuned(x, shape)
            plans = (ops.pd_fusedk_plan_form(x, shape, 1), ops.pd_fusedk_plan_form(x, shape, 0))
            _lib.set_param("pdk_tune_min_mvox", 16)
            if tuned == 1:
                break
        print("plan pass: %d runs of 60 iterations, shifted %s, unshifted %s"
              % (run + 1, plans[0], plans[1]))
        assert tuned == 1, "the plans did not settle in 40 runs of 60 iterations"
        assert plans[0] is not None and plans[1] is not None
        for iters, shifted in ((31, 10), (20, 0)):
            before = (ops.pd_shift_launches(), ops.pd_fusedk_launches(3))
            got = _run(shape, dtype, iters, knobs)
            assert ops.pd_shift_launches() - before[0] == shifted
            assert ops.pd_fusedk_launches(3) - before[1] == (shifted or iters // 3)
            for name, u, v in zip(("x", "xbar", "p"), got, _reference(shape, dtype, iters)):
                assert torch.equal(u, v), (iters, name)
    finally:
        _lib.set_param("pdk_forget", 1)
