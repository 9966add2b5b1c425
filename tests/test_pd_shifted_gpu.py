"""The shifted depth-3 form (k_pd_shift3, nsol_pdk.hip): a long run is cut after the
dual step, so a launch runs P D P D P D on (x, p) alone -- no xbar crosses it.

nsol_pd_run_* sends N iterations through (N - 1) mod 3 leading iterations, a
stand-alone dual step, m = (N - 1) // 3 shifted launches and a stand-alone primal
step.  Everything here holds that run to the one-iteration kernel
(primal_dual_solver.py:242-256 per launch; pdk_enable=0, pd2_enable=0) with
torch.equal on x, xbar[slot] and p[slot]: the arithmetic per voxel and its order are
the same, so not a bit may differ.  Small volumes reach the kernel with
pdk_min_kvox=0, and pdk_shift=1 takes the block from 4 iterations on."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [
    ((20, 30, 256), np.float32),
    ((17, 9, 512), np.float32),     # fewer volume rows than footprint rows
    ((9, 70, 264), np.float32),     # an x tile that is not a whole wave
    ((64, 64, 64), np.float32),
    ((16, 40, 32), np.float32),
    ((8, 8, 1280), np.float32),     # the minimum z and y
    ((21, 13, 132), np.float64),
    ((10, 37, 256), np.float64),
]
ITERS = [4, 5, 6, 7, 10, 11, 12]    # every (N - 1) mod 3, m = 1 .. 3

_PDK_DEFAULTS = dict(pdk_enable=1, pdk_kmax=3, pdk_nw=0, pdk_zchunk=0, pdk_ntx=0,
                     pdk_min_kvox=1024, pdk_shift=-1, pdk_shift_min_iters=30,
                     pdk_tune_min_mvox=16)


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()                      # fails loudly if the .so is missing
    return nsol_amd


def _state(shape, dtype, seed=0):
    import torch
    n = int(np.prod(shape))
    td = torch.float32 if dtype == np.float32 else torch.float64
    gen = torch.Generator(device="cuda").manual_seed(seed)
    bt = torch.rand(n, device="cuda", dtype=td, generator=gen)
    return dict(bt=bt, x=bt.clone(), xb=[bt.clone(), torch.empty_like(bt)],
                p=[torch.empty(3 * n, device="cuda", dtype=td) for _ in range(2)],
                slot=0, done=0)


def _advance(st, shape, iters, flags, w, pdk, total=None, x_alt=True, swap_ok=False):
    """`iters` more iterations of the state's run (one schedule of `total` iterations
    for the whole run).  pdk=None: the one-iteration kernel, the reference."""
    import torch
    from nsol_amd import ops, _lib
    from nsol_amd.primal_dual_solver import step_schedule
    total = total or iters
    sig, ta, th = step_schedule("ALG2", 12.0, 1 / 0.05, total)
    lo, hi = st["done"], st["done"] + iters
    _lib.set_param("pd2_enable", 0)
    knobs = dict(_PDK_DEFAULTS, **(dict(dict(pdk_min_kvox=0), **pdk) if pdk is not None
                                   else dict(pdk_enable=0)))
    for k, v in knobs.items():
        _lib.set_param(k, v)
    try:
        a = st["slot"]
        alt = torch.empty_like(st["x"]) if x_alt else None
        end = ops.pd_run(st["xb"][a], st["xb"][1 - a], st["x"], st["bt"], st["p"][a],
                         st["p"][1 - a], shape, w, 20.0, sig[lo:hi], ta[lo:hi], th[lo:hi],
                         lo == 0, 0.05, flags, x_alt=alt, swap_ok=swap_ok)
        torch.cuda.synchronize()
    finally:
        _lib.set_param("pd2_enable", 1)
        for k, v in _PDK_DEFAULTS.items():
            _lib.set_param(k, v)
    st["slot"] = a ^ end
    st["done"] = hi
    return st


def _same(a, b, what):
    import torch
    for name, u, v in (("x", a["x"], b["x"]),
                       ("xbar", a["xb"][a["slot"]], b["xb"][b["slot"]]),
                       ("p", a["p"][a["slot"]], b["p"][b["slot"]])):
        assert torch.equal(u, v), (what, name)


_REF = {}


def _reference(shape, dtype, runs, flags, w):
    """The one-iteration kernel's states after each of `runs` (iteration counts of
    consecutive runs on one state); computed once per key, never modified."""
    key = (shape, np.dtype(dtype).name, tuple(runs), flags, w)
    if key not in _REF:
        st = _state(shape, dtype)
        out = []
        for n in runs:
            _advance(st, shape, n, flags, w, None, total=sum(runs))
            out.append(dict(x=st["x"].clone(), xb=[t.clone() for t in st["xb"]],
                            p=[t.clone() for t in st["p"]], slot=st["slot"]))
        _REF[key] = out
    return _REF[key]


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_shifted_run_is_bit_identical(nsol, shape, dtype, iters):
    """Every remainder (N - 1) mod 3 and m = 1 .. 3, from p = 0 and -- a second run on
    the state the first one left -- from a dual variable that is read; with no forced
    tiling the shifted-launch counter rises by exactly m per run."""
    from nsol_amd import ops
    flags = ops.PD_REG_TV | ops.PD_DATA_L2
    w = (1.0, 1.0, 1.0)
    ref = _reference(shape, dtype, (iters, iters), flags, w)
    st = _state(shape, dtype)
    for run in range(2):
        before, before3 = ops.pd_shift_launches(), ops.pd_fusedk_launches(3)
        _advance(st, shape, iters, flags, w, dict(pdk_shift=1), total=2 * iters)
        m = (iters - 1) // 3
        assert ops.pd_shift_launches() == before + m, "the shifted form did not run"
        # (the leading (N - 1) mod 3 iterations never take a depth-3 launch)
        assert ops.pd_fusedk_launches(3) == before3 + m
        _same(st, ref[run], (shape, iters, "run %d" % run))


@pytest.mark.parametrize("nw", [12, 8])
@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_shifted_forced_geometry_is_bit_identical(nsol, shape, dtype, nw):
    """z-chunk seams shorter than the pipeline (chunks of 4 and 5 planes), one to three
    tiles along x, both workgroup sizes, all four flag combinations, each with unit
    spacing and with (1.0, 0.5, 2.0) in both orders.  8 iterations: one leading
    iteration, two launches."""
    from nsol_amd import ops
    iters, m = 8, 2
    forced_ran = 0
    spacings = [(1.0, 1.0, 1.0), (1.0, 0.5, 2.0), (2.0, 0.5, 1.0)]
    # every flag combination with every spacing on the default tiling and one forced
    # tiling with seams (all 16 instantiations of this type and workgroup size); the
    # remaining forced geometries once per flag combination
    for fi, flags in enumerate((ops.PD_REG_HUBER | ops.PD_DATA_L1,
                                ops.PD_REG_TV | ops.PD_DATA_L2,
                                ops.PD_REG_TV | ops.PD_DATA_L1,
                                ops.PD_REG_HUBER | ops.PD_DATA_L2)):
        for wi, w in enumerate(spacings):
            ref = _reference(shape, dtype, (iters,), flags, w)
            cfgs = [dict(), dict(pdk_ntx=2, pdk_zchunk=4)]
            if wi == fi % 3:
                cfgs += [dict(pdk_zchunk=4), dict(pdk_zchunk=5), dict(pdk_ntx=1),
                         dict(pdk_ntx=3)]
            for cfg in cfgs:
                cfg = dict(dict(pdk_shift=1, pdk_nw=nw), **cfg)
                before = ops.pd_shift_launches()
                st = _advance(_state(shape, dtype), shape, iters, flags, w, cfg)
                ran = ops.pd_shift_launches() == before + m
                # (a forced tiling may not fit a shape; the run then takes the old path)
                assert ran or "pdk_ntx" in cfg, ("k_pd_shift3 did not run", cfg)
                forced_ran += int(ran and "pdk_ntx" in cfg)
                _same(st, ref[0], (shape, cfg, flags, w))
    # (rows of more than 4 KiB need more than the three tiles forced above: the rule of
    # test_k_iterations_per_pass_is_bit_identical)
    assert forced_ran >= 1 or shape[2] * np.dtype(dtype).itemsize > 4096, \
        "no forced tiling fitted this shape"


@pytest.mark.parametrize("swap_ok", [False, True])
@pytest.mark.parametrize("x_alt", [True, False])
def test_shifted_run_hands_back_the_standard_state(nsol, x_alt, swap_ok):
    """The returned slot names the buffers that hold the final xbar and p, x names the
    final iterate whether or not the tensors may trade storage, and an unshifted run
    continues from that state exactly as the reference does.  Without x_alt no
    multi-iteration kernel runs at all: the old path."""
    from nsol_amd import ops
    shape, dtype = (20, 30, 256), np.float32
    flags = ops.PD_REG_TV | ops.PD_DATA_L2
    w = (1.0, 1.0, 1.0)
    for iters in (7, 11):
        ref = _reference(shape, dtype, (iters, 5), flags, w)
        st = _state(shape, dtype)
        before = ops.pd_shift_launches()
        _advance(st, shape, iters, flags, w, dict(pdk_shift=1), total=iters + 5,
                 x_alt=x_alt, swap_ok=swap_ok)
        assert ops.pd_shift_launches() == before + ((iters - 1) // 3 if x_alt else 0)
        _same(st, ref[0], (iters, x_alt, swap_ok))
        before = ops.pd_shift_launches()
        _advance(st, shape, 5, flags, w, dict(pdk_shift=0), total=iters + 5)
        assert ops.pd_shift_launches() == before
        _same(st, ref[1], (iters, x_alt, swap_ok, "continued"))


@pytest.mark.parametrize("shape,dtype,flag", [
    ((20, 30, 258), np.float32, 0), ((21, 13, 131), np.float64, 0),
    ((20, 30, 256), np.float32, "iso"), ((20, 30, 256), np.float32, "weighted")])
def test_declined_forms_take_the_old_path(nsol, shape, dtype, flag):
    """Ragged rows, the isotropic projection and weighted data terms: nothing shifted
    is launched and the results are those of the one-iteration kernel."""
    import torch
    from nsol_amd import ops, _lib
    iters = 8
    before = ops.pd_shift_launches()
    if flag == "weighted":
        from nsol_amd.primal_dual_solver import step_schedule
        flags = ops.PD_REG_TV | ops.PD_DATA_L2 | ops.PD_DATA_WEIGHTED
        sig, ta, th = step_schedule("ALG2", 12.0, 1 / 0.05, iters)
        got = []
        for shift in (0, 1):
            st = _state(shape, dtype)
            wt = torch.rand(st["bt"].numel(), device="cuda", dtype=st["bt"].dtype,
                            generator=torch.Generator(device="cuda").manual_seed(5))
            _lib.set_param("pdk_min_kvox", 0)
            _lib.set_param("pdk_shift", shift)
            slot = ops.pd_weighted_run(st["xb"][0], st["xb"][1], st["x"], st["bt"], wt,
                                       st["p"][0], st["p"][1], 1, shape, (1.0, 1.0, 1.0),
                                       20.0, sig, ta, th, True, 0.05, flags)
            torch.cuda.synchronize()
            got.append((st["x"], st["xb"][slot], st["p"][slot]))
        for u, v in zip(*got):
            assert torch.equal(u, v)
    else:
        flags = ops.PD_REG_TV | ops.PD_DATA_L2 | \
            (ops.PD_REG_ISOTROPIC if flag == "iso" else 0)
        w = (1.0, 1.0, 1.0)
        ref = _reference(shape, dtype, (iters,), flags, w)
        st = _advance(_state(shape, dtype), shape, iters, flags, w, dict(pdk_shift=1))
        _same(st, ref[0], (shape, flag))
    assert ops.pd_shift_launches() == before


def test_block_starts_at_the_threshold_by_default(nsol):
    """pdk_shift=-1: a run below pdk_shift_min_iters launches nothing shifted, a run of
    exactly that length does (the volume counts as one the online tuner handles)."""
    from nsol_amd import ops
    shape, dtype = (20, 30, 256), np.float32
    flags = ops.PD_REG_TV | ops.PD_DATA_L2
    w = (1.0, 1.0, 1.0)
    knobs = dict(pdk_shift=-1, pdk_shift_min_iters=10, pdk_tune_min_mvox=0,
                 pdk_autotune=0)
    for iters, m in ((9, 0), (10, 3)):
        ref = _reference(shape, dtype, (iters,), flags, w)
        before, before3 = ops.pd_shift_launches(), ops.pd_fusedk_launches(3)
        st = _advance(_state(shape, dtype), shape, iters, flags, w, knobs)
        assert ops.pd_shift_launches() == before + m
        assert ops.pd_fusedk_launches(3) == before3 + 3
        _same(st, ref[0], iters)
    # ... and not at all on a volume below the tuner's size, whatever the length
    before = ops.pd_shift_launches()
    _advance(_state(shape, dtype), shape, 10, flags, w,
             dict(pdk_shift=-1, pdk_shift_min_iters=10))
    assert ops.pd_shift_launches() == before
