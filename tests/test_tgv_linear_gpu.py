"""TGV behind a linear operator and weighted TGV on the GPU: k_tgv_primal's LIN and WGT
forms through the C ABI against the NumPy restatement (tgv_numpy.primal_step_lin /
primal_step_weighted) on every access path, weights of 0 over garbage, unit weights
against the plain entry, guard bands, the float32 box, the entries that must decline;
TGVPrimalDualLinearSolver against tgv_numpy.iterate_linear in its execution forms, its
stopping rule, observers and masking; TGVPrimalDualSolver(weights=); the command line."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from device_arena import Arena
from nsol_amd import tgv_numpy as tg
from test_pd_linear_host import box_kernel, gaussian_kernel
from test_pd_weighted_host import mixed_weights
from test_sampled_conv_host import numpy_start, sampled_adjoint, sampled_forward
from test_tgv_gpu import (BETA, BOTH, F32_TOL, F64_TOL, L1, SHAPES, SPACING, TAU, THETA, TL,
                          _dims, _gate, _iw, _obs, _rounded_spacing, _suffix)
from test_tgv_gpu import _state as _tgv_state

pytestmark = pytest.mark.gpu

# LIN: a finite box, a half-open one and none (the scaled state is N(0, 1))
BOXES = [(-0.4, 0.5), (0., np.inf), (-np.inf, np.inf)]
_WORST32 = {}


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


@functools.lru_cache(maxsize=None)
def _state(shape, dtype):
    """test_tgv_gpu's state (rounded to dtype, held in float64) with g = A^T r in bt's
    place for the LIN form and weights, about a fifth of them exactly 0, for WGT.  Never
    modified."""
    rng = np.random.default_rng(2000 + sum(shape) + len(shape))
    st = dict(_tgv_state(shape, dtype))
    rnd = lambda a: a.astype(dtype).astype(np.float64)
    st["g"] = rnd(0.8 * rng.standard_normal(shape))
    wt = rng.uniform(0.05, 3., shape)
    wt[rng.uniform(size=shape) < 0.2] = 0.
    st["wt"] = rnd(wt)
    for v in st.values():
        v.setflags(write=False)
    return st


def _c(dtype, v):
    return float(np.dtype(dtype).type(v))


@functools.lru_cache(maxsize=None)
def _want_lin(shape, dtype, box):
    s = _state(shape, dtype)
    return tg.primal_step_lin(s["p"], s["q"], s["x"], s["w"], s["g"], _c(dtype, TAU),
                              _c(dtype, THETA), box[0], box[1],
                              _rounded_spacing(shape, dtype), dtype)


@functools.lru_cache(maxsize=None)
def _want_w(shape, dtype, l1):
    s = _state(shape, dtype)
    return tg.primal_step_weighted(s["p"], s["q"], s["x"], s["w"], s["bt"], s["wt"],
                                   _c(dtype, TAU), _c(dtype, TL), _c(dtype, THETA),
                                   _rounded_spacing(shape, dtype), "ell1" if l1 else "ell2")


LIN_ARRAYS = ("p", "q", "x", "xbar", "w", "wbar", "g")
WGT_ARRAYS = ("p", "q", "x", "xbar", "w", "wbar", "bt", "wt")


def _call_lin(shape, dtype, ar, box, tau=TAU, theta=THETA):
    from nsol_amd import _lib
    from nsol_amd.device import stream_ptr
    fn = getattr(_lib.load(), "nsol_tgv_primal_lin_" + _suffix(dtype))
    return fn(*[ar.ptr(k) for k in LIN_ARRAYS], *_dims(shape), *_iw(len(shape)), tau, theta,
              box[0], box[1], stream_ptr())


def _call_w(shape, dtype, ar, flags, tau=TAU, tl=TL, theta=THETA):
    from nsol_amd import _lib
    from nsol_amd.device import stream_ptr
    fn = getattr(_lib.load(), "nsol_tgv_primal_w_" + _suffix(dtype))
    return fn(*[ar.ptr(k) for k in WGT_ARRAYS], *_dims(shape), *_iw(len(shape)), tau, tl,
              theta, flags, stream_ptr())


def _compare(ar, want, s, inputs, dtype, label):
    errs = [rel_l2(ar.get(k, v.shape), v, label + " " + k)
            for k, v in zip(("x", "xbar", "w", "wbar"), want)]
    print("%s %s: x %.3g xbar %.3g w %.3g wbar %.3g" % ((label, _suffix(dtype)) + tuple(errs)))
    if np.dtype(dtype) == np.float32:
        form = label.split(" ")[0]
        _WORST32[form] = max(_WORST32.get(form, 0.), max(errs))
    assert max(errs) <= _gate(dtype)
    assert ar.guards_intact()
    for k in inputs:                                    # the inputs are only read
        assert np.array_equal(ar.get(k, s[k].shape), s[k]), k


def _check_lin(shape, dtype, box, offset=0, last=None):
    import torch
    s = _state(shape, dtype)
    ar = Arena({k: s[k] for k in LIN_ARRAYS}, dtype, offset, last)
    assert _call_lin(shape, dtype, ar, box) == 0
    torch.cuda.synchronize()
    _compare(ar, _want_lin(shape, dtype, box), s, ("p", "q", "g"), dtype,
             "lin %r box=%r off=%d last=%s" % (shape, box, offset, last))


def _check_w(shape, dtype, l1, offset=0, last=None):
    import torch
    s = _state(shape, dtype)
    ar = Arena({k: s[k] for k in WGT_ARRAYS}, dtype, offset, last)
    assert _call_w(shape, dtype, ar, L1 if l1 else 0) == 0
    torch.cuda.synchronize()
    _compare(ar, _want_w(shape, dtype, l1), s, ("p", "q", "bt", "wt"), dtype,
             "wgt %r l1=%d off=%d last=%s" % (shape, l1, offset, last))


# ------------------------------------------------------------ 1. single kernel calls
def test_the_state_straddles_the_box_and_the_weights():
    for shape in ((259,), (6, 259), (4, 6, 259)):
        s = _state(shape, np.float64)
        kx, _ = tg.K_adj(s["p"], s["q"], SPACING[:len(shape)])
        u = s["x"] - TAU * (kx + s["g"])
        lo, hi = BOXES[0]
        shares = (float(np.mean(u < lo)), float(np.mean((u >= lo) & (u <= hi))),
                  float(np.mean(u > hi)))
        assert min(shares) > 0.05, (shape, shares)
        assert 0 < float(np.mean(u < BOXES[1][0])) < 1
        zero = float(np.mean(s["wt"] == 0))
        assert 0.1 < zero < 0.3, (shape, zero)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_lin_kernel_matches_numpy(nsol, shape, dtype):
    for box in BOXES:
        _check_lin(shape, dtype, box)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_weighted_kernel_matches_numpy(nsol, shape, dtype):
    for l1 in (False, True):
        _check_w(shape, dtype, l1)


def test_the_largest_float32_errors(nsol):
    """(for DESIGN section 4j; runs after the two tests above)"""
    print("largest float32 relative l2 error of a single call:", _WORST32)


# ------------------------------------------------------------------------ 2. weights
@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (4, 6, 259)])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("l1", [False, True])
def test_a_zero_weight_hides_what_the_observation_holds(nsol, shape, dtype, l1):
    import torch
    s = _state(shape, dtype)
    zero = s["wt"] == 0
    assert zero.any()
    clean = np.where(zero, 0., s["bt"])
    junk = clean.copy()
    junk[zero] = np.resize([np.nan, np.inf, -np.inf], int(zero.sum()))
    got = {}
    for name, bt in (("clean", clean), ("junk", junk)):
        ar = Arena(dict({k: s[k] for k in WGT_ARRAYS}, bt=bt), dtype)
        assert _call_w(shape, dtype, ar, L1 if l1 else 0) == 0
        torch.cuda.synchronize()
        got[name] = [ar.get(k, s[k].shape) for k in ("x", "xbar", "w", "wbar")]
        assert ar.guards_intact()
    for a, b in zip(got["clean"], got["junk"]):
        assert np.isfinite(b).all()
        assert np.array_equal(a, b)
    # ... and the voxel keeps u = x - tau K^T p
    kx, _ = tg.K_adj(s["p"], s["q"], _rounded_spacing(shape, dtype))
    u = s["x"] - _c(dtype, TAU) * kx
    assert rel_l2(got["junk"][0][zero], u[zero]) <= _gate(dtype)


@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (4, 6, 259), (5, 4, 64)])
@pytest.mark.parametrize("l1", [False, True])
def test_unit_weights_give_the_bits_of_the_plain_entry_in_float64(nsol, shape, l1):
    import torch
    from nsol_amd import _lib
    from nsol_amd.device import stream_ptr
    dtype = np.float64
    s = _state(shape, dtype)
    ar = Arena(dict({k: s[k] for k in WGT_ARRAYS}, wt=np.ones(shape)), dtype)
    assert _call_w(shape, dtype, ar, L1 if l1 else 0) == 0
    plain = Arena({k: s[k] for k in WGT_ARRAYS[:-1]}, dtype)
    fn = _lib.load().nsol_tgv_primal_f64
    assert fn(*[plain.ptr(k) for k in WGT_ARRAYS[:-1]], *_dims(shape), *_iw(len(shape)),
              TAU, TL, THETA, L1 if l1 else 0, stream_ptr()) == 0
    torch.cuda.synchronize()
    for k in ("x", "xbar", "w", "wbar"):
        assert np.array_equal(ar.get(k, s[k].shape), plain.get(k, s[k].shape)), k


# ---------------------------------------------------------------- 3. guards and ends
@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (5, 4, 64), (3, 5, 8)])
@pytest.mark.parametrize("dtype", BOTH)
def test_arrays_off_16_byte_alignment(nsol, shape, dtype):
    _check_lin(shape, dtype, BOXES[0], offset=1)
    _check_w(shape, dtype, False, offset=3)


@pytest.mark.parametrize("shape", [(259,), (6, 259), (4, 6, 259), (3, 5, 7), (5, 4, 64)])
@pytest.mark.parametrize("dtype", BOTH)
def test_stacks_that_end_with_their_allocation(nsol, shape, dtype):
    """Every array in turn ends exactly where the device allocation ends."""
    for last in LIN_ARRAYS:
        _check_lin(shape, dtype, BOXES[1], last=last)
    for last in WGT_ARRAYS:
        _check_w(shape, dtype, True, last=last)


@pytest.mark.parametrize("shape", [(259,), (4, 6, 259)])
def test_a_float32_box_is_rounded_towards_its_inside(nsol, shape):
    """-0.1 rounds DOWN to float32 and 0.6 UP: rounded to nearest, both ends would let
    iterates out of the caller's float64 box."""
    import torch
    from nsol_amd import vector_numpy as vn
    dtype, box = np.float32, (-0.1, 0.6)
    assert float(np.float32(box[0])) < box[0] and float(np.float32(box[1])) > box[1]
    s = _state(shape, dtype)
    ar = Arena({k: s[k] for k in LIN_ARRAYS}, dtype)
    assert _call_lin(shape, dtype, ar, box) == 0
    torch.cuda.synchronize()
    x = ar.get("x", shape)
    assert x.min() >= box[0] and x.max() <= box[1]
    lo, hi = vn.box_in(box[0], box[1], np.float32)       # one float32 spacing inside
    assert box[0] < lo < box[0] + 1e-7 and box[1] - 1e-7 < hi < box[1]
    assert (x == lo).any() and (x == hi).any()
    assert rel_l2(x, _want_lin(shape, dtype, box)[0]) <= F32_TOL


# ------------------------------------------------------------------------ 4. declines
@pytest.mark.parametrize("dtype", BOTH)
def test_the_new_entries_decline(nsol, dtype):
    import torch
    from nsol_amd import _lib, ops
    from nsol_amd.device import stream_ptr, to_device
    lib = _lib.load()
    lin = getattr(lib, "nsol_tgv_primal_lin_" + _suffix(dtype))
    wgt = getattr(lib, "nsol_tgv_primal_w_" + _suffix(dtype))
    shape = (3, 4, 6)
    n = 3 * 4 * 6
    mk = lambda k: to_device(np.full(k * n, 0.25), dtype)
    p, q, x, xbar, w, wbar, bt, wt = mk(3), mk(6), mk(1), mk(1), mk(3), mk(3), mk(1), mk(1)
    every = (p, q, x, xbar, w, wbar, bt, wt)
    ptr = lambda t: None if t is None else t.data_ptr()
    good_l, good_w = (p, q, x, xbar, w, wbar, bt), every

    def cl(a=good_l, dims=(3,) + shape, tau=0.3, theta=1., lo=-1., hi=1.):
        return lin(*[ptr(t) for t in a], *dims, 1., 1., 1., tau, theta, lo, hi,
                   stream_ptr())

    def cw(a=good_w, dims=(3,) + shape, tau=0.3, tl=0.5, theta=1., flags=0):
        return wgt(*[ptr(t) for t in a], *dims, 1., 1., 1., tau, tl, theta, flags,
                   stream_ptr())

    before = ops.tgv_launches()
    for call, good in ((cl, good_l), (cw, good_w)):
        for k in range(len(good)):                       # a missing pointer
            a = list(good)
            a[k] = None
            assert call(a) == -1, k
        for i in range(len(good)):                       # two arguments that alias
            for j in range(i):
                a = list(good)
                a[i] = a[j]
                assert call(a) == -1, (i, j)
    assert cl((p, q, x, xbar, w, w[n:], bt)) == -1       # ... or overlap
    assert cw((p, q, x, xbar, w, wbar, bt, q[5 * n:])) == -1
    for bad in (0., -0.3, np.inf, np.nan):
        assert cl(tau=bad) == -1 and cw(tau=bad) == -1, bad
    for bad in (np.inf, np.nan):
        assert cl(theta=bad) == -1 and cw(theta=bad) == -1, bad
    assert cw(tl=-0.1) == -1 and cw(tl=np.nan) == -1 and cw(tl=np.inf) == -1
    assert cl(lo=1., hi=0.) == -1 and cl(lo=np.nan) == -1 and cl(hi=np.nan) == -1
    for flags in (1, 4, 8, 0x100, L1 | 4, L1 | 8):       # Huber, isotropic, weighted, run
        assert cw(flags=flags) == -1, flags
    for dims in ((0,) + shape, (4,) + shape, (2,) + shape, (1, 1, 4, 6), (3, -1, 4, 6)):
        assert cl(dims=dims) == -1 and cw(dims=dims) == -1, dims
    # more than 2^31 voxels: declined, nothing launched
    for dims in ((3, 1 << 11, 1 << 11, 1 << 10), (1, 1, 1, (1 << 31) + 1),
                 (2, 1, 1 << 20, (1 << 11) + 1), (3, 1 << 40, 1 << 40, 1 << 40)):
        assert cl(dims=dims) == -2 and cw(dims=dims) == -2, dims
    # an extent of 0: nothing to do, whatever else is passed
    for dims in ((3, 0, 4, 6), (3, 3, 0, 6), (1, 1, 1, 0)):
        assert cl(dims=dims) == 0 and cw(dims=dims) == 0
        assert cl((None,) * 7, dims=dims) == 0 and cw((None,) * 8, dims=dims) == 0
    torch.cuda.synchronize()
    assert ops.tgv_launches() == before
    for t in every:
        assert torch.equal(t, torch.full_like(t, 0.25))
    # and the good calls run: infinite ends, lo == hi, tl = 0, the l1 flag
    assert cl() == 0 and cl(lo=-np.inf, hi=np.inf) == 0 and cl(lo=0.5, hi=0.5) == 0
    assert cw(tl=0.) == 0 and cw(flags=L1) == 0
    torch.cuda.synchronize()
    assert ops.tgv_launches() == before + 5
    # the Python wrappers check their operands before the library sees them
    iw = (1., 1., 1.)
    other = np.float32 if dtype is np.float64 else np.float64
    with pytest.raises(ValueError):
        ops.tgv_primal_lin(p, q, x, xbar, w, wbar[:2 * n], bt, shape, iw, 0.3)
    with pytest.raises(ValueError):
        ops.tgv_primal_lin(p, q, x, xbar, w, wbar, to_device(np.zeros(n), other), shape,
                           iw, 0.3)
    with pytest.raises(ValueError):
        ops.tgv_primal_w(p, q, x, xbar, w, wbar, bt, wt[:n - 1], shape, iw, 0.3, 0.5)
    with pytest.raises(ValueError):
        ops.tgv_primal_w(p, q[:3 * n], x, xbar, w, wbar, bt, wt, shape, iw, 0.3, 0.5)
    with pytest.raises(ValueError):
        ops.tgv_primal_lin(p, q, x, xbar, w, wbar, bt, shape, iw, 0.3, lo=1., hi=0.)
    # -2 comes back as False
    assert ops.tgv_primal_lin(p, q, x, xbar, w, wbar, bt, shape, iw, 0.3) is True


# ------------------------------------------------------- 5. the solver behind A
SOLVER_SHAPES = [(5, 7), (3, 5, 7), (4, 6, 259)]
SAMPLED = {(5, 7): (1, 2), (4, 6, 259): (2, 1, 3)}          # factors per array axis
X_SCALE, ALPHA, ITERS = 2.0, 0.3, 25
BOX = (0.25, 0.85)                                           # of the scaled variable


def _kernel_for(shape):
    return box_kernel(len(shape)) if min(shape) < 7 else gaussian_kernel(len(shape), 1.)


def _sampled_taps(shape):
    return [gaussian_kernel(1, 1.) if s >= 7 else np.array([0.25, 0.5, 0.25])
            for s in shape]


def _outer(ks):
    out = ks[0]
    for k in ks[1:]:
        out = np.multiply.outer(out, k)
    return out


@functools.lru_cache(maxsize=None)
def _problem(shape, sampled):
    """(obs, x0, weights, numpy A, numpy A^T): the observation of test_tgv_gpu blurred (and
    sampled), the start the command line would form.  Never modified."""
    from scipy.ndimage import convolve
    truth = _obs(shape)
    rng = np.random.default_rng(31 + sum(shape))
    if sampled:
        ks, f, o = _sampled_taps(shape), SAMPLED[shape], (0,) * len(shape)
        A = lambda x: sampled_forward(np.asarray(x, np.float64).reshape(shape), ks, "wrap",
                                      f, o)
        obs = A(truth)
        At = lambda r: sampled_adjoint(np.asarray(r, np.float64).reshape(obs.shape), ks,
                                       "wrap", f, o, shape)
        obs = obs + 0.02 * rng.standard_normal(obs.shape)
        x0 = numpy_start(obs, ks, "wrap", f, o, shape)
    else:
        k = _kernel_for(shape)
        A = At = lambda x: convolve(np.asarray(x, np.float64).reshape(shape), k,
                                    mode="wrap")
        obs = A(truth) + 0.02 * rng.standard_normal(shape)
        x0 = obs.copy()
    wt = mixed_weights(obs.shape, 5)
    for a in (obs, x0, wt):
        a.setflags(write=False)
    return obs, x0, wt, A, At


@functools.lru_cache(maxsize=None)
def _restated(shape, sampled, iso, data, wb, iterations=ITERS, keep=False):
    obs, x0, wt, A, At = _problem(shape, sampled)
    return tg.iterate_linear(A, At, obs.reshape(-1) / X_SCALE, x0 / X_SCALE, iterations,
                             ALPHA, BETA, SPACING[:len(shape)], data, iso, keep=keep,
                             weights=wt.reshape(-1) if wb else None,
                             bounds=BOX if wb else None, A_norm2=1.)


def _device_operators(shape, sampled):
    from nsol_amd.linear_operators import ConvolutionOperator, SampledConvolutionOperator
    if sampled:
        A = SampledConvolutionOperator(len(shape), _outer(_sampled_taps(shape)),
                                       SAMPLED[shape], (0,) * len(shape))
        return A, A.adjoint(shape)
    A = ConvolutionOperator(len(shape), _kernel_for(shape))
    return A, A


def _solver(nsol, shape, dtype, sampled=False, iso=False, data="ell2", wb=False, **kw):
    obs, x0, wt, _, _ = _problem(shape, sampled)
    A, At = _device_operators(shape, sampled)
    coarse = obs.shape
    args = dict(A=lambda x: A(x.reshape(*shape)).flatten(),
                A_adj=lambda r: At(r.reshape(*coarse)).flatten(), b=obs.flatten(),
                x0=x0.flatten(), dimension=len(shape), spacing=SPACING[:len(shape)],
                alpha=ALPHA, beta=BETA, iterations=ITERS, data_loss=data, isotropic=iso,
                x_scale=X_SCALE, dtype=dtype, shape=shape)
    if wb:
        args.update(weights=wt.flatten(), bounds=BOX)
    args.update(kw)
    return nsol.TGVPrimalDualLinearSolver(**args)


def _against(s, want, dtype, label):
    ex = rel_l2(s.get_x(), want["x"] * X_SCALE, label + " x")
    ew = rel_l2(s.get_w(), want["w"] * X_SCALE, label + " w")
    print("%s %s: x %.3g w %.3g" % (label, _suffix(dtype), ex, ew))
    assert ex <= _gate(dtype) and ew <= _gate(dtype)


@pytest.mark.parametrize("shape", SOLVER_SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("data", ["ell2", "ell1"])
@pytest.mark.parametrize("wb", [False, True], ids=["plain", "weights+box"])
def test_solver_matches_the_restatement(nsol, shape, dtype, iso, data, wb):
    from nsol_amd import ops
    s = _solver(nsol, shape, dtype, False, iso, data, wb)
    assert s.get_execution() == "fused" and s.get_A_norm2() == pytest.approx(1., abs=1e-12)
    before = ops.tgv_launches()
    s.run()
    assert ops.tgv_launches() == before + 2 * ITERS
    want = _restated(shape, False, iso, data, wb)
    _against(s, want, dtype, "solver %r iso=%d %s wb=%d" % (shape, iso, data, wb))
    assert s.get_iterations_done() == ITERS and s.get_stop_reason() == "iterations"
    assert s.get_execution() == "fused" and len(s.get_changes()) == 0
    assert np.linalg.norm(want["w"]) > 0.01 * np.linalg.norm(want["x"])   # w is at work
    if wb:
        x = s.get_x() / X_SCALE
        assert x.min() >= BOX[0] * (1 - 1e-6) and x.max() <= BOX[1] * (1 + 1e-6)
        # the box is active (the 35 pixels of the 2-D case stay below its upper end)
        assert (want["x"] == BOX[0]).any()
        assert len(shape) < 3 or (want["x"] == BOX[1]).any()


@pytest.mark.parametrize("shape", sorted(SAMPLED))
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("iso,data,wb", [(False, "ell2", False), (True, "ell1", True),
                                         (False, "ell1", True), (True, "ell2", False)])
def test_solver_on_a_sampled_operator(nsol, shape, dtype, iso, data, wb):
    s = _solver(nsol, shape, dtype, True, iso, data, wb)
    assert s.get_execution() == "fused" and s.get_shape() == shape
    s.run()
    assert s.get_x().shape == (int(np.prod(shape)),)
    _against(s, _restated(shape, True, iso, data, wb), dtype,
             "sampled %r iso=%d %s wb=%d" % (shape, iso, data, wb))


EPILOGUE = [((9, 5, 16), 4., np.float64), ((20, 37, 64), 2., np.float32)]


@pytest.mark.parametrize("shape, var, dtype", EPILOGUE)
def test_blur_epilogue_on_and_off(nsol, monkeypatch, shape, var, dtype):
    from scipy.ndimage import convolve
    from nsol_amd import linear_operators as LO, ops
    A, _ = LO.LinearOperators3D().get_gaussian_blurring_operators(np.diag([var] * 3))
    obs = _obs(shape)
    wt = mixed_weights(shape, 1)
    ran = []
    real = ops.corr3_wrap_axpby

    def counted(*a, **k):
        out = real(*a, **k)
        ran.append(out is not None)
        return out
    monkeypatch.setattr(ops, "corr3_wrap_axpby", counted)
    wrapped = lambda x: A(x.reshape(*shape)).flatten()
    got = {}
    for on in (True, False):
        monkeypatch.setattr(LO, "USE_BLUR_EPILOGUE", on)
        del ran[:]
        s = nsol.TGVPrimalDualLinearSolver(
            wrapped, wrapped, obs.flatten(), obs.flatten(), 3, alpha=ALPHA, beta=BETA,
            iterations=ITERS, weights=wt.flatten(), bounds=BOX, x_scale=X_SCALE, dtype=dtype)
        s.run()
        assert s.get_execution() == "fused"
        assert ran == ([True] * ITERS if on else [])
        got[on] = s
    blur = lambda x: convolve(np.asarray(x, np.float64).reshape(shape), A.kernel,
                              mode="wrap")
    want = tg.iterate_linear(blur, blur, obs.reshape(-1) / X_SCALE, obs / X_SCALE, ITERS,
                             ALPHA, BETA, weights=wt.reshape(-1), bounds=BOX,
                             A_norm2=got[True].get_A_norm2())
    for on in (True, False):
        _against(got[on], want, dtype, "epilogue=%d %r" % (on, shape))
    assert rel_l2(got[True].get_x(), got[False].get_x()) <= _gate(dtype)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("shape,sampled", [((4, 6, 259), False), ((4, 6, 259), True),
                                           ((5, 7), True)])
def test_fused_against_device_and_host_callables(nsol, dtype, shape, sampled):
    """The same operators behind opaque callables (device tensors only), and a NumPy-only
    pair, with A_norm2 given."""
    from nsol_amd.device import is_device_tensor
    obs, _, _, A_np, At_np = _problem(shape, sampled)
    A, At = _device_operators(shape, sampled)
    coarse = obs.shape

    def opaque(op, shp):
        def f(t):
            if not is_device_tensor(t):
                raise TypeError("device tensors only")
            return op(t.view(*shp)).reshape(-1)
        return f
    kw = dict(data="ell1", wb=True)
    fused = _solver(nsol, shape, dtype, sampled, **kw)
    with pytest.raises(ValueError, match="A_norm2"):
        _solver(nsol, shape, dtype, sampled, A=opaque(A, shape), A_adj=opaque(At, coarse),
                **kw)
    dev = _solver(nsol, shape, dtype, sampled, A=opaque(A, shape), A_adj=opaque(At, coarse),
                  A_norm2=1., **kw)
    host = _solver(nsol, shape, dtype, sampled, A=lambda v: A_np(v).reshape(-1),
                   A_adj=lambda v: At_np(v).reshape(-1), A_norm2=1., **kw)
    want = _restated(shape, sampled, False, "ell1", True)
    for s, name in ((fused, "fused"), (dev, "device"), (host, "host")):
        s.run()
        assert s.get_execution() == name
        _against(s, want, dtype, "%s %r sampled=%d" % (name, shape, sampled))
    for s in (dev, host):
        assert rel_l2(s.get_x(), fused.get_x()) <= _gate(dtype)
        assert rel_l2(s.get_w(), fused.get_w()) <= _gate(dtype)


def test_solver_takes_device_tensors_and_zero_iterations(nsol):
    from nsol_amd.device import to_device
    shape = (5, 7)
    obs, x0, _, _, _ = _problem(shape, False)
    s = _solver(nsol, shape, np.float64, b=to_device(obs.flatten(), np.float64),
                x0=to_device(x0.flatten(), np.float64))
    s.run()
    _against(s, _restated(shape, False, False, "ell2", False), np.float64, "device data")
    s = _solver(nsol, shape, np.float64, iterations=0)
    s.run()
    assert np.array_equal(s.get_x(), x0.flatten()) and not s.get_w().any()
    assert s.get_iterations_done() == 0


# ------------------------------------------------------------------------ 6. stopping
@pytest.mark.parametrize("shape,sampled", [((5, 7), False), ((3, 5, 7), False),
                                           ((5, 7), True)])
def test_solver_stops_where_the_restatement_does(nsol, shape, sampled):
    iters, every = 60, 5
    want = _restated(shape, sampled, False, "ell2", True, iters)
    points = list(range(every, iters + 1, every))
    worst = [float(max(want["ratios"][k - 1, 1:])) for k in points]
    # stop at the fourth check point: the tolerance is the geometric mean of its change
    # and the smallest one before it, so rounding cannot move the decision
    j = 3
    assert worst[j] < 0.9 * min(worst[:j])
    tol = float(np.sqrt(worst[j] * min(worst[:j])))
    stop = points[j]
    s = _solver(nsol, shape, np.float64, sampled, wb=True, iterations=iters, tolerance=tol,
                check_every=every)
    s.run()
    assert s.get_iterations_done() == stop and s.get_stop_reason() == "tolerance"
    ch = s.get_changes()
    assert list(ch[:, 0]) == points[:j + 1]
    # (the dual ratio holds r: without it the restatement's column is another number)
    np.testing.assert_allclose(ch[:, 1:], want["ratios"][[k - 1 for k in points[:j + 1]],
                                                         1:], rtol=1e-10, atol=0)
    plain = _solver(nsol, shape, np.float64, sampled, wb=True, iterations=stop)
    plain.run()
    assert np.array_equal(plain.get_x(), s.get_x())
    assert np.array_equal(plain.get_w(), s.get_w())
    # a tolerance that is never met: all iterations, the last one checked
    s = _solver(nsol, shape, np.float64, sampled, iterations=12, tolerance=0.,
                check_every=5)
    s.run()
    assert s.get_iterations_done() == 12 and s.get_stop_reason() == "iterations"
    assert list(s.get_changes()[:, 0]) == [5, 10, 12]


# ----------------------------------------------------------------------- 7. observers
def test_observers_in_both_modes(nsol):
    from nsol_amd.observer import Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as SM
    shape, iters = (4, 6, 259), 9
    ref = (_obs(shape) + 0.05).flatten()
    measures = lambda: {k: (lambda x, k=k: SM.similarity_measures[k](x, ref))
                        for k in ("SSD", "RMSE", "PSNR", "NCC", "MAE")}
    host = Observer()
    host.set_measures(measures())
    s = _solver(nsol, shape, np.float64, wb=True, iterations=iters)
    s.set_observer(host)
    s.run()
    host.compute_measures()
    assert host.get_observed_iterations() == list(range(iters + 1))
    want = _restated(shape, False, False, "ell2", True, iters, True)["iterates"]
    hv = host.get_measures()
    for k in (0, 1, iters):
        assert hv["SSD"][k] == pytest.approx(
            SM.similarity_measures["SSD"](want[k].flatten() * X_SCALE, ref), rel=1e-10)
    for every in (1, 4):
        dev = Observer(keep_iterates=False, every=every)
        dev.set_measures(measures())
        s = _solver(nsol, shape, np.float64, wb=True, iterations=iters)
        s.set_observer(dev)
        s.run()
        dev.compute_measures()
        pts = dev.get_observed_iterations()
        assert pts == sorted(set(list(range(0, iters + 1, every)) + [iters]))
        for k, v in dev.get_measures().items():
            np.testing.assert_allclose(np.asarray(v), np.asarray(hv[k])[pts], rtol=1e-10,
                                       atol=0, err_msg=k)


# ------------------------------------------------------------------------- 8. masking
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("data", ["ell2", "ell1"])
@pytest.mark.parametrize("shape,sampled", [((4, 6, 259), False), ((5, 7), True)])
def test_masked_out_nan_never_reaches_x(nsol, dtype, data, shape, sampled):
    obs, x0, wt, _, _ = _problem(shape, sampled)
    zero = wt == 0
    assert zero.any()
    clean, holed = np.where(zero, 0., obs), np.where(zero, np.nan, obs)
    runs = []
    for b in (clean, holed):
        s = _solver(nsol, shape, dtype, sampled, data=data, wb=True, b=b.flatten())
        s.run()
        runs.append((s.get_x(), s.get_w()))
    assert np.isfinite(runs[1][0]).all() and np.isfinite(runs[1][1]).all()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


# ------------------------------------------------- 9. TGVPrimalDualSolver(weights=...)
def _denoiser(nsol, shape, dtype, iso=False, data="ell2", **kw):
    obs = _obs(shape)
    args = dict(b=obs.flatten(), x0=obs.flatten(), dimension=len(shape), shape=shape,
                spacing=SPACING[:len(shape)], alpha=ALPHA, beta=BETA, iterations=ITERS,
                data_loss=data, isotropic=iso, x_scale=X_SCALE, dtype=dtype)
    args.update(kw)
    return nsol.TGVPrimalDualSolver(**args)


@functools.lru_cache(maxsize=None)
def _restated_weighted(shape, iso, data):
    obs = _obs(shape)
    return tg.iterate(obs / X_SCALE, obs / X_SCALE, ITERS, ALPHA, BETA,
                      SPACING[:len(shape)], data, iso, weights=mixed_weights(shape, 4))


@pytest.mark.parametrize("shape", SOLVER_SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("iso,data", [(False, "ell2"), (True, "ell1"), (False, "ell1"),
                                      (True, "ell2")])
def test_weighted_denoiser_matches_the_restatement(nsol, shape, dtype, iso, data):
    from nsol_amd import ops
    wt = mixed_weights(shape, 4)
    s = _denoiser(nsol, shape, dtype, iso, data, weights=wt.flatten())
    before = ops.tgv_launches()
    s.run()
    assert ops.tgv_launches() == before + 2 * ITERS
    _against(s, _restated_weighted(shape, iso, data), dtype,
             "weighted denoiser %r iso=%d %s" % (shape, iso, data))
    # a masked-out NaN in b changes nothing
    holed = np.where(wt == 0, np.nan, _obs(shape))
    h = _denoiser(nsol, shape, dtype, iso, data, weights=wt.flatten(), b=holed.flatten())
    h.run()
    assert np.array_equal(h.get_x(), s.get_x()) and np.array_equal(h.get_w(), s.get_w())


@pytest.mark.parametrize("shape", SOLVER_SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_no_weights_is_the_loop_over_the_two_plain_entries(nsol, shape, dtype):
    """weights=None: the bits of k_tgv_dual / k_tgv_primal called in a loop, the solver's
    path before it took weights."""
    import torch
    from nsol_amd import ops
    from nsol_amd.device import to_device, to_numpy
    from nsol_amd.proximal_operators import scaled_data_on_device
    s = _denoiser(nsol, shape, dtype, data="ell1")
    s.run()
    d, n = len(shape), int(np.prod(shape))
    M = tg.components(d)
    obs = _obs(shape).flatten()
    mk = lambda k: to_device(np.zeros(k * n), dtype)
    x = scaled_data_on_device(obs.copy(), X_SCALE, mk(1)).clone()
    bt = x.clone()
    xbar, w, wbar, p, q = x.clone(), mk(d), mk(d), mk(d), mk(M)
    iw = ops.inv_spacing(np.asarray(SPACING[:d]), d)
    for _ in range(ITERS):
        assert ops.tgv_dual(xbar, wbar, p, q, shape, iw, s.get_sigma(), BETA, 0)
        assert ops.tgv_primal(p, q, x, xbar, w, wbar, bt, shape, iw, s.get_tau(),
                              s.get_tau() / ALPHA, 1., ops.PD_DATA_L1)
    torch.cuda.synchronize()
    assert np.array_equal(s.get_x(), to_numpy(ops.scale(x, X_SCALE)))
    assert np.array_equal(s.get_w(), to_numpy(ops.scale(w, X_SCALE)))


# -------------------------------------------------------------------- 10. command line
def test_cli_tgv_deconvolution_writes_the_solvers_result(nsol, tmp_path, capsys):
    from nsol_amd.application import run_deconvolution as rd
    obs = _obs((8, 9)) + 1.0
    mask = np.ones((8, 9))
    mask[2:4, 3:6] = 0
    src, out, mfile = (str(tmp_path / f) for f in ("obs.npy", "out.npy", "mask.npy"))
    np.save(src, obs)
    np.save(mfile, mask)
    base = ["--observation", src, "--result", out, "--solver", "PDL",
            "--reconstruction-type", "TGVL2", "--beta", "1.5", "--iterations", "15",
            "--alpha", "0.2", "--blur", "1.0"]
    assert rd.main(base + ["--mask", mfile, "--nonnegative"]) == 0
    assert "TGVL2" in capsys.readouterr().out
    s = rd.build_solver(obs, np.ones(2), 1.0, "TGVL2", "PDL", 0.2, 15, dtype=np.float32,
                        weights=mask, nonnegative=True, beta=1.5)
    s.run()
    assert type(s) is nsol.TGVPrimalDualLinearSolver and s.get_execution() == "fused"
    assert s.get_beta() == 1.5 and s.get_bounds() == (0., np.inf)
    got = np.load(out)
    assert got.shape == obs.shape
    assert rel_l2(got, s.get_x().reshape(obs.shape)) < 1e-6
    assert rel_l2(got, obs) > 1e-3                       # it did something
    # the other options, and several alphas in a loop
    assert rd.main(base[:-4] + ["--alpha", "0.1", "0.2", "--isotropic", "--dtype",
                                "float64", "--data-loss", "ell1", "--tolerance", "1e-2",
                                "--check-every", "4", "--reference", src,
                                "--observe-every", "5", "--iterations", "20"]) == 0
    text = capsys.readouterr().out
    assert text.count("TGVL2 alpha=") == 2 and "stopped after" in text and "RMSE" in text
    with pytest.raises(SystemExit) as e:
        rd.main(base + ["--slice-wise"])
    assert e.value.code != 0 and "--slice-wise" in capsys.readouterr().err


def test_cli_tgv_super_resolution(nsol, tmp_path, capsys):
    from nsol_amd.application import run_deconvolution as rd
    obs = _obs((6, 9)) + 1.0
    src, out = str(tmp_path / "obs.npy"), str(tmp_path / "out.npy")
    np.save(src, obs)
    assert rd.main(["--observation", src, "--result", out, "--solver", "PDL",
                    "--reconstruction-type", "TGVL2", "--iterations", "15", "--alpha",
                    "0.2", "--blur", "1.0", "--upsample", "2", "1"]) == 0
    s = rd.build_solver(obs, np.ones(2), 1.0, "TGVL2", "PDL", 0.2, 15, dtype=np.float32,
                        upsample=[2, 1])
    s.run()
    assert s.get_shape() == (12, 9) and s.get_execution() == "fused"
    np.testing.assert_allclose(s.get_spacing(), [1., 0.5])
    got = np.load(out)
    assert got.shape == (12, 9)
    assert rel_l2(got, s.get_x().reshape(12, 9)) < 1e-6
