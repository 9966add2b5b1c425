"""The generic vector kernels of csrc/nsol_ops.hip -- the parts most of the GPU suite
measures fused kernels against -- each beside a float64 reference of its own
(nsol_amd/vector_numpy.py, anchored on the oracle and the goldens by
test_vector_ops_host.py): lincomb2/3, scale, clip, extrapolate, prox_ell1/ell2,
prox_dual_clamp, dot/norm2, loss_cost_grad, loss_eval, vector_shrink, vector_norm_sum,
pair_stats, diff_axis, grad, grad_adj, grad_adj_axpy.

Through the C ABI on arrays in a guard-band arena (device_arena.py), at the lengths where
a grid-stride kernel can go wrong (one element, one workgroup -1 / +0 / +1, a second and
a partial third trip, the grid cap crossed, more partial sums than k_reduce_final has
threads), on and off 16-byte alignment, with values planted on every branch, and once
through every ops.* wrapper.  The gates are derived in vector_cases.py, per element.
"""
import functools
import math

import numpy as np
import pytest

import vector_cases as vc
from device_arena import Arena, SENTINEL
from nsol_amd import vector_numpy as vn

pytestmark = pytest.mark.gpu

BOTH = [np.float64, np.float32]
LENGTHS = [1, 3, 255, 256, 257, 1021]
N_TRIPS = 2 * 256 * 2 + 37          # with max_grid_blocks = 2: two trips and part of a third
N_CAP = 2048 * 256 + 5              # the default cap crossed: 5 threads make a second trip
N_FINAL = 256 * 257 + 3             # 258 partial sums: k_reduce_final's own loop runs twice
FILL = -7.5                         # what outputs hold before a call
SPACING = (0.8, 1.3, 2.0)           # spacing[0] belongs to the last array axis
TAU = 0.37
SHAPES = [(1,), (5,), (259,),
          (5, 7), (6, 259), (1, 9), (9, 1),
          (3, 5, 7), (4, 6, 259), (2, 1, 5), (3, 5, 8), (5, 4, 64)]
ELEMENTWISE = ["lincomb2", "lincomb3", "scale", "scale_div", "clip", "clip_inf",
               "extrapolate", "prox_dual_clamp", "prox_ell1", "prox_ell2", "shrink1",
               "shrink2", "shrink3"]
# out == x, the forms the solvers use (lsmr.py, admm_linear_solver.py,
# tikhonov_linear_solver.py); extrapolate and lincomb3 are never called in place
IN_PLACE = ["scale", "lincomb2", "clip"]


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _suffix(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _fn(name, dtype):
    from nsol_amd import _lib
    return getattr(_lib.load(), "nsol_%s_%s" % (name, _suffix(dtype)))


def _sync():
    import torch
    torch.cuda.synchronize()


def _stream():
    from nsol_amd.device import stream_ptr
    return stream_ptr()


def _is64(dtype):
    return np.dtype(dtype) == np.float64


def _assert_close(got, want, R, S, dtype, label, f64_rtol=None):
    """float64: equal (rtol f64_rtol where a libm function differs); float32: per element
    |got - want| <= R 2^-24 S, equal where R == 0."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, label
    assert np.all(np.isfinite(got)), label
    if _is64(dtype) and f64_rtol is not None:
        bad = np.abs(got - want) > f64_rtol * np.abs(want)
    elif _is64(dtype) or R == 0:
        bad = got != want
    else:
        bound = R * vc.U32 * S
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.)))
        print("%s f32: worst |got - want| / (R u S) = %.3g (R = %d)" % (label, worst, R))
        bad = err > bound
    if np.any(bad):
        i = np.flatnonzero(bad.reshape(-1))
        raise AssertionError("%s %s: %d of %d elements differ, first at %d: got %r want %r"
                             % (label, _suffix(dtype), i.size, got.size, i[0],
                                got.reshape(-1)[i[0]], want.reshape(-1)[i[0]]))


# ============================================================== 1. element-wise maps
def _call_elementwise(op, dtype, ar, n, out):
    p, s = ar.ptr, _stream()
    o = p(out)
    if op == "lincomb2":
        return _fn(op, dtype)(o, vc.A, p("x"), vc.B, p("y"), n, s)
    if op == "lincomb3":
        return _fn(op, dtype)(o, vc.A, p("x"), vc.B, p("y"), vc.C, p("z"), n, s)
    if op in ("scale", "scale_div"):
        return _fn("scale", dtype)(o, p("x"), vc.SCALE, int(op == "scale_div"), n, s)
    if op == "clip":
        return _fn("clip", dtype)(o, p("x"), vc.LO, vc.HI, n, s)
    if op == "clip_inf":
        return _fn("clip", dtype)(o, p("x"), -np.inf, np.inf, n, s)
    if op == "extrapolate":
        return _fn(op, dtype)(o, p("x"), p("y"), vc.THETA, n, s)
    if op == "prox_dual_clamp":
        return _fn(op, dtype)(o, p("x"), vc.DEN, n, s)
    if op == "prox_ell1":
        return _fn(op, dtype)(o, p("x"), p("bt"), vc.TAU1, n, s)
    if op == "prox_ell2":
        return _fn(op, dtype)(o, p("x"), p("bt"), vc.TAU2, n, s)
    if op.startswith("shrink"):
        return _fn("vector_shrink", dtype)(p("t"), o, int(op[-1]), n, vc.THR, s)
    raise ValueError(op)


def _check_elementwise(op, n, dtype, offset=0, inplace=False):
    v = vc.inputs(op, n, dtype)
    want, R, S = vc.expected(op, v, dtype)
    arrays = dict(v)
    out = "x" if inplace else "out"
    if not inplace:
        arrays["out"] = np.full(want.shape, FILL)
    ar = Arena(arrays, dtype, offset)
    assert _call_elementwise(op, dtype, ar, n, out) == 0
    _sync()
    label = "%s n=%d off=%d%s" % (op, n, offset, " in place" if inplace else "")
    _assert_close(ar.get(out, want.shape), want, R, S, dtype, label)
    assert ar.guards_intact(), label
    for k in v:
        if k != out:
            assert np.array_equal(ar.get(k, v[k].shape), v[k]), (label, k)


@pytest.mark.parametrize("op", ELEMENTWISE)
@pytest.mark.parametrize("dtype", BOTH)
def test_elementwise_kernel_matches_numpy(nsol, op, dtype):
    for n in LENGTHS:
        _check_elementwise(op, n, dtype)
    for n, offset in ((257, 1), (1021, 3)):
        _check_elementwise(op, n, dtype, offset)


@pytest.mark.parametrize("dtype", BOTH)
def test_a_second_and_a_partial_third_trip_of_the_grid_stride_loop(nsol, dtype):
    """Two workgroups for 2 * 512 + 37 elements: every thread makes two trips, 37 a third."""
    from nsol_amd import _lib
    _lib.set_param("max_grid_blocks", 2)
    try:
        for op in ELEMENTWISE:
            _check_elementwise(op, N_TRIPS, dtype)
        for name in vn.LOSSES:
            _check_loss_eval(name, N_TRIPS, dtype)
        _check_diff_axis((1, 1, N_TRIPS), dtype)
        _check_diff_axis((5, 7, 31), dtype)              # (1 085 voxels)
    finally:
        _lib.reset_params()


@pytest.mark.parametrize("dtype", BOTH)
def test_the_default_grid_cap_is_crossed(nsol, dtype):
    """2048 * 256 + 5 elements: the grid stops at max_grid_blocks and the first five
    threads come round again."""
    for op in ELEMENTWISE:
        _check_elementwise(op, N_CAP, dtype)
    _check_loss_eval("huber", N_CAP, dtype)
    _check_diff_axis((1, 1, N_CAP), dtype, directions=(0,))


@pytest.mark.parametrize("op", IN_PLACE)
@pytest.mark.parametrize("dtype", BOTH)
def test_in_place_forms_the_solvers_use(nsol, op, dtype):
    for n in (3, 257, 1021):
        _check_elementwise(op, n, dtype, inplace=True)


@pytest.mark.parametrize("dtype", BOTH)
def test_shrink_with_a_zero_threshold_yields_zero_not_nan(nsol, dtype):
    """thr = 0 and the zero vector: nrm > thr is false and the result 0 -- with >= it
    would be 0 * 0 / 0."""
    for ndim in (1, 2, 3):
        n = 257
        t = vc.inputs("shrink%d" % ndim, n, dtype)["t"]
        t[:, 100:110] = 0.
        ar = Arena(dict(t=t, out=np.full(t.shape, FILL)), dtype)
        assert _fn("vector_shrink", dtype)(ar.ptr("t"), ar.ptr("out"), ndim, n, 0.,
                                           _stream()) == 0
        _sync()
        got = ar.get("out", t.shape)
        assert np.all(np.isfinite(got)) and not got[:, 100:110].any() and not got[:, 3].any()
        # (nrm - 0) * t / nrm: the bound of vector_cases.expected with thr = 0
        _assert_close(got, vn.vector_shrink(t, ndim, 0., dtype), 4 * ndim + 9, np.abs(t),
                      dtype, "shrink%d thr=0" % ndim)
        assert ar.guards_intact() and np.array_equal(ar.get("t", t.shape), t)


# ------------------------------------------------------------------------ loss_eval
def _check_loss_eval(name, n, dtype, offset=0, skip=None):
    from nsol_amd.ops import LOSSES
    f2 = vc.inputs("loss_eval", n, dtype)["f2"]
    want = vn.loss_eval(name, f2, vc.F_SCALE, vc.GAMMA, dtype)
    S = vc.loss_S(name, f2, vc.F_SCALE, vc.GAMMA, dtype)
    fill = np.full(n, FILL)
    ar = Arena(dict(f2=f2, rho=fill, drho=fill), dtype, offset)
    ptrs = [None if skip == k else ar.ptr(k) for k in ("rho", "drho")]
    assert _fn("loss_eval", dtype)(ar.ptr("f2"), ptrs[0], ptrs[1], n, LOSSES[name],
                                   vc.F_SCALE, vc.GAMMA, _stream()) == 0
    _sync()
    label = "loss_eval %s n=%d off=%d skip=%s" % (name, n, offset, skip)
    for k, key in enumerate(("rho", "drho")):
        if skip == key:                                  # a null output: nothing written
            assert np.array_equal(ar.get(key, (n,)), fill), label
            continue
        # float64: cauchy's log1p and arctan's atan come from another libm than NumPy's
        rtol = vc.F64_LIBM_RTOL if k == 0 and name in vc.F64_INEXACT_RHO else None
        _assert_close(ar.get(key, (n,)), want[k], vc.LOSS_R[name][k], S[k], dtype,
                      label + " " + key, rtol)
    assert ar.guards_intact(), label
    assert np.array_equal(ar.get("f2", (n,)), f2), label


@pytest.mark.parametrize("name", vn.LOSSES)
@pytest.mark.parametrize("dtype", BOTH)
def test_loss_eval_matches_numpy(nsol, name, dtype):
    for n in LENGTHS:
        _check_loss_eval(name, n, dtype)
    _check_loss_eval(name, 257, dtype, offset=1)
    _check_loss_eval(name, 257, dtype, skip="rho")
    _check_loss_eval(name, 257, dtype, skip="drho")


# ============================================================================ 2. sums
class _Result(object):
    """k doubles for a reduction's result between sentinels, and the workspace."""

    def __init__(self, k=1):
        import torch
        from nsol_amd import _lib
        self.k = k
        self.t = torch.full((k + 16,), SENTINEL, dtype=torch.float64, device="cuda")
        self.ws = torch.empty(_lib.load().nsol_hip_reduce_ws_doubles(),
                              dtype=torch.float64, device="cuda")

    def ptr(self):
        return self.t[8:].data_ptr()

    def get(self):
        h = self.t.cpu().numpy()
        assert np.all(h[:8] == SENTINEL) and np.all(h[8 + self.k:] == SENTINEL)
        return h[8:8 + self.k].copy()


DEFAULT_GRID = 2048                 # max_grid_blocks as the library is built


def _check_dot(n, dtype, offset=0, grid=DEFAULT_GRID):
    x, y = vc.cancelling_pair(n, dtype)
    ar, res = Arena(dict(x=x, y=y), dtype, offset), _Result()
    for a, b in (("x", "y"), ("x", "x")):
        assert _fn("dot", dtype)(ar.ptr(a), ar.ptr(b), n, res.ptr(), res.ws.data_ptr(),
                                 _stream()) == 0
        _sync()
        terms = vn.dot_terms(ar.get(a, (n,)), ar.get(b, (n,)))
        want, bound = math.fsum(terms), vc.sum_bound(terms, vc.trips(n, grid))
        got = float(res.get()[0])
        print("dot(%s, %s) n=%d %s: |got - fsum| %.3g, bound %.3g, sum %.3g of %.3g"
              % (a, b, n, _suffix(dtype), abs(got - want), bound, want,
                 np.sum(np.abs(terms))))
        assert abs(got - want) <= bound, (a, b, n)
    assert ar.guards_intact()
    assert np.array_equal(ar.get("x", (n,)), x) and np.array_equal(ar.get("y", (n,)), y)


def _check_norm_sum(n, ndim, mode, dtype, offset=0, grid=DEFAULT_GRID):
    t = vc.field(n, ndim, dtype)
    ar, res = Arena(dict(t=t), dtype, offset), _Result()
    assert _fn("vector_norm_sum", dtype)(ar.ptr("t"), ndim, n, mode, vc.NORM_GAMMA,
                                         res.ptr(), res.ws.data_ptr(), _stream()) == 0
    _sync()
    terms = vn.vector_norm_terms(t, ndim, mode, vc.NORM_GAMMA, dtype)
    bound = vc.sum_bound(terms, vc.trips(n, grid), vc.norm_R(ndim, mode), dtype)
    got = float(res.get()[0])
    print("norm_sum n=%d ndim=%d mode=%d %s: err %.3g bound %.3g"
          % (n, ndim, mode, _suffix(dtype), abs(got - math.fsum(terms)), bound))
    assert abs(got - math.fsum(terms)) <= bound, (n, ndim, mode)
    assert ar.guards_intact() and np.array_equal(ar.get("t", t.shape), t)


def _check_pair_stats(n, dtype, offset=0, grid=DEFAULT_GRID):
    x = vc.rounded(3. + vc.normal(n, dtype, 70), dtype)
    y = vc.rounded(-1. + 0.5 * vc.normal(n, dtype, 71) + 0.3 * (x - 3.), dtype)
    mx, my = 3.0625, -0.96875
    ar, res = Arena(dict(x=x, y=y), dtype, offset), _Result(8)
    assert _fn("pair_stats", dtype)(ar.ptr("x"), ar.ptr("y"), n, mx, my, res.ptr(),
                                    res.ws.data_ptr(), _stream()) == 0
    _sync()
    got, terms = res.get(), vn.pair_terms(x, y, mx, my)
    for k in range(8):
        if k == 5:
            assert got[k] == np.max(y), n                # a maximum is exact
            continue
        # k_pair_final adds the workgroups' partial sums one after the other in ONE thread
        # (up to 2 048 of them), which the 32 of (trips + 32) does not formally cover: at
        # the 258 partials of N_FINAL the error measured is below a quarter of the bound
        bound = vc.sum_bound(terms[k], vc.trips(n, grid, cap=2048))
        err = abs(got[k] - math.fsum(terms[k]))
        print("pair_stats[%d] n=%d %s: err %.3g bound %.3g" % (k, n, _suffix(dtype), err,
                                                              bound))
        assert err <= bound, (k, n)
    assert ar.guards_intact()
    assert np.array_equal(ar.get("x", (n,)), x) and np.array_equal(ar.get("y", (n,)), y)


@pytest.mark.parametrize("dtype", BOTH)
def test_dot_matches_fsum_under_heavy_cancellation(nsol, dtype):
    for n in LENGTHS + [N_FINAL]:
        _check_dot(n, dtype)
    _check_dot(1021, dtype, offset=1)


@pytest.mark.parametrize("dtype", BOTH)
def test_vector_norm_sum_matches_fsum(nsol, dtype):
    for ndim in (1, 2, 3):
        for mode in (0, 1):
            for n in LENGTHS + [N_FINAL]:
                _check_norm_sum(n, ndim, mode, dtype)
            _check_norm_sum(1021, ndim, mode, dtype, offset=3)


@pytest.mark.parametrize("dtype", BOTH)
def test_pair_stats_match_fsum(nsol, dtype):
    for n in LENGTHS + [N_FINAL]:
        _check_pair_stats(n, dtype)
    _check_pair_stats(257, dtype, offset=1)


@pytest.mark.parametrize("dtype", BOTH)
def test_sums_with_several_trips_per_thread(nsol, dtype):
    from nsol_amd import _lib
    VW = 16 // np.dtype(dtype).itemsize
    _lib.set_param("max_grid_blocks", 2)
    try:
        _check_dot(N_TRIPS, dtype, grid=2)
        _check_pair_stats(N_TRIPS, dtype, grid=2)
        for ndim in (1, 3):
            for mode in (0, 1):
                _check_norm_sum(N_TRIPS, ndim, mode, dtype, grid=2)
        for name in vn.LOSSES:
            _check_cost(name, N_TRIPS, dtype, True, True, grid=2)        # by element
            _check_cost(name, VW * N_TRIPS, dtype, True, True, grid=2)   # by 16 bytes
    finally:
        _lib.reset_params()


# ------------------------------------------------------------------- loss_cost_grad
def _check_cost(name, n, dtype, with_b, with_g, offset=0, inplace=False,
                grid=DEFAULT_GRID):
    """k_loss<T, VW> when n % VW == 0 and r, b and g are 16-byte aligned, else
    k_loss<T, 1>.  Measured: the cost's error is below a tenth of its bound for four of
    the losses; soft_l1 in float32 reaches 0.98 of it at n = 4 (3.24e-07 of 3.31e-07),
    because 2 (sqrt(1 + z) - 1) cancels for small z and its rounding error is relative to
    2 (sqrt(1 + z) + 1), not to rho.  That is the formula of loss_functions.py; the
    bound is not adjusted for it."""
    from nsol_amd.ops import LOSSES
    VW = 16 // np.dtype(dtype).itemsize
    vec = n % VW == 0 and offset == 0
    r, b = vc.residual_inputs(n, dtype)
    arrays = dict(r=r)
    if with_b:
        arrays["b"] = b
    if with_g and not inplace:
        arrays["g"] = np.full(n, FILL)
    ar, res = Arena(arrays, dtype, offset), _Result()
    gp = None if not with_g else ar.ptr("r" if inplace else "g")
    if with_b:
        rc = _fn("loss_residual_cost_grad", dtype)(
            ar.ptr("r"), ar.ptr("b"), gp, n, LOSSES[name], vc.COST_F_SCALE, res.ptr(),
            res.ws.data_ptr(), _stream())
    else:
        rc = _fn("loss_cost_grad", dtype)(ar.ptr("r"), gp, n, LOSSES[name],
                                          vc.COST_F_SCALE, res.ptr(), res.ws.data_ptr(),
                                          _stream())
    assert rc == 0
    _sync()
    label = "cost %s n=%d %s b=%d g=%d off=%d%s" % (name, n, "vec" if vec else "scalar",
                                                   with_b, with_g, offset,
                                                   " in place" if inplace else "")
    rho, g = vn.loss_terms(r, name, vc.COST_F_SCALE, b if with_b else None, dtype)
    n_trips = vc.trips(n, grid, per=VW if vec else 1)
    bound = 0.5 * vc.sum_bound(rho, n_trips, vc.rho_R(name), dtype)
    got = float(res.get()[0])
    err = abs(got - 0.5 * math.fsum(rho))
    print("%s %s: cost err %.3g bound %.3g" % (label, _suffix(dtype), err, bound))
    assert err <= bound, label
    if with_g:
        # float64: rho' r takes neither log1p nor atan: the same bits for all five
        _assert_close(ar.get("r" if inplace else "g", (n,)), g, vc.grad_R(name), np.abs(g),
                      dtype, label)
    assert ar.guards_intact(), label
    if not inplace:
        assert np.array_equal(ar.get("r", (n,)), r), label
    if with_b:
        assert np.array_equal(ar.get("b", (n,)), b), label


@pytest.mark.parametrize("name", vn.LOSSES)
@pytest.mark.parametrize("dtype", BOTH)
def test_loss_cost_and_gradient_match_numpy(nsol, name, dtype):
    VW = 16 // np.dtype(dtype).itemsize
    for with_b in (False, True):
        for with_g in (False, True):
            for n in LENGTHS:                            # (256: whole vectors; else odd)
                _check_cost(name, n, dtype, with_b, with_g)
            for n in (4, 1020, 2052):                    # whole vectors, a partial block
                _check_cost(name, n, dtype, with_b, with_g)
            # whole vectors, but an operand off alignment: element by element
            _check_cost(name, 256, dtype, with_b, with_g, offset=1)
            _check_cost(name, 1020, dtype, with_b, with_g, offset=3)
    # more partial sums than k_reduce_final has threads, on either path
    _check_cost(name, N_FINAL, dtype, True, True)
    _check_cost(name, VW * N_FINAL, dtype, True, True)
    # g == r, as the Tikhonov objective calls it
    for with_b in (False, True):
        for n in (256, 257):
            _check_cost(name, n, dtype, with_b, True, inplace=True)


# ======================================================================== 3. stencils
def _w(d):
    return [1. / SPACING[a] if a < d else 1. for a in range(3)]


def _dims(shape):
    return (len(shape),) + (1,) * (3 - len(shape)) + tuple(shape)


def _wabs(u, w, dtype, forward):
    """(|u| + |neighbour|) w per component: the magnitudes of a difference's terms."""
    d = u.shape[0]
    a_ = np.abs(u)
    return np.stack([(a_[a] + vn.shifted(a_[a], u.ndim - 2 - a, forward)) * vc.c(w[a], dtype)
                     for a in range(d)])


@functools.lru_cache(maxsize=None)
def _stencil_case(shape, dtype):
    """Inputs (never modified), float64 results of the restatement and the float32
    magnitudes S.  R: grad 3 (two products, a sum); grad_adj 3 per component and d - 1
    sums; the axpy one product and one difference more."""
    d, w = len(shape), _w(len(shape))
    rng = np.random.default_rng(4000 + 7 * sum(shape) + d)
    r = lambda *s: vc.rounded(rng.standard_normal(s), dtype)
    x, p = r(*shape), r(d, *shape)
    adj = vn.grad_adj(p, w, dtype)
    S_adj = np.sum(_wabs(p, w, dtype, False), axis=0)
    case = dict(x=x, p=p, grad=vn.grad(x, w, dtype), adj=adj,
                axpy=vn.grad_adj_axpy(p, x, TAU, w, dtype),
                S_grad=_wabs(np.stack([x] * d), w, dtype, True), S_adj=S_adj,
                S_axpy=np.abs(x) + abs(vc.c(TAU, dtype)) * S_adj,
                R_grad=3, R_adj=4 * d - 1, R_axpy=4 * d + 1)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _check_stencils(shape, dtype, offset=0, last=None, which=("grad", "adj", "axpy")):
    cs = _stencil_case(shape, dtype)
    d, dims, w, s = len(shape), _dims(shape), _w(len(shape)), _stream()
    label = "%r off=%d last=%s" % (shape, offset, last)
    out = {}
    if "grad" in which:
        ar = Arena(dict(x=cs["x"], g=np.full((d,) + shape, FILL)), dtype, offset,
                   {None: None, "in": "x", "out": "g"}[last])
        assert _fn("grad", dtype)(ar.ptr("x"), ar.ptr("g"), *dims, *w, s) == 0
        _sync()
        out["grad"] = ar.get("g", (d,) + shape)
        _assert_close(out["grad"], cs["grad"], cs["R_grad"], cs["S_grad"], dtype,
                      "grad " + label)
        assert ar.guards_intact() and np.array_equal(ar.get("x", shape), cs["x"]), label
    if "adj" in which:
        ar = Arena(dict(p=cs["p"], out=np.full(shape, FILL)), dtype, offset,
                   {None: None, "in": "p", "out": "out"}[last])
        assert _fn("grad_adj", dtype)(ar.ptr("p"), ar.ptr("out"), *dims, *w, s) == 0
        _sync()
        out["adj"] = ar.get("out", shape)
        _assert_close(out["adj"], cs["adj"], cs["R_adj"], cs["S_adj"], dtype,
                      "grad_adj " + label)
        assert ar.guards_intact(), label
        assert np.array_equal(ar.get("p", (d,) + shape), cs["p"]), label
    if "axpy" in which:
        for end in (("p", "x") if last == "in" else (None,)):
            ar = Arena(dict(p=cs["p"], x=cs["x"], out=np.full(shape, FILL)), dtype, offset,
                       "out" if last == "out" else end)
            assert _fn("grad_adj_axpy", dtype)(ar.ptr("p"), ar.ptr("x"), ar.ptr("out"),
                                               *dims, *w, TAU, s) == 0
            _sync()
            _assert_close(ar.get("out", shape), cs["axpy"], cs["R_axpy"], cs["S_axpy"],
                          dtype, "grad_adj_axpy " + label)
            assert ar.guards_intact(), label
            assert np.array_equal(ar.get("p", (d,) + shape), cs["p"]), label
            assert np.array_equal(ar.get("x", shape), cs["x"]), label
    return out


def _adjoint_identity(Dx, y, x, DTy, label):
    lhs = math.fsum((Dx * y).reshape(-1))
    rhs = math.fsum((x * DTy).reshape(-1))
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)
    print("device adjoint identity %s: %.3g" % (label, rel))
    assert rel <= 1e-12, label


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_gradient_kernels_match_numpy_with_spacing(nsol, shape, dtype):
    """Vector, ragged and element rows, one row and four rows per workgroup, with the
    weights 1 / h that the goldens cover on three small volumes only; <grad x, p> =
    <x, grad^T p> from the device's float64 results alone."""
    out = _check_stencils(shape, dtype)
    if _is64(dtype):
        cs = _stencil_case(shape, dtype)
        _adjoint_identity(out["grad"], cs["p"], cs["x"], out["adj"], repr(shape))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_gradient_kernels_off_alignment_and_at_the_end_of_the_allocation(nsol, shape,
                                                                           dtype):
    for offset in (1, 3):
        _check_stencils(shape, dtype, offset=offset)
    # every output, then every input, ends where the device allocation ends
    _check_stencils(shape, dtype, last="out")
    _check_stencils(shape, dtype, last="in")


@pytest.mark.parametrize("dtype", BOTH)
def test_gradient_kernels_loop_over_row_groups(nsol, dtype):
    """8 x 65 = 520 row groups on 256 workgroups: every workgroup loops two or three
    times, with the slab mapping of voxel_at in force."""
    from nsol_amd import _lib
    shape = (65, 32, 67)
    _lib.set_param("stencil_blocks", 256)
    try:
        _check_stencils(shape, dtype)
    finally:
        _lib.reset_params()
        _stencil_case.cache_clear()


def test_a_float64_signal_longer_than_a_grid_row_of_tiles(nsol):
    """4096 * 256 * 2 + 5 doubles: one tile more than kStencilMaxTilesX, so the outer x
    loop of voxel_at runs.  test_long_1d_signal (float64, 3 000 017 and 4 000 000 samples)
    already takes k_grad and k_grad_adj through that loop at unit-like spacing, bit for
    bit; here it is run with a weight that float32 would round, by grad_adj_axpy as well,
    inside the guard band, and with the adjoint identity from the device's results."""
    shape = (4096 * 256 * 2 + 5,)
    try:
        out = _check_stencils(shape, np.float64)
        cs = _stencil_case(shape, np.float64)
        _adjoint_identity(out["grad"], cs["p"], cs["x"], out["adj"], "outer x")
    finally:
        _stencil_case.cache_clear()                      # (2 M samples per array)


# ------------------------------------------------------------------------ diff_axis
def _check_diff_axis(shape3, dtype, offset=0, directions=(0, 1, 2)):
    n = int(np.prod(shape3))
    x = vc.inputs("diff_axis", n, dtype)["x"].reshape(shape3)
    y = vc.normal(n, dtype, 31).reshape(shape3)
    w = vc.c(vc.W_AXIS, dtype)
    for direction in directions:
        ar = Arena(dict(x=x, y=y, fwd=np.full(shape3, FILL), adj=np.full(shape3, FILL)),
                   dtype, offset)
        fn = _fn("diff_axis", dtype)
        assert fn(ar.ptr("x"), ar.ptr("fwd"), direction, 0, *shape3, vc.W_AXIS,
                  _stream()) == 0
        assert fn(ar.ptr("y"), ar.ptr("adj"), direction, 1, *shape3, vc.W_AXIS,
                  _stream()) == 0
        _sync()
        label = "diff_axis %r dir=%d off=%d" % (shape3, direction, offset)
        axis = 2 - direction
        fwd, adj = ar.get("fwd", shape3), ar.get("adj", shape3)
        # nb w + c (-w): two products and a sum
        _assert_close(fwd, vn.diff_axis(x, direction, False, vc.W_AXIS, dtype), 3,
                      (np.abs(x) + vn.shifted(np.abs(x), axis, True)) * w, dtype,
                      label + " forward")
        _assert_close(adj, vn.diff_axis(y, direction, True, vc.W_AXIS, dtype), 3,
                      (np.abs(y) + vn.shifted(np.abs(y), axis, False)) * w, dtype,
                      label + " adjoint")
        assert ar.guards_intact(), label
        assert np.array_equal(ar.get("x", shape3), x), label
        assert np.array_equal(ar.get("y", shape3), y), label
        if _is64(dtype):
            _adjoint_identity(fwd, y, x, adj, label)


@pytest.mark.parametrize("shape3", [(3, 5, 7), (1, 9, 1), (9, 1, 1), (1, 1, 9),
                                    (4, 6, 259)])
@pytest.mark.parametrize("dtype", BOTH)
def test_diff_axis_every_direction_with_a_weight(nsol, shape3, dtype):
    _check_diff_axis(shape3, dtype)
    _check_diff_axis(shape3, dtype, offset=1)


@pytest.mark.parametrize("dtype", BOTH)
def test_diff_axis_at_the_grid_stride_lengths(nsol, dtype):
    for n in LENGTHS:
        _check_diff_axis((1, 1, n), dtype, directions=(0,))


# ===================================================================== 4. the wrappers
@pytest.mark.parametrize("dtype", BOTH)
def test_every_ops_wrapper_hands_its_arguments_on_in_order(nsol, dtype):
    from nsol_amd import ops
    from nsol_amd.device import to_device, to_numpy
    n = 257
    dev = lambda a: to_device(np.ascontiguousarray(a), dtype)
    host = lambda t, shape=None: to_numpy(t, np.float64).reshape(shape or (-1,))

    def ew(op, call):
        v = vc.inputs(op, n, dtype)
        want, R, S = vc.expected(op, v, dtype)
        d = {k: dev(a) for k, a in v.items()}
        got = call(d)
        _assert_close(host(got, want.shape), want, R, S, dtype, "ops." + op)
        for k in v:
            if d[k] is not got:
                assert np.array_equal(host(d[k], v[k].shape), v[k]), (op, k)

    ew("lincomb2", lambda d: ops.lincomb2(vc.A, d["x"], vc.B, d["y"]))
    ew("lincomb2", lambda d: ops.lincomb2(vc.A, d["x"], vc.B, d["y"], out=d["x"]))
    ew("lincomb3", lambda d: ops.lincomb3(vc.A, d["x"], vc.B, d["y"], vc.C, d["z"]))
    ew("scale", lambda d: ops.scale(d["x"], vc.SCALE))
    ew("scale", lambda d: ops.scale(d["x"], vc.SCALE, out=d["x"]))
    ew("scale_div", lambda d: ops.scale(d["x"], vc.SCALE, divide=True))
    ew("clip", lambda d: ops.clip(d["x"], vc.LO, vc.HI))
    ew("clip", lambda d: ops.clip(d["x"], vc.LO, vc.HI, out=d["x"]))
    ew("clip_inf", lambda d: ops.clip(d["x"], -np.inf, np.inf))
    ew("extrapolate", lambda d: ops.extrapolate(d["x"], d["y"], vc.THETA))
    ew("prox_dual_clamp", lambda d: ops.prox_dual_clamp(d["x"], vc.DEN))
    ew("prox_ell1", lambda d: ops.prox_ell1(d["x"], d["bt"], vc.TAU1))
    ew("prox_ell2", lambda d: ops.prox_ell2(d["x"], d["bt"], vc.TAU2))
    for ndim in (1, 2, 3):
        ew("shrink%d" % ndim,
           lambda d: ops.vector_shrink(d["t"].reshape(-1), ndim, vc.THR))

    # sums
    x, y = vc.cancelling_pair(n, dtype)
    terms = vn.dot_terms(x, y)
    assert abs(ops.dot(dev(x), dev(y)) - math.fsum(terms)) <= vc.sum_bound(terms, 1)
    sq = vn.dot_terms(x, x)
    assert abs(ops.norm2(dev(x)) ** 2 - math.fsum(sq)) <= vc.sum_bound(sq, 1 + 2)
    t = vc.field(n, 3, dtype)
    for mode in (0, 1):
        terms = vn.vector_norm_terms(t, 3, mode, vc.NORM_GAMMA, dtype)
        got = ops.vector_norm_sum(dev(t.reshape(-1)), 3, mode, vc.NORM_GAMMA)
        assert abs(got - math.fsum(terms)) <= vc.sum_bound(terms, 1, vc.norm_R(3, mode),
                                                           dtype)
    mx, my = 0.125, -0.25
    got, terms = ops.pair_stats(dev(x), dev(y), mx, my), vn.pair_terms(x, y, mx, my)
    for k in range(8):
        if k == 5:
            assert got[k] == np.max(y)
        else:
            assert abs(got[k] - math.fsum(terms[k])) <= vc.sum_bound(terms[k], 1), k
    r, b = vc.residual_inputs(n, dtype)
    for name in vn.LOSSES:
        for minus in (None, b):
            rho, g = vn.loss_terms(r, name, vc.COST_F_SCALE, minus, dtype)
            cost, gd = ops.loss_cost_grad(dev(r), name, vc.COST_F_SCALE,
                                          minus=None if minus is None else dev(minus))
            assert abs(cost - 0.5 * math.fsum(rho)) <= 0.5 * vc.sum_bound(
                rho, 1, vc.rho_R(name), dtype), name
            _assert_close(host(gd), g, vc.grad_R(name), np.abs(g), dtype,
                          "ops.loss_cost_grad " + name)
        rd = dev(r)                                      # g == r; no gradient wanted
        _, gd = ops.loss_cost_grad(rd, name, vc.COST_F_SCALE, out=rd, minus=dev(b))
        assert gd is rd
        _assert_close(host(gd), vn.loss_terms(r, name, vc.COST_F_SCALE, b, dtype)[1],
                      vc.grad_R(name), np.abs(g), dtype, "ops.loss_cost_grad in place")
        assert ops.loss_cost_grad(dev(r), name, vc.COST_F_SCALE, want_grad=False)[1] is None
        f2 = vc.inputs("loss_eval", n, dtype)["f2"]
        for kw, fs, gm in ((dict(), 1.0, vn.HUBER_GAMMA),
                           (dict(f_scale=vc.F_SCALE, huber_gamma=vc.GAMMA), vc.F_SCALE,
                            vc.GAMMA)):
            got = ops.loss_eval(dev(f2), name, **kw)
            want, S = vn.loss_eval(name, f2, fs, gm, dtype), vc.loss_S(name, f2, fs, gm,
                                                                       dtype)
            for k in range(2):
                rtol = vc.F64_LIBM_RTOL if k == 0 and name in vc.F64_INEXACT_RHO else None
                _assert_close(host(got[k]), want[k], vc.LOSS_R[name][k], S[k], dtype,
                              "ops.loss_eval %s %d" % (name, k), rtol)

    # stencils
    shape = (3, 5, 7)
    cs, w = _stencil_case(shape, dtype), _w(3)
    xd, pd = dev(cs["x"].reshape(-1)), dev(cs["p"].reshape(-1))
    _assert_close(host(ops.grad(xd, shape, w), (3,) + shape), cs["grad"], cs["R_grad"],
                  cs["S_grad"], dtype, "ops.grad")
    _assert_close(host(ops.grad_adj(pd, shape, w), shape), cs["adj"], cs["R_adj"],
                  cs["S_adj"], dtype, "ops.grad_adj")
    _assert_close(host(ops.grad_adj_axpy(pd, xd, TAU, shape, w), shape), cs["axpy"],
                  cs["R_axpy"], cs["S_axpy"], dtype, "ops.grad_adj_axpy")
    out = dev(np.full(shape, FILL).reshape(-1))
    assert ops.grad_adj_axpy(pd, xd, TAU, shape, w, out=out) is out
    _assert_close(host(out, shape), cs["axpy"], cs["R_axpy"], cs["S_axpy"], dtype,
                  "ops.grad_adj_axpy out=")
    wt = vc.c(vc.W_AXIS, dtype)
    for direction in range(3):
        for adjoint in (False, True):
            got = host(ops.diff_axis(xd, shape, direction, adjoint, vc.W_AXIS), shape)
            S = (np.abs(cs["x"]) + vn.shifted(np.abs(cs["x"]), 2 - direction,
                                              not adjoint)) * wt
            _assert_close(got, vn.diff_axis(cs["x"], direction, adjoint, vc.W_AXIS, dtype),
                          3, S, dtype, "ops.diff_axis %d %d" % (direction, adjoint))


# ======================================================================== 5. declines
@pytest.mark.parametrize("dtype", BOTH)
def test_the_entries_decline(nsol, dtype):
    """NSOL_EINVAL (-1) and nothing written for bad arguments; 0 for n == 0, with 0.0
    reported by the sums."""
    import torch
    from nsol_amd.device import to_device
    n, s = 60, _stream()
    shape = (3, 4, 5)
    mk = lambda k=1: to_device(np.full(k * n, 0.25), dtype)
    x, y, z, out = mk(), mk(), mk(), mk()
    t3, v3 = mk(3), mk(3)
    every = [x, y, z, out, t3, v3]
    P = lambda t: None if t is None else t.data_ptr()
    res = _Result(8)
    ws, rp = res.ws.data_ptr(), res.ptr()
    f = lambda name: _fn(name, dtype)

    maps = {
        "lincomb2": lambda o, a, n_: f("lincomb2")(P(o), 1., P(a), 1., P(y), n_, s),
        "lincomb3": lambda o, a, n_: f("lincomb3")(P(o), 1., P(a), 1., P(y), 1., P(z), n_, s),
        "scale": lambda o, a, n_: f("scale")(P(o), P(a), 2., 0, n_, s),
        "scale_div": lambda o, a, n_: f("scale")(P(o), P(a), 2., 1, n_, s),
        "clip": lambda o, a, n_: f("clip")(P(o), P(a), 0., 1., n_, s),
        "extrapolate": lambda o, a, n_: f("extrapolate")(P(o), P(a), P(y), 1., n_, s),
        "prox_dual_clamp": lambda o, a, n_: f("prox_dual_clamp")(P(o), P(a), 1., n_, s),
        "prox_ell1": lambda o, a, n_: f("prox_ell1")(P(o), P(a), P(y), 0.1, n_, s),
        "prox_ell2": lambda o, a, n_: f("prox_ell2")(P(o), P(a), P(y), 0.1, n_, s),
    }
    for name, call in maps.items():
        assert call(out, x, -1) == -1, name
        assert call(None, x, n) == -1 and call(out, None, n) == -1, name
        assert call(out, x, 0) == 0 and call(None, None, 0) == 0, name
    assert f("lincomb2")(P(out), 1., P(x), 1., None, n, s) == -1
    assert f("lincomb3")(P(out), 1., P(x), 1., P(y), 1., None, n, s) == -1
    assert f("extrapolate")(P(out), P(x), None, 1., n, s) == -1
    assert f("prox_ell1")(P(out), P(x), None, 0.1, n, s) == -1
    assert f("prox_ell2")(P(out), P(x), None, 0.1, n, s) == -1

    shrink = lambda t_, v_, ndim, m: f("vector_shrink")(P(t_), P(v_), ndim, m, 0.1, s)
    assert shrink(t3, v3, 0, n) == -1 and shrink(t3, v3, 4, n) == -1
    assert shrink(t3, v3, 3, -1) == -1
    assert shrink(None, v3, 3, n) == -1 and shrink(t3, None, 3, n) == -1
    assert shrink(t3, v3, 3, 0) == 0

    ev = lambda f2, rho, n_, loss: f("loss_eval")(P(f2), P(rho), P(out), n_, loss, 1., 1.3,
                                                  s)
    assert ev(x, y, -1, 0) == -1 and ev(None, y, n, 0) == -1
    assert ev(x, y, n, -1) == -1 and ev(x, y, n, 5) == -1
    assert ev(x, y, 0, 2) == 0

    # the sums: result and workspace must be there; n == 0 reports 0.0
    dot = lambda a, b, n_, r=rp, w=ws: f("dot")(P(a), P(b), n_, r, w, s)
    assert dot(x, y, -1) == -1 and dot(None, y, n) == -1 and dot(x, None, n) == -1
    assert dot(x, y, n, r=None) == -1 and dot(x, y, n, w=None) == -1
    _sync()
    assert np.all(res.get() == SENTINEL)
    assert dot(x, y, 0) == 0
    _sync()
    assert res.get()[0] == 0. and np.all(res.get()[1:] == SENTINEL)
    res.t.fill_(SENTINEL)
    assert dot(None, None, 0) == 0
    _sync()
    assert res.get()[0] == 0.

    res.t.fill_(SENTINEL)
    cost = lambda r_, g_, n_, loss, r=rp, w=ws: f("loss_cost_grad")(P(r_), P(g_), n_, loss,
                                                                    1., r, w, s)
    rcost = lambda r_, b_, g_, n_, loss: f("loss_residual_cost_grad")(
        P(r_), P(b_), P(g_), n_, loss, 1., rp, ws, s)
    assert cost(x, out, -1, 0) == -1 and cost(None, out, n, 0) == -1
    assert cost(x, out, n, -1) == -1 and cost(x, out, n, 5) == -1
    assert cost(x, out, n, 0, r=None) == -1 and cost(x, out, n, 0, w=None) == -1
    assert rcost(x, None, out, n, 0) == -1 and rcost(None, y, out, n, 0) == -1
    assert rcost(x, y, out, -1, 0) == -1 and rcost(x, y, out, n, 7) == -1
    _sync()
    assert np.all(res.get() == SENTINEL)
    assert cost(x, out, 0, 2) == 0
    _sync()
    assert res.get()[0] == 0.
    res.t.fill_(SENTINEL)
    assert rcost(x, y, out, 0, 1) == 0
    _sync()
    assert res.get()[0] == 0.

    res.t.fill_(SENTINEL)
    ns = lambda t_, ndim, m, mode, r=rp, w=ws: f("vector_norm_sum")(P(t_), ndim, m, mode,
                                                                    0.05, r, w, s)
    assert ns(t3, 0, n, 0) == -1 and ns(t3, 4, n, 0) == -1 and ns(t3, 3, -1, 0) == -1
    assert ns(t3, 3, n, -1) == -1 and ns(t3, 3, n, 2) == -1 and ns(None, 3, n, 0) == -1
    assert ns(t3, 3, n, 0, r=None) == -1 and ns(t3, 3, n, 0, w=None) == -1
    _sync()
    assert np.all(res.get() == SENTINEL)
    for mode in (0, 1):
        res.t.fill_(SENTINEL)
        assert ns(t3, 3, 0, mode) == 0
        _sync()
        assert res.get()[0] == 0.

    res.t.fill_(SENTINEL)
    ps = lambda a, b, n_, r=rp, w=ws: f("pair_stats")(P(a), P(b), n_, 0., 0., r, w, s)
    assert ps(x, y, 0) == -1 and ps(x, y, -3) == -1
    assert ps(None, y, n) == -1 and ps(x, None, n) == -1
    assert ps(x, y, n, r=None) == -1 and ps(x, y, n, w=None) == -1
    _sync()
    assert np.all(res.get() == SENTINEL)

    # stencils: ndim outside 1..3, extents that do not fit ndim or are < 1, null pointers
    g3 = mk(3)
    every.append(g3)
    grad = lambda a, o, dims: f("grad")(P(a), P(o), *dims, 1., 1., 1., s)
    gadj = lambda a, o, dims: f("grad_adj")(P(a), P(o), *dims, 1., 1., 1., s)
    axpy = lambda p_, a, o, dims: f("grad_adj_axpy")(P(p_), P(a), P(o), *dims, 1., 1., 1.,
                                                     0.5, s)
    good = (3,) + shape
    for dims in ((0,) + shape, (4,) + shape, (-1,) + shape, (2,) + shape, (1, 1, 4, 5),
                 (3, 0, 4, 5), (3, 3, 0, 5), (3, 3, 4, 0), (3, -3, 4, 5)):
        assert grad(x, g3, dims) == -1 and gadj(t3, out, dims) == -1, dims
        assert axpy(t3, x, out, dims) == -1, dims
    assert grad(None, g3, good) == -1 and grad(x, None, good) == -1
    assert gadj(None, out, good) == -1 and gadj(t3, None, good) == -1
    assert axpy(None, x, out, good) == -1 and axpy(t3, None, out, good) == -1
    assert axpy(t3, x, None, good) == -1
    da = lambda a, o, direction, dims=shape: f("diff_axis")(P(a), P(o), direction, 0, *dims,
                                                            1., s)
    assert da(x, x, 0) == -1                             # x == out
    assert da(x, out, -1) == -1 and da(x, out, 3) == -1
    assert da(None, out, 0) == -1 and da(x, None, 0) == -1
    for dims in ((0, 4, 5), (3, 0, 5), (3, 4, 0), (3, 4, -5)):
        assert da(x, out, 0, dims) == -1, dims
    _sync()
    for t in every:
        assert torch.equal(t, torch.full_like(t, 0.25))
    # ... and the good calls run
    assert grad(x, g3, good) == 0 and gadj(t3, out, good) == 0 and da(x, y, 2) == 0
    assert ps(x, z, n) == 0
    _sync()
    assert not torch.equal(g3, torch.full_like(g3, 0.25))
    assert res.get()[5] == 0.25
