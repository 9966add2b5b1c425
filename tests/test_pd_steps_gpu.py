"""The kernels underneath every fast primal-dual path -- k_dual_step, k_primal_step,
k_pd_fused (csrc/nsol_pd.hip, nsol_pd_fused_body.hpp) and k_dual_step_iso, k_pd_fused_iso
(csrc/nsol_pdi.hip, nsol_pd_iso_body.hpp) -- ONE call at a time through the C ABI, per
voxel against the float64 restatement of nsol_amd/vector_numpy.py (pd_dual_step,
pd_primal_step; anchored on the oracle by test_pd_steps_host.py): bit for bit in float64,
inside the gate derived in pd_step_cases.py in float32.

Every access form the launch path can choose is taken (the catalogue of pd_step_cases.py,
whose coverage the host test asserts through a mirror of the launch path), on arrays in a
guard-band arena (device_arena.py), on and off 16-byte alignment, with each array in turn
ending where the allocation ends; the fused call must equal the two step kernels bit for
bit; the tie states must come out exactly in either type.
"""
import numpy as np
import pytest

import pd_step_cases as pc
from device_arena import Arena

pytestmark = pytest.mark.gpu

BOTH = pc.BOTH
FILL = -7.5                         # what outputs hold before a call
CASE_NAMES = [cs.name for cs in pc.catalogue(np.float32)]
assert CASE_NAMES == [cs.name for cs in pc.catalogue(np.float64)]
FUSED_ARRAYS = ("xbar_in", "xbar_out", "x", "bt", "p_in", "p_out")
WORST = {}                          # float32: kernel -> worst err / bound seen


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    yield nsol_amd
    for key in sorted(WORST):
        print("GPU float32, worst err / (R u S): %-28s %.3f" % (key, WORST[key]))


def _fn(name, dtype):
    from nsol_amd import _lib
    return getattr(_lib.load(), "nsol_%s_%s" % (name, pc.suffix(dtype)))


def _sync():
    import torch
    torch.cuda.synchronize()


def _stream():
    from nsol_amd.device import stream_ptr
    return stream_ptr()


def _flags(huber, l1, iso):
    from nsol_amd import ops
    return ((ops.PD_REG_HUBER if huber else ops.PD_REG_TV)
            | (ops.PD_DATA_L1 if l1 else ops.PD_DATA_L2)
            | (ops.PD_REG_ISOTROPIC if iso else 0))


class _Ctx(object):
    """One case on one kernel family: what a failure message names."""

    def __init__(self, name, shape, dtype, iso, plan, st, sc, w, offset=0):
        self.name, self.shape, self.dtype, self.iso, self.plan = name, shape, dtype, iso, plan
        self.st, self.sc, self.w, self.offset = st, sc, w, offset
        self.d, self.dims = len(shape), pc.dims3(shape)
        self.fill = np.full(shape, FILL)
        self.pfill = np.full((self.d,) + shape, FILL)

    def label(self, what):
        return "%s %r %s %s, form %r: %s" % (
            self.name, self.shape, pc.suffix(self.dtype), "iso" if self.iso else "aniso",
            tuple(self.plan.form), what)

    def same(self, got, want, what, array):
        got, want = np.asarray(got), np.asarray(want)
        bad = (got != want) | (np.signbit(got) != np.signbit(want))
        if np.any(bad):
            raise AssertionError(self.label(what) + ": %s differs at %d elements, first at %s"
                                 % (array, np.count_nonzero(bad),
                                    pc.first_bad(bad, self.shape)))

    def judge(self, got, what, kernel, huber, l1, has_p, which, exact=False, primal=None):
        for array, bad, ratio in pc.judge(got, self.st, self.sc, self.w, self.dtype, huber,
                                          l1, self.iso, has_p, exact, which, primal):
            if not pc.is64(self.dtype) and not exact:
                key = "%s %s" % (kernel, array)
                WORST[key] = max(WORST.get(key, 0.), ratio)
            if np.any(bad):
                how = ("is not the restatement's bits" if pc.is64(self.dtype) or exact else
                       "is outside the gate (worst err / bound %.3g)" % ratio)
                raise AssertionError(
                    self.label(what) + ": %s %s at %d places, first at %s"
                    % (array, how, np.count_nonzero(bad), pc.first_bad(bad, self.shape)))

    def intact(self, ar, what, **inputs):
        assert ar.guards_intact(), self.label(what) + ": a guard band was written"
        for k, v in inputs.items():
            self.same(ar.get(k, v.shape), v, what, k + " (an input)")

    # ----------------------------------------------------------------- the calls
    def dual(self, huber, has_p, inplace=False):
        st, sc = self.st, self.sc
        arrays = dict(xbar=st["xbar"], p_in=st["p"])
        if not inplace:
            arrays["p_out"] = self.pfill           # (sentinels where p_in is NULL)
        ar = Arena(arrays, self.dtype, self.offset)
        out = "p_in" if inplace else "p_out"
        fn = _fn("pd_dual_step_iso" if self.iso else "pd_dual_step", self.dtype)
        rc = fn(ar.ptr("xbar"), ar.ptr("p_in") if has_p else None, ar.ptr(out), *self.dims,
                *self.w, sc.sigma, sc.hden if huber else 1.0, _stream())
        what = "dual step huber=%d p_in=%s%s" % (huber, "given" if has_p else "NULL",
                                                  " in place" if inplace else "")
        assert rc == 0, self.label(what)
        _sync()
        got = ar.get(out, self.pfill.shape)
        keep = dict(xbar=st["xbar"])
        if not inplace:
            keep["p_in"] = st["p"]
        self.intact(ar, what, **keep)
        return got, what

    def primal(self, p, l1):
        st, sc = self.st, self.sc
        ar = Arena(dict(p=p, x=st["x"], xbar=self.fill, bt=st["bt"]), self.dtype, self.offset)
        rc = _fn("pd_primal_step", self.dtype)(
            ar.ptr("p"), ar.ptr("x"), ar.ptr("xbar"), ar.ptr("bt"), *self.dims, *self.w,
            sc.tau, sc.tl, sc.theta, _flags(False, l1, False), _stream())
        what = "primal step l1=%d" % l1
        assert rc == 0, self.label(what)
        _sync()
        self.intact(ar, what, p=p, bt=st["bt"])
        return (p, ar.get("x", self.shape), ar.get("xbar", self.shape)), what

    def fused(self, huber, l1, has_p, last=None):
        st, sc = self.st, self.sc
        ar = Arena(dict(xbar_in=st["xbar"], xbar_out=self.fill, x=st["x"], bt=st["bt"],
                        p_in=st["p"], p_out=self.pfill), self.dtype, self.offset, last)
        rc = _fn("pd_fused_iter", self.dtype)(
            ar.ptr("xbar_in"), ar.ptr("xbar_out"), ar.ptr("x"), ar.ptr("bt"),
            ar.ptr("p_in") if has_p else None, ar.ptr("p_out"), *self.dims, *self.w,
            sc.sigma, sc.hden if huber else 1.0, sc.tau, sc.tl, sc.theta,
            _flags(huber, l1, self.iso), _stream())
        what = "fused huber=%d l1=%d p_in=%s last=%s" % (
            huber, l1, "given" if has_p else "NULL", last)
        assert rc == 0, self.label(what)
        _sync()
        self.intact(ar, what, xbar_in=st["xbar"], bt=st["bt"], p_in=st["p"])
        return (ar.get("p_out", self.pfill.shape), ar.get("x", self.shape),
                ar.get("xbar_out", self.shape)), what


def _knobs(cs):
    from nsol_amd import _lib
    _lib.set_param("pd_ry", cs.ry)
    _lib.set_param("pd_rag", cs.rag)
    _lib.set_param("pd_zchunk", cs.zchunk)


def _ctx(cs, dtype, iso, st=None, sc=pc.RANDOM, unit=None):
    unit = cs.unit if unit is None else unit
    return _Ctx(cs.name, cs.shape, dtype, iso, pc.case_plan(cs, dtype, iso),
                pc.state(cs.shape, dtype) if st is None else st, sc,
                pc.weights(cs.shape, unit), cs.offset)


def _check_case(cx):
    kd = "k_dual_step_iso" if cx.iso else "k_dual_step"
    kf = "k_pd_fused_iso" if cx.iso else "k_pd_fused"
    fused = {}
    for huber in (False, True):
        for has_p in (True, False):
            p_dev, what = cx.dual(huber, has_p)
            cx.judge((p_dev,), what, kd, huber, False, has_p, "p")
            if has_p:
                p_same, what = cx.dual(huber, True, inplace=True)
                for a in range(cx.d):
                    cx.same(p_same[a], p_dev[a], what + " against out of place", "p_out")
            for l1 in (False, True):
                two, what = cx.primal(p_dev, l1)
                cx.judge(two, what, "k_primal_step", huber, l1, has_p, "xb")
                one, what = cx.fused(huber, l1, has_p)
                cx.judge(one, what, kf, huber, l1, has_p, "pxb")
                for a in range(cx.d):
                    cx.same(one[0][a], two[0][a], what + " against the two steps", "p_out")
                cx.same(one[1], two[1], what + " against the two steps", "x")
                cx.same(one[2], two[2], what + " against the two steps", "xbar_out")
                fused[(huber, l1, has_p)] = one
    # each array in turn ends where the device allocation ends
    keys = sorted(fused)
    for k, last in enumerate(FUSED_ARRAYS):
        huber, l1, has_p = keys[(3 * k + 1) % len(keys)]
        got, what = cx.fused(huber, l1, has_p, last=last)
        want = fused[(huber, l1, has_p)]
        for a in range(cx.d):
            cx.same(got[0][a], want[0][a], what, "p_out")
        cx.same(got[1], want[1], what, "x")
        cx.same(got[2], want[2], what, "xbar_out")


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_one_iteration_per_voxel_in_every_form(nsol, name, dtype):
    """{TV, Huber} x {l2, l1} x {p_in given, NULL}, anisotropic and isotropic, under the
    case's knobs and pointer offset: the dual step (also in place), the primal step on its
    result, the fused call -- equal to the two steps bit for bit -- and the fused call
    again with each array in turn at the end of the allocation."""
    from nsol_amd import _lib
    cs = pc.case_named(name, dtype)
    try:
        _knobs(cs)
        for iso in (False, True):
            _check_case(_ctx(cs, dtype, iso))
    finally:
        _lib.reset_params()


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_tie_states_come_out_exactly(nsol, dtype):
    """|q| == 1 and its neighbours, both zeros, |u - bt| == tl from both sides and u == bt:
    equal to the restatement in float32 as well (pd_step_cases.dual_tie_state,
    primal_tie_state)."""
    from nsol_amd import _lib
    for name in pc.TIE_CASES:
        cs = pc.case_named(name, dtype)
        try:
            _knobs(cs)
            for iso in (False, True):
                seam = pc.seam_of(cs, dtype, iso)
                cx = _ctx(cs, dtype, iso, pc.dual_tie_state(cs.shape, dtype, seam), pc.TIE,
                          unit=True)
                p_dev, what = cx.dual(False, True)
                cx.judge((p_dev,), what + " (dual ties)", "", False, False, True, "p", True)
                one, what = cx.fused(False, False, True)
                cx.judge(one, what + " (dual ties)", "", False, False, True, "p", True)
                cx.judge(one, what + " (dual ties)", "k_pd_fused tie state", False, False,
                         True, "xb")
                for a in range(cx.d):
                    cx.same(one[0][a], p_dev[a], what + " against the dual step", "p_out")
                cx = _ctx(cs, dtype, iso, pc.primal_tie_state(cs.shape, dtype, seam),
                          pc.TIE, unit=True)
                one, what = cx.fused(False, True, False)
                assert not one[0].any(), cx.label(what + " (primal ties): p_out != 0")
                cx.judge(one, what + " (primal ties)", "", False, True, False, "pxb", True)
                two, what = cx.primal(one[0], True)
                cx.judge(two, what + " (primal ties)", "", False, True, False, "xb", True)
        finally:
            _lib.reset_params()


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_step_kernels_with_several_trips_of_the_grid_stride_loop(nsol, dtype):
    """max_grid_blocks = 2 on 5 x 7 x 31 = 1 085 voxels: every thread of the two-pass
    kernels makes two trips, 61 a third."""
    from nsol_amd import _lib
    cs = pc.Case("trips", (5, 7, 31), False, 0, 1, 0, 0)
    _lib.set_param("max_grid_blocks", 2)
    try:
        for iso in (False, True):
            cx = _ctx(cs, dtype, iso)
            for huber in (False, True):
                p_dev, what = cx.dual(huber, True)
                cx.judge((p_dev,), what + " (2 blocks)",
                         "k_dual_step_iso" if iso else "k_dual_step", huber, False, True, "p")
                for l1 in (False, True):
                    two, what = cx.primal(p_dev, l1)
                    cx.judge(two, what + " (2 blocks)", "k_primal_step", huber, l1, True,
                             "xb")
    finally:
        _lib.reset_params()


# ============================================================================ refusals
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_entries_decline_and_write_nothing(nsol, dtype):
    import torch
    from nsol_amd import ops
    from nsol_amd.device import to_device
    shape = (3, 4, 5)
    n, s = 60, _stream()
    mk = lambda k=1: to_device(np.full(k * n, 0.25), dtype)
    xi, xo, x, bt, pi, po = mk(), mk(), mk(), mk(), mk(3), mk(3)
    every = [xi, xo, x, bt, pi, po]
    P = lambda t: None if t is None else t.data_ptr()
    good = (3,) + shape
    bad_dims = [(0,) + shape, (4,) + shape, (-1,) + shape,          # ndim outside 1..3
                (3, 0, 4, 5), (3, 3, 0, 5), (3, 3, 4, 0), (3, -3, 4, 5),   # an extent < 1
                (2,) + shape, (1, 3, 1, 20), (1, 1, 4, 5)]          # nz / ny != 1 below
    sc = pc.RANDOM
    w = (1., 1., 1.)

    def dual(name, xb, p_in, p_out, dims=good):
        return _fn(name, dtype)(P(xb), P(p_in), P(p_out), *dims, *w, sc.sigma, 1.0, s)

    def primal(p, x_, xb, bt_, dims=good, flags=0):
        return _fn("pd_primal_step", dtype)(P(p), P(x_), P(xb), P(bt_), *dims, *w, sc.tau,
                                            sc.tl, sc.theta, flags, s)

    def fused(a, b, c_, d_, e, f, dims=good, flags=0):
        return _fn("pd_fused_iter", dtype)(P(a), P(b), P(c_), P(d_), P(e), P(f), *dims, *w,
                                           sc.sigma, 1.0, sc.tau, sc.tl, sc.theta, flags, s)

    for name in ("pd_dual_step", "pd_dual_step_iso"):
        assert dual(name, None, pi, po) == -1 and dual(name, xi, pi, None) == -1, name
        for dims in bad_dims:
            assert dual(name, xi, pi, po, dims) == -1, (name, dims)
    assert primal(None, x, xo, bt) == -1 and primal(pi, None, xo, bt) == -1
    assert primal(pi, x, None, bt) == -1 and primal(pi, x, xo, None) == -1
    for dims in bad_dims:
        assert primal(pi, x, xo, bt, dims) == -1, dims
    for iso in (0, ops.PD_REG_ISOTROPIC):
        ok = (xi, xo, x, bt, pi, po)
        for k in (0, 1, 2, 3, 5):                                    # (p_in may be NULL)
            args = list(ok)
            args[k] = None
            assert fused(*args, flags=iso) == -1, (iso, k)
        assert fused(xi, xi, x, bt, pi, po, flags=iso) == -1         # xbar_in == xbar_out
        assert fused(xi, xo, x, bt, pi, pi, flags=iso) == -1         # p_in == p_out
        for dims in bad_dims:
            assert fused(*ok, dims=dims, flags=iso) == -1, (iso, dims)
        # the weighted data term has an entry of its own (nsol_pd_weighted_iter_*)
        assert fused(*ok, flags=iso | ops.PD_DATA_WEIGHTED) == -2
        assert fused(*ok, flags=iso | ops.PD_DATA_WEIGHTED | ops.PD_DATA_L1) == -2
    _sync()
    for t in every:
        assert torch.equal(t, torch.full_like(t, 0.25))
    # ... and the good calls run
    assert dual("pd_dual_step", xi, pi, po) == 0 and fused(xi, xo, x, bt, None, po) == 0
    _sync()
    assert not torch.equal(po, torch.full_like(po, 0.25))
    assert not torch.equal(xo, torch.full_like(xo, 0.25))


# ============================================================================ wrappers
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_ops_wrappers_hand_their_arguments_on_in_order(nsol, dtype):
    """Distinct weights per axis and distinct scalars: an argument in another's place
    shows."""
    from nsol_amd import ops
    from nsol_amd.device import to_device, to_numpy
    cs = pc.Case("ops", (3, 5, 7), False, 0, 1, 0, 0)
    sc = pc.Scalars(0.3, 1.0175, 0.4, 0.55, 0.9)
    dev = lambda a: to_device(np.array(a).reshape(-1), dtype)     # (a writable copy)
    host = lambda t, shape: to_numpy(t, np.float64).reshape(shape)
    for iso in (False, True):
        cx = _ctx(cs, dtype, iso, sc=sc)
        st, shape, w, pshape = cx.st, cs.shape, cx.w, (3,) + cs.shape
        assert len(set(w)) == 3
        xbar, p_in, p_out = dev(st["xbar"]), dev(st["p"]), dev(cx.pfill)
        (ops.pd_dual_step_iso if iso else ops.pd_dual_step)(xbar, p_in, p_out, shape, w,
                                                           sc.sigma, sc.hden)
        p_dev = host(p_out, pshape)
        cx.judge((p_dev,), "ops dual step", "ops wrappers", True, False, True, "p")
        cx.same(host(xbar, shape), st["xbar"], "ops dual step", "xbar")
        for l1 in (False, True):
            x, xb, bt = dev(st["x"]), dev(cx.fill), dev(st["bt"])
            ops.pd_primal_step(p_out, x, xb, bt, shape, w, sc.tau, sc.tl, sc.theta,
                               _flags(True, l1, False))
            two = (p_dev, host(x, shape), host(xb, shape))
            cx.judge(two, "ops.pd_primal_step l1=%d" % l1, "ops wrappers", True, l1, True, "xb")
            x, xo, po = dev(st["x"]), dev(cx.fill), dev(cx.pfill)
            ops.pd_fused_iter(xbar, xo, x, bt, p_in, po, shape, w, sc.sigma, sc.hden,
                              sc.tau, sc.tl, sc.theta, _flags(True, l1, iso))
            one = (host(po, pshape), host(x, shape), host(xo, shape))
            cx.judge(one, "ops.pd_fused_iter l1=%d" % l1, "ops wrappers", True, l1, True, "pxb")
            for a, b, k in zip(one, two, ("p_out", "x", "xbar_out")):
                assert np.array_equal(a, b), cx.label("ops fused against ops steps: " + k)
            cx.same(host(bt, shape), st["bt"], "ops.pd_fused_iter", "bt")
            assert np.array_equal(host(p_in, pshape), st["p"]), cx.label("ops: p_in")
