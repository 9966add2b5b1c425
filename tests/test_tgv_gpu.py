"""Second-order TGV on the GPU: k_tgv_dual / k_tgv_primal through the C ABI against the
NumPy restatement (nsol_amd/tgv_numpy.py) on every access path, the transposes on the
device, guard bands, the entries that must decline, TGVPrimalDualSolver with its
stopping rule and observers, and the command line."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from device_arena import Arena
from nsol_amd import tgv_numpy as tg

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12     # float64 kernels vs the float64 restatement
F32_TOL = 1e-5      # the project's standing gate
BOTH = [np.float64, np.float32]
SPACING = (0.8, 1.3, 2.0)          # spacing[0] belongs to the last array axis
BETA, SIGMA, TAU, TL, THETA = 1.7, 0.3, 0.4, 0.6, 0.9
ISO, L1 = 4, 2                      # NSOL_PD_REG_ISOTROPIC, NSOL_PD_DATA_L1

# first / last index on every axis, extents of 1, rows shorter than a vector, ragged and
# whole rows, a row that crosses an x tile, row counts that are no multiple of ROWS
SHAPES = [(1,), (5,), (259,),
          (5, 7), (6, 259), (1, 9), (9, 1),
          (3, 5, 7), (4, 6, 259), (2, 1, 5), (3, 5, 8), (5, 4, 64)]
# longer than a grid row of x tiles (kStencilMaxTilesX * 256 * VEC + 5, float32)
X_OUTER = (4096 * 256 * 4 + 5,)


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _gate(dtype):
    return F64_TOL if np.dtype(dtype) == np.float64 else F32_TOL


def _suffix(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _iw(d):
    return [1. / SPACING[a] if a < d else 1. for a in range(3)]


def _dims(shape):
    return (len(shape),) + (1,) * (3 - len(shape)) + tuple(shape)


@functools.lru_cache(maxsize=None)
def _state(shape, dtype):
    """Random state, rounded to dtype and held in float64: dual variables that put some
    voxels inside and some outside both projections.  Never modified."""
    rng = np.random.default_rng(1000 + sum(shape) + len(shape))
    d, M = len(shape), tg.components(len(shape))
    r = lambda *s, scale=1.: (scale * rng.standard_normal(s)).astype(dtype).astype(
        np.float64)
    st = dict(xbar=r(*shape), wbar=r(d, *shape), p=r(d, *shape, scale=0.7),
              q=r(M, *shape, scale=0.7 * BETA), x=r(*shape), w=r(d, *shape),
              bt=r(*shape))
    for v in st.values():
        v.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def _want_dual(shape, dtype, iso):
    s = _state(shape, dtype)
    # float32: the weights 1/h and the scalars are rounded as the library rounds them
    c = lambda v: float(np.dtype(dtype).type(v))
    g, e = _K_rounded(s["xbar"], s["wbar"], shape, dtype)
    p = tg.project_p(s["p"] + c(SIGMA) * g, iso)
    q = tg.project_q(s["q"] + c(SIGMA) * e, c(BETA), len(shape), iso)
    inside = (float(np.mean(np.abs(s["p"] + c(SIGMA) * g) <= 1.)),
              float(np.mean(np.abs(s["q"] + c(SIGMA) * e) <= c(BETA))))
    return p, q, inside


def _rounded_spacing(shape, dtype):
    """The spacing whose inverse is the inverse the kernels use (1/h rounded to dtype)."""
    return tuple(1. / float(np.dtype(dtype).type(1. / h)) for h in SPACING[:len(shape)])


def _K_rounded(x, w, shape, dtype):
    return tg.K(x, w, _rounded_spacing(shape, dtype))


@functools.lru_cache(maxsize=None)
def _want_primal(shape, dtype, l1):
    s = _state(shape, dtype)
    c = lambda v: float(np.dtype(dtype).type(v))
    return tg.primal_step(s["p"], s["q"], s["x"], s["w"], s["bt"], c(TAU), c(TL),
                          c(THETA), _rounded_spacing(shape, dtype),
                          "ell1" if l1 else "ell2")


def _call_dual(shape, dtype, flags, ar, sigma=SIGMA, beta=BETA):
    from nsol_amd import _lib
    from nsol_amd.device import stream_ptr
    fn = getattr(_lib.load(), "nsol_tgv_dual_" + _suffix(dtype))
    return fn(ar.ptr("xbar"), ar.ptr("wbar"), ar.ptr("p"), ar.ptr("q"), *_dims(shape),
              *_iw(len(shape)), sigma, beta, flags, stream_ptr())


def _call_primal(shape, dtype, flags, ar, tau=TAU, tl=TL, theta=THETA):
    from nsol_amd import _lib
    from nsol_amd.device import stream_ptr
    fn = getattr(_lib.load(), "nsol_tgv_primal_" + _suffix(dtype))
    return fn(ar.ptr("p"), ar.ptr("q"), ar.ptr("x"), ar.ptr("xbar"), ar.ptr("w"),
              ar.ptr("wbar"), ar.ptr("bt"), *_dims(shape), *_iw(len(shape)), tau, tl,
              theta, flags, stream_ptr())


def _check_dual(shape, dtype, iso, offset=0, last=None):
    import torch
    s = _state(shape, dtype)
    d, M = len(shape), tg.components(len(shape))
    ar = Arena({k: s[k] for k in ("xbar", "wbar", "p", "q")}, dtype, offset, last)
    assert _call_dual(shape, dtype, ISO if iso else 0, ar) == 0
    torch.cuda.synchronize()
    p, q, _ = _want_dual(shape, dtype, iso)
    label = "dual %r iso=%d off=%d last=%s" % (shape, iso, offset, last)
    ep = rel_l2(ar.get("p", (d,) + shape), p, label + " p")
    eq = rel_l2(ar.get("q", (M,) + shape), q, label + " q")
    print("%s %s: p %.3g q %.3g" % (label, _suffix(dtype), ep, eq))
    assert ep <= _gate(dtype) and eq <= _gate(dtype)
    assert ar.guards_intact()
    # the inputs are only read
    assert np.array_equal(ar.get("xbar", shape), s["xbar"])
    assert np.array_equal(ar.get("wbar", (d,) + shape), s["wbar"])


def _check_primal(shape, dtype, l1, offset=0, last=None):
    import torch
    s = _state(shape, dtype)
    d, M = len(shape), tg.components(len(shape))
    ar = Arena({k: s[k] for k in ("p", "q", "x", "xbar", "w", "wbar", "bt")}, dtype,
               offset, last)
    assert _call_primal(shape, dtype, L1 if l1 else 0, ar) == 0
    torch.cuda.synchronize()
    want = _want_primal(shape, dtype, l1)
    label = "primal %r l1=%d off=%d last=%s" % (shape, l1, offset, last)
    errs = [rel_l2(ar.get(k, v.shape), v, label + " " + k)
            for k, v in zip(("x", "xbar", "w", "wbar"), want)]
    print("%s %s: x %.3g xbar %.3g w %.3g wbar %.3g" % ((label, _suffix(dtype)) +
                                                       tuple(errs)))
    assert max(errs) <= _gate(dtype)
    assert ar.guards_intact()
    for k in ("p", "q", "bt"):
        assert np.array_equal(ar.get(k, s[k].shape), s[k]), k


# ------------------------------------------------------------ 1. single kernel calls
def test_the_state_straddles_both_projections():
    for shape in ((259,), (6, 259), (4, 6, 259)):
        _, _, inside = _want_dual(shape, np.float64, False)
        assert 0.1 < inside[0] < 0.9 and 0.1 < inside[1] < 0.9, (shape, inside)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_dual_kernel_matches_numpy(nsol, shape, dtype):
    for iso in (False, True):
        _check_dual(shape, dtype, iso)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_primal_kernel_matches_numpy(nsol, shape, dtype):
    for l1 in (False, True):
        _check_primal(shape, dtype, l1)


def test_a_signal_longer_than_a_grid_row_of_tiles(nsol):
    try:
        _check_dual(X_OUTER, np.float32, False)
        _check_primal(X_OUTER, np.float32, True)
    finally:
        for f in (_state, _want_dual, _want_primal):     # (4 M samples per array)
            f.cache_clear()


@pytest.mark.parametrize("dtype", BOTH)
def test_every_workgroup_takes_several_row_groups(nsol, dtype):
    """The knob's floor is 256 workgroups, more than the row groups of the small shapes:
    a volume of 8 x 65 = 520 row groups of one x tile, so that every workgroup loops
    (twice or three times) and the slab mapping of voxel_at is in force as well."""
    from nsol_amd import _lib
    shape = (65, 32, 67)
    _lib.set_param("stencil_blocks", 256)
    try:
        _check_dual(shape, dtype, True)
        _check_primal(shape, dtype, False)
    finally:
        _lib.reset_params()


# ---------------------------------------------------------------- 2. guards and ends
@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (5, 4, 64), (3, 5, 8)])
@pytest.mark.parametrize("dtype", BOTH)
def test_arrays_off_16_byte_alignment(nsol, shape, dtype):
    """Element-aligned arrays take the ragged kernels (the element kernels for short
    rows) whatever the row length."""
    _check_dual(shape, dtype, False, offset=1)
    _check_primal(shape, dtype, False, offset=3)


@pytest.mark.parametrize("shape", [(259,), (6, 259), (4, 6, 259), (3, 5, 7), (5, 4, 64)])
@pytest.mark.parametrize("dtype", BOTH)
def test_stacks_that_end_with_their_allocation(nsol, shape, dtype):
    """Every stacked array in turn ends exactly where the device allocation ends: the
    last rows of its LAST component have nothing of the array behind them."""
    for last in ("wbar", "p", "q", "xbar"):
        _check_dual(shape, dtype, True, last=last)
    for last in ("w", "wbar", "p", "q", "bt"):
        _check_primal(shape, dtype, True, last=last)


# -------------------------------------------------------- 3. transposes on the device
@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (4, 6, 259)])
def test_transposes_on_the_device(nsol, shape):
    """From p = q = 0 with sigma = 1 and small inputs the dual kernel yields K(xbar,
    wbar); from x = w = 0 with tau = 1, tl = 0 the primal kernel yields -K^T(p, q)."""
    import torch
    dtype = np.float64
    s = _state(shape, dtype)
    d, M = len(shape), tg.components(len(shape))
    small = {k: 0.01 * s[k] for k in ("xbar", "wbar")}
    ar = Arena(dict(xbar=small["xbar"], wbar=small["wbar"], p=np.zeros((d,) + shape),
                    q=np.zeros((M,) + shape)), dtype)
    assert _call_dual(shape, dtype, 0, ar, sigma=1.) == 0
    torch.cuda.synchronize()
    g, e = ar.get("p", (d,) + shape), ar.get("q", (M,) + shape)
    gw, ew = tg.K(small["xbar"], small["wbar"], SPACING[:d])
    assert max(np.abs(gw).max(), np.abs(ew).max()) < 1.      # no projection acts
    assert rel_l2(g, gw) <= F64_TOL and rel_l2(e, ew) <= F64_TOL

    zeros = np.zeros(shape), np.zeros((d,) + shape)
    ar = Arena(dict(p=s["p"], q=s["q"], x=zeros[0], xbar=zeros[0], w=zeros[1],
                    wbar=zeros[1], bt=s["bt"]), dtype)
    assert _call_primal(shape, dtype, 0, ar, tau=1., tl=0., theta=0.) == 0
    torch.cuda.synchronize()
    kx, kw = -ar.get("x", shape), -ar.get("w", (d,) + shape)
    kxw, kww = tg.K_adj(s["p"], s["q"], SPACING[:d])
    assert rel_l2(kx, kxw) <= F64_TOL and rel_l2(kw, kww) <= F64_TOL
    # theta = 0: the bars are the new iterates
    assert np.array_equal(ar.get("xbar", shape), -kx)
    # <K(xbar, wbar), (p, q)> = <(xbar, wbar), K^T(p, q)>, both sides from the device
    lhs = tg.inner_dual(g, e, s["p"], s["q"])
    rhs = float(np.sum(small["xbar"] * kx) + np.sum(small["wbar"] * kw))
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print("device adjoint identity %r: %.3g" % (shape, rel))
    assert rel <= 1e-12


# ------------------------------------------------------------------------ 4. declines
@pytest.mark.parametrize("dtype", BOTH)
def test_the_entries_decline(nsol, dtype):
    import torch
    from nsol_amd import _lib, ops
    from nsol_amd.device import stream_ptr, to_device
    lib = _lib.load()
    dual = getattr(lib, "nsol_tgv_dual_" + _suffix(dtype))
    primal = getattr(lib, "nsol_tgv_primal_" + _suffix(dtype))
    shape = (3, 4, 6)
    n = 3 * 4 * 6
    mk = lambda k: to_device(np.full(k * n, 0.25), dtype)
    xbar, wbar, p, q = mk(1), mk(3), mk(3), mk(6)
    x, w, bt = mk(1), mk(3), mk(1)
    every = (xbar, wbar, p, q, x, w, bt)
    ptr = lambda t: None if t is None else t.data_ptr()

    def cd(a=(xbar, wbar, p, q), dims=(3,) + shape, sigma=0.3, beta=2., flags=0):
        return dual(*[ptr(t) for t in a], *dims, 1., 1., 1., sigma, beta, flags,
                    stream_ptr())

    def cp(a=(p, q, x, xbar, w, wbar, bt), dims=(3,) + shape, tau=0.3, tl=0.5, theta=1.,
           flags=0):
        return primal(*[ptr(t) for t in a], *dims, 1., 1., 1., tau, tl, theta, flags,
                      stream_ptr())

    before = ops.tgv_launches()
    good_d, good_p = (xbar, wbar, p, q), (p, q, x, xbar, w, wbar, bt)
    for k in range(4):                                   # a missing pointer
        a = list(good_d)
        a[k] = None
        assert cd(a) == -1, k
    for k in range(7):
        a = list(good_p)
        a[k] = None
        assert cp(a) == -1, k
    for i in range(4):                                   # two arguments that alias
        for j in range(i):
            a = list(good_d)
            a[i] = a[j]
            assert cd(a) == -1, (i, j)
    for i in range(7):
        for j in range(i):
            a = list(good_p)
            a[i] = a[j]
            assert cp(a) == -1, (i, j)
    assert cd((xbar, wbar, p, p[n:])) == -1              # ... or overlap
    for bad in (0., -0.3, np.inf, np.nan):
        assert cd(sigma=bad) == -1 and cd(beta=bad) == -1 and cp(tau=bad) == -1, bad
    assert cp(tl=-0.1) == -1 and cp(tl=np.nan) == -1 and cp(theta=np.nan) == -1
    for flags in (1, 8, 0x100, ISO | 1, L1 | 8):         # Huber, weighted, run flags
        assert cd(flags=flags) == -1 and cp(flags=flags) == -1, flags
    for dims in ((0,) + shape, (4,) + shape, (2,) + shape, (1, 1, 4, 6),
                 (3, -1, 4, 6)):
        assert cd(dims=dims) == -1 and cp(dims=dims) == -1, dims
    # more than 2^31 voxels: declined, nothing launched
    for dims in ((3, 1 << 11, 1 << 11, 1 << 10), (1, 1, 1, (1 << 31) + 1),
                 (2, 1, 1 << 20, (1 << 11) + 1), (3, 1 << 40, 1 << 40, 1 << 40)):
        assert cd(dims=dims) == -2 and cp(dims=dims) == -2, dims
    # an extent of 0: nothing to do, whatever else is passed
    for dims in ((3, 0, 4, 6), (3, 3, 0, 6), (1, 1, 1, 0)):
        assert cd(dims=dims) == 0 and cp(dims=dims) == 0
        assert cd((None,) * 4, dims=dims) == 0
    torch.cuda.synchronize()
    assert ops.tgv_launches() == before
    for t in every:
        assert torch.equal(t, torch.full_like(t, 0.25))
    assert cd() == 0 and cp(tl=0.) == 0                  # and the good calls run
    assert cd(flags=ISO) == 0 and cp(flags=L1) == 0
    torch.cuda.synchronize()
    assert ops.tgv_launches() == before + 4
    # the Python wrappers check their operands before the library sees them
    iw = (1., 1., 1.)
    with pytest.raises(ValueError):
        ops.tgv_dual(xbar, wbar[:2 * n], p, q, shape, iw, 0.3, 2.)
    with pytest.raises(ValueError):
        ops.tgv_dual(xbar, wbar, p, q[:3 * n], shape, iw, 0.3, 2.)
    other = np.float32 if dtype is np.float64 else np.float64
    with pytest.raises(ValueError):
        ops.tgv_primal(p, q, x, xbar, w, wbar, to_device(np.zeros(n), other), shape, iw,
                       0.3, 0.5)
    with pytest.raises(ValueError):
        ops.tgv_dual(xbar, wbar, p, q, shape, iw, -1., 2.)


# -------------------------------------------------------------------------- 5. solver
SOLVER_SHAPES = [(5, 7), (3, 5, 7), (4, 6, 259)]
X_SCALE, ALPHA, ITERS = 2.0, 0.3, 25


def _obs(shape):
    """A ramp with a step and noise, in [0, 2] or so."""
    rng = np.random.default_rng(7 + sum(shape))
    grids = np.meshgrid(*[np.arange(s) / float(s) for s in shape], indexing="ij")
    v = sum((k + 1) * 0.4 * g for k, g in enumerate(grids)) + 0.6 * (grids[-1] > 0.5)
    return v + 0.1 * rng.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def _restated(shape, iso, data, iterations=ITERS):
    obs = _obs(shape)
    sp = SPACING[:len(shape)]
    return tg.iterate(obs / X_SCALE, obs / X_SCALE, iterations, ALPHA, BETA, sp, data,
                      iso, keep=True)


def _solver(nsol, shape, dtype, iso=False, data="ell2", **kw):
    obs = _obs(shape)
    args = dict(b=obs.flatten(), x0=obs.flatten(), dimension=len(shape), shape=shape,
                spacing=SPACING[:len(shape)], alpha=ALPHA, beta=BETA, iterations=ITERS,
                data_loss=data, isotropic=iso, x_scale=X_SCALE, dtype=dtype)
    args.update(kw)
    return nsol.TGVPrimalDualSolver(**args)


@pytest.mark.parametrize("shape", SOLVER_SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("data", ["ell2", "ell1"])
def test_solver_matches_the_restatement(nsol, shape, dtype, iso, data):
    from nsol_amd import ops
    s = _solver(nsol, shape, dtype, iso, data)
    before = ops.tgv_launches()
    s.run()
    assert ops.tgv_launches() == before + 2 * ITERS
    want = _restated(shape, iso, data)
    ex = rel_l2(s.get_x(), want["x"] * X_SCALE, "x")
    ew = rel_l2(s.get_w(), want["w"] * X_SCALE, "w")
    print("solver %r %s iso=%d %s: x %.3g w %.3g" % (shape, _suffix(dtype), iso, data,
                                                      ex, ew))
    assert ex <= _gate(dtype) and ew <= _gate(dtype)
    assert s.get_iterations_done() == ITERS and s.get_stop_reason() == "iterations"
    assert s.get_execution() == "fused" and len(s.get_changes()) == 0
    assert np.linalg.norm(want["w"]) > 0.01 * np.linalg.norm(want["x"])   # w is at work


def test_solver_takes_device_tensors_and_zero_iterations(nsol):
    from nsol_amd.device import to_device
    shape = (5, 7)
    obs = _obs(shape)
    dev = to_device(obs.flatten(), np.float64)
    s = _solver(nsol, shape, np.float64, b=dev, x0=dev)
    s.run()
    assert rel_l2(s.get_x(), _restated(shape, False, "ell2")["x"] * X_SCALE) <= F64_TOL
    s = _solver(nsol, shape, np.float64, iterations=0)
    s.run()
    assert np.array_equal(s.get_x(), obs.flatten()) and not s.get_w().any()
    assert s.get_iterations_done() == 0


# ------------------------------------------------------------------------ 6. stopping
@pytest.mark.parametrize("shape", [(5, 7), (3, 5, 7)])
def test_solver_stops_where_the_restatement_does(nsol, shape):
    iters, every = 60, 5
    want = tg.iterate(_obs(shape) / X_SCALE, _obs(shape) / X_SCALE, iters, ALPHA, BETA,
                      SPACING[:len(shape)])
    points = list(range(every, iters + 1, every))
    worst = [float(max(want["ratios"][k - 1, 1:])) for k in points]
    # stop at the fourth check point: the tolerance is the geometric mean of its change
    # and the smallest one before it, so rounding cannot move the decision
    j = 3
    assert worst[j] < 0.9 * min(worst[:j])
    tol = float(np.sqrt(worst[j] * min(worst[:j])))
    stop = points[j]
    s = _solver(nsol, shape, np.float64, iterations=iters, tolerance=tol,
                check_every=every)
    s.run()
    assert s.get_iterations_done() == stop and s.get_stop_reason() == "tolerance"
    ch = s.get_changes()
    assert list(ch[:, 0]) == points[:j + 1]
    np.testing.assert_allclose(ch[:, 1:], want["ratios"][[k - 1 for k in points[:j + 1]],
                                                         1:], rtol=1e-10, atol=0)
    plain = _solver(nsol, shape, np.float64, iterations=stop)
    plain.run()
    assert np.array_equal(plain.get_x(), s.get_x())
    assert np.array_equal(plain.get_w(), s.get_w())
    # a tolerance that is never met: all iterations, the last one checked
    s = _solver(nsol, shape, np.float64, iterations=12, tolerance=0., check_every=5)
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
    s = _solver(nsol, shape, np.float64, iterations=iters)
    s.set_observer(host)
    s.run()
    host.compute_measures()
    assert host.get_observed_iterations() == list(range(iters + 1))
    want = _restated(shape, False, "ell2", iters)["iterates"]
    hv = host.get_measures()
    for k in (0, 1, iters):
        assert hv["SSD"][k] == pytest.approx(
            SM.similarity_measures["SSD"](want[k].flatten() * X_SCALE, ref), rel=1e-10)
    for every in (1, 4):
        dev = Observer(keep_iterates=False, every=every)
        dev.set_measures(measures())
        s = _solver(nsol, shape, np.float64, iterations=iters)
        s.set_observer(dev)
        s.run()
        dev.compute_measures()
        pts = dev.get_observed_iterations()
        assert pts == sorted(set(list(range(0, iters + 1, every)) + [iters]))
        for k, v in dev.get_measures().items():
            np.testing.assert_allclose(np.asarray(v), np.asarray(hv[k])[pts], rtol=1e-10,
                                       atol=0, err_msg=k)


# --------------------------------------------------------------------- 8. command line
def test_cli_tgv_writes_the_solvers_result(nsol, tmp_path, capsys):
    from nsol_amd.application import run_denoising
    obs = _obs((16, 20)) + 1.0
    src, out = str(tmp_path / "obs.npy"), str(tmp_path / "out.npy")
    np.save(src, obs)
    base = ["--observation", src, "--result", out, "--reconstruction-type", "TGVL2",
            "--beta", "2", "--iterations", "15", "--alpha", "0.2"]
    assert run_denoising.main(base) == 0
    assert "TGVL2" in capsys.readouterr().out
    s = run_denoising.build_tgv_solver(obs, "TGVL2", 0.2, 2., 15, dtype=np.float32)
    s.run()
    assert s.get_L2() == pytest.approx(tg.norm_bound(2))
    got = np.load(out)
    assert got.shape == obs.shape
    assert rel_l2(got, s.get_x().reshape(obs.shape)) < 1e-6
    assert rel_l2(got, obs) > 1e-3                       # it did something
    assert run_denoising.main(base[:5] + ["TGVL1", "--isotropic", "--dtype", "float64",
                                          "--tolerance", "1e-2", "--check-every", "4",
                                          "--reference", src, "--observe-every", "5",
                                          "--iterations", "20"]) == 0
    text = capsys.readouterr().out
    assert "stopped after" in text and "RMSE" in text
    with pytest.raises(SystemExit) as e:
        run_denoising.main(base + ["--slice-wise"])
    assert e.value.code != 0 and "--slice-wise" in capsys.readouterr().err
