"""PrimalDualLinearSolver on the GPU: the element-wise update of the data term's dual
variable, the one-pass kernels k_pd_lin / k_pd_lin_iso against the NumPy restatement
of test_pd_linear_host.py in every access form, the blur-epilogue path, the three
execution forms, masking, convergence to the minimiser, the stopping rule, the
entries that must decline, and the command line."""
import os

import numpy as np
import pytest

from conftest import rel_l2
from test_pd_linear_host import (box_kernel, convergence_case, dual_data,
                                 gaussian_kernel, minimiser_of, pd_linear_restatement,
                                 separable_taps)
from test_pd_weighted_host import mixed_weights

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12     # float64 kernels vs the float64 restatement
F32_TOL = 1e-5      # the project's standing gate on the primal iterate
ITERS = 25
BOTH = [np.float64, np.float32]


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


def _obs(shape, seed=None):
    rng = np.random.default_rng(sum(shape) if seed is None else seed)
    return 50.0 + 30.0 * rng.standard_normal(shape)


def _kernel_for(shape):
    """(1/4, 1/2, 1/4) per axis where an extent is below the Gaussian's 7 taps."""
    return box_kernel(len(shape)) if min(shape) < 7 else gaussian_kernel(len(shape), 1.)


def _wrapped(op, shape):
    return lambda x: op(x.reshape(*shape)).flatten()


def _solver(nsol, obs, kernel, dtype, op=None, **kw):
    """The wiring a caller writes: a ConvolutionOperator behind lambdas on the flat
    vector, x0 = b, x_scale = max."""
    from nsol_amd.linear_operators import ConvolutionOperator
    shape = obs.shape
    A = ConvolutionOperator(len(shape), kernel) if op is None else op
    args = dict(A=_wrapped(A, shape), A_adj=_wrapped(A, shape), b=obs.flatten(),
                x0=obs.flatten(), dimension=len(shape), alpha=0.05, iterations=ITERS,
                x_scale=float(obs.max()), dtype=dtype)
    args.update(kw)
    return nsol.PrimalDualLinearSolver(**args)


# --------------------------------------------------- 1. the dual of the data term
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1031])
@pytest.mark.parametrize("data", ["ell2", "ell1"])
@pytest.mark.parametrize("dtype", BOTH)
def test_pdl_dual_data_matches_numpy(nsol, n, data, dtype):
    from nsol_amd import ops
    from nsol_amd.device import to_device, to_numpy
    rng = np.random.default_rng(n)
    q0 = rng.standard_normal(n).astype(dtype)
    t = rng.standard_normal(n).astype(dtype)
    bt = (0.5 * rng.standard_normal(n)).astype(dtype)
    w = mixed_weights((n,), n).astype(dtype)      # zeros, ones and values in (0, 3]
    if n > 2:
        w[1] = 2.5
    sigma, lmbda = dtype(0.3), dtype(20.)
    up = lambda a: to_device(a, dtype)
    for wt in (None, w):
        wn = np.ones(n, dtype) if wt is None else wt
        for with_t in (True, False):
            v = q0 + sigma * (t - bt) if with_t else q0 - sigma * bt
            want = dual_data(v, lmbda * wn, sigma, wn, data).astype(dtype)
            q = up(q0)
            ops.pdl_dual_data(q, up(t) if with_t else None, up(bt),
                              None if wt is None else up(wt), sigma, lmbda,
                              data == "ell1")
            got = to_numpy(q, dtype)
            if dtype is np.float64:
                assert np.array_equal(got, want), (wt is None, with_t)
            else:
                assert rel_l2(got, want) <= 1e-6
            assert np.all(got[wn == 0] == 0)
    # garbage in the observation under a zero weight: exactly 0 comes back
    junk = bt.copy()
    junk[w == 0] = [np.nan, np.inf, -np.inf][n % 3]
    for with_t in (True, False):
        q = up(q0)
        ops.pdl_dual_data(q, up(t) if with_t else None, up(junk), up(w), sigma, lmbda,
                          data == "ell1")
        got = to_numpy(q, dtype)
        assert np.all(np.isfinite(got)) and np.all(got[w == 0] == 0)
        clean = up(q0)
        ops.pdl_dual_data(clean, up(t) if with_t else None, up(bt), up(w), sigma, lmbda,
                          data == "ell1")
        assert np.array_equal(got, to_numpy(clean, dtype))


def test_pdl_dual_data_refuses_mismatched_operands(nsol):
    from nsol_amd import ops
    from nsol_amd.device import to_device
    q = to_device(np.zeros(8), np.float64)
    with pytest.raises(ValueError):
        ops.pdl_dual_data(q, None, q[:7], None, 0.3, 1.)
    with pytest.raises(ValueError):
        ops.pdl_dual_data(q, None, to_device(np.zeros(8), np.float32), None, 0.3, 1.)
    with pytest.raises(ValueError):
        ops.pdl_dual_data(q, None, q.clone(), None, 0., 1.)       # sigma must be > 0
    with pytest.raises(ValueError):
        ops.pdl_dual_data(q, q, q.clone(), None, 0.3, 1.)          # t must not be q


# --------------------------------------------------- 2. runs against the restatement
SHAPES = [(1,), (2,), (65,), (1031,), (37, 50), (16, 64), (5, 7, 9), (16, 20, 24),
          (6, 9, 130), (3, 5, 256), (3, 5, 260)]


def _options(i, dtype):
    """{TV, huber} x {ell2, ell1} x {aniso, iso} x {weights, none} spread over the
    shapes, differently in the two dtypes: all 16 combinations occur."""
    c = (5 * i + (3 if np.dtype(dtype) == np.float32 else 0)) % 16
    return ("huber" if c & 1 else "TV", "ell1" if c & 2 else "ell2", bool(c & 4),
            bool(c & 8))


def test_the_options_cover_every_combination():
    seen = {_options(i, dt) for i in range(len(SHAPES)) for dt in BOTH}
    assert len(seen) == 16


_REF = {}


def _reference(key, *args, **kw):
    if key not in _REF:
        _REF[key] = pd_linear_restatement(*args, **kw)
    return _REF[key]


@pytest.mark.parametrize("i", range(len(SHAPES)))
@pytest.mark.parametrize("dtype", BOTH)
def test_runs_match_the_restatement(nsol, i, dtype):
    from nsol_amd import ops
    shape = SHAPES[i]
    reg, data, iso, weighted = _options(i, dtype)
    obs, kernel = _obs(shape), _kernel_for(shape)
    w = mixed_weights(shape, i) if weighted else None
    s = _solver(nsol, obs, kernel, dtype, reg_type=reg, data_loss=data, isotropic=iso,
                weights=None if w is None else w.flatten())
    before = ops.pdl_launches()
    s.run()
    assert ops.pdl_launches() - before == ITERS
    assert s.get_execution() == "fused" and s.get_iterations_done() == ITERS
    ref = _reference((i, reg, data, iso, weighted), obs, kernel, shape, reg, data, 0.05,
                     ITERS, weights=w, iso=iso, x_scale=obs.max())
    err = rel_l2(s.get_x(), ref, np.dtype(dtype).name)
    print(shape, reg, data, iso, weighted, np.dtype(dtype).name, err)
    assert err <= _gate(dtype), err


def test_two_rows_per_lane_match_the_restatement(nsol):
    from nsol_amd import ops
    shape, iters = (64, 128, 256), 10
    obs = _obs(shape)
    kernel = gaussian_kernel(3, 1.)
    s = _solver(nsol, obs, kernel, np.float32, iterations=iters, reg_type="huber")
    before = ops.pdl_launches()
    s.run()
    assert ops.pdl_launches() - before == iters
    ref = pd_linear_restatement(obs, separable_taps(kernel), shape, "huber", "ell2", 0.05,
                                iters, x_scale=obs.max())
    err = rel_l2(s.get_x(), ref)
    print(shape, err)
    assert err <= F32_TOL, err


@pytest.mark.parametrize("dtype", BOTH)
def test_spacing_and_scale(nsol, dtype):
    shape, sp = (5, 7, 9), (0.7, 1.3, 2.0)
    obs, kernel = _obs(shape), _kernel_for(shape)
    w = mixed_weights(shape, 3)
    s = _solver(nsol, obs, kernel, dtype, spacing=sp, x_scale=37.5, reg_type="huber",
                isotropic=True, weights=w.flatten())
    assert abs(s.get_L2() - (4 / 0.49 + 4 / 1.69 + 1. + 1.)) <= 1e-12
    s.run()
    ref = _reference(("spacing",), obs, kernel, shape, "huber", "ell2", 0.05, ITERS,
                     weights=w, iso=True, spacing=sp, x_scale=37.5)
    err = rel_l2(s.get_x(), ref, np.dtype(dtype).name)
    assert err <= _gate(dtype), err


@pytest.mark.parametrize("dtype", BOTH)
def test_active_bounds_are_an_exact_projection(nsol, dtype):
    from nsol_amd.device import to_numpy
    shape, box = (16, 20, 24), (0.31, 0.33)
    obs, kernel = _obs(shape), _kernel_for(shape)
    s = _solver(nsol, obs, kernel, dtype, bounds=box)
    s.run()
    scaled = to_numpy(s._x, np.float64)          # the scaled iterate, as the kernel left it
    assert np.all(scaled >= box[0]) and np.all(scaled <= box[1])
    assert np.sum(scaled <= box[0] * (1 + 1e-6)) > 0 and \
        np.sum(scaled >= box[1] * (1 - 1e-6)) > 0
    ref = _reference(("bounds",), obs, kernel, shape, "TV", "ell2", 0.05, ITERS,
                     bounds=box, x_scale=obs.max())
    err = rel_l2(s.get_x(), ref, np.dtype(dtype).name)
    assert err <= _gate(dtype), err


# --------------------------------------------------- 3. the blur-epilogue path
EPILOGUE = [((9, 5, 16), 4., np.float64, True), ((20, 37, 64), 2., np.float32, True),
            ((14, 65, 45), 2., np.float64, True), ((10, 70, 130), 2., np.float32, True),
            ((16, 16, 16), 7., np.float64, False)]


@pytest.mark.parametrize("shape, var, dtype, applies", EPILOGUE)
def test_blur_epilogue_path(nsol, monkeypatch, shape, var, dtype, applies):
    from nsol_amd import linear_operators as LO, ops
    A, _ = LO.LinearOperators3D().get_gaussian_blurring_operators(np.diag([var] * 3))
    obs = _obs(shape)
    w = mixed_weights(shape, 1)
    ran = []
    real = ops.corr3_wrap_axpby

    def counted(*a, **k):
        out = real(*a, **k)
        ran.append(out is not None)
        return out
    monkeypatch.setattr(ops, "corr3_wrap_axpby", counted)
    got = {}
    for on in (True, False):
        monkeypatch.setattr(LO, "USE_BLUR_EPILOGUE", on)
        del ran[:]
        s = _solver(nsol, obs, None, dtype, op=A, reg_type="huber",
                    weights=w.flatten())
        s.run()
        assert s.get_execution() == "fused"
        if on and applies:
            assert ran == [True] * ITERS
        elif on:
            # the epilogue declined (at most one attempt), and the solver went on
            assert not any(ran) and len(ran) <= 1
        else:
            assert not ran
        got[on] = s.get_x()
    ref = pd_linear_restatement(obs, separable_taps(A.kernel), shape, "huber", "ell2",
                                0.05, ITERS, weights=w, x_scale=obs.max())
    name = np.dtype(dtype).name
    assert rel_l2(got[True], got[False], name + " on/off") <= _gate(dtype)
    for on in (True, False):
        err = rel_l2(got[on], ref, "%s epilogue=%d" % (name, on))
        print(shape, name, on, err)
        assert err <= _gate(dtype), err


# --------------------------------------------------- 4. the three execution forms
@pytest.mark.parametrize("dtype", BOTH)
def test_the_three_execution_forms_agree(nsol, dtype):
    from scipy.ndimage import convolve
    from nsol_amd.device import is_device_tensor
    from nsol_amd.linear_operators import ConvolutionOperator
    shape = (6, 9, 130)
    obs, kernel = _obs(shape), _kernel_for(shape)
    op = ConvolutionOperator(3, kernel)
    w = mixed_weights(shape, 2).flatten()

    def on_device(t):
        if not is_device_tensor(t):
            raise TypeError("device tensors only")
        return op(t.view(*shape)).reshape(-1)

    def on_host(v):
        return convolve(np.asarray(v, np.float64).reshape(shape), kernel,
                        mode="wrap").reshape(-1)
    kw = dict(reg_type="TV", data_loss="ell1", weights=w, shape=shape)
    for f in (on_device, on_host):
        with pytest.raises(ValueError, match="A_norm2"):
            _solver(nsol, obs, kernel, dtype, A=f, A_adj=f, **kw)
    runs = {}
    for name, f in (("fused", None), ("device", on_device), ("host", on_host)):
        extra = {} if f is None else dict(A=f, A_adj=f, A_norm2=1.)
        s = _solver(nsol, obs, kernel, dtype, **dict(kw, **extra))
        s.run()
        assert s.get_execution() == name
        runs[name] = s.get_x()
    for name in ("device", "host"):
        err = rel_l2(runs[name], runs["fused"], "%s %s" % (name, np.dtype(dtype).name))
        assert err <= _gate(dtype), (name, err)


# --------------------------------------------------- 5. masking
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("data", ["ell2", "ell1"])
def test_a_masked_block_never_shows_what_it_holds(nsol, dtype, data):
    shape = (6, 9, 130)
    obs, kernel = _obs(shape), _kernel_for(shape)
    w = np.ones(shape)
    w[2:4, 3:7, 40:90] = 0
    junk, zero = obs.copy(), obs.copy()
    junk[w == 0] = np.nan
    zero[w == 0] = 0
    out = []
    for b in (junk, zero):
        s = _solver(nsol, obs, kernel, dtype, b=b.flatten(), x0=zero.flatten(),
                    weights=w.flatten(), data_loss=data)
        s.run()
        out.append(s.get_x())
    assert np.all(np.isfinite(out[0]))
    assert np.array_equal(out[0], out[1])
    ref = pd_linear_restatement(junk, kernel, shape, "TV", data, 0.05, ITERS, weights=w,
                                x_scale=obs.max(), x0=zero)
    assert rel_l2(out[0], ref, np.dtype(dtype).name) <= _gate(dtype)


# --------------------------------------------------- 6. convergence on the device
def test_the_device_run_reaches_the_minimiser(nsol):
    obs, kernel, shape, w, scale = convergence_case(True)
    s = _solver(nsol, obs, kernel, np.float64, iterations=1000, reg_type="huber",
                weights=w.flatten(), x_scale=scale)
    assert abs(s.get_L2() - 9.) <= 1e-12
    s.run()
    err = rel_l2(s.get_x(), minimiser_of(True))
    print("rel. l2 to the L-BFGS-B minimiser", err)
    assert err <= 1e-5, err


# --------------------------------------------------- 7. stopping
def _ratios(trace, k):
    """(r_x, r_dual) of iteration k (1-based) from the restatement's iterates."""
    x1, p1, q1 = trace[k - 1]
    if k > 1:
        x0, p0, q0 = trace[k - 2]
    else:
        x0, p0, q0 = None, np.zeros_like(p1), np.zeros_like(q1)
    return (np.sqrt(np.sum((x1 - x0) ** 2) / np.sum(x1 ** 2)),
            np.sqrt((np.sum((p1 - p0) ** 2) + np.sum((q1 - q0) ** 2)) /
                    (np.sum(p1 ** 2) + np.sum(q1 ** 2))))


@pytest.mark.parametrize("dtype", BOTH)
def test_stopping_rule(nsol, monkeypatch, dtype):
    from nsol_amd import primal_dual_linear_solver as pdl
    shape, iters, every = (16, 20, 24), 120, 10
    obs, kernel = _obs(shape), _kernel_for(shape)
    w = mixed_weights(shape, 4)
    trace = []
    pd_linear_restatement(obs, kernel, shape, "huber", "ell2", 0.05, iters, weights=w,
                          x_scale=obs.max(), trace=trace)
    want = [(k,) + _ratios(trace, k) for k in range(every, iters + 1, every)]
    # a tolerance between the changes at the 5th and the 6th check: the run stops at 60
    worst = [max(r[1:]) for r in want]
    assert min(worst[:5]) > worst[5]
    tol = float(np.sqrt(worst[4] * worst[5]))
    kw = dict(reg_type="huber", weights=w.flatten(), iterations=iters)
    s = _solver(nsol, obs, kernel, dtype, tolerance=tol, check_every=every, **kw)
    s.run()
    assert s.get_iterations_done() == 60 and s.get_stop_reason() == "tolerance"
    rows = s.get_changes()
    assert rows.shape == (6, 3) and list(rows[:, 0]) == [10., 20., 30., 40., 50., 60.]
    if dtype is np.float64:
        for got, ref in zip(rows, want):
            assert np.allclose(got[1:], ref[1:], rtol=1e-9, atol=0), (got, ref)
    else:
        # float32 iterates: a change of ~1e-2 |x| is known to ~1e-5 of itself
        for got, ref in zip(rows, want):
            assert np.allclose(got[1:], ref[1:], rtol=1e-3, atol=0), (got, ref)
    plain = _solver(nsol, obs, kernel, dtype, **dict(kw, iterations=60))
    plain.run()
    assert np.array_equal(s.get_x(), plain.get_x())
    assert plain.get_stop_reason() == "iterations" and plain.get_changes().shape == (0, 3)
    # a tolerance that is never met runs to the end, the last iteration is a check
    s = _solver(nsol, obs, kernel, dtype, tolerance=0., check_every=7,
                **dict(kw, iterations=16))
    s.run()
    assert s.get_iterations_done() == 16 and s.get_stop_reason() == "iterations"
    assert list(s.get_changes()[:, 0]) == [7., 14., 16.]
    # without a tolerance nothing is read back
    def no_read_back(self, it):
        raise AssertionError("a run without a tolerance read the board back")
    monkeypatch.setattr(pdl._LinearStopRule, "decide", no_read_back)
    again = _solver(nsol, obs, kernel, dtype, **dict(kw, iterations=60))
    again.run()
    assert again._rule is None and np.array_equal(again.get_x(), plain.get_x())


def test_observers_see_the_same_iterates(nsol):
    """A host-mode observer gets a copy per iteration, a device-mode one is served at
    its points without one; both leave x as an unobserved run does."""
    from nsol_amd import observer as Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    shape, iters = (6, 9, 130), 12
    obs, kernel = _obs(shape), _kernel_for(shape)
    truth = _obs(shape, 99).flatten()
    runs = {}
    for name, o in (("none", None), ("host", Observer.Observer()),
                    ("device", Observer.Observer(keep_iterates=False, every=5))):
        s = _solver(nsol, obs, kernel, np.float64, iterations=iters)
        if o is not None:
            o.set_measures({"RMSE": lambda x: sm.similarity_measures["RMSE"](x, truth)})
            s.set_observer(o)
        s.run()
        if o is not None:
            o.compute_measures()
        runs[name] = (s.get_x(), o)
    assert np.array_equal(runs["host"][0], runs["none"][0])
    assert np.array_equal(runs["device"][0], runs["none"][0])
    host, dev = runs["host"][1], runs["device"][1]
    assert host.get_observed_iterations() == list(range(iters + 1))
    points = dev.get_observed_iterations()
    assert points == [0, 5, 10, 12]
    hv, dv = host.get_measures()["RMSE"], dev.get_measures()["RMSE"]
    assert np.allclose(dv, np.asarray(hv)[points], rtol=1e-10, atol=0)


# --------------------------------------------------- 8. declines
@pytest.mark.parametrize("dtype", BOTH)
def test_the_entries_decline(nsol, dtype):
    import torch
    from nsol_amd import _lib, ops
    from nsol_amd.device import stream_ptr, to_device
    lib = _lib.load()
    fn = getattr(lib, "nsol_pdl_iter_" + ("f64" if dtype is np.float64 else "f32"))
    n = 4 * 5 * 6
    x = to_device(np.ones(n), dtype)
    xb, xo, g = x.clone(), x.clone(), x.clone()
    p0, p1 = to_device(np.zeros(3 * n), dtype), to_device(np.zeros(3 * n), dtype)
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(xi, xout, xx, gg, pi, po, dims=(3, 4, 5, 6), lo=-np.inf, hi=np.inf,
             flags=0):
        return fn(ptr(xi), ptr(xout), ptr(xx), ptr(gg), ptr(pi), ptr(po), *dims, 1., 1.,
                  1., 0.3, 1., 0.3, 1., lo, hi, flags, 1, stream_ptr())
    before = ops.pdl_launches()
    assert call(xb, xb, x, g, p0, p1) == -1            # aliased xbar
    assert call(xb, xo, x, g, p0, p0) == -1            # aliased p
    for k in range(6):
        args = [xb, xo, x, g, p0, p1]
        args[k] = None
        assert call(*args) == -1, k
    assert call(xb, xo, x, g, p0, p1, lo=1., hi=0.) == -1
    assert call(xb, xo, x, g, p0, p1, flags=ops.PD_DATA_L1) == -1
    # geometries beyond geom_ok: -2
    for dims in ((4, 4, 5, 6), (0, 1, 1, n), (2, 4, 5, 6), (1, 1, 5, 24), (3, 0, 5, 6),
                 (3, 1 << 11, 1 << 11, 1 << 11)):
        assert call(xb, xo, x, g, p0, p1, dims=dims) == -2, dims
    torch.cuda.synchronize()
    assert ops.pdl_launches() == before
    for t in (x, xb, xo, g):
        assert torch.equal(t, torch.ones_like(t))
    assert not p0.any() and not p1.any()
    assert call(xb, xo, x, g, p0, p1) == 0             # and the good call runs
    torch.cuda.synchronize()
    assert ops.pdl_launches() == before + 1
    # the Python wrapper checks its operands before the library sees them
    with pytest.raises(ValueError):
        ops.pdl_iter(xb, xo, x, g[:n - 1], p0, p1, (4, 5, 6), (1., 1., 1.), 0.3, 1., 0.3,
                     1., -np.inf, np.inf, 0)
    with pytest.raises(ValueError):
        ops.pdl_iter(xb, xo, x, g, p0, p1[:2 * n], (4, 5, 6), (1., 1., 1.), 0.3, 1., 0.3,
                     1., -np.inf, np.inf, 0)


# --------------------------------------------------- 9. command line
def test_cli_pdl_with_a_mask_equals_the_solver_built_by_hand(nsol, golden, tmp_path,
                                                            capsys):
    from nsol_amd import nifti
    from nsol_amd.data_reader import DataReader
    from nsol_amd.application import run_deconvolution
    vol = golden("configs")["phantom64"][20:32, :32, :40].astype(np.float64)
    mask = np.ones(vol.shape)
    mask[3:6, 8:20, 10:30] = 0
    nii, mnii = str(tmp_path / "obs.nii.gz"), str(tmp_path / "mask.nii.gz")
    out = str(tmp_path / "out.nii.gz")
    nifti.write(nii, vol)
    nifti.write(mnii, mask)
    reader = DataReader(nii)
    reader.read_data()
    data = reader.get_data()
    base = ["--observation", nii, "--result", out, "--solver", "PDL", "--iterations",
            "12", "--alpha", "0.03", "--blur", "1.0"]
    assert run_deconvolution.main(base + ["--mask", mnii]) == 0
    capsys.readouterr()
    s = run_deconvolution.build_solver(data, np.ones(3), 1.0, "TVL2", "PDL", 0.03, 12,
                                       dtype=np.float32, weights=mask)
    s.run()
    got, _, _ = nifti.read(out)
    assert rel_l2(got, s.get_x().reshape(data.shape)) < 1e-6     # float32 file
    # the l1 data term with the projection onto x >= 0, and a tolerance
    assert run_deconvolution.main(base + ["--mask", mnii, "--data-loss", "ell1",
                                          "--nonnegative", "--isotropic",
                                          "--reconstruction-type", "HuberL2",
                                          "--tolerance", "1e-2", "--check-every",
                                          "4"]) == 0
    assert "stopped after" in capsys.readouterr().out
    got, _, _ = nifti.read(out)
    assert np.all(np.isfinite(got)) and got.min() >= 0
