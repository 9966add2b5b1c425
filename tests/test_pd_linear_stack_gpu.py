"""The stacked forms of PrimalDualLinearSolver on the GPU (nsol_pdls.hip,
nsol_amd/linear_stack.py): the stacked update of q and the stacked tile against the
single-volume entries bit for bit, PrimalDualLinearBatch and PrimalDualLinearSweep
against every member's own run() bit for bit and against the NumPy restatement of
test_pd_linear_host.py, the blur-epilogue path, groups, fallbacks, the entries that
must decline, and the command line."""
import numpy as np
import pytest

from conftest import rel_l2
from test_pd_linear_host import (box_kernel, dual_data, gaussian_kernel,
                                 pd_linear_restatement, separable_taps)
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
    """The wiring a caller writes: a ConvolutionOperator (one per solver) behind lambdas
    on the flat vector, x0 = b, x_scale = max."""
    from nsol_amd.linear_operators import ConvolutionOperator
    shape = obs.shape
    A = ConvolutionOperator(len(shape), kernel) if op is None else op
    args = dict(A=_wrapped(A, shape), A_adj=_wrapped(A, shape), b=obs.flatten(),
                x0=obs.flatten(), dimension=len(shape), alpha=0.05, iterations=ITERS,
                x_scale=float(obs.max()), dtype=dtype)
    args.update(kw)
    return nsol.PrimalDualLinearSolver(**args)


def _bits(solver):
    """The scaled iterate as the kernels left it on the device."""
    from nsol_amd.device import to_numpy
    return to_numpy(solver._x, solver.get_dtype())


# --------------------------------------------------- 1. the stacked update of q
@pytest.mark.parametrize("n", [1, 63, 65, 1031])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("data", ["ell2", "ell1"])
@pytest.mark.parametrize("dtype", BOTH)
def test_stacked_dual_data_is_the_single_entry_per_member(nsol, n, P, data, dtype):
    from nsol_amd import ops
    from nsol_amd.device import to_device, to_numpy
    rng = np.random.default_rng(n + P)
    q0 = rng.standard_normal((P, n)).astype(dtype)
    t = rng.standard_normal((P, n)).astype(dtype)
    bt = (0.5 * rng.standard_normal((P, n))).astype(dtype)
    w = np.stack([mixed_weights((n,), n + m) for m in range(P)]).astype(dtype)
    lmbda = np.array([20., 3.5, 0.75][:P])
    sigma = 0.3
    l1 = data == "ell1"
    up = lambda a: to_device(np.ascontiguousarray(a).reshape(-1), dtype)
    lam = ops.pdl_lambdas(lmbda, up(q0))
    assert lam.numel() == P and np.array_equal(to_numpy(lam, dtype), lmbda.astype(dtype))
    for own_b in (False, True):                       # bt at stride n or 0
        for w_mode in ("none", "shared", "own"):      # no weights, stride 0, stride n
            # the weight every member meets, and NaN in the observation wherever
            # every weight that meets it is zero
            W = {"none": np.ones((P, n), dtype), "shared": np.repeat(w[:1], P, 0),
                 "own": w}[w_mode]
            B = bt.copy() if own_b else np.repeat(bt[:1], P, 0)
            if own_b:
                B[W == 0] = np.nan
            else:
                B[:, np.all(W == 0, axis=0)] = np.nan
            b_in = B if own_b else B[:1]
            w_in = None if w_mode == "none" else (W if w_mode == "own" else W[:1])
            for with_t in (True, False):
                q = up(q0)
                assert ops.pdl_stack_dual_data(q, up(t) if with_t else None, up(b_in),
                                               None if w_in is None else up(w_in),
                                               sigma, lam, P, l1)
                got = to_numpy(q, dtype).reshape(P, n)
                for m in range(P):
                    one = up(q0[m])
                    ops.pdl_dual_data(one, up(t[m]) if with_t else None, up(B[m]),
                                      None if w_in is None else up(W[m]), sigma,
                                      lmbda[m], l1)
                    key = (own_b, w_mode, with_t, m)
                    assert np.array_equal(got[m], to_numpy(one, dtype)), key
                    wn = W[m].astype(np.float64)
                    s_t, l_t = np.float64(dtype(sigma)), np.float64(dtype(lmbda[m]))
                    b64 = B[m].astype(np.float64)
                    with np.errstate(invalid="ignore"):
                        v = q0[m] + s_t * (t[m].astype(np.float64) - b64) if with_t \
                            else q0[m] - s_t * b64
                    want = dual_data(v, l_t * wn, s_t, wn, data)
                    assert np.all(np.isfinite(got[m])) and np.all(got[m][wn == 0] == 0)
                    assert rel_l2(got[m], want) <= _gate(dtype), key


# --------------------------------------------------- 2. the stacked tile
TILE_SHAPES = [(65,), (1031,), (37, 50), (16, 64), (5, 7, 9), (6, 9, 130), (3, 5, 260)]
BOX_SHAPE = (16, 64)


def _tile_options(i, dtype):
    """{TV, huber} x {anisotropic, isotropic} spread over the shapes, differently in
    the two dtypes: all four occur in both."""
    c = (i + (2 if np.dtype(dtype) == np.float32 else 0)) % 4
    return bool(c & 1), bool(c & 2)


def test_the_tile_options_cover_every_combination():
    for dt in BOTH:
        assert len({_tile_options(i, dt) for i in range(len(TILE_SHAPES))}) == 4


@pytest.mark.parametrize("i", range(len(TILE_SHAPES)))
@pytest.mark.parametrize("dtype", BOTH)
def test_stacked_tile_is_the_single_entry_per_member(nsol, i, dtype):
    import torch
    from nsol_amd import ops
    from nsol_amd.device import to_device, to_numpy
    shape, P = TILE_SHAPES[i], 3
    huber, iso = _tile_options(i, dtype)
    dim, n = len(shape), int(np.prod(shape))
    flags = (ops.PD_REG_HUBER if huber else ops.PD_REG_TV) | \
        (ops.PD_REG_ISOTROPIC if iso else 0)
    w = ops.inv_spacing((0.7, 1.3, 2.0)[:dim], dim)
    sigma, tau, theta = 0.3, 0.25, 1.
    hden = 1. + sigma * 0.05 if huber else 1.
    lo, hi = (0.31, 0.33) if shape == BOX_SHAPE else (-np.inf, np.inf)
    rng = np.random.default_rng(n)
    start = 0.2 + 0.25 * rng.random((P, n))
    g = [0.3 * rng.standard_normal((P, n)) for _ in range(2)]
    up = lambda a: to_device(np.ascontiguousarray(a).reshape(-1), dtype)
    # ---- the stack: two consecutive iterations over the ping-pong slots
    x, xb = up(start), [up(start), up(np.zeros((P, n)))]
    p = [up(np.zeros((P, dim * n))), up(np.zeros((P, dim * n)))]
    stack0, single0 = ops.pdl_stack_launches(), ops.pdl_launches()
    after = []
    for it in range(2):
        k = it & 1
        assert ops.pdl_stack_iter(xb[k], xb[1 - k], x, up(g[it]), p[k], p[1 - k], P,
                                  shape, w, sigma, hden, tau, theta, lo, hi, flags,
                                  has_p=it > 0)
        after.append([to_numpy(v, dtype).reshape(P, -1)
                      for v in (x, xb[1 - k], p[1 - k])])
    assert ops.pdl_stack_launches() - stack0 == 2
    assert ops.pdl_launches() == single0          # the single kernels' counter stays
    # ---- the yardstick: every member alone
    for m in range(P):
        xm, xbm = up(start[m]), [up(start[m]), up(np.zeros(n))]
        pm = [up(np.zeros(dim * n)), up(np.zeros(dim * n))]
        for it in range(2):
            k = it & 1
            assert ops.pdl_iter(xbm[k], xbm[1 - k], xm, up(g[it][m]), pm[k], pm[1 - k],
                                shape, w, sigma, hden, tau, theta, lo, hi, flags,
                                has_p=it > 0)
            for name, got, want in zip(("x", "xbar", "p"), after[it],
                                       (xm, xbm[1 - k], pm[1 - k])):
                assert np.array_equal(got[m], to_numpy(want, dtype)), \
                    (name, m, it, shape, huber, iso)
    torch.cuda.synchronize()
    assert ops.pdl_launches() - single0 == 2 * P
    assert ops.pdl_stack_launches() - stack0 == 2
    final = after[1][0].astype(np.float64)
    assert np.all(np.isfinite(final))
    if shape == BOX_SHAPE:
        assert np.all(final >= lo) and np.all(final <= hi)
        assert np.sum(final <= lo * (1 + 1e-6)) > 0 and np.sum(final >= hi * (1 - 1e-6)) > 0


# --------------------------------------------------- 3. PrimalDualLinearBatch
BATCH_CASES = [((37, 50), 4), ((16, 64), 4), ((1031,), 3), ((16, 20, 24), 3)]


def _batch_options(i, dtype):
    """(reg, data, isotropic, weighted): half the cases are weighted."""
    c = 2 * i + (1 if np.dtype(dtype) == np.float32 else 0)
    return ("huber" if c & 1 else "TV", "ell1" if c & 4 else "ell2", bool(c & 2),
            (i + (np.dtype(dtype) == np.float32)) % 2 == 0)


def _members(nsol, shape, P, dtype, reg, data, iso, weighted, **kw):
    """(solver arguments per member, observation, weights, alpha): different data,
    alpha and x_scale for every member."""
    out = []
    for m in range(P):
        obs = (1. + 0.5 * m) * _obs(shape, seed=sum(shape) + 7 * m)
        w = mixed_weights(shape, m) if weighted else None
        alpha = [0.05, 0.02, 0.2, 0.01, 0.1][m]
        args = dict(reg_type=reg, data_loss=data, isotropic=iso, alpha=alpha,
                    weights=None if w is None else w.flatten())
        args.update(kw)
        out.append((args, obs, w, alpha))
    return out


@pytest.mark.parametrize("i", range(len(BATCH_CASES)))
@pytest.mark.parametrize("dtype", BOTH)
def test_batch_members_are_their_own_runs(nsol, i, dtype):
    from nsol_amd import ops
    shape, P = BATCH_CASES[i]
    reg, data, iso, weighted = _batch_options(i, dtype)
    kernel = _kernel_for(shape)
    members = _members(nsol, shape, P, dtype, reg, data, iso, weighted)
    solvers = [_solver(nsol, obs, kernel, dtype, **args) for args, obs, _, _ in members]
    batch = nsol.PrimalDualLinearBatch(solvers)
    stack0, single0 = ops.pdl_stack_launches(), ops.pdl_launches()
    batch.run()
    assert batch.get_execution() == ["stacked"] * P
    assert batch.get_group_size() == P
    assert ops.pdl_stack_launches() - stack0 == ITERS * 1       # iterations x groups
    assert ops.pdl_launches() == single0
    assert batch.get_solvers() == solvers
    X = batch.get_x_all_device()
    assert tuple(X.shape) == (P, int(np.prod(shape)))
    for m, (args, obs, w, alpha) in enumerate(members):
        s = solvers[m]
        assert s.get_execution() == "fused" and s.get_iterations_done() == ITERS
        assert s.get_stop_reason() == "iterations" and s.get_changes().shape == (0, 3)
        own = _solver(nsol, obs, kernel, dtype, **args)
        own.run()
        assert np.array_equal(_bits(s), _bits(own)), (m, shape)
        assert np.array_equal(s.get_x(), own.get_x())
        assert np.array_equal(batch.get_x(m), own.get_x())
        assert np.array_equal(X[m].cpu().numpy(), own.get_x_device().cpu().numpy())
        ref = pd_linear_restatement(obs, kernel, shape, reg, data, alpha, ITERS,
                                    weights=w, iso=iso, x_scale=obs.max())
        err = rel_l2(s.get_x(), ref, "%s member %d" % (np.dtype(dtype).name, m))
        print(shape, reg, data, iso, weighted, np.dtype(dtype).name, m, err)
        assert err <= _gate(dtype), err


# --------------------------------------------------- 3b. the other blur paths
def _dense_kernel():
    """A symmetric cross: no outer product, and its own adjoint."""
    return np.array([[0., 0.2, 0.], [0.2, 0.2, 0.2], [0., 0.2, 0.]])


@pytest.mark.parametrize("shape, kernel, mode", [
    ((5, 7, 9), "box", "wrap"),             # member slices off the 16-byte grid, 3-D
    ((7, 9, 10), "gauss", "wrap"),          # the same with the 7-tap Gaussian
    ((37, 50), "dense", "wrap"),            # taps that are no outer product: per member
    ((37, 50), "gauss", "reflect"),         # a boundary mode without a wrap kernel
    ((16, 64), "gauss", "mirror"),
    ((1031,), "gauss", "nearest")], ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("dtype", BOTH)
def test_batch_on_every_blur_path_is_bit_identical(nsol, shape, kernel, mode, dtype):
    from nsol_amd import ops
    from nsol_amd.linear_operators import ConvolutionOperator
    P = 3
    taps = {"box": box_kernel(len(shape)), "gauss": gaussian_kernel(len(shape), 1.),
            "dense": _dense_kernel()}[kernel]
    make = lambda: ConvolutionOperator(len(shape), taps, mode)
    assert make().separable == (kernel != "dense")
    members = _members(nsol, shape, P, dtype, "huber", "ell2", True, True)
    solvers = [_solver(nsol, obs, None, dtype, op=make(), **args)
               for args, obs, _, _ in members]
    batch = nsol.PrimalDualLinearBatch(solvers)
    before = ops.pdl_stack_launches()
    batch.run()
    assert batch.get_execution() == ["stacked"] * P
    assert ops.pdl_stack_launches() - before == ITERS
    for m, (args, obs, w, alpha) in enumerate(members):
        own = _solver(nsol, obs, None, dtype, op=make(), **args)
        own.run()
        assert np.array_equal(_bits(solvers[m]), _bits(own)), (m, shape, kernel, mode)
        if mode == "wrap":
            ref = pd_linear_restatement(obs, taps, shape, "huber", "ell2", alpha, ITERS,
                                        weights=w, iso=True, x_scale=obs.max())
            assert rel_l2(solvers[m].get_x(), ref) <= _gate(dtype)


@pytest.mark.parametrize("dtype", BOTH)
def test_batch_of_device_tensors_with_device_mode_observers(nsol, dtype):
    """b, x0 and the weights already on the device, and an observer per member that is
    served at the members' common points."""
    from nsol_amd.device import to_device
    from nsol_amd.observer import Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    shape, P = (16, 64), 3
    kernel = _kernel_for(shape)
    truth = _obs(shape, 99).flatten()
    members = _members(nsol, shape, P, dtype, "TV", "ell1", False, True)

    def build():
        out = []
        for args, obs, w, _ in members:
            on_device = dict(b=to_device(obs.flatten(), np.float64),
                             x0=to_device(obs.flatten(), dtype),
                             weights=to_device(w.flatten(), dtype))
            s = _solver(nsol, obs, kernel, dtype, **dict(args, **on_device))
            o = Observer(keep_iterates=False, every=10)
            o.set_measures({"RMSE": lambda x: sm.similarity_measures["RMSE"](x, truth),
                            "NCC": lambda x: sm.similarity_measures["NCC"](x, truth)})
            s.set_observer(o)
            out.append(s)
        return out
    solvers, own = build(), build()
    batch = nsol.PrimalDualLinearBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["stacked"] * P
    for s, o in zip(solvers, own):
        o.run()
        assert np.array_equal(_bits(s), _bits(o))
        a, b = s.get_observer(), o.get_observer()
        a.compute_measures()
        b.compute_measures()
        assert a.get_observed_iterations() == b.get_observed_iterations() == [0, 10, 20, 25]
        for name in ("RMSE", "NCC"):
            assert np.array_equal(a.get_measures()[name], b.get_measures()[name]), name
            assert np.all(np.isfinite(a.get_measures()[name]))


# --------------------------------------------------- 4. the blur-epilogue path
@pytest.mark.parametrize("shape, var, dtype", [((20, 37, 64), 2., np.float32),
                                               ((9, 5, 16), 4., np.float64)])
def test_batch_on_the_blur_epilogue_path(nsol, monkeypatch, shape, var, dtype):
    from nsol_amd import linear_operators as LO, ops
    A, _ = LO.LinearOperators3D().get_gaussian_blurring_operators(np.diag([var] * 3))
    P = 3
    members = _members(nsol, shape, P, dtype, "huber", "ell2", False, True)
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
        solvers = [_solver(nsol, obs, None, dtype, op=A, **args)
                   for args, obs, _, _ in members]
        del ran[:]
        batch = nsol.PrimalDualLinearBatch(solvers)
        batch.run()
        assert batch.get_execution() == ["stacked"] * P
        # the epilogue ran for every member in every iteration, or never
        assert ran == ([True] * (ITERS * P) if on else [])
        for m, (args, obs, _, _) in enumerate(members):
            own = _solver(nsol, obs, None, dtype, op=A, **args)
            own.run()
            assert np.array_equal(_bits(solvers[m]), _bits(own)), (on, m)
        got[on] = [s.get_x() for s in solvers]
    for m, (args, obs, w, alpha) in enumerate(members):
        ref = pd_linear_restatement(obs, separable_taps(A.kernel), shape, "huber",
                                    "ell2", alpha, ITERS, weights=w, x_scale=obs.max())
        for on in (True, False):
            err = rel_l2(got[on][m], ref, "%s epilogue=%d member %d" % (
                np.dtype(dtype).name, on, m))
            assert err <= _gate(dtype), (on, m, err)


# --------------------------------------------------- 5. PrimalDualLinearSweep
ALPHAS = [0.01, 0.02, 0.05, 0.1, 0.3]


@pytest.mark.parametrize("shape, weighted, dtype", [((16, 20, 24), False, np.float32),
                                                    ((37, 50), True, np.float64),
                                                    ((37, 50), True, np.float32)])
def test_sweep_members_are_single_solvers(nsol, shape, weighted, dtype):
    from nsol_amd import ops
    from nsol_amd.linear_operators import ConvolutionOperator
    from nsol_amd.observer import Observer, observation_points
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    obs, kernel = _obs(shape), _kernel_for(shape)
    truth = _obs(shape, 99).flatten()
    w = mixed_weights(shape, 5).flatten() if weighted else None
    op = ConvolutionOperator(len(shape), kernel)
    measures = {"PSNR": lambda x: sm.similarity_measures["PSNR"](x, truth),
                "SSD": lambda x: sm.similarity_measures["SSD"](x, truth)}
    kw = dict(reg_type="huber", isotropic=True, weights=w, iterations=ITERS)
    sweep = nsol.PrimalDualLinearSweep(_wrapped(op, shape), _wrapped(op, shape),
                                       obs.flatten(), obs.flatten(), len(shape),
                                       parameters={"alpha": ALPHAS},
                                       x_scale=float(obs.max()), dtype=dtype, **kw)
    sweep.set_measures(measures, every=10)
    stack0, single0 = ops.pdl_stack_launches(), ops.pdl_launches()
    sweep.run()
    assert sweep.get_execution() == "stacked" and sweep.get_group_size() == 5
    assert ops.pdl_stack_launches() - stack0 == ITERS and ops.pdl_launches() == single0
    assert sweep.get_parameters() == [{"alpha": a} for a in ALPHAS]
    assert sweep.get_iterations_done() == [ITERS] * 5
    assert sweep.get_observed_iterations() == observation_points(ITERS, 10)
    got = sweep.get_measures()
    X = sweep.get_x_all_device().cpu().numpy()
    for m, alpha in enumerate(ALPHAS):
        s = _solver(nsol, obs, kernel, dtype, alpha=alpha, **kw)
        o = Observer(keep_iterates=False, every=10)
        o.set_measures(measures)
        s.set_observer(o)
        s.run()
        o.compute_measures()
        assert np.array_equal(sweep.get_x(m), s.get_x()), (m, alpha)
        assert np.array_equal(X[m], s.get_x_device().cpu().numpy())
        for name in measures:
            assert got[name].shape == (5, 4)
            assert np.array_equal(got[name][m], o.get_measures()[name]), (name, alpha)
    k, best = sweep.best("PSNR")
    assert k == int(np.argmax(got["PSNR"][:, -1])) and best == {"alpha": ALPHAS[k]}
    assert sweep.best("SSD", mode="min")[0] == int(np.argmin(got["SSD"][:, -1]))


def test_a_sweep_with_a_tolerance_runs_plain_solvers(nsol):
    shape = (16, 64)
    obs, kernel = _obs(shape), _kernel_for(shape)
    from nsol_amd.linear_operators import ConvolutionOperator
    op = ConvolutionOperator(2, kernel)
    kw = dict(iterations=40, tolerance=2e-2, check_every=5)
    sweep = nsol.PrimalDualLinearSweep(_wrapped(op, shape), _wrapped(op, shape),
                                       obs.flatten(), obs.flatten(), 2,
                                       parameters={"alpha": [0.02, 0.2]},
                                       x_scale=float(obs.max()), dtype=np.float64, **kw)
    sweep.run()
    assert sweep.get_execution() == "sequential" and sweep.get_group_size() is None
    for m, alpha in enumerate([0.02, 0.2]):
        s = _solver(nsol, obs, kernel, np.float64, alpha=alpha, **kw)
        s.run()
        assert sweep.get_iterations_done()[m] == s.get_iterations_done()
        assert np.array_equal(sweep.get_x(m), s.get_x())


# --------------------------------------------------- 6. groups
def test_groups_leave_the_same_bits(nsol, monkeypatch):
    from nsol_amd import ops
    shape, P, dtype = (37, 50), 5, np.float32
    kernel = _kernel_for(shape)
    members = _members(nsol, shape, P, dtype, "TV", "ell2", True, False)
    runs = {}
    n = int(np.prod(shape))
    # a member here owns x, two xbar, q, g, b~ and t and two p of two parts
    per_member = (7 + 2 * 2) * n * 4
    for name, budget in (("one", ops.PDL_STACK_GROUP_BYTES),
                         ("2 + 2 + 1", 2 * per_member + per_member // 2)):
        monkeypatch.setattr(ops, "PDL_STACK_GROUP_BYTES", budget)
        solvers = [_solver(nsol, obs, kernel, dtype, **args)
                   for args, obs, _, _ in members]
        batch = nsol.PrimalDualLinearBatch(solvers)
        before = ops.pdl_stack_launches()
        batch.run()
        assert batch.get_execution() == ["stacked"] * P
        runs[name] = ([_bits(s) for s in solvers], batch.get_group_size(),
                      ops.pdl_stack_launches() - before)
    assert runs["one"][1:] == (5, ITERS)
    assert runs["2 + 2 + 1"][1:] == (2, 3 * ITERS)
    for a, b in zip(runs["one"][0], runs["2 + 2 + 1"][0]):
        assert np.array_equal(a, b)


# --------------------------------------------------- 7. fallbacks
def test_what_does_not_stack_runs_on_its_own(nsol):
    from scipy.ndimage import convolve
    from nsol_amd.observer import Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    shape, dtype = (16, 64), np.float64
    kernel = _kernel_for(shape)
    truth = _obs(shape, 99).flatten()

    def on_host(v):
        return convolve(np.asarray(v, np.float64).reshape(shape), kernel,
                        mode="wrap").reshape(-1)

    def host_observer():
        o = Observer()
        o.set_measures({"RMSE": lambda x: sm.similarity_measures["RMSE"](x, truth)})
        return o
    # (arguments, observer factory) of the seven, in the list's order
    specs = [(dict(tolerance=1e-2, check_every=5), None),
             (dict(alpha=0.02), None),
             (dict(), host_observer),
             (dict(alpha=0.1), None),
             (dict(A=on_host, A_adj=on_host, A_norm2=1., shape=shape), None),
             (dict(kernel=gaussian_kernel(2, 1.5)), None),
             (dict(alpha=0.2), None)]
    stackable = [1, 3, 6]

    def build():
        out = []
        for k, (kw, make) in enumerate(specs):
            kw = dict(kw)
            s = _solver(nsol, _obs(shape, seed=k), kw.pop("kernel", kernel), dtype,
                        iterations=12, **kw)
            if make is not None:
                s.set_observer(make())
            out.append(s)
        return out
    solvers = build()
    batch = nsol.PrimalDualLinearBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["stacked" if k in stackable else "sequential"
                                     for k in range(7)]
    assert batch.get_group_size() == 3
    assert [s.get_execution() for s in solvers] == \
        ["fused", "fused", "fused", "fused", "host", "fused", "fused"]
    own = build()
    for k, (s, o) in enumerate(zip(solvers, own)):
        o.run()
        assert np.array_equal(s.get_x(), o.get_x()), k
        assert s.get_iterations_done() == o.get_iterations_done(), k
        assert s.get_stop_reason() == o.get_stop_reason(), k
    assert len(solvers[2].get_observer().get_x_list()) == 13


# --------------------------------------------------- 8. declines
@pytest.mark.parametrize("dtype", BOTH)
def test_the_stacked_entries_decline(nsol, dtype):
    import torch
    from nsol_amd import _lib, ops
    from nsol_amd.device import stream_ptr, to_device
    lib = _lib.load()
    suf = "f64" if dtype is np.float64 else "f32"
    it = getattr(lib, "nsol_pdl_stack_iter_" + suf)
    dd = getattr(lib, "nsol_pdl_stack_dual_data_" + suf)
    shape, P = (4, 5, 6), 2
    n = 4 * 5 * 6
    x = to_device(np.ones(P * n), dtype)
    xb, xo, g = x.clone(), x.clone(), x.clone()
    p0, p1 = to_device(np.zeros(3 * P * n), dtype), to_device(np.zeros(3 * P * n), dtype)
    lam = ops.pdl_lambdas([2., 3.], x)
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(members=P, dims=(3, 4, 5, 6)):
        return it(ptr(xb), ptr(xo), ptr(x), ptr(g), ptr(p0), ptr(p1), members, *dims, 1.,
                  1., 1., 0.3, 1., 0.3, 1., -np.inf, np.inf, 0, 1, stream_ptr())
    before, single = ops.pdl_stack_launches(), ops.pdl_launches()
    for members in (0, -1, 65536):
        assert call(members) == -2, members
        assert dd(ptr(x), None, ptr(g), 0, None, 0, 0.3, ptr(lam), 0, members, n,
                  stream_ptr()) == -2, members
    # members * n over 2^31 (2 x 1024^3 is exactly 2^31 and would be taken), and the
    # geometries nsol_pdl_iter_* declines
    assert call(3, (3, 1 << 10, 1 << 10, 1 << 10)) == -2
    assert call(2, (3, 1 << 10, 1 << 10, (1 << 10) + 1)) == -2
    for dims in ((4, 4, 5, 6), (0, 1, 1, n), (2, 4, 5, 6), (3, 0, 5, 6)):
        assert call(P, dims) == -2, dims
    assert dd(ptr(x), None, ptr(g), 0, None, 0, 0.3, ptr(lam), 0, 2, (1 << 30) + 1,
              stream_ptr()) == -2
    # what the library refuses as an invalid argument: ValueError through ops
    w = (1., 1., 1.)
    args = (shape, w, 0.3, 1., 0.3, 1.)
    with pytest.raises(ValueError):
        ops.pdl_stack_iter(xb, xb, x, g, p0, p1, P, *args, -np.inf, np.inf, 0)
    with pytest.raises(ValueError):
        ops.pdl_stack_iter(xb, xo, x, g, p0, p0, P, *args, -np.inf, np.inf, 0)
    with pytest.raises(ValueError):
        ops.pdl_stack_iter(xb, xo, x, g, p0, p1, P, *args, 1., 0., 0)       # lo > hi
    with pytest.raises(ValueError):
        ops.pdl_stack_iter(xb, xo, x, g, p0, p1, P, *args, np.nan, 1., 0)
    with pytest.raises(ValueError):
        ops.pdl_stack_iter(xb, xo, x, g, p0, p1, P, *args, -np.inf, np.inf,
                           ops.PD_DATA_L1)                                 # a stray flag
    with pytest.raises(ValueError):
        ops.pdl_stack_iter(xb, xo, x, g, p0, p1, P, shape, w, 0., 1., 0.3, 1., -np.inf,
                           np.inf, 0)                                      # sigma <= 0
    with pytest.raises(ValueError):
        ops.pdl_stack_iter(xb, xo, x, g[:P * n - 1], p0, p1, P, *args, -np.inf, np.inf, 0)
    with pytest.raises(ValueError):
        ops.pdl_stack_iter(xb, xo, x, g, p0, p1, P + 1, *args, -np.inf, np.inf, 0)
    # the update of q: a stride that is neither 0 nor n, t == q, sigma <= 0
    q = to_device(np.zeros(P * n), dtype)
    for bad in (1, n - 1, 2 * n):
        assert dd(ptr(q), None, ptr(g), bad, None, 0, 0.3, ptr(lam), 0, P, n,
                  stream_ptr()) == -1, bad
        assert dd(ptr(q), None, ptr(g), 0, ptr(x), bad, 0.3, ptr(lam), 0, P, n,
                  stream_ptr()) == -1, bad
    with pytest.raises(ValueError):
        ops.pdl_stack_dual_data(q, None, g[:n + 1], None, 0.3, lam, P)
    with pytest.raises(ValueError):
        ops.pdl_stack_dual_data(q, None, g, x[:2 * n - 1], 0.3, lam, P)
    with pytest.raises(ValueError):
        ops.pdl_stack_dual_data(q, q, g, None, 0.3, lam, P)
    with pytest.raises(ValueError):
        ops.pdl_stack_dual_data(q, None, g, None, 0., lam, P)
    with pytest.raises(ValueError):
        ops.pdl_stack_dual_data(q, None, g, None, 0.3, lam[:1], P)
    torch.cuda.synchronize()
    assert ops.pdl_stack_launches() == before and ops.pdl_launches() == single
    for t in (x, xb, xo, g):
        assert torch.equal(t, torch.ones_like(t))
    assert not p0.any() and not p1.any() and not q.any()
    assert call() == 0                                  # and the good call runs
    torch.cuda.synchronize()
    assert ops.pdl_stack_launches() == before + 1 and ops.pdl_launches() == single


# --------------------------------------------------- 9. command line
def test_cli_result_dir_writes_every_member_of_the_sweep(nsol, golden, tmp_path, capsys):
    from nsol_amd.application import run_deconvolution
    from nsol_amd.application.run_denoising import member_result_path
    img = golden("configs")["phantom64"][32, :32, :40].astype(np.float64)
    obs, out, d = str(tmp_path / "obs.npy"), str(tmp_path / "out.npy"), \
        str(tmp_path / "members")
    np.save(obs, img)
    alphas = [0.02, 0.05]
    argv = ["--observation", obs, "--result", out, "--solver", "PDL", "--iterations",
            "12", "--blur", "1.0", "--result-dir", d, "--alpha", "0.02", "0.05"]
    assert run_deconvolution.main(argv) == 0
    text = capsys.readouterr().out
    assert text.count("(stacked)") == 2 and "sequentially" not in text
    for alpha in alphas:
        s = run_deconvolution.build_solver(img, np.ones(2), 1.0, "TVL2", "PDL", alpha, 12,
                                           dtype=np.float32)
        s.run()
        got = np.load(member_result_path(d, out, alpha))
        assert np.array_equal(got, s.get_x().reshape(img.shape)), alpha
    assert np.array_equal(np.load(out), got)              # --result: the last member
    z = np.load(str(tmp_path / "members" / "sweep.npz"))
    assert list(z["parameter_names"]) == ["alpha"]
    assert np.array_equal(z["parameters"], np.array(alphas).reshape(-1, 1))
    # with a tolerance the members run one after the other, and the tool says so
    assert run_deconvolution.main(argv + ["--tolerance", "1e-2", "--check-every",
                                          "4", "--nonnegative", "--isotropic"]) == 0
    text = capsys.readouterr().out
    assert "sequentially" in text and text.count("stopped after") == 2


def test_cli_slice_wise_equals_one_solver_per_slice(nsol, golden, tmp_path, capsys):
    from nsol_amd import nifti
    from nsol_amd.data_reader import DataReader
    from nsol_amd.application import run_deconvolution
    vol = golden("configs")["phantom64"][20:26, :24, :40].astype(np.float64)
    mask = np.ones(vol.shape)
    mask[:, 8:14, 10:30] = 0
    nii, mnii = str(tmp_path / "obs.nii.gz"), str(tmp_path / "mask.nii.gz")
    out = str(tmp_path / "out.nii.gz")
    nifti.write(nii, vol)
    nifti.write(mnii, mask)
    reader = DataReader(nii)
    reader.read_data()
    data = reader.get_data()
    assert data.shape == (6, 24, 40)
    spacing = np.array(reader.get_image_sitk().GetSpacing())
    argv = ["--observation", nii, "--result", out, "--solver", "PDL", "--iterations",
            "12", "--alpha", "0.03", "--blur", "1.0", "--slice-wise", "--mask", mnii]
    assert run_deconvolution.main(argv) == 0
    assert "6 slices stacked, 0 copied through, 0 sequential" in capsys.readouterr().out
    want = np.empty(data.shape)
    for k in range(6):
        s = run_deconvolution.build_solver(data[k], spacing[:2], 1.0, "TVL2", "PDL", 0.03,
                                           12, dtype=np.float32, weights=mask[k])
        assert s.get_x_scale() == data[k][mask[k] > 0].max()
        s.run()
        want[k] = s.get_x().reshape(data.shape[1:])
    got, _, _ = nifti.read(out)
    assert rel_l2(got, want) < 1e-6                      # a float32 file
