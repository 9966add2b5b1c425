"""TGV behind a linear operator, and weighted TGV, without a GPU: the NumPy restatement
(tgv_numpy.iterate_linear, primal_step_lin, primal_step_weighted, norm_bound_linear) --
adjoint identity of the extended map K(x, w) = (grad x - w, E w, A x), its norm bound,
that the iteration minimises the stated energy (against a linear programme with weights
and a box), the reductions to the denoising iteration -- and the host logic of
TGVPrimalDualLinearSolver and TGVPrimalDualSolver(weights=), the C ABI's declarations
and run_deconvolution's parser."""
import numpy as np
import pytest

from nsol_amd import tgv_numpy as tg

# (shape, spacing, sampling factors per array axis)
CASES = [((9,), (0.7,), (3,)), ((5, 6), (0.5, 2.0), (1, 2)),
         ((3, 4, 5), (0.8, 1.3, 2.0), (1, 2, 1))]
BOUND_CASES = [((9,), (0.7,)), ((5, 6), (1., 1.)), ((5, 6), (0.5, 2.0)),
               ((3, 4, 5), (1., 1., 1.)), ((3, 4, 5), (0.8, 1.3, 2.0))]


def _taps(sigma=1., r=3):
    t = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    return t / t.sum()


def _blur(x, taps=None):
    """The separable `wrap` blur: non-negative taps of sum 1, so |A|^2 = 1."""
    taps = _taps() if taps is None else taps
    r = len(taps) // 2
    for ax in range(x.ndim):
        x = sum(t * np.roll(x, k - r, axis=ax) for k, t in enumerate(taps))
    return x


def _dense(fn, shape):
    n = int(np.prod(shape))
    cols = []
    for j in range(n):
        v = np.zeros(n)
        v[j] = 1.
        cols.append(np.asarray(fn(v.reshape(shape))).reshape(-1))
    return np.stack(cols, axis=1)


def _operators(shape, factors=None, taps=None):
    """(A, A_adj, m) as callables on arrays through the DENSE matrix of the blur, or of
    blur-then-sample (every F-th sample per axis)."""
    if factors is None:
        fn = lambda x: _blur(x, taps)
    else:
        keep = tuple(slice(None, None, f) for f in factors)
        fn = lambda x: _blur(x, taps)[keep]
    mat = _dense(fn, shape)
    A = lambda x: mat @ np.asarray(x).reshape(-1)
    A_adj = lambda r: (mat.T @ np.asarray(r).reshape(-1)).reshape(shape)
    return A, A_adj, mat.shape[0]


def _state(shape, m, seed):
    rng = np.random.default_rng(seed)
    d = len(shape)
    M = tg.components(d)
    return (rng.standard_normal(shape), rng.standard_normal((d,) + shape),
            rng.standard_normal((d,) + shape), rng.standard_normal((M,) + shape),
            rng.standard_normal(m))


# ------------------------------------------------------------------ the extended map
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("shape,spacing,factors", CASES)
def test_adjoint_identity_of_the_extended_map(shape, spacing, factors, sampled):
    A, A_adj, m = _operators(shape, factors if sampled else None)
    assert m == (int(np.prod([-(-s // f) for s, f in zip(shape, factors)])) if sampled
                 else int(np.prod(shape)))
    x, w, p, q, r = _state(shape, m, 21 + len(shape))
    g, e = tg.K(x, w, spacing)
    kx, kw = tg.K_adj(p, q, spacing)
    kx = kx + A_adj(r)
    lhs = tg.inner_dual(g, e, p, q) + float(np.sum(A(x) * r))
    rhs = float(np.sum(x * kx) + np.sum(w * kw))
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print("adjoint identity %r sampled=%s: relative difference %.3g" % (shape, sampled, rel))
    assert rel <= 1e-12


@pytest.mark.parametrize("shape,spacing", BOUND_CASES)
def test_norm_bound_linear_holds(shape, spacing):
    """3 000 power iterations on K^T K with the 7-tap Gaussian (sigma 1, wrap, |A|^2 = 1)."""
    d = len(shape)
    A, A_adj, m = _operators(shape)
    x, w, _, _, _ = _state(shape, m, 5)
    wq = tg.inner_weights(d).reshape((-1,) + (1,) * d)
    for _ in range(3000):
        g, e = tg.K(x, w, spacing)
        kx, kw = tg.K_adj(g, e, spacing)
        kx = kx + A_adj(A(x))
        lam = np.sqrt(np.sum(kx * kx) + np.sum(kw * kw))
        x, w = kx / lam, kw / lam
    g, e = tg.K(x, w, spacing)
    t = A(x)
    norm2 = float(np.sum(g * g) + np.sum(wq * e * e) + np.sum(t * t))
    bound = tg.norm_bound_linear(d, spacing, 1.)
    print("|K|^2 %r h=%r: %.4f <= %.4f" % (shape, spacing, norm2, bound))
    assert norm2 <= bound
    assert norm2 >= 0.5 * bound          # the bound is not vacuous
    assert bound <= tg.norm_bound(d, spacing) + 1.


@pytest.mark.parametrize("shape,spacing", BOUND_CASES)
def test_norm_bound_linear_reduces_and_is_below_the_crude_sum(shape, spacing):
    d = len(shape)
    assert tg.norm_bound_linear(d, spacing, 0.) == tg.norm_bound(d, spacing)   # the bits
    assert tg.norm_bound_linear(d, None, 0.) == tg.norm_bound(d)
    for a in (0.25, 1., 4., 100.):
        assert tg.norm_bound_linear(d, spacing, a) <= tg.norm_bound(d, spacing) + a
        # the largest eigenvalue of [[g + a, sqrt g], [sqrt g, 1 + g]]
        g = 4. * float(np.sum(1. / np.asarray(spacing) ** 2))
        top = np.linalg.eigvalsh(np.array([[g + a, np.sqrt(g)], [np.sqrt(g), 1. + g]]))[-1]
        assert tg.norm_bound_linear(d, spacing, a) == pytest.approx(top, rel=1e-12)


def test_norm_bound_linear_values():
    # the table of DESIGN section 4j (A_norm2 = 1)
    for (shape, spacing), want in zip(BOUND_CASES, (12.02, 11.83, 22.12, 16.46, 13.72)):
        assert tg.norm_bound_linear(len(shape), spacing, 1.) == pytest.approx(want, abs=6e-3)


# ------------------------------------------------ the minimiser, by linear programming
LP_SHAPE, LP_SPACING, LP_ALPHA, LP_BETA = (5, 6), (1., 1.3), 0.8, 2.
LP_BOX = (0.3, 1.4)
LP_ITERATIONS = 20000
# relative gap of the energy after LP_ITERATIONS iterations measured on this instance
# (float64 NumPy, deterministic); the test allows ten times as much for library
# differences, the margin of test_tgv_host's LP test
LP_GAP = 3.36e-6


def _lp_instance():
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:LP_SHAPE[0], 0:LP_SHAPE[1]]
    b = 0.2 * xx + 0.1 * yy + (xx > 2) * 0.7 + 0.1 * rng.standard_normal(LP_SHAPE)
    wt = rng.uniform(0.2, 2., LP_SHAPE)
    wt[rng.uniform(size=LP_SHAPE) < 0.25] = 0.
    return b, wt


def _lp_optimum(b, wt, mat):
    """min lambda sum wt_i |(A x - b)_i| + |grad x - w|_1 + beta |E w|_1 over lo <= x <= hi
    as a linear programme in (x, w, slacks): test_tgv_host's, with A's matrix in the data
    rows, the weights in their cost and the box as bounds of x."""
    from scipy.optimize import linprog
    shape, d = b.shape, b.ndim
    n, M = b.size, tg.components(d)
    nv = (1 + d) * n
    rows = (d + M) * n
    Kmat = np.zeros((rows, nv))
    for j in range(nv):
        v = np.zeros(nv)
        v[j] = 1.
        g, e = tg.K(v[:n].reshape(shape), v[n:].reshape((d,) + shape), LP_SPACING)
        Kmat[:, j] = np.concatenate([g.reshape(-1), e.reshape(-1)])
    m = mat.shape[0]
    ns = m + rows
    cost = np.concatenate([np.zeros(nv), wt.reshape(-1) / LP_ALPHA, np.ones(d * n),
                           LP_BETA * np.repeat(tg.inner_weights(d), n)])
    A = np.vstack([np.hstack([mat, np.zeros((m, d * n))]), Kmat])
    c = np.concatenate([b.reshape(-1), np.zeros(rows)])
    I = np.eye(ns)
    A_ub = np.vstack([np.hstack([A, -I]), np.hstack([-A, -I])])
    b_ub = np.concatenate([c, -c])
    res = linprog(cost, A_ub=A_ub, b_ub=b_ub,
                  bounds=[LP_BOX] * n + [(None, None)] * (d * n) + [(0, None)] * ns,
                  method="highs")
    assert res.status == 0, res.message
    return float(res.fun), res.x[:n]


def test_iteration_minimises_the_stated_energy():
    b, wt = _lp_instance()
    assert (wt == 0).sum() >= 3
    taps = np.array([0.25, 0.5, 0.25])
    mat = _dense(lambda x: _blur(x, taps), LP_SHAPE)
    A = lambda x: mat @ x.reshape(-1)
    A_adj = lambda r: (mat.T @ r.reshape(-1)).reshape(LP_SHAPE)
    opt, x_lp = _lp_optimum(b, wt, mat)
    # the box is active in the optimum: the projection is part of what is tested
    assert np.isclose(x_lp, LP_BOX[0]).any() or np.isclose(x_lp, LP_BOX[1]).any()
    gaps = {}
    x0 = np.clip(b, *LP_BOX)
    for iters in (LP_ITERATIONS // 10, LP_ITERATIONS):
        r = tg.iterate_linear(A, A_adj, b.reshape(-1), x0, iters, LP_ALPHA, LP_BETA,
                              LP_SPACING, data_loss="ell1", weights=wt.reshape(-1),
                              bounds=LP_BOX, A_norm2=1.)
        assert r["x"].min() >= LP_BOX[0] and r["x"].max() <= LP_BOX[1]
        e = tg.energy_linear(r["x"], r["w"], A(r["x"]), b, 1. / LP_ALPHA, LP_BETA,
                             LP_SPACING, "ell1", weights=wt)
        gaps[iters] = (e - opt) / opt
        print("TGV-l1 (linear) energy after %d iterations: %.12g, LP optimum %.12g, "
              "relative gap %.3g" % (iters, e, opt, gaps[iters]))
    assert gaps[LP_ITERATIONS] >= -1e-9          # the LP optimum is a lower bound
    assert abs(gaps[LP_ITERATIONS]) <= 10 * LP_GAP
    assert abs(gaps[LP_ITERATIONS]) < abs(gaps[LP_ITERATIONS // 10])


# ------------------------------------------------ reductions to the existing iteration
def test_identity_operator_reaches_the_denoising_energy():
    """A = identity, no box, no weights: another iteration on the denoising problem.  The
    iterates differ (the data term is dualised), the energies in the limit do not."""
    b, _ = _lp_instance()
    ident = lambda t: np.asarray(t).reshape(b.shape)
    for loss in ("ell2", "ell1"):
        lin = tg.iterate_linear(ident, ident, b, b, 6000, LP_ALPHA, LP_BETA, LP_SPACING,
                                data_loss=loss, A_norm2=1.)
        den = tg.iterate(b, b, 6000, LP_ALPHA, LP_BETA, LP_SPACING, data_loss=loss)
        e_lin = tg.energy_linear(lin["x"], lin["w"], lin["x"], b, 1. / LP_ALPHA, LP_BETA,
                                 LP_SPACING, loss)
        e_den = tg.energy(den["x"], den["w"], b, 1. / LP_ALPHA, LP_BETA, LP_SPACING, loss)
        # energy_linear with A = identity IS energy
        assert e_lin == pytest.approx(
            tg.energy(lin["x"], lin["w"], b, 1. / LP_ALPHA, LP_BETA, LP_SPACING, loss),
            rel=1e-14)
        print("%s: energy linear %.10g, denoising %.10g, relative difference %.3g" %
              (loss, e_lin, e_den, abs(e_lin - e_den) / e_den))
        # both iterations are O(1/N) on a 30-voxel instance and N = 6000: each is within
        # 1e-3 of the optimum by the gaps of the two LP tests (6.9e-4 at 2 000 iterations
        # here).  Measured differences: 3e-11 (l2), 8.9e-5 (l1).
        assert abs(e_lin - e_den) <= 1e-3 * e_den


@pytest.mark.parametrize("loss", ["ell2", "ell1"])
def test_unit_weights_are_the_unweighted_iteration(loss):
    b, _ = _lp_instance()
    plain = tg.iterate(b, b, 40, LP_ALPHA, LP_BETA, LP_SPACING, data_loss=loss)
    ones = tg.iterate(b, b, 40, LP_ALPHA, LP_BETA, LP_SPACING, data_loss=loss,
                      weights=np.ones(b.shape))
    for k in ("x", "w", "p", "q", "ratios"):
        np.testing.assert_array_equal(plain[k], ones[k])


@pytest.mark.parametrize("loss", ["ell2", "ell1"])
def test_masked_out_nan_never_enters(loss):
    b, wt = _lp_instance()
    zeroed, holed = np.where(wt == 0, 0., b), np.where(wt == 0, np.nan, b)
    x0 = zeroed.copy()
    a = tg.iterate(zeroed, x0, 30, LP_ALPHA, LP_BETA, LP_SPACING, data_loss=loss, weights=wt)
    c = tg.iterate(holed, x0, 30, LP_ALPHA, LP_BETA, LP_SPACING, data_loss=loss, weights=wt)
    for k in ("x", "w", "p", "q"):
        assert np.isfinite(c[k]).all()
        np.testing.assert_array_equal(a[k].view(np.uint64), c[k].view(np.uint64))
    A, A_adj, _ = _operators(LP_SHAPE, taps=np.array([0.25, 0.5, 0.25]))
    kw = dict(data_loss=loss, weights=wt.reshape(-1), bounds=(0., np.inf), A_norm2=1.)
    a = tg.iterate_linear(A, A_adj, zeroed.reshape(-1), x0, 30, LP_ALPHA, LP_BETA,
                          LP_SPACING, **kw)
    c = tg.iterate_linear(A, A_adj, holed.reshape(-1), x0, 30, LP_ALPHA, LP_BETA,
                          LP_SPACING, **kw)
    for k in ("x", "w", "p", "q", "r"):
        assert np.isfinite(c[k]).all()
        np.testing.assert_array_equal(a[k].view(np.uint64), c[k].view(np.uint64))


def test_ratios_are_the_stopping_rules_with_r():
    b, wt = _lp_instance()
    A, A_adj, m = _operators(LP_SHAPE, (1, 2))
    bc = b[:, ::2].reshape(-1)
    kw = dict(weights=wt[:, ::2].reshape(-1), bounds=(0.3, np.inf), A_norm2=1.)
    r1 = tg.iterate_linear(A, A_adj, bc, b, 3, 0.5, keep=True, **kw)
    r0 = tg.iterate_linear(A, A_adj, bc, b, 2, 0.5, **kw)
    assert r1["ratios"].shape == (3, 3) and len(r1["iterates"]) == 4
    assert r1["r"].shape == (m,) and r1["x"].shape == LP_SHAPE
    sq = lambda *t: sum(float(np.sum(v ** 2)) for v in t)
    num = sq(r1["x"] - r0["x"], r1["w"] - r0["w"])
    assert r1["ratios"][2, 1] == pytest.approx(np.sqrt(num / sq(r1["x"], r1["w"])),
                                               rel=1e-12)
    num = sq(r1["p"] - r0["p"], r1["q"] - r0["q"], r1["r"] - r0["r"])
    den = sq(r1["p"], r1["q"], r1["r"])
    assert r1["ratios"][2, 2] == pytest.approx(np.sqrt(num / den), rel=1e-12)
    # without r the dual ratio is another number
    assert abs(np.sqrt(sq(r1["p"] - r0["p"], r1["q"] - r0["q"]) / sq(r1["p"], r1["q"])) -
               r1["ratios"][2, 2]) > 1e-6
    assert tg.iterate_linear(A, A_adj, bc, b, 2, 0.5, dtype=np.float32,
                             **kw)["x"].dtype == np.float32
    with pytest.raises(ValueError, match="A_norm2"):
        tg.iterate_linear(A, A_adj, bc, b, 2, 0.5)


def test_steps_of_the_restatement():
    b, _ = _lp_instance()
    A, A_adj, _ = _operators(LP_SHAPE)
    r = tg.iterate_linear(A, A_adj, b.reshape(-1), b, 1, 0.5, spacing=LP_SPACING,
                          A_norm2=1.)
    L2 = tg.norm_bound_linear(2, LP_SPACING, 1.)
    assert r["tau"] == r["sigma"] == pytest.approx(1. / np.sqrt(L2), rel=1e-15)


# ------------------------------------------------------------------- host logic
SHAPE = (5, 6)


def _own_blur(shape=SHAPE):
    from nsol_amd.linear_operators import ConvolutionOperator
    k = _taps()
    for _ in range(len(shape) - 1):
        k = np.multiply.outer(k, _taps())
    op = ConvolutionOperator(len(shape), k)
    return lambda x: op(x.reshape(*shape)).flatten()


def _linear(**kw):
    from nsol_amd.tgv_solver import TGVPrimalDualLinearSolver
    b = 1. + np.arange(30.)
    A1 = _own_blur()
    args = dict(A=A1, A_adj=A1, b=b, x0=b.copy(), dimension=2)
    args.update(kw)
    return TGVPrimalDualLinearSolver(**args)


def _denoiser(**kw):
    from nsol_amd.tgv_solver import TGVPrimalDualSolver
    b = np.arange(30.)
    args = dict(b=b, x0=b.copy(), dimension=2, shape=SHAPE)
    args.update(kw)
    return TGVPrimalDualSolver(**args)


_FOREIGN = lambda x: np.asarray(x) * 0.5
_BAD_WEIGHTS = [dict(weights=-np.ones(30)), dict(weights=np.full(30, np.nan)),
                dict(weights=np.ones(29)), dict(weights=np.ones(30) * 1j)]


@pytest.mark.parametrize("bad", [
    dict(dimension=0), dict(dimension=4), dict(dimension=2.5),
    dict(shape=(5, 7)), dict(shape=(30,)), dict(shape=(5, 6, 1)),
    dict(x0=np.zeros(29)),
    dict(alpha=0.), dict(alpha=-1.), dict(alpha=np.inf), dict(alpha=np.nan),
    dict(beta=0.), dict(beta=-2.), dict(beta=np.inf), dict(beta=np.nan),
    dict(spacing=(1., 0.)), dict(spacing=(1., -1.)), dict(spacing=(1., np.inf)),
    dict(spacing=(1., np.nan)), dict(spacing=(1., 1., 1.)),
    dict(data_loss="huber"),
    dict(L2=0.), dict(L2=-1.), dict(L2=np.nan), dict(tau=-1.), dict(sigma=0.),
    dict(tau=1., sigma=1.),                       # tau sigma L2 > 1
    dict(tolerance=-1.), dict(check_every=0), dict(dtype=np.float16),
    dict(bounds=(1., 0.)), dict(bounds=(np.nan, 1.)), dict(bounds=3.),
    dict(A_norm2=-1.), dict(A_norm2=np.inf),
    dict(A=_FOREIGN, A_adj=_FOREIGN, shape=SHAPE),              # A_norm2 is missing
    dict(A=_FOREIGN, A_adj=_FOREIGN, A_norm2=0.25),             # the shape is not known
] + _BAD_WEIGHTS)
def test_linear_constructor_refuses(bad):
    with pytest.raises(ValueError):
        _linear(**bad)


@pytest.mark.parametrize("bad", _BAD_WEIGHTS)
def test_weighted_denoiser_refuses_bad_weights(bad):
    with pytest.raises(ValueError):
        _denoiser(**bad)


def test_linear_constructor_defaults():
    import nsol_amd
    from nsol_amd.primal_dual_linear_solver import PrimalDualLinearSolver
    from nsol_amd.solver import Solver
    s = _linear(spacing=(0.5, 2.))
    # the two linear solvers share a base, not each other: a TGV solver is no member of
    # PrimalDualLinearSolver's stacks and has no reg_type
    assert isinstance(s, Solver) and not isinstance(s, PrimalDualLinearSolver)
    assert type(s).__mro__[1] is PrimalDualLinearSolver.__mro__[1]
    assert not hasattr(s, "get_reg_type") and not hasattr(s, "set_huber_gamma")
    assert nsol_amd.TGVPrimalDualLinearSolver is type(s)
    L2 = tg.norm_bound_linear(2, (0.5, 2.), 1.)
    assert abs(s.get_A_norm2() - 1.) <= 1e-12                  # Young's bound
    assert s.get_L2() == pytest.approx(L2, rel=1e-12) and L2 == pytest.approx(22.12, abs=5e-3)
    assert s.get_tau() == s.get_sigma() == pytest.approx(1. / np.sqrt(L2))
    assert s.get_theta() == 1. and s.get_beta() == 2. and s.get_alpha() == 0.01
    assert s.get_execution() == "fused" and s.get_shape() == SHAPE
    assert s.get_bounds() == (-np.inf, np.inf) and s.get_data_loss() == "ell2"
    assert s.get_iterations_done() is None and s.get_stop_reason() is None
    assert s.get_changes().shape == (0, 3)
    assert s.get_w().shape == (60,) and not s.get_w().any()
    np.testing.assert_array_equal(s.get_x(), 1. + np.arange(30.))
    s = _linear(L2=20., tau=0.1, bounds=(0., np.inf), weights=np.ones(30), beta=1.5,
                data_loss="ell1", isotropic=True)
    assert s.get_sigma() == pytest.approx(0.5) and s.get_bounds() == (0., np.inf)
    assert s.get_beta() == 1.5 and s.get_isotropic() and s.get_data_loss() == "ell1"
    # a foreign callable: the bound from the given A_norm2, the execution form not yet known
    s = _linear(A=_FOREIGN, A_adj=_FOREIGN, A_norm2=0.25, shape=SHAPE)
    assert s.get_execution() is None
    assert s.get_L2() == pytest.approx(tg.norm_bound_linear(2, None, 0.25), rel=1e-12)
    # the plain linear solver keeps its own default
    A1 = _own_blur()
    b = 1. + np.arange(30.)
    assert abs(PrimalDualLinearSolver(A1, A1, b, b, 2).get_L2() - 9.) <= 1e-12


def test_sampled_operator_puts_b_and_the_weights_on_the_coarse_grid():
    from nsol_amd.linear_operators import LinearOperators2D
    fine, coarse = (6, 8), (3, 4)
    A, A_adj = LinearOperators2D().get_sampled_gaussian_blurring_operators(
        np.diag([1., 1.]), (2, 2), None, fine_shape=fine)
    A1 = lambda x: A(x.reshape(*fine)).flatten()
    At1 = lambda r: A_adj(r.reshape(*coarse)).flatten()
    s = _linear(A=A1, A_adj=At1, b=np.ones(12), x0=np.ones(48), weights=np.ones(12))
    assert s.get_execution() == "fused" and s.get_shape() == fine
    assert s.get_w().shape == (96,)
    with pytest.raises(ValueError):
        _linear(A=A1, A_adj=At1, b=np.ones(12), x0=np.ones(48), weights=np.ones(48))


def test_weighted_denoiser_defaults():
    s = _denoiser()
    assert s.get_weights() is None
    wt = np.linspace(0., 2., 30)
    s = _denoiser(weights=wt)
    assert s.get_weights() is wt and s.get_execution() == "fused"
    assert _denoiser(weights=np.ones(30, dtype=bool)).get_L2() == _denoiser().get_L2()


def test_declarations_of_the_new_entries():
    from nsol_amd import _lib
    syms = _lib.declared_symbols()
    for name, nargs in (("nsol_tgv_primal_w_f32", 20), ("nsol_tgv_primal_w_f64", 20),
                        ("nsol_tgv_primal_lin_f32", 19), ("nsol_tgv_primal_lin_f64", 19)):
        assert name in syms, name
        assert len(syms[name][1]) == nargs, (name, len(syms[name][1]))
    from nsol_amd import ops
    assert callable(ops.tgv_primal_w) and callable(ops.tgv_primal_lin)


# ----------------------------------------------------------------- command line
def _parse(*extra):
    from nsol_amd.application import run_deconvolution
    return run_deconvolution.parse_args(
        ["--observation", "in.npy", "--result", "out.npy"] + list(extra))


def test_cli_takes_tgv_with_the_linear_solver():
    a = _parse("--solver", "PDL", "--reconstruction-type", "TGVL2")
    assert a.beta == 2.0 and a.data_loss == "linear"
    a = _parse("--solver", "PDL", "--reconstruction-type", "TGVL2", "--beta", "1.5",
               "--data-loss", "ell1", "--mask", "m.npy", "--nonnegative", "--isotropic",
               "--tolerance", "1e-4", "--check-every", "5", "--upsample", "2", "1",
               "--sample-offset", "1", "0", "--observe-every", "10", "--dtype", "float64",
               "--alpha", "0.1", "0.2")
    assert a.beta == 1.5 and a.data_loss == "ell1" and a.mask == "m.npy"
    assert a.nonnegative and a.isotropic and a.tolerance == 1e-4 and a.check_every == 5
    assert a.upsample == [2, 1] and a.sample_offset == [1, 0] and a.observe_every == 10
    assert a.dtype == "float64" and a.alpha == [0.1, 0.2]
    assert _parse("--solver", "PDL", "--reconstruction-type", "TGVL2", "--weights",
                  "w.npy").weights == "w.npy"


def test_cli_keeps_the_existing_types():
    a = _parse()
    assert a.reconstruction_type == "TVL2" and a.solver == "PD" and a.beta is None
    assert a.L2 == 8
    a = _parse("--solver", "PDL", "--reconstruction-type", "HuberL2", "--result-dir", "d",
               "--alpha", "0.1", "0.2")
    assert a.result_dir == "d" and a.beta is None
    assert _parse("--solver", "PDL", "--slice-wise").slice_wise
    assert _parse("--solver", "PDL", "--reconstruction-type", "TGVL2", "--L2", "12").L2 == 12.


@pytest.mark.parametrize("extra,named", [
    (("--reconstruction-type", "TGVL2"), "--solver"),                    # PD by default
    (("--reconstruction-type", "TGVL2", "--solver", "PD"), "--solver"),
    (("--reconstruction-type", "TGVL2", "--solver", "ADMM"), "--solver"),
    (("--solver", "PDL", "--beta", "2"), "--beta"),
    (("--solver", "PDL", "--reconstruction-type", "HuberL2", "--beta", "2"), "--beta"),
    (("--beta", "2"), "--beta"),
    (("--solver", "PDL", "--reconstruction-type", "TGVL2", "--beta", "0"), "--beta"),
    (("--solver", "PDL", "--reconstruction-type", "TGVL2", "--beta", "-1"), "--beta"),
    (("--solver", "PDL", "--reconstruction-type", "TGVL2", "--beta", "nan"), "--beta"),
    (("--solver", "PDL", "--reconstruction-type", "TGVL2", "--result-dir", "d"),
     "--result-dir"),
    (("--solver", "PDL", "--reconstruction-type", "TGVL2", "--slice-wise"), "--slice-wise"),
    (("--solver", "PDL", "--reconstruction-type", "TGVL2", "--data-loss", "huber"),
     "--data-loss"),
    (("--solver", "PDL", "--reconstruction-type", "TK0L2"), "--solver PDL"),
])
def test_cli_refuses(extra, named, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*extra)
    assert e.value.code != 0
    assert named in capsys.readouterr().err


def test_build_solver_wires_tgv():
    from nsol_amd.application import run_deconvolution as rd
    from nsol_amd.tgv_solver import TGVPrimalDualLinearSolver
    obs = 1. + np.arange(48.).reshape(6, 8)
    wt = np.ones((6, 8))
    wt[0, :3] = 0
    s = rd.build_solver(obs, np.ones(2), 1.2, "TGVL2", "PDL", 0.05, 7, weights=wt,
                        pdl_data_loss="ell1", nonnegative=True, isotropic=True, beta=1.5,
                        tolerance=1e-3, check_every=4, dtype=np.float64)
    assert isinstance(s, TGVPrimalDualLinearSolver)
    assert s.get_execution() == "fused" and s.get_shape() == (6, 8)
    assert s.get_beta() == 1.5 and s.get_data_loss() == "ell1" and s.get_isotropic()
    assert s.get_bounds() == (0., np.inf) and s.get_iterations() == 7
    assert s.get_L2() == pytest.approx(tg.norm_bound_linear(2, None, s.get_A_norm2()))
    # (--upsample forms its start on the device: test_tgv_linear_gpu.py)
    with pytest.raises(ValueError, match="PDL"):
        rd.build_solver(obs, np.ones(2), 1.2, "TGVL2", "PD")
