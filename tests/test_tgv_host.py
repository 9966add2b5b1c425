"""Second-order TGV without a GPU: the NumPy restatement (nsol_amd/tgv_numpy.py) --
adjoint identity, norm bound, that the iteration minimises the stated energy (against a
linear programme), that TGV beats TV on a piecewise-linear signal -- and the host logic
of TGVPrimalDualSolver, the build list, the C ABI's declarations and the command line."""
import numpy as np
import pytest

from nsol_amd import tgv_numpy as tg

# (shape, spacing): non-unit, unequal spacing; spacing[0] belongs to the last axis
ADJOINT_CASES = [((9,), (0.7,)), ((5, 6), (0.5, 2.0)), ((3, 4, 5), (0.8, 1.3, 2.0))]
BOUND_CASES = ADJOINT_CASES + [((5, 6), (1., 1.)), ((3, 4, 5), (1., 1., 1.))]


def _random_pair(shape, seed):
    rng = np.random.default_rng(seed)
    d = len(shape)
    M = tg.components(d)
    return (rng.standard_normal(shape), rng.standard_normal((d,) + shape),
            rng.standard_normal((d,) + shape), rng.standard_normal((M,) + shape))


def test_layout_of_the_symmetric_components():
    assert tg.pairs(1) == [] and tg.pairs(2) == [(0, 1)]
    assert tg.pairs(3) == [(0, 1), (0, 2), (1, 2)]          # xy, xz, yz after xx, yy, zz
    assert [tg.components(d) for d in (1, 2, 3)] == [1, 3, 6]
    assert list(tg.inner_weights(3)) == [1, 1, 1, 2, 2, 2]


def test_difference_is_zero_padded_with_component_0_on_the_last_axis():
    u = np.arange(6.).reshape(2, 3)
    np.testing.assert_array_equal(tg.D(u, 0, 2.), [[2, 2, -4], [2, 2, -10]])
    np.testing.assert_array_equal(tg.D(u, 1, 1.), [[3, 3, 3], [-3, -4, -5]])


@pytest.mark.parametrize("shape,spacing", ADJOINT_CASES)
def test_adjoint_identity(shape, spacing):
    x, w, p, q = _random_pair(shape, 11 + len(shape))
    g, e = tg.K(x, w, spacing)
    kx, kw = tg.K_adj(p, q, spacing)
    lhs = tg.inner_dual(g, e, p, q)
    rhs = float(np.sum(x * kx) + np.sum(w * kw))
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print("adjoint identity %r: relative difference %.3g" % (shape, rel))
    assert rel <= 1e-12


@pytest.mark.parametrize("shape,spacing", BOUND_CASES)
def test_norm_bound_holds(shape, spacing):
    """3 000 power iterations on K^T K in the doubled-off-diagonal geometry."""
    d = len(shape)
    x, w, _, _ = _random_pair(shape, 5)
    wq = tg.inner_weights(d).reshape((-1,) + (1,) * d)
    lam = 0.
    for _ in range(3000):
        g, e = tg.K(x, w, spacing)
        # K^T in the weighted inner product acts on (g, e) as they are: the weights are
        # part of the product, K_adj is its transpose
        kx, kw = tg.K_adj(g, e, spacing)
        lam = np.sqrt(np.sum(kx * kx) + np.sum(kw * kw))
        x, w = kx / lam, kw / lam
    g, e = tg.K(x, w, spacing)
    norm2 = float(np.sum(g * g) + np.sum(wq * e * e))
    bound = tg.norm_bound(d, spacing)
    print("|K|^2 %r h=%r: %.4f <= %.4f" % (shape, spacing, norm2, bound))
    assert norm2 <= bound
    assert norm2 >= 0.5 * bound          # the bound is not vacuous


def test_norm_bound_values():
    assert tg.norm_bound(3) == pytest.approx(16.0)
    assert tg.norm_bound(2) == pytest.approx(11.3723, abs=1e-4)
    assert tg.norm_bound(1, (0.7,)) == pytest.approx(11.56, abs=5e-3)


# ------------------------------------------------ the minimiser, by linear programming
LP_SHAPE, LP_SPACING, LP_ALPHA, LP_BETA = (5, 6), (1., 1.3), 0.8, 2.
# relative gap of the energy after 20 000 iterations measured on this instance (float64
# NumPy, deterministic); the test allows ten times as much for library differences
LP_GAP_20000 = 2.72e-7


def _lp_instance():
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:LP_SHAPE[0], 0:LP_SHAPE[1]]
    return 0.2 * xx + 0.1 * yy + (xx > 2) * 0.7 + 0.1 * rng.standard_normal(LP_SHAPE)


def _lp_optimum(b):
    """min lambda |x - b|_1 + |grad x - w|_1 + beta |E w|_1 as a linear programme in
    (x, w, slacks)."""
    from scipy.optimize import linprog
    shape, d = b.shape, b.ndim
    n, M = b.size, tg.components(d)
    nv = (1 + d) * n
    # the matrix of K, column by column
    rows = (d + M) * n
    Kmat = np.zeros((rows, nv))
    for j in range(nv):
        v = np.zeros(nv)
        v[j] = 1.
        g, e = tg.K(v[:n].reshape(shape), v[n:].reshape((d,) + shape), LP_SPACING)
        Kmat[:, j] = np.concatenate([g.reshape(-1), e.reshape(-1)])
    ns = n + rows                                     # slacks: data, then K's rows
    cost = np.concatenate([np.zeros(nv), np.full(n, 1. / LP_ALPHA), np.ones(d * n),
                           LP_BETA * np.repeat(tg.inner_weights(d), n)])
    # |r| <= s  as  r - s <= 0 and -r - s <= 0, r = A v - c
    A = np.vstack([np.hstack([np.eye(n), np.zeros((n, d * n))]), Kmat])
    c = np.concatenate([b.reshape(-1), np.zeros(rows)])
    I = np.eye(ns)
    A_ub = np.vstack([np.hstack([A, -I]), np.hstack([-A, -I])])
    b_ub = np.concatenate([c, -c])
    res = linprog(cost, A_ub=A_ub, b_ub=b_ub,
                  bounds=[(None, None)] * nv + [(0, None)] * ns, method="highs")
    assert res.status == 0, res.message
    return float(res.fun)


def test_iteration_minimises_the_stated_energy():
    b = _lp_instance()
    opt = _lp_optimum(b)
    gaps = {}
    for iters in (2000, 20000):
        r = tg.iterate(b, b, iters, LP_ALPHA, LP_BETA, LP_SPACING, data_loss="ell1")
        e = tg.energy(r["x"], r["w"], b, 1. / LP_ALPHA, LP_BETA, LP_SPACING, "ell1")
        gaps[iters] = (e - opt) / opt
        print("TGV-l1 energy after %d iterations: %.12g, LP optimum %.12g, relative "
              "gap %.3g" % (iters, e, opt, gaps[iters]))
    assert gaps[20000] >= -1e-9                 # the LP optimum is a lower bound
    assert abs(gaps[20000]) <= 10 * LP_GAP_20000
    assert abs(gaps[20000]) < abs(gaps[2000])


# ------------------------------------------------------------ what TGV is for
def _ramp_with_jump(n=256):
    t = np.arange(n) / float(n)
    return np.where(t < 0.5, 0.2 + 1.2 * t, 1.4 - 1.6 * (t - 0.5))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tgv_beats_tv_on_a_piecewise_linear_signal(seed):
    truth = _ramp_with_jump()
    b = truth + 0.05 * np.random.default_rng(seed).standard_normal(truth.size)
    alphas = (0.02, 0.05, 0.1, 0.2, 0.4, 0.8)
    rmse = lambda x: float(np.sqrt(np.mean((x - truth) ** 2)))
    tgv = min(rmse(tg.iterate(b, b, 3000, a, 2.)["x"]) for a in alphas)
    tv = min(rmse(tg.tv_iterate(b, b, 3000, a)) for a in alphas)
    print("seed %d: best RMSE TGV %.4f, TV %.4f" % (seed, tgv, tv))
    assert tgv < tv


def test_ratios_are_the_stopping_rules():
    b = _lp_instance()
    r1 = tg.iterate(b, b, 3, 0.5, keep=True)
    r0 = tg.iterate(b, b, 2, 0.5)
    assert r1["ratios"].shape == (3, 3) and len(r1["iterates"]) == 4
    num = np.sum((r1["x"] - r0["x"]) ** 2) + np.sum((r1["w"] - r0["w"]) ** 2)
    den = np.sum(r1["x"] ** 2) + np.sum(r1["w"] ** 2)
    assert r1["ratios"][2, 1] == pytest.approx(np.sqrt(num / den), rel=1e-12)
    assert tg.iterate(b, b, 2, 0.5, dtype=np.float32)["x"].dtype == np.float32


# ------------------------------------------------------------------- host logic
def _solver(**kw):
    from nsol_amd.tgv_solver import TGVPrimalDualSolver
    b = np.arange(30.)
    args = dict(b=b, x0=b.copy(), dimension=2, shape=(5, 6))
    args.update(kw)
    return TGVPrimalDualSolver(**args)


@pytest.mark.parametrize("bad", [
    dict(dimension=0), dict(dimension=4), dict(dimension=2.5),
    dict(shape=(5, 7)), dict(shape=(30,)), dict(shape=(5, 6, 1)), dict(shape=None),
    dict(x0=np.zeros(29)),
    dict(alpha=0.), dict(alpha=-1.), dict(alpha=np.inf), dict(alpha=np.nan),
    dict(beta=0.), dict(beta=-2.), dict(beta=np.inf), dict(beta=np.nan),
    dict(spacing=(1., 0.)), dict(spacing=(1., -1.)), dict(spacing=(1., np.inf)),
    dict(spacing=(1., np.nan)), dict(spacing=(1., 1., 1.)),
    dict(data_loss="huber"),
    dict(L2=0.), dict(L2=-1.), dict(L2=np.nan), dict(tau=-1.), dict(sigma=0.),
    dict(tau=1., sigma=1.),                       # tau sigma L2 > 1
    dict(tolerance=-1.), dict(check_every=0), dict(dtype=np.float16),
])
def test_constructor_refuses(bad):
    with pytest.raises(ValueError):
        _solver(**bad)


def test_constructor_defaults():
    s = _solver(spacing=(0.5, 2.))
    L2 = tg.norm_bound(2, (0.5, 2.))
    assert s.get_L2() == pytest.approx(L2) and L2 == pytest.approx(21.65, abs=5e-3)
    assert s.get_tau() == s.get_sigma() == pytest.approx(1. / np.sqrt(L2))
    assert s.get_theta() == 1. and s.get_beta() == 2. and s.get_alpha() == 0.01
    assert s.get_execution() == "fused" and s.get_shape() == (5, 6)
    assert s.get_iterations_done() is None and s.get_stop_reason() is None
    assert s.get_changes().shape == (0, 3)
    assert s.get_w().shape == (60,) and not s.get_w().any()
    np.testing.assert_array_equal(s.get_x(), np.arange(30.))
    s = _solver(L2=20., tau=0.1)
    assert s.get_sigma() == pytest.approx(0.5)
    assert _solver(dimension=1, shape=None).get_shape() == (30,)
    assert _solver(b=np.zeros((5, 6)), x0=np.zeros(30), shape=None).get_shape() == (5, 6)
    import nsol_amd
    assert nsol_amd.TGVPrimalDualSolver is type(s)


def test_build_list_and_declarations():
    from nsol_amd import _lib, build
    assert "nsol_tgv.hip" in build.SOURCES
    syms = _lib.declared_symbols()
    for name in ("nsol_tgv_dual_f32", "nsol_tgv_dual_f64", "nsol_tgv_primal_f32",
                 "nsol_tgv_primal_f64", "nsol_tgv_launches"):
        assert name in syms
    assert len(syms["nsol_tgv_dual_f32"][1]) == 15
    assert len(syms["nsol_tgv_primal_f64"][1]) == 19
    assert syms["nsol_tgv_launches"][1] == []


# ----------------------------------------------------------------- command line
def _parse(*extra):
    from nsol_amd.application import run_denoising
    return run_denoising.parse_args(["--observation", "in.npy", "--result", "out.npy"] +
                                    list(extra))


def test_cli_takes_the_tgv_types():
    a = _parse("--reconstruction-type", "TGVL2")
    assert a.beta == 2.0 and a.L2 is None
    a = _parse("--reconstruction-type", "TGVL1", "--beta", "1.5", "--isotropic",
               "--tolerance", "1e-4", "--check-every", "5", "--dtype", "float64",
               "--observe-every", "10", "--L2", "20")
    assert a.beta == 1.5 and a.L2 == 20. and a.isotropic and a.observe_every == 10


def test_cli_keeps_the_l2_of_the_existing_types():
    for t in ("TVL1", "TVL2", "HuberL1", "HuberL2"):
        assert _parse("--reconstruction-type", t).L2 == 8
    assert _parse("--L2", "12").L2 == 12.


@pytest.mark.parametrize("extra,named", [
    (("--alpha", "0.1", "0.2"), "--alpha"),
    (("--slice-wise",), "--slice-wise"),
    (("--mask", "m.npy"), "--mask"),
    (("--weights", "w.npy"), "--weights"),
    (("--alg-type", "ALG3"), "--alg-type"),
    (("--beta", "0"), "--beta"),
])
def test_cli_refuses(extra, named, capsys):
    with pytest.raises(SystemExit) as e:
        _parse("--reconstruction-type", "TGVL2", *extra)
    assert e.value.code != 0
    assert named in capsys.readouterr().err


def test_cli_refuses_beta_without_tgv(capsys):
    with pytest.raises(SystemExit):
        _parse("--reconstruction-type", "TVL2", "--beta", "2")
    assert "--beta" in capsys.readouterr().err
