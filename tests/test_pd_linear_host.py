"""CPU-only side of PrimalDualLinearSolver (the primal-dual iteration with the data
term behind a linear operator A): the NumPy float64 restatement the GPU tests are
held to, its own check against a quasi-Newton minimiser of the same smooth objective,
and the host logic -- step sizes, the operator norm, the refusals, the declared
symbols and the command-line arguments."""
import numpy as np
import pytest

from nsol_amd import vector_numpy as vn
from test_pd_isotropic_host import project_iso


# ------------------------------------------------------------------ yardstick
def gaussian_kernel(dim, sigma, cut=3.):
    """Normalised separable Gaussian with odd extent 2 ceil(cut sigma) + 1 per axis."""
    r = int(np.ceil(cut * sigma))
    t = np.exp(-0.5 * (np.arange(-r, r + 1) / float(sigma)) ** 2)
    t /= t.sum()
    k = t
    for _ in range(dim - 1):
        k = np.multiply.outer(k, t)
    return k


def box_kernel(dim):
    """The separable 3-tap kernel (1/4, 1/2, 1/4) per axis."""
    t = np.array([0.25, 0.5, 0.25])
    k = t
    for _ in range(dim - 1):
        k = np.multiply.outer(k, t)
    return k


def separable_taps(kernel):
    """The 1-D factors of a normalised rank-1 kernel (its marginals), one per axis."""
    kernel = np.asarray(kernel, np.float64)
    taps = [kernel.sum(axis=tuple(b for b in range(kernel.ndim) if b != a))
            for a in range(kernel.ndim)]
    back = taps[0]
    for t in taps[1:]:
        back = np.multiply.outer(back, t)
    assert abs(kernel.sum() - 1.) <= 1e-14 and np.max(np.abs(back - kernel)) <= 1e-15
    return taps


def blur(v, kernel, adjoint=False):
    """scipy.ndimage.convolve(v, kernel, mode="wrap"); kernel an N-D array, or a list of
    1-D taps, one per axis, applied axis by axis (large volumes).  adjoint: with the
    reversed kernel."""
    from scipy.ndimage import convolve, convolve1d
    if isinstance(kernel, (list, tuple)):
        for a, t in enumerate(kernel):
            v = convolve1d(v, t[::-1] if adjoint else t, axis=a, mode="wrap")
        return v
    if adjoint:
        kernel = kernel[tuple([slice(None, None, -1)] * kernel.ndim)]
    return convolve(v, kernel, mode="wrap")


def kernel_abs_sum(kernel):
    if isinstance(kernel, (list, tuple)):
        return float(np.prod([np.sum(np.abs(t)) for t in kernel]))
    return float(np.sum(np.abs(kernel)))


def _widths(shape, spacing):
    # spacing[0] belongs to the LAST array axis (GradientOperator)
    d = len(shape)
    sp = np.ones(d) if spacing is None else np.atleast_1d(spacing).astype(float)
    return [1. / sp[d - 1 - a] for a in range(d)]          # per array axis


def grad(x, spacing=None):
    """Zero-padded forward differences, (d,) + shape: (x[i + e_a] - x[i]) / h_a with
    x = 0 past the last index."""
    out = np.zeros((x.ndim,) + x.shape)
    for a, w in enumerate(_widths(x.shape, spacing)):
        hi = np.zeros_like(x)
        sl = [slice(None)] * x.ndim
        sl[a] = slice(0, -1)
        sr = list(sl)
        sr[a] = slice(1, None)
        hi[tuple(sl)] = x[tuple(sr)]
        out[a] = hi * w + x * (-w)
    return out


def grad_adj(p, spacing=None):
    """The adjoint of grad: sum_a (p_a[i - e_a] - p_a[i]) / h_a, p = 0 before the first
    index; the axes are added in the tile body's order x, y, z (last axis first)."""
    shape = p.shape[1:]
    ws = _widths(shape, spacing)
    out = None
    for a in reversed(range(len(shape))):
        lo = np.zeros(shape)
        sl = [slice(None)] * len(shape)
        sl[a] = slice(1, None)
        sr = list(sl)
        sr[a] = slice(0, -1)
        lo[tuple(sl)] = p[a][tuple(sr)]
        term = p[a] * (-ws[a]) + lo * ws[a]
        out = term if out is None else out + term
    return out


def dual_data(v, c, sigma, w, data):
    """nsol_amd.vector_numpy.pdl_dual_prox (the restatement of k_pdl_dual_data's prox): l2
    (v c) / (c + sigma), l1 the two selects onto [-c, c]; exactly 0 where w == 0, whatever
    v holds there."""
    return vn.pdl_dual_prox(v, c, sigma, w, data == "ell1")


def default_steps(shape, kernel, spacing=None, tau=None, sigma=None):
    L2 = sum(4. * w * w for w in _widths(shape, spacing)) + kernel_abs_sum(kernel) ** 2
    if tau is None and sigma is None:
        tau = sigma = 1. / np.sqrt(L2)
    elif tau is None:
        tau = 1. / (L2 * sigma)
    elif sigma is None:
        sigma = 1. / (L2 * tau)
    return L2, tau, sigma


def pd_linear_restatement(obs, kernel, shape, reg, data, alpha, iters, weights=None,
                          bounds=None, iso=False, spacing=None, x_scale=1., tau=None,
                          sigma=None, gamma=0.05, x0=None, trace=None, scaled=False):
    """NumPy float64 statement of PrimalDualLinearSolver's iteration with
    A = scipy.ndimage.convolve(., kernel, mode="wrap") and A^T the convolution with the
    reversed kernel (kernel: an N-D array or per-axis taps, see blur).  reg: "TV" | "huber"; data: "ell2" | "ell1".  x0: the start, default
    the observation.  trace: a list that receives (x, p, q) copies after every
    iteration.  Returns x * x_scale with the volume's shape (scaled: x)."""
    shape = tuple(shape)
    d = len(shape)
    if not isinstance(kernel, (list, tuple)):
        kernel = np.asarray(kernel, dtype=np.float64)
    A = lambda v: blur(v, kernel)
    At = lambda v: blur(v, kernel, adjoint=True)
    x_scale = float(x_scale)
    bt = np.asarray(obs, np.float64).reshape(shape) / x_scale
    w = np.ones(shape) if weights is None else \
        np.asarray(weights, np.float64).reshape(shape)
    lo, hi = (-np.inf, np.inf) if bounds is None else bounds
    _, tau, sigma = default_steps(shape, kernel, spacing, tau, sigma)
    lmbda, theta = 1. / float(alpha), 1.
    c = lmbda * w
    start = obs if x0 is None else x0
    x = np.asarray(start, np.float64).reshape(shape) / x_scale
    xbar = x.copy()
    p = np.zeros((d,) + shape)
    q = np.zeros(shape)
    hden = 1. + sigma * gamma if reg == "huber" else None
    for _ in range(iters):
        pq = p + sigma * grad(xbar, spacing)
        if iso:
            p = project_iso(pq.reshape(-1), d, hden).reshape(pq.shape)
        else:
            p = np.clip(pq / hden if hden is not None else pq, -1., 1.)
        with np.errstate(invalid="ignore"):
            v = q + sigma * (A(xbar) - bt)
        q = dual_data(v, c, sigma, w, data)
        xn = np.clip(x - tau * (grad_adj(p, spacing) + At(q)), lo, hi)
        xbar = xn + theta * (xn - x)
        x = xn
        if trace is not None:
            trace.append((x.copy(), p.copy(), q.copy()))
    return x if scaled else x * x_scale


def huber(t, gamma):
    a = np.abs(t)
    return np.where(a <= gamma, t * t / (2. * gamma), a - 0.5 * gamma)


def huber_prime(t, gamma):
    return np.clip(t / gamma, -1., 1.)


def lbfgsb_minimiser(bt, kernel, alpha, w, gamma=0.05, bounds=None):
    """The minimiser of lambda/2 sum w (A x - bt)^2 + sum_a huber_gamma((grad x)_a)
    (anisotropic Huber, scaled variable) over the box, by SciPy's L-BFGS-B."""
    from scipy.ndimage import convolve
    from scipy.optimize import minimize
    shape = bt.shape
    flipped = kernel[tuple([slice(None, None, -1)] * bt.ndim)]
    lmbda = 1. / alpha

    def fg(v):
        x = v.reshape(shape)
        r = convolve(x, kernel, mode="wrap") - bt
        gx = grad(x)
        f = 0.5 * lmbda * np.sum(w * r * r) + np.sum(huber(gx, gamma))
        g = lmbda * convolve(w * r, flipped, mode="wrap") + \
            grad_adj(huber_prime(gx, gamma))
        return f, g.reshape(-1)

    box = None if bounds is None else [bounds] * bt.size
    start = bt.reshape(-1) if bounds is None else np.clip(bt.reshape(-1), *bounds)
    res = minimize(fg, start, jac=True, method="L-BFGS-B", bounds=box,
                   options=dict(maxiter=100000, maxfun=200000, ftol=1e-15, gtol=1e-10,
                                maxcor=30))
    return res.x.reshape(shape)


def convergence_case(mixed):
    """The 24 x 20 case: blocks of 20 / 50 / 80 / 110 under a Gaussian blur of sigma = 1
    (wrap) plus noise of sigma 3, scaled by its maximum; optionally two zero-weight
    rows and a column of weight 2.5.  After 1 000 iterations the restatement is
    1.4e-7 (all weights 1) and 3.0e-6 (mixed) from the L-BFGS-B minimiser, whose own
    floor is 2-4e-8; the zero-weight rows are inpainted by diffusion alone, which is
    what takes the iterations (2 000 reach 2e-8 there as well)."""
    from scipy.ndimage import convolve
    rng = np.random.default_rng(5)
    shape = (24, 20)
    kernel = gaussian_kernel(2, 1.)
    truth = np.full(shape, 20.)
    truth[4:14, 3:11] = 80.
    truth[10:21, 8:17] = 50.
    truth[16:19, 2:6] = 110.
    obs = convolve(truth, kernel, mode="wrap") + 3. * rng.standard_normal(shape)
    w = np.ones(shape)
    if mixed:
        w[:, 4] = 2.5
        w[7] = 0.
        w[15] = 0.
    return obs, kernel, shape, w, float(obs.max())


_MINIMISER = {}


def minimiser_of(mixed, bounds=None):
    key = (mixed, bounds)
    if key not in _MINIMISER:
        obs, kernel, shape, w, s = convergence_case(mixed)
        _MINIMISER[key] = lbfgsb_minimiser(obs / s, kernel, 0.05, w, bounds=bounds) * s
    return _MINIMISER[key]


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


# ------------------------------------------------------- the yardstick's own check
def test_grad_adj_is_the_adjoint_of_grad():
    rng = np.random.default_rng(0)
    for shape, sp in (((11,), None), ((5, 7), (0.7, 1.3)), ((3, 4, 5), (0.7, 1.3, 2.0))):
        x = rng.standard_normal(shape)
        p = rng.standard_normal((len(shape),) + shape)
        assert abs(np.sum(grad(x, sp) * p) - np.sum(x * grad_adj(p, sp))) <= 1e-12


@pytest.mark.parametrize("mixed", [False, True])
def test_restatement_reaches_the_minimiser(mixed):
    obs, kernel, shape, w, s = convergence_case(mixed)
    L2, tau, sigma = default_steps(shape, kernel)
    assert abs(L2 - 9.) <= 1e-12 and abs(tau - 1. / 3.) <= 1e-12
    x = pd_linear_restatement(obs, kernel, shape, "huber", "ell2", 0.05, 1000,
                              weights=w if mixed else None, x_scale=s)
    err = rel(x, minimiser_of(mixed))
    print("mixed weights" if mixed else "all weights 1", "rel. l2 to the minimiser", err)
    assert err <= 1e-5


def test_restatement_reaches_the_minimiser_inside_active_bounds():
    obs, kernel, shape, w, s = convergence_case(True)
    box = (0.3, 0.9)
    x = pd_linear_restatement(obs, kernel, shape, "huber", "ell2", 0.05, 1000, weights=w,
                              bounds=box, x_scale=s, x0=np.clip(obs / s, *box) * s)
    want = minimiser_of(True, box)
    # the box is active
    assert np.sum(want / s <= box[0]) + np.sum(want / s >= box[1]) > 10
    assert np.all(x / s >= box[0]) and np.all(x / s <= box[1])
    err = rel(x, want)
    print("bounds (0.3, 0.9): rel. l2 to the minimiser", err)
    assert err <= 1e-5


def test_zero_weight_hides_what_the_observation_holds():
    obs, kernel, shape, w, s = convergence_case(True)
    junk = obs.copy()
    junk[7] = np.nan
    junk[15, ::2] = np.inf
    zero = obs.copy()
    zero[7] = 0
    zero[15, ::2] = 0
    for data in ("ell2", "ell1"):
        a = pd_linear_restatement(junk, kernel, shape, "TV", data, 0.05, 20, weights=w,
                                  x_scale=s, x0=zero)
        b = pd_linear_restatement(zero, kernel, shape, "TV", data, 0.05, 20, weights=w,
                                  x_scale=s, x0=zero)
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)


# ------------------------------------------------------------------ host logic
def _solver(**kw):
    import nsol_amd
    from nsol_amd.linear_operators import ConvolutionOperator
    shape = kw.pop("shape_", (6, 8))
    A = ConvolutionOperator(len(shape), gaussian_kernel(len(shape), 1.))
    obs = 1. + np.arange(int(np.prod(shape)), dtype=float)
    A1 = lambda x: A(x.reshape(*shape)).flatten()
    args = dict(A=A1, A_adj=A1, b=obs, x0=obs, dimension=len(shape))
    args.update(kw)
    return nsol_amd.PrimalDualLinearSolver(**args)


def test_constructor_defaults_without_a_gpu():
    import nsol_amd
    from nsol_amd.solver import Solver
    s = _solver()
    assert isinstance(s, Solver) and isinstance(s, nsol_amd.PrimalDualLinearSolver)
    assert s.get_execution() == "fused" and s.get_shape() == (6, 8)
    assert abs(s.get_A_norm2() - 1.) <= 1e-12
    assert abs(s.get_L2() - 9.) <= 1e-12
    assert abs(s.get_tau() - 1. / 3.) <= 1e-12 and abs(s.get_sigma() - 1. / 3.) <= 1e-12
    assert s.get_theta() == 1. and s.get_bounds() == (-np.inf, np.inf)
    assert s.get_iterations_done() is None and s.get_stop_reason() is None
    assert s.get_changes().shape == (0, 3)
    assert s.get_alpha() == 0.01 and s.get_iterations() == 10
    # spacing enters L2 as sum 4 / h^2
    s = _solver(spacing=(0.5, 2.0))
    assert abs(s.get_L2() - (16. + 1. + 1.)) <= 1e-12


def test_step_sizes():
    s = _solver(tau=0.1)
    assert s.get_tau() == 0.1 and abs(s.get_sigma() - 1. / (9. * 0.1)) <= 1e-12
    s = _solver(sigma=0.25)
    assert s.get_sigma() == 0.25 and abs(s.get_tau() - 1. / (9. * 0.25)) <= 1e-12
    s = _solver(tau=0.2, sigma=0.5, L2=10.)
    assert (s.get_tau(), s.get_sigma(), s.get_L2()) == (0.2, 0.5, 10.)
    with pytest.raises(ValueError):
        _solver(tau=0.5, sigma=0.5)                 # 0.25 * 9 > 1
    with pytest.raises(ValueError):
        _solver(tau=0.)
    # the product may touch 1 within rounding
    _solver(tau=1. / 3., sigma=1. / 3.)


def test_operator_norm():
    from nsol_amd.linear_operators import LinearOperators3D
    A, _ = LinearOperators3D().get_gaussian_blurring_operators(np.diag([2., 2., 2.]))
    shape = (4, 5, 6)
    obs = np.ones(int(np.prod(shape)))
    A1 = lambda x: A(x.reshape(*shape)).flatten()
    import nsol_amd
    s = nsol_amd.PrimalDualLinearSolver(A1, A1, obs, obs, 3)
    assert abs(s.get_A_norm2() - 1.) <= 1e-12 and abs(s.get_L2() - 13.) <= 1e-12
    # Young's bound with taps of both signs
    s = _solver(A=lambda x: _signed(x), A_adj=lambda x: _signed(x))
    assert abs(s.get_A_norm2() - 4.) <= 1e-12
    foreign = lambda x: np.asarray(x) * 0.5
    with pytest.raises(ValueError, match="A_norm2"):
        _solver(A=foreign, A_adj=foreign, shape=(6, 8))
    s = _solver(A=foreign, A_adj=foreign, shape=(6, 8), A_norm2=0.25)
    assert s.get_execution() is None and abs(s.get_L2() - 8.25) <= 1e-12
    # a foreign A needs the volume's shape from somewhere
    with pytest.raises(ValueError, match="shape"):
        _solver(A=foreign, A_adj=foreign, A_norm2=0.25)
    s = _solver(A=foreign, A_adj=foreign, A_norm2=0.25, b=np.ones((6, 8)))
    assert s.get_shape() == (6, 8)


def _signed(x):
    from nsol_amd.linear_operators import ConvolutionOperator
    op = ConvolutionOperator(2, np.array([[0., -0.5, 0.], [-0.5, 0., 0.5], [0., 0.5, 0.]]))
    return op(x.reshape(6, 8)).flatten()


@pytest.mark.parametrize("kw", [
    dict(weights=-np.ones(48)), dict(weights=np.ones(47)),
    dict(weights=np.full(48, np.nan)), dict(weights=np.ones(48, dtype=complex)),
    dict(bounds=(1., 0.)), dict(bounds=(np.nan, 1.)), dict(bounds=3.), dict(bounds=(1,)),
    dict(reg_type="TK1"), dict(reg_type="Huber"), dict(data_loss="linear"),
    dict(data_loss="huber"), dict(tolerance=-1.), dict(check_every=0),
    dict(dimension=3), dict(spacing=(1., 1., 1.)), dict(alpha=0.)])
def test_bad_arguments_raise(kw):
    with pytest.raises(ValueError):
        _solver(**kw)


def test_good_arguments_are_taken():
    _solver(weights=np.ones(48, dtype=bool))
    _solver(weights=np.arange(48, dtype=np.int32))
    _solver(weights=np.ones((6, 8), dtype=np.float32))
    assert _solver(bounds=(0., np.inf)).get_bounds() == (0., np.inf)
    assert _solver(bounds=(0.5, 0.5)).get_bounds() == (0.5, 0.5)
    _solver(reg_type="huber", data_loss="ell1", isotropic=True, tolerance=0., check_every=3)


def test_the_new_symbols_are_declared():
    from nsol_amd import _lib, build
    sym = _lib.declared_symbols()
    for name in ("nsol_pdl_dual_data_f32", "nsol_pdl_dual_data_f64", "nsol_pdl_iter_f32",
                 "nsol_pdl_iter_f64", "nsol_pdl_launches"):
        assert name in sym, name
    assert len(sym["nsol_pdl_dual_data_f32"][1]) == 9
    assert len(sym["nsol_pdl_iter_f64"][1]) == 22
    assert sym["nsol_pdl_launches"][1] == []
    assert "nsol_pdl.hip" in build.SOURCES


# ------------------------------------------------------------------ command line
def _cli(argv):
    from nsol_amd.application import run_deconvolution
    return run_deconvolution.main(["--observation", "o.nii.gz", "--result", "r.nii.gz"] +
                                  argv)


def test_cli_pdl_takes_a_mask(monkeypatch):
    """--solver PDL --mask passes the argument checks: the run gets as far as reading
    the observation."""
    from nsol_amd import data_reader

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(data_reader, "DataReader", stop)
    for extra in (["--mask", "m.nii.gz"], ["--weights", "w.nii.gz"],
                  ["--mask", "m.nii.gz", "--data-loss", "ell1", "--nonnegative",
                   "--isotropic", "--tolerance", "1e-3", "--check-every", "5",
                   "--reconstruction-type", "HuberL2"]):
        with pytest.raises(Reached):
            _cli(["--solver", "PDL"] + extra)


@pytest.mark.parametrize("argv", [
    ["--solver", "PDL", "--mask", "m.nii.gz", "--weights", "w.nii.gz"],
    ["--solver", "PDL", "--data-loss", "cauchy"],
    ["--solver", "PDL", "--reconstruction-type", "TK1L2"],
    ["--solver", "ADMM", "--nonnegative"],
    ["--solver", "ADMM", "--tolerance", "1e-3"]])
def test_cli_refusals_exit_with_status_2(capsys, argv):
    with pytest.raises(SystemExit) as e:
        _cli(argv)
    assert e.value.code == 2
    assert capsys.readouterr().err


def test_cli_build_solver_wires_pdl():
    from nsol_amd.application import run_deconvolution
    import nsol_amd
    obs = 10. + np.arange(6 * 8, dtype=float).reshape(6, 8)
    w = np.ones((6, 8))
    w[-1] = 0
    junk = obs.copy()
    junk[-1] = np.nan
    s = run_deconvolution.build_solver(junk, np.ones(2), 1.0, "HuberL2", "PDL", 0.02, 7,
                                       dtype=np.float64, isotropic=True, weights=w,
                                       pdl_data_loss="ell1", nonnegative=True,
                                       tolerance=1e-3, check_every=4)
    assert isinstance(s, nsol_amd.PrimalDualLinearSolver)
    assert s.get_execution() == "fused" and s.get_shape() == (6, 8)
    assert s.get_reg_type() == "huber" and s.get_data_loss() == "ell1"
    assert s.get_isotropic() and s.get_bounds() == (0., np.inf)
    assert s.get_x_scale() == obs[:-1].max()         # over the voxels that count
    assert np.all(np.isfinite(s.get_x0()))
    assert s.get_tolerance() == 1e-3 and s.get_check_every() == 4
    assert s.get_alpha() == 0.02 and s.get_iterations() == 7
