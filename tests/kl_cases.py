"""What tests/test_kl_host.py and tests/test_kl_gpu.py share for the Poisson (Kullback-
Leibler) data term: the stress vector of the two closed-form proxes, their one-line forms
(which the vector must tell apart from the branched ones), the NumPy float64 restatement
of PrimalDualLinearSolver's iteration with data_loss="kl", and the convergence case with
its L-BFGS-B minimiser."""
import numpy as np

from nsol_amd import vector_numpy as vn
from test_pd_isotropic_host import project_iso
from test_pd_linear_host import (blur, default_steps, gaussian_kernel, grad, grad_adj,
                                 huber, huber_prime)

STRESS_N = 200000


def stress_vector(n=STRESS_N, seed=20):
    """dict of float32 arrays c, sigma, bt, v, u: c in 1e-3 .. 1e3, sigma in 1e-2 .. 1e1,
    bt in 1e-4 .. 1e4 with a tenth exactly 0, v and u = +-c * (1e-3 .. 1e6), log-uniform,
    all rounded to float32 first."""
    rng = np.random.default_rng(seed)

    def logu(lo, hi):
        return 10. ** rng.uniform(np.log10(lo), np.log10(hi), n)

    c, sigma, bt = logu(1e-3, 1e3), logu(1e-2, 1e1), logu(1e-4, 1e4)
    bt[rng.permutation(n)[:n // 10]] = 0.
    v = c * logu(1e-3, 1e6) * rng.choice([-1., 1.], n)
    u = c * logu(1e-3, 1e6) * rng.choice([-1., 1.], n)
    return {k: a.astype(np.float32) for k, a in
            dict(c=c, sigma=sigma, bt=bt, v=v, u=u).items()}


def dual_one_line(v, c, sigma, bt):
    """0.5 (c + v - sqrt((v - c)^2 + 4 sigma c bt)) in the arrays' precision."""
    d = v - c
    return 0.5 * (c + v - np.sqrt(d * d + 4. * sigma * c * bt))


def primal_one_line(u, bt, t):
    """0.5 (u - t + sqrt((u - t)^2 + 4 t bt)) in the arrays' precision."""
    e = u - t
    return 0.5 * (e + np.sqrt(e * e + 4. * t * bt))


def dual_scaled_error(got, ref, c):
    """max |got - ref| / max(|ref|, c): q crosses zero at v = sigma bt, so a purely
    relative gate is not meaningful for the dual prox."""
    got, ref, c = (np.asarray(a, np.float64) for a in (got, ref, c))
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), c)))


def relative_error(got, ref):
    """max |got - ref| / |ref| over ref != 0; where ref == 0, got must be 0 too."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    zero = ref == 0
    assert np.all(got[zero] == 0)
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero]))) \
        if np.any(~zero) else 0.


def pd_linear_kl_restatement(obs, kernel, shape, reg, alpha, iters, weights=None,
                             bounds=None, iso=False, x_scale=1., background=0.,
                             gamma=0.05, x0=None, trace=None, scaled=False, A=None,
                             At=None, A_norm2=None, tolerance=None, check_every=10):
    """NumPy float64 statement of PrimalDualLinearSolver's iteration with data_loss="kl":
    test_pd_linear_host.pd_linear_restatement with q <- vn.kl_dual_prox(q + sigma (A xbar
    + g), c, sigma, bt), g = background / x_scale.  A, At: callables on arrays (x of
    `shape` to the observation's shape and back) in the blur's place, with A_norm2 their
    bound.  tolerance: the solver's stopping rule, checked every check_every iterations
    and at the last.  Returns x * x_scale (scaled: x); with a tolerance (x, iterations
    done)."""
    shape = tuple(shape)
    d = len(shape)
    if A is None:
        kernel = np.asarray(kernel, dtype=np.float64)
        A = lambda v: blur(v, kernel)
        At = lambda v: blur(v, kernel, adjoint=True)
        _, tau, sigma = default_steps(shape, kernel)
    else:
        tau = sigma = 1. / np.sqrt(4. * d + A_norm2)
    x_scale = float(x_scale)
    bt = np.asarray(obs, np.float64) / x_scale
    g = float(background) / x_scale
    w = np.ones(bt.shape) if weights is None else \
        np.asarray(weights, np.float64).reshape(bt.shape)
    lo, hi = (-np.inf, np.inf) if bounds is None else bounds
    c = (1. / float(alpha)) * w
    x = np.asarray(obs if x0 is None else x0, np.float64).reshape(shape) / x_scale
    xbar = x.copy()
    p = np.zeros((d,) + shape)
    q = np.zeros(bt.shape)
    hden = 1. + sigma * gamma if reg == "huber" else None
    done = iters
    for i in range(iters):
        pq = p + sigma * grad(xbar)
        if iso:
            pn = project_iso(pq.reshape(-1), d, hden).reshape(pq.shape)
        else:
            pn = np.clip(pq / hden if hden is not None else pq, -1., 1.)
        qn = vn.kl_dual_prox(q + sigma * (A(xbar) + g), c, sigma, bt, w)
        xn = np.clip(x - tau * (grad_adj(pn) + At(qn)), lo, hi)
        xbar = xn + (xn - x)
        if tolerance is not None and ((i + 1) % check_every == 0 or i + 1 == iters):
            r_x = np.sqrt(np.sum((xn - x) ** 2) / np.sum(xn ** 2))
            r_d = np.sqrt((np.sum((pn - p) ** 2) + np.sum((qn - q) ** 2)) /
                          (np.sum(pn ** 2) + np.sum(qn ** 2)))
            if max(r_x, r_d) <= tolerance:
                x, p, q, done = xn, pn, qn, i + 1
                break
        x, p, q = xn, pn, qn
        if trace is not None:
            trace.append((x.copy(), p.copy(), q.copy()))
    out = x if scaled else x * x_scale
    return (out, done) if tolerance is not None else out


def kl_lbfgsb_minimiser(bt, kernel, alpha, w, g, gamma=0.05):
    """The minimiser over x >= 0 of lambda sum w ((A x + g) - bt log(A x + g)) + sum_a
    huber_gamma((grad x)_a) (anisotropic Huber, scaled variable) by SciPy's L-BFGS-B with
    the options of test_pd_linear_host.lbfgsb_minimiser; weight 0 hides bt."""
    from scipy.ndimage import convolve
    from scipy.optimize import minimize
    shape = bt.shape
    flipped = kernel[tuple([slice(None, None, -1)] * bt.ndim)]
    lmbda = 1. / alpha
    on = w > 0
    b0 = np.where(on, bt, 0.)

    def fg(v):
        x = v.reshape(shape)
        u = convolve(x, kernel, mode="wrap") + g
        gx = grad(x)
        f = lmbda * np.sum(w * (u - b0 * np.log(u))) + np.sum(huber(gx, gamma))
        gr = lmbda * convolve(w * (1. - b0 / u), flipped, mode="wrap") + \
            grad_adj(huber_prime(gx, gamma))
        return f, gr.reshape(-1)

    start = np.clip(np.where(on, bt, np.mean(bt[on])).reshape(-1), 0., None)
    res = minimize(fg, start, jac=True, method="L-BFGS-B", bounds=[(0., np.inf)] * bt.size,
                   options=dict(maxiter=100000, maxfun=200000, ftol=1e-15, gtol=1e-10,
                                maxcor=30))
    return res.x.reshape(shape)


KL_BACKGROUND = 2.


def kl_convergence_case(mixed):
    """test_pd_linear_host.convergence_case's 24 x 20 block image with Poisson noise:
    rng.poisson(A truth + 2), background 2; mixed: rows 7-8 of weight 0 over NaN and
    column 15 of weight 2.5 outside those rows.  (obs, kernel, shape, w, scale): the scale
    is the maximum of the counts that count."""
    from scipy.ndimage import convolve
    rng = np.random.default_rng(5)
    shape = (24, 20)
    kernel = gaussian_kernel(2, 1.)
    truth = np.full(shape, 20.)
    truth[4:14, 3:11] = 80.
    truth[10:21, 8:17] = 50.
    truth[16:19, 2:6] = 110.
    obs = rng.poisson(convolve(truth, kernel, mode="wrap") + KL_BACKGROUND).astype(float)
    w = np.ones(shape)
    s = float(obs.max())
    if mixed:
        w[:, 15] = 2.5
        w[7:9] = 0.
        obs[7:9] = np.nan
    return obs, kernel, shape, w, s


_MINIMISER = {}


def kl_minimiser_of(mixed):
    """The L-BFGS-B minimiser of the convergence case in the observation's units,
    computed once."""
    if mixed not in _MINIMISER:
        obs, kernel, shape, w, s = kl_convergence_case(mixed)
        _MINIMISER[mixed] = kl_lbfgsb_minimiser(obs / s, kernel, 0.05, w,
                                                KL_BACKGROUND / s) * s
    return _MINIMISER[mixed]
