"""NumPy restatement of the second-order TGV iteration of TGVPrimalDualSolver
(nsol_amd/tgv_solver.py, csrc/nsol_tgv.hip): the written specification of its
arithmetic and the reference of its tests.  float64 or float32, 1-D to 3-D, any spacing.

In the solver's scaled units (b = observation / x_scale, lmbda = 1 / alpha):

    min over x (an array of `shape`) and w (d arrays of `shape`)
        lmbda D(x, b) + |grad x - w|_1 + beta |E w|_1

    (grad x)_a = D_a x         D_a: forward difference along component a, weight 1/h_a,
    (E w)_aa   = D_a w_a            zero-padded past the last index (the library's one
    (E w)_ab   = (D_a w_b + D_b w_a) / 2,  a < b            boundary convention)

Component a = 0 is the x axis, the LAST array axis; spacing[a] belongs to it.  E w is
symmetric and stored as M = d (d + 1) / 2 components, diagonals first: xx, yy, zz, xy,
xz, yz in 3-D, xx, yy, xy in 2-D, xx in 1-D.  Off-diagonal components count twice in
every norm and inner product.  D is 1/2 |.|^2 ("ell2"), |.|_1 ("ell1") or the Poisson
(Kullback-Leibler) term sum (x - b log x) ("kl": b >= 0, and behind a linear operator
sum ((A x + background) - b log(A x + background))).

Arrays: x `shape`, w and p (d,) + shape, q (M,) + shape.
"""
import numpy as np

from . import vector_numpy

DATA_LOSSES = ("ell2", "ell1", "kl")


def pairs(d):
    """The off-diagonal components (a, b), a < b, in stored order (after the d
    diagonals)."""
    return [(a, b) for a in range(d) for b in range(a + 1, d)]


def components(d):
    """M = d (d + 1) / 2."""
    return d * (d + 1) // 2


def inner_weights(d):
    """The weight of every stored component of q in norms and inner products."""
    return np.array([1.] * d + [2.] * len(pairs(d)))


def _inv(spacing, d, dtype):
    sp = np.ones(d) if spacing is None else np.atleast_1d(spacing).astype(float)
    if sp.size != d:
        raise ValueError("spacing must hold %d values" % d)
    return [dtype(1. / s) for s in sp]


def D(u, a, wgt):
    """Forward difference along component a (array axis u.ndim - 1 - a), hi * w +
    u * (-w) with hi = 0 past the last index."""
    ax = u.ndim - 1 - a
    hi = np.zeros_like(u)
    src = [slice(None)] * u.ndim
    dst = [slice(None)] * u.ndim
    src[ax], dst[ax] = slice(1, None), slice(0, -1)
    hi[tuple(dst)] = u[tuple(src)]
    return hi * wgt + u * (-wgt)


def D_adj(u, a, wgt):
    """The exact transpose of D: u * (-w) + lo * w with lo = 0 before the first index."""
    ax = u.ndim - 1 - a
    lo = np.zeros_like(u)
    src = [slice(None)] * u.ndim
    dst = [slice(None)] * u.ndim
    src[ax], dst[ax] = slice(0, -1), slice(1, None)
    lo[tuple(dst)] = u[tuple(src)]
    return u * (-wgt) + lo * wgt


def K(x, w, spacing=None):
    """(grad x - w, E w): arrays of shape (d,) + x.shape and (M,) + x.shape."""
    d = x.ndim
    dt = x.dtype.type
    iw = _inv(spacing, d, dt)
    g = np.stack([D(x, a, iw[a]) - w[a] for a in range(d)])
    e = [D(w[a], a, iw[a]) for a in range(d)]
    e += [dt(0.5) * (D(w[b], a, iw[a]) + D(w[a], b, iw[b])) for a, b in pairs(d)]
    return g, np.stack(e)


def K_adj(p, q, spacing=None):
    """The transpose of K in the inner product that counts q's off-diagonals twice:
    (sum_a D_a^T p_a,  [-p_a + D_a^T q_aa + sum_{b != a} D_b^T q_ab]_a)."""
    d = p.shape[0]
    iw = _inv(spacing, d, p.dtype.type)
    off = {ab: d + m for m, ab in enumerate(pairs(d))}
    kx = D_adj(p[0], 0, iw[0])
    for a in range(1, d):
        kx = kx + D_adj(p[a], a, iw[a])
    kw = []
    for a in range(d):
        v = -p[a] + D_adj(q[a], a, iw[a])
        for b in range(d):
            if b != a:
                v = v + D_adj(q[off[(min(a, b), max(a, b))]], b, iw[b])
        kw.append(v)
    return kx, np.stack(kw)


def inner_dual(p1, q1, p2, q2):
    """<(p1, q1), (p2, q2)> with the off-diagonals of q doubled."""
    d = p1.shape[0]
    wq = inner_weights(d).reshape((-1,) + (1,) * (q1.ndim - 1))
    return float(np.sum(p1 * p2) + np.sum(wq * q1 * q2))


def norm_bound(dimension, spacing=None):
    """An upper bound of |K|^2: (2 g + 1 + sqrt(4 g + 1)) / 2 with g = 4 sum 1/h_a^2, the
    largest eigenvalue of [[g, sqrt g], [sqrt g, 1 + g]] (|E| <= |grad| <= sqrt g)."""
    sp = np.ones(dimension) if spacing is None else np.atleast_1d(spacing).astype(float)
    g = 4. * float(np.sum(1. / sp ** 2))
    return (2. * g + 1. + np.sqrt(4. * g + 1.)) / 2.


def energy(x, w, b, lmbda, beta, spacing=None, data_loss="ell2", isotropic=False):
    """lmbda D(x, b) + |grad x - w|_1 + beta |E w|_1 (float64)."""
    x, w, b = (np.asarray(t, dtype=np.float64) for t in (x, w, b))
    d = x.ndim
    g, e = K(x, w, spacing)
    wq = inner_weights(d).reshape((-1,) + (1,) * d)
    if isotropic:
        r1 = np.sum(np.sqrt(np.sum(g * g, axis=0)))
        r2 = np.sum(np.sqrt(np.sum(wq * e * e, axis=0)))
    else:
        r1 = np.sum(np.abs(g))
        r2 = np.sum(wq * np.abs(e))
    if data_loss == "kl":
        data = _kl(x, b, np.ones_like(x))
    else:
        r = x - b
        data = np.sum(np.abs(r)) if data_loss == "ell1" else 0.5 * np.sum(r * r)
    return float(lmbda * data + r1 + beta * r2)


def _kl(u, b, wt):
    """sum wt (u - b log u) over the samples of positive weight, 0 log 0 = 0 (float64)."""
    on = wt > 0
    u, b, wt = u[on], b[on], wt[on]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sum(wt * (u - np.where(b > 0, b * np.log(u), 0.))))


def project_p(p, isotropic):
    """P_1: the clamp to [-1, 1] per component, or p / max(1, |p|_2) per voxel."""
    one = p.dtype.type(1)
    if not isotropic:
        return np.minimum(np.maximum(p, -one), one)
    s = p[0] * p[0]
    for a in range(1, p.shape[0]):
        s = s + p[a] * p[a]
    return p / np.maximum(one, np.sqrt(s))


def project_q(q, beta, d, isotropic):
    """P_beta: the clamp to [-beta, beta] per component, or q / max(1, |q|_F / beta)
    per voxel with the off-diagonals doubled inside the Frobenius norm."""
    dt = q.dtype.type
    beta = dt(beta)
    if not isotropic:
        return np.minimum(np.maximum(q, -beta), beta)
    s = q[0] * q[0]
    for m in range(1, d):
        s = s + q[m] * q[m]
    for m in range(d, q.shape[0]):
        s = s + dt(2) * (q[m] * q[m])
    return q / np.maximum(dt(1), np.sqrt(s) / beta)


def prox_data(u, b, tl, data_loss):
    """prox of tl D(., b): (u + tl b) / (1 + tl), or b + max(|u - b| - tl, 0) sign."""
    dt = u.dtype.type
    tl = dt(tl)
    if data_loss == "kl":      # vector_numpy.prox_kl, all weights 1
        return vector_numpy.prox_kl_w(u, b, None, tl, u.dtype).astype(dt)
    if data_loss == "ell1":
        r = u - b
        return b + np.maximum(np.abs(r) - tl, dt(0)) * np.sign(r)
    return (u + tl * b) / (dt(1) + tl)


def dual_step(xbar, wbar, p, q, sigma, beta, spacing=None, isotropic=False):
    """(p, q) after the dual half of one iteration."""
    d = xbar.ndim
    sigma = xbar.dtype.type(sigma)
    g, e = K(xbar, wbar, spacing)
    return (project_p(p + sigma * g, isotropic),
            project_q(q + sigma * e, beta, d, isotropic))


def primal_step(p, q, x, w, b, tau, tl, theta=1., spacing=None, data_loss="ell2"):
    """(x+, xbar, w+, wbar) after the primal half of one iteration."""
    dt = x.dtype.type
    tau, theta = dt(tau), dt(theta)
    kx, kw = K_adj(p, q, spacing)
    xn = prox_data(x - tau * kx, b, tl, data_loss)
    wn = w - tau * kw
    return xn, xn + theta * (xn - x), wn, wn + theta * (wn - w)


def primal_step_weighted(p, q, x, w, b, wt, tau, tl, theta=1., spacing=None,
                         data_loss="ell2"):
    """primal_step with per-voxel weights wt >= 0 on the data term (k_tgv_primal's WGT
    form): the data prox is vector_numpy.prox_data_w, which keeps u where wt == 0,
    whatever b holds there."""
    dt = x.dtype.type
    tau, theta = dt(tau), dt(theta)
    kx, kw = K_adj(p, q, spacing)
    if data_loss == "kl":
        xn = vector_numpy.prox_kl_w(x - tau * kx, b, wt, tl, x.dtype).astype(dt)
    else:
        xn = vector_numpy.prox_data_w(x - tau * kx, b, wt, tl, data_loss == "ell1",
                                      x.dtype).astype(dt)
    wn = w - tau * kw
    return xn, xn + theta * (xn - x), wn, wn + theta * (wn - w)


def primal_step_lin(p, q, x, w, g, tau, theta=1., lo=-np.inf, hi=np.inf, spacing=None,
                    dtype=None):
    """The primal half behind a linear operator (k_tgv_primal's LIN form): g = A^T r and
    x+ = vector_numpy.pd_lin_step(x, sum_a D_a^T p_a, g): the explicit step, clipped to
    box_in(lo, hi) as the kernel of element type `dtype` (default: x's) sees the box."""
    dt = x.dtype.type
    kx, kw = K_adj(p, q, spacing)
    xn = vector_numpy.pd_lin_step(x, kx, g, tau, lo, hi, dtype or x.dtype).astype(dt)
    tau, theta = dt(tau), dt(theta)
    wn = w - tau * kw
    return xn, xn + theta * (xn - x), wn, wn + theta * (wn - w)


def norm_bound_linear(dimension, spacing=None, A_norm2=0.):
    """An upper bound of |K|^2 for K(x, w) = (grad x - w, E w, A x) with |A|^2 <= a =
    A_norm2: |K(x, w)|^2 <= (g + a) |x|^2 + 2 sqrt(g) |x| |w| + (1 + g) |w|^2, so the
    largest eigenvalue of [[g + a, sqrt g], [sqrt g, 1 + g]],
    ((2 g + a + 1) + sqrt((a - 1)^2 + 4 g)) / 2 with g = 4 sum 1/h_a^2.  a = 0 is
    norm_bound, bit for bit."""
    sp = np.ones(dimension) if spacing is None else np.atleast_1d(spacing).astype(float)
    g = 4. * float(np.sum(1. / sp ** 2))
    a = float(A_norm2)
    return ((2. * g + a + 1.) + np.sqrt((a - 1.) ** 2 + 4. * g)) / 2.


def energy_linear(x, w, Ax, b, lmbda, beta, spacing=None, data_loss="ell2",
                  isotropic=False, weights=None, background=0.):
    """lmbda D_wt(A x, b) + |grad x - w|_1 + beta |E w|_1 (float64); Ax is A applied to x.
    Samples of weight 0 do not enter, whatever b holds there.  background: the constant
    of the "kl" term.  (The box is a constraint: it is not part of the value.)"""
    x, w = (np.asarray(t, dtype=np.float64) for t in (x, w))
    reg = energy(x, w, x, 1., beta, spacing, "ell2", isotropic)    # x - x: no data term
    r = np.asarray(Ax, dtype=np.float64).ravel() - np.asarray(b, dtype=np.float64).ravel()
    wt = np.ones_like(r) if weights is None else \
        np.asarray(weights, dtype=np.float64).ravel()
    if data_loss == "kl":
        u = np.asarray(Ax, dtype=np.float64).ravel() + float(background)
        return float(lmbda * _kl(u, np.asarray(b, dtype=np.float64).ravel(), wt) + reg)
    r = np.where(wt == 0, 0., r)
    data = np.sum(wt * np.abs(r)) if data_loss == "ell1" else 0.5 * np.sum(wt * r * r)
    return float(lmbda * data + reg)


def _ratio(num, den):
    if num == 0.:
        return 0.
    if den == 0.:
        return float("inf")
    return float(np.sqrt(num / den))


def _sq(*arrs):
    return float(sum(np.sum(np.asarray(t, dtype=np.float64) ** 2) for t in arrs))


def iterate_linear(A, A_adj, b, x0, iterations, alpha, beta=2., spacing=None,
                   data_loss="ell2", isotropic=False, tau=None, sigma=None, theta=1.,
                   L2=None, dtype=None, keep=False, weights=None, bounds=None,
                   A_norm2=None, background=0.):
    """`iterations` iterations of the TGV iteration whose data term sits behind a linear
    operator, lmbda D_wt(A x, b) + |grad x - w|_1 + beta |E w|_1 + indicator_[lo, hi](x),
    from x = xbar = x0, w = wbar = p = q = r = 0.  A and A_adj are callables on arrays: A
    takes an array of x0's shape and returns the m values of b (any shape), A_adj the
    reverse.  weights: m values >= 0 or None (all 1); bounds: (lo, hi) or None; A_norm2:
    an upper bound of |A|^2, required unless L2 is given.  One iteration:

        (p, q) <- dual_step(xbar, wbar, p, q)
        r      <- vector_numpy.pdl_dual_data(r, A xbar, b, weights, sigma, lmbda, l1)
                  ("kl": pdl_dual_data_kl with the constant `background` >= 0)
        (x, xbar, w, wbar) <- primal_step_lin(p, q, x, w, A_adj r, tau, theta, lo, hi)

    Returns what iterate returns plus r; the primal ratio runs over (x, w), the dual one
    over (p, q, r)."""
    if data_loss not in DATA_LOSSES:
        raise ValueError("data_loss must be one of %r" % (DATA_LOSSES,))
    dt = np.dtype(dtype or np.asarray(b).dtype).type
    b = np.asarray(b, dtype=dt)
    x = np.array(x0, dtype=dt)
    d = x.ndim
    if L2 is None:
        if A_norm2 is None:
            raise ValueError("A_norm2 (an upper bound of |A|^2) or L2 is required")
        L2 = norm_bound_linear(d, spacing, A_norm2)
    if tau is None and sigma is None:
        tau = sigma = 1. / np.sqrt(L2)
    elif tau is None:
        tau = 1. / (L2 * sigma)
    elif sigma is None:
        sigma = 1. / (L2 * tau)
    lmbda = 1. / alpha
    lo, hi = (-np.inf, np.inf) if bounds is None else (float(bounds[0]), float(bounds[1]))
    wt = None if weights is None else np.asarray(weights, dtype=dt).reshape(b.shape)
    w = np.zeros((d,) + x.shape, dtype=dt)
    p = np.zeros((d,) + x.shape, dtype=dt)
    q = np.zeros((components(d),) + x.shape, dtype=dt)
    r = np.zeros(b.shape, dtype=dt)
    xbar, wbar = x.copy(), w.copy()
    ratios, iterates = [], [x.copy()]
    for k in range(1, int(iterations) + 1):
        pn, qn = dual_step(xbar, wbar, p, q, sigma, beta, spacing, isotropic)
        t = np.asarray(A(xbar), dtype=dt).reshape(b.shape)
        if data_loss == "kl":
            rn = vector_numpy.pdl_dual_data_kl(r, t, b, wt, sigma, lmbda, background,
                                               dt).astype(dt)
        else:
            rn = vector_numpy.pdl_dual_data(r, t, b, wt, sigma, lmbda,
                                            data_loss == "ell1", dt).astype(dt)
        g = np.asarray(A_adj(rn), dtype=dt).reshape(x.shape)
        xn, xbar, wn, wbar = primal_step_lin(pn, qn, x, w, g, tau, theta, lo, hi, spacing,
                                             dt)
        ratios.append((float(k),
                       _ratio(_sq(xn - x, wn - w), _sq(xn, wn)),
                       _ratio(_sq(pn - p, qn - q, rn - r), _sq(pn, qn, rn))))
        x, w, p, q, r = xn, wn, pn, qn, rn
        if keep:
            iterates.append(x.copy())
    out = dict(x=x, w=w, p=p, q=q, r=r, tau=float(tau), sigma=float(sigma),
               ratios=np.array(ratios, dtype=np.float64).reshape(-1, 3))
    if keep:
        out["iterates"] = iterates
    return out


def iterate(b, x0, iterations, alpha, beta=2., spacing=None, data_loss="ell2",
            isotropic=False, tau=None, sigma=None, theta=1., L2=None, dtype=None,
            keep=False, weights=None):
    """`iterations` iterations from x = xbar = x0, w = wbar = p = q = 0 on arrays in the
    scaled units (b and x0 of the volume's shape).  Returns a dict: x, w, p, q (the last
    iterate), ratios (one row (k, r_primal, r_dual) per iteration: the stopping rule's
    r = sqrt(sum (v_k - v_{k-1})^2 / sum v_k^2) over (x, w) and over (p, q)), tau, sigma,
    and with keep the list `iterates` of every x, the start included.  weights: per-voxel
    weights >= 0 of the data term (primal_step_weighted) or None, the unweighted step."""
    if data_loss not in DATA_LOSSES:
        raise ValueError("data_loss must be one of %r" % (DATA_LOSSES,))
    dt = np.dtype(dtype or np.asarray(b).dtype).type
    b = np.asarray(b, dtype=dt)
    x = np.array(x0, dtype=dt).reshape(b.shape)
    wt = None if weights is None else np.asarray(weights, dtype=dt).reshape(b.shape)
    d = b.ndim
    if L2 is None:
        L2 = norm_bound(d, spacing)
    if tau is None and sigma is None:
        tau = sigma = 1. / np.sqrt(L2)
    elif tau is None:
        tau = 1. / (L2 * sigma)
    elif sigma is None:
        sigma = 1. / (L2 * tau)
    lmbda = 1. / alpha
    w = np.zeros((d,) + b.shape, dtype=dt)
    p = np.zeros((d,) + b.shape, dtype=dt)
    q = np.zeros((components(d),) + b.shape, dtype=dt)
    xbar, wbar = x.copy(), w.copy()
    ratios, iterates = [], [x.copy()]

    sq = _sq
    for k in range(1, int(iterations) + 1):
        pn, qn = dual_step(xbar, wbar, p, q, sigma, beta, spacing, isotropic)
        if wt is None:
            xn, xbar, wn, wbar = primal_step(pn, qn, x, w, b, tau, tau * lmbda, theta,
                                             spacing, data_loss)
        else:
            xn, xbar, wn, wbar = primal_step_weighted(pn, qn, x, w, b, wt, tau,
                                                      tau * lmbda, theta, spacing,
                                                      data_loss)
        ratios.append((float(k),
                       _ratio(sq(xn - x, wn - w), sq(xn, wn)),
                       _ratio(sq(pn - p, qn - q), sq(pn, qn))))
        x, w, p, q = xn, wn, pn, qn
        if keep:
            iterates.append(x.copy())
    out = dict(x=x, w=w, p=p, q=q, tau=float(tau), sigma=float(sigma),
               ratios=np.array(ratios, dtype=np.float64).reshape(-1, 3))
    if keep:
        out["iterates"] = iterates
    return out


def tv_iterate(b, x0, iterations, alpha, spacing=None, data_loss="ell2"):
    """The anisotropic TV iteration with theta = 1 and constant steps 1/sqrt(g), the
    first-order model TGV is compared with; returns x."""
    dt = np.asarray(b).dtype.type
    b = np.asarray(b)
    x = np.array(x0, dtype=dt).reshape(b.shape)
    d = b.ndim
    iw = _inv(spacing, d, dt)
    sp = np.ones(d) if spacing is None else np.atleast_1d(spacing).astype(float)
    tau = sigma = dt(1. / np.sqrt(4. * np.sum(1. / sp ** 2)))
    p = np.zeros((d,) + b.shape, dtype=dt)
    xbar = x.copy()
    for _ in range(int(iterations)):
        g = np.stack([D(xbar, a, iw[a]) for a in range(d)])
        p = project_p(p + sigma * g, False)
        kx = D_adj(p[0], 0, iw[0])
        for a in range(1, d):
            kx = kx + D_adj(p[a], a, iw[a])
        xn = prox_data(x - tau * kx, b, tau / alpha, data_loss)
        xbar = xn + (xn - x)
        x = xn
    return x
