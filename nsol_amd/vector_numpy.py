"""NumPy restatement of the generic vector kernels of csrc/nsol_ops.hip (reached through
nsol_amd/ops.py): the written specification of their arithmetic and the reference of
tests/test_vector_ops_host.py and tests/test_vector_ops_gpu.py.

Every function works in float64 and performs the kernel's operations in the kernel's
order, so that a float64 kernel (built without FMA contraction) yields the same bits.
`dtype` names the kernel's element type where the kernel rounds a scalar to it or uses
a reciprocal formed on the host: with dtype=np.float32 the scalars are the float32
values the kernel sees, held in float64, and the arithmetic stays float64 -- the
reference a float32 kernel is measured against, on float32-rounded inputs.

Sums are math.fsum of the terms the kernel adds (the kernels accumulate in double);
the `*_terms` functions hand out the terms themselves so that a test can bound the
summation error by their magnitudes.

The last section restates one Chambolle-Pock iteration of csrc/nsol_pd.hip and
csrc/nsol_pdi.hip (k_dual_step, k_primal_step, k_pd_fused and their isotropic twins) from
the functions above: the reference of tests/test_pd_steps_host.py and
tests/test_pd_steps_gpu.py; then the same iteration with the tile bodies' WGT switch (the
weighted data prox of csrc/nsol_pd_weighted.hpp: k_pd_w, k_prox_w) and LIN switch (the
explicit step into a box: k_pd_lin, k_pdl_stack) and the element-wise update of the linear
data term's dual variable (k_pdl_dual_data): the reference of
tests/test_pd_weighted_linear_host.py and tests/test_pd_weighted_linear_gpu.py.

Stencils: x is the LAST array axis, component a of a gradient field acts on array axis
ndim - 1 - a, w = (wx, wy, wz) are the inverse spacings 1/h as the C ABI takes them;
everything beyond the boundary is zero (the library's one boundary convention).
"""
import math

import numpy as np

LOSSES = ("linear", "soft_l1", "huber", "cauchy", "arctan")
HUBER_GAMMA = 1.345            # loss_functions.py's default, fixed in loss_cost_grad


def as_scalar(v, dtype):
    """The scalar v as the kernel of element type dtype sees it: (T)v, in float64."""
    with np.errstate(over="ignore"):
        return float(np.dtype(dtype).type(v))


def _f(x):
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------ element-wise
def lincomb2(a, x, b, y, dtype=np.float64):
    return as_scalar(a, dtype) * _f(x) + as_scalar(b, dtype) * _f(y)


def lincomb3(a, x, b, y, c, z, dtype=np.float64):
    return (as_scalar(a, dtype) * _f(x) + as_scalar(b, dtype) * _f(y)
            + as_scalar(c, dtype) * _f(z))


def scale(x, a, divide=False, dtype=np.float64):
    return _f(x) / as_scalar(a, dtype) if divide else _f(x) * as_scalar(a, dtype)


def clip(x, lo, hi, dtype=np.float64):
    """v < lo ? lo : v, then v > hi ? hi : v (bounds of +-inf stay +-inf)."""
    lo, hi = as_scalar(lo, dtype), as_scalar(hi, dtype)
    v = _f(x)
    v = np.where(v < lo, lo, v)
    return np.where(v > hi, hi, v)


def extrapolate(a, b, theta, dtype=np.float64):
    a = _f(a)
    return a + as_scalar(theta, dtype) * (a - _f(b))


def prox_ell1(u, bt, tau, dtype=np.float64):
    """bt + max(|u - bt| - tau, 0) * sign(u - bt)."""
    u, bt = _f(u), _f(bt)
    d = u - bt
    return bt + np.maximum(np.abs(d) - as_scalar(tau, dtype), 0.) * np.sign(d)


def prox_ell2(u, bt, tau, dtype=np.float64):
    """float64: (u + tau bt) / (1 + tau); float32: (u + tau bt) * float32(1 / (1 + tau)),
    the reciprocal formed in double on the host."""
    num = _f(u) + as_scalar(tau, dtype) * _f(bt)
    if np.dtype(dtype) == np.float64:
        return num / (1.0 + float(tau))
    return num * as_scalar(1.0 / (1.0 + float(tau)), dtype)


def prox_dual_clamp(x, den=1.0, dtype=np.float64):
    """q / max(1, |q|) = min(max(q, -1), 1) with q = x / den; float32 multiplies by
    float32(1 / den)."""
    if np.dtype(dtype) == np.float64:
        q = _f(x) / float(den)
    else:
        q = _f(x) * as_scalar(1.0 / float(den), dtype)
    return np.minimum(np.maximum(q, -1.), 1.)


def _norm2(t, ndim):
    """t_0^2 + t_1^2 + ... added in this order; t: (ndim, m)."""
    t = _f(t).reshape(ndim, -1)
    n2 = t[0] * t[0]
    for a in range(1, ndim):
        n2 = n2 + t[a] * t[a]
    return t, n2


def vector_shrink(t, ndim, thr, dtype=np.float64):
    """Isotropic soft threshold of the ndim-vectors of a stacked field (ndim blocks):
    max(|nrm| - thr, 0) * sign(nrm) * t_a / nrm where nrm > thr, else 0 -- also where
    nrm = 0 = thr (never 0 / 0)."""
    shape = np.shape(t)
    t, n2 = _norm2(t, ndim)
    thr = as_scalar(thr, dtype)
    nrm = np.sqrt(n2)
    on = nrm > thr
    mag = np.maximum(np.abs(nrm) - thr, 0.) * np.sign(nrm)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(on[None], mag[None] * t / nrm[None], 0.)
    return v.reshape(shape)


# ------------------------------------------------------------------- robust losses
def loss_eval(name, f2, f_scale=1.0, gamma=HUBER_GAMMA, dtype=np.float64):
    """(rho, rho') of loss_functions.py at f2 = r^2 with z = f2 / f_scale^2:
    linear   f2                           1
    soft_l1  2 (sqrt(1 + z) - 1) s2       1 / sqrt(1 + z)
    huber    z s2 | (2 g sqrt(z) - g^2) s2      1 | g / sqrt(z)      (z < g^2 | else)
    cauchy   log1p(z) s2                  1 / (1 + z)
    arctan   atan(z) s2                   1 / (1 + z^2)"""
    f2 = _f(f2)
    s2 = as_scalar(float(f_scale) * float(f_scale), dtype)
    z = f2 / s2
    if name == "linear":
        return f2.copy(), np.ones_like(f2)
    if name == "soft_l1":
        q = np.sqrt(1. + z)
        return 2. * (q - 1.) * s2, 1. / q
    if name == "huber":
        gm = as_scalar(gamma, dtype)
        g2 = gm * gm
        q = np.sqrt(z)
        with np.errstate(divide="ignore"):
            return (np.where(z < g2, z * s2, (2. * gm * q - g2) * s2),
                    np.where(z < g2, 1., gm / q))
    if name == "cauchy":
        return np.log1p(z) * s2, 1. / (1. + z)
    if name == "arctan":
        return np.arctan(z) * s2, 1. / (1. + z * z)
    raise ValueError(name)


def loss_terms(r, name, f_scale=1.0, minus=None, dtype=np.float64):
    """(rho_i, g_i) of loss_cost_grad: the residual r (1 * r + (-1) * minus when given),
    rho(r^2) and rho'(r^2) * r, Huber's gamma at its default."""
    rv = _f(r) if minus is None else 1. * _f(r) + (-1.) * _f(minus)
    rho, drho = loss_eval(name, rv * rv, f_scale, HUBER_GAMMA, dtype)
    return rho, drho * rv


def loss_cost_grad(r, name, f_scale=1.0, minus=None, dtype=np.float64):
    """(0.5 * sum rho, gradient)."""
    rho, g = loss_terms(r, name, f_scale, minus, dtype)
    return 0.5 * math.fsum(rho), g


# ---------------------------------------------------------------------- reductions
def dot_terms(x, y):
    return _f(x).reshape(-1) * _f(y).reshape(-1)


def dot(x, y):
    return math.fsum(dot_terms(x, y))


def norm2(x):
    return math.sqrt(dot(x, x))


def vector_norm_terms(t, ndim, mode=0, gamma=0.05, dtype=np.float64):
    """Per voxel: mode 0 sqrt(sum_a t_a^2); mode 1 huber(sum_a t_a^2; gamma) / (2 gamma)
    with f_scale = 1 (prior_measures.py:27-52)."""
    _, n2 = _norm2(t, ndim)
    if mode == 0:
        return np.sqrt(n2)
    if mode != 1:
        raise ValueError("mode must be 0 or 1")
    rho, _ = loss_eval("huber", n2, 1.0, gamma, dtype)
    return rho / (2. * as_scalar(gamma, dtype))


def vector_norm_sum(t, ndim, mode=0, gamma=0.05, dtype=np.float64):
    return math.fsum(vector_norm_terms(t, ndim, mode, gamma, dtype))


def pair_terms(x, y, mx=0.0, my=0.0):
    """The terms of the eight statistics of one (x, y) pair, a row each:
    (x-mx)(y-my), (x-mx)^2, (y-my)^2, |x-y|, (x-y)^2, y, x, y.  Row 5 is reduced by a
    maximum, every other row by a sum."""
    x, y = _f(x).reshape(-1), _f(y).reshape(-1)
    dx, dy, d = x - float(mx), y - float(my), x - y
    return np.stack([dx * dy, dx * dx, dy * dy, np.abs(d), d * d, y, x, y])


def pair_stats(x, y, mx=0.0, my=0.0):
    t = pair_terms(x, y, mx, my)
    return np.array([float(np.max(t[k])) if k == 5 else math.fsum(t[k])
                     for k in range(8)])


# ------------------------------------------------------------------------ stencils
def shifted(u, axis, forward):
    """u moved by one along axis: forward -> the neighbour at +1, else at -1; zero
    where there is none."""
    nb = np.zeros_like(u)
    src = [slice(None)] * u.ndim
    dst = [slice(None)] * u.ndim
    if forward:
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
    else:
        src[axis], dst[axis] = slice(0, -1), slice(1, None)
    nb[tuple(dst)] = u[tuple(src)]
    return nb


def diff_axis(x, direction, adjoint, w, dtype=np.float64):
    """Difference along direction 0 (x, the last axis), 1 (y) or 2 (z) of an array of
    up to three axes: forward nb * w + x * (-w) with nb the neighbour at +1, adjoint
    x * (-w) + nb * w with nb the neighbour at -1."""
    x = _f(x)
    w = as_scalar(w, dtype)
    axis = x.ndim - 1 - direction
    if adjoint:
        return x * (-w) + shifted(x, axis, False) * w
    return shifted(x, axis, True) * w + x * (-w)


def grad(x, w=(1., 1., 1.), dtype=np.float64):
    """Forward differences of every axis, stacked on a new first axis (component 0 = x)."""
    x = _f(x)
    return np.stack([diff_axis(x, a, False, w[a], dtype) for a in range(x.ndim)])


def grad_adj(p, w=(1., 1., 1.), dtype=np.float64):
    """The exact transpose of grad: p of shape (d,) + volume; the components are added
    x, y, z."""
    p = _f(p)
    acc = diff_axis(p[0], 0, True, w[0], dtype)
    for a in range(1, p.shape[0]):
        acc = acc + diff_axis(p[a], a, True, w[a], dtype)
    return acc


def grad_adj_axpy(p, x, tau, w=(1., 1., 1.), dtype=np.float64):
    """x - tau * grad_adj(p)."""
    return _f(x) - as_scalar(tau, dtype) * grad_adj(p, w, dtype)


# ------------------------------------------- one primal-dual iteration (nsol_pd*.hip)
def project_iso(q, dimension, den=None):
    """q: `dimension` stacked blocks.  q_a <- q_a / den (Huber only), then
    s = ((q0 q0) + q1 q1) + q2 q2, m = max(1, sqrt(s)), p_a = q_a / m: dual_project of
    csrc/nsol_pd_iso_body.hpp.  Works in q's own precision."""
    if den is not None:
        q = q / den
    parts = np.array_split(q, dimension)
    s = parts[0] * parts[0]
    for a in range(1, dimension):
        s = s + parts[a] * parts[a]
    m = np.maximum(1, np.sqrt(s))
    return np.concatenate([pa / m for pa in parts])


def pd_dual_q(xbar, p, sigma, w, dtype=np.float64):
    """q_a = p_a + sigma * (hi * w_a + lo * (-w_a)), stacked on a new first axis: the
    argument of the dual prox (dual_update / dual_q).  p = None: zero."""
    xbar = _f(xbar)
    sg = as_scalar(sigma, dtype)
    return np.stack([(0. if p is None else _f(p)[a])
                     + sg * diff_axis(xbar, a, False, w[a], dtype)
                     for a in range(xbar.ndim)])


def pd_dual_step(xbar, p, sigma, hden, w, dtype=np.float64, iso=False):
    """The new dual field, shape (ndim,) + volume.  Huber (hden != 1): float64 q / hden,
    float32 q * float32(1 / hden); then min(max(q, -1), 1) per component, or (iso) the
    projection of the voxel's vector onto the unit ball, project_iso."""
    q = pd_dual_q(xbar, p, sigma, w, dtype)
    if not iso:
        return prox_dual_clamp(q, hden, dtype)
    den = None
    if float(hden) != 1.0:
        if np.dtype(dtype) == np.float64:
            den = float(hden)
        else:
            q = q * as_scalar(1.0 / float(hden), dtype)
    return project_iso(q.reshape(-1), q.shape[0], den).reshape(q.shape)


def pd_primal_step(p, x, bt, tau, tl, theta, w, l1, dtype=np.float64):
    """(x_new, xbar_new): kt = grad_adj(p) (components added x, y, z), u = x - tau * kt,
    x_new = prox_ell1 / prox_ell2 (u, bt, tl), xbar_new = x_new + theta * (x_new - x)."""
    u = grad_adj_axpy(p, x, tau, w, dtype)
    x_new = prox_ell1(u, bt, tl, dtype) if l1 else prox_ell2(u, bt, tl, dtype)
    return x_new, extrapolate(x_new, x, theta, dtype)


def pd_iteration(xbar, x, bt, p, sigma, hden, tau, tl, theta, w, l1, dtype=np.float64,
                 iso=False):
    """(p_new, x_new, xbar_new) of one iteration: pd_dual_step, then pd_primal_step on
    its result."""
    p_new = pd_dual_step(xbar, p, sigma, hden, w, dtype, iso)
    return (p_new,) + pd_primal_step(p_new, x, bt, tau, tl, theta, w, l1, dtype)


# ------------------------- the weighted (WGT) and the linear (LIN) form of the iteration
def prox_data_w(u, bt, w, tl, l1, dtype=np.float64):
    """prox_data_w of csrc/nsol_pd_weighted.hpp: t = tl * w, then (u + t bt) / (1 + t) --
    a division in either type -- or (l1) bt + max(|u - bt| - t, 0) sign(u - bt); u ITSELF
    where w == 0, whatever bt holds there (a select on w, not a product with 0).  Works in
    the arrays' own precision, as project_iso does: float64 arrays give the reference."""
    u, bt, w = np.asarray(u), np.asarray(bt), np.asarray(w)
    t = as_scalar(tl, dtype) * w
    with np.errstate(invalid="ignore", over="ignore"):
        if l1:
            d = u - bt
            r = bt + np.maximum(np.abs(d) - t, 0.) * np.sign(d)
        else:
            r = (u + t * bt) / (1. + t)
    return np.where(w == 0, u, r)


def box_in(lo, hi, dtype=np.float64):
    """(lo, hi) as the linear kernels see the caller's float64 box (box_in of
    csrc/nsol_pd_launch.hpp): float64 as given; float32 rounded to nearest and then moved
    one spacing INWARD where that left the box -- except lo == hi, and a box that holds no
    float32 at all, which stay as rounded to nearest."""
    lo, hi = float(lo), float(hi)
    if np.dtype(dtype) == np.float64:
        return lo, hi
    with np.errstate(over="ignore"):
        l, h = np.float32(lo), np.float32(hi)
    if lo != hi:
        li, hj = l, h
        if float(li) < lo:
            li = np.nextafter(li, np.float32(np.inf))
        if float(hj) > hi:
            hj = np.nextafter(hj, np.float32(-np.inf))
        if li <= hj:
            l, h = li, hj
    return float(l), float(h)


def pd_lin_step(x, kt, g, tau, lo, hi, dtype=np.float64):
    """lin_step of csrc/nsol_pd_lin_step.hpp: u = x - tau * (kt + g), then
    c = u < lo ? lo : u and c > hi ? hi : c on the box box_in(lo, hi): the selects as the
    kernel makes them (u == lo keeps u, so -0.0 stays -0.0 on lo = 0)."""
    lo, hi = box_in(lo, hi, dtype)
    u = _f(x) - as_scalar(tau, dtype) * (_f(kt) + _f(g))
    cl = np.where(u < lo, lo, u)
    return np.where(cl > hi, hi, cl)


def pd_weighted_primal_step(p, x, bt, wt, tau, tl, theta, w, l1, dtype=np.float64):
    """(x_new, xbar_new) of k_pd_w: pd_primal_step with prox_data_w as the data prox."""
    u = grad_adj_axpy(p, x, tau, w, dtype)
    x_new = prox_data_w(u, bt, wt, tl, l1, dtype)
    return x_new, extrapolate(x_new, x, theta, dtype)


def pd_lin_primal_step(p, x, g, tau, theta, lo, hi, w, dtype=np.float64):
    """(x_new, xbar_new) of k_pd_lin: kt = grad_adj(p), x_new = pd_lin_step(x, kt, g)."""
    x_new = pd_lin_step(x, grad_adj(p, w, dtype), g, tau, lo, hi, dtype)
    return x_new, extrapolate(x_new, x, theta, dtype)


def pd_weighted_iteration(xbar, x, bt, wt, p, sigma, hden, tau, tl, theta, w, l1,
                          dtype=np.float64, iso=False):
    """(p_new, x_new, xbar_new): pd_dual_step, then pd_weighted_primal_step on its result."""
    p_new = pd_dual_step(xbar, p, sigma, hden, w, dtype, iso)
    return (p_new,) + pd_weighted_primal_step(p_new, x, bt, wt, tau, tl, theta, w, l1,
                                              dtype)


def pd_lin_iteration(xbar, x, g, p, sigma, hden, tau, theta, lo, hi, w, dtype=np.float64,
                     iso=False):
    """(p_new, x_new, xbar_new): pd_dual_step, then pd_lin_primal_step on its result."""
    p_new = pd_dual_step(xbar, p, sigma, hden, w, dtype, iso)
    return (p_new,) + pd_lin_primal_step(p_new, x, g, tau, theta, lo, hi, w, dtype)


def pdl_dual_prox(v, c, sigma, w, l1):
    """The prox of the data term's conjugate as k_pdl_dual_data writes it: (v c) / (c + sigma)
    or (l1) r = v < -c ? -c : v, then r > c ? c : r; +0 where w == 0, whatever v holds.  Works
    in the arrays' own precision."""
    v, c, w = np.asarray(v), np.asarray(c), np.asarray(w)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if l1:
            r = np.where(v < -c, -c, v)
            r = np.where(r > c, c, r)
        else:
            r = (v * c) / (c + sigma)
    return np.where(w == 0, np.zeros_like(r), r)


def pdl_dual_data(q, t, bt, wt, sigma, lmbda, l1, dtype=np.float64):
    """k_pdl_dual_data of csrc/nsol_pdl.hip: v = q + sigma * (t - bt), or q - sigma * bt
    with t None; c = lmbda * w (w = 1 with wt None); pdl_dual_prox."""
    sg, lm = as_scalar(sigma, dtype), as_scalar(lmbda, dtype)
    w = np.ones_like(_f(q)) if wt is None else _f(wt)
    with np.errstate(invalid="ignore", over="ignore"):
        v = _f(q) + sg * (_f(t) - _f(bt)) if t is not None else _f(q) - sg * _f(bt)
    return pdl_dual_prox(v, lm * w, sg, w, l1)


# ------------------------------ the Poisson (Kullback-Leibler) data term (csrc/nsol_kl.hpp)
def kl_dual_prox(v, c, sigma, bt, w=None):
    """kl_dual_prox of csrc/nsol_kl.hpp, the prox of sigma F* for F = c (u - bt log u) at
    v: d = v - c, s = sqrt(d d + 4 ((sigma c) bt)), then c - (2 ((sigma c) bt)) / (d + s)
    where d > 0 and c + 0.5 (d - s) elsewhere -- one number in two forms, each free of the
    other's cancellation; never above c, and min(v, c) where bt == 0.  +0 where w == 0,
    whatever bt holds there (w None: no such select).  Works in the arrays' own precision,
    as prox_data_w does: float64 arrays give the reference."""
    v, c, sigma, bt = np.asarray(v), np.asarray(c), np.asarray(sigma), np.asarray(bt)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = v - c
        scb = (sigma * c) * bt
        s = np.sqrt(d * d + 4. * scb)
        r = np.where(d > 0, c - (2. * scb) / (d + s), c + 0.5 * (d - s))
    return r if w is None else np.where(np.asarray(w) == 0, np.zeros_like(r), r)


def prox_kl(u, bt, t, w=None):
    """prox_kl of csrc/nsol_kl.hpp, the prox of t (x - bt log x) at u: e = u - t,
    s = sqrt(e e + 4 (t bt)), then 0.5 (e + s) where e >= 0 and (2 (t bt)) / (s - e)
    elsewhere; never negative, and max(u - t, 0) where bt == 0.  u ITSELF where w == 0,
    whatever bt holds there (w None: no such select).  Works in the arrays' own
    precision."""
    u, bt, t = np.asarray(u), np.asarray(bt), np.asarray(t)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = u - t
        tb = t * bt
        s = np.sqrt(e * e + 4. * tb)
        r = np.where(e >= 0, 0.5 * (e + s), (2. * tb) / (s - e))
    return r if w is None else np.where(np.asarray(w) == 0, u, r)


def prox_kl_w(u, bt, wt, tl, dtype=np.float64):
    """k_prox_kl and the KL form of k_tgv_primal: t = tl * w (w = 1 with wt None), then
    prox_kl with the select on w."""
    u = np.asarray(u)
    w = np.ones_like(u) if wt is None else np.asarray(wt)
    return prox_kl(u, bt, as_scalar(tl, dtype) * w, w)


def pdl_dual_data_kl(q, t, bt, wt, sigma, lmbda, background=0., dtype=np.float64):
    """k_pdl_dual_data_kl of csrc/nsol_pdl.hip: v = q + sigma * (t + background), or
    q + sigma * background with t None; c = lmbda * w (w = 1 with wt None); kl_dual_prox
    with the select on w."""
    sg, lm, bg = (as_scalar(s, dtype) for s in (sigma, lmbda, background))
    w = np.ones_like(_f(q)) if wt is None else _f(wt)
    with np.errstate(invalid="ignore", over="ignore"):
        v = _f(q) + sg * (_f(t) + bg) if t is not None else _f(q) + sg * bg
    return kl_dual_prox(v, lm * w, sg, _f(bt), w)
