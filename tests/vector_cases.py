"""Inputs, scalars and derived error bounds of the generic vector kernels' tests
(test_vector_ops_host.py checks them on the CPU, test_vector_ops_gpu.py uses them).

Inputs are random values rounded to the kernel's element type and held in float64, with
values PLANTED exactly on every branch at the front and again at the very end of the
array (the tail element of the last workgroup).  All branch scalars are dyadic, so the
planted values sit on the branch in float32 as well.

Float32 gate, per element:  |got - want| <= R * 2^-24 * S_i  with R the number of
rounded float32 operations of the expression (a divide or a square root counts 3) and
S_i the sum of the magnitudes of the expression's terms in float64.  R and S are written
down here from the kernels' source (csrc/nsol_ops.hip, csrc/nsol_common.hpp), before any
kernel ran against them.
"""
import numpy as np

from nsol_amd import vector_numpy as vn

U32 = 2.0 ** -24
U64 = 2.0 ** -53

A, B, C = 1.7, -0.6, 0.35           # lincomb coefficients
SCALE = 1.0 / 3.0
LO, HI = -0.5, 0.75                 # clip
THETA = 0.9
TAU1 = 0.5                          # prox_ell1 (dyadic: |u - bt| == tau can be planted)
TAU2 = 0.3
DEN = 1.035                         # 1 + sigma * gamma of prox_huber_conj
THR = 0.5                           # vector_shrink
F_SCALE, GAMMA = 2.0, 1.5           # loss_eval: s2 = 4, gamma^2 = 2.25, both exact
COST_F_SCALE = 1.7                  # loss_cost_grad (gamma fixed at 1.345)
NORM_GAMMA = 0.6                    # vector_norm_sum, mode 1
W_AXIS = 1.3                        # diff_axis


def unit(dtype):
    return U64 if np.dtype(dtype) == np.float64 else U32


def c(v, dtype):
    return vn.as_scalar(v, dtype)


def rounded(a, dtype):
    return np.asarray(a).astype(dtype).astype(np.float64)


def plant(x, values):
    """values at the front of x and, reversed, at its end (as many as fit)."""
    v = np.asarray(values, dtype=np.float64)
    k = min(v.size, x.size)
    x[:k] = v[:k]
    if x.size >= 2 * v.size:
        x[x.size - v.size:] = v[::-1]
    return x


def _rng(n, salt):
    return np.random.default_rng(77000 + 13 * salt + n % 100003)


def normal(n, dtype, salt, scale=1.0):
    return rounded(scale * _rng(n, salt).standard_normal(n), dtype)


# ---------------------------------------------------------------- element-wise inputs
def inputs(op, n, dtype):
    """Dict of the float64 input arrays of `op` at length n (field ops: (ndim, n))."""
    up = lambda v: float(np.nextafter(np.dtype(dtype).type(v), np.dtype(dtype).type(np.inf)))
    dn = lambda v: float(np.nextafter(np.dtype(dtype).type(v), np.dtype(dtype).type(-np.inf)))
    if op in ("lincomb2", "extrapolate"):
        return dict(x=normal(n, dtype, 1), y=normal(n, dtype, 2))
    if op == "lincomb3":
        return dict(x=normal(n, dtype, 1), y=normal(n, dtype, 2), z=normal(n, dtype, 3))
    if op in ("scale", "scale_div"):
        return dict(x=normal(n, dtype, 4))
    if op in ("clip", "clip_inf"):
        x = normal(n, dtype, 5, 0.8)
        return dict(x=plant(x, [LO, HI, dn(LO), up(LO), dn(HI), up(HI), 0.]))
    if op == "prox_dual_clamp":
        x = normal(n, dtype, 6, 1.2)
        return dict(x=plant(x, [0., -0., 1., -1.]))
    if op in ("prox_ell1", "prox_ell2"):
        u, bt = normal(n, dtype, 7, 0.5), normal(n, dtype, 8, 0.5)
        # |u - bt| == tau on both sides, u == bt, one ulp inside and outside
        plant(bt, [0.25, 0.25, 0.25, 0.25, 0.25, 0.25])
        plant(u, [0.75, -0.25, 0.25, up(0.75), dn(0.75), dn(-0.5) + 0.25])
        return dict(x=u, bt=bt)
    if op.startswith("shrink"):
        ndim = int(op[-1])
        t = np.stack([normal(n, dtype, 10 + a, 0.5) for a in range(ndim)])
        # norm == thr, just above, just below (sqrt(fl(a * a)) == a in IEEE arithmetic),
        # the zero vector, and 3-4-5 scaled to norm == thr where there are two components
        heads = [THR, up(THR), dn(THR), 0., -THR]
        cols = [[h] + [0.] * (ndim - 1) for h in heads]
        if ndim >= 2:
            cols.append([0.3, 0.4] + [0.] * (ndim - 2))   # (not exact: either side)
            cols.append([0.] * (ndim - 1) + [THR])
        cols = np.array(cols).T                            # (ndim, k)
        for a in range(ndim):
            plant(t[a], rounded(cols[a], dtype))
        return dict(t=t)
    if op.startswith("loss_eval"):
        f2 = rounded(normal(n, dtype, 20, 3.0) ** 2, dtype)
        g2s2 = GAMMA * GAMMA * F_SCALE * F_SCALE           # z == gamma^2 exactly
        return dict(f2=plant(f2, [g2s2, 0., up(g2s2), dn(g2s2), 1.0]))
    if op == "diff_axis":
        return dict(x=normal(n, dtype, 30))
    raise ValueError(op)


def residual_inputs(n, dtype):
    """r and b of loss_cost_grad: r == b and r == 0 planted (f2 == 0)."""
    r, b = normal(n, dtype, 40, 2.0), normal(n, dtype, 41, 1.0)
    plant(r, [0., 0.75, -0.75])
    plant(b, [0., 0.75, 0.25])
    return r, b


def cancelling_pair(n, dtype):
    """x, y with sum x y << sum |x y|: y's second half undoes the first."""
    x, y = normal(n, dtype, 50), normal(n, dtype, 51)
    h = n // 2
    x[h:2 * h] = x[:h]
    y[h:2 * h] = -y[:h]
    return x, y


def field(n, ndim, dtype, salt=60):
    return np.stack([normal(n, dtype, salt + a, 0.5) for a in range(ndim)])


# --------------------------------------------------- element-wise: want, R and S
def _abs(*terms):
    return sum(np.abs(t) for t in terms)


def expected(op, v, dtype):
    """(want, R, S) of an element-wise operation on the inputs v.  R = 0: the
    kernel performs no rounded operation (or, float64, the same IEEE operations in the
    same order as the restatement): the result must be equal."""
    x = v.get("x")
    if op == "lincomb2":            # a x, b y, + : 3
        return (vn.lincomb2(A, x, B, v["y"], dtype), 3,
                _abs(c(A, dtype) * x, c(B, dtype) * v["y"]))
    if op == "lincomb3":            # three products, two sums: 5
        return (vn.lincomb3(A, x, B, v["y"], C, v["z"], dtype), 5,
                _abs(c(A, dtype) * x, c(B, dtype) * v["y"], c(C, dtype) * v["z"]))
    if op == "scale":               # one product
        return vn.scale(x, SCALE, False, dtype), 1, _abs(x * c(SCALE, dtype))
    if op == "scale_div":           # one division: 3
        return vn.scale(x, SCALE, True, dtype), 3, _abs(x / c(SCALE, dtype))
    if op == "clip":                # comparisons and selects only
        return vn.clip(x, LO, HI, dtype), 0, None
    if op == "clip_inf":
        return vn.clip(x, -np.inf, np.inf, dtype), 0, None
    if op == "extrapolate":         # v - b, theta *, v + : 3
        return (vn.extrapolate(x, v["y"], THETA, dtype), 3,
                _abs(x) + abs(c(THETA, dtype)) * _abs(x, v["y"]))
    if op == "prox_dual_clamp":     # float32: one product, then a median of three
        return vn.prox_dual_clamp(x, DEN, dtype), 1, _abs(x * c(1. / DEN, dtype))
    if op == "prox_ell1":           # u - bt, |d| - tau, (sign: exact), bt + : 3
        return (vn.prox_ell1(x, v["bt"], TAU1, dtype), 3,
                _abs(x, v["bt"], v["bt"]) + TAU1)
    if op == "prox_ell2":           # tau bt, u +, * reciprocal: 3
        return (vn.prox_ell2(x, v["bt"], TAU2, dtype), 3,
                _abs(x, c(TAU2, dtype) * v["bt"]) / (1. + TAU2))
    if op.startswith("shrink"):
        # nrm = sqrt(n2): ndim products, ndim - 1 sums, sqrt 3 -- and nrm enters the
        # result twice, through mag = nrm - thr (an error e there moves the result by
        # e |t| / nrm) and as the divisor: 2 (2 ndim + 2); then |nrm| - thr 1, mag * t 1,
        # / nrm 3.  Every term is bounded by u (nrm + thr) |t_a| / nrm
        ndim = int(op[-1])
        t = v["t"]
        nrm = np.sqrt(np.sum(t * t, axis=0))
        with np.errstate(divide="ignore", invalid="ignore"):
            S = np.where(nrm > 0, (nrm + THR) * np.abs(t) / nrm, 0.)
        return vn.vector_shrink(t, ndim, THR, dtype), 4 * ndim + 9, S
    if op == "diff_axis":           # nb w, c (-w), + : 3
        raise ValueError("diff_axis has its own check")
    raise ValueError(op)


# R of (rho, rho') of loss_eval in float32, with z = f2 / s2 counted 3:
#  linear   no operation
#  soft_l1  q = sqrt(1 + z): 3 + 1 + 3 = 7 (its relative error, that of 1 + z halved, is
#           within 7 u); rho = 2 (q - 1) s2: the error of q enters (q - 1) absolutely, then
#           one subtraction and one product: 9, against S = 2 (q + 1) s2;  rho' = 1 / q: 10
#  huber    below: rho = z s2: 4;  above: q = sqrt(z) 6, g2 = gm gm 1, 2 gm q 1, - 1, s2 1:
#           10 against S = (2 gm q + g2) s2;  rho' = gm / q: 9.  The two forms agree to
#           second order where z = g2, so a branch decided differently within the error
#           of z stays inside the bound
#  cauchy   rho = (T)log1p((double)z) s2: 3 + 1 + 1 = 5 (d log1p(z) / log1p(z) <= dz / z);
#           rho' = 1 / (1 + z): 3 + 1 + 3 = 7
#  arctan   rho = (T)atan((double)z) s2: 5 (d atan(z) / atan(z) <= dz / z);
#           rho' = 1 / (1 + z z): the error of z counts twice in z z: 6 + 1 + 1 + 3 = 11
LOSS_R = {"linear": (0, 0), "soft_l1": (9, 10), "huber": (10, 9), "cauchy": (5, 7),
          "arctan": (5, 11)}
# float64: the same IEEE operations as NumPy's (correctly rounded sqrt and division),
# except log1p and atan, which come from different libraries: the goldens' rtol 1e-14
F64_INEXACT_RHO = ("cauchy", "arctan")
F64_LIBM_RTOL = 1e-14


def loss_S(name, f2, f_scale, gamma, dtype):
    """(S_rho, S_drho): the magnitudes the float32 bounds of loss_eval refer to."""
    rho, drho = vn.loss_eval(name, f2, f_scale, gamma, dtype)
    s2 = c(f_scale * f_scale, dtype)
    z = f2 / s2
    if name == "soft_l1":
        return 2. * (np.sqrt(1. + z) + 1.) * s2, drho
    if name == "huber":
        gm = c(gamma, dtype)
        return np.where(z < gm * gm, z * s2, (2. * gm * np.sqrt(z) + gm * gm) * s2), drho
    return np.abs(rho), drho


# rho'(r^2) r of loss_cost_grad: r - b is one rounding (relative to r - b itself), r r
# one more, so f2 carries 3 u on top of what LOSS_R counts from z = f2 / s2 on (twice
# that for arctan's z z); then the product with r - b and that factor's own rounding: 2.
def grad_R(name):
    return LOSS_R[name][1] + (6 if name == "arctan" else 3) + 2


def rho_R(name):
    """rho(r^2) as a term of the cost (formed in T before it is added in double)."""
    return LOSS_R[name][0] + 3


def norm_R(ndim, mode):
    """The per-voxel term of vector_norm_sum: n2 (2 ndim - 1), then sqrt (3) or Huber's
    rho (10) divided (3) by 2 gamma."""
    return 2 * ndim - 1 + (3 if mode == 0 else 13)


# ---------------------------------------------------------------------- reductions
def trips(n, max_grid_blocks=2048, per=1, cap=None):
    """Additions a thread makes into its double accumulator: trips of the grid-stride
    loop of `per` elements each."""
    count = n // per
    grid = min(max(1, -(-count // 256)), max_grid_blocks)
    if cap is not None:
        grid = min(grid, cap)
    return -(-count // (grid * 256)) * per


def sum_bound(terms, n_trips, R=0, dtype=np.float64):
    """|got - fsum(terms)| <= ((trips + 32) 2^-53 + R eps_T) sum |terms|: 32 covers the
    wave tree (6), the four wave partials and the final pass; R eps_T the rounding of
    terms formed in T before they are widened."""
    return ((n_trips + 32) * U64 + R * unit(dtype)) * float(np.sum(np.abs(terms)))


# ----------------------------------------------------------------- branch fractions
def branch_fractions(n=1021, dtype=np.float32):
    """The share of the RANDOM elements (planted ones included: a handful) on the
    'active' side of every branch, from the restatement alone."""
    out = {}
    x = inputs("clip", n, dtype)["x"]
    out["clip below"] = np.mean(x < LO)
    out["clip above"] = np.mean(x > HI)
    out["clip inside"] = np.mean((x >= LO) & (x <= HI))
    x = inputs("prox_dual_clamp", n, dtype)["x"]
    out["dual clamp inside"] = np.mean(np.abs(x / DEN) <= 1.)
    v = inputs("prox_ell1", n, dtype)
    out["prox_ell1 shrunk to bt"] = np.mean(np.abs(v["x"] - v["bt"]) <= TAU1)
    for ndim in (1, 2, 3):
        t = inputs("shrink%d" % ndim, n, dtype)["t"]
        out["shrink%d on" % ndim] = np.mean(np.sqrt(np.sum(t * t, axis=0)) > THR)
        t = field(n, ndim, dtype)
        out["norm sum huber%d quadratic" % ndim] = np.mean(
            np.sum(t * t, axis=0) < NORM_GAMMA ** 2)
    f2 = inputs("loss_eval", n, dtype)["f2"]
    out["loss_eval huber quadratic"] = np.mean(f2 / F_SCALE ** 2 < GAMMA ** 2)
    r, b = residual_inputs(n, dtype)
    g2 = vn.HUBER_GAMMA ** 2
    out["cost huber quadratic"] = np.mean(r * r / COST_F_SCALE ** 2 < g2)
    out["cost huber quadratic (r - b)"] = np.mean((r - b) ** 2 / COST_F_SCALE ** 2 < g2)
    return {k: float(f) for k, f in out.items()}
