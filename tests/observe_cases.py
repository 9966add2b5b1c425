"""Inputs, float64 reference and derived gates of the observation kernels' tests
(csrc/nsol_observe.hip: k_observe, k_observe_final, k_observe_widen).
test_observe_kernels_host.py anchors the reference on the oracle on the CPU,
test_observe_kernels_gpu.py holds the kernels to it.

The kernel widens every voxel as (double)(x[i] * (T)x_scale), the product rounded in
the element type T, and does everything after that in float64 without contraction
(-ffp-contract=off) with IEEE square root and division.  observe_sums_ref repeats those
operations in that order, so a term of the reference is the term the kernel forms; what
is left between the two is the order in which the terms are added.

Gate of a sum, from vector_cases.sum_bound with R = 0 (no term is formed in T):

    |got - fsum(terms)| <= ((trips + 32) + ops) 2^-53 sum |terms|

trips: the additions a thread makes into its accumulator (obs_trips); 32 covers the
wave tree (6), the four wave partials (3), the partial sums one thread of
k_observe_final adds (at most 4096 / 256 = 16), its wave tree (6) and wave partials
(4): 35 at the cap of 4096 workgroups and 27 at the 2048 the library launches at most,
which is the grid that runs; ops: the float64 operations that form a term (TERM_OPS),
one unit roundoff each against the term's magnitude.  That last allowance is sound only
because the reference performs the same operations (a forward difference cancels, and
its rounding error is not small against the difference itself); it leaves room for a
last-place disagreement per operation and no more.
"""
import math

import numpy as np

import vector_cases as vc

PAIR, GRAD, SQ, HUBER = 1, 2, 4, 8
SUMS = 9
NAMES = ("sum d^2", "sum |d|", "sum c", "sum dc (y - ybar)", "sum dc^2", "sum q",
         "sum huber", "sum n2", "sum c^2")
GROUP = (PAIR, PAIR, PAIR, PAIR, PAIR, GRAD, GRAD | HUBER, GRAD, SQ)
SIGNED = (2, 3)                     # sums whose terms change sign
KOBS_BLOCKS = 4096                  # kObsBlocks
KOBS_UNROLL = 4                     # kObsUnroll
HUBER_GAMMA = 0.5                   # of huber_field: gamma^2 = 0.25, both exact

SHAPES = [(1,), (5,), (259,), (1031,), (5, 7), (6, 259), (1, 9), (9, 1), (3, 5, 7),
          (4, 6, 259), (2, 1, 5), (5, 4, 64), (7, 10, 13)]
SCALES = (1.0, 37.5, 0.1)           # 0.1 is not a float32: the kernel rounds it first
SPACINGS = ((1.0, 1.0, 1.0), (0.8, 1.3, 2.0))   # spacing[0] belongs to the last axis
FLAG_SETS = (PAIR, GRAD, SQ, GRAD | HUBER, PAIR | GRAD | SQ | HUBER, HUBER)


def weights(spacing):
    """(wx, wy, wz) = 1 / spacing, as ops.inv_spacing hands them to the kernel."""
    return tuple(1.0 / s for s in spacing)


def dims3(shape):
    shape = tuple(int(s) for s in shape)
    return (len(shape),) + (1,) * (3 - len(shape)) + shape


def term_ops(k, ndim):
    """Float64 operations that form one term of sum k.
      0  d = c - y (1), enters d d twice (2), the product (1)              : 3
      1  d (1); |d| is exact                                               : 1
      2  c itself                                                          : 0
      3  dc = c - ybar (1), y - ybar (1), their product (1)                : 3
      4  dc (1) twice, the product (1)                                     : 3
      7  n2: per component h w (1), c (-w) (1), their sum (1), the square
         (1) -- 4 ndim -- and ndim - 1 additions                           : 5 ndim - 1
      5  q = sqrt(n2): n2's operations (the root halves their relative
         error; not claimed) and the root (1)                              : 5 ndim
      6  huber: n2, and on the linear side q (1), 2 gamma (1), its product
         with q (1), gamma gamma (1), the difference (1); the quotient by
         2 gamma (1)                                                       : 5 ndim + 5
      8  c c                                                               : 1
    """
    return (3, 1, 0, 3, 3, 5 * ndim, 5 * ndim + 5, 5 * ndim - 1, 1)[k]


def obs_trips(n, max_grid_blocks=2048):
    """Additions a thread of k_observe makes into an accumulator: the trips of the grid
    that runs (grid_for(n), at most kObsBlocks workgroups), rounded up to whole steps of
    kObsUnroll elements."""
    strides = vc.trips(n, max_grid_blocks, cap=KOBS_BLOCKS)
    return -(-strides // KOBS_UNROLL) * KOBS_UNROLL


def gate(k, terms, n_trips, ndim):
    return vc.sum_bound(terms, n_trips) + \
        term_ops(k, ndim) * vc.U64 * float(np.sum(np.abs(terms)))


# ------------------------------------------------------------------------ reference
def widen(x, x_scale, dtype):
    """float64(T(x) * T(x_scale)): the product rounded in T, as widen_scaled does."""
    T = np.dtype(dtype).type
    return (np.asarray(x).astype(dtype) * T(x_scale)).astype(np.float64)


def gradient_norm2(xs3, w, ndim):
    """n2 of the zero-padded forward differences D_a = xs[i + e_a] w_a + xs[i] (-w_a),
    the components added in the order x, y, z."""
    n2 = None
    for a in range(ndim):
        axis = 2 - a
        nb = np.zeros_like(xs3)
        dst, src = [slice(None)] * 3, [slice(None)] * 3
        dst[axis], src[axis] = slice(0, -1), slice(1, None)
        nb[tuple(dst)] = xs3[tuple(src)]
        g = nb * w[a] + xs3 * (-w[a])
        n2 = g * g if n2 is None else n2 + g * g
    return n2


def observe_terms(x, x_scale, y, ybar, shape, w, gamma, flags, ndim, dtype):
    """The nine arrays of terms (None where the sum is not asked for)."""
    xs3 = widen(x, x_scale, dtype).reshape(dims3(shape)[1:])
    xs = xs3.reshape(-1)
    t = [None] * SUMS
    if flags & PAIR:
        yv = np.asarray(y, np.float64).reshape(-1)
        d, dc = xs - yv, xs - ybar
        t[0], t[1], t[2], t[3], t[4] = d * d, np.abs(d), xs, dc * (yv - ybar), dc * dc
    if flags & GRAD:
        n2 = gradient_norm2(xs3, w, ndim).reshape(-1)
        q = np.sqrt(n2)
        t[5], t[7] = q, n2
        if flags & HUBER:
            g2, two_gm = gamma * gamma, 2.0 * gamma
            rho = np.where(n2 < g2, n2, 2.0 * gamma * q - g2)
            t[6] = rho / two_gm
    if flags & SQ:
        t[8] = xs * xs
    return t


def observe_sums_ref(x, x_scale, y, ybar, shape, w, gamma, flags, ndim, dtype):
    """(sums, terms) of nsol_observe_*: sums[k] = fsum(terms[k]), exactly 0.0 (and
    terms[k] None) where sum k is not asked for."""
    terms = observe_terms(x, x_scale, y, ybar, shape, w, gamma, flags, ndim, dtype)
    sums = np.array([0.0 if t is None else math.fsum(t) for t in terms])
    return sums, terms


# --------------------------------------------------------------------------- inputs
def _rng(shape, salt):
    return np.random.default_rng(91000 + 17 * salt + 31 * len(shape) +
                                 int(np.prod(shape)) % 100003)


def smooth_field(shape, dtype, salt=0):
    """A smooth field plus noise of a tenth of its amplitude, rounded to dtype."""
    rng = _rng(shape, salt)
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    v = np.ones(shape)
    for a, g in enumerate(grids):
        v = v * np.cos(0.37 * (a + 1) * g / (1.0 + 0.02 * shape[a]) + 0.3 * a)
    return vc.rounded(0.4 + v + 0.1 * rng.standard_normal(shape), dtype)


def reference_for(x, x_scale, dtype, salt=1):
    """A reference near x * x_scale, rounded to dtype (the element type or float64)."""
    rng = _rng(x.shape, salt)
    return vc.rounded(x_scale * (0.9 * x + 0.05 * rng.standard_normal(x.shape)), dtype)


def cancelling_field(shape, dtype, ybar):
    """x = ybar + e and y = ybar + f with e's second half the negative of its first and
    f's the same as its first: sum (x - ybar) and sum (x - ybar)(y - ybar) are next to
    nothing against the sums of their terms' magnitudes (and sum x itself for ybar = 0).
    """
    n = int(np.prod(shape))
    rng = _rng(shape, 2)
    e, f = rng.standard_normal(n), rng.standard_normal(n)
    h = n // 2
    e[h:2 * h], f[h:2 * h] = -e[:h], f[:h]
    return (vc.rounded(ybar + e, dtype).reshape(shape),
            vc.rounded(ybar + f, dtype).reshape(shape))


def huber_field(shape):
    """Quarter steps 0, 1/4, 1/2 and 2 (exact in float32), drawn so that with unit
    weights, x_scale = 1 and gamma = HUBER_GAMMA the norm n2 of the gradient falls below
    gamma^2 (all differences within a quarter), above it, on it (one difference of a
    half, the others 0) and on 0 (a voxel equal to its forward neighbours)."""
    rng = _rng(shape, 3)
    return 0.25 * rng.choice([0.0, 1.0, 2.0, 8.0], size=shape, p=[0.5, 0.2, 0.1, 0.2])


def huber_shares(x, shape, ndim=None):
    """Shares of the voxels of huber_field on either side of, on, and at zero of the
    Huber branch, from the reference's own n2."""
    ndim = len(shape) if ndim is None else ndim
    n2 = gradient_norm2(np.asarray(x, np.float64).reshape(dims3(shape)[1:]),
                        (1.0, 1.0, 1.0), ndim)
    g2 = HUBER_GAMMA * HUBER_GAMMA
    return dict(below=float(np.mean(n2 < g2)), above=float(np.mean(n2 > g2)),
                on=int(np.sum(n2 == g2)), zero=int(np.sum(n2 == 0.0)))


def median_gamma(x, x_scale, shape, w, ndim, dtype):
    """A gamma that splits the voxels of a field about evenly between the two branches."""
    n2 = gradient_norm2(widen(x, x_scale, dtype).reshape(dims3(shape)[1:]), w, ndim)
    return max(float(np.sqrt(np.median(n2))), 2.0 ** -10)


def pitches(nx, dtype):
    """nx + 1, nx + 3 and the next multiple of the 16-byte vector above nx."""
    vw = 16 // np.dtype(dtype).itemsize
    return (nx + 1, nx + 3, (nx // vw + 1) * vw)


def pitched(x, shape, pitch, fill):
    """The rows of x `pitch` elements apart, the gaps holding `fill`."""
    _, nz, ny, nx = dims3(shape)
    out = np.full((nz * ny, pitch), fill, dtype=np.float64)
    out[:, :nx] = np.asarray(x, np.float64).reshape(nz * ny, nx)
    return out.reshape(-1)


def periodic_sums(px, py, n, x_scale, ybar, wx, dtype):
    """(sums, sums of magnitudes) of a 1-D PAIR | GRAD | SQ observation of the period
    (px, py) repeated to n elements, in closed form: every term but the last element's
    difference depends on its place in the period alone, so the sums are reps times
    those of one period, plus the remainder's, with the last element's zero-padded
    difference in place of its periodic one.  Exact rational arithmetic."""
    from fractions import Fraction
    p = px.size
    reps, rem = divmod(n, p)
    flags = PAIR | GRAD | SQ
    # one period followed by its first element: the first p terms are the periodic ones
    ext_x, ext_y = np.append(px, px[0]), np.append(py, py[0])
    t = observe_terms(ext_x, x_scale, ext_y, ybar, (p + 1,), (wx, 1., 1.), 1.0, flags, 1,
                      dtype)
    last = (n - 1) % p
    tl = observe_terms(px[last:last + 1], x_scale, py[last:last + 1], ybar, (1,),
                       (wx, 1., 1.), 1.0, flags, 1, dtype)
    sums, mags = np.zeros(SUMS), np.zeros(SUMS)
    for k in range(SUMS):
        if t[k] is None:
            continue
        per = [Fraction(float(v)) for v in t[k][:p]]
        fix = Fraction(float(tl[k][0])) - per[last] if GROUP[k] & GRAD else Fraction(0)
        sums[k] = float(reps * sum(per) + sum(per[:rem]) + fix)
        aper = [abs(v) for v in per]
        mags[k] = float(reps * sum(aper) + sum(aper[:rem]) + abs(fix))
    return sums, mags
