"""Inputs, float64 references, lengths, counts and gates for the second half of an
L-BFGS-B iteration (nsol_amd/csrc/nsol_lbfgsb.hip: k_wcomb and its CLIP form,
k_subspace_step with r read or formed, k_mdot, k_mdots, k_diff_dots, k_projgr,
k_count_free).  Plain NumPy, no torch; shared by test_lbfgsb_step_host.py (which proves
what is claimed here) and test_lbfgsb_step_gpu.py.

THE REFERENCES restate the formulas of include/nsol_hip.h in float64, from inputs that
are already rounded to the element type T and with every coefficient, scale and bound
rounded to T as the launchers cast them.  None calls device code.  Each takes
mistake=NAME and then evaluates one PLANTED MISTAKE (MISTAKES below) instead: the host
module shows that every one of them changes the expected values at every case of the
tables, so a kernel that made it could not pass.

LATTICE INPUTS.  A stored vector at variable i is a multiple of 1/4 in [-8, 8] from a
32-bit integer hash of (i, row); xcp, x, g, r and y come from the same hash.  Every
coefficient is a multiple of 1/8 in [-1, 1]; the scales (2 for wcomb, 1/4 for the subspace
step), rb3 = (-1/2, 1/2, -1) and the bounds LO = -3.25, HI = 4.5 are dyadic.  Then
  * a term c * v is a multiple of 1/32 of magnitude <= 8, a sum of at most 3 + 40 + 24
    of them a multiple of 1/32 below 536, scaled by 1/4 a multiple of 1/128, and with xcp
    and x added or subtracted still a multiple of 1/128 below 160: 160 * 128 < 2^24, so
    every partial sum is exact in float32, in any order, with or without FMA;
  * a term of a reduction (d * d, g * d, w * d, w * y) is a multiple of 2^-14 below
    2^12: the float64 sums of up to 2^21 of them are exact in any order (< 2^53 * 2^-14).
So the expected values are the same for float32 and float64 (but for the step ratio, a
quotient rounded to T and expected as such) and the gate is EQUALITY
(test_lbfgsb_step_host.py checks both bounds on the arrays themselves and evaluates every
case in float32 in the kernel's order).

The coefficients that meet a box (the subspace step, lincomb_clip) shrink with the number
of vectors (box_coefs: about sqrt(1.4 / nw)), so that the sum keeps the spread of one
vector and of the FREE variables at least a quarter end strictly inside [LO, HI] and at
least a tenth at each bound, whatever nw; variables P_HI / P_LO end exactly at HI / LO
WITHOUT being clipped (all stored vectors 0 there, r = +-1, xcp = x one quarter inside).
x lies strictly inside the box, xcp of a free variable inside or at a face; a variable
that is not free keeps the raw lattice value as xcp (up to 8, outside the box), so its
d = xcp - x overshoots and the smallest step ratio over ALL variables (< 1, lnsrlb's
stpmx) is smaller than the one over the free variables (>= 1).

THE MASK holds {-128, -1, 0} (free, about 60 %) and {1, 2, 127} (not free) from
gram_cases' hash; planted on top: free and fixed variables inside the first 16-byte vector
(0: mask 0, free; 1: mask 1, not free), runs of 16 fixed variables at [16, 32) and one 16
short of the end (whole 16-byte vectors fixed: k_wcomb's skip).

GATES FOR RANDOM DATA (normal values rounded to T), per element |got - ref| <= C u S with
u = 2^-24 / 2^-53 and S the same expression with every term replaced by its magnitude.
The library is built with -ffp-contract=off, so a term c * v is rounded once as a product
and once per addition it then passes through:
  wcomb, lincomb_clip   acc = 0 + c_0 v_0 (exact add) + c_1 v_1 + ... ; acc *= scale.  With
                        m = nbase + nw terms the first two terms pass through 1 product,
                        m - 1 additions and the scaling: m + 1 roundings, (1 + u)^(m+1) - 1
                        <= (m + 2) u.  C = nbase + nw + 2.  The clip is 1-Lipschitz and the
                        mask writes exact zeros.
  subspace step, xn     acc = 0 + 1 * r (both exact) + sum of nw terms, * scale, + xcp: the
                        terms of acc pass through at most 1 + nw + 1 + 1 roundings, xcp
                        through one: C = nw + 4 on S = |xcp| + |scale| (|r| + sum |c w|).
  ... with r formed     r's 3 + nw terms are rounded 3 + nw times (product, additions)
                        before r enters acc, then nw additions, the scaling and + xcp:
                        C = 2 nw + 6 on S with |r| replaced by the sum of its terms'
                        magnitudes.
  d = xn - x            one rounding of the difference of what the kernel STORED as xn:
                        C = 1 on |xn| + |x|.  (diff_dots' out likewise; both are compared
                        in T arithmetic and must be equal.)
hits, count_free, projgr and the step ratio are exact functions of values of T: equal on
random data too (hits and the ratio of what the kernel stored).  Sums: against math.fsum
over the stored values with gram_cases.random_gate's order-free bound, and against the
float64 reference within SUM_GATE (3e-7 / 1e-12, test_blur3_gpu.py's) of the sum of the
reference terms' magnitudes -- g'd and w'd of normal data cancel, their own size is no
scale.
"""
import functools
import math

import numpy as np

import gram_cases as gc

U32, U64 = 2.0 ** -24, 2.0 ** -53
KBLOCK, KRED, DEFAULT_GRID = 256, 1024, 2048
MAXW_COMB, MAXW_STEP, DOTS_PER_LAUNCH = 40, 24, 24
NW_ROWS = 49                         # stored vectors (mdots' longest list)
ROW_XCP, ROW_X, ROW_G, ROW_R, ROW_Y = 49, 50, 51, 52, 53
LO, HI = -3.25, 4.5
STEP_SCALE, RB3 = 0.25, (-0.5, 0.5, -1.0)
COMB_SCALE, BCOEF = 2.0, (-0.75, 0.5, -1.0)
FILL = -7.3                          # outputs before a call (float32(-7.3): on no grid used here)
RES_FILL, WS_FILL = 12345.0, 12345.0  # result rows / ws before a call
DECLINED, EINVAL = -2, -1
SALT = 7
P_HI, P_LO = 5, 6                    # free variables that end at a bound unclipped (n >= 8)
SUM_GATE = {np.float32: 3e-7, np.float64: 1e-12}

MISTAKES = (
    "coef_index",          # wcoef[j + 1] used for vector j
    "drop_fourth",         # the last of an unrolled group of four stored vectors dropped
    "swap_halves",         # the coefficients of the wy and ws halves swapped
    "scale_first",         # the scale applied before r (wcomb: before the base vectors)
    "mask_lt",             # free taken as mask < 0 instead of <= 0
    "fixed_not_zeroed",    # a wholly fixed 16-byte vector keeps the combination
    "clip_swapped",        # the two bounds of the clip swapped
    "d_from_xcp",          # d = xn - xcp instead of xn - x
    "ratio_free_only",     # the step ratio over the free variables only
    "ratio_other_slot",    # the ratio partial read from the other NV's slot of ws
    "tail_skipped",        # the last 16-byte vector (scalar form: element) not visited
    "second_launch",       # mdots' later launches write to result instead of result + 24k
)


def unit(dtype):
    return U64 if np.dtype(dtype) == np.float64 else U32


def vw(dtype):
    return 16 // np.dtype(dtype).itemsize


def rnd(v, dtype):
    """v as the launcher casts it: (T)v."""
    return float(np.dtype(dtype).type(v))


def rounded(a, dtype):
    return np.asarray(a).astype(dtype).astype(np.float64)


def rgrid(units, cap=DEFAULT_GRID):
    """Workgroups of a reduction over `units` vectors (scalar form: elements)."""
    return max(1, min((units + KBLOCK - 1) // KBLOCK, cap, KRED))


# ---- lattice inputs ------------------------------------------------------------------
def _hash_row(k, n):
    i = np.arange(n, dtype=np.uint64)
    h = gc._mix((i * np.uint64(64) + np.uint64(k)) ^ np.uint64(SALT)) % np.uint64(65)
    return (h.astype(np.int64) - 32) / 4.0


def fixed_runs(n):
    """[lo, hi) of the planted runs of 16 fixed variables."""
    runs = []
    if n >= 64:
        runs.append((16, 32))
    if n >= 160:
        e = n // 16 * 16
        runs.append((e - 32, e - 16))
    return runs


def lattice_mask(n):
    m = np.array(gc.mask_values(0, n))
    front = np.array([0, 1, -128, 127, -1, -1, 0, 2], dtype=np.int8)
    m[:min(n, 8)] = front[:n]
    if n >= 9:
        m[n - 1] = -1                            # the tail element counts
    for k, (a, b) in enumerate(fixed_runs(n)):
        m[a:b] = np.array([1, 2, 127], dtype=np.int8)[(np.arange(b - a) + k) % 3]
    return m


class Lattice(object):
    """The lattice problem of n variables: w(k), xcp, x, g, r, y (float64, read-only) and
    mask (int8)."""

    def __init__(self, n):
        self.n = n
        self.mask = lattice_mask(n)
        self.mask.setflags(write=False)
        self.free = self.mask <= 0
        self._rows = {}

    def _row(self, key, make):
        if key not in self._rows:
            a = make()
            a.setflags(write=False)
            self._rows[key] = a
        return self._rows[key]

    def _plant(self, a, hi_value, lo_value, first=None, last=None):
        """The values at P_HI / P_LO; a non-zero first and last element (the only free
        variable of the shortest cases, and the tail)."""
        for i in (0, self.n - 1):
            if a[i] == 0.0:
                a[i] = 1.0
        if first is not None:
            a[0] = first
        if last is not None and self.n >= 9:
            a[self.n - 1] = last                 # x != xcp in the tail element
        if self.n >= 8:
            a[P_HI], a[P_LO] = hi_value, lo_value
        return a

    def w(self, k):
        return self._row(k, lambda: self._plant(_hash_row(k, self.n), 0.0, 0.0))

    @property
    def x(self):
        def make():
            a = np.clip(_hash_row(ROW_X, self.n), LO + 0.25, HI - 0.25)
            return self._plant(a, HI - 0.25, LO + 0.25, 0.5, 1.0)
        return self._row("x", make)

    @property
    def xcp(self):
        def make():
            raw = _hash_row(ROW_XCP, self.n)
            a = np.where(self.free, np.clip(raw, LO, HI), raw)
            if self.n >= 2:
                a[1] = 8.0                       # not free, outside the box: ratio < 1
            return self._plant(a, HI - 0.25, LO + 0.25, 1.0, 2.0)
        return self._row("xcp", make)

    @property
    def g(self):
        return self._row("g", lambda: self._plant(_hash_row(ROW_G, self.n), -1.0, 1.0, -3.0))

    @property
    def r(self):
        return self._row("r", lambda: self._plant(_hash_row(ROW_R, self.n), 1.0, -1.0, 2.0))

    @property
    def y(self):
        return self._row("y", lambda: self._plant(_hash_row(ROW_Y, self.n), 0.5, -0.5))


@functools.lru_cache(maxsize=3)
def lattice(n):
    return Lattice(n)


def comb_coefs(nw):
    """wcomb's coefficients: multiples of 1/8 in [-1, 1]; [1] and [18] are zero (0 * NaN is
    still NaN)."""
    return [(((5 * k + 3) % 17) - 8) / 8.0 for k in range(nw)]


def box_coefs(nw, salt):
    """Coefficients for a sum that meets the box: magnitudes a / 8 and (a - 1) / 8 in turn
    with a^2 / 64 about 1.4 / nw, signs without a short period."""
    a = max(2, min(8, int(round(8.0 * math.sqrt(1.4 / max(nw, 1))))))
    return [(1 if (7 * j + 3 * (j // 5) + salt) % 5 < 3 else -1) * (a - j % 2) / 8.0
            for j in range(nw)]


def step_coefs(nw):
    """(wcoef, rcoef) of the subspace step."""
    return box_coefs(nw, 0), box_coefs(nw, 2)


def projgr_inputs(n):
    """(x, g): g < 0, = 0, = -0.0, > 0 against x below, at, inside (twice) and above each
    bound, at the front and, reversed, before the last two elements.  |g| <= 7.25 elsewhere;
    the last element gives 7.5 with a lower bound (x - lo) and 8 without, the one before
    7.25 with an upper bound and 7.75 without: the largest value sits in the tail and
    differs between the bound combinations."""
    x = _hash_row(ROW_X, n)
    g = np.clip(_hash_row(ROW_G, n), -7.25, 7.25)
    gs = [-2.0, 0.0, -0.0, 2.0]
    xs = [LO - 1.0, LO, LO + 0.5, HI - 0.5, HI, HI + 1.0]
    px = np.array([a for a in xs for _ in gs])
    pg = np.array([b for _ in xs for b in gs])
    k = min(n, px.size)
    x[:k], g[:k] = px[:k], pg[:k]
    if n >= 2 * px.size + 2:
        x[n - 2 - px.size:n - 2], g[n - 2 - px.size:n - 2] = px[::-1], pg[::-1]
    if n >= 2:
        x[n - 2], g[n - 2] = HI - 7.25, -7.75
    x[n - 1], g[n - 1] = LO + 7.5, 8.0
    return x, g


def random_inputs(n, dtype, seed=0):
    """Normal data rounded to T: dict of w [NW, n], xcp, x, g, r, y, mask."""
    rng = np.random.default_rng(4100 + seed + n)
    out = {"w": rounded(rng.standard_normal((MAXW_STEP + 3, n)), dtype)}
    for name in ("xcp", "x", "g", "r", "y"):
        out[name] = rounded(rng.standard_normal(n), dtype)
    out["mask"] = lattice_mask(n)
    return out


# ---- references ----------------------------------------------------------------------
def _free(mask, n, mistake=None):
    if mask is None:
        return np.ones(n, bool)
    return mask < 0 if mistake == "mask_lt" else mask <= 0


def _visited(n, width, mistake):
    """False at what the 'tail_skipped' mistake leaves out: the last `width` elements when
    the vector form runs (n a multiple of width), else the last one."""
    v = np.ones(n, bool)
    if mistake == "tail_skipped":
        v[n - (width if n % width == 0 else 1):] = False
    return v


def _lincomb(coefs, vecs, n, skip=()):
    s, a = np.zeros(n), np.zeros(n)
    for j, (c, v) in enumerate(zip(coefs, vecs)):
        if j in skip:
            continue
        s = s + c * v
        a = a + np.abs(c * v)
    return s, a


def _w_coefs(wcoef, dtype, mistake):
    wc = [rnd(c, dtype) for c in wcoef]
    nw = len(wc)
    if mistake == "coef_index":
        wc = wc[1:] + wc[:1]
    if mistake == "swap_halves":
        h = nw // 2
        wc = wc[h:2 * h] + wc[:h] + wc[2 * h:]
    skip = ()
    if mistake == "drop_fourth":
        skip = tuple(range(3, nw // 4 * 4, 4))
    return wc, skip


def _whole_fixed(free, width):
    """True at the elements of 16-byte vectors that hold no free variable."""
    n = free.size
    if n % width:
        return np.zeros(n, bool)
    return np.repeat(~free.reshape(-1, width).any(axis=1), width)


def wcomb_ref(n, base, bcoef, w, wcoef, scale, mask, dtype, box=None, mistake=None):
    """(out, S) of nsol_lb_wcomb_* (box=None) / nsol_lincomb_clip_* (box=(lo, hi), no base
    vectors, scale 1, no mask): out = free ? scale (sum bcoef base + sum wcoef w) : 0."""
    wc, skip = _w_coefs(wcoef, dtype, mistake)
    sb, ab = _lincomb([rnd(c, dtype) for c in bcoef], base, n)
    sw, aw = _lincomb(wc, w, n, skip)
    sc = rnd(scale, dtype)
    out = sb + sc * sw if mistake == "scale_first" else sc * (sb + sw)
    S = abs(sc) * (ab + aw)
    if box is not None:
        lo, hi = rnd(box[0], dtype), rnd(box[1], dtype)
        if mistake == "clip_swapped":
            lo, hi = hi, lo
        out = np.minimum(np.maximum(out, lo), hi)
    if mask is not None:
        free = _free(mask, n, mistake)
        keep = free | _whole_fixed(free, vw(dtype)) if mistake == "fixed_not_zeroed" else free
        out = np.where(keep, out, 0.0)
        S = np.where(free, S, 0.0)
    out = np.where(_visited(n, vw(dtype), mistake), out, FILL)
    return out, S


def wcomb_count(nbase, nw):
    return nbase + nw + 2


def step_ratio(x, d, lo, hi, dtype):
    """The feasible step ratio of every variable, in T arithmetic as step_ratio() of
    nsol_lbfgsb.hip: d < 0: (lo - x) / d, 0 if lo - x >= 0; d > 0: (hi - x) / d, 0 if
    hi - x <= 0; else inf."""
    T = np.dtype(dtype).type
    xt, dt = np.asarray(x).astype(dtype), np.asarray(d).astype(dtype)
    out = np.full(xt.size, np.inf)
    with np.errstate(all="ignore"):
        if lo > -np.inf:
            sel = dt < 0
            t2 = T(lo) - xt[sel]
            out[sel] = np.where(t2 >= 0, T(0), t2 / dt[sel]).astype(np.float64)
        if hi < np.inf:
            sel = dt > 0
            t2 = T(hi) - xt[sel]
            out[sel] = np.where(t2 <= 0, T(0), t2 / dt[sel]).astype(np.float64)
    return out


def neg_ratio(x, d, lo, hi, dtype, where=None):
    """result[nw + 3]: -(smallest ratio), -inf when nothing limits the step."""
    r = step_ratio(x, d, lo, hi, dtype)
    if where is not None:
        r = r[where]
    return -float(r.min()) if r.size else -np.inf


def block_sums(terms, width, grid):
    """What the workgroups of a reduction leave in ws: vector j belongs to workgroup
    (j / 256) mod grid."""
    per = terms.reshape(-1, width).sum(axis=1)
    return np.bincount((np.arange(per.size) // KBLOCK) % grid, weights=per, minlength=grid)


def step_ref(w, wcoef, r, rcoef, xcp, x, g, mask, scale, lo, hi, dtype, mistake=None,
             grid_cap=DEFAULT_GRID):
    """nsol_lb_subspace_step_* (r given) / nsol_lb_subspace_step_r_* (r None: formed from
    RB3 and rcoef).  Dict of xn, d, S (of xn), C, and the result row: hits, dd, gd, wd [nw],
    nratio; also dsub (before the clip) and free."""
    n, nw, width = xcp.size, len(w), vw(dtype)
    free = _free(mask, n, mistake)
    wc, skip = _w_coefs(wcoef, dtype, mistake)
    if r is None:
        rb = [rnd(c, dtype) for c in RB3]
        rs, ra = _lincomb(rb + [rnd(c, dtype) for c in rcoef], [xcp, x, g] + list(w), n)
        rs, ra = np.where(free, rs, 0.0), np.where(free, ra, 0.0)
        count = 2 * nw + 6
    else:
        rs, ra = r, np.abs(r)
        count = nw + 4
    sw, aw = _lincomb(wc, w, n, skip)
    sc = rnd(scale, dtype)
    dsub = sc * sw + rs if mistake == "scale_first" else sc * (rs + sw)
    S = np.abs(xcp) + abs(sc) * (ra + aw)
    v = xcp + dsub
    tlo, thi = rnd(lo, dtype), rnd(hi, dtype)
    if mistake == "clip_swapped":
        tlo, thi = thi, tlo
    v = np.minimum(np.maximum(v, tlo), thi)
    xn = np.where(free, v, xcp)
    d = xn - (xcp if mistake == "d_from_xcp" else x)
    seen = _visited(n, width, mistake)
    at = free & ((xn == tlo) | (xn == thi)) & seen
    out = {"free": free, "dsub": dsub, "S": np.where(free, S, np.abs(xcp)), "C": count,
           "xn": np.where(seen, xn, FILL), "d": np.where(seen, d, FILL)}
    out.update(step_row(w, out["xn"], out["d"], x, g, free, lo, hi, dtype, mistake,
                        grid_cap))
    out["hits"] = float(at.sum())
    return out


def step_row(w, xn, d, x, g, free, lo, hi, dtype, mistake=None, grid_cap=DEFAULT_GRID):
    """The sums and the ratio of the result row from given xn and d (the reference's, or
    what the kernel stored): hits, dd, gd, wd, nratio, and the sums of magnitudes."""
    n, nw, width = d.size, len(w), vw(dtype)
    seen = _visited(n, width, mistake)
    ds = np.where(seen, d, 0.0)
    tlo, thi = rnd(lo, dtype), rnd(hi, dtype)
    where = seen & free if mistake == "ratio_free_only" else seen
    nratio = neg_ratio(x, ds, lo, hi, dtype, where)
    if mistake == "ratio_other_slot":
        # the NV = 12 form keeps its ratio partials behind 15 rows of ws, the NV = 24 form
        # behind 27: row 27 is never written when NV = 12 (it holds what ws held before),
        # row 15 holds the workgroups' partial sums of w[9]'d when NV = 24
        if nw <= 12:
            nratio = WS_FILL
        else:
            nratio = float(block_sums(w[9] * ds, width, rgrid(n // width, grid_cap)).max())
    return {
        "hits": float((free & seen & ((xn == tlo) | (xn == thi))).sum()),
        "dd": _sum(ds * ds), "gd": _sum(ds * g), "wd": np.array([_sum(wk * ds) for wk in w]),
        "nratio": nratio,
        "dd_abs": float(np.sum(ds * ds)), "gd_abs": float(np.sum(np.abs(ds * g))),
        "wd_abs": np.array([float(np.sum(np.abs(wk * ds))) for wk in w]),
    }


FSUM_BELOW = 1 << 17


def _sum(terms):
    """The exact sum rounded once (math.fsum); for the long lattice cases NumPy's sum,
    which is exact there because every partial sum is (the module's docstring)."""
    if terms.size < FSUM_BELOW:
        return math.fsum(terms.tolist())
    return float(np.sum(terms))


def mdot_ref(a, b, mask, dtype, mistake=None):
    """(sum over the free variables of a * b, sum of the magnitudes)."""
    keep = _free(mask, a.size, mistake) & _visited(a.size, vw(dtype), mistake)
    t = a[keep] * b[keep]
    return _sum(t), float(np.sum(np.abs(t)))


def mdots_ref(vecs, y, mask, dtype, mistake=None):
    """The result row of nsol_lb_mdots_* (nvec doubles; RES_FILL where nothing is written)
    and the sums of magnitudes."""
    nvec = len(vecs)
    sums = [mdot_ref(v, y, mask, dtype, mistake) for v in vecs]
    row = np.full(nvec, RES_FILL)
    for b in range(0, nvec, DOTS_PER_LAUNCH):
        cnt = min(DOTS_PER_LAUNCH, nvec - b)
        at = 0 if mistake == "second_launch" else b
        row[at:at + cnt] = [s for s, _ in sums[b:b + cnt]]
    return row, np.array([m for _, m in sums])


def diff_dots_ref(a, b, c, dtype, mistake=None):
    """nsol_lb_diff_dots_*: out = a - b in T arithmetic (one rounding), result = (sum
    out^2, sum out * c or 0); and the sums of magnitudes."""
    out = (a.astype(dtype) - b.astype(dtype)).astype(np.float64)
    seen = _visited(a.size, vw(dtype), mistake)
    o = np.where(seen, out, 0.0)
    res = [_sum(o * o), _sum(o * c) if c is not None else 0.0]
    mag = [float(np.sum(o * o)), float(np.sum(np.abs(o * c))) if c is not None else 0.0]
    return np.where(seen, out, FILL), res, mag


def projgr_ref(x, g, lo, hi, dtype, mistake=None):
    """max |projected gradient| in T arithmetic: g < 0: max(x - hi, g) if hi is finite;
    else (g >= 0, -0.0 included): min(x - lo, g) if lo is finite."""
    T = np.dtype(dtype).type
    xt, gt = x.astype(dtype), g.astype(dtype)
    gi = gt.copy()
    neg = gt < 0
    if hi < np.inf:
        gi[neg] = np.maximum(xt[neg] - T(hi), gt[neg])
    if lo > -np.inf:
        gi[~neg] = np.minimum(xt[~neg] - T(lo), gt[~neg])
    gi = gi[_visited(x.size, vw(dtype), mistake)]
    return float(np.max(np.abs(gi.astype(np.float64)))) if gi.size else 0.0


def count_free_ref(mask, mistake=None):
    keep = _free(mask, mask.size, mistake) & _visited(mask.size, 16, mistake)
    return float(keep.sum())


# ---- lengths and counts --------------------------------------------------------------
SMALL_NV = (1, 255, 256, 257)
TRIPS_NV = 2 * KBLOCK * 2 + 37       # max_grid_blocks = 2: two trips and part of a third
FINAL_NV = KBLOCK * 257 + 3          # 258 partial sums: k_final's own loop runs twice
CAP_NV = KRED * KBLOCK + 5           # rgrid's cap of 1024 workgroups crossed
WCOMB_NBASE = (0, 1, 2, 3)
WCOMB_NW = (0, 1, 3, 4, 5, 8, 39, 40)
MDOTS_NVEC = (1, 12, 13, 24, 25, 49)
STEP_NW = (1, 2, 11, 12, 13, 23, 24)
BIG_NW = 24                          # stored vectors at the two largest lengths


def vector_form(n, dtype):
    return n % vw(dtype) == 0


def small_lengths(dtype, width=None):
    """1, 255, 256, 257 vectors and the same plus 1, 2, 3 elements."""
    width = width or vw(dtype)
    return sorted({nv * width + e for nv in SMALL_NV for e in range(4)})


def long_lengths(dtype, width=None):
    """[(n, max_grid_blocks or None)]: the trips length (vector and scalar forms) with two
    workgroups, then the two largest once, and the scalar form across the cap."""
    width = width or vw(dtype)
    return [(TRIPS_NV * width, 2), (TRIPS_NV * width + 1, 2), (TRIPS_NV * width + 3, 2),
            (FINAL_NV * width, None), (FINAL_NV * width + 1, None), (CAP_NV * width, None)]


def wcomb_cases(dtype):
    """[(n, nbase, nw, masked, grid cap)]"""
    out = [(n, nb, nw, True, None) for n in small_lengths(dtype) for nb in WCOMB_NBASE
           for nw in WCOMB_NW]
    out += [(n, 3, 5, False, None) for n in small_lengths(dtype)]
    out += [(n, 3, BIG_NW, True, cap) for n, cap in long_lengths(dtype)]
    return out


def clip_cases(dtype):
    """[(n, nw, grid cap)] of nsol_lincomb_clip_* (nw >= 1)"""
    out = [(n, nw, None) for n in small_lengths(dtype) for nw in WCOMB_NW if nw]
    return out + [(n, BIG_NW, cap) for n, cap in long_lengths(dtype)]


def step_cases(dtype):
    """[(n, nw, grid cap)] of both subspace-step forms; a length that is no multiple of
    16 bytes must be declined."""
    out = [(n, nw, None) for n in small_lengths(dtype) for nw in STEP_NW]
    return out + [(n, BIG_NW, cap) for n, cap in long_lengths(dtype)]


def mdots_cases(dtype):
    out = [(n, nv, None) for n in small_lengths(dtype) for nv in MDOTS_NVEC]
    return out + [(n, BIG_NW, cap) for n, cap in long_lengths(dtype)]


def plain_cases(dtype, width=None):
    """[(n, grid cap)] of the kernels without a count (mdot, diff_dots, projgr,
    count_free with width 16)."""
    return [(n, None) for n in small_lengths(dtype, width)] + long_lengths(dtype, width)


# ---- the lattice cases' inputs and expected values -----------------------------------
def wcomb_args(n, nbase, nw):
    L = lattice(n)
    return ([L.xcp, L.x, L.g][:nbase], list(BCOEF[:nbase]), [L.w(k) for k in range(nw)],
            comb_coefs(nw))


def step_args(n, nw):
    L = lattice(n)
    wc, rc = step_coefs(nw)
    return [L.w(k) for k in range(nw)], wc, rc


def step_expected(n, nw, dtype, rin, mistake=None, grid_cap=None, masked=True, lo=LO, hi=HI):
    L = lattice(n)
    w, wc, rc = step_args(n, nw)
    return step_ref(w, wc, None if rin else L.r, rc, L.xcp, L.x, L.g,
                    L.mask if masked else None, STEP_SCALE, lo, hi, dtype, mistake,
                    grid_cap or DEFAULT_GRID)


def shares(ref, xcp, lo=LO, hi=HI):
    """Of the free variables: the shares that end strictly inside the box, at lo and at
    hi, and how many end exactly at a bound without being clipped."""
    f = ref["free"]
    xn, pre = ref["xn"][f], (xcp + ref["dsub"])[f]
    k = float(max(int(f.sum()), 1))
    return {"inside": ((xn > lo) & (xn < hi)).sum() / k, "at_lo": (xn == lo).sum() / k,
            "at_hi": (xn == hi).sum() / k,
            "unclipped": int(((pre == lo) | (pre == hi)).sum())}
