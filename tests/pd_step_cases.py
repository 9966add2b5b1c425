"""States, scalars, derived error bounds, the shape catalogue and a mirror of the launch
path's form choice for the tests of the one-iteration primal-dual kernels: k_dual_step,
k_primal_step, k_pd_fused (csrc/nsol_pd.hip, nsol_pd_fused_body.hpp) and k_dual_step_iso,
k_pd_fused_iso (csrc/nsol_pdi.hip, nsol_pd_iso_body.hpp).  test_pd_steps_host.py checks
all of this on the CPU, test_pd_steps_gpu.py uses it.

States are random values rounded to the kernel's element type and held in float64,
read-only.  The two TIE states sit exactly on the branches in either type: every scalar
that matters there is dyadic and every value a multiple of 1/64 (or a planted neighbour
of a branch point), so that each float32 operation is exact and the results must be equal.

Float32 gate, per element:  |got - want| <= R * 2^-24 * S_i, the rule of vector_cases.py:
R counts the rounded float32 operations (a divide or a square root counts 3), S_i sums the
magnitudes of the terms.  Written down from the source before any kernel ran against it:

dual step, one component (dual_update, nsol_pd_common.hpp; dual_q, nsol_pd_iso_body.hpp):
    q = p + sigma * (hi * w + lo * (-w))        hi w, lo (-w), +, sigma *, p + : 5
    Huber, float32: q * float32(1 / hden)       (huber_div, nsol_common.hpp)   : 1 more
    S = (|p| + |sigma| (|hi| + |lo|) |w|) [* 1 / hden]
  dual_clamp (nsol_common.hpp) is a median of three: no rounding, and 1-Lipschitz, so the
  bound of q is the bound of p_new: R = 5 (TV), 6 (Huber).
isotropic projection (dual_project, nsol_pd_iso_body.hpp), d components:
    s = ((q0 q0) + q1 q1) + q2 q2               d products, d - 1 sums
    m = max(1, sqrt(s)),  p_a = q_a / m         sqrt 3, divide 3              : 2 d + 5
  against |p_a| <= |q_a|.  The projection onto the unit ball is 1-Lipschitz in the
  voxel's EUCLIDEAN norm -- not component by component -- so what q carries in reaches
  p_new as a vector: the bound is on the voxel's vector error,
    |got - want|_2 <= (R_q + 2 d + 5) * 2^-24 * |S|_2,   S the vector of the S above
  (|p|_2 <= |q|_2 <= |S|_2 lets the two parts share one S).
primal step (k_primal_step, nsol_pd.hip; the same lines in both tile bodies):
    kt = sum_a p_a (-w_a) + p_a[i - e_a] w_a    3 per axis, d - 1 sums        : 4 d - 1
    u = x - tau * kt                                                          : 2
    l2 (prox_ell2, nsol_common.hpp): (u + tl bt) * float32(1 / (1 + tl))      : 3
    l1 (prox_ell1): d = u - bt, |d| - tl, bt + (max and sign are exact)       : 3
    S_u = |x| + |tau| sum_a (|p_a| + |p_a[i - e_a]|) |w_a|
    x_new:  R = 4 d + 4,  S = (S_u + |tl bt|) / (1 + tl)  (l2),  S_u + 2 |bt| + tl  (l1)
  both proxes are 1-Lipschitz in u.
    xbar_new = x_new + theta * (x_new - x)      -, theta *, +                 : 3
  carries x_new's error (1 + |theta|) times, and |x_new| <= S:
    xbar_new:  R = 4 d + 7,  S = (1 + |theta|) S_x + |theta| |x|
The dual and the primal step are bounded separately: the primal outputs of any call are
compared with pd_primal_step applied to the call's OWN p_out, so that no dual error is
propagated into the primal bound.

The WGT and LIN forms of the two tile bodies (k_pd_w, nsol_pdw.hip; k_pd_lin, nsol_pdl.hip;
k_pdl_stack, nsol_pdls.hip) and the element-wise kernels beside them, counted from the
source in the same way before any of them ran against these gates.  The dual half is the
plain kernels'.  kt (4 d - 1) and S_u are as above:
LIN (lin_step, nsol_pd_fused_body.hpp):
    u = x - tau * (kt + g)                      kt + g, tau *, x -             : 3
    c = u < lo ? lo : u;  c > hi ? hi : c       selects: exact, 1-Lipschitz in u
    x_new:  R = 4 d + 2,  S = |x| + |tau| (sum_a (|p_a| + |p_a[i - e_a]|) |w_a| + |g|)
  on the box the kernel itself uses (box_in), so the clip adds nothing.  Where u lies outside
  the box by more than R u S the kernel's u lies outside it too and x_new is the bound
  itself: R = 0 there, the bits of box_in's lo or hi.  A clipped x_new may be larger than S
  (u = -0.1, lo = 0.5), so xbar_new's S takes max(S, |x_new|) for S_x.
WGT (prox_data_w, nsol_pd_weighted.hpp), u = x - tau * kt as above (4 d + 1):
    t = tl * w                                                                 : 1
    l2: (u + t * bt) / (1 + t)                  t bt, u +, 1 +, divide 3       : 6
    l1: d = u - bt, |d| - t, bt +                                              : 3
    x_new:  R = 4 d + 8,  S = (S_u + |t bt|) / (1 + t)     (l2)
            R = 4 d + 5,  S = S_u + 2 |bt| + t             (l1)
            R = 4 d + 1,  S = S_u                          (w == 0: u itself)
    xbar_new: 3 more, as above.
k_prox_w (nsol_pdw.hip) is prox_data_w on a given u: R = 7 (l2), 4 (l1), and w == 0 hands u
  back: R = 0, the bits of u.
k_pdl_dual_data (nsol_pdl.hip) and its stacked twin (nsol_pdls.hip):
    v = q + sigma * (t - bt)                    -, sigma *, q +                : 3
        q - sigma * bt            (t NULL)      sigma *, q -                   : 2
    c = lmbda * w                               (wt NULL: lmbda * 1, exact)    : 1 / 0
    l2: (v * c) / (c + sigma)                   v c, c +, divide 3             : 5
    l1: v < -c ? -c : v;  r > c ? c : r         selects: exact, 1-Lipschitz in v
    S_v = |q| + |sigma| (|t| + |bt|)
    l2:  R = R_v + R_c + 5,  S = S_v c / (c + sigma)
    l1:  R = R_v + R_c,      S = S_v + c     (what comes out is v or +-c, c one rounding)
    w == 0: +0 exactly.
"""
import collections
import functools

import numpy as np

from nsol_amd import vector_numpy as vn
from vector_cases import U32, U64, unit, c, rounded, plant     # noqa: F401

SIGMA, TAU, TL, THETA = 0.3, 0.4, 0.5, 0.9
HUBER_GAMMA = 0.05
HDEN = 1. + SIGMA * HUBER_GAMMA
SPACING = (0.8, 1.3, 2.0)           # spacing[0] belongs to the last array axis
P_SCALE = 0.7
Scalars = collections.namedtuple("Scalars", "sigma hden tau tl theta")
RANDOM = Scalars(SIGMA, HDEN, TAU, TL, THETA)
TIE = Scalars(0.25, 1.0, 0.5, 0.5, 1.0)      # (hden = 1: the tie states are TV)
MAX_VOXELS = 100000
# the cases of the catalogue whose shapes carry the tie states (two tiles along x, room
# for every planted value in every component)
TIE_CASES = ("rag16-3d-ry2", "vec64-2d-ry1", "elem64-3d-ry1", "unit-1d", "unit-3d")
BRANCH_MIN_VOXELS = 250

BOTH = [np.float64, np.float32]


def is64(dtype):
    return np.dtype(dtype) == np.float64


def suffix(dtype):
    return "f64" if is64(dtype) else "f32"


def vw(dtype):
    """Elements per 16-byte access."""
    return 16 // np.dtype(dtype).itemsize


def dims3(shape):
    """(ndim, nz, ny, nx) as the C ABI takes them."""
    return (len(shape),) + (1,) * (3 - len(shape)) + tuple(shape)


def weights(shape, unit_spacing=False):
    """(wx, wy, wz) = 1 / h, 1 on the axes the volume does not have."""
    d = len(shape)
    return tuple(1. if unit_spacing or a >= d else 1. / SPACING[a] for a in range(3))


def zyx(index, shape):
    """An index into a volume of up to three axes as (z, y, x)."""
    index = tuple(int(i) for i in index)
    return (0,) * (3 - len(shape)) + index


# ------------------------------------------------------------------------- states
def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def state(shape, dtype):
    """The random state of a shape: xbar, x, bt ~ N(0, 1), p ~ 0.7 N(0, 1)."""
    d = len(shape)
    rng = np.random.default_rng(5100 + 7 * sum(shape) + 31 * d + np.dtype(dtype).itemsize)
    r = lambda scale, *s: rounded(scale * rng.standard_normal(s), dtype)
    return _frozen(dict(xbar=r(1., *shape), x=r(1., *shape), bt=r(1., *shape),
                        p=r(P_SCALE, d, *shape)))


def _grid(rng, *shape):
    """Multiples of 1/64 in [-2, 2]: sums and differences of a few of them, and their
    products with 0.25, 0.5 and 1, are exact in float32."""
    return rng.integers(-128, 129, shape).astype(np.float64) / 64.


def tie_values(dtype):
    """p_in on, beside and far from |q| == 1, and both zeros."""
    t = np.dtype(dtype).type
    up = lambda v: float(np.nextafter(t(v), t(np.inf)))
    dn = lambda v: float(np.nextafter(t(v), t(-np.inf)))
    return [1., -1., up(1.), dn(1.), up(-1.), dn(-1.), 0., -0., 2.5]


def _plant_sites(n, seam, k, d, a):
    """Flat voxels of component a's k planted values: the first voxels, the voxels from
    the first tile seam on, the last voxels -- interleaved so that no voxel is planted
    in two components."""
    step = a + d * np.arange(k)
    sites = [step]
    if seam is not None:
        sites.append(seam + step)
    sites.append(n - d * k + step)
    return sites


@functools.lru_cache(maxsize=None)
def dual_tie_state(shape, dtype, seam):
    """xbar = 0, so q = p_in exactly (sigma = 0.25, unit spacing, TV).  Every voxel has
    ONE nonzero component -- sqrt(fl(q q)) == |q| in IEEE arithmetic, so the isotropic
    projection is as exact there as the clamp -- and tie_values() is planted in every
    component.  seam: flat index of the first voxel of the second tile along x, or None."""
    d, n = len(shape), int(np.prod(shape))
    rng = np.random.default_rng(6100 + 7 * sum(shape) + d)
    p = _grid(rng, d, n)
    p[np.arange(n)[None, :] % d != np.arange(d)[:, None]] = 0.
    vals = np.array(tie_values(dtype))
    taken = np.zeros(n, dtype=bool)
    for a in range(d):
        for sites in _plant_sites(n, seam, vals.size, d, a):
            ok = (sites >= 0) & (sites < n)
            ok[ok] &= ~taken[sites[ok]]
            p[:, sites[ok]] = 0.
            p[a, sites[ok]] = vals[ok]
            taken[sites[ok]] = True
    z = np.zeros(shape)
    return _frozen(dict(xbar=z, x=_grid(rng, *shape), bt=_grid(rng, *shape),
                        p=p.reshape((d,) + shape)))


@functools.lru_cache(maxsize=None)
def primal_tie_state(shape, dtype, seam):
    """xbar = 0 and p_in NULL: p_new = 0, kt = 0 and u = x exactly.  x - bt is planted
    on |u - bt| == tl from both sides, on u == bt and one ulp inside and outside, as
    vector_cases.inputs("prox_ell1", ...) does -- at the first voxels, from the tile seam
    on and, reversed, at the last voxels.  (l1 only: the reciprocal of the l2 prox is not
    dyadic.)"""
    n = int(np.prod(shape))
    t = np.dtype(dtype).type
    up = lambda v: float(np.nextafter(t(v), t(np.inf)))
    dn = lambda v: float(np.nextafter(t(v), t(-np.inf)))
    rng = np.random.default_rng(6200 + 7 * sum(shape) + len(shape))
    x, bt = _grid(rng, n), _grid(rng, n)
    bts = [0.25] * 6
    us = [0.75, -0.25, 0.25, up(0.75), dn(0.75), dn(-0.5) + 0.25]
    plant(bt, bts)
    plant(x, us)
    if seam is not None and seam + len(us) <= n - len(us):
        bt[seam:seam + len(us)] = bts
        x[seam:seam + len(us)] = us
    return _frozen(dict(xbar=np.zeros(shape), x=x.reshape(shape), bt=bt.reshape(shape),
                        p=np.zeros((len(shape),) + shape)))


# --------------------------------------------------------------- want, R and S
def _abs_pair(u, axis, forward):
    a = np.abs(u)
    return a + vn.shifted(a, axis, forward)


def dual_expected(st, sc, w, dtype, huber, iso, has_p):
    """(want, R, S) of the dual step on the state st: want and S of shape (d,) + volume;
    isotropic: S per VOXEL, the bound of the Euclidean norm of the voxel's error."""
    xbar, p = st["xbar"], st["p"] if has_p else None
    d = xbar.ndim
    hden = sc.hden if huber else 1.0
    want = vn.pd_dual_step(xbar, p, sc.sigma, hden, w, dtype, iso)
    sg = abs(c(sc.sigma, dtype))
    S = np.stack([(np.abs(p[a]) if has_p else 0.)
                  + sg * _abs_pair(xbar, d - 1 - a, True) * abs(c(w[a], dtype))
                  for a in range(d)])
    R = 5
    if huber:
        R, S = R + 1, S * c(1. / hden, dtype)
    if iso:
        R, S = R + 2 * d + 5, np.sqrt(np.sum(S * S, axis=0))
    return want, R, S


def primal_expected(p, st, sc, w, dtype, l1):
    """((x_new, R, S), (xbar_new, R, S)) of the primal step on the dual field p."""
    x, bt = st["x"], st["bt"]
    d = x.ndim
    x_new, xbar_new = vn.pd_primal_step(p, x, bt, sc.tau, sc.tl, sc.theta, w, l1, dtype)
    S_u = np.abs(x) + abs(c(sc.tau, dtype)) * sum(
        _abs_pair(p[a], d - 1 - a, False) * abs(c(w[a], dtype)) for a in range(d))
    if l1:
        S_x = S_u + 2. * np.abs(bt) + c(sc.tl, dtype)
    else:
        S_x = (S_u + np.abs(c(sc.tl, dtype) * bt)) / (1. + sc.tl)
    th = abs(c(sc.theta, dtype))
    return ((x_new, 4 * d + 4, S_x),
            (xbar_new, 4 * d + 7, (1. + th) * S_x + th * np.abs(x)))


def excess(got, want, R, S, dtype, exact=False, vector=False):
    """(bad, worst): the elements outside the gate and the largest err / bound (float32
    only).  float64, exact and R zero everywhere: bad = not equal.  vector: got, want of shape
    (d,) + volume are judged per voxel, by the Euclidean norm of the difference."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    if is64(dtype) or exact or not np.any(R):
        # bit for bit: the sign of a zero counts
        bad = (got != want) | ~np.isfinite(got) | (np.signbit(got) != np.signbit(want))
        if vector:
            bad = np.any(bad, axis=0)
        return bad, 0.
    err = np.abs(got - want)
    if vector:
        err = np.sqrt(np.sum(err * err, axis=0))
    bound = R * U32 * S
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.))
    ratio = np.where(np.isfinite(err), ratio, np.inf)
    return ~(err <= bound), float(np.max(ratio)) if ratio.size else 0.


def judge(got, st, sc, w, dtype, huber, l1, iso, has_p, exact=False, which="pxb",
          primal=None):
    """The outputs (p, x, xbar) of one iteration against the restatement: p against
    pd_dual_step, x and xbar against pd_primal_step of the call's own p.  Returns
    [(array name, bad, worst ratio)]; which: the letters of the outputs to judge.
    primal: p -> ((x_new, R, S), (xbar_new, R, S)) of another primal half (weighted_expected,
    lin_expected) in pd_primal_step's place."""
    out = []
    p = np.asarray(got[0], np.float64)
    if "p" in which:
        want, R, S = dual_expected(st, sc, w, dtype, huber, iso, has_p)
        out.append(("p_out",) + excess(p, want, R, S, dtype, exact, vector=iso))
    if "x" in which or "b" in which:
        ex, eb = (primal_expected(p, st, sc, w, dtype, l1) if primal is None
                  else primal(p))
        if "x" in which:
            out.append(("x",) + excess(got[1], ex[0], ex[1], ex[2], dtype, exact))
        if "b" in which:
            out.append(("xbar_out",) + excess(got[2], eb[0], eb[1], eb[2], dtype, exact))
    return out


def first_bad(bad, shape):
    """'(z, y, x)' of the first failing element, with the component of a dual field."""
    i = np.argwhere(bad)[0]
    if bad.ndim > len(shape):
        return "component %d at (z, y, x) = %r" % (i[0], zyx(i[1:], shape))
    return "(z, y, x) = %r" % (zyx(i, shape),)


# ------------------------------------------------------- the launch path's choice
Form = collections.namedtuple("Form", "kind LX RY NDIM ntx nty nzc slab")
Plan = collections.namedtuple("Plan", "form TX TY zchunk")
K_WAVE, K_BLOCK = 64, 256


def _ceil(a, b):
    return -(-a // b)


def plan(shape, dtype, offset=0, ry=0, rag=1, zchunk=0, iso=False, xcd_map=1, members=1):
    """What pd_launch, FusedKernel::launch / IsoKernel::launch, pd_auto_rows_per_lane and
    pd_plan_grid (nsol_pd_launch.hpp, nsol_pd.hip, nsol_pdi.hip) make of a single volume
    whose arrays all start `offset` elements behind a 16-byte boundary, under the knobs
    pd_ry, pd_rag, pd_zchunk.  members: the volumes of a stacked launch; they count as tiles
    in the automatic rows per lane and in the automatic z chunk.  The stacked, the weighted
    and the linear launchers (pd_launch_forms) have one or two rows per lane and take no
    knobs (kPdStackTune): that is ry = 0, rag = 1, zchunk = 0 here, where iso makes no
    difference."""
    VW = vw(dtype)
    ndim, nz, ny, nx = dims3(shape)
    n = nz * ny * nx
    aligned = (offset * np.dtype(dtype).itemsize) % 16 == 0
    if nx % VW == 0 and aligned and n % VW == 0:
        kind, VEC, LX = "vec", VW, 64 if nx // VW >= K_WAVE else 16
    elif rag and nx >= 2 * VW:
        kind, VEC, LX = "rag", VW, 64 if _ceil(nx, VW) >= K_WAVE else 16
    else:
        kind, VEC, LX = "elem", 1, 64 if nx >= K_WAVE else 16
    TX, LY = LX * VEC, K_WAVE // LX
    auto = lambda: 1 if (_ceil(nx, TX) * _ceil(ny, (K_BLOCK // K_WAVE) * LY * 2) * members
                         * ((nz + 1) // 2) < 512) else 2
    if iso:
        RY = ry if ry in (1, 2) else auto()
    else:
        RY = ry if ry != 0 else auto()
        if RY == 4 and kind == "rag":
            RY = 2
        elif RY not in (1, 4):
            RY = 2
    if ndim == 1:
        RY = 1
    TY = (K_BLOCK // K_WAVE) * LY * RY
    ntx, nty = _ceil(nx, TX), _ceil(ny, TY)
    zc = zchunk
    if zc <= 0:
        zc = max(2, _ceil(nz, _ceil(4096, ntx * nty * members)))
    zc = min(zc, nz)
    slab = _ceil(nty, 8) if xcd_map and nty >= 16 else 0
    return Plan(Form(kind, LX, RY, ndim, ntx, nty, _ceil(nz, zc), slab), TX, TY, zc)


def form(shape, dtype, offset=0, ry=0, rag=1, zchunk=0, iso=False):
    return plan(shape, dtype, offset, ry, rag, zchunk, iso).form


def blocks(f):
    """Workgroups of the launch and how many of them have a tile."""
    tiles = f.ntx * f.nty * f.nzc
    return (8 * f.slab * f.ntx * f.nzc if f.slab else tiles), tiles


# ------------------------------------------------------------------ the catalogue
Case = collections.namedtuple("Case", "name shape unit ry rag zchunk offset")


def case_plan(case, dtype, iso):
    return plan(case.shape, dtype, case.offset, case.ry, case.rag, case.zchunk, iso)


def case_weights(case):
    return weights(case.shape, case.unit)


@functools.lru_cache(maxsize=None)
def catalogue(dtype):
    """One case per form (kind, LX, RY, NDIM) with two tiles along x and along y whose
    last one is partial and, in 3-D, two z chunks with a shorter last one; then the
    cases the forms do not ask for by themselves.  The same list serves the anisotropic
    and the isotropic kernel (pd_ry = 4 means `choose` to the latter)."""
    VW = vw(dtype)
    cases = []

    def add(name, shape, unit=False, ry=0, rag=1, zchunk=0, offset=0):
        if zchunk == "nz":
            zchunk = dims3(shape)[1]
        cases.append(Case(name, tuple(shape), unit, ry, rag, zchunk, offset))

    for kind in ("vec", "rag", "elem"):
        for LX in (64, 16):
            TX = LX * (1 if kind == "elem" else VW)
            # vec: whole vectors, one more than a tile; rag: one element more than that
            # (the last vector has 1 valid element); elem (pd_rag = 0): 3 more than a tile
            nx = TX + {"vec": VW, "rag": VW + 1, "elem": 3}[kind]
            for ndim in (1, 2, 3):
                rys = (0,) if ndim == 1 else ((1, 2) if kind == "rag" else (1, 2, 4))
                for ry in rys:
                    TY = 4 * (64 // LX) * max(ry, 1)
                    ny = TY + max(1, ry - 1)     # RY 4: three of the lane's four rows
                    shape = ((nx,), (ny, nx), (3, ny, nx))[ndim - 1]
                    add("%s%d-%dd-ry%d" % (kind, LX, ndim, ry), shape, ry=ry,
                        rag=0 if kind == "elem" else 1)
    # unit spacing, one per dimension (the shapes of the branch shares)
    add("unit-1d", (259,), unit=True)
    add("unit-2d", (6, 259), unit=True)
    add("unit-3d", (4, 6, 259), unit=True)
    add("small-3d", (3, 5, 7))
    add("spaced-3d", (4, 6, 259))
    # every plane recomputes pzprev; one chunk; one plane in 3-D
    add("zchunk1", (5, 9, 16 * VW + VW + 1), zchunk=1)
    add("one-chunk", (5, 9, 16 * VW + VW), zchunk="nz")
    add("nz1-3d", (1, 9, 16 * VW + VW + 1))
    # ragged rows whose last vector has 2 and 3 valid elements (float32), and
    # ceil(nx / VW) == 64 exactly: the first row length that takes 64 lanes
    tail = lambda k: k if VW == 4 else 1         # (float64: a vector is two elements)
    add("rag-2-valid", (3, 5, 64 * VW + VW + tail(2)))
    add("rag-3-valid", (2, 5, 64 * VW + VW + tail(3)))
    add("rag16-2-valid", (2, 9, 16 * VW + tail(2)), ry=2)
    add("rag16-3-valid", (9, 16 * VW + tail(3)), ry=1)
    add("rag-64-vectors", (2, 3, 64 * VW - VW + 1))
    # extents of 1 on every axis
    add("ones", (1, 1, 1))
    add("one-1d", (1,))
    add("nx1-2d", (7, 1))
    add("ny1-2d", (1, 7))
    add("ny1-3d", (3, 1, 9))
    add("nx1-3d", (3, 9, 1))
    # nty = 17 >= 16: the XCD slab map, 24 block rows for 17 tile rows
    add("slab", (3, 67, 64 * VW + VW), ry=1)
    # arrays off 16-byte alignment: whole-vector shapes fall to the ragged form, or to
    # single elements with pd_rag = 0
    add("off1-3d", (3, 9, 16 * VW + VW), offset=1, ry=2)
    add("off3-3d", (2, 5, 64 * VW + VW), offset=3)
    add("off1-elem64", (3, 5, 67), offset=1, rag=0)
    add("off3-1d", (259,), offset=3)
    add("off1-2d", (6, 259), offset=1, ry=2)
    # the automatic choice of two rows per lane: 2 x tiles, 256 pairs of planes
    add("auto-ry2", (511, 1, 17), rag=0)
    for cs in cases:
        assert int(np.prod(cs.shape)) <= MAX_VOXELS, cs
    assert len({cs.name for cs in cases}) == len(cases)
    return tuple(cases)


def case_named(name, dtype):
    return [cs for cs in catalogue(dtype) if cs.name == name][0]


def seam_of(case, dtype, iso=False):
    """Flat index of the first voxel of the second tile along x (None: one tile)."""
    pl = case_plan(case, dtype, iso)
    return pl.TX if pl.form.ntx >= 2 else None


# ----------------------------------------------------------------- branch shares
def branch_shares(case, dtype, huber=False):
    """The share of the random state's components / voxels on the active side of each
    branch of one iteration with p_in given, from the restatement alone."""
    st, w = state(case.shape, dtype), case_weights(case)
    hden = HDEN if huber else 1.0
    q = vn.pd_dual_q(st["xbar"], st["p"], SIGMA, w, dtype) / hden
    out = {"clamped": np.mean(np.abs(q) > 1.),
           "outside the ball": np.mean(np.sum(q * q, axis=0) > 1.)}
    for iso in (False, True):
        p = vn.pd_dual_step(st["xbar"], st["p"], SIGMA, hden, w, dtype, iso)
        u = vn.grad_adj_axpy(p, st["x"], TAU, w, dtype)
        out["l1 shrunk onto bt (%s)" % ("iso" if iso else "aniso")] = np.mean(
            np.abs(u - st["bt"]) <= TL)
    return {k: float(v) for k, v in out.items()}


# =========================================================================================
# The WGT and LIN forms (k_pd_w, k_pd_lin, k_pdl_stack) and their element-wise kernels
# =========================================================================================
LMBDA = 1.25
# the weighted entry takes its scalars from a table row: tl = tau * lmbda, in double
WEIGHTED = Scalars(SIGMA, HDEN, TAU, TAU * LMBDA, THETA)
# neither bound is a float32, and float32(lo) < lo, float32(hi) > hi: rounded to nearest,
# both bounds of the float32 box would lie outside the caller's
BOX = (-0.46, 0.55)
BOXES = (BOX, (-0.46, np.inf), (-np.inf, 0.55), (-np.inf, np.inf))
DD_SIGMA, DD_LMBDA = 0.3, 1.7       # the element-wise dual update of the data term
SCase = collections.namedtuple("SCase", "name shape unit offset members")


def scase_plan(cs, dtype, members=None):
    """The plan of the launchers without knobs (kPdStackTune) for the case's stack, or for
    `members` of its volumes."""
    return plan(cs.shape, dtype, cs.offset, members=cs.members if members is None else members)


def scase_weights(cs):
    return weights(cs.shape, cs.unit)


@functools.lru_cache(maxsize=None)
def catalogue_stack(dtype):
    """Shapes (and member counts) that reach every form the launchers WITHOUT knobs have:
    (vec | rag) x (64 | 16 lanes) and single elements where nx < 2 VW (16 lanes only),
    1-D, 2-D and 3-D at one and two rows per lane, each with two tiles along x (not elem)
    and y whose last one is partial and two z chunks in 3-D.  Two rows per lane need
    tiles * members * ((nz + 1) / 2) >= 512, which no single volume under MAX_VOXELS has
    with 2 x 2 tiles: those cases are stacks.  Then the edges the forms do not ask for."""
    VW = vw(dtype)
    cases = []

    def add(name, shape, members=1, unit=False, offset=0):
        cases.append(SCase(name, tuple(shape), unit, offset, members))

    for kind in ("vec", "rag", "elem"):
        for LX in (64, 16) if kind != "elem" else (16,):
            TX = LX * (1 if kind == "elem" else VW)
            nx = {"vec": TX + VW, "rag": TX + VW + 1, "elem": 2 * VW - 1}[kind]
            ntx = 1 if kind == "elem" else 2
            TY1 = 4 * (64 // LX)
            add("%s%d-1d" % (kind, LX), (nx,))
            add("%s%d-2d-ry1" % (kind, LX), (TY1 + 1, nx))
            add("%s%d-2d-ry2" % (kind, LX), (2 * TY1 + 1, nx), members=512 // (2 * ntx))
            add("%s%d-3d-ry1" % (kind, LX), (3, TY1 + 1, nx))
            add("%s%d-3d-ry2" % (kind, LX), (3, 2 * TY1 + 1, nx), members=256 // (2 * ntx))
    # the stack switches the form: ragged rows, 16 lanes, one tile along x and two tile rows
    # of two rows per lane; 2 x 32 = 64 < 512 alone, 8 x 2 x 32 = 512 stacked (both types)
    add("switch-3d-alone", (64, 33, 17))
    add("switch-3d-stack", (64, 33, 17), members=8)
    add("switch-2d-alone", (33, 17))                # 2 tiles alone, 512 in 256 members
    add("switch-2d-stack", (33, 17), members=256)
    add("unit-1d", (259,), unit=True)
    add("unit-2d", (6, 259), unit=True)
    add("unit-3d", (4, 6, 259), unit=True)
    add("spaced-3d", (4, 6, 259))
    add("small-3d", (3, 5, 7))
    tail = lambda k: k if VW == 4 else 1         # (float64: a vector is two elements)
    add("rag-2-valid", (3, 5, 64 * VW + VW + tail(2)))
    add("rag-3-valid", (2, 5, 64 * VW + VW + tail(3)))
    add("rag16-2-valid", (2, 9, 16 * VW + tail(2)))
    add("rag16-3-valid", (9, 16 * VW + tail(3)))
    add("rag-64-vectors", (2, 3, 64 * VW - VW + 1))
    add("ones", (1, 1, 1))
    add("one-1d", (1,))
    add("nx1-2d", (7, 1))
    add("ny1-2d", (1, 7))
    add("ny1-3d", (3, 1, 9))
    add("nx1-3d", (3, 9, 1))
    add("ones-stack", (1, 1, 1), members=3)
    # nty = 17 >= 16: the XCD slab map, 24 block rows for 17 tile rows
    add("slab", (3, 67, 64 * VW + VW))
    # arrays off 16-byte alignment: whole-vector shapes fall to the ragged form
    add("off1-3d", (3, 9, 16 * VW + VW), offset=1)
    add("off3-3d", (2, 5, 64 * VW + VW), offset=3)
    add("off3-1d", (259,), offset=3)
    add("off1-2d", (6, 259), offset=1)
    add("off1-stack", (3, 9, 16 * VW + VW), offset=1, members=3)
    for cs in cases:
        assert int(np.prod(cs.shape)) <= MAX_VOXELS, cs
    assert len({cs.name for cs in cases}) == len(cases)
    return tuple(cases)


def scase_named(name, dtype):
    return [cs for cs in catalogue_stack(dtype) if cs.name == name][0]


# the cases that carry the tie states of the two forms and the other boxes
STACK_TIE_CASES = ("rag16-3d-ry1", "vec64-2d-ry1", "unit-1d", "unit-3d", "off1-3d")


# -------------------------------------------------------------------------- states
@functools.lru_cache(maxsize=None)
def member_state(shape, dtype, m=0):
    """state() for member m of a stack: member 0 is state() itself, the others differ."""
    if m == 0:
        return state(shape, dtype)
    d = len(shape)
    rng = np.random.default_rng([5100 + 7 * sum(shape) + 31 * d + np.dtype(dtype).itemsize, m])
    r = lambda scale, *s: rounded(scale * rng.standard_normal(s), dtype)
    return _frozen(dict(xbar=r(1., *shape), x=r(1., *shape), bt=r(1., *shape),
                        p=r(P_SCALE, d, *shape)))


@functools.lru_cache(maxsize=None)
def lin_state(shape, dtype, m=0):
    """member_state plus g ~ N(0, 1), the array in bt's place: u = x - tau (kt + g) has a
    standard deviation above 1, so about a third of it falls on either side of BOX."""
    st = dict(member_state(shape, dtype, m))
    rng = np.random.default_rng([5300 + 7 * sum(shape) + np.dtype(dtype).itemsize, m])
    st["g"] = rounded(rng.standard_normal(shape), dtype)
    return _frozen(st)


def _zero_weight_sites(shape):
    """Flat voxels whose weight is forced to zero: the two corners that lie on every face
    between them, and in the first and the last row both sides of every tile seam along
    x that a form can have (TX = 16, 32, 64, 128 or 256 elements)."""
    n, nx = int(np.prod(shape)), shape[-1]
    sites = {0, n - 1}
    for TX in (16, 32, 64, 128, 256):
        if nx > TX:
            sites |= {TX - 1, TX, n - nx + TX - 1, n - nx + TX}
    return np.array(sorted(sites))


@functools.lru_cache(maxsize=None)
def weights_state(shape, dtype, m=0):
    """member_state plus the weights wt: about 30 % exact zeros (the sites of
    _zero_weight_sites among them), 15 % exact ones, the rest in (0, 3]; and under three
    in four of the zeros bt holds NaN, +inf or -inf."""
    st = dict(member_state(shape, dtype, m))
    n = int(np.prod(shape))
    rng = np.random.default_rng([5400 + 7 * sum(shape) + np.dtype(dtype).itemsize, m])
    kind = rng.random(n)
    wt = np.where(kind < 0.3, 0., np.where(kind < 0.45, 1., 3. - 3. * rng.random(n)))
    wt[_zero_weight_sites(shape)] = 0.
    wt = rounded(wt, dtype)
    assert np.all(wt >= 0) and np.all(wt <= 3)
    bt = st["bt"].reshape(-1).copy()
    zeros = np.flatnonzero(wt == 0)
    for k, junk in enumerate((np.nan, np.inf, -np.inf)):
        bt[zeros[k::4]] = junk
    st["wt"], st["bt"] = wt.reshape(shape), bt.reshape(shape)
    return _frozen(st)


def _nb(dtype):
    t = np.dtype(dtype).type
    return (lambda v: float(np.nextafter(t(v), t(np.inf))),
            lambda v: float(np.nextafter(t(v), t(-np.inf))))


def _plant_rows(n, seam, k):
    """Where k planted values start: the first voxels, from the tile seam on, the last."""
    starts = [0, n - k]
    if seam is not None and k <= seam and seam + k <= n - k:
        starts.append(seam)
    return [s for s in starts if 0 <= s and s + k <= n]


LIN_TIE_BOXES = {"box": (-0.5, 0.75), "zero": (0., 0.75), "point": (0.375, 0.375)}


@functools.lru_cache(maxsize=None)
def lin_tie_state(shape, dtype, seam, kind):
    """xbar = 0 and has_p = 0: p_new = 0 and kt = +0 exactly, tau = 0.5, so u = x - g / 2
    with x, g on 1/64.  Planted (g = 0 there): u on lo, on hi and one ulp either side of
    each, u = -0.0 (which stays -0.0 on lo = 0), u = +0.0, far below and far above.
    kind: "box" [-0.5, 0.75], "zero" [0, 0.75], "point" lo == hi == 0.375
    (inside a binade: the mirror image of either neighbour is a number of the type)."""
    n = int(np.prod(shape))
    lo, hi = LIN_TIE_BOXES[kind]
    up, dn = _nb(dtype)
    rng = np.random.default_rng(6300 + 7 * sum(shape) + len(shape))
    x, g = _grid(rng, n), _grid(rng, n)
    us = [lo, hi, up(lo), dn(lo), up(hi), dn(hi), -0., 0., -2.5, 2.5]
    for s in _plant_rows(n, seam, len(us)):
        x[s:s + len(us)] = us
        g[s:s + len(us)] = 0.
    return _frozen(dict(xbar=np.zeros(shape), x=x.reshape(shape), g=g.reshape(shape),
                        bt=np.zeros(shape), p=np.zeros((len(shape),) + shape)))


def _l1_chain(T, u, bt, t):
    """x_new and xbar_new (theta = 1) of the l1 prox at u in the arithmetic of type T."""
    u, bt, t = T(u), T(bt), T(t)
    d = u - bt
    r = bt + np.maximum(np.abs(d) - t, T(0)) * np.sign(d)
    return float(r), float(r + (r - u))


def _l1_tie_pairs(dtype, t, bts=(0.25, -0.25, 0.5, 0.)):
    """(u, bt) with u - bt on +-t, one ulp either side of each, and on 0 -- for the first
    bt of bts at which u = bt + (u - bt) is a number of the type and no operation of the
    prox and of the extrapolation behind it rounds in the type (theta = 1 mirrors x at
    x_new, which next to a power of two need not be a number of the type)."""
    up, dn = _nb(dtype)
    T = np.dtype(dtype).type
    out = []
    for dv in (t, -t, up(t), dn(t), up(-t), dn(-t), 0.):
        for bt in bts:
            u = bt + dv
            if float(T(u)) == u and u - bt == dv and \
                    _l1_chain(T, u, bt, t) == _l1_chain(np.float64, u, bt, t):
                out.append((u, bt))
                break
        else:
            raise AssertionError((dtype, t, dv))
    return out


@functools.lru_cache(maxsize=None)
def wgt_tie_state(shape, dtype, seam):
    """xbar = 0, has_p = 0: u = x exactly; tl = 0.5 and w in {0, 0.5, 1, 2}, so t = tl w is
    exact, with x and bt on 1/64.  Planted: for w = 0.5, 1, 2 and 2^-20 the pairs of
    _l1_tie_pairs (|u - bt| on and beside t), and w = 0 over NaN beside w = 2^-20.  (l1
    only: the quotient of the l2 prox is not exact.)"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(6400 + 7 * sum(shape) + len(shape))
    x, bt = _grid(rng, n), _grid(rng, n)
    wt = rng.choice([0., 0.5, 1., 2.], n)
    us, bs, ws = [], [], []
    for wv in (0.5, 1., 2., 2. ** -20):
        for u, b in _l1_tie_pairs(dtype, TIE.tl * wv):
            us.append(u), bs.append(b), ws.append(wv)
        us.append(0.375), bs.append(np.nan), ws.append(0.)     # (w = 0 beside 2^-20 last)
    for s in _plant_rows(n, seam, len(us)):
        x[s:s + len(us)], bt[s:s + len(us)], wt[s:s + len(us)] = us, bs, ws
    return _frozen(dict(xbar=np.zeros(shape), x=x.reshape(shape), bt=bt.reshape(shape),
                        wt=wt.reshape(shape), p=np.zeros((len(shape),) + shape)))


@functools.lru_cache(maxsize=None)
def dual_data_tie_state(n, dtype, lmbda):
    """q, t, bt on 1/64 and sigma = 0.25: v = q + sigma (t - bt) is exact; w in
    {0, 0.5, 1, 2} and lmbda 1 or 0, so c = lmbda w is exact.  Planted (t = bt = 0): q on
    +-c and one ulp either side of each, and w = 0 over NaN in bt."""
    up, dn = _nb(dtype)
    rng = np.random.default_rng(6500 + n)
    q, t, bt = _grid(rng, n), _grid(rng, n), _grid(rng, n)
    wt = rng.choice([0., 0.5, 1., 2.], n)
    qs, ws = [], []
    for wv in (0.5, 1., 2.):
        cv = lmbda * wv
        qs += [cv, -cv, up(cv), dn(cv), up(-cv), dn(-cv), 0., -0.]
        ws += [wv] * 8
    k = len(qs)
    if n >= 2 * k + 2:
        for s in (0, n - k):
            q[s:s + k], wt[s:s + k], t[s:s + k], bt[s:s + k] = qs, ws, 0., 0.
        wt[k], bt[k] = 0., np.nan
    return _frozen(dict(q=q, t=t, bt=bt, wt=wt))


# ----------------------------------------------------------------- want, R and S
def _S_u(p, x, tau, w, dtype, g=None):
    d = x.ndim
    inner = sum(_abs_pair(p[a], d - 1 - a, False) * abs(c(w[a], dtype)) for a in range(d))
    if g is not None:
        inner = inner + np.abs(g)
    return np.abs(x) + abs(c(tau, dtype)) * inner


def _xbar_bound(x_new, R, S_x, x, theta, dtype):
    th = abs(c(theta, dtype))
    return R + 3, (1. + th) * np.maximum(S_x, np.abs(x_new)) + th * np.abs(x)


def lin_expected(p, st, sc, w, dtype, box):
    """((x_new, R, S), (xbar_new, R, S)) of the LIN primal half on the dual field p."""
    x, g = st["x"], st["g"]
    d = x.ndim
    x_new, xbar_new = vn.pd_lin_primal_step(p, x, g, sc.tau, sc.theta, box[0], box[1], w,
                                            dtype)
    S_x = _S_u(p, x, sc.tau, w, dtype, g)
    R = 4 * d + 2
    # a u that lies outside the box by more than its own bound is outside it in the kernel
    # as well: there x_new is the bound of the box itself, bit for bit (R = 0)
    lo, hi = vn.box_in(box[0], box[1], dtype)
    u = x - c(sc.tau, dtype) * (vn.grad_adj(p, w, dtype) + g)
    margin = R * U32 * S_x
    R_x = np.where((u < lo - margin) | (u > hi + margin), 0, R)
    return (x_new, R_x, S_x), (xbar_new,) + _xbar_bound(x_new, R, S_x, x, sc.theta, dtype)


def weighted_expected(p, st, sc, w, dtype, l1):
    """The same of the WGT primal half; R is an array: 4 d + 1 where the weight is zero."""
    x, bt, wt = st["x"], st["bt"], st["wt"]
    d = x.ndim
    x_new, xbar_new = vn.pd_weighted_primal_step(p, x, bt, wt, sc.tau, sc.tl, sc.theta, w,
                                                 l1, dtype)
    S_u = _S_u(p, x, sc.tau, w, dtype)
    t = c(sc.tl, dtype) * wt
    with np.errstate(invalid="ignore"):
        S_on = S_u + 2. * np.abs(bt) + t if l1 else (S_u + np.abs(t * bt)) / (1. + t)
    S_x = np.where(wt == 0, S_u, S_on)
    R = np.where(wt == 0, 4 * d + 1, 4 * d + (5 if l1 else 8))
    return (x_new, R, S_x), (xbar_new,) + _xbar_bound(x_new, R, S_x, x, sc.theta, dtype)


def prox_w_expected(u, bt, wt, tl, l1, dtype):
    """(want, R, S) of k_prox_w; where the weight is zero R = 0: the bits of u."""
    want = vn.prox_data_w(u, bt, wt, tl, l1, dtype)
    t = c(tl, dtype) * wt
    with np.errstate(invalid="ignore"):
        S = np.abs(u) + 2. * np.abs(bt) + t if l1 else (np.abs(u) + np.abs(t * bt)) / (1. + t)
    return want, np.where(wt == 0, 0, 4 if l1 else 7), np.where(wt == 0, 0., S)


def dual_data_expected(q, t, bt, wt, sigma, lmbda, l1, dtype):
    """(want, R, S) of k_pdl_dual_data; where the weight is zero R = 0: +0."""
    want = vn.pdl_dual_data(q, t, bt, wt, sigma, lmbda, l1, dtype)
    sg, lm = abs(c(sigma, dtype)), c(lmbda, dtype)
    w = np.ones_like(q) if wt is None else wt
    cc = lm * w
    with np.errstate(invalid="ignore"):
        S_v = np.abs(q) + sg * ((np.abs(t) if t is not None else 0.) + np.abs(bt))
        S = S_v + cc if l1 else S_v * cc / (cc + sg)
    R = (3 if t is not None else 2) + (0 if wt is None else 1) + (0 if l1 else 5)
    return want, np.where(w == 0, 0, R), np.where(w == 0, 0., S)


def box_holds_a_number(box, dtype):
    """Whether the type has a number in the caller's [lo, hi]: then every iterate the
    linear kernels hand back lies in it, in double."""
    lo, hi = vn.box_in(box[0], box[1], dtype)
    return box[0] <= lo <= hi <= box[1]


# ----------------------------------------------------------------- branch shares
def stack_branch_shares(cs, dtype, m=0):
    """The shares of the voxels of member m's random states on each side of the branches
    of the two forms, from the restatement alone (TV, anisotropic, p_in given)."""
    w = scase_weights(cs)
    st = lin_state(cs.shape, dtype, m)
    p = vn.pd_dual_step(st["xbar"], st["p"], SIGMA, 1., w, dtype)
    lo, hi = vn.box_in(BOX[0], BOX[1], dtype)
    u = st["x"] - vn.as_scalar(TAU, dtype) * (vn.grad_adj(p, w, dtype) + st["g"])
    out = {"below lo": np.mean(u < lo), "above hi": np.mean(u > hi),
           "inside the box": np.mean((u >= lo) & (u <= hi))}
    st = weights_state(cs.shape, dtype, m)
    u = vn.grad_adj_axpy(p, st["x"], TAU, w, dtype)
    on = st["wt"] != 0
    with np.errstate(invalid="ignore"):
        shrunk = on & (np.abs(u - st["bt"]) <= vn.as_scalar(WEIGHTED.tl, dtype) * st["wt"])
    out.update({"w == 0": np.mean(~on), "l1 shrunk onto bt": np.mean(shrunk),
                "l1 not shrunk (w > 0)": np.mean(on & ~shrunk)})
    return {k: float(v) for k, v in out.items()}
