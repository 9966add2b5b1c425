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
    only).  float64, exact and R == 0: bad = not equal.  vector: got, want of shape
    (d,) + volume are judged per voxel, by the Euclidean norm of the difference."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    if is64(dtype) or exact or R == 0:
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


def judge(got, st, sc, w, dtype, huber, l1, iso, has_p, exact=False, which="pxb"):
    """The outputs (p, x, xbar) of one iteration against the restatement: p against
    pd_dual_step, x and xbar against pd_primal_step of the call's own p.  Returns
    [(array name, bad, worst ratio)]; which: the letters of the outputs to judge."""
    out = []
    p = np.asarray(got[0], np.float64)
    if "p" in which:
        want, R, S = dual_expected(st, sc, w, dtype, huber, iso, has_p)
        out.append(("p_out",) + excess(p, want, R, S, dtype, exact, vector=iso))
    if "x" in which or "b" in which:
        ex, eb = primal_expected(p, st, sc, w, dtype, l1)
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


def plan(shape, dtype, offset=0, ry=0, rag=1, zchunk=0, iso=False, xcd_map=1):
    """What pd_launch, FusedKernel::launch / IsoKernel::launch, pd_auto_rows_per_lane and
    pd_plan_grid (nsol_pd_launch.hpp, nsol_pd.hip, nsol_pdi.hip) make of a single volume
    whose arrays all start `offset` elements behind a 16-byte boundary, under the knobs
    pd_ry, pd_rag, pd_zchunk."""
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
    auto = lambda: 1 if (_ceil(nx, TX) * _ceil(ny, (K_BLOCK // K_WAVE) * LY * 2)
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
        zc = max(2, _ceil(nz, _ceil(4096, ntx * nty)))
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
