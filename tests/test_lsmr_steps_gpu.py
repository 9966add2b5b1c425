"""The step kernels of the LSMR / ADMM inner loop, each against plain NumPy float64 built
from oracle.nsol_oracle.grad, grad_adj (with spacing) and admm_prox_g, through
nsol_amd.ops (ctypes -> C ABI).  Needs a real MI355X.

  nsol_lsmr.hip   k_lsmr_u, k_lsmr_v (also as _to), k_lsmr_hx, k_tk1_reg MODE 0 (cost and
                  gradient), MODE 1 (norm), MODE 2 (Lanczos)
  nsol_ops.hip    k_admm_vw, k_admm_vw<NORM>, k_admm_vw_g

Nothing here compares a kernel with another kernel: the shared mapping layer of
nsol_stencil.hpp (voxel_at, vlc / vs, dispatch_stencil, stencil_grid) moves every kernel
alike, so only an independent reference sees a mistake in it.

Which instantiation a shape reaches (VW = 4 float32 / 2 float64 elements per vector):
  (5, 6, 64), (2, 5, 260)            vector, 4 rows per workgroup; 260: two / three x tiles
  (3, 7, 67), (2, 5, 259)            ragged, 4 rows (a row's last vector is partial)
  (5, 6, 64) one element off         ragged, 4 rows (operands off the 16-byte grid)
  (4, 5, 7)                          scalar, 4 rows (rows shorter than 4 vectors)
  (1000,), (1031,), (7,), (5, 1, 16) 1 row per workgroup: vector, ragged, scalar, vector
  (1, 9, 12), (6, 7, 1)              nz = 1; nx = 1 (scalar, every lane but one idle)
  (33, 20), (64, 259)                2-D: vector, ragged
  (40, 36, 64), stencil_blocks 256   grid-stride loop: 360 row groups on 256 workgroups,
                                     9 row groups per plane: no slab permutation
  (5, 32, 64), stencil_slabs 1 / 0   slab permutation (P = 8, 8 row groups per plane) in
                                     one trip, and the natural order
  (40, 32, 64), blocks 256, slabs 1/0  the permutation under the loop (320 row groups)
  2 * 4096 * 256 + 38, float64, 1-D  outer x index (two trips of 4096 tiles of 512)
  k_lsmr_hx: n = 1, 7, 255, 256, 257 and 1024 * 256 + 259 (past its 1024 workgroups)
  k_admm_vw_g: (6, 7, 64), (2, 9, 260), (1, 4, 8); (18, 5, 8): two z chunks, the second
               starts with the warm-up plane

The reference is evaluated on what the device holds: float32 inputs widened; weights,
coefficients, thr and alpha rounded to the working type T first, as the kernels cast
them; the spacing handed to the oracle is chosen so that 1 / spacing is that rounded
weight exactly.

Bounds (derived, not measured).  Per element |got - ref| <= C * eps(T) * M, M the same
expression in float64 with every term replaced by its absolute value (differences become
sums), C the number of roundings on the kernel's longest chain (-ffp-contract=off: every
product and every sum rounds once).  eps = 2u: half of the bound is the kernel's C
roundings of at most u each, the other half is left to the float64 reference's own
(float64 case) and to second-order terms.
  k_lsmr_u    C = 4   hi*w, + lo*(-w), * c_bv, + c_u*u
  k_lsmr_v    C = 7   t*(-wx), + l*wx, + y term, + z term, * c_btu, + c_atu*Atu, + c_v*v
  k_lsmr_hx   C = 4   c_hbar*hbar, + h (hbar: 2), * c_x, + x (x: 4); h: 2
  k_tk1_reg   C = 8   d: 2, * (-wx), + l*wx, + y term, + z term (6), * alpha, + g;
              Lanczos C = 10: the same 7, + c_g*g, + c_x*x, + c_z*z
  k_admm_vw   t_a = grad_a x + w_a - c_a: 4 roundings against Mt_a = gradabs_a|x| + |w_a|
              + |c_a|.  v_a = (|t| - thr) t_a / |t| moves with EVERY component of t (the
              norm), so its M is |Mt|_2 + thr, not Mt_a: squares and two sums (3), sqrt,
              - thr, * t_a, / |t| -> C = 11.  The map t -> v is 1-Lipschitz, so nothing
              is amplified at |t| = thr.  w'_a = t_a - v_a: C = 12, M = Mt_a + M_v.
              rhs_a = rhs_scale (v_a - w'_a + c_a): C = 15, M = |rhs_scale| (M_v + M_w'
              + |c_a|).
  k_admm_vw_g w' as above; g = c_atu atb + c_btu grad^T rhs: C = 15 + 4 + 2 = 21,
              M = |c_atu| |atb| + |c_btu| gradadjabs(M_rhs).  sum rhs^2 (rhs is never
              stored): |got - sum ref^2| <= sum (2 |ref| e + e^2), e the rhs bound.
Every returned sum that has its values in memory: math.fsum over the float64 squares of
what the kernel stored, relative 1e-12 (lanes past a row's end, row groups visited twice
or never).  sum |K x|^2 has no stored values: the differences hi*w + lo*(-w) are formed
in T by NumPy (three roundings, which contraction off makes the kernel's own) and summed
by fsum, and the same differences are held to the float64 oracle within 2 eps M.

Guards: every operand lies inside a larger allocation, 64 elements of 7.25 before and
after it; afterwards every guard and every read-only input is bit-identical.

Largest |got - ref| / (eps * M) observed on an MI355X, float32 (float64: 0 for every
kernel and output -- with contraction off the kernels round where NumPy rounds, in the
same order, so the float64 results are the reference's bit for bit):
  k_lsmr_u     u_top 0.96, u_bot 1.53                       (C = 4)
  k_lsmr_v     in place 1.61, out fresh 1.50, out = Atu 1.38 (C = 7)
  k_lsmr_hx    hbar 0.88 (2), x 1.42 (4), h 0.96 (2)
  k_tk1_reg    cost-grad 1.56 (C = 8), Lanczos 1.54 (C = 10)
  k_admm_vw    v 1.79 (C = 11), w' 0.54 (12), rhs 0.94 (15)
  k_admm_vw_g  w' 0.45 (C = 12), g 0.43 (21)
Every sum met its 1e-12 gate.  Value-only mutations of a scratch build that the module
was checked to notice: wy and wz swapped in k_lsmr_u (every anisotropic case with a y
axis), the y term's lower neighbour taken as zero in k_lsmr_v (every case with more than
one row), v summed for rhs in k_admm_vw<NORM> (every case)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
DT_IDS = ("f64", "f32")
GUARD = 64
SENT = 7.25                          # finite, exact in both types
W_ISO = (1.0, 1.0, 1.0)
W_ANISO = (1.0, 0.7, 1.3)            # inverse spacings (wx, wy, wz), non-dyadic
WEIGHTS = (W_ISO, W_ANISO)
W_IDS = ("iso", "aniso")
B_NONE, B_GRAD, B_IDENTITY = 0, 1, 2

# (id, shape, knobs, offset of every operand from the 16-byte grid in elements)
CASES = (
    ("vec4", (5, 6, 64), {}, 0),
    ("vec4-tiles", (2, 5, 260), {}, 0),
    ("rag4-67", (3, 7, 67), {}, 0),
    ("rag4-259", (2, 5, 259), {}, 0),
    ("rag4-offgrid", (5, 6, 64), {}, 1),
    ("scalar4", (4, 5, 7), {}, 0),
    ("row1-1000", (1000,), {}, 0),
    ("row1-1031", (1031,), {}, 0),
    ("row1-7", (7,), {}, 0),
    ("row1-ny1", (5, 1, 16), {}, 0),
    ("nz1", (1, 9, 12), {}, 0),
    ("nx1", (6, 7, 1), {}, 0),
    ("2d-33x20", (33, 20), {}, 0),
    ("2d-64x259", (64, 259), {}, 0),
    ("loop", (40, 36, 64), {"stencil_blocks": 256}, 0),
    ("slabs-on", (5, 32, 64), {"stencil_slabs": 1}, 0),
    ("slabs-off", (5, 32, 64), {"stencil_slabs": 0}, 0),
    ("loop-slabs-on", (40, 32, 64), {"stencil_blocks": 256, "stencil_slabs": 1}, 0),
    ("loop-slabs-off", (40, 32, 64), {"stencil_blocks": 256, "stencil_slabs": 0}, 0),
)
CASE_IDS = tuple(c[0] for c in CASES)
OUTER_X_N = 2 * 4096 * 256 + 38

_RATIOS = {}


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()                      # fails loudly if the .so is missing
    yield nsol_amd
    for key in sorted(_RATIOS):
        print("largest |got - ref| / (eps M): %-28s %.3g" % ("%s %s" % key, _RATIOS[key]))


def _knobs(knobs):
    from nsol_amd import _lib
    for k, v in knobs.items():
        _lib.set_param(k, v)         # (put back after the test by conftest)


# ------------------------------------------------------------------ operands
class _Op(object):
    """A flat device operand inside a larger allocation filled with SENT."""

    def __init__(self, host, dtype, off=0):
        import torch
        self.dtype = dtype
        self.host = np.ascontiguousarray(host, dtype=dtype).reshape(-1).copy()
        self.n = self.host.size
        self.lo = GUARD + off
        td = torch.float32 if dtype == np.float32 else torch.float64
        self.big = torch.full((self.lo + self.n + GUARD + 3,), SENT, dtype=td, device="cuda")
        assert self.big.data_ptr() % 16 == 0
        self.t = self.big[self.lo:self.lo + self.n]
        self.t.copy_(torch.from_numpy(self.host))
        assert (self.t.data_ptr() % 16 == 0) == (off * self.host.itemsize % 16 == 0)

    def f64(self, shape=None):
        a = self.host.astype(np.float64)
        return a if shape is None else a.reshape(shape)

    def get(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        big = self.big.cpu().numpy()
        sent = np.full(1, SENT, dtype=self.dtype).tobytes()
        head, tail = big[:self.lo], big[self.lo + self.n:]
        return head.tobytes() == sent * head.size and tail.tobytes() == sent * tail.size

    def unchanged(self):
        return self.get().tobytes() == self.host.tobytes()


def _check_memory(written, read_only):
    for name, op in list(written.items()) + list(read_only.items()):
        if op is not None:
            assert op.guards_intact(), "guard elements around %s were written" % name
    for name, op in read_only.items():
        if op is not None:
            assert op.unchanged(), "read-only input %s was written" % name


def _rand(rng, n, dtype, off=0, scale=1.0):
    return _Op(scale * rng.standard_normal(n), dtype, off)


def _sentinels(n, dtype, off=0):
    return _Op(np.full(n, SENT), dtype, off)


def _r(c, dtype):
    """A coefficient as the kernel holds it: rounded to the working type."""
    return float(dtype(c))


def _weights(w, dtype):
    return tuple(_r(v, dtype) for v in w)


def _spacing(w, nd):
    """h with 1 / h == w exactly in float64 (the oracle divides by the spacing)."""
    out = []
    for a in range(nd):
        h = 1.0 / w[a]
        for cand in (h, np.nextafter(h, 0.0), np.nextafter(h, np.inf)):
            if 1.0 / float(cand) == w[a]:
                out.append(float(cand))
                break
        else:
            raise AssertionError("no spacing inverts to %r" % (w[a],))
    return np.array(out)


def _stacked(shape):
    nd = len(shape)
    return (nd * shape[0],) + tuple(shape[1:])


# ------------------------------------------------ magnitudes (|.| everywhere)
def _shift(a, axis, fwd):
    """a[i + 1] (fwd) or a[i - 1] along axis, zero outside."""
    out = np.zeros_like(a)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis], dst[axis] = (slice(1, None), slice(0, -1)) if fwd else \
        (slice(0, -1), slice(1, None))
    out[tuple(dst)] = a[tuple(src)]
    return out


def _grad_abs(ax, w):
    """Per direction a (0 = x = last axis): w_a (|x[i + 1]| + |x[i]|)."""
    nd = ax.ndim
    return [w[a] * (_shift(ax, nd - 1 - a, True) + ax) for a in range(nd)]


def _grad_adj_abs(parts, w):
    nd = parts[0].ndim
    return sum(w[a] * (parts[a] + _shift(parts[a], nd - 1 - a, False)) for a in range(nd))


def _grad_in_T(x, w, dtype):
    """The differences as the kernels form them: hi*w + lo*(-w), each operation rounded
    in T (contraction is off in the library's build)."""
    nd = x.ndim
    x = x.astype(dtype)
    return [_shift(x, nd - 1 - a, True) * dtype(w[a]) + x * dtype(-w[a]) for a in range(nd)]


def _split(a, nd):
    return np.array_split(a, nd) if nd > 1 else [a]


# ------------------------------------------------------------------ gates
def _hold(kernel, what, got, ref, M, C, dtype):
    eps = float(np.finfo(dtype).eps)
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    M = np.asarray(M, np.float64).reshape(-1)
    assert got.shape == ref.shape == M.shape
    assert np.all(np.isfinite(got)), "%s %s: not finite" % (kernel, what)
    err = np.abs(got - ref)
    pos = M > 0
    ratio = float(np.max(err[pos] / (eps * M[pos]))) if pos.any() else 0.0
    key = ("%s %s" % (kernel, what), np.dtype(dtype).name)
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), ratio)
    bad = err > C * eps * M
    assert not bad.any(), "%s %s: %d of %d elements past %d eps M, worst ratio %.2f, " \
        "first at %d (got %r, ref %r)" % (kernel, what, int(bad.sum()), bad.size, C, ratio,
                                          int(np.argmax(bad)), got[np.argmax(bad)],
                                          ref[np.argmax(bad)])


def _hold_sum(kernel, got, *stored):
    ref = math.fsum(v for a in stored
                    for v in (np.asarray(a, np.float64).reshape(-1) ** 2).tolist())
    assert abs(got - ref) <= 1e-12 * ref, "%s: sum %.17g, fsum of what was stored %.17g" % \
        (kernel, got, ref)


# ------------------------------------------------------------------ k_lsmr_u
C_U = 4


def _run_u(shape, dtype, w, off, bmode, with_av, coef, seed, u_sentinels=False,
           v_sentinels=False):
    from nsol_amd import ops
    from oracle import nsol_oracle as orc
    rng = np.random.default_rng(seed)
    n, nd = int(np.prod(shape)), len(shape)
    rows = nd * n if bmode == B_GRAD else n
    wT = _weights(w, dtype)
    c_av, c_bv, c_u = (_r(c, dtype) for c in coef)
    Av = _rand(rng, n, dtype, off) if with_av else None
    v = _sentinels(n, dtype, off) if v_sentinels else _rand(rng, n, dtype, off)
    if u_sentinels:
        u_top, u_bot = _sentinels(n, dtype, off), _sentinels(rows, dtype, off)
    else:
        u_top, u_bot = _rand(rng, n, dtype, off), _rand(rng, rows, dtype, off)
    got = ops.lsmr_u_update(None if Av is None else Av.t, v.t, u_top.t, u_bot.t, bmode,
                            shape, wT, c_av, c_bv, c_u)
    _check_memory({"u_bot": u_bot, "u_top": u_top if with_av else None},
                  {"Av": Av, "v": v, "u_top": None if with_av else u_top})
    v64 = v.f64(shape)
    if bmode == B_GRAD:
        Bv = orc.grad(v64, _spacing(wT, nd)).reshape(-1)
        MB = np.concatenate([p.reshape(-1) for p in _grad_abs(np.abs(v64), wT)])
    else:
        Bv, MB = v64.reshape(-1), np.abs(v64).reshape(-1)
    ub0 = u_bot.f64()
    _hold("k_lsmr_u", "u_bot", u_bot.get(), c_bv * Bv + c_u * ub0,
          abs(c_bv) * MB + abs(c_u) * np.abs(ub0), C_U, dtype)
    stored = [u_bot.get()]
    if with_av:
        ut0 = u_top.f64()
        _hold("k_lsmr_u", "u_top", u_top.get(), c_av * Av.f64() + c_u * ut0,
              abs(c_av) * np.abs(Av.f64()) + abs(c_u) * np.abs(ut0), C_U, dtype)
        stored.append(u_top.get())
    _hold_sum("k_lsmr_u", got, *stored)


@pytest.mark.parametrize("w", WEIGHTS, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_lsmr_u_update(nsol, case, dtype, w):
    _, shape, knobs, off = case
    _knobs(knobs)
    coef = (0.8, -0.37, 1.3)
    _run_u(shape, dtype, w, off, B_GRAD, True, coef, 1)
    _run_u(shape, dtype, w, off, B_GRAD, False, coef, 2)       # Av = None: lower block only
    _run_u(shape, dtype, w, off, B_IDENTITY, True, coef, 3)
    # zero coefficients: what u / v held must not matter
    _run_u(shape, dtype, w, off, B_GRAD, True, (0.8, -0.37, 0.0), 4, u_sentinels=True)
    _run_u(shape, dtype, w, off, B_GRAD, True, (0.8, 0.0, 1.3), 5, v_sentinels=True)


# ------------------------------------------------------------------ k_lsmr_v
C_V = 7


def _run_v(shape, dtype, w, off, bmode, where, coef, seed, v_sentinels=False):
    from nsol_amd import ops
    from oracle import nsol_oracle as orc
    rng = np.random.default_rng(seed)
    n, nd = int(np.prod(shape)), len(shape)
    rows = nd * n if bmode == B_GRAD else n
    wT = _weights(w, dtype)
    c_atu, c_btu, c_v = (_r(c, dtype) for c in coef)
    Atu = _rand(rng, n, dtype, off)
    u_bot = _rand(rng, rows, dtype, off)
    v = _sentinels(n, dtype, off) if v_sentinels else _rand(rng, n, dtype, off)
    fresh = _sentinels(n, dtype, off) if where == "fresh" else None
    out = {"inplace": v, "fresh": fresh, "atu": Atu}[where]
    got = ops.lsmr_v_update(Atu.t, u_bot.t, v.t, bmode, shape, wT, c_atu, c_btu, c_v,
                            out=None if where == "inplace" else out.t)
    _check_memory({"out": out}, {"u_bot": u_bot, "Atu": None if where == "atu" else Atu,
                                 "v": None if where == "inplace" else v})
    ub = u_bot.f64(_stacked(shape) if bmode == B_GRAD else shape)
    if bmode == B_GRAD:
        Bt = orc.grad_adj(ub, _spacing(wT, nd)).reshape(-1)
        MB = _grad_adj_abs(_split(np.abs(ub), nd), wT).reshape(-1)
    else:
        Bt, MB = ub.reshape(-1), np.abs(ub).reshape(-1)
    ref = c_atu * Atu.f64() + c_btu * Bt + c_v * v.f64()
    M = abs(c_atu) * np.abs(Atu.f64()) + abs(c_btu) * MB + abs(c_v) * np.abs(v.f64())
    _hold("k_lsmr_v", where, out.get(), ref, M, C_V, dtype)
    _hold_sum("k_lsmr_v", got, out.get())


@pytest.mark.parametrize("w", WEIGHTS, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_lsmr_v_update(nsol, case, dtype, w):
    _, shape, knobs, off = case
    _knobs(knobs)
    coef = (0.9, 0.41, -1.2)
    _run_v(shape, dtype, w, off, B_GRAD, "inplace", coef, 11)
    _run_v(shape, dtype, w, off, B_GRAD, "fresh", coef, 12)
    _run_v(shape, dtype, w, off, B_GRAD, "atu", coef, 13)
    _run_v(shape, dtype, w, off, B_IDENTITY, "fresh", coef, 14)
    _run_v(shape, dtype, w, off, B_GRAD, "fresh", (0.9, 0.41, 0.0), 15, v_sentinels=True)


# ------------------------------------------------------------------ k_lsmr_hx
C_HX = 4


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", (1, 7, 255, 256, 257, 1024 * 256 + 259))
def test_lsmr_hx_update(nsol, n, dtype):
    from nsol_amd import ops
    rng = np.random.default_rng(n)
    for off in (0, 1):
        c_hbar, c_x, c_h, c_v = (_r(c, dtype) for c in (0.6, -0.45, 1.7, 0.3))
        hbar, x, h, v = (_rand(rng, n, dtype, off) for _ in range(4))
        got = ops.lsmr_hx_update(hbar.t, x.t, h.t, v.t, c_hbar, c_x, c_h, c_v)
        _check_memory({"hbar": hbar, "x": x, "h": h}, {"v": v})
        hb = c_hbar * hbar.f64() + h.f64()
        Mhb = abs(c_hbar) * np.abs(hbar.f64()) + np.abs(h.f64())
        _hold("k_lsmr_hx", "hbar", hbar.get(), hb, Mhb, 2, dtype)
        _hold("k_lsmr_hx", "x", x.get(), x.f64() + c_x * hb,
              np.abs(x.f64()) + abs(c_x) * Mhb, C_HX, dtype)
        _hold("k_lsmr_hx", "h", h.get(), c_h * h.f64() + c_v * v.f64(),
              abs(c_h) * np.abs(h.f64()) + abs(c_v) * np.abs(v.f64()), 2, dtype)
        _hold_sum("k_lsmr_hx", got, x.get())


# ------------------------------------------------------------------ k_tk1_reg
C_TK1, C_LANCZOS, C_DIFF = 8, 10, 2


def _ktk(x64, wT, nd):
    from oracle import nsol_oracle as orc
    sp = _spacing(wT, nd)
    ref = orc.grad_adj(orc.grad(x64, sp), sp).reshape(-1)
    M = _grad_adj_abs(_grad_abs(np.abs(x64), wT), wT).reshape(-1)
    return ref, M


def _hold_grad_sum(kernel, got, x, shape, wT, dtype):
    """sum |K x|^2: no stored values -- the differences formed in T by NumPy, themselves
    held to the float64 oracle, summed by fsum."""
    from oracle import nsol_oracle as orc
    nd = len(shape)
    x64 = x.f64(shape)
    d = np.concatenate([p.reshape(-1) for p in _grad_in_T(x64, wT, dtype)])
    assert d.dtype == dtype
    _hold(kernel, "differences in T", d, orc.grad(x64, _spacing(wT, nd)).reshape(-1),
          np.concatenate([p.reshape(-1) for p in _grad_abs(np.abs(x64), wT)]), C_DIFF, dtype)
    _hold_sum(kernel, got, d)


def _run_tk1(shape, dtype, w, off, seed):
    from nsol_amd import ops
    rng = np.random.default_rng(seed)
    n, nd = int(np.prod(shape)), len(shape)
    wT = _weights(w, dtype)
    alpha, c_g, c_x, c_z = (_r(c, dtype) for c in (0.37, 0.8, -1.3, -0.6))
    x, g, z = (_rand(rng, n, dtype, off) for _ in range(3))
    lap, Mlap = _ktk(x.f64(shape), wT, nd)
    # MODE 0
    out = _sentinels(n, dtype, off)
    s, _ = ops.tk1_reg_cost_grad(x.t, g.t, shape, wT, alpha, out=out.t)
    _check_memory({"grad": out}, {"x": x, "g": g})
    _hold("k_tk1_reg", "cost-grad", out.get(), g.f64() + alpha * lap,
          np.abs(g.f64()) + abs(alpha) * Mlap, C_TK1, dtype)
    _hold_grad_sum("k_tk1_reg cost-grad", s, x, shape, wT, dtype)
    # MODE 1
    s = ops.tk1_grad_norm(x.t, shape, wT)
    _check_memory({}, {"x": x})
    _hold_grad_sum("k_tk1_reg norm", s, x, shape, wT, dtype)
    # MODE 2
    for zz, cz in ((z, c_z), (None, 0.0)):
        out = _sentinels(n, dtype, off)
        s = ops.tk1_lanczos(x.t, g.t, None if zz is None else zz.t, shape, wT, alpha, c_g,
                            c_x, cz, out=out.t)
        _check_memory({"out": out}, {"x": x, "g": g, "z": zz})
        ref = c_g * g.f64() + alpha * lap + c_x * x.f64()
        M = abs(c_g) * np.abs(g.f64()) + abs(alpha) * Mlap + abs(c_x) * np.abs(x.f64())
        if zz is not None:
            ref, M = ref + cz * zz.f64(), M + abs(cz) * np.abs(zz.f64())
        _hold("k_tk1_reg", "Lanczos", out.get(), ref, M, C_LANCZOS, dtype)
        _hold_sum("k_tk1_reg Lanczos", s, out.get())


@pytest.mark.parametrize("w", WEIGHTS, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_tk1_regulariser_kernels(nsol, case, dtype, w):
    _, shape, knobs, off = case
    _knobs(knobs)
    _run_tk1(shape, dtype, w, off, 21)


# -------------------------------------------------------------- outer x index
def test_outer_x_index_of_a_long_signal(nsol):
    """A 1-D float64 signal of more than 4096 tiles of 256 lanes x 2 elements: the units
    dealt to blockIdx.y carry an outer x index.  k_lsmr_v and k_tk1_reg's norm only."""
    from nsol_amd import ops
    dtype, shape = np.float64, (OUTER_X_N,)
    assert OUTER_X_N > 4096 * 256 * 2 and OUTER_X_N % 2 == 0
    for w in WEIGHTS:
        _run_v(shape, dtype, w, 0, B_GRAD, "inplace", (0.9, 0.41, -1.2), 31)
        wT = _weights(w, dtype)
        x = _rand(np.random.default_rng(32), OUTER_X_N, dtype)
        s = ops.tk1_grad_norm(x.t, shape, wT)
        _check_memory({}, {"x": x})
        _hold_grad_sum("k_tk1_reg norm", s, x, shape, wT, dtype)


# ------------------------------------------------------------------ k_admm_vw
C_VW_V, C_VW_W, C_VW_RHS, C_VW_G = 11, 12, 15, 21


def _admm_reference(x64, w0, c0, shape, wT, thr, rs):
    """(t, v, w', rhs) and the magnitudes (M_v, M_w', M_rhs), flat and stacked by
    component, from the oracle's grad and admm_prox_g."""
    from oracle import nsol_oracle as orc
    nd = len(shape)
    t = orc.grad(x64, _spacing(wT, nd)).reshape(-1) + w0 - c0
    v = orc.admm_prox_g(t, thr, nd)
    wn = t - v
    rhs = rs * (v - wn + c0)
    Mt = np.concatenate([p.reshape(-1) for p in _grad_abs(np.abs(x64), wT)]) + \
        np.abs(w0) + np.abs(c0)
    Mn = np.sqrt(sum(p ** 2 for p in _split(Mt, nd)))
    Mv = np.tile(Mn + thr, nd)
    Mw = Mt + Mv
    Mr = abs(rs) * (Mv + Mw + np.abs(c0))
    return t, v, wn, rhs, Mv, Mw, Mr


def _run_vw(shape, dtype, w, off, seed, have_v=True, have_c=True, have_rhs=True,
            want_norm=False, thr=0.3, rs=0.7, edit=None):
    from nsol_amd import ops
    rng = np.random.default_rng(seed)
    n, nd = int(np.prod(shape)), len(shape)
    wT = _weights(w, dtype)
    thr, rs = _r(thr, dtype), _r(rs, dtype)
    xh = rng.standard_normal(n)
    wh = 0.5 * rng.standard_normal(nd * n)
    ch = 0.5 * rng.standard_normal(nd * n)
    if edit is not None:
        edit(xh.reshape(shape), wh.reshape((nd,) + tuple(shape)),
             ch.reshape((nd,) + tuple(shape)))
    x, w_ = _Op(xh, dtype, off), _Op(wh, dtype, off)
    c = _Op(ch, dtype, off) if have_c else None
    v = _sentinels(nd * n, dtype, off) if have_v else None
    rhs = _sentinels(nd * n, dtype, off) if have_rhs else None
    got = ops.admm_vw_update(x.t, None if v is None else v.t, w_.t,
                             None if c is None else c.t, None if rhs is None else rhs.t,
                             shape, wT, thr, rs, want_norm=want_norm)
    _check_memory({"v": v, "w": w_, "rhs": rhs}, {"x": x, "c": c})
    c0 = c.f64() if have_c else np.zeros(nd * n)
    t, vr, wr, rr, Mv, Mw, Mr = _admm_reference(x.f64(shape), w_.f64(), c0, shape, wT, thr, rs)
    if have_v:
        _hold("k_admm_vw", "v", v.get(), vr, Mv, C_VW_V, dtype)
    _hold("k_admm_vw", "w'", w_.get(), wr, Mw, C_VW_W, dtype)
    if have_rhs:
        _hold("k_admm_vw", "rhs", rhs.get(), rr, Mr, C_VW_RHS, dtype)
    if want_norm:
        _hold_sum("k_admm_vw<NORM>", got, rhs.get())
    return t, (v.get() if have_v else None), w_.get()


@pytest.mark.parametrize("w", WEIGHTS, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_admm_vw_update(nsol, case, dtype, w):
    _, shape, knobs, off = case
    _knobs(knobs)
    _run_vw(shape, dtype, w, off, 41)
    _run_vw(shape, dtype, w, off, 42, want_norm=True)
    _run_vw(shape, dtype, w, off, 43, have_v=False, want_norm=True)
    _run_vw(shape, dtype, w, off, 44, have_c=False)
    _run_vw(shape, dtype, w, off, 45, have_rhs=False)
    _run_vw(shape, dtype, w, off, 46, have_v=False, have_c=False, have_rhs=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_admm_vw_shrink_edges(nsol, dtype):
    # a block where grad x + w - c is exactly zero: x constant (zero) around it, w = c
    shape = (5, 6, 64)

    def zero_block(x, w, c):
        x[1:4, 1:5, 8:40] = 0.0
        w[:, 1:3, 1:4, 8:39] = c[:, 1:3, 1:4, 8:39]
    for thr in (0.3, 0.0):
        t, v, wn = _run_vw(shape, dtype, W_ANISO, 0, 51, thr=thr, edit=zero_block,
                           want_norm=True)
        blk = np.zeros((3,) + shape, bool)
        blk[:, 1:3, 1:4, 8:39] = True
        blk = blk.reshape(-1)
        assert np.all(t[blk] == 0.0)                       # (the case is what it claims)
        assert np.all(v[blk] == 0.0) and np.all(wn[blk] == 0.0)
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(wn))
    # thr = 0 elsewhere: v = t, w' = 0 up to the roundings of the bound
    _run_vw((3, 7, 67), dtype, W_ANISO, 0, 52, thr=0.0)
    # 1-D, |t| == thr exactly (x = 0, c absent, w = +-0.5 = thr): v = 0 there
    n = 1031

    def at_threshold(x, w, c):
        x[:] = 0.0
        w[0, ::3] = 0.5
        w[0, 1::3] = -0.5
    t, v, wn = _run_vw((n,), dtype, W_ISO, 0, 53, thr=0.5, have_c=False, edit=at_threshold)
    hit = np.abs(t) == 0.5
    assert hit.sum() >= 2 * (n // 3)
    assert np.all(v[hit] == 0.0) and np.array_equal(wn[hit], t[hit].astype(dtype))


# ------------------------------------------------------------------ k_admm_vw_g
def _run_vw_g(shape, dtype, w, off, seed, have_c, expect=True):
    import torch
    from nsol_amd import ops
    from oracle import nsol_oracle as orc
    rng = np.random.default_rng(seed)
    n, nd = int(np.prod(shape)), len(shape)
    wT = _weights(w, dtype)
    thr, rs, c_atu, c_btu = (_r(c, dtype) for c in (0.3, 0.7, 0.9, 0.41))
    x, atb = _rand(rng, n, dtype, off), _rand(rng, n, dtype, off)
    w_in = _rand(rng, nd * n, dtype, off, 0.5)
    c = _rand(rng, nd * n, dtype, off, 0.5) if have_c else None
    w_out, g = _sentinels(nd * n, dtype, off), _sentinels(n, dtype, off)
    res = _Op(np.full(2, SENT), np.float64)
    ok = ops.admm_vw_update_g(x.t, w_in.t, w_out.t, None if c is None else c.t, atb.t, g.t,
                              shape, wT, thr, rs, c_atu, c_btu, res.t)
    torch.cuda.synchronize()
    assert ok is expect
    _check_memory({"w_out": w_out, "g": g, "result": res},
                  {"x": x, "w_in": w_in, "c": c, "atb": atb})
    if not expect:
        assert w_out.unchanged() and g.unchanged() and res.unchanged()
        return
    eps = float(np.finfo(dtype).eps)
    c0 = c.f64() if have_c else np.zeros(nd * n)
    _, _, wr, rr, _, Mw, Mr = _admm_reference(x.f64(shape), w_in.f64(), c0, shape, wT, thr, rs)
    _hold("k_admm_vw_g", "w'", w_out.get(), wr, Mw, C_VW_W, dtype)
    sp = _spacing(wT, nd)
    gref = c_atu * atb.f64() + c_btu * orc.grad_adj(rr.reshape(_stacked(shape)), sp).reshape(-1)
    Mg = abs(c_atu) * np.abs(atb.f64()) + abs(c_btu) * _grad_adj_abs(
        [p.reshape(shape) for p in _split(Mr, nd)], wT).reshape(-1)
    _hold("k_admm_vw_g", "g", g.get(), gref, Mg, C_VW_G, dtype)
    sums = res.get()
    _hold_sum("k_admm_vw_g sum g^2", float(sums[1]), g.get())
    e = C_VW_RHS * eps * Mr
    assert abs(float(sums[0]) - math.fsum((rr ** 2).tolist())) <= \
        float(np.sum(2 * np.abs(rr) * e + e * e)), "k_admm_vw_g sum rhs^2"


@pytest.mark.parametrize("have_c", (True, False), ids=("c", "no-c"))
@pytest.mark.parametrize("w", WEIGHTS, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", ((6, 7, 64), (2, 9, 260), (1, 4, 8), (18, 5, 8)),
                         ids=("6x7x64", "2x9x260", "1x4x8", "18x5x8-chunks"))
def test_admm_vw_update_g(nsol, shape, dtype, w, have_c):
    _run_vw_g(shape, dtype, w, 0, 61, have_c)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_admm_vw_update_g_declines_what_it_cannot_take(nsol, dtype):
    """False and nothing written: a 2-D shape, a ragged row, operands off the grid."""
    _run_vw_g((33, 20), dtype, W_ISO, 0, 62, True, expect=False)
    _run_vw_g((3, 7, 67), dtype, W_ISO, 0, 63, True, expect=False)
    _run_vw_g((6, 7, 64), dtype, W_ISO, 1, 64, True, expect=False)
