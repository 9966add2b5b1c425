"""Reference, tap sets, inputs, shapes and the table of answering entry points of the
one-pass periodic 3-D blur's tests (test_blur3_host.py checks them on the CPU,
test_blur3_gpu.py uses them).  NumPy only.

reference() is the blur by index arithmetic in float64 with the float64 taps UNROUNDED;
magnitude() is the same expression with every term replaced by its absolute value -- the S
the per-voxel bounds  |got - ref| <= C u S  refer to (u = 2^-24 / 2^-53).

C is counted from the kernels' arithmetic (nsol_blur3_dma.hpp, nsol_conv.hip), before any
kernel ran against it:
  * a voxel's value is a sum of products wz wy wx x.  Each tap is rounded to the working
    type T once on the host: 3 roundings per product;
  * k_blur3_dma applies a pass's taps with fused multiply-adds onto the running sum -- one
    rounding per tap, ntaps per pass (the packed float x pass sums the even and the odd
    taps apart and adds the two: (ntaps + 1) / 2 + 1 <= ntaps for ntaps >= 3).  No tap pair
    is folded (a + b) before the multiply.  Three passes:            C_DMA = 3 ntaps + 3
  * k_blur3_wrap / k_blur3_wrap_pp are written `acc += w * v`: a product and a sum per
    tap, and the library is built with -ffp-contract=off, so both round -- 2 ntaps - 1
    per pass, three passes, + 3:                                     C_REG = 6 ntaps
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
DTYPES = (np.float32, np.float64)
NTAPS = (3, 5, 7, 9, 11, 13, 15, 17)
SPIKE = 1.0e3

DMA_ROWS, DMA_LANES = 64, 16          # a DMA tile: 64 rows of 16 vectors (NWD = 16, kDmaLxb)


def unit(dtype):
    return U64 if np.dtype(dtype) == np.float64 else U32


def vec(dtype):
    """Elements per 16-byte vector."""
    return 16 // np.dtype(dtype).itemsize


def rounded(a, dtype):
    return np.asarray(a).astype(dtype).astype(np.float64)


def c_dma(ntaps):
    return 3 * ntaps + 3


def c_reg(ntaps):
    return 6 * ntaps


# ------------------------------------------------------------------------- reference
def corr_axis(x, w, axis):
    """out[i] = sum_t w[t] x[(i + t - R) mod n] along axis; any R, also R >= n."""
    w = np.asarray(w, dtype=np.float64)
    n, R = x.shape[axis], w.size // 2
    out = np.zeros_like(x, dtype=np.float64)
    i = np.arange(n)
    for t in range(w.size):
        out += w[t] * np.take(x, (i + t - R) % n, axis=axis)
    return out


def reference(x, tz, ty, tx):
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 3
    return corr_axis(corr_axis(corr_axis(x, tx, 2), ty, 1), tz, 0)


def magnitude(x, tz, ty, tx):
    return reference(np.abs(x), np.abs(tz), np.abs(ty), np.abs(tx))


def grad_sums(x, w=(1.0, 1.0, 1.0)):
    """sum over voxels and axes of (w_a (x[i + 1] - x[i]))^2 with ZERO behind the last
    voxel of an axis; w = (wx, wy, wz)."""
    x = np.asarray(x, dtype=np.float64)
    total = []
    for a, axis in enumerate((2, 1, 0)):
        nxt = np.zeros_like(x)
        src = [slice(None)] * 3
        dst = [slice(None)] * 3
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
        nxt[tuple(dst)] = x[tuple(src)]
        total.append(((w[a] * (nxt - x)) ** 2).reshape(-1))
    return np.concatenate(total)


# -------------------------------------------------------------------------- tap sets
# covariance (and spacing) whose three axes give `ntaps` taps each and different taps:
# half = ceil(3 sqrt(cov_aa) / spacing_a) is the same on every axis
GAUSS_ANISO = {
    3: (np.diag([0.05, 0.08, 0.10]), None),
    5: (np.diag([0.30, 0.38, 0.44]), None),
    7: (np.diag([0.5, 0.8, 1.0]), None),
    9: (np.diag([1.1, 1.4, 1.7]), None),
    11: (np.diag([1.9, 2.3, 2.7]), None),
    13: (np.diag([3.0, 3.6, 4.0]), None),
    15: (np.diag([4.2, 4.8, 5.4]), None),
    17: (np.diag([5.5, 6.5, 7.0]), None),
}
# the issue's fourth confirmed row: an isotropic covariance on an anisotropic grid
GAUSS_SPACING_13 = (np.diag([4.0, 4.0, 4.0]), np.array([1.0, 1.05, 1.1]))

KINDS = ("gauss_aniso", "sym_signed", "asym", "iso32")
SYMMETRIC = {"gauss_aniso": True, "gauss_spacing": True, "sym_signed": True, "asym": False,
             "iso32": True}


def gaussian_operator(cov, spacing=None):
    import nsol_amd.linear_operators as LO
    lo = LO.LinearOperators3D() if spacing is None else LO.LinearOperators3D(spacing=spacing)
    return lo.get_gaussian_blurring_operators(cov)[0]


_TAPS = {}


def taps(kind, ntaps):
    """(tz, ty, tx): float64 taps of the array axes 0, 1, 2."""
    key = (kind, ntaps)
    if key in _TAPS:
        return _TAPS[key]
    rng = np.random.default_rng(5100 + 17 * ntaps + KINDS.index(kind) if kind in KINDS else 7)
    R = ntaps // 2
    if kind in ("gauss_aniso", "gauss_spacing"):
        cov, sp = GAUSS_ANISO[ntaps] if kind == "gauss_aniso" else GAUSS_SPACING_13
        A = gaussian_operator(cov, sp)
        out = tuple(np.array(A._passes[a][1], dtype=np.float64) for a in range(3))
    elif kind == "sym_signed":
        out = []
        for _ in range(3):
            h = rng.standard_normal(R + 1)
            h[0] = 1.0 + abs(h[0])                       # the centre
            h[1:] *= 0.6
            h[R] = -abs(h[R]) - 0.05                     # a negative side lobe at the rim
            out.append(np.concatenate([h[:0:-1], h]))
        out = tuple(out)
    elif kind == "asym":
        out = tuple(rng.standard_normal(ntaps) for _ in range(3))
    elif kind == "iso32":
        k = np.arange(-R, R + 1, dtype=np.float64)
        base = np.exp(-0.5 * k * k / (0.11 * ntaps * ntaps / 9.0 + 0.2))
        base = rounded(base / base.sum(), np.float32)    # exact in float32
        base[R + 1:] = base[:R][::-1]
        # (a common factor on a whole set would commute between the axes: the relative
        # change differs from tap to tap, far below half a float32 ulp)
        out = (base.copy(), base * (1.0 + 2.0 ** -30 * np.abs(k) / R),
               base * (1.0 - 2.0 ** -30 * (k / R) ** 2))
    else:
        raise ValueError(kind)
    assert all(t.size == ntaps for t in out), (kind, ntaps, [t.size for t in out])
    _TAPS[key] = out
    return out


def is_symmetric(ts, dtype):
    return all(np.array_equal(t.astype(dtype), t.astype(dtype)[::-1]) for t in ts)


def is_iso(ts, dtype):
    """What launch_blur3_dma computes as `iso`: the three sets equal after the cast."""
    tz, ty, tx = (t.astype(dtype) for t in ts)
    return bool(np.array_equal(tz, tx) and np.array_equal(ty, tx))


# ---------------------------------------------------------------------------- shapes
def dma_rag_bound(dtype, ntaps):
    """Shortest ragged / off-grid row the DMA kernel takes: (16 + 2 ceil(R / VEC)) VEC."""
    V, R = vec(dtype), ntaps // 2
    return (DMA_LANES + 2 * -(-R // V)) * V


def reg_rag_bound(dtype, ntaps):
    return 2 * ntaps + 2 * vec(dtype)


def shapes(dtype, ntaps):
    """{name: (shape, offset)}: the smallest shapes that cross each structure of the
    kernels for this type and tap count (offset: elements off the 16-byte grid)."""
    V = vec(dtype)
    b = dma_rag_bound(dtype, ntaps)
    out = {
        # one tile, smaller than the halo on z and y (13 - 17 taps: R > nz, R > ny)
        "tiny": ((3, 5, 16), 0),
        # two tile rows, two tile columns, aligned
        "tiles": ((7, 66, 68) if V == 4 else (7, 66, 36), 0),
        # operands one element off the grid (a ragged DMA form: rows at the bound)
        "offgrid": ((5, 9, 80) if V == 4 else (5, 9, 48), 1),
    }
    # ragged DMA rows one above the bound: every remainder; one with ny = 65
    for r in range(1, V):
        out["rag%d" % r] = ((4, 65, b + r) if r == V // 2 else (5, 9, b + r), 0)
    # ragged rows below the DMA bound, at or above the register kernels' bound
    nxr = 45 if V == 4 else 31
    if 5 <= ntaps <= (13 if V == 4 else 11) and reg_rag_bound(dtype, ntaps) <= nxr < b:
        out["ragreg"] = ((5, 9, nxr), 0)
    return out


ZCHUNKS = (1, 4)                       # on "tiles" (nz = 7): seams after every plane / 4 + 3


def spike_sites(shape, dtype):
    """Voxels that carry a spike: the two corners, the ends of a row's last (partial)
    vector, both sides of every tile seam in x and y."""
    nz, ny, nx = shape
    V = vec(dtype)
    tw = DMA_LANES * V
    sites = [(0, 0, 0), (nz - 1, ny - 1, nx - 1)]
    last = (nx - 1) // V * V                               # first element of the last vector
    zc, yc = nz // 2, ny // 2
    sites += [(zc, yc, last), (min(zc + 1, nz - 1), max(yc - 1, 0), nx - 1)]
    for k, xs in enumerate(range(tw, nx, tw)):
        sites += [(k % nz, (3 + k) % ny, xs - 1), ((k + 1) % nz, (5 + k) % ny, xs)]
    for k, ys in enumerate(range(DMA_ROWS, ny, DMA_ROWS)):
        sites += [((k + 2) % nz, ys - 1, (7 + k) % nx), ((k + 3) % nz, ys, (11 + k) % nx)]
    seen, out = set(), []
    for s in sites:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def volume(shape, dtype, salt=0):
    """Noise plus a ramp along each axis plus the spikes, rounded to dtype, in float64."""
    nz, ny, nx = shape
    rng = np.random.default_rng(9000 + 31 * salt + (nz * 131 + ny) * 137 + nx)
    x = rng.standard_normal(shape)
    z, y, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    x += 0.30 * z / max(nz - 1, 1) - 0.45 * y / max(ny - 1, 1) + 0.60 * xx / max(nx - 1, 1)
    for k, s in enumerate(spike_sites(shape, dtype)):
        x[s] = SPIKE * (1.0 + 0.125 * (k % 5)) * (-1.0 if k % 3 == 1 else 1.0)
    return rounded(x, dtype)


# ------------------------------------------------------------------ planted mistakes
MISTAKES = ("swap_zy", "swap_yx", "reverse_x", "reverse_z", "wrap_x", "seam_row", "tap_2^-12")


def mistaken(name, x, tz, ty, tx):
    """reference() with one mistake of a kernel planted; None where it is no mistake."""
    x = np.asarray(x, dtype=np.float64)
    nz, ny, nx = x.shape
    if name == "swap_zy":
        return reference(x, ty, tz, tx)
    if name == "swap_yx":
        return reference(x, tz, tx, ty)
    if name == "reverse_x":
        return None if np.array_equal(tx, tx[::-1]) else reference(x, tz, ty, tx[::-1])
    if name == "reverse_z":
        return None if np.array_equal(tz, tz[::-1]) else reference(x, tz[::-1], ty, tx)
    if name == "wrap_x":
        # the first halo element behind the row's end read as x[nx - 1] in place of x[0]
        R = tx.size // 2
        out = np.zeros_like(x)
        i = np.arange(nx)
        for t in range(tx.size):
            j = i + t - R
            src = np.where(j == nx, nx - 1, j % nx)
            out += tx[t] * np.take(x, src, axis=2)
        return corr_axis(corr_axis(out, ty, 1), tz, 0)
    if name == "seam_row":
        # the row at the tile seam (the last row where there is one tile row) taken from
        # the next plane
        if nz < 2:
            return None
        ys = DMA_ROWS if ny > DMA_ROWS else ny - 1
        bad = x.copy()
        bad[:, ys, :] = np.roll(x, -1, axis=0)[:, ys, :]
        return reference(bad, tz, ty, tx)
    if name == "tap_2^-12":
        t2 = tx.copy()
        t2[int(np.argmax(np.abs(tx)))] *= 1.0 + 2.0 ** -12
        return reference(x, tz, ty, t2)
    raise ValueError(name)


# ----------------------------------------------------- which entry point answers what
FORMS = ("plain", "axpby", "norms", "lanczos_a", "lanczos_b", "lanczos_a2", "lanczos_b2",
         "loss")
EPI = {"plain": 0, "axpby": 1, "norms": 2, "lanczos_a": 3, "lanczos_b": 4, "loss": 5,
       "lanczos_a2": 2, "lanczos_b2": 6}
LDS_LIMIT = 160 * 1024


def dma_lds(dtype, ntaps, epi, rag=False):
    """Bytes of LDS a k_blur3_dma workgroup asks for (launch_blur3_dma: three raw tiles in
    whole 1-KiB pieces, two x-filtered tiles, the epilogue's own-position tiles, the
    ragged form's patch slots); above 160 KiB the launcher returns -2."""
    V, R = vec(dtype), ntaps // 2
    nbh = -(-R // V)
    frows = DMA_ROWS + 2 * R
    npieces = -(-frows * (DMA_LANES + 2 * nbh) // 64)
    base = 3 * npieces * 64 + 2 * frows * DMA_LANES
    tile = DMA_ROWS * DMA_LANES
    if epi == 6:
        mini = (base + tile + 16 * 128) * 16 <= LDS_LIMIT
        own = tile + (16 * 128 if mini else -(-(DMA_ROWS + 2) * (DMA_LANES + 2) // 64) * 64)
    else:
        own = 2 * tile if epi in (1, 3, 4, 5) else 0
    return (base + own) * 16 + (3 * -(-frows * 4 // 64) * 256 if rag else 0)


def applies(form, dtype, shape, ntaps, symmetric, aligned, dma=True, dma_rag=True):
    """The kernel that answers, or None where the entry point returns -2 (nothing
    launched): "dma", "dma_rag", "reg" (k_blur3_wrap), "reg_pp2", "reg_pp1_rag"
    (k_blur3_wrap_pp).  include/nsol_hip.h and the conditions of corr3_impl,
    corr3_axpby_impl, lanczos_taps, lanczos_a2_impl and launch_blur3_dma.
    aligned: x and out on the 16-byte grid; dma / dma_rag: the knobs corr_blur3_dma and
    corr_blur3_dma_rag."""
    nz, ny, nx = shape
    f64 = np.dtype(dtype) == np.float64
    V = vec(dtype)
    if ntaps % 2 == 0 or ntaps < 3 or ntaps > 17:
        return None
    ragged = nx % V != 0
    rag = ragged or not aligned

    def dma_form(rag_ok=True):
        if not (dma and symmetric):
            return None
        if rag and not (rag_ok and dma_rag and nx >= dma_rag_bound(dtype, ntaps)):
            return None
        if dma_lds(dtype, ntaps, EPI[form], rag) > LDS_LIMIT:
            return None
        return "dma_rag" if rag else "dma"

    if form == "plain":
        if ragged and nx < reg_rag_bound(dtype, ntaps):
            return None
        got = dma_form()
        if got:
            return got
        if not aligned:
            return None
        if 5 <= ntaps <= (11 if f64 else 13):
            return "reg_pp1_rag" if ragged else "reg_pp2"
        return None if ragged else "reg"                  # 3, 15, 17 (float64: 13 too)
    if form == "axpby":                                    # (float64, 15 / 17 taps: no LDS
        return dma_form()                                  # left for the io tiles)
    if form == "norms":
        if f64 and ntaps >= 15:
            return None
        return dma_form(rag_ok=ntaps < 17)
    if form in ("lanczos_a", "lanczos_b", "loss"):
        if ntaps < 5 or ntaps > (9 if f64 else 13):
            return None
        return dma_form(rag_ok=False)
    if form in ("lanczos_a2", "lanczos_b2"):
        if ntaps < 5 or ntaps > (11 if f64 else 13):
            return None
        return dma_form(rag_ok=False)
    raise ValueError(form)
