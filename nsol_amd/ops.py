"""Device-tensor front end of the C ABI (include/nsol_hip.h).

Every function takes/returns contiguous torch HIP tensors of float32 or
float64 and launches hand-written kernels from libnsol_hip.so on the current
torch stream.  No arithmetic is done by torch itself.
"""
import numpy as np
import torch

from . import _lib, _timing
from .device import suffix, stream_ptr, empty_like

MODES = {"constant": 0, "wrap": 1, "nearest": 2, "reflect": 3, "mirror": 4}
LOSSES = {"linear": 0, "soft_l1": 1, "huber": 2, "cauchy": 3, "arctan": 4}
PD_REG_TV, PD_REG_HUBER, PD_DATA_L2, PD_DATA_L1 = 0, 1, 0, 2
# or-ed with PD_REG_TV / PD_REG_HUBER: the dual projection divides the voxel's
# whole gradient vector by max(1, its Euclidean norm) (NSOL_PD_REG_ISOTROPIC)
PD_REG_ISOTROPIC = 4
# or-ed with PD_DATA_L2 / PD_DATA_L1: the data term carries per-voxel weights
# (NSOL_PD_DATA_WEIGHTED); pd_weighted_run / pd_weighted_iter alone take it
PD_DATA_WEIGHTED = 8


def _fn(name, t):
    fn = getattr(_lib.load(), "nsol_%s_%s" % (name, suffix(t)))
    kt = _timing.active()              # (measurement only: bench.py / bench_admm.py)
    return fn if kt is None else kt.wrap(name, fn)


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
        raise TypeError("expected a contiguous HIP device tensor")
    return t


_bump = torch.autograd.graph.increment_version


def _wrote(first, *more):
    """The kernels write through raw pointers, which torch cannot see: count the
    write on the tensors' version counters (views share their base's).  That counter
    is what the caches of b / x_scale, A^T b and |b|^2 are keyed on
    (nsol_amd/_caches.py).  Returns its first argument."""
    if first is not None:
        _bump(first)
    for t in more:
        if t is not None:
            _bump(t)
    return first


def _same(x, *others):
    """Multi-operand kernels take their launch geometry and element type from
    the first operand: every other operand must be a contiguous device tensor
    of the same dtype and length, or the kernel would read out of bounds /
    reinterpret the bytes."""
    _chk(x)
    for t in others:
        _chk(t)
        if t.dtype != x.dtype or t.numel() != x.numel():
            raise ValueError(
                "operand mismatch: %s[%d] against %s[%d]" %
                (str(t.dtype), t.numel(), str(x.dtype), x.numel()))
    return x


def dims3(shape):
    """(ndim, nz, ny, nx) of an N-D volume shape (N = 1, 2, 3)."""
    shape = tuple(int(s) for s in shape)
    nd = len(shape)
    if nd == 1:
        return 1, 1, 1, shape[0]
    if nd == 2:
        return 2, 1, shape[0], shape[1]
    if nd == 3:
        return 3, shape[0], shape[1], shape[2]
    raise ValueError("only 1-D, 2-D and 3-D volumes are supported")


def inv_spacing(spacing, ndim):
    """(wx, wy, wz) = 1/spacing; spacing[0] belongs to the LAST array axis
    (reference kernels.py:240-286)."""
    sp = np.atleast_1d(spacing).astype(float)
    w = [1.0, 1.0, 1.0]
    for a in range(ndim):
        w[a] = 1.0 / sp[a]
    return tuple(w)


# ------------------------------------------------------------ operators ----
def grad(x, shape, w, out=None):
    _chk(x)
    ndim, nz, ny, nx = dims3(shape)
    if out is None:
        out = empty_like(x, ndim * x.numel())
    _lib.check(_fn("grad", x)(_p(x), _p(out), ndim, nz, ny, nx, w[0], w[1],
                              w[2], stream_ptr()), "nsol_grad")
    return _wrote(out)


def grad_adj(p, shape, w, out=None):
    _chk(p)
    ndim, nz, ny, nx = dims3(shape)
    if out is None:
        out = empty_like(p, nz * ny * nx)
    _lib.check(_fn("grad_adj", p)(_p(p), _p(out), ndim, nz, ny, nx, w[0], w[1],
                                  w[2], stream_ptr()), "nsol_grad_adj")
    return _wrote(out)


def grad_adj_axpy(p, x, tau, shape, w, out=None):
    """x - tau * grad_adj(p) in one pass."""
    _chk(p)
    _chk(x)
    ndim, nz, ny, nx = dims3(shape)
    if p.dtype != x.dtype or x.numel() != nz * ny * nx or \
            p.numel() != ndim * x.numel():
        raise ValueError("operand mismatch: p %s[%d], x %s[%d] for shape %r" %
                         (str(p.dtype), p.numel(), str(x.dtype), x.numel(),
                          tuple(shape)))
    if out is None:
        out = empty_like(x)
    _lib.check(_fn("grad_adj_axpy", p)(_p(p), _p(x), _p(out), ndim, nz, ny, nx,
                                       w[0], w[1], w[2], float(tau),
                                       stream_ptr()), "nsol_grad_adj_axpy")
    return _wrote(out)


def extrapolate(a, b, theta, out=None):
    """a + theta * (a - b) (the over-relaxation step, the reference's rounding)."""
    _same(a, b)
    if out is None:
        out = empty_like(a)
    _lib.check(_fn("extrapolate", a)(_p(out), _p(a), _p(b), float(theta),
                                     a.numel(), stream_ptr()), "nsol_extrapolate")
    return _wrote(out)


def diff_axis(x, shape, direction, adjoint, w):
    _chk(x)
    _, nz, ny, nx = dims3(shape)
    out = empty_like(x)
    _lib.check(_fn("diff_axis", x)(_p(x), _p(out), int(direction),
                                   int(bool(adjoint)), nz, ny, nx, float(w),
                                   stream_ptr()), "nsol_diff_axis")
    return _wrote(out)


def corr_axis(x, shape, axis3, taps, centre, mode, out=None):
    """1-D correlation along axis3 (0=z,1=y,2=x of the padded 3-D shape)."""
    _chk(x)
    _, nz, ny, nx = dims3(shape)
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    if out is None:
        out = empty_like(x)
    _lib.check(_fn("corr_axis", x)(
        _p(x), _p(out), int(axis3), nz, ny, nx, taps.ctypes.data,
        int(taps.size), int(centre), MODES[mode], stream_ptr()),
        "nsol_corr_axis")
    return _wrote(out)


SAMPLED_MODES = ("wrap", "constant")


def sampled_extent(length, factor, offset):
    """Samples that [offset::factor] keeps of `length`: ceil((length - offset) / factor)."""
    return -((int(offset) - int(length)) // int(factor))


def _sampled_call(name, src, shape, axis3, taps, centre, mode, factor, offset, out, up):
    _chk(src)
    _, nz, ny, nx = dims3(shape)
    if mode not in SAMPLED_MODES:
        raise ValueError("%s: mode '%s' has no transpose that is a correlation "
                         "(supported: wrap, constant)" % (name, mode))
    factor, offset = int(factor), int(offset)
    full = (nz, ny, nx)
    if int(axis3) not in (0, 1, 2):
        raise ValueError("%s: axis3 must be 0, 1 or 2" % name)
    length = full[int(axis3)]
    if factor < 1 or not 0 <= offset < min(factor, length):
        raise ValueError("%s: factor %d, offset %d on an axis of extent %d" %
                         (name, factor, offset, length))
    coarse = list(full)
    coarse[int(axis3)] = sampled_extent(length, factor, offset)
    n_full, n_coarse = nz * ny * nx, coarse[0] * coarse[1] * coarse[2]
    n_in, n_out = (n_coarse, n_full) if up else (n_full, n_coarse)
    if src.numel() != n_in:
        raise ValueError("operand mismatch: %d elements for the %d of shape %r" %
                         (src.numel(), n_in, tuple(shape)))
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    if out is None:
        out = empty_like(src, n_out)
    else:
        _chk(out)
        if out.dtype != src.dtype or out.numel() != n_out:
            raise ValueError("operand mismatch: out %s[%d], expected %s[%d]" %
                             (str(out.dtype), out.numel(), str(src.dtype), n_out))
    _lib.check(_fn(name, src)(
        _p(src), _p(out), int(axis3), nz, ny, nx, taps.ctypes.data, int(taps.size),
        int(centre), MODES[mode], factor, offset, stream_ptr()), "nsol_" + name)
    return _wrote(out)


def corr_axis_down(x, shape, axis3, taps, centre, mode, factor, offset, out=None):
    """corr_axis followed by [offset::factor] along axis3, computing only the samples
    it keeps.  shape: the FULL-RESOLUTION volume x holds; the result has
    sampled_extent(...) along axis3.  mode: "wrap" or "constant"."""
    return _sampled_call("corr_axis_down", x, shape, axis3, taps, centre, mode, factor,
                         offset, out, False)


def corr_axis_up(q, shape, axis3, taps, centre, mode, factor, offset, out=None):
    """The exact transpose of corr_axis_down with the same arguments (taps: the FORWARD
    taps).  shape: the FULL-RESOLUTION volume of the result; q holds the sampled one."""
    return _sampled_call("corr_axis_up", q, shape, axis3, taps, centre, mode, factor,
                         offset, out, True)


def corr3_wrap(x, shape, taps_z, taps_y, taps_x, out=None):
    """Separable periodic 3-D correlation in one pass (passes x, y, z); returns
    None when the fused kernel does not apply (nothing was launched)."""
    _chk(x)
    _, nz, ny, nx = dims3(shape)
    tz, ty, tx = (np.ascontiguousarray(t, dtype=np.float64)
                  for t in (taps_z, taps_y, taps_x))
    if not (tz.size == ty.size == tx.size):
        return None
    if out is None:
        out = empty_like(x)
    rc = _fn("corr3_wrap", x)(_p(x), _p(out), nz, ny, nx, tz.ctypes.data,
                              ty.ctypes.data, tx.ctypes.data, int(tz.size),
                              stream_ptr())
    if rc == -2:
        return None
    _lib.check(rc, "nsol_corr3_wrap")
    return _wrote(out)


def corr3_wrap_axpby(x, io, shape, taps_z, taps_y, taps_x, ca, cb, sync=True,
                     result=None):
    """io = ca * blur(x) + cb * io in place (the blur's epilogue; A x never goes
    to memory); returns the sum of squares of the new io, or None when the
    LDS-DMA staged kernel does not apply (nothing was launched).  result: a
    one-element float64 device tensor of the caller's that receives the sum
    instead (returned as it is, not read back)."""
    _same(x, io)
    _, nz, ny, nx = dims3(shape)
    tz, ty, tx = (np.ascontiguousarray(t, dtype=np.float64)
                  for t in (taps_z, taps_y, taps_x))
    if not (tz.size == ty.size == tx.size):
        return None
    ws, res = _workspace(x.device)
    if result is not None:
        res, sync = result, False
    rc = _fn("corr3_wrap_axpby", x)(
        _p(x), _p(io), nz, ny, nx, tz.ctypes.data, ty.ctypes.data, tx.ctypes.data,
        int(tz.size), float(ca), float(cb), _p(res), _p(ws), int(ws.numel()),
        stream_ptr())
    if rc == -2:
        return None
    _lib.check(rc, "nsol_corr3_wrap_axpby")
    _wrote(io)
    return float(res.item()) if sync else res


def corr3_wrap_norms(x, out, shape, taps_z, taps_y, taps_x, w, result):
    """out = blur(x) with result[0] = sum out^2 and result[1] = sum |grad x|^2 of the
    INPUT (weights w = inverse spacings as for tk1_grad_norm), both taken by the blur
    itself; result: a two-element float64 device tensor of the caller's (returned, not
    read back).  None when that kernel does not apply (nothing was launched)."""
    _same(x, out)
    _chk(result)
    if result.numel() != 2 or str(result.dtype) != "torch.float64":
        raise ValueError("corr3_wrap_norms: result must hold two float64 values")
    ndim, nz, ny, nx = dims3(shape)
    tz, ty, tx = (np.ascontiguousarray(t, dtype=np.float64)
                  for t in (taps_z, taps_y, taps_x))
    if nz * ny * nx != x.numel():
        raise ValueError("corr3_wrap_norms: %d elements for shape %r" %
                         (x.numel(), tuple(shape)))
    if ndim != 3 or not (tz.size == ty.size == tx.size):
        return None
    ws, _ = _workspace(x.device)
    rc = _fn("corr3_wrap_norms", x)(
        _p(x), _p(out), nz, ny, nx, tz.ctypes.data, ty.ctypes.data, tx.ctypes.data,
        int(tz.size), float(w[0]), float(w[1]), float(w[2]), _p(result), _p(ws),
        int(ws.numel()), stream_ptr())
    if rc == -2:
        return None
    _lib.check(rc, "nsol_corr3_wrap_norms")
    _wrote(out)
    return result


class LanczosBoard(object):
    """Device scalars of an LSMR solve run as Lanczos on the normal equations with both
    halves of a step taken by the blur (nsol_corr3_wrap_lanczos_*): the sums of every
    step (board: |y_j|^2, |A y_j|^2, |grad y_j|^2 at 3 j ..) and the coefficients the
    next kernel reads (coef).  The host reads the board when it needs the scalars --
    the kernels never wait for it."""

    def __init__(self, like, steps, rho_grad, rho_ident):
        self.steps = int(steps)
        self.rho_grad, self.rho_ident = float(rho_grad), float(rho_ident)
        self.board = torch.zeros(3 * (self.steps + 2), dtype=torch.float64,
                                 device=like.device)
        self.coef = torch.zeros(8, dtype=like.dtype, device=like.device)

    def slot_norm2(self, j):
        """The one-element view |y_j|^2 lands in (a reduction kernel's `result`)."""
        return self.board[3 * j:3 * j + 1]

    def init(self):
        _lib.check(_fn("corr3_wrap_lanczos_init", self.coef)(
            _p(self.board), _p(self.coef), self.rho_grad, self.rho_ident, stream_ptr()),
            "nsol_corr3_wrap_lanczos_init")


def corr3_lanczos_a(y, y_prev, t, q0, shape, taps_z, taps_y, taps_x, lb, step):
    """First half of Lanczos step `step` (see LanczosBoard): t = blur(y), q0 = c1 K'K y +
    c0 y + c2 y_prev, sums onto the board.  False when the kernel does not apply
    (nothing launched)."""
    _same(y, t, q0)
    if y_prev is not None:
        _same(y, y_prev)
    ndim, nz, ny, nx = dims3(shape)
    tz, ty, tx = (np.ascontiguousarray(v, dtype=np.float64)
                  for v in (taps_z, taps_y, taps_x))
    if ndim != 3 or nz * ny * nx != y.numel() or not (tz.size == ty.size == tx.size):
        return False
    ws, _ = _workspace(y.device)
    rc = _fn("corr3_wrap_lanczos_a", y)(
        _p(y), _p(y_prev), _p(t), _p(q0), nz, ny, nx, tz.ctypes.data, ty.ctypes.data,
        tx.ctypes.data, int(tz.size), lb.rho_grad, lb.rho_ident, _p(lb.board), int(step),
        _p(lb.coef), _p(ws), int(ws.numel()), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_corr3_wrap_lanczos_a")
    _wrote(t, q0)
    return True


# True: the halves of a Lanczos step as nsol_corr3_wrap_lanczos_a2 / _b2 (no q0 array:
# the second half forms the step's K'K y itself; 25 B per voxel and step instead of 33)
LEAN_LANCZOS_HALVES = True


def corr3_lanczos_a2(y, t, shape, taps_z, taps_y, taps_x, lb, step):
    """First half, lean form: t = blur(y), its two sums onto the board, the second
    half's coefficients.  False when the kernel does not apply (nothing launched)."""
    _same(y, t)
    ndim, nz, ny, nx = dims3(shape)
    tz, ty, tx = (np.ascontiguousarray(v, dtype=np.float64)
                  for v in (taps_z, taps_y, taps_x))
    if ndim != 3 or nz * ny * nx != y.numel() or not (tz.size == ty.size == tx.size):
        return False
    ws, _ = _workspace(y.device)
    rc = _fn("corr3_wrap_lanczos_a2", y)(
        _p(y), _p(t), nz, ny, nx, tz.ctypes.data, ty.ctypes.data, tx.ctypes.data,
        int(tz.size), lb.rho_grad, lb.rho_ident, _p(lb.board), int(step), _p(lb.coef),
        _p(ws), int(ws.numel()), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_corr3_wrap_lanczos_a2")
    _wrote(t)
    return True


def corr3_lanczos_b2(t, y, y_prev, y_new, shape, taps_z, taps_y, taps_x, lb, step):
    """Second half, lean form: y_new = ca blur(t) + (c1 K'K y + c0 y + c2 y_prev) + cy y
    with |y_new|^2 onto the board (y_prev may be None; y_new None: the sum alone)."""
    _same(t, y)
    if y_new is not None:
        _same(t, y_new)
    if y_prev is not None:
        _same(y, y_prev)
    ndim, nz, ny, nx = dims3(shape)
    tz, ty, tx = (np.ascontiguousarray(v, dtype=np.float64)
                  for v in (taps_z, taps_y, taps_x))
    if ndim != 3 or nz * ny * nx != y.numel() or not (tz.size == ty.size == tx.size):
        return False
    ws, _ = _workspace(y.device)
    rc = _fn("corr3_wrap_lanczos_b2", y)(
        _p(t), _p(y), _p(y_prev), _p(y_new), nz, ny, nx, tz.ctypes.data, ty.ctypes.data,
        tx.ctypes.data, int(tz.size), lb.rho_grad, lb.rho_ident, _p(lb.board), int(step),
        _p(lb.coef), _p(ws), int(ws.numel()), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_corr3_wrap_lanczos_b2")
    _wrote(y_new)
    return True


def corr3_wrap_loss(x, b, shape, taps_z, taps_y, taps_x, loss, f_scale, result):
    """rho'(r^2) r for r = blur(x) - b with 1/2 sum rho(r^2) in result[0] (the caller's
    device slot), from the blur itself; None when that kernel does not apply (nothing
    launched): then corr3_wrap and loss_cost_grad(minus=b)."""
    _same(x, b)
    ndim, nz, ny, nx = dims3(shape)
    tz, ty, tx = (np.ascontiguousarray(v, dtype=np.float64)
                  for v in (taps_z, taps_y, taps_x))
    if ndim != 3 or nz * ny * nx != x.numel() or not (tz.size == ty.size == tx.size):
        return None
    ws, _ = _workspace(x.device)
    g = empty_like(x)
    rc = _fn("corr3_wrap_loss", x)(
        _p(x), _p(b), _p(g), nz, ny, nx, tz.ctypes.data, ty.ctypes.data, tx.ctypes.data,
        int(tz.size), LOSSES[loss], float(f_scale), _p(result), _p(ws), int(ws.numel()),
        stream_ptr())
    if rc == -2:
        return None
    _lib.check(rc, "nsol_corr3_wrap_loss")
    return g


def corr3_lanczos_b(t, q0, y, y_new, shape, taps_z, taps_y, taps_x, lb, step):
    """Second half: y_new = ca blur(t) + q0 + cy y with |y_new|^2 onto the board."""
    _same(t, q0, y, y_new)
    ndim, nz, ny, nx = dims3(shape)
    tz, ty, tx = (np.ascontiguousarray(v, dtype=np.float64)
                  for v in (taps_z, taps_y, taps_x))
    if ndim != 3 or nz * ny * nx != y.numel() or not (tz.size == ty.size == tx.size):
        return False
    ws, _ = _workspace(y.device)
    rc = _fn("corr3_wrap_lanczos_b", y)(
        _p(t), _p(q0), _p(y), _p(y_new), nz, ny, nx, tz.ctypes.data, ty.ctypes.data,
        tx.ctypes.data, int(tz.size), lb.rho_grad, lb.rho_ident, _p(lb.board), int(step),
        _p(lb.coef), _p(ws), int(ws.numel()), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_corr3_wrap_lanczos_b")
    _wrote(y_new)
    return True


def corr_dense(x, shape, taps_dev, kshape3, centre3, mode):
    _chk(x)
    _chk(taps_dev)
    _, nz, ny, nx = dims3(shape)
    out = empty_like(x)
    _lib.check(_fn("corr_dense", x)(
        _p(x), _p(out), nz, ny, nx, _p(taps_dev), kshape3[0], kshape3[1],
        kshape3[2], centre3[0], centre3[1], centre3[2], MODES[mode],
        stream_ptr()), "nsol_corr_dense")
    return _wrote(out)


def corr_dense_tiled_plan(shape, kshape3, elem_size, tile=(0, 0, 0)):
    """The tiled dense correlation's plan for a volume shape, a tap shape (kz, ky, kx) and
    an element size (4 or 8) without launching: a dict with ty, tx, slab, lds_bytes, ntx,
    nty, nslab, blocks -- or None where nsol_corr_dense_tiled_* declines (then
    corr_dense answers).  tile: forced (ty, tx, slab), 0 = the planner's choice."""
    import ctypes
    _, nz, ny, nx = dims3(shape)
    plan = (ctypes.c_int64 * 8)()
    rc = _lib.load().nsol_corr_dense_tiled_plan(
        nz, ny, nx, int(kshape3[0]), int(kshape3[1]), int(kshape3[2]), int(elem_size),
        int(tile[0]), int(tile[1]), int(tile[2]), ctypes.addressof(plan))
    if rc == -2:
        return None
    _lib.check(rc, "nsol_corr_dense_tiled_plan")
    return dict(zip(("ty", "tx", "slab", "lds_bytes", "ntx", "nty", "nslab", "blocks"),
                    (int(v) for v in plan)))


def corr_dense_tiled(x, shape, taps_dev, kshape3, centre3, mode, tile=(0, 0, 0),
                     out=None):
    """corr_dense through the tiled kernel (k_corr_dense_tile), bit-identical to it;
    None, with nothing launched, where that kernel declines.  tile: forced
    (ty, tx, slab), 0 = the planner's choice; out: where the result goes (it must not
    overlap x)."""
    _chk(x)
    _chk(taps_dev)
    _, nz, ny, nx = dims3(shape)
    if nz * ny * nx != x.numel() or taps_dev.dtype != x.dtype or \
            taps_dev.numel() != int(kshape3[0]) * int(kshape3[1]) * int(kshape3[2]):
        raise ValueError("operand mismatch: shape %r on x[%d], %r taps in [%d]" %
                         (tuple(shape), x.numel(), tuple(kshape3), taps_dev.numel()))
    if any(not 0 <= int(c) < int(k) for c, k in zip(centre3, kshape3)):
        raise ValueError("nsol_corr_dense_tiled: centre %r outside the kernel %r" %
                         (tuple(centre3), tuple(kshape3)))
    if out is not None:
        _same(x, out)
    elif corr_dense_tiled_plan(shape, kshape3, x.element_size(), tile) is None:
        return None                      # (the planner is host code: nothing allocated)
    else:
        out = empty_like(x)
    rc = _fn("corr_dense_tiled", x)(
        _p(x), _p(out), nz, ny, nx, _p(taps_dev), int(kshape3[0]), int(kshape3[1]),
        int(kshape3[2]), int(centre3[0]), int(centre3[1]), int(centre3[2]), MODES[mode],
        int(tile[0]), int(tile[1]), int(tile[2]), stream_ptr())
    if rc == -2:
        return None
    _lib.check(rc, "nsol_corr_dense_tiled")
    return _wrote(out)


# --------------------------------------------------------- element-wise ----
def lincomb2(a, x, b, y, out=None):
    _same(x, y)
    if out is None:
        out = empty_like(x)
    else:
        _same(x, out)
    _lib.check(_fn("lincomb2", x)(_p(out), float(a), _p(x), float(b), _p(y),
                                  x.numel(), stream_ptr()), "nsol_lincomb2")
    return _wrote(out)


def lincomb3(a, x, b, y, c, z, out=None):
    _same(x, y, z)
    if out is None:
        out = empty_like(x)
    else:
        _same(x, out)
    _lib.check(_fn("lincomb3", x)(_p(out), float(a), _p(x), float(b), _p(y),
                                  float(c), _p(z), x.numel(), stream_ptr()),
               "nsol_lincomb3")
    return _wrote(out)


def lincomb_many(vecs, coefs, out=None, bounds=None):
    """sum_k coefs[k] * vecs[k] in one pass (up to 40 vectors; the terms are added
    in order): nsol_lb_wcomb_* without base vectors or mask.  bounds = (lo, hi): the
    sum clipped to them in the same pass (nsol_lincomb_clip_*)."""
    import ctypes
    x = _same(vecs[0], *vecs[1:])
    if len(vecs) != len(coefs) or len(vecs) > 40:
        raise ValueError("lincomb_many: %d vectors, %d coefficients"
                         % (len(vecs), len(coefs)))
    if out is None:
        out = empty_like(x)
    else:
        _same(x, out)
    ptrs = (ctypes.c_void_p * len(vecs))(*[v.data_ptr() for v in vecs])
    co = np.ascontiguousarray(coefs, dtype=np.float64)
    if bounds is not None:
        lo, hi = _clip_bounds(x, bounds[0], bounds[1])       # (as clip() has them)
        if lo <= hi:
            _lib.check(_fn("lincomb_clip", x)(
                _p(out), x.numel(), len(vecs), ctypes.cast(ptrs, ctypes.c_void_p),
                co.ctypes.data, lo, hi, stream_ptr()), "nsol_lincomb_clip")
            return _wrote(out)
        return clip(lincomb_many(vecs, coefs, out=out), bounds[0], bounds[1], out=out)
    fn = getattr(_lib.load(), "nsol_lb_wcomb_%s" % suffix(x))
    kt = _timing.active()
    if kt is not None:
        fn = kt.wrap("lb_wcomb", fn)
    _lib.check(fn(_p(out), x.numel(), None, 1.0, 0, None, None, len(vecs),
                  ctypes.cast(ptrs, ctypes.c_void_p), co.ctypes.data,
                  stream_ptr()), "nsol_lb_wcomb")
    return _wrote(out)


def scale(x, a, divide=False, out=None):
    _chk(x)
    if out is None:
        out = empty_like(x)
    _lib.check(_fn("scale", x)(_p(out), _p(x), float(a), int(bool(divide)),
                               x.numel(), stream_ptr()), "nsol_scale")
    return _wrote(out)


def _clip_bounds(x, lo, hi):
    lo = -1.7976931348623157e308 if lo == -np.inf else float(lo)
    hi = 1.7976931348623157e308 if hi == np.inf else float(hi)
    if x.dtype == torch.float32:
        lo = max(lo, -3.4028234663852886e38)
        hi = min(hi, 3.4028234663852886e38)
    return lo, hi


def clip(x, lo, hi, out=None):
    _chk(x)
    if out is None:
        out = empty_like(x)
    lo, hi = _clip_bounds(x, lo, hi)
    _lib.check(_fn("clip", x)(_p(out), _p(x), lo, hi, x.numel(),
                              stream_ptr()), "nsol_clip")
    return _wrote(out)


def prox_dual_clamp(x, den=1.0, out=None):
    _chk(x)
    if out is None:
        out = empty_like(x)
    _lib.check(_fn("prox_dual_clamp", x)(_p(out), _p(x), float(den),
                                         x.numel(), stream_ptr()),
               "nsol_prox_dual_clamp")
    return _wrote(out)


def prox_dual_project(x, dim, den=1.0, out=None):
    """x holds `dim` blocks of x.numel() / dim elements; every voxel's vector
    (x / den) is divided by max(1, its Euclidean norm): the isotropic prox_tv_conj
    (den = 1) / prox_huber_conj (den = 1 + sigma * gamma)."""
    _chk(x)
    dim = int(dim)
    if dim < 1 or dim > 3:
        raise ValueError("dimension must be 1, 2 or 3, not %d" % dim)
    if x.numel() == 0 or x.numel() % dim:
        raise ValueError("%d elements are not %d blocks of equal length" %
                         (x.numel(), dim))
    if out is None:
        out = empty_like(x)
    else:
        _same(x, out)
    _lib.check(_fn("prox_dual_project", x)(_p(out), _p(x), float(den),
                                           x.numel() // dim, dim, stream_ptr()),
               "nsol_prox_dual_project")
    return _wrote(out)


def prox_ell2(x, bt, tau, out=None):
    _same(x, bt)
    if out is None:
        out = empty_like(x)
    _lib.check(_fn("prox_ell2", x)(_p(out), _p(x), _p(bt), float(tau),
                                   x.numel(), stream_ptr()), "nsol_prox_ell2")
    return _wrote(out)


def prox_ell1(x, bt, tau, out=None):
    _same(x, bt)
    if out is None:
        out = empty_like(x)
    _lib.check(_fn("prox_ell1", x)(_p(out), _p(x), _p(bt), float(tau),
                                   x.numel(), stream_ptr()), "nsol_prox_ell1")
    return _wrote(out)


def prox_ell2_weighted(x, bt, wt, tau, out=None):
    """(x + t bt) / (1 + t) with t = tau * wt per element; x where wt == 0."""
    _same(x, bt, wt)
    if out is None:
        out = empty_like(x)
    else:
        _same(x, out)
    _lib.check(_fn("prox_ell2_weighted", x)(_p(out), _p(x), _p(bt), _p(wt), float(tau),
                                            x.numel(), stream_ptr()),
               "nsol_prox_ell2_weighted")
    return _wrote(out)


def prox_ell1_weighted(x, bt, wt, tau, out=None):
    """Soft threshold of x - bt by t = tau * wt per element; x where wt == 0."""
    _same(x, bt, wt)
    if out is None:
        out = empty_like(x)
    else:
        _same(x, out)
    _lib.check(_fn("prox_ell1_weighted", x)(_p(out), _p(x), _p(bt), _p(wt), float(tau),
                                            x.numel(), stream_ptr()),
               "nsol_prox_ell1_weighted")
    return _wrote(out)


def prox_kl(x, bt, wt, tau, out=None):
    """The prox of the Poisson (Kullback-Leibler) term t (x - bt log x) with t = tau * wt
    per element (wt None: all 1), csrc/nsol_kl.hpp: never negative; x where wt == 0."""
    _same(x, bt)
    if wt is not None:
        _same(x, wt)
    if out is None:
        out = empty_like(x)
    else:
        _same(x, out)
    _lib.check(_fn("prox_kl", x)(_p(out), _p(x), _p(bt), _p(wt), float(tau), x.numel(),
                                 stream_ptr()), "nsol_prox_kl")
    return _wrote(out)


# ------------------------------------------------------------ reductions ----
_ws = {}


def _workspace(dev):
    key = (dev.index, stream_ptr())
    if key not in _ws:
        n = _lib.load().nsol_hip_reduce_ws_doubles()
        _ws[key] = (torch.empty(n, dtype=torch.float64, device=dev),
                    torch.empty(1, dtype=torch.float64, device=dev))
    return _ws[key]


def dot(x, y):
    """sum(x*y) accumulated in float64; returns a Python float (syncs)."""
    _same(x, y)
    ws, res = _workspace(x.device)
    _lib.check(_fn("dot", x)(_p(x), _p(y), x.numel(), _p(res), _p(ws),
                             stream_ptr()), "nsol_dot")
    return float(res.item())


def norm2(x):
    return float(np.sqrt(dot(x, x)))


def loss_cost_grad(r, loss, f_scale, want_grad=True, out=None, minus=None,
                   result=None):
    """(0.5*sum rho(r^2), rho'(r^2)*r); with `minus` the residual is r - minus,
    formed in the same pass.  result: the caller's one-element float64 device
    tensor for the cost (then nothing is read back and it is returned as it is)."""
    _chk(r)
    ws, res = _workspace(r.device)
    if result is not None:
        res = result
    g = None
    if want_grad:
        g = empty_like(r) if out is None else out
    if minus is None:
        _lib.check(_fn("loss_cost_grad", r)(
            _p(r), _p(g), r.numel(), LOSSES[loss], float(f_scale), _p(res),
            _p(ws), stream_ptr()), "nsol_loss_cost_grad")
    else:
        _same(r, minus)
        _lib.check(_fn("loss_residual_cost_grad", r)(
            _p(r), _p(minus), _p(g), r.numel(), LOSSES[loss], float(f_scale),
            _p(res), _p(ws), stream_ptr()), "nsol_loss_residual_cost_grad")
    return (res if result is not None else float(res.item())), _wrote(g)


def tk1_reg_cost_grad(x, g, shape, w, alpha, out=None, result=None):
    """(sum |grad x|^2, g + alpha * grad_adj(grad x)) in one pass over x
    (the regulariser's share of tikhonov_linear_solver.py:201-208 with
    B = gradient).  out may be g.  result: as in loss_cost_grad."""
    _same(x, g)
    ndim, nz, ny, nx = dims3(shape)
    if out is None:
        out = empty_like(g)
    ws, res = _workspace(x.device)
    if result is not None:
        res = result
    _lib.check(_fn("tk1_reg_cost_grad", x)(
        _p(x), _p(g), _p(out), ndim, nz, ny, nx, w[0], w[1], w[2], float(alpha),
        _p(res), _p(ws), stream_ptr()), "nsol_tk1_reg_cost_grad")
    return (res if result is not None else float(res.item())), _wrote(out)


_ws3 = {}


def tk1_reg_objective(x, g, d, shape, w, alpha, lo, hi, out, result, gold=None,
                      ydiff=None):
    """tk1_reg_cost_grad with the new gradient's product with d (None: 0) and its
    largest projected component for lo <= x <= hi in result[1], result[2]; with gold,
    ydiff = out - gold and its sum of squares in result[3] (result: the caller's
    four-element float64 device slots; nothing is read back here)."""
    _same(x, g)
    if d is not None:
        _same(x, d)
    if gold is not None:
        _same(x, gold, ydiff)
    ndim, nz, ny, nx = dims3(shape)
    key = (x.device.index, stream_ptr())
    if key not in _ws3:
        _ws3[key] = torch.empty(4 * _lib.load().nsol_hip_reduce_ws_doubles(),
                                dtype=torch.float64, device=x.device)
    _lib.check(_fn("tk1_reg_objective", x)(
        _p(x), _p(g), _p(out), _p(d), _p(gold), _p(ydiff), ndim, nz, ny, nx, w[0], w[1],
        w[2], float(alpha), float(lo), float(hi), _p(result), _p(_ws3[key]),
        stream_ptr()), "nsol_tk1_reg_objective")
    return _wrote(out, ydiff)


def tk1_grad_norm(x, shape, w, result=None):
    """sum |grad x|^2 alone (one read of x); result: the caller's device slot."""
    _chk(x)
    ndim, nz, ny, nx = dims3(shape)
    ws, res = _workspace(x.device)
    if result is not None:
        res = result
    _lib.check(_fn("tk1_grad_norm", x)(
        _p(x), ndim, nz, ny, nx, w[0], w[1], w[2], _p(res), _p(ws), stream_ptr()),
        "nsol_tk1_grad_norm")
    return res if result is not None else float(res.item())


def tk1_lanczos(x, g, z, shape, w, alpha, c_g, c_x, c_z, out, result=None):
    """out = c_g g + alpha grad_adj(grad x) + c_x x + c_z z (z may be None) with the
    sum of squares of out: the Lanczos update of the normal equations."""
    _same(x, g, out)
    if z is not None:
        _same(x, z)
    ndim, nz, ny, nx = dims3(shape)
    ws, res = _workspace(x.device)
    if result is not None:
        res = result
    _lib.check(_fn("tk1_lanczos", x)(
        _p(x), _p(g), _p(z), _p(out), ndim, nz, ny, nx, w[0], w[1], w[2],
        float(alpha), float(c_g), float(c_x), float(c_z), _p(res), _p(ws),
        stream_ptr()), "nsol_tk1_lanczos")
    _wrote(out)
    return res if result is not None else float(res.item())


class ScalarFetch(object):
    """Device scalars to the host while later kernels run: an event behind the
    kernels that produce them, a copy into pinned memory on a side stream, and a
    wait on that copy alone -- the stream the solver enqueues on is not drained
    (a `.cpu()` on it would wait for everything enqueued so far)."""

    def __init__(self, device, count):
        self.host = torch.empty(count, dtype=torch.float64).pin_memory()
        self.side = torch.cuda.Stream(device=device)
        self.ready = torch.cuda.Event()
        self.done = torch.cuda.Event()

    def start(self, dev_scalars):
        self.ready.record(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            self.side.wait_event(self.ready)
            self.host[:dev_scalars.numel()].copy_(dev_scalars, non_blocking=True)
            self.done.record(self.side)

    def wait(self):
        self.done.synchronize()
        return self.host.numpy()


_fetchers = {}


def scalar_fetchers(device, count, n):
    """n ScalarFetch objects of `count` doubles each, kept per device and stream (pinned
    memory and a side stream cost far more to create than to use)."""
    key = (device.index, stream_ptr(), int(count), int(n))
    if key not in _fetchers:
        _fetchers[key] = [ScalarFetch(device, count) for _ in range(n)]
    return _fetchers[key]


_ws8 = {}


def pair_stats(x, y, mx=0.0, my=0.0):
    """NumPy array of the 8 sums documented at nsol_pair_stats_* (syncs)."""
    _same(x, y)
    ws, _ = _workspace(x.device)
    key = (x.device.index, stream_ptr())
    if key not in _ws8:
        _ws8[key] = torch.empty(8, dtype=torch.float64, device=x.device)
    res = _ws8[key]
    _lib.check(_fn("pair_stats", x)(_p(x), _p(y), x.numel(), float(mx),
                                    float(my), _p(res), _p(ws), stream_ptr()),
               "nsol_pair_stats")
    return res.cpu().numpy()


# ------------------------------------------- SSIM, ranges, histograms ----
# (nsol_measures.hip; the measures themselves are in similarity_measures.py)
_ws_res = {}


def _result(dev, n):
    """Small per-device, per-stream device result buffer of n doubles."""
    key = (dev.index, stream_ptr(), n)
    if key not in _ws_res:
        _ws_res[key] = torch.empty(n, dtype=torch.float64, device=dev)
    return _ws_res[key]


def ssim_sum(x, y, shape, win, C1, C2, cov_norm, out=None):
    """Sum of the SSIM map over the valid windows of a box window `win` wide
    along every axis of `shape` (nsol_ssim_*); x, y hold that volume.  Syncs;
    out (a float64 device tensor of one element): the sum is written there and
    nothing is read back (returns out)."""
    _same(x, y)
    ndim, nz, ny, nx = dims3(shape)
    if nz * ny * nx != x.numel():
        raise ValueError("shape %s does not match %d elements" %
                         (tuple(shape), x.numel()))
    ws, _ = _workspace(x.device)
    res = _result(x.device, 1) if out is None else out
    if res.dtype != torch.float64 or res.numel() < 1:
        raise ValueError("out: a float64 device tensor of one element")
    _lib.check(_fn("ssim", x)(_p(x), _p(y), ndim, nz, ny, nx, int(win),
                              float(C1), float(C2), float(cov_norm), _p(res),
                              _p(ws), stream_ptr()), "nsol_ssim")
    if out is not None:
        return _wrote(out)
    return float(res.item())


# ------------------------------------------------------ observation ----
# (nsol_observe.hip; the observer itself is observer.py)
OBS_PAIR, OBS_GRAD, OBS_SQ, OBS_HUBER = 1, 2, 4, 8
OBS_SUMS = 9


def observe(x, x_scale, row, shape, y=None, ybar=0.0, w=(1.0, 1.0, 1.0),
            ndim=None, gamma=0.05, flags=0, pitch=0):
    """The 9 sums of nsol_observe_* of x * x_scale into the float64 device
    tensor `row` (at least 9 elements); x holds the volume `shape` with its rows
    `pitch` elements apart (0: contiguous).  y: contiguous reference of the
    volume's size, x's dtype or float64 (OBS_PAIR).  ndim: gradient components
    (OBS_GRAD; default len(shape)).  Does not synchronise."""
    _chk(x)
    _chk(row)
    gdim, nz, ny, nx = dims3(shape)
    ndim = gdim if ndim is None else int(ndim)
    rows = nz * ny
    if x.numel() != rows * (pitch if pitch else nx) or (pitch and pitch < nx):
        raise ValueError("x does not hold a %s volume at pitch %d" %
                         (tuple(shape), pitch))
    if row.dtype != torch.float64 or row.numel() < OBS_SUMS:
        raise ValueError("row: a float64 device tensor of %d elements" % OBS_SUMS)
    y_f64 = 0
    if flags & OBS_PAIR:
        _chk(y)
        if y.numel() != rows * nx or y.dtype not in (x.dtype, torch.float64):
            raise ValueError("y: %d elements of %s or float64" % (rows * nx, x.dtype))
        y_f64 = int(y.dtype == torch.float64)
    else:
        y = None
    ws, _ = _workspace(x.device)
    _lib.check(_fn("observe", x)(
        _p(x), float(x_scale), _p(y), y_f64, float(ybar), ndim, nz, ny, nx,
        int(pitch), float(w[0]), float(w[1]), float(w[2]), float(gamma), int(flags),
        _p(row), _p(ws), stream_ptr()), "nsol_observe")
    return _wrote(row)


def observe_widen(x, x_scale, shape, pitch=0, out=None):
    """(double)(x * (T)x_scale) as a contiguous float64 device tensor: the
    iterate Solver.get_x() hands the host, without leaving the device."""
    _chk(x)
    _, nz, ny, nx = dims3(shape)
    if x.numel() != nz * ny * (pitch if pitch else nx) or (pitch and pitch < nx):
        raise ValueError("x does not hold a %s volume at pitch %d" %
                         (tuple(shape), pitch))
    if out is None:
        out = torch.empty(nz * ny * nx, dtype=torch.float64, device=x.device)
    _chk(out)
    if out.dtype != torch.float64 or out.numel() != nz * ny * nx:
        raise ValueError("out: %d float64 elements" % (nz * ny * nx))
    _lib.check(_fn("observe_widen", x)(_p(out), _p(x), float(x_scale), nz, ny, nx,
                                       int(pitch), stream_ptr()),
               "nsol_observe_widen")
    return _wrote(out)


def pair_range(x, y):
    """(min x, max x, min y, max y, number of non-finite values) over the
    finite values of x and y (nsol_pair_range_*).  Syncs."""
    _same(x, y)
    ws, _ = _workspace(x.device)
    res = _result(x.device, 5)
    _lib.check(_fn("pair_range", x)(_p(x), _p(y), x.numel(), _p(res), _p(ws),
                                    stream_ptr()), "nsol_pair_range")
    r = res.cpu().numpy()
    return float(r[0]), float(r[1]), float(r[2]), float(r[3]), int(r[4])


def numpy_dtype(x):
    """NumPy dtype of a NumPy array or torch tensor."""
    if isinstance(x, torch.Tensor):
        return torch.empty(0, dtype=x.dtype).numpy().dtype
    return np.asarray(x).dtype


def _hist_dtype(dt):
    """NumPy histograms bool data as uint8; float16 and complex are not covered."""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return np.dtype(np.uint8)
    if dt.kind not in "iuf" or dt == np.float16 or dt.itemsize > 8:
        raise TypeError("histograms of %s data are not supported" % dt)
    return dt


def _as_compare(t, edges):
    """t in the comparison dtype of `edges` (float32 or float64; exact casts)."""
    td = torch.float32 if edges.dtype == np.float32 else torch.float64
    if edges.dtype not in (np.float32, np.float64):
        raise TypeError("histogram edges of dtype %s are not supported" % edges.dtype)
    return t if t.dtype == td else t.to(td).contiguous()


def _edges_dev(e, t):
    return torch.from_numpy(np.ascontiguousarray(e)).to(t.device)


def _scale(e):
    return (len(e) - 1) / (float(e[-1]) - float(e[0]))


def hist1d_counts(x, edges):
    """np.histogram counts (int64) of the values of device tensor x over the
    increasing edges (NumPy array; its dtype is the comparison dtype).  Every
    value must lie inside [edges[0], edges[-1]].  Syncs."""
    _chk(x)
    x = _as_compare(x.reshape(-1), edges)
    e = _edges_dev(edges, x)
    out = torch.empty(len(edges) - 1, dtype=torch.int64, device=x.device)
    _lib.check(_fn("hist1d", x)(_p(x), x.numel(), _p(e), len(edges) - 1,
                                _scale(edges), _p(out), stream_ptr()),
               "nsol_hist1d")
    return out.cpu().numpy()


def hist2d_counts(x, y, xedges, yedges):
    """np.histogram2d counts (int64, shape (bx, by)) of the pairs (x[i], y[i])
    over increasing edges of one dtype (the comparison dtype).  Syncs."""
    _chk(x)
    _chk(y)
    if xedges.dtype != yedges.dtype:
        raise TypeError("edges of one comparison dtype expected")
    x = _as_compare(x.reshape(-1), xedges)
    y = _as_compare(y.reshape(-1), yedges)
    _same(x, y)
    ex, ey = _edges_dev(xedges, x), _edges_dev(yedges, x)
    bx, by = len(xedges) - 1, len(yedges) - 1
    out = torch.empty(bx * by, dtype=torch.int64, device=x.device)
    _lib.check(_fn("hist2d", x)(_p(x), _p(y), x.numel(), _p(ex), bx,
                                _scale(xedges), _p(ey), by, _scale(yedges),
                                _p(out), stream_ptr()), "nsol_hist2d")
    return out.cpu().numpy().reshape(bx, by)


def _float_tensor(t):
    return t if t.dtype in (torch.float32, torch.float64) else t.to(torch.float64)


def _int_bins(bins, n):
    b = tuple(np.atleast_1d(bins).tolist()) if np.ndim(bins) else (bins,) * n
    if len(b) != n or not all(isinstance(v, (int, np.integer)) for v in b):
        raise ValueError("bins: an integer (or one per axis) is supported; "
                         "explicit bin edges are not")
    if any(v < 1 for v in b):
        raise ValueError("bins must be positive")
    return tuple(int(v) for v in b)


def _check_range(r):
    if r[4]:
        raise ValueError("autodetected range of the data is not finite")


def hist_edges(lo, hi, dtype, bins):
    """np.histogram's edges for data of `dtype` with minimum lo and maximum hi
    (exact in float64 for every supported dtype): NumPy builds them itself from
    a two-point array of that dtype, so they are bit-identical to its own."""
    return np.histogram_bin_edges(np.array([lo, hi], dtype), bins)


def hist2d_edges(xrange_, yrange_, dx, dy, bins):
    """np.histogram2d's (xedges, yedges) for data of dtypes dx, dy with the
    given (min, max): NumPy's own, from two-point arrays (both axes in the
    promoted dtype)."""
    _, ex, ey = np.histogram2d(np.array(xrange_, dx), np.array(yrange_, dy), bins)
    return ex, ey


def histogram1d(x, bins=100, dtype=None):
    """(counts, edges) of np.histogram(a, bins) for the array a held by the
    device tensor x; dtype: a's NumPy dtype (fixes the edges' dtype), default
    x's own."""
    _chk(x)
    (bins,) = _int_bins(bins, 1)
    dt = _hist_dtype(dtype if dtype is not None else numpy_dtype(x))
    x = _float_tensor(x).reshape(-1)
    lo, hi, _, _, bad = pair_range(x, x)
    _check_range((0, 0, 0, 0, bad))
    edges = hist_edges(lo, hi, dt, bins)
    return hist1d_counts(x, edges), edges


def histogram2d(x, y, bins=100, dtypes=None, marginals=False):
    """(counts, xedges, yedges) of np.histogram2d(a, b, bins) for the arrays a,
    b held by the device tensors x, y (dtypes: their NumPy dtypes, default the
    tensors' own).  marginals=True also returns the two 1-D np.histogram counts
    of a and b: the joint histogram's row / column sums where NumPy's 1-D edges
    are the joint ones (one pass), else a pass in each array's own dtype."""
    _chk(x)
    _chk(y)
    bx, by = _int_bins(bins, 2)
    if x.numel() != y.numel():
        raise ValueError("x and y differ in length")
    dx, dy = dtypes if dtypes is not None else (numpy_dtype(x), numpy_dtype(y))
    dx, dy = _hist_dtype(dx), _hist_dtype(dy)
    xf, yf = _float_tensor(x).reshape(-1), _float_tensor(y).reshape(-1)
    common = torch.float32 if (xf.dtype == yf.dtype == torch.float32) else torch.float64
    xc = xf if xf.dtype == common else xf.to(common)
    yc = yf if yf.dtype == common else yf.to(common)
    r = pair_range(xc, yc)
    _check_range(r)
    xedges, yedges = hist2d_edges(r[0:2], r[2:4], dx, dy, (bx, by))
    counts = hist2d_counts(xc, yc, xedges, yedges)
    if not marginals:
        return counts, xedges, yedges
    hx = hy = None
    ex1 = hist_edges(r[0], r[1], dx, bx)
    ey1 = hist_edges(r[2], r[3], dy, by)
    if ex1.dtype == xedges.dtype and np.array_equal(ex1, xedges):
        hx = counts.sum(axis=1)
    else:
        hx = hist1d_counts(xf, ex1)
    if ey1.dtype == yedges.dtype and np.array_equal(ey1, yedges):
        hy = counts.sum(axis=0)
    else:
        hy = hist1d_counts(yf, ey1)
    return counts, xedges, yedges, hx, hy


def loss_eval(f2, loss, f_scale=1.0, huber_gamma=1.345):
    """Element-wise (rho(f2), rho'(f2))."""
    _chk(f2)
    rho, drho = empty_like(f2), empty_like(f2)
    _lib.check(_fn("loss_eval", f2)(_p(f2), _p(rho), _p(drho), f2.numel(),
                                    LOSSES[loss], float(f_scale),
                                    float(huber_gamma), stream_ptr()),
               "nsol_loss_eval")
    return rho, drho


def vector_norm_sum(t, ndim, mode=0, gamma=0.05):
    _chk(t)
    ws, res = _workspace(t.device)
    _lib.check(_fn("vector_norm_sum", t)(
        _p(t), int(ndim), t.numel() // int(ndim), int(mode), float(gamma),
        _p(res), _p(ws), stream_ptr()), "nsol_vector_norm_sum")
    return float(res.item())


# ------------------------------------------------------------------- PD ----
def pd_dual_step(xbar, p_in, p_out, shape, w, sigma, hden):
    ndim, nz, ny, nx = dims3(shape)
    _lib.check(_fn("pd_dual_step", xbar)(
        _p(xbar), _p(p_in), _p(p_out), ndim, nz, ny, nx, w[0], w[1], w[2],
        float(sigma), float(hden), stream_ptr()), "nsol_pd_dual_step")
    _wrote(p_out)


def pd_dual_step_iso(xbar, p_in, p_out, shape, w, sigma, hden):
    """pd_dual_step with the isotropic projection (PD_REG_ISOTROPIC)."""
    ndim, nz, ny, nx = dims3(shape)
    _lib.check(_fn("pd_dual_step_iso", xbar)(
        _p(xbar), _p(p_in), _p(p_out), ndim, nz, ny, nx, w[0], w[1], w[2],
        float(sigma), float(hden), stream_ptr()), "nsol_pd_dual_step_iso")
    _wrote(p_out)


def pd_primal_step(p, x, xbar, bt, shape, w, tau, tl, theta, flags):
    ndim, nz, ny, nx = dims3(shape)
    _lib.check(_fn("pd_primal_step", x)(
        _p(p), _p(x), _p(xbar), _p(bt), ndim, nz, ny, nx, w[0], w[1], w[2],
        float(tau), float(tl), float(theta), int(flags), stream_ptr()),
        "nsol_pd_primal_step")
    _wrote(x, xbar)


def pd_fused_iter(xbar_in, xbar_out, x, bt, p_in, p_out, shape, w, sigma,
                  hden, tau, tl, theta, flags):
    ndim, nz, ny, nx = dims3(shape)
    _lib.check(_fn("pd_fused_iter", x)(
        _p(xbar_in), _p(xbar_out), _p(x), _p(bt), _p(p_in), _p(p_out), ndim,
        nz, ny, nx, w[0], w[1], w[2], float(sigma), float(hden), float(tau),
        float(tl), float(theta), int(flags), stream_ptr()),
        "nsol_pd_fused_iter")
    _wrote(xbar_out, x, p_out)


def pd_fused2_iter(xbar_in, xbar_out, x_in, x_out, bt, p_in, p_out, shape, w,
                   sigma2, hden2, tau2, tl2, theta2, flags):
    """Two iterations in one pass; returns False if the kernel does not apply
    to this problem (nothing was launched)."""
    ndim, nz, ny, nx = dims3(shape)
    arr = [np.ascontiguousarray(a, dtype=np.float64)
           for a in (sigma2, hden2, tau2, tl2, theta2)]
    rc = _fn("pd_fused2_iter", x_in)(
        _p(xbar_in), _p(xbar_out), _p(x_in), _p(x_out), _p(bt), _p(p_in),
        _p(p_out), ndim, nz, ny, nx, w[0], w[1], w[2], arr[0].ctypes.data,
        arr[1].ctypes.data, arr[2].ctypes.data, arr[3].ctypes.data,
        arr[4].ctypes.data, int(flags), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pd_fused2_iter")
    _wrote(xbar_out, x_out, p_out)
    return True


def pd_fusedk_iter(xbar_in, xbar_out, x_in, x_out, bt, p_in, p_out, shape, w,
                   sigma, hden, tau, tl, theta, flags):
    """len(sigma) = 2 or 3 iterations in one pass on tiled footprints; returns
    False if the kernel does not apply (nothing was launched)."""
    ndim, nz, ny, nx = dims3(shape)
    arr = [np.ascontiguousarray(a, dtype=np.float64)
           for a in (sigma, hden, tau, tl, theta)]
    k = int(arr[0].size)
    if any(a.size != k for a in arr):
        raise ValueError("step-size arrays must have equal length")
    rc = _fn("pd_fusedk_iter", x_in)(
        _p(xbar_in), _p(xbar_out), _p(x_in), _p(x_out), _p(bt), _p(p_in),
        _p(p_out), ndim, nz, ny, nx, w[0], w[1], w[2], k, arr[0].ctypes.data,
        arr[1].ctypes.data, arr[2].ctypes.data, arr[3].ctypes.data,
        arr[4].ctypes.data, int(flags), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pd_fusedk_iter")
    _wrote(xbar_out, x_out, p_out)
    return True


def pd_fusedk_tuned(x, shape, k=3):
    """1 once the online tuner of the k-iterations-per-pass kernel has settled
    for this shape / dtype, 0 while exploring, -1 if the shape is unknown."""
    ndim, nz, ny, nx = dims3(shape)
    return int(_lib.load().nsol_pd_fusedk_tuned(int(x.element_size()), int(k),
                                                nz, ny, nx))


def pd_fusedk_launches(k=3):
    """k_pd_fusedk launches of depth k made by this process so far."""
    return int(_lib.load().nsol_pd_fusedk_launches(int(k)))


def pd_fusedk_plan_form(x, shape, form, k=3):
    """The settled plan of one form of the depth-k kernel (0: k_pd_fusedk, 1: the
    shifted k_pd_shift3), or None."""
    import ctypes
    ndim, nz, ny, nx = dims3(shape)
    wv, nt, zc = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.load().nsol_pd_fusedk_plan_form(
        int(x.element_size()), int(k), nz, ny, nx, int(form), ctypes.byref(wv),
        ctypes.byref(nt), ctypes.byref(zc))
    return None if rc else (int(wv.value), int(nt.value), int(zc.value))


def pd_shift_launches():
    """Launches of the shifted depth-3 form (k_pd_shift3) by this process so far;
    they count into pd_fusedk_launches(3) as well."""
    return int(_lib.load().nsol_pd_shift_launches())


def lb_gram_launches(form):
    """Launches of one form of the masked Gram pass by this process so far (0:
    k_masked_gram, 1: k_masked_gram_dma, 2: k_masked_gram_mfma; -1 for another form)."""
    return int(_lib.load().nsol_lb_gram_launches(int(form)))


def pd_run_parts(iterations, min_iters):
    """(taken, lead, launches): how nsol_pd_run_* cuts a run of `iterations` when the
    shifted block starts at `min_iters` iterations (0: never)."""
    import ctypes
    lead, m = ctypes.c_int(0), ctypes.c_int(0)
    taken = _lib.load().nsol_pd_run_parts(int(iterations), int(min_iters),
                                          ctypes.byref(lead), ctypes.byref(m))
    return bool(taken), int(lead.value), int(m.value)


def pd_fusedk_plan(x, shape, k=3):
    """(waves, tiles along x, z-chunk) the online tuner settled on, or None."""
    import ctypes
    ndim, nz, ny, nx = dims3(shape)
    wv, nt, zc = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.load().nsol_pd_fusedk_plan(
        int(x.element_size()), int(k), nz, ny, nx, ctypes.byref(wv),
        ctypes.byref(nt), ctypes.byref(zc))
    return None if rc else (int(wv.value), int(nt.value), int(zc.value))


# Cache-resident volumes (BASELINE configs 1-2): the whole run in ONE launch of the
# persistent kernel (nsol_pd_persist_run_*), from this many iterations on and up to
# this many voxels (above, three iterations per pass take over).
PD_PERSIST = True
PD_PERSIST_MIN_ITERS = 16
PD_PERSIST_MAX_VOXELS = 1 << 20
_persist_launches = 0


def pd_persist_launches():
    """Runs that went through the persistent kernel (for tests and tools)."""
    return _persist_launches


# Error words of the persistent runs: a ring of 32-bit words in pinned host
# memory the kernels write to directly.  A persistent run reads its state from
# one set of arrays and writes the result to another, so a run whose word came
# back raised (a workgroup gave up waiting for a neighbour: the device is shared
# or CU-masked and not every workgroup was resident) is REPEATED from the
# untouched inputs with one launch per iteration -- the same bits -- by
# settle_persist_runs().  That is called wherever a result is consumed after a
# synchronisation the caller performs anyway: Solver.run() (after its own
# torch.cuda.synchronize), device.to_numpy, solve_batch before its gather, the
# next pd_run on the device; never with a synchronisation in the middle of
# enqueued work.
_ERR_SLOTS = 256
_err_ring = None
_err_next = 0
_pending_runs = []         # PersistRun records, oldest first
_fallback_warned = False
persist_fallbacks = 0      # runs repeated so far (tests, tools)


class PersistRun(object):
    """What it takes to repeat a persistent run through nsol_pd_run_*."""

    def __init__(self, slot, stream, src, dst, bt, shape, w, lmbda, sigma, tau,
                 theta, p_is_zero, gamma_huber, flags, keep):
        self.slot, self.stream = slot, stream
        self.src, self.dst = src, dst         # (xbar, x, p) tensors read / written
        self.bt, self.shape, self.w, self.lmbda = bt, shape, w, lmbda
        self.sigma, self.tau, self.theta = sigma, tau, theta
        self.p_is_zero, self.gamma_huber, self.flags = p_is_zero, gamma_huber, flags
        self.keep = keep                      # tensors that must outlive the run


def _err_slot():
    global _err_ring, _err_next
    if _err_ring is None:
        _err_ring = torch.zeros(_ERR_SLOTS, dtype=torch.int32).pin_memory()
    slot = _err_next
    _err_next = (_err_next + 1) % _ERR_SLOTS
    if any(r.slot == slot for r in _pending_runs):
        settle_persist_runs()             # the ring has wrapped: settle first
    _err_ring[slot] = 0
    return slot


def _repeat_with_a_launch_per_iteration(r):
    """The inputs of run r are intact (it wrote elsewhere): the same iterations
    through nsol_pd_run_*, the result put where the persistent run left it."""
    import ctypes
    xb_in, x_in, p_in = r.src
    xb_out, x_out, p_out = r.dst
    ndim, nz, ny, nx = dims3(r.shape)
    n_it = int(r.sigma.size)
    slot = ctypes.c_int(0)
    # scratch state so that neither the inputs' nor the outputs' roles matter:
    # start from copies of the inputs, ping-pong against the output arrays
    xb0, x0, p0 = xb_in.clone(), x_in.clone(), p_in.clone()
    _lib.check(_fn("pd_run", x0)(
        _p(xb0), _p(xb_out), _p(x0), _p(x_out), _p(r.bt), _p(p0), _p(p_out), ndim,
        nz, ny, nx, r.w[0], r.w[1], r.w[2], float(r.lmbda), r.sigma.ctypes.data,
        r.tau.ctypes.data, r.theta.ctypes.data, n_it, int(bool(r.p_is_zero)),
        float(r.gamma_huber), int(r.flags) | PD_RUN_X_MAY_SWAP,
        ctypes.addressof(slot), stream_ptr()), "nsol_pd_run")
    _wrote(xb_out, x_out, p_out)
    if not (slot.value & 1):              # final xbar / p in the scratch pair
        xb_out.copy_(xb0)
        p_out.copy_(p0)
    if not (slot.value & 2):              # final x in x0, not in x_out
        x_out.copy_(x0)
    torch.cuda.synchronize()


def settle_persist_runs(synchronize=True):
    """Look at the error word of every persistent run enqueued so far; repeat
    the runs that timed out (see above); returns how many were repeated.
    synchronize=False: the caller has just synchronised the device."""
    global _fallback_warned, persist_fallbacks
    if not _pending_runs:
        return 0
    if synchronize:
        torch.cuda.synchronize()
    saved = (globals()["PD_PERSIST"],)
    repeated = 0
    while _pending_runs:
        r = _pending_runs.pop(0)
        if int(_err_ring[r.slot]) == 0:
            continue
        if r.dst[0] is r.src[0]:          # in place: the inputs are gone
            del _pending_runs[:]
            raise _lib.NsolHipError(
                "nsol_pd_persist_run: a workgroup gave up waiting for a neighbour "
                "(device shared or CU-masked?) in a run that updated its state in "
                "place; the result is invalid")
        if not _fallback_warned:
            import warnings
            warnings.warn(
                "nsol_pd_persist_run: a workgroup gave up waiting for a "
                "neighbour (device shared or CU-masked?); the run is repeated "
                "with one launch per iteration -- set nsol_amd.ops.PD_PERSIST "
                "= False to skip the attempt", RuntimeWarning)
            _fallback_warned = True
        persist_fallbacks += 1
        repeated += 1
        globals()["PD_PERSIST"] = False
        try:
            _repeat_with_a_launch_per_iteration(r)
        finally:
            globals()["PD_PERSIST"] = saved[0]
    return repeated


def drain_persist_checks():
    """(former name) settle after the caller's own synchronisation."""
    settle_persist_runs(synchronize=False)


def pd_persist_run(xbar, x, bt, p, shape, w, lmbda, sigma, tau, theta, p_is_zero,
                   gamma_huber, flags, out=None):
    """All len(sigma) iterations in one launch.  out = (xbar_out, x_out, p_out):
    where the result goes -- arrays other than the inputs, which then survive a
    timed-out run (settle_persist_runs repeats it); out=None: in place, and a
    time-out surfaces as an exception from settle_persist_runs instead.  Returns
    False when the kernel does not apply (nothing launched).  Does not
    synchronise."""
    global _persist_launches
    ndim, nz, ny, nx = dims3(shape)
    iters = int(np.size(sigma))
    need = int(_lib.load().nsol_pd_persist_ws_bytes(int(x.element_size()), ndim,
                                                    nz, ny, nx, iters))
    if need < 0:
        return False
    sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    slot = _err_slot()
    dst = (xbar, x, p) if out is None else tuple(out)
    rc = _fn("pd_persist_run_to", x)(
        _p(xbar), _p(x), _p(bt), _p(p), _p(dst[0]), _p(dst[1]), _p(dst[2]), ndim,
        nz, ny, nx, w[0], w[1], w[2],
        float(lmbda), sigma.ctypes.data, tau.ctypes.data, theta.ctypes.data, iters,
        int(bool(p_is_zero)), float(gamma_huber), int(flags), _p(ws), need,
        _err_ring.data_ptr() + 4 * slot, stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pd_persist_run")
    _wrote(*dst)
    ws.record_stream(torch.cuda.current_stream())      # freed once the run is done
    _pending_runs.append(PersistRun(
        slot, stream_ptr(), (xbar, x, p), dst, bt, tuple(shape), tuple(w), lmbda,
        sigma, tau, theta, p_is_zero, gamma_huber, flags, keep=(ws,)))
    _persist_launches += 1
    return True


def persist_pays(shape, iterations):
    """Where one launch per run beats one launch per iteration (tools/
    bench_persist.py): the persistent kernel takes 4.2-4.8 us per iteration whatever
    the size (the hand-off between workgroups) plus ~20 us per run; a launch per
    iteration costs 5.3-6.7 us on 3-D volumes but only 3.4 us on small images."""
    n = int(np.prod(shape))
    if n > PD_PERSIST_MAX_VOXELS or iterations < PD_PERSIST_MIN_ITERS:
        return False
    return len(shape) == 3 or n >= (1 << 19)


PD_RUN_X_MAY_SWAP = 0x100


def row_pitch(shape, like):
    """Elements between the starts of consecutive rows of a padded 3-D layout: the row
    length rounded up to whole 16-byte vectors (0 where the rows are whole already, or
    the volume is not 3-D)."""
    if len(tuple(shape)) != 3:
        return 0
    vec = 16 // like.element_size()
    nx = int(shape[2])
    if nx < 2 * vec:
        # (the pitched one-iteration kernel -- a run's odd trailing iteration -- needs
        # two vectors per row, nsol_pd.hip fused_iter_impl: such rows stay contiguous)
        return 0
    return 0 if nx % vec == 0 else (nx + vec - 1) // vec * vec


def to_pitched(t, shape, pitch, comps=1, fill=0.0):
    """A flat (comps x volume) tensor re-laid with its rows at `pitch` (padding = fill)."""
    nz, ny, nx = (int(v) for v in shape)
    out = torch.full((comps * nz * ny * pitch,), fill, dtype=t.dtype, device=t.device)
    out.view(comps * nz, ny, pitch)[:, :, :nx].copy_(t.view(comps * nz, ny, nx))
    return _wrote(out)


def from_pitched(t, shape, pitch, comps=1):
    """The contiguous tensor back out of a pitched one."""
    nz, ny, nx = (int(v) for v in shape)
    return t.view(comps * nz, ny, pitch)[:, :, :nx].contiguous().view(-1)


def pd_run(xbar0, xbar1, x, bt, p0, p1, shape, w, lmbda, sigma, tau, theta,
           p_is_zero, gamma_huber, flags, x_alt=None, swap_ok=False, pitch=0):
    """Enqueue len(sigma) iterations; returns the slot (0/1) of xbar/p that
    holds the final state.  x holds the final primal iterate.

    pitch > 0: every array is held with its rows at that pitch (row_pitch /
    to_pitched; nsol_pd_run_pitched_*).

    swap_ok: x and x_alt are whole tensors nobody else aliases -- when the
    multi-iteration kernels leave the final iterate in x_alt, the two tensors
    trade their storage (x still names the result) instead of a copy of the
    volume."""
    import ctypes
    ndim, nz, ny, nx = dims3(shape)
    if _pending_runs:
        # an earlier persistent run may feed this one: its verdict first (the
        # device is drained here; runs of cache-resident volumes are ~1 ms)
        settle_persist_runs()
    if pitch:
        sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        slot = ctypes.c_int(0)
        _lib.check(_fn("pd_run_pitched", x)(
            _p(xbar0), _p(xbar1), _p(x), _p(x_alt), _p(bt), _p(p0), _p(p1), ndim,
            nz, ny, nx, int(pitch), w[0], w[1], w[2], float(lmbda), sigma.ctypes.data,
            tau.ctypes.data, theta.ctypes.data, int(sigma.size), int(bool(p_is_zero)),
            float(gamma_huber),
            int(flags) | (PD_RUN_X_MAY_SWAP if swap_ok and x_alt is not None else 0),
            ctypes.addressof(slot), stream_ptr()), "nsol_pd_run_pitched")
        _wrote(xbar0, xbar1, x, x_alt, p0, p1)
        if slot.value & 2:
            x.data, x_alt.data = x_alt.data, x.data
        return int(slot.value) & 1
    # (the persistent kernel declines the isotropic projection: no attempt, so
    # no pending-run record for a launch that is never made)
    if PD_PERSIST and not (int(flags) & PD_REG_ISOTROPIC) and \
            persist_pays(shape, np.size(sigma)):
        # the result goes to the other half of the ping-pong arrays (and to the
        # x scratch volume): the inputs stay as they are until the run's error
        # word has been looked at
        xo = x_alt if x_alt is not None else empty_like(x)
        if pd_persist_run(xbar0, x, bt, p0, shape, w, lmbda, sigma, tau, theta,
                          p_is_zero, gamma_huber, flags, out=(xbar1, xo, p1)):
            if swap_ok and x_alt is not None:
                x.data, x_alt.data = x_alt.data, x.data
                # (the record holds tensors, not storages: keep it pointing at
                # the input / output storages after the swap of names)
                r = _pending_runs[-1]
                r.src = (r.src[0], x_alt, r.src[2])
                r.dst = (r.dst[0], x, r.dst[2])
            else:
                # x must hold the result: the input x survives in a copy
                r = _pending_runs[-1]
                keep = x.clone()
                x.copy_(xo)
                r.src = (r.src[0], keep, r.src[2])
                r.dst = (r.dst[0], x, r.dst[2])
            return 1
    sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    slot = ctypes.c_int(0)
    _lib.check(_fn("pd_run", x)(
        _p(xbar0), _p(xbar1), _p(x), _p(x_alt), _p(bt), _p(p0), _p(p1), ndim,
        nz, ny, nx, w[0], w[1], w[2], float(lmbda), sigma.ctypes.data,
        tau.ctypes.data, theta.ctypes.data, int(sigma.size),
        int(bool(p_is_zero)), float(gamma_huber),
        int(flags) | (PD_RUN_X_MAY_SWAP if swap_ok and x_alt is not None else 0),
        ctypes.addressof(slot), stream_ptr()), "nsol_pd_run")
    _wrote(xbar0, xbar1, x, x_alt, p0, p1)
    if slot.value & 2:
        x.data, x_alt.data = x_alt.data, x.data
    return int(slot.value) & 1


# ------------------------------------------------------- parameter sweep ----
# Members of a sweep (nsol_amd/parameter_sweep.py) are stacked in one launch per
# iteration while one member has at most PD_SWEEP_MAX_VOXELS voxels, in groups whose
# state (x, two xbar, two p: 3 + 2 dim arrays of the member's size) stays under
# PD_SWEEP_GROUP_BYTES.  Both decide speed only: results are the same bits on either
# side of them.  From tools/bench_sweep.py --explore (float32 TV-l2, 100 iterations,
# 4 / 16 / 64 alphas; DESIGN.md section 4a has the table):
#  * a group that stays within the 256 MB last-level cache beats one launch for all
#    members once their state outgrows it -- 1024^2 x 16: 10.7 ms in groups of 9
#    against 13.1 ms in one group; 128^3 x 16: 28.1 ms in groups of 3 against 34.9 ms;
#    128^3 x 64: 114 against 127 ms -- and costs 2 % where it splits a stack that was
#    cache-resident anyway (64^3 x 64: 17.7 against 17.4 ms);
#  * at 256^3, the largest size measured, the stacked form (one member per launch by
#    then) still beats one solver after the other, 0.108 against 0.143 s for 4 alphas
#    and 1.00 against 1.59 s for 64, because it uploads and scales the observation
#    once; nothing larger was measured, so the limit is that size.
PD_SWEEP_MAX_VOXELS = 1 << 24
PD_SWEEP_GROUP_BYTES = 256 << 20
_sweep_staging = []        # (event, pinned table) of runs whose upload may be pending


def pd_sweep_launches():
    """Launches of the member-stacked kernel so far (for tests and tools)."""
    return int(_lib.load().nsol_pd_sweep_launches())


def _group_size(members, n, dim, elem_size, arrays, group_bytes, most=1 << 31):
    """Members per stacked group: as many as keep a group's state (`arrays` + 2 dim
    arrays of n elements per member) under group_bytes and within the kernel's 2^31
    voxels and `most` members, at least one."""
    per_member = (arrays + 2 * int(dim)) * int(n) * int(elem_size)
    g = min(group_bytes // per_member, (1 << 31) // int(n), most)
    return int(max(1, min(int(members), g)))


def sweep_group_size(members, n, dim, elem_size):
    """Members per stacked group of a sweep (x, two xbar, two p: 3 + 2 dim arrays),
    under PD_SWEEP_GROUP_BYTES."""
    return _group_size(members, n, dim, elem_size, 3, PD_SWEEP_GROUP_BYTES)


def sweep_groups(members, group):
    """[(first, last + 1), ...]: every member once, in order, `group` at a time."""
    members, group = int(members), int(group)
    if members < 1 or group < 1:
        raise ValueError("members and group size must be positive")
    return [(a, min(a + group, members)) for a in range(0, members, group)]


def _schedules(members, lmbda, sigma, tau, theta, reshape=False):
    """The schedules as contiguous float64 arrays, lmbda (members,), the others
    (members, iterations); reshape: any layout of members * iterations counts (a 1-D
    schedule for one member)."""
    lmbda = np.ascontiguousarray(lmbda, dtype=np.float64).reshape(-1)
    sigma, tau, theta = (np.ascontiguousarray(a, dtype=np.float64)
                         for a in (sigma, tau, theta))
    if reshape:
        sigma, tau, theta = (a.reshape(members, -1) for a in (sigma, tau, theta))
    if sigma.ndim != 2 or sigma.shape[0] != members or lmbda.size != members or \
            tau.shape != sigma.shape or theta.shape != sigma.shape:
        raise ValueError("schedules must be (members, iterations) arrays")
    return lmbda, sigma, tau, theta


def _table_entry_bytes(x):
    return int(_lib.load().nsol_pd_sweep_entry_bytes(int(x.element_size())))


def _table_buffers(x, members, iters):
    """(pinned host table, device table, bytes) for PdScalars[iters][members]."""
    _sweep_staging[:] = [s for s in _sweep_staging if not s[0].query()]
    nbytes = max(16, _table_entry_bytes(x) * members * iters)
    return (torch.empty(nbytes, dtype=torch.uint8).pin_memory(),
            torch.empty(nbytes, dtype=torch.uint8, device=x.device), nbytes)


def _table_keep(tab_host):
    # the upload is stream-ordered: its pinned source lives until the event has passed
    ev = torch.cuda.Event()
    ev.record()
    _sweep_staging.append((ev, tab_host))


def _table_has(tab, x, members, iteration):
    if int(iteration) < 0 or \
            tab.numel() < _table_entry_bytes(x) * members * (int(iteration) + 1):
        raise ValueError("the table has no iteration %d for %d members" %
                         (iteration, members))


def _stacked_run(name, x, operands, members, schedules, p_is_zero, gamma_huber, flags,
                 wrote):
    """nsol_<name>_*(operands..., schedules, table buffers, slot, stream): the slot of
    the final state, or None when the library declined."""
    import ctypes
    lmbda, sigma, tau, theta = schedules
    iters = int(sigma.shape[1])
    if _pending_runs:
        settle_persist_runs()     # as pd_run: an earlier persistent run may feed this
    tab_host, tab, nbytes = _table_buffers(x, members, iters)
    slot = ctypes.c_int(0)
    rc = _fn(name, x)(
        *operands, lmbda.ctypes.data, sigma.ctypes.data, tau.ctypes.data,
        theta.ctypes.data, iters, int(bool(p_is_zero)), float(gamma_huber), int(flags),
        tab_host.data_ptr(), _p(tab), nbytes, ctypes.addressof(slot), stream_ptr())
    if rc == -2:
        return None
    _lib.check(rc, "nsol_" + name)
    _wrote(*wrote)
    tab.record_stream(torch.cuda.current_stream())     # freed once the run is done
    _table_keep(tab_host)
    return int(slot.value)


def pd_sweep_run(xbar0, xbar1, x, bt, p0, p1, members, shape, w, lmbda, sigma, tau,
                 theta, p_is_zero, gamma_huber, flags):
    """Enqueue sigma.shape[1] iterations of `members` stacked primal-dual runs that
    share the scaled observation bt: one launch per iteration for all of them.
    x, xbar0/1 hold members * n elements, p0/p1 members * dim * n, member-major;
    lmbda is (members,), sigma/tau/theta (members, iterations).  Returns the slot
    (0/1) of xbar/p that holds the final state, or None when the library declined
    (nothing was launched).  Does not synchronise."""
    ndim, nz, ny, nx = dims3(shape)
    members = int(members)
    n = nz * ny * nx
    _chk(bt)
    _same(x, xbar0, xbar1)
    _same(p0, p1)
    if bt.dtype != x.dtype or p0.dtype != x.dtype or bt.numel() != n or \
            x.numel() != members * n or p0.numel() != members * ndim * n:
        raise ValueError("operand mismatch: %d members of %d voxels against x[%d], "
                         "bt[%d], p[%d]" % (members, n, x.numel(), bt.numel(),
                                            p0.numel()))
    return _stacked_run(
        "pd_sweep_run", x,
        (_p(xbar0), _p(xbar1), _p(x), _p(bt), _p(p0), _p(p1), members, ndim, nz, ny, nx,
         w[0], w[1], w[2]), members, _schedules(members, lmbda, sigma, tau, theta),
        p_is_zero, gamma_huber, flags, (xbar0, xbar1, x, p0, p1))


# ----------------------------------------------------------- image stack ----
# Independent images of one shape (nsol_amd/solver_batch.py) are stacked in one launch
# per iteration like the members of a sweep, except that every member brings its own
# scaled observation: a member's state is x, two xbar, two p AND bt, 4 + 2 dim arrays
# (12 words per voxel in 3-D where a sweep member has 11 + 1/P).  The two constants
# decide speed only, as the sweep's do; DESIGN.md section 4b has the table they come
# from (tools/bench_batch.py --explore).
PD_BATCH_MAX_VOXELS = 1 << 24
PD_BATCH_GROUP_BYTES = 256 << 20


def pd_batch_launches():
    """Launches of the image-stacked kernels so far (for tests and tools)."""
    return int(_lib.load().nsol_pd_batch_launches())


def batch_group_size(members, n, dim, elem_size):
    """Members per stacked group of independent images: the per-member observation
    counts (4 + 2 dim arrays), under PD_BATCH_GROUP_BYTES, at most 65535 members."""
    return _group_size(members, n, dim, elem_size, 4, PD_BATCH_GROUP_BYTES, 65535)


def scale_rows(x, s, members, divide=False, out=None, dtype=None):
    """Row m of the (members, n) array x divided (divide=True) or multiplied by s[m],
    one launch: every row the bits ops.scale gives for it alone.  s: a device
    float64 tensor of `members` scales.  dtype=torch.float32 with a float64 x: the
    operation in float64, rounded once (scaled_data_on_device's form)."""
    _chk(x)
    _chk(s)
    members = int(members)
    if s.dtype != torch.float64 or s.numel() != members or members < 1 or \
            x.numel() % members:
        raise ValueError("scale_rows needs one float64 scale per row: %d rows, "
                         "%d scales, %d elements" % (members, s.numel(), x.numel()))
    if members > 65535:
        raise ValueError("scale_rows takes at most 65535 rows")
    n = x.numel() // members
    to = x.dtype if dtype is None else dtype
    if out is None:
        out = torch.empty(x.numel(), dtype=to, device=x.device).view(x.shape)
    _chk(out)
    if out.dtype != to or out.numel() != x.numel():
        raise ValueError("operand mismatch: out is %s[%d]" % (out.dtype, out.numel()))
    if to == x.dtype:
        fn, what = _fn("scale_rows", x), "nsol_scale_rows"
    elif x.dtype == torch.float64 and to == torch.float32:
        fn, what = _lib.load().nsol_scale_rows_f64_to_f32, "nsol_scale_rows_f64_to_f32"
    else:
        raise ValueError("scale_rows converts float64 to float32 only")
    _lib.check(fn(_p(out), _p(x), _p(s), int(bool(divide)), members, n, stream_ptr()),
               what)
    return _wrote(out)


def pd_batch_run(xbar0, xbar1, x, bt, p0, p1, members, shape, w, lmbda, sigma, tau,
                 theta, p_is_zero, gamma_huber, flags):
    """pd_sweep_run for `members` independent images: bt holds members * n elements,
    member-major, and flags may carry PD_REG_ISOTROPIC.  Returns the slot (0/1) of
    xbar/p that holds the final state, or None when the library declined (nothing
    was launched).  Does not synchronise."""
    ndim, nz, ny, nx = dims3(shape)
    members = int(members)
    n = nz * ny * nx
    _same(x, xbar0, xbar1, bt)
    _same(p0, p1)
    if p0.dtype != x.dtype or x.numel() != members * n or \
            p0.numel() != members * ndim * n:
        raise ValueError("operand mismatch: %d members of %d voxels against x[%d], "
                         "p[%d]" % (members, n, x.numel(), p0.numel()))
    return _stacked_run(
        "pd_batch_run", x,
        (_p(xbar0), _p(xbar1), _p(x), _p(bt), _p(p0), _p(p1), members, ndim, nz, ny, nx,
         w[0], w[1], w[2]), members, _schedules(members, lmbda, sigma, tau, theta),
        p_is_zero, gamma_huber, flags, (xbar0, xbar1, x, p0, p1))


# ------------------------------------------------- weighted data term ----
# Runs whose data term carries per-voxel weights (PD_DATA_WEIGHTED; nsol_pdw.hip): one
# stacked kernel family for the single run (members = 1), the parameter sweep (bt and
# wt shared by all members) and the stack of images (every member its own of each).
def pd_weighted_launches():
    """Launches of the weighted kernels so far (for tests and tools)."""
    return int(_lib.load().nsol_pd_weighted_launches())


def weighted_batch_group_size(members, n, dim, elem_size):
    """batch_group_size with the member's own weights counted: 5 + 2 dim arrays."""
    return _group_size(members, n, dim, elem_size, 5, PD_BATCH_GROUP_BYTES, 65535)


def _weighted_operands(x, xbar0, xbar1, bt, wt, p0, p1, members, shape):
    """(ndim, nz, ny, nx, bt_stride, wt_stride) after the checks that keep the
    kernel inside its arrays."""
    ndim, nz, ny, nx = dims3(shape)
    n = nz * ny * nx
    _same(x, xbar0, xbar1)
    _same(p0, p1)
    _chk(bt)
    _chk(wt)
    if p0.dtype != x.dtype or bt.dtype != x.dtype or wt.dtype != x.dtype or \
            members < 1 or x.numel() != members * n or \
            p0.numel() != members * ndim * n or \
            bt.numel() not in (n, members * n) or wt.numel() not in (n, members * n):
        raise ValueError("operand mismatch: %d members of %d voxels against x[%d], "
                         "bt[%d], wt[%d], p[%d]" % (members, n, x.numel(), bt.numel(),
                                                    wt.numel(), p0.numel()))
    return (ndim, nz, ny, nx, 0 if bt.numel() == n else n,
            0 if wt.numel() == n else n)


def pd_weighted_run(xbar0, xbar1, x, bt, wt, p0, p1, members, shape, w, lmbda, sigma,
                    tau, theta, p_is_zero, gamma_huber, flags):
    """Enqueue the iterations of `members` stacked primal-dual runs with a weighted
    data term (flags carry PD_DATA_WEIGHTED): one launch per iteration for all of
    them.  Layout as pd_batch_run; bt and wt hold n elements (shared by the members)
    or members * n (member-major), each on its own.  lmbda is (members,),
    sigma/tau/theta (members, iterations) -- or 1-D for one member.  Returns the slot
    (0/1) of xbar/p that holds the final state, or None when the library declined
    (nothing was launched).  Does not synchronise."""
    members = int(members)
    ndim, nz, ny, nx, bts, wts = _weighted_operands(x, xbar0, xbar1, bt, wt, p0, p1,
                                                    members, shape)
    return _stacked_run(
        "pd_weighted_run", x,
        (_p(xbar0), _p(xbar1), _p(x), _p(bt), bts, _p(wt), wts, _p(p0), _p(p1), members,
         ndim, nz, ny, nx, w[0], w[1], w[2]), members,
        _schedules(members, lmbda, sigma, tau, theta, reshape=True), p_is_zero,
        gamma_huber, flags, (xbar0, xbar1, x, p0, p1))


def pd_weighted_table(like, members, lmbda, sigma, tau, theta, p_is_zero, gamma_huber,
                      flags):
    """The device table of a weighted run's scalars ([iteration][member], the element
    type of `like`) for pd_weighted_iter; schedules as in pd_weighted_run."""
    members = int(members)
    lmbda, sigma, tau, theta = _schedules(members, lmbda, sigma, tau, theta,
                                          reshape=True)
    iters = int(sigma.shape[1])
    tab_host, tab, nbytes = _table_buffers(like, members, iters)
    _lib.check(_fn("pd_weighted_table", like)(
        members, lmbda.ctypes.data, sigma.ctypes.data, tau.ctypes.data,
        theta.ctypes.data, iters, int(bool(p_is_zero)), float(gamma_huber), int(flags),
        tab_host.data_ptr(), _p(tab), nbytes, stream_ptr()), "nsol_pd_weighted_table")
    _table_keep(tab_host)
    return tab


def pd_weighted_iter(xbar_in, xbar_out, x, bt, wt, p_in, p_out, members, shape, w, tab,
                     iteration, flags):
    """One launch: iteration `iteration` of the table pd_weighted_table made.  p_in
    is not read where the table says that p is zero, but must be given.  Returns
    False when the library declined (nothing was launched)."""
    members = int(members)
    ndim, nz, ny, nx, bts, wts = _weighted_operands(x, xbar_in, xbar_out, bt, wt, p_in,
                                                    p_out, members, shape)
    _table_has(tab, x, members, iteration)
    rc = _fn("pd_weighted_iter", x)(
        _p(xbar_in), _p(xbar_out), _p(x), _p(bt), bts, _p(wt), wts, _p(p_in), _p(p_out),
        members, ndim, nz, ny, nx, w[0], w[1], w[2], _p(tab), int(iteration), int(flags),
        stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pd_weighted_iter")
    _wrote(xbar_out, x, p_out)
    return True


# ------------------------------------ data term behind a linear operator ----
# (nsol_pdl.hip; the loop is primal_dual_linear_solver.py's)
def pdl_launches():
    """Launches of k_pd_lin / k_pd_lin_iso so far (for tests and tools)."""
    return int(_lib.load().nsol_pdl_launches())


def pdl_dual_data(q, t, bt, wt, sigma, lmbda, l1=False):
    """The data term's dual variable q in place: v = q + sigma * (t - bt) with t = A xbar,
    or, t None, v = q - sigma * bt with q already holding q + sigma A xbar (the blur's
    epilogue); then q = v c / (c + sigma) (l2) or clamp(v, -c, c) (l1) with
    c = lmbda * wt (wt None: 1), and exactly 0 where wt is 0.  Does not synchronise."""
    _same(q, bt)
    if t is not None:
        _same(q, t)
    if wt is not None:
        _same(q, wt)
    _lib.check(_fn("pdl_dual_data", q)(
        _p(q), _p(t), _p(bt), _p(wt), float(sigma), float(lmbda), int(bool(l1)),
        q.numel(), stream_ptr()), "nsol_pdl_dual_data")
    return _wrote(q)


def pdl_dual_data_kl(q, t, bt, wt, sigma, lmbda, background=0.):
    """pdl_dual_data for the Poisson (Kullback-Leibler) data term with a constant
    background >= 0: v = q + sigma * (t + background), or, t None, q + sigma * background;
    then kl_dual_prox of csrc/nsol_kl.hpp with c = lmbda * wt (never above c), and exactly
    0 where wt is 0.  Does not synchronise."""
    _same(q, bt)
    if t is not None:
        _same(q, t)
    if wt is not None:
        _same(q, wt)
    _lib.check(_fn("pdl_dual_data_kl", q)(
        _p(q), _p(t), _p(bt), _p(wt), float(sigma), float(lmbda), float(background),
        q.numel(), stream_ptr()), "nsol_pdl_dual_data_kl")
    return _wrote(q)


def pdl_iter(xbar_in, xbar_out, x, g, p_in, p_out, shape, w, sigma, hden, tau, theta,
             lo, hi, flags, has_p=True):
    """One iteration's regulariser side and explicit primal step in one pass:
    p_out = prox(p_in + sigma grad xbar_in), x = clip(x - tau (grad^T p_out + g), lo, hi),
    xbar_out = x + theta (x - x_old); g = A^T q.  has_p False: p_in counts as zero (it
    must still be given).  flags: PD_REG_TV / PD_REG_HUBER, PD_REG_ISOTROPIC.  Returns
    False when the library declined the geometry (nothing was launched).  Does not
    synchronise."""
    ndim, nz, ny, nx = dims3(shape)
    n = nz * ny * nx
    _same(x, xbar_in, xbar_out, g)
    _same(p_out, p_in)
    if p_out.dtype != x.dtype or x.numel() != n or p_out.numel() != ndim * n:
        raise ValueError("operand mismatch: x %s[%d], p %s[%d] for shape %r" %
                         (str(x.dtype), x.numel(), str(p_out.dtype), p_out.numel(),
                          tuple(shape)))
    rc = _fn("pdl_iter", x)(
        _p(xbar_in), _p(xbar_out), _p(x), _p(g), _p(p_in), _p(p_out), ndim, nz, ny, nx,
        w[0], w[1], w[2], float(sigma), float(hden), float(tau), float(theta), float(lo),
        float(hi), int(flags), int(bool(has_p)), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pdl_iter")
    _wrote(xbar_out, x, p_out)
    return True


# --------------------------- second-order TGV (nsol_tgv.hip, tgv_numpy.py) ----
def tgv_launches():
    """Successful launches of k_tgv_dual / k_tgv_primal so far (for tests and tools)."""
    return int(_lib.load().nsol_tgv_launches())


def _tgv_operands(shape, x_like, vectors, tensors):
    """Checks the stacks of a TGV call: every tensor of `vectors` holds ndim * n values
    and every one of `tensors` M * n, in the element type of x_like (n values)."""
    ndim, nz, ny, nx = dims3(shape)
    n = nz * ny * nx
    for group, size in ((vectors, ndim * n), (tensors, ndim * (ndim + 1) // 2 * n),
                        ((x_like,), n)):
        for t in group:
            if _chk(t).dtype != x_like.dtype or t.numel() != size:
                raise ValueError("operand mismatch: %s[%d] where %s[%d] is expected for "
                                 "shape %r" % (str(t.dtype), t.numel(), str(x_like.dtype),
                                               size, tuple(shape)))
    return ndim, nz, ny, nx


def tgv_dual(xbar, wbar, p, q, shape, w, sigma, beta, flags=0):
    """The dual half of a TGV iteration, p and q in place: p_a <- P_1(p_a + sigma (D_a
    xbar - wbar_a)), q <- P_beta(q + sigma E wbar).  flags: PD_REG_ISOTROPIC.  Returns
    False when the library declined the geometry (nothing was launched).  Does not
    synchronise."""
    ndim, nz, ny, nx = _tgv_operands(shape, xbar, (wbar, p), (q,))
    rc = _fn("tgv_dual", xbar)(
        _p(xbar), _p(wbar), _p(p), _p(q), ndim, nz, ny, nx, w[0], w[1], w[2],
        float(sigma), float(beta), int(flags), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_tgv_dual")
    _wrote(p, q)
    return True


def tgv_primal(p, q, x, xbar, w_field, wbar, bt, shape, w, tau, tl, theta=1., flags=0):
    """The primal half, x, w_field, xbar and wbar in place: x <- prox_{tl D}(x - tau
    grad^T p), w_a <- w_a - tau (-p_a + D_a^T q_aa + sum_{b != a} D_b^T q_ab), the bars
    extrapolated by theta.  flags: PD_DATA_L1.  Returns False when the library declined
    the geometry (nothing was launched).  Does not synchronise."""
    _same(x, xbar, bt)
    ndim, nz, ny, nx = _tgv_operands(shape, x, (p, w_field, wbar), (q,))
    rc = _fn("tgv_primal", x)(
        _p(p), _p(q), _p(x), _p(xbar), _p(w_field), _p(wbar), _p(bt), ndim, nz, ny, nx,
        w[0], w[1], w[2], float(tau), float(tl), float(theta), int(flags), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_tgv_primal")
    _wrote(x, xbar, w_field, wbar)
    return True


def tgv_primal_w(p, q, x, xbar, w_field, wbar, bt, wt, shape, w, tau, tl, theta=1.,
                 flags=0):
    """tgv_primal with per-voxel weights wt >= 0 on the data term: x <- prox_data_w(x -
    tau grad^T p, bt, wt, tl); a voxel with wt == 0 keeps its u, whatever bt holds there.
    flags: PD_DATA_L1.  Returns False when the library declined the geometry (nothing was
    launched).  Does not synchronise."""
    _same(x, xbar, bt, wt)
    ndim, nz, ny, nx = _tgv_operands(shape, x, (p, w_field, wbar), (q,))
    rc = _fn("tgv_primal_w", x)(
        _p(p), _p(q), _p(x), _p(xbar), _p(w_field), _p(wbar), _p(bt), _p(wt), ndim, nz, ny,
        nx, w[0], w[1], w[2], float(tau), float(tl), float(theta), int(flags),
        stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_tgv_primal_w")
    _wrote(x, xbar, w_field, wbar)
    return True


def tgv_primal_kl(p, q, x, xbar, w_field, wbar, bt, wt, shape, w, tau, tl, theta=1.):
    """tgv_primal with the Poisson (Kullback-Leibler) data term: x <- prox_kl(x - tau
    grad^T p, bt, wt, tl) of csrc/nsol_kl.hpp, wt None: all weights 1; w_field and the
    bars as in tgv_primal.  Returns False when the library declined the geometry (nothing
    was launched).  Does not synchronise."""
    _same(x, xbar, bt)
    if wt is not None:
        _same(x, wt)
    ndim, nz, ny, nx = _tgv_operands(shape, x, (p, w_field, wbar), (q,))
    rc = _fn("tgv_primal_kl", x)(
        _p(p), _p(q), _p(x), _p(xbar), _p(w_field), _p(wbar), _p(bt), _p(wt), ndim, nz, ny,
        nx, w[0], w[1], w[2], float(tau), float(tl), float(theta), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_tgv_primal_kl")
    _wrote(x, xbar, w_field, wbar)
    return True


def tgv_primal_lin(p, q, x, xbar, w_field, wbar, g, shape, w, tau, theta=1., lo=-np.inf,
                   hi=np.inf):
    """The primal half behind a linear operator: x <- clip(x - tau (grad^T p + g), lo, hi)
    with g = A^T r in bt's place (pdl_iter's step), w_field and the bars as in tgv_primal.
    Returns False when the library declined the geometry (nothing was launched).  Does
    not synchronise."""
    _same(x, xbar, g)
    ndim, nz, ny, nx = _tgv_operands(shape, x, (p, w_field, wbar), (q,))
    rc = _fn("tgv_primal_lin", x)(
        _p(p), _p(q), _p(x), _p(xbar), _p(w_field), _p(wbar), _p(g), ndim, nz, ny, nx,
        w[0], w[1], w[2], float(tau), float(theta), float(lo), float(hi), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_tgv_primal_lin")
    _wrote(x, xbar, w_field, wbar)
    return True


# ----------------- TGV, member-stacked (k_tgv_*_stack in nsol_tgv.hip; tgv_stack.py) ----
# A stack of images of one shape or an (alpha, beta) sweep on one image: two launches per
# iteration for all members of a group.  A member's state is x, xbar, w, wbar, p and q:
# (2 + 3 dim + M) n words, M = dim (dim + 1) / 2, plus its own scaled observation and
# weights where the members do not share them.  The value is PD_BATCH_GROUP_BYTES',
# borrowed, not measured for TGV; it decides speed only.  The stacked linear form
# (tgv_linear_stack.py, tgv_lin_stack_group_size below) counts its groups against it too.
TGV_STACK_GROUP_BYTES = 256 << 20
TGV_STACK_MAX_MEMBERS = 65535


def tgv_stack_launches():
    """Successful launches of the member-stacked TGV kernels so far (tgv_launches() does
    not count them)."""
    return int(_lib.load().nsol_tgv_stack_launches())


def tgv_stack_group_size(members, n, dim, itemsize, weighted, own_data=True):
    """Members per stacked group of TGV runs: as many as keep a group's state ((2 + 3 dim
    + M) n words per member, and with own_data -- a batch -- the member's own observation
    and, weighted, its own weights; a sweep shares both) under TGV_STACK_GROUP_BYTES, at
    most TGV_STACK_MAX_MEMBERS, at least one."""
    dim, n = int(dim), int(n)
    words = 2 + 3 * dim + dim * (dim + 1) // 2
    if own_data:
        words += 2 if weighted else 1
    g = min(TGV_STACK_GROUP_BYTES // (words * n * int(itemsize)), TGV_STACK_MAX_MEMBERS)
    return int(max(1, min(int(members), g)))


def tgv_stack_table(like, beta, tl):
    """The device table of a stack's per-member scalars (beta[m], tl[m] = tau / alpha_m
    and the prox denominator, in the element type of `like`) for tgv_stack_dual and
    tgv_stack_primal: one table for all iterations of a run.  Returns None when the
    library declined the member count."""
    beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
    tl = np.ascontiguousarray(tl, dtype=np.float64).reshape(-1)
    if beta.size != tl.size:
        raise ValueError("%d values of beta, %d of tl" % (beta.size, tl.size))
    _chk(like)
    _sweep_staging[:] = [s for s in _sweep_staging if not s[0].query()]
    nbytes = max(16, 4 * like.element_size() * beta.size)
    tab_host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    tab = torch.empty(nbytes, dtype=torch.uint8, device=like.device)
    rc = _fn("tgv_stack_table", like)(
        int(beta.size), beta.ctypes.data, tl.ctypes.data, tab_host.data_ptr(), _p(tab),
        nbytes, stream_ptr())
    if rc == -2:
        return None
    _lib.check(rc, "nsol_tgv_stack_table")
    _table_keep(tab_host)
    return tab


def _tgv_stack_operands(members, shape, x_like, scalars, vectors, tensors, tab):
    """Checks the stacks of a member-stacked TGV call: members * n values in every tensor
    of `scalars`, members * ndim * n in `vectors`, members * M * n in `tensors`, all in the
    element type of x_like, and a table with a row for every member."""
    ndim, nz, ny, nx = dims3(shape)
    n = nz * ny * nx
    members = int(members)
    if members < 1:
        return ndim, nz, ny, nx, n          # (the library declines it)
    for group, size in ((scalars, n), (vectors, ndim * n),
                        (tensors, ndim * (ndim + 1) // 2 * n)):
        for t in group:
            if _chk(t).dtype != x_like.dtype or t.numel() != members * size:
                raise ValueError("operand mismatch: %s[%d] where %s[%d] is expected for "
                                 "%d members of shape %r" % (
                                     str(t.dtype), t.numel(), str(x_like.dtype),
                                     members * size, members, tuple(shape)))
    if _chk(tab).numel() < 4 * x_like.element_size() * members:
        raise ValueError("the table has no row for %d members" % members)
    return ndim, nz, ny, nx, n


def _tgv_member_stride(t, x_like, members, n, what):
    """0 (one array shared by the members) or n (every member its own)."""
    if _chk(t).dtype != x_like.dtype or t.numel() not in (n, members * n):
        raise ValueError("operand mismatch: %s holds %s[%d], neither %d nor %d x %d "
                         "values" % (what, str(t.dtype), t.numel(), n, members, n))
    return 0 if t.numel() == n else n


def tgv_stack_dual(xbar, wbar, p, q, members, shape, w, sigma, tab, flags=0):
    """tgv_dual on `members` stacked problems in one launch: every array holds the
    members one after the other, beta comes from tgv_stack_table's table.  Returns False
    when the library declined (nothing was launched).  Does not synchronise."""
    ndim, nz, ny, nx, _ = _tgv_stack_operands(members, shape, xbar, (xbar,), (wbar, p),
                                              (q,), tab)
    rc = _fn("tgv_stack_dual", xbar)(
        _p(xbar), _p(wbar), _p(p), _p(q), int(members), ndim, nz, ny, nx, w[0], w[1], w[2],
        float(sigma), _p(tab), int(flags), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_tgv_stack_dual")
    _wrote(p, q)
    return True


def tgv_stack_primal(p, q, x, xbar, w_field, wbar, bt, members, shape, w, tau, tab,
                     theta=1., flags=0, wt=None):
    """tgv_primal (wt None) or tgv_primal_w on `members` stacked problems in one launch;
    bt and wt hold n values shared by the members or members * n, each on its own; tl
    comes from tgv_stack_table's table.  Returns False when the library declined (nothing
    was launched).  Does not synchronise."""
    ndim, nz, ny, nx, n = _tgv_stack_operands(members, shape, x, (x, xbar),
                                              (p, w_field, wbar), (q,), tab)
    members = int(members)
    bts = _tgv_member_stride(bt, x, members, n, "bt") if members >= 1 else 0
    if wt is None:
        rc = _fn("tgv_stack_primal", x)(
            _p(p), _p(q), _p(x), _p(xbar), _p(w_field), _p(wbar), _p(bt), bts, members,
            ndim, nz, ny, nx, w[0], w[1], w[2], float(tau), float(theta), _p(tab),
            int(flags), stream_ptr())
    else:
        wts = _tgv_member_stride(wt, x, members, n, "wt") if members >= 1 else 0
        rc = _fn("tgv_stack_primal_w", x)(
            _p(p), _p(q), _p(x), _p(xbar), _p(w_field), _p(wbar), _p(bt), bts, _p(wt), wts,
            members, ndim, nz, ny, nx, w[0], w[1], w[2], float(tau), float(theta), _p(tab),
            int(flags), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_tgv_stack_primal" + ("" if wt is None else "_w"))
    _wrote(x, xbar, w_field, wbar)
    return True


def tgv_stack_primal_lin(p, q, x, xbar, w_field, wbar, g, members, shape, w, tau,
                         theta=1., lo=-np.inf, hi=np.inf):
    """tgv_primal_lin on `members` stacked problems in one launch: every array holds the
    members one after the other, g = A^T r included (every member has its own); tau,
    theta and the box are common to the stack, so there is no table.  Returns False when
    the library declined (nothing was launched).  Does not synchronise."""
    members = int(members)
    ndim, nz, ny, nx = dims3(shape)
    if members >= 1:
        n = nz * ny * nx
        for group, size in (((x, xbar, g), n), ((p, w_field, wbar), ndim * n),
                            ((q,), ndim * (ndim + 1) // 2 * n)):
            for t in group:
                if _chk(t).dtype != x.dtype or t.numel() != members * size:
                    raise ValueError("operand mismatch: %s[%d] where %s[%d] is expected "
                                     "for %d members of shape %r" % (
                                         str(t.dtype), t.numel(), str(x.dtype),
                                         members * size, members, tuple(shape)))
    rc = _fn("tgv_stack_primal_lin", x)(
        _p(p), _p(q), _p(x), _p(xbar), _p(w_field), _p(wbar), _p(g), members, ndim, nz, ny,
        nx, w[0], w[1], w[2], float(tau), float(theta), float(lo), float(hi), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_tgv_stack_primal_lin")
    _wrote(x, xbar, w_field, wbar)
    return True


def tgv_lin_stack_group_size(members, n, dim, itemsize, own_data=True, own_weights=False,
                             with_t=False):
    """Members per stacked group of TGVPrimalDualLinearSolver runs: (2 + 3 dim + M + 2) n
    words per member -- x and xbar; w, wbar and p; q; r and g = A^T r -- and one more
    each for t = A xbar (with_t: the blur runs without its epilogue), the member's own
    observation (own_data) and its own weights (own_weights), under
    TGV_STACK_GROUP_BYTES, at most TGV_STACK_MAX_MEMBERS, at least one."""
    dim, n = int(dim), int(n)
    words = 2 + 3 * dim + dim * (dim + 1) // 2 + 2 + int(bool(with_t)) + \
        int(bool(own_data)) + int(bool(own_weights))
    g = min(TGV_STACK_GROUP_BYTES // (words * n * int(itemsize)), TGV_STACK_MAX_MEMBERS)
    return int(max(1, min(int(members), g)))


# ------------------------------ the same, member-stacked (nsol_pdls.hip) ----
# An alpha sweep on one observation or a stack of images of one shape
# (nsol_amd/linear_stack.py).  A member's state is x, two xbar, q, g = A^T q and two p
# (5 + 2 dim arrays), plus its own scaled observation, its own weights and t = A xbar
# where the caller counts them (a sweep shares the first two, the blur's epilogue
# spares the third).  The constant decides speed only, as the other stacks' do.
PDL_STACK_GROUP_BYTES = 256 << 20


def pdl_stack_launches():
    """Launches of k_pdl_stack / k_pdl_stack_iso so far (for tests and tools)."""
    return int(_lib.load().nsol_pdl_stack_launches())


def pdl_group_size(members, n, dim, elem_size, own_data=True, own_weights=False,
                   with_t=True):
    """Members per stacked group of PrimalDualLinearSolver runs: 5 + 2 dim arrays per
    member and one more each for a member's own observation (own_data), its own
    weights (own_weights) and t = A xbar (with_t), under PDL_STACK_GROUP_BYTES, at
    most 65535 members."""
    arrays = 5 + int(bool(own_data)) + int(bool(own_weights)) + int(bool(with_t))
    return _group_size(members, n, dim, elem_size, arrays, PDL_STACK_GROUP_BYTES, 65535)


def pdl_lambdas(lmbda, like):
    """The members' lambdas as pdl_stack_dual_data takes them: a device array in the
    element type of `like`, each rounded as pdl_dual_data rounds its own."""
    lm = np.ascontiguousarray(lmbda, dtype=np.float64).reshape(-1)
    if lm.size < 1 or not np.all(lm >= 0):
        raise ValueError("lmbda: at least one value, all >= 0")
    host = lm.astype(np.float32 if like.dtype == torch.float32 else np.float64)
    return torch.from_numpy(host).to(like.device)


def pdl_stack_dual_data(q, t, bt, wt, sigma, lmbda, members, l1=False):
    """pdl_dual_data on `members` stacked runs in one launch: q (and t, where given)
    hold members * n elements, member-major; bt and wt (None: all 1) hold n elements
    (shared by the members) or members * n (member-major), each on its own; lmbda is
    pdl_lambdas' device array.  Every member's q has the bits pdl_dual_data gives it
    alone.  Returns False when the library declined (nothing was launched).  Does not
    synchronise."""
    members, n, bts, wts = _pdl_stack_operands(q, t, bt, wt, lmbda, members)
    rc = _fn("pdl_stack_dual_data", q)(
        _p(q), _p(t), _p(bt), bts, _p(wt), wts, float(sigma), _p(lmbda), int(bool(l1)),
        members, n, stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pdl_stack_dual_data")
    _wrote(q)
    return True


def pdl_stack_dual_data_kl(q, t, bt, wt, sigma, lmbda, members, background=0.):
    """pdl_dual_data_kl on `members` stacked runs in one launch, operands as
    pdl_stack_dual_data's; the background is common to the stack.  Every member's q has
    the bits pdl_dual_data_kl gives it alone.  Returns False when the library declined
    (nothing was launched).  Does not synchronise."""
    members, n, bts, wts = _pdl_stack_operands(q, t, bt, wt, lmbda, members)
    rc = _fn("pdl_stack_dual_data_kl", q)(
        _p(q), _p(t), _p(bt), bts, _p(wt), wts, float(sigma), _p(lmbda),
        float(background), members, n, stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pdl_stack_dual_data_kl")
    _wrote(q)
    return True


def _pdl_stack_operands(q, t, bt, wt, lmbda, members):
    """(members, n, bt's member stride, wt's) of a stacked update of q, checked."""
    members = int(members)
    _chk(q)
    _chk(bt)
    _chk(lmbda)
    if members < 1 or q.numel() % members:
        raise ValueError("operand mismatch: q[%d] for %d members" % (q.numel(), members))
    n = q.numel() // members
    if t is not None:
        _same(q, t)
    if wt is not None:
        _chk(wt)
    if bt.dtype != q.dtype or lmbda.dtype != q.dtype or lmbda.numel() != members or \
            bt.numel() not in (n, members * n) or \
            (wt is not None and (wt.dtype != q.dtype or
                                 wt.numel() not in (n, members * n))):
        raise ValueError("operand mismatch: %d members of %d elements against bt[%d], "
                         "wt[%s], lmbda[%d]" % (
                             members, n, bt.numel(),
                             "-" if wt is None else wt.numel(), lmbda.numel()))
    bts = 0 if bt.numel() == n else n
    wts = 0 if wt is None or wt.numel() == n else n
    return members, n, bts, wts


def pdl_stack_iter(xbar_in, xbar_out, x, g, p_in, p_out, members, shape, w, sigma, hden,
                   tau, theta, lo, hi, flags, has_p=True):
    """pdl_iter on `members` stacked runs in one launch: x, xbar_in/out and g hold
    members * n elements, p_in/out members * dim * n, member-major; the scalars, the
    flags and the box are common to the stack.  Every member has the bits pdl_iter
    gives it alone.  Returns False when the library declined (nothing was launched).
    Does not synchronise."""
    ndim, nz, ny, nx = dims3(shape)
    members = int(members)
    n = nz * ny * nx
    _same(x, xbar_in, xbar_out, g)
    _same(p_out, p_in)
    if p_out.dtype != x.dtype or members < 1 or x.numel() != members * n or \
            p_out.numel() != members * ndim * n:
        raise ValueError("operand mismatch: %d members of shape %r against x %s[%d], "
                         "p %s[%d]" % (members, tuple(shape), str(x.dtype), x.numel(),
                                       str(p_out.dtype), p_out.numel()))
    rc = _fn("pdl_stack_iter", x)(
        _p(xbar_in), _p(xbar_out), _p(x), _p(g), _p(p_in), _p(p_out), members, ndim, nz,
        ny, nx, w[0], w[1], w[2], float(sigma), float(hden), float(tau), float(theta),
        float(lo), float(hi), int(flags), int(bool(has_p)), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pdl_stack_iter")
    _wrote(xbar_out, x, p_out)
    return True


# ------------------------------------------------------ stopping rule ----
# (nsol_pdc.hip; the rule itself is primal_dual_solver.py's)
PD_CHECK_SUMS = 4


def pd_check_launches():
    """Calls of pd_check_iter so far (for tests and tools)."""
    return _check_launches


_check_launches = 0


def pd_check_workspace(like, shape):
    """The float64 device scratch pd_check_iter and pd_change need for a volume of
    `shape` in the element type of `like` (nsol_pd_check_ws_doubles)."""
    ndim, nz, ny, nx = dims3(shape)
    need = int(_lib.load().nsol_pd_check_ws_doubles(int(like.element_size()), ndim, nz,
                                                    ny, nx))
    if need < 0:
        raise ValueError("nsol_pd_check does not take a volume of shape %r" %
                         (tuple(shape),))
    return torch.empty(need, dtype=torch.float64, device=like.device)


def _check_row(ws, row):
    _chk(ws)
    _chk(row)
    if ws.dtype != torch.float64 or row.dtype != torch.float64 or \
            row.numel() < PD_CHECK_SUMS or ws.numel() < PD_CHECK_SUMS:
        raise ValueError("ws, row: float64 device tensors of at least %d elements" %
                         PD_CHECK_SUMS)


def pd_check_iter(xbar_in, xbar_out, x, bt, wt, p_in, p_out, shape, w, sigma, hden, tau,
                  tl, theta, flags, ws, row):
    """One iteration as pd_fused_iter (wt None) or as pd_weighted_iter with one member
    (wt the weights, flags with PD_DATA_WEIGHTED) -- the same bits in xbar_out, x and
    p_out -- and the four sums of the stopping rule, {sum dx^2, sum x^2, sum dp^2,
    sum p^2} of that iteration, in row[0:4] (float64, device).  p_in None: p is zero.
    ws: pd_check_workspace().  Returns False when the library declined (nothing was
    launched).  Does not synchronise."""
    global _check_launches
    ndim, nz, ny, nx = dims3(shape)
    n = nz * ny * nx
    _same(x, xbar_in, xbar_out, bt)
    _chk(p_out)
    _check_row(ws, row)
    weighted = bool(int(flags) & PD_DATA_WEIGHTED)
    if weighted != (wt is not None):
        raise ValueError("weights go with PD_DATA_WEIGHTED, and only with it")
    for t, size in ((wt, n), (p_in, ndim * n), (p_out, ndim * n)):
        if t is not None and (_chk(t).dtype != x.dtype or t.numel() != size):
            raise ValueError("operand mismatch: %s[%d] where %s[%d] is expected" %
                             (str(t.dtype), t.numel(), str(x.dtype), size))
    if x.numel() != n:
        raise ValueError("x does not hold a volume of shape %r" % (tuple(shape),))
    rc = _fn("pd_check_iter", x)(
        _p(xbar_in), _p(xbar_out), _p(x), _p(bt), _p(wt), _p(p_in), _p(p_out), ndim, nz,
        ny, nx, w[0], w[1], w[2], float(sigma), float(hden), float(tau), float(tl),
        float(theta), int(flags), _p(ws), ws.numel(), _p(row), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pd_check_iter")
    _wrote(xbar_out, x, p_out, row)
    _check_launches += 1
    return True


def pd_change(x_old, x_new, p_old, p_new, ws, row):
    """The four sums of the stopping rule from the iterates before and after an
    iteration (p_old None: p was zero) into row[0:4]; for the loops of separate
    kernels.  Does not synchronise."""
    _same(x_new, x_old)
    _chk(p_new)
    _check_row(ws, row)
    if p_new.dtype != x_new.dtype or (p_old is not None and (
            _chk(p_old).dtype != p_new.dtype or p_old.numel() != p_new.numel())):
        raise ValueError("operand mismatch between x and p, or p_old and p_new")
    _lib.check(_fn("pd_change", x_new)(
        _p(x_old), _p(x_new), x_new.numel(), _p(p_old), _p(p_new), p_new.numel(),
        _p(ws), ws.numel(), _p(row), stream_ptr()), "nsol_pd_change")
    return _wrote(row)


# ------------------------------------- stacks that stop member by member ----
# (nsol_pdm.hip; the host loop is nsol_amd/stacked_stopping.py)
def pd_stack_launches():
    """Launches of the member-mapped stacked kernels so far (for tests and tools)."""
    return int(_lib.load().nsol_pd_stack_launches())


def pd_stack_workspace(like, shape, members):
    """The float64 device scratch pd_stack_iter's checking form needs for a group of
    `members` volumes of `shape` in the element type of `like`, whatever number of
    them is active (nsol_pd_stack_ws_doubles)."""
    ndim, nz, ny, nx = dims3(shape)
    need = int(_lib.load().nsol_pd_stack_ws_doubles(int(like.element_size()), ndim, nz,
                                                    ny, nx, int(members)))
    if need < 0:
        raise ValueError("nsol_pd_stack does not take %d volumes of shape %r" %
                         (int(members), tuple(shape)))
    return torch.empty(need, dtype=torch.float64, device=like.device)


def pd_stack_iter(xbar_in, xbar_out, x, bt, wt, p_in, p_out, members, map, active,
                  shape, w, tab, iteration, flags, ws=None, rows=None):
    """One launch: iteration `iteration` of the table (pd_weighted_table's layout, row
    stride `members`) for the `active` members map[0:active] of a group of `members`
    stacked runs.  map: an int32 device tensor of strictly increasing member indices in
    [0, members); a member that is not in it is not touched.  Layout as
    pd_weighted_iter: bt and wt hold n elements (shared) or members * n (member-major);
    wt goes with PD_DATA_WEIGHTED, and only with it.  rows None: the plain form.  rows
    a float64 device tensor of 4 * members: the checking form, the four sums of the
    stopping rule of every active member m in rows[4 m : 4 m + 4], ws from
    pd_stack_workspace().  Returns False when the library declined (nothing was
    launched).  Does not synchronise."""
    members, active = int(members), int(active)
    ndim, nz, ny, nx = dims3(shape)
    n = nz * ny * nx
    _same(x, xbar_in, xbar_out)
    _same(p_in, p_out)
    _chk(bt)
    _chk(map)
    weighted = bool(int(flags) & PD_DATA_WEIGHTED)
    if weighted != (wt is not None):
        raise ValueError("weights go with PD_DATA_WEIGHTED, and only with it")
    if p_in.dtype != x.dtype or bt.dtype != x.dtype or members < 1 or \
            x.numel() != members * n or p_in.numel() != members * ndim * n or \
            bt.numel() not in (n, members * n) or (wt is not None and (
                _chk(wt).dtype != x.dtype or wt.numel() not in (n, members * n))):
        raise ValueError("operand mismatch: %d members of %d voxels against x[%d], "
                         "bt[%d], p[%d]" % (members, n, x.numel(), bt.numel(),
                                            p_in.numel()))
    if map.dtype != torch.int32 or not 0 <= active <= members or map.numel() < active:
        raise ValueError("map: an int32 device tensor of at least `active` entries, "
                         "0 <= active <= members")
    if rows is not None:
        _chk(rows)
        if ws is None or _chk(ws).dtype != torch.float64 or \
                rows.dtype != torch.float64 or rows.numel() < PD_CHECK_SUMS * members:
            raise ValueError("rows: a float64 device tensor of %d per member, with a "
                             "float64 workspace" % PD_CHECK_SUMS)
    _table_has(tab, x, members, iteration)
    bts = 0 if bt.numel() == n else n
    wts = 0 if wt is None or wt.numel() == n else n
    rc = _fn("pd_stack_iter", x)(
        _p(xbar_in), _p(xbar_out), _p(x), _p(bt), bts, _p(wt), wts, _p(p_in), _p(p_out),
        members, _p(map), active, ndim, nz, ny, nx, w[0], w[1], w[2], _p(tab),
        int(iteration), int(flags), _p(ws) if rows is not None else None,
        ws.numel() if rows is not None else 0, _p(rows), stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_pd_stack_iter")
    if active:
        _wrote(xbar_out, x, p_out, rows)
    return True


# ----------------------------------------------------------------- ADMM ----
def admm_vw_update(x, v, w_, c, rhs, shape, w, thr, rhs_scale, want_norm=False):
    """v, w_ and the next right-hand side rhs = rhs_scale * (v - w_ + c) from one
    pass over x; want_norm: returns sum(rhs^2) (syncs)."""
    ndim, nz, ny, nx = dims3(shape)
    if want_norm:
        ws, res = _workspace(x.device)
        _lib.check(_fn("admm_vw_update_norm", x)(
            _p(x), _p(v), _p(w_), _p(c), _p(rhs), ndim, nz, ny, nx, w[0], w[1],
            w[2], float(thr), float(rhs_scale), _p(res), _p(ws), stream_ptr()),
            "nsol_admm_vw_update_norm")
        _wrote(v, w_, rhs)
        return float(res.item())
    _lib.check(_fn("admm_vw_update", x)(
        _p(x), _p(v), _p(w_), _p(c), _p(rhs), ndim, nz, ny, nx, w[0], w[1],
        w[2], float(thr), float(rhs_scale), stream_ptr()),
        "nsol_admm_vw_update")
    _wrote(v, w_, rhs)


def admm_vw_update_g(x, w_in, w_out, c, atb, g, shape, w, thr, rhs_scale, c_atu, c_btu,
                     result):
    """The outer update and the vector the next x-update's LSMR starts from in one pass
    (nsol_admm_vw_update_g_*): w_out, g as admm_vw_update(x, None, w, c, rhs, ...,
    rhs_scale) followed by lsmr_v_update(atb, rhs, atb, B_GRAD, ..., c_atu, c_btu, 0,
    out=g) leave them, rhs never written; result[0] = sum rhs^2, result[1] = sum g^2
    (the caller's two-element float64 device tensor, not read back here).  False when
    the kernel does not apply (nothing launched)."""
    _same(x, atb, g)
    _same(w_in, w_out)
    if c is not None:
        _same(w_in, c)
    ndim, nz, ny, nx = dims3(shape)
    if w_in.dtype != x.dtype or w_in.numel() != ndim * x.numel() or \
            nz * ny * nx != x.numel():
        raise ValueError("admm_vw_update_g: operand sizes do not fit shape %r" %
                         (tuple(shape),))
    _chk(result)
    if result.numel() != 2 or result.dtype != torch.float64:
        raise ValueError("admm_vw_update_g: result must hold two float64 values")
    ws, _ = _workspace(x.device)
    rc = _fn("admm_vw_update_g", x)(
        _p(x), _p(w_in), _p(w_out), _p(c), _p(atb), _p(g), ndim, nz, ny, nx, w[0], w[1],
        w[2], float(thr), float(rhs_scale), float(c_atu), float(c_btu), _p(result), _p(ws),
        stream_ptr())
    if rc == -2:
        return False
    _lib.check(rc, "nsol_admm_vw_update_g")
    _wrote(w_out, g)
    return True


def vector_shrink(t, ndim, thr, out=None):
    _chk(t)
    if out is None:
        out = empty_like(t)
    _lib.check(_fn("vector_shrink", t)(_p(t), _p(out), int(ndim),
                                       t.numel() // int(ndim), float(thr),
                                       stream_ptr()), "nsol_vector_shrink")
    return _wrote(out)


# ----------------------------------------------------------------- LSMR ----
B_NONE, B_GRAD, B_IDENTITY = 0, 1, 2


def flat_geometry(n):
    """(ny, nx) with ny * nx = n for the element-wise modes of the LSMR kernels
    (B = identity / no regulariser): their thread mapping wants rows of at most
    a few thousand elements, a flat vector of 512^3 elements is folded; without
    a suitable power-of-two factor it stays one long row (the stencil mapping
    then loops over x)."""
    n = int(n)
    if n <= (1 << 16):
        return 1, n
    for nx in (4096, 2048, 1024, 512, 256, 128, 64):
        if n % nx == 0:
            return n // nx, nx
    return 1, n


def _bgeom(bmode, shape, w, n):
    if bmode == B_GRAD:
        return dims3(shape), w
    geom = flat_geometry(n)
    if geom is None:
        raise ValueError("no row folding for a vector of %d elements" % n)
    ny, nx = geom
    return ((1 if ny == 1 else 2), 1, ny, nx), (1.0, 1.0, 1.0)


def lsmr_u_update(Av, v, u_top, u_bot, bmode, shape, w, c_av, c_bv, c_u,
                  sync=True, result=None):
    """u_top = c_av*Av + c_u*u_top; u_bot = c_bv*B(v) + c_u*u_bot;
    returns ||[u_top; u_bot]||^2 (sync=False: the device scalar, not read
    back)."""
    if Av is None:               # lower block only (top: corr3_wrap_axpby)
        _same(u_top, v)
        Av_ptr, nn = None, u_top.numel()
    else:
        _same(Av, v, u_top)
        Av_ptr, nn = Av, Av.numel()
    if u_bot is not None:
        _chk(u_bot)
        rows = (len(tuple(shape)) if bmode == B_GRAD else 1) * nn
        if u_bot.dtype != u_top.dtype or u_bot.numel() != rows:
            raise ValueError("lsmr_u_update: lower block has %d elements, "
                             "expected %d" % (u_bot.numel(), rows))
    (ndim, nz, ny, nx), w = _bgeom(bmode, shape, w, nn)
    ws, res = _workspace(u_top.device)
    if result is not None:       # the caller's slot: not read back here
        res, sync = result, False
    _lib.check(_fn("lsmr_u_update", u_top)(
        _p(Av_ptr), _p(v), _p(u_top), _p(u_bot), int(bmode), ndim, nz, ny, nx,
        w[0], w[1], w[2], float(c_av), float(c_bv), float(c_u), _p(res),
        _p(ws), stream_ptr()), "nsol_lsmr_u_update")
    _wrote(u_top, u_bot)
    return float(res.item()) if sync else res


def lsmr_v_update(Atu, u_bot, v, bmode, shape, w, c_atu, c_btu, c_v,
                  sync=True, out=None, result=None):
    """v = c_atu*Atu + c_btu*B^T(u_bot) + c_v*v; returns ||v||^2.  out: where
    the new vector goes instead of v (may be Atu: v then stays as it was)."""
    _same(Atu, v)
    if out is not None:
        _same(Atu, out)
    if u_bot is not None:
        _chk(u_bot)
        rows = (len(tuple(shape)) if bmode == B_GRAD else 1) * Atu.numel()
        if u_bot.dtype != Atu.dtype or u_bot.numel() != rows:
            raise ValueError("lsmr_v_update: lower block has %d elements, "
                             "expected %d" % (u_bot.numel(), rows))
    (ndim, nz, ny, nx), w = _bgeom(bmode, shape, w, Atu.numel())
    ws, res = _workspace(Atu.device)
    if result is not None:       # the caller's slot: not read back here
        res, sync = result, False
    if out is not None:
        _lib.check(_fn("lsmr_v_update_to", Atu)(
            _p(Atu), _p(u_bot), _p(v), _p(out), int(bmode), ndim, nz, ny, nx,
            w[0], w[1], w[2], float(c_atu), float(c_btu), float(c_v), _p(res),
            _p(ws), stream_ptr()), "nsol_lsmr_v_update_to")
        _wrote(out)
        return float(res.item()) if sync else res
    _lib.check(_fn("lsmr_v_update", Atu)(
        _p(Atu), _p(u_bot), _p(v), int(bmode), ndim, nz, ny, nx, w[0], w[1],
        w[2], float(c_atu), float(c_btu), float(c_v), _p(res), _p(ws),
        stream_ptr()), "nsol_lsmr_v_update")
    _wrote(v)
    return float(res.item()) if sync else res


def lsmr_hx_update(hbar, x, h, v, c_hbar, c_x, c_h, c_v, sync=True):
    """hbar = h + c_hbar*hbar; x += c_x*hbar; h = c_v*v + c_h*h;
    returns ||x||^2."""
    _same(x, hbar, h, v)
    ws, res = _workspace(x.device)
    _lib.check(_fn("lsmr_hx_update", x)(
        _p(hbar), _p(x), _p(h), _p(v), x.numel(), float(c_hbar), float(c_x),
        float(c_h), float(c_v), _p(res), _p(ws), stream_ptr()),
        "nsol_lsmr_hx_update")
    _wrote(hbar, x, h)
    return float(res.item()) if sync else res
