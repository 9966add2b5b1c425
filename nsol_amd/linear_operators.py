"""Linear operators of the NSoL hot path on MI355X (drop-in for
nsol/linear_operators.py).

The factories keep the reference's names and return CALLABLE OBJECTS instead of
lambdas.  A callable accepts
  * an N-D NumPy array  -> uploads, runs the HIP kernel, returns a NumPy array
    of the same float dtype (float64 unless the input is float32);
  * an N-D torch HIP tensor (float32/float64) -> returns a device tensor, no
    host traffic (what the solvers use);
  * the solvers' symbolic probe (symbolic.Sym) -> describes itself so that
    PrimalDualSolver / ADMMLinearSolver can dispatch to fused kernels.
Shapes follow the reference: grad maps (Z,Y,X) -> (3Z,Y,X) (linear_operators.py:140).
"""
import numpy as np

from . import kernels as Kernels
from . import ops
from .device import is_device_tensor, to_device, to_numpy
from .symbolic import Sym, TraceAbort


def _stacked_shape(shape, dim):
    shape = tuple(shape)
    if dim == 1:
        return shape
    return (dim * shape[0],) + shape[1:]


def _unstacked_shape(shape, dim):
    shape = tuple(shape)
    if dim == 1:
        return shape
    if shape[0] % dim:
        raise ValueError("leading axis %d is not a multiple of %d" %
                         (shape[0], dim))
    return (shape[0] // dim,) + shape[1:]


class DeviceOperator(object):
    """Common host/device/symbolic dispatch."""

    kind = "operator"

    def _out_shape(self, in_shape):
        return tuple(in_shape)

    def _apply(self, x, in_shape):  # x: flat contiguous device tensor
        raise NotImplementedError

    def _describe(self, in_shape):
        return (self.kind, self, tuple(in_shape))

    def __call__(self, x):
        if isinstance(x, Sym):
            if x.desc is not None:
                raise TraceAbort("composition of operators is not fused")
            return Sym(self._out_shape(x.shape), self._describe(x.shape))
        if is_device_tensor(x):
            shape = tuple(x.shape)
            out = self._apply(x.contiguous().view(-1), shape)
            return out.view(self._out_shape(shape))
        arr = np.asarray(x)
        dt = arr.dtype.type if arr.dtype in (np.float32, np.float64) \
            else np.float64
        out = self._apply(to_device(arr, dt).view(-1), arr.shape)
        return to_numpy(out, dt).reshape(self._out_shape(arr.shape))


class _DimChecked(DeviceOperator):

    def __init__(self, dimension, spacing):
        self.dimension = dimension
        self.spacing = np.atleast_1d(spacing).astype(float)
        self.w = ops.inv_spacing(self.spacing, dimension)

    def _check(self, shape, stacked=False):
        if len(shape) != self.dimension:
            raise RuntimeError(
                "%dD operator applied to an array with %d axes" %
                (self.dimension, len(shape)))


class GradientOperator(_DimChecked):
    """K = nabla, zero-padded forward differences stacked on axis 0
    (linear_operators.py:121-144, mode="constant")."""
    kind = "grad"

    def _out_shape(self, in_shape):
        return _stacked_shape(in_shape, self.dimension)

    def _apply(self, x, in_shape):
        self._check(in_shape)
        return ops.grad(x, in_shape, self.w)


class GradientAdjointOperator(_DimChecked):
    """K^T (linear_operators.py:158-169)."""
    kind = "grad_adj"

    def _out_shape(self, in_shape):
        return _unstacked_shape(in_shape, self.dimension)

    def _apply(self, p, in_shape):
        self._check(in_shape)
        return ops.grad_adj(p, _unstacked_shape(in_shape, self.dimension),
                            self.w)


class AxisDifferenceOperator(_DimChecked):
    """D_a or D_a^T along one direction (linear_operators.py:98-106)."""
    kind = "diff"

    def __init__(self, dimension, spacing, direction, adjoint):
        _DimChecked.__init__(self, dimension, spacing)
        self.direction = direction
        self.adjoint = adjoint

    def _describe(self, in_shape):
        return (self.kind, self, tuple(in_shape))

    def _apply(self, x, in_shape):
        self._check(in_shape)
        return ops.diff_axis(x, in_shape, self.direction, self.adjoint,
                             self.w[self.direction])


def _ndimage_convolve_params(kernel):
    """scipy.ndimage.convolve(x, k) == correlate(x, flip(k)) with the centre
    of the flipped kernel at size//2 (odd) or size//2-1 (even)."""
    flipped = kernel[tuple([slice(None, None, -1)] * kernel.ndim)]
    centre = [s // 2 - (1 if s % 2 == 0 else 0) for s in kernel.shape]
    return np.ascontiguousarray(flipped, dtype=np.float64), centre


def _rank1_factors(kernel, tol=1e-13):
    """Per-axis factors if the tap array is an outer product, else None."""
    if kernel.ndim == 1:
        return [kernel]
    total = kernel.sum()
    if total == 0:
        return None
    facs = [kernel.sum(axis=tuple(a for a in range(kernel.ndim) if a != ax))
            for ax in range(kernel.ndim)]
    rebuilt = facs[0]
    for f in facs[1:]:
        rebuilt = np.multiply.outer(rebuilt, f)
    rebuilt = rebuilt / total ** (kernel.ndim - 1)
    if np.max(np.abs(rebuilt - kernel)) > tol * np.max(np.abs(kernel)):
        return None
    facs[0] = facs[0] / total ** (kernel.ndim - 1)
    return facs


# one-pass 3-D blur (nsol_corr3_wrap_*); False = always three 1-D passes
USE_FUSED_BLUR3 = True
# LSMR's top-block update as the epilogue of that blur (nsol_corr3_wrap_axpby_*)
USE_BLUR_EPILOGUE = True
# dense taps through the tiled kernel (nsol_corr_dense_tiled_*) where its planner takes
# the shape; False = always the plain one (nsol_corr_dense_*).  The bits are the same.
USE_TILED_DENSE = True


class ConvolutionOperator(DeviceOperator):
    """x -> scipy.ndimage.convolve(x, kernel, mode) on the GPU
    (linear_operators.py:60-68).  Separable kernels (every Gaussian with a
    diagonal covariance) run as 1-D passes, anything else as dense taps."""
    kind = "conv"

    def __init__(self, dimension, kernel, mode="wrap"):
        kernel = np.asarray(kernel, dtype=np.float64)
        if kernel.ndim != dimension:
            raise RuntimeError("filter weights array has incorrect shape.")
        if mode not in ops.MODES:
            raise RuntimeError("boundary mode not supported")
        self.dimension = dimension
        self.kernel = kernel
        self.mode = mode
        flipped, centre = _ndimage_convolve_params(kernel)
        self._flipped, self._centre = flipped, centre
        facs = _rank1_factors(flipped)
        if facs is not None and max(f.size for f in facs) <= 129:
            self._passes = [(ax + 3 - dimension, facs[ax], centre[ax])
                            for ax in range(dimension)
                            if not (facs[ax].size == 1 and facs[ax][0] == 1.0)]
        else:
            self._passes = None
        self._taps_dev = {}

    @property
    def separable(self):
        return self._passes is not None

    def _fusable3(self):
        """Three periodic passes with the same odd tap count, centred: one
        launch of nsol_corr3_wrap_* instead of three of nsol_corr_axis_*."""
        p = self._passes
        return (self.dimension == 3 and self.mode == "wrap" and len(p) == 3
                and [a for a, _, _ in p] == [0, 1, 2]
                and len({t.size for _, t, _ in p}) == 1
                and p[0][1].size % 2 == 1
                and all(c == t.size // 2 for _, t, c in p))

    def apply_axpby(self, x, io, in_shape, ca, cb, result=None):
        """io = ca * A(x) + cb * io in place with the sum of squares of the
        result (flat device tensors; the top block of LSMR's u update as the
        epilogue of the one-pass blur).  None when that kernel does not apply.
        result: the caller's one-element float64 device tensor for the sum (then
        nothing is read back)."""
        if not (USE_FUSED_BLUR3 and USE_BLUR_EPILOGUE and self._passes and
                len(in_shape) == 3 and self._fusable3()):
            return None
        return ops.corr3_wrap_axpby(x, io, in_shape, self._passes[0][1],
                                    self._passes[1][1], self._passes[2][1], ca, cb,
                                    result=result)

    def apply_norms(self, x, out, in_shape, w, result):
        """out = A(x) with result[0] = sum out^2 and result[1] = sum |grad x|^2 of
        the input (w: the gradient's weights), both from the one-pass blur; None
        when that kernel does not apply."""
        if not (USE_FUSED_BLUR3 and USE_BLUR_EPILOGUE and self._passes and
                len(in_shape) == 3 and self._fusable3()):
            return None
        return ops.corr3_wrap_norms(x, out, in_shape, self._passes[0][1],
                                    self._passes[1][1], self._passes[2][1], w, result)

    def lanczos_halves(self, in_shape):
        """(half_a, half_b) -- ops.corr3_lanczos_a / _b bound to this blur's taps -- when
        the one-pass blur can take both halves of a Lanczos step on A'A + rho B'B itself
        (symmetric separable taps on a 3-D grid), else None."""
        if not (USE_FUSED_BLUR3 and USE_BLUR_EPILOGUE and self._passes and
                len(in_shape) == 3 and self._fusable3()):
            return None
        tz, ty, tx = (self._passes[0][1], self._passes[1][1], self._passes[2][1])

        lean = bool(ops.LEAN_LANCZOS_HALVES)
        held = {}

        def half_a(y, y_prev, t, q0, lb, step):
            if lean:
                # (q0 is not formed: the second half takes y_prev itself)
                held["y_prev"] = y_prev
                return ops.corr3_lanczos_a2(y, t, in_shape, tz, ty, tx, lb, step)
            return ops.corr3_lanczos_a(y, y_prev, t, q0, in_shape, tz, ty, tx, lb, step)

        def half_b(t, q0, y, y_new, lb, step):
            if lean:
                return ops.corr3_lanczos_b2(t, y, held.get("y_prev"), y_new, in_shape, tz,
                                            ty, tx, lb, step)
            return ops.corr3_lanczos_b(t, q0, y, y_new, in_shape, tz, ty, tx, lb, step)
        half_a.lean = lean
        return half_a, half_b

    def apply_loss(self, x, b, in_shape, loss, f_scale, result):
        """rho'(r^2) r for r = A x - b with 1/2 sum rho(r^2) in the device slot `result`,
        from the one-pass blur (ops.corr3_wrap_loss); None where it does not apply."""
        if not (USE_FUSED_BLUR3 and USE_BLUR_EPILOGUE and self._passes and
                len(in_shape) == 3 and self._fusable3()):
            return None
        return ops.corr3_wrap_loss(x, b, in_shape, self._passes[0][1], self._passes[1][1],
                                   self._passes[2][1], loss, f_scale, result)

    def _apply(self, x, in_shape):
        if len(in_shape) != self.dimension:
            raise RuntimeError("%dD convolution applied to %d axes" %
                               (self.dimension, len(in_shape)))
        if self._passes is not None:
            if not self._passes:
                return x.clone()
            if USE_FUSED_BLUR3 and self._fusable3():
                res = ops.corr3_wrap(x, in_shape, self._passes[0][1],
                                     self._passes[1][1], self._passes[2][1])
                if res is not None:
                    return res
            cur = x
            for axis3, taps, centre in self._passes:
                cur = ops.corr_axis(cur, in_shape, axis3, taps, centre,
                                    self.mode)
            return cur
        key = (x.dtype, x.device.index)
        if key not in self._taps_dev:
            self._taps_dev[key] = to_device(
                self._flipped.reshape(-1),
                np.float32 if "32" in str(x.dtype) else np.float64)
        k3, c3 = self._dense3()
        if USE_TILED_DENSE:
            res = ops.corr_dense_tiled(x, in_shape, self._taps_dev[key], k3, c3,
                                       self.mode)
            if res is not None:
                return res
        return ops.corr_dense(x, in_shape, self._taps_dev[key], k3, c3,
                              self.mode)

    def _dense3(self):
        """The taps' shape and centre padded to three axes."""
        return ((1,) * (3 - self.dimension) + self._flipped.shape,
                (0,) * (3 - self.dimension) + tuple(self._centre))

    def dense_form(self, in_shape, dtype=np.float64):
        """Which kernel a dense-tap application to a volume of in_shape runs: "tiled"
        (nsol_corr_dense_tiled_*) or "plain" (nsol_corr_dense_*); None for a separable
        operator, which has no dense form.  dtype: the element type (the tiled kernel's
        ring in the LDS is twice as large in float64)."""
        if self._passes is not None:
            return None
        if len(in_shape) != self.dimension:
            raise RuntimeError("%dD convolution applied to %d axes" %
                               (self.dimension, len(in_shape)))
        if USE_TILED_DENSE and ops.corr_dense_tiled_plan(
                in_shape, self._dense3()[0], np.dtype(dtype).itemsize) is not None:
            return "tiled"
        return "plain"

    def transpose(self):
        """The exact transpose A^T as a ConvolutionOperator of the same mode: the kernel
        reversed along every axis, with one zero tap prepended along every even-sized
        axis (ndimage.convolve centres an even kernel one tap off its middle; the zero
        puts the reversed kernel's centre where the transpose has it).  An outer
        product stays one, so a separable kernel keeps its 1-D passes.  "wrap" and
        "constant" only."""
        if self.mode not in ("wrap", "constant"):
            raise ValueError("mode '%s': only 'wrap' and 'constant' have a transpose "
                             "that is a correlation" % (self.mode,))
        kt = self.kernel[tuple([slice(None, None, -1)] * self.kernel.ndim)]
        kt = np.pad(kt, [(1, 0) if s % 2 == 0 else (0, 0) for s in kt.shape])
        return ConvolutionOperator(self.dimension, kt, self.mode)


    # ---- `members` volumes of one shape, member-major in one flat tensor
    # (nsol_amd/linear_stack.py).  Every member's result has the bits _apply /
    # apply_axpby give for it alone: the kernels pick their access form from the
    # 16-byte alignment of their pointers, so a member whose slice does not start on
    # one goes through an aligned copy, as a single run's own tensors are.
    def _stack_batches_passes(self, in_shape):
        """The 1-D passes of a separable 1-D / 2-D operator run over the whole stack
        at once: no pass runs along the member axis."""
        return self._passes is not None and self.dimension < 3 and \
            len(in_shape) == self.dimension

    def stacked_launches(self, in_shape, members):
        """Launches _apply_stacked makes for `members` volumes of in_shape."""
        if self._stack_batches_passes(in_shape):
            return max(len(self._passes), 1)
        return int(members) * max(self._launches(in_shape), 1)

    def _launches(self, in_shape):
        if self._passes is None:
            return 1
        if USE_FUSED_BLUR3 and self._fusable3():
            return 1            # (three where nsol_corr3_wrap_* declines the shape)
        return len(self._passes)

    def _apply_stacked(self, x, in_shape, members, out=None):
        """A applied to every one of the `members` volumes of in_shape that the flat
        device tensor x holds; returns the flat stacked result (`out` when given).
        A separable 1-D / 2-D operator: ONE ops.corr_axis launch per pass over the
        padded shape (members, ny, nx) (1-D: (1, members, nx)).  Everything else --
        3-D, dense taps -- member by member on its slice, with exactly the call
        _apply makes."""
        members = int(members)
        n = int(np.prod(in_shape))
        if len(in_shape) != self.dimension:
            raise RuntimeError("%dD convolution applied to %d axes" %
                               (self.dimension, len(in_shape)))
        if x.numel() != members * n or (out is not None and
                                        (out.numel() != x.numel() or
                                         out.dtype != x.dtype)):
            raise ValueError("operand mismatch: %d members of %d elements against "
                             "x[%d]" % (members, n, x.numel()))
        if self._stack_batches_passes(in_shape):
            if not self._passes:
                return x.clone() if out is None else out.copy_(x)
            padded = (members,) + tuple(in_shape) if self.dimension == 2 else \
                (1, members) + tuple(in_shape)
            cur = x
            for k, (axis3, taps, centre) in enumerate(self._passes):
                last = k == len(self._passes) - 1
                cur = ops.corr_axis(cur, padded, axis3, taps, centre, self.mode,
                                    out=out if last else None)
            return cur
        if out is None:
            out = ops.empty_like(x)
        on_slices = (n * x.element_size()) % 16 == 0
        for m in range(members):
            xm = x[m * n:(m + 1) * n]
            if on_slices and USE_FUSED_BLUR3 and self._passes and self._fusable3() and \
                    ops.corr3_wrap(xm, in_shape, self._passes[0][1], self._passes[1][1],
                                   self._passes[2][1],
                                   out=out[m * n:(m + 1) * n]) is not None:
                continue
            out[m * n:(m + 1) * n].copy_(
                self._apply(xm if on_slices else xm.clone(), in_shape))
        return out

    def apply_axpby_stacked(self, x, io, in_shape, members, ca, cb, results=None):
        """apply_axpby on every one of the `members` volumes: io = ca A(x) + cb io in
        place, member by member (the one-pass blur is a 3-D kernel); results: a
        float64 device tensor with a slot per member for the sums.  None when the
        kernel does not apply -- decided on the first member, with nothing run; the
        choice depends on the shape alone, so a later member that declines is an
        error."""
        members = int(members)
        n = int(np.prod(in_shape))
        on_slices = (n * x.element_size()) % 16 == 0
        for m in range(members):
            xm, iom = x[m * n:(m + 1) * n], io[m * n:(m + 1) * n]
            slot = None if results is None else results[m:m + 1]
            if on_slices:
                got = self.apply_axpby(xm, iom, in_shape, ca, cb, result=slot)
            else:
                tmp = iom.clone()
                got = self.apply_axpby(xm.clone(), tmp, in_shape, ca, cb, result=slot)
                if got is not None:
                    iom.copy_(tmp)
            if got is None:
                if m == 0:
                    return None
                raise RuntimeError("the blur's epilogue declined member %d of a stack "
                                   "it had taken" % m)
        return results if results is not None else True


def _per_axis_ints(values, dimension, what, default):
    if values is None:
        return [default] * dimension
    try:
        vals = [v for v in np.atleast_1d(np.asarray(values, dtype=object)).tolist()]
        if len(vals) != dimension:
            raise ValueError
        out = [int(v) for v in vals]
        if any(float(v) != o for v, o in zip(vals, out)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("%s must hold one integer per array axis (%d)" %
                         (what, dimension))
    return out


class SampledConvolutionOperator(DeviceOperator):
    """Acquisition on a coarser grid, A = S G:
        x -> scipy.ndimage.convolve(x, kernel, mode)[o_0::f_0, o_1::f_1, ...]
    on the GPU, computing only the samples it keeps (ops.corr_axis_down).

    factors, offsets: one integer per ARRAY AXIS, in the order of `kernel`'s axes --
    factors[0] belongs to the first (slowest) axis.  This is NOT the reversed order
    of `spacing`, whose first entry belongs to the last array axis.  f >= 1 and
    0 <= o < f; offsets=None: zeros.  mode: "wrap" or "constant" (the transpose of
    the other boundary modes is not a correlation).  The kernel must be separable
    (an outer product, as every Gaussian with a diagonal covariance) with at most
    129 taps per axis.  Everything else raises ValueError.

    The passes run the axes with f > 1 first, largest factor first (ties in axis
    order), each on the grid the earlier ones have reduced; the axes with f = 1
    follow on the reduced grid through ops.corr_axis.  adjoint() is the exact
    transpose, the same list backwards."""
    kind = "sampled_conv"

    def __init__(self, dimension, kernel, factors, offsets=None, mode="wrap"):
        kernel = np.asarray(kernel, dtype=np.float64)
        dimension = int(dimension)
        if dimension not in (1, 2, 3) or kernel.ndim != dimension:
            raise ValueError("the kernel must have %d axes" % dimension)
        if mode not in ops.SAMPLED_MODES:
            raise ValueError("mode '%s': only 'wrap' and 'constant' have a transpose "
                             "that is a correlation" % (mode,))
        factors = _per_axis_ints(factors, dimension, "factors", 1)
        offsets = _per_axis_ints(offsets, dimension, "offsets", 0)
        if any(f < 1 for f in factors):
            raise ValueError("factors must be >= 1")
        if any(not 0 <= o < f for o, f in zip(offsets, factors)):
            raise ValueError("offsets must satisfy 0 <= offset < factor")
        flipped, centre = _ndimage_convolve_params(kernel)
        facs = _rank1_factors(flipped)
        if facs is None or max(f.size for f in facs) > 129:
            raise ValueError("the kernel must be separable with at most 129 taps per "
                             "axis (a dense form is not provided)")
        self.dimension = dimension
        self.kernel = kernel
        self.mode = mode
        self.factors, self.offsets = tuple(factors), tuple(offsets)
        self._taps = [np.ascontiguousarray(f, dtype=np.float64) for f in facs]
        self._centre = list(centre)
        # the pass order: sampled axes by falling factor, then the others
        self._down = sorted((a for a in range(dimension) if factors[a] > 1),
                            key=lambda a: (-factors[a], a))
        self._plain = [a for a in range(dimension) if factors[a] == 1 and
                       not (self._taps[a].size == 1 and self._taps[a][0] == 1.0)]

    def _check(self, shape):
        if len(shape) != self.dimension:
            raise RuntimeError("%dD operator applied to an array with %d axes" %
                               (self.dimension, len(shape)))

    def _out_shape(self, in_shape):
        self._check(in_shape)
        for s, o in zip(in_shape, self.offsets):
            if not int(s) > o:
                raise ValueError("offset %d is outside an axis of extent %d" % (o, s))
        return tuple(ops.sampled_extent(s, f, o)
                     for s, f, o in zip(in_shape, self.factors, self.offsets))

    def _apply(self, x, in_shape):
        self._out_shape(in_shape)
        d = self.dimension
        cur_shape = [int(s) for s in in_shape]
        cur = x
        for a in self._down:
            cur = ops.corr_axis_down(cur, cur_shape, a + 3 - d, self._taps[a],
                                     self._centre[a], self.mode, self.factors[a],
                                     self.offsets[a])
            cur_shape[a] = ops.sampled_extent(cur_shape[a], self.factors[a],
                                              self.offsets[a])
        for a in self._plain:
            cur = ops.corr_axis(cur, cur_shape, a + 3 - d, self._taps[a],
                                self._centre[a], self.mode)
        return cur.clone() if cur is x else cur

    def adjoint(self, fine_shape=None):
        """The exact transpose, a SampledConvolutionAdjointOperator.  fine_shape: the
        shape of the fine grid it maps to; None: factor * extent on every axis."""
        return SampledConvolutionAdjointOperator(self, fine_shape)


class SampledConvolutionAdjointOperator(DeviceOperator):
    """The exact transpose of a SampledConvolutionOperator: the sampled data spread
    back onto the fine grid and correlated with the transposed taps
    (ops.corr_axis_up), the forward operator's passes backwards.

    The coarse shape does not determine the fine one: an extent m belongs to every
    fine extent from o + (m - 1) f + 1 to o + m f.  The operator is therefore BUILT
    WITH the fine shape (fine_shape=); without one it maps to f * m on every axis,
    the grid of an observation upsampled by whole factors."""
    kind = "sampled_conv_adj"

    def __init__(self, forward, fine_shape=None):
        if not isinstance(forward, SampledConvolutionOperator):
            raise ValueError("the adjoint is built from a SampledConvolutionOperator")
        self.forward = forward
        self.dimension = forward.dimension
        if fine_shape is not None:
            fine_shape = tuple(int(s) for s in fine_shape)
            forward._out_shape(fine_shape)
        self.fine_shape = fine_shape

    def _out_shape(self, in_shape):
        fw = self.forward
        fw._check(in_shape)
        in_shape = tuple(int(s) for s in in_shape)
        fine = self.fine_shape
        if fine is None:
            fine = tuple(s * f for s, f in zip(in_shape, fw.factors))
        if fw._out_shape(fine) != in_shape:
            raise ValueError("a sampled array of shape %r does not belong to the fine "
                             "grid %r (pass fine_shape=)" % (in_shape, fine))
        return fine

    def _apply(self, q, in_shape):
        fw, d = self.forward, self.dimension
        fine = self._out_shape(in_shape)
        cur_shape = [int(s) for s in in_shape]
        cur = q
        for a in reversed(fw._plain):
            taps = fw._taps[a]
            cur = ops.corr_axis(cur, cur_shape, a + 3 - d, taps[::-1],
                                taps.size - 1 - fw._centre[a], fw.mode)
        for a in reversed(fw._down):
            cur_shape[a] = fine[a]
            cur = ops.corr_axis_up(cur, cur_shape, a + 3 - d, fw._taps[a],
                                   fw._centre[a], fw.mode, fw.factors[a],
                                   fw.offsets[a])
        return cur.clone() if cur is q else cur


def sampled_start(A_adj, b, fine_shape):
    """The usual start on the fine grid for a sampled observation b: A^T b / A^T 1,
    with 0 where A^T 1 == 0 (fine voxels no sample sees).  A_adj: the adjoint operator
    (or a callable on arrays of the coarse shape); b: the coarse data, NumPy array or
    device tensor; returns an array of fine_shape of b's kind."""
    fine_shape = tuple(int(s) for s in fine_shape)
    if isinstance(A_adj, SampledConvolutionAdjointOperator):
        coarse = A_adj.forward._out_shape(fine_shape)
        if A_adj._out_shape(coarse) != fine_shape:
            raise ValueError("the adjoint maps to %r, not to fine_shape %r" %
                             (A_adj._out_shape(coarse), fine_shape))
        b = b.reshape(coarse)
    if is_device_tensor(b):
        import torch
        num, den = A_adj(b), A_adj(torch.ones_like(b))
        safe = torch.where(den != 0, den, torch.ones_like(den))
        return torch.where(den != 0, num / safe, torch.zeros_like(num)).reshape(
            fine_shape)
    b = np.asarray(b)
    num, den = np.asarray(A_adj(b)), np.asarray(A_adj(np.ones_like(b)))
    out = np.zeros_like(num)
    np.divide(num, den, out=out, where=den != 0)
    return out.reshape(fine_shape)


class LinearOperators(object):

    def __init__(self, dimension, spacing):
        self._dimension = dimension
        self._spacing = spacing
        self._kernels = {1: Kernels.Kernels1D, 2: Kernels.Kernels2D,
                         3: Kernels.Kernels3D}[dimension](spacing=spacing)

    def get_spacing(self):
        return self._spacing

    def get_dimension(self):
        return self._dimension

    def get_convolution_and_adjoint_convolution_operators(
            self, kernel, mode="wrap", exact_adjoint=False):
        # the reference uses the SAME kernel for the adjoint
        # (linear_operators.py:63); exact for point-symmetric taps.
        # exact_adjoint=True: (A, A.transpose()), exact for every kernel ("wrap" and
        # "constant"; the other modes raise ValueError)
        A = ConvolutionOperator(self._dimension, kernel, mode)
        if exact_adjoint:
            return A, A.transpose()
        return A, A

    def get_gaussian_blurring_operators(self, cov, alpha_cut=3):
        kernel = self._kernels.get_gaussian(cov=cov, alpha_cut=alpha_cut)
        return self.get_convolution_and_adjoint_convolution_operators(kernel)

    def get_sampled_convolution_operators(self, kernel, factors, offsets=None,
                                          mode="wrap", fine_shape=None):
        """(A, A_adj) of the acquisition model "blur, then keep every f-th sample":
        SampledConvolutionOperator and its exact transpose.  factors / offsets: one
        integer per ARRAY axis (not spacing's reversed order); fine_shape: the fine
        grid the adjoint maps to (None: factor * extent on every axis)."""
        A = SampledConvolutionOperator(self._dimension, kernel, factors, offsets, mode)
        return A, A.adjoint(fine_shape)

    def get_sampled_gaussian_blurring_operators(self, cov, factors, offsets=None,
                                                alpha_cut=3, fine_shape=None):
        """The same with the Gaussian of get_gaussian_blurring_operators, whose
        spacing is the FINE grid's (periodic boundary)."""
        kernel = self._kernels.get_gaussian(cov=cov, alpha_cut=alpha_cut)
        return self.get_sampled_convolution_operators(kernel, factors, offsets,
                                                      fine_shape=fine_shape)

    def _axis_operators(self, direction, mode):
        if direction >= self._dimension:
            raise AttributeError("no such direction in %dD" % self._dimension)
        if mode == "constant":
            sp = self._kernels.get_spacing()
            return (AxisDifferenceOperator(self._dimension, sp, direction, 0),
                    AxisDifferenceOperator(self._dimension, sp, direction, 1))
        fwd = self._kernels._difference(direction, False)
        bwd = -self._kernels._difference(direction, True)
        return (ConvolutionOperator(self._dimension, fwd, mode),
                ConvolutionOperator(self._dimension, bwd, mode))

    def get_dx_operators(self, mode="constant"):
        return self._axis_operators(0, mode)

    def get_gradient_operators(self, mode="constant"):
        sp = self._kernels.get_spacing()
        if mode == "constant":
            return (GradientOperator(self._dimension, sp),
                    GradientAdjointOperator(self._dimension, sp))
        pairs = [self._axis_operators(a, mode)
                 for a in range(self._dimension)]
        return (_StackedOperator([p[0] for p in pairs]),
                _StackedAdjointOperator([p[1] for p in pairs]))


class _StackedOperator(DeviceOperator):
    """grad for non-default boundary modes: concatenation of per-axis passes."""
    kind = "stack"

    def __init__(self, parts):
        self.parts = parts

    def _out_shape(self, in_shape):
        return _stacked_shape(in_shape, len(self.parts))

    def _apply(self, x, in_shape):
        import torch
        return torch.cat([p._apply(x, in_shape) for p in self.parts])


class _StackedAdjointOperator(DeviceOperator):
    kind = "stack_adj"

    def __init__(self, parts):
        self.parts = parts

    def _out_shape(self, in_shape):
        return _unstacked_shape(in_shape, len(self.parts))

    def _apply(self, p, in_shape):
        d = len(self.parts)
        shp = _unstacked_shape(in_shape, d)
        m = p.numel() // d
        acc = self.parts[0]._apply(p[:m], shp)
        for a in range(1, d):
            acc = ops.lincomb2(1.0, acc, 1.0,
                               self.parts[a]._apply(p[a * m:(a + 1) * m], shp),
                               out=acc)
        return acc


class LinearOperators1D(LinearOperators):

    def __init__(self, spacing=1):
        LinearOperators.__init__(self, dimension=1, spacing=spacing)


class LinearOperators2D(LinearOperators):

    def __init__(self, spacing=np.ones(2)):
        LinearOperators.__init__(self, dimension=2, spacing=spacing)

    def get_dy_operators(self, mode="constant"):
        return self._axis_operators(1, mode)


class LinearOperators3D(LinearOperators2D):

    def __init__(self, spacing=np.ones(3)):
        LinearOperators.__init__(self, dimension=3, spacing=spacing)

    def get_dz_operators(self, mode="constant"):
        return self._axis_operators(2, mode)
