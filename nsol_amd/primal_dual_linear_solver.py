"""Chambolle-Pock primal-dual solver for a data term behind a linear operator A on
MI355X -- deconvolution without inner solves:

    min_x  lambda D_w(A x, b~) + R(grad x) + indicator_[lo, hi](x),   lambda = 1/alpha,

in the scaled variable x / x_scale (b~ = b / x_scale; the box is the scaled
variable's, as TikhonovLinearSolver's bounds are), with
  D_w   1/2 sum w_i (.)^2 (data_loss="ell2"), sum w_i |.| ("ell1") or the Poisson
        (Kullback-Leibler) term sum w_i ((u_i + g) - b~_i log(u_i + g)) of u = A x
        ("kl": photon counts b >= 0; g = background / x_scale >= 0 a known constant such
        as a dark current, which keeps the log finite where A x reaches 0), per-voxel
        weights w_i >= 0 (a mask, a confidence map; None: all 1),
  R     TV or Huber(gamma), anisotropic or isotropic,
  grad  the zero-padded forward difference of GradientOperator.

PrimalDualSolver deconvolves through prox_linear_least_squares: every iteration is a
whole Tikhonov / LSMR solve.  Here A is part of the saddle-point problem's linear map
K = (grad, A), with a dual variable p for the regulariser and q for the data term, and
one iteration (constant steps, theta = 1: Chambolle-Pock's basic algorithm -- G is an
indicator, so the accelerated schedules do not apply) is

    p <- prox_{sigma R*}(p + sigma grad xbar)
    v  = q + sigma (A xbar - b~)
    q <- l2: v c / (c + sigma), c = lambda w;   l1: clamp(v, -c, c);   w = 0: 0
         kl: v = q + sigma (A xbar + g), d = v - c, s = sqrt(d^2 + 4 sigma c b~),
             q <- d > 0 ? c - 2 sigma c b~ / (d + s) : c + (d - s) / 2   (csrc/nsol_kl.hpp)
    x+ = clip(x - tau (grad^T p + A^T q), lo, hi);  xbar <- x+ + theta (x+ - x);  x <- x+

one application of A, one of A^T, one element-wise kernel (ops.pdl_dual_data) and one
pass of the fused primal-dual tile (ops.pdl_iter, nsol_pdl.hip).  Weights, masks, the
l1 data term and the box cost nothing extra; the KL term costs one square root and one
division per value.  Like TV, the KL term is 1-homogeneous, so the minimiser of TV-KL does
not depend on x_scale in exact arithmetic (a finite run does: the steps act on the scaled
variable).  A list of such solvers on volumes of one
shape, or one observation under several alphas, runs in stacked launches through
PrimalDualLinearBatch / PrimalDualLinearSweep (nsol_amd/linear_stack.py, nsol_pdls.hip).

`run()` picks one of three execution forms for A and A^T; the regulariser side is
nsol_pdl_iter_* in all of them:
  fused   A, A_adj are device operators of this package, recognised THROUGH
          caller-side lambdas (symbolic.trace_operator).  Where A is a
          ConvolutionOperator whose one-pass blur has the axpby epilogue, A xbar is
          never stored: q <- sigma A xbar + q is the blur's epilogue.  A
          SampledConvolutionOperator with its adjoint (super-resolution: b, q and the
          weights live on the m sampled values, x on the n of the fine grid, which
          `shape` defaults to) runs here too, without that epilogue;
  device  callables on torch HIP tensors;
  host    NumPy-only callables: their argument is copied to the host for the call only.

Stopping rule: PrimalDualSolver's, with the dual ratio taken over the stacked dual
(p, q): r_dual = sqrt((sum dp^2 + sum dq^2) / (sum p^2 + sum q^2)); one read-back per
check, none without a tolerance.
"""
import numpy as np

from . import linear_operators, ops
from .bridge import BridgedCallable
from .device import is_device_tensor
from .linear_operators import (ConvolutionOperator, DeviceOperator,
                               SampledConvolutionOperator)
from .proximal_operators import (check_weights, scaled_data_on_device,
                                 weights_on_device)
from .solver import Solver
from .stopping import Stopping, _StopRule, criterion_met, relative_changes
from .symbolic import trace_operator
from ._accessors import add_accessors

REG_TYPES = ("TV", "huber")
DATA_LOSSES = ("ell2", "ell1", "kl")


def step_sizes(L2, tau=None, sigma=None):
    """(tau, sigma): 1/sqrt(L2) each by default; with one given, the other is
    1 / (L2 * it).  ValueError unless both are positive and tau sigma L2 <= 1."""
    L2 = float(L2)
    if not (np.isfinite(L2) and L2 > 0):
        raise ValueError("L2 must be a positive number")
    if tau is None and sigma is None:
        tau = sigma = 1. / np.sqrt(L2)
    elif tau is None:
        sigma = float(sigma)
        tau = 1. / (L2 * sigma) if sigma > 0 else sigma
    elif sigma is None:
        tau = float(tau)
        sigma = 1. / (L2 * tau) if tau > 0 else tau
    tau, sigma = float(tau), float(sigma)
    if not (np.isfinite(tau) and np.isfinite(sigma) and tau > 0 and sigma > 0):
        raise ValueError("tau and sigma must be positive numbers")
    if tau * sigma * L2 > 1. + 1e-12:
        raise ValueError("tau * sigma * L2 = %g > 1: the iteration need not converge" %
                         (tau * sigma * L2))
    return tau, sigma


def checked_background(background, data_loss):
    """`background` as a float: finite, >= 0, and 0 unless data_loss is "kl"."""
    try:
        background = float(background)
    except (TypeError, ValueError):
        raise ValueError("background must be a number")
    if not (np.isfinite(background) and background >= 0):
        raise ValueError("background must be a finite number >= 0")
    if background != 0 and data_loss != "kl":
        raise ValueError("background belongs to data_loss=\"kl\", not to %r" %
                         (data_loss,))
    return background


def check_counts(b, weights):
    """ValueError unless the observation `b` is >= 0 wherever its weight is positive
    (weights None: everywhere), NaN counting as negative: what the Poisson (KL) data term
    needs.  One reduction when a solver is set up, on the host for NumPy arrays and on the
    device (one read-back) for device tensors; what sits under weight 0 is not looked at."""
    if is_device_tensor(b) or is_device_tensor(weights):
        import torch
        if not is_device_tensor(b):
            b = torch.as_tensor(np.asarray(b), device=weights.device)
        bad = ~(b.reshape(-1) >= 0)
        if weights is not None:
            if not is_device_tensor(weights):
                weights = torch.as_tensor(np.asarray(weights), device=b.device)
            bad = bad & (weights.reshape(-1) > 0)
        found = bool(torch.any(bad))
    else:
        with np.errstate(invalid="ignore"):
            bad = ~(np.asarray(b).reshape(-1) >= 0)
            if weights is not None:
                bad = bad & (np.asarray(weights).reshape(-1) > 0)
        found = bool(np.any(bad))
    if found:
        raise ValueError("data_loss=\"kl\" needs observations >= 0 wherever the weight is "
                         "positive (negative or NaN values found)")


def checked_bounds(bounds):
    """(lo, hi) as floats with lo <= hi, infinities allowed; None: (-inf, inf)."""
    if bounds is None:
        return -np.inf, np.inf
    try:
        lo, hi = bounds
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError("bounds must be None or a pair (lo, hi)")
    if not lo <= hi:
        raise ValueError("bounds must satisfy lo <= hi")
    return lo, hi


class _LinearStopRule(_StopRule):
    """_StopRule with two rows of sums per check: nsol_pd_change_* over (x, p) and
    over q; the dual ratio is taken over the stacked dual (p, q)."""

    def allocate(self, like, shape=None):
        import torch
        self.ws = torch.empty(ops.PD_CHECK_SUMS * 4096, dtype=torch.float64,
                              device=like.device)
        self.board = torch.empty((max(len(self.points), 1), 2 * ops.PD_CHECK_SUMS),
                                 dtype=torch.float64, device=like.device)

    def decide(self, it):
        s = self.row(it).cpu().numpy()         # the one read-back of this check
        r_x, r_d = relative_changes((s[0], s[1], s[2] + s[4], s[3] + s[5]))
        self.rows.append((float(it), r_x, r_d))
        return criterion_met(r_x, r_d, self.tolerance)


class _DataSide:
    """The data term's side of one run of a _LinearDataTermSolver: A and A^T in the run's execution form, and
    the dual step q <- prox(q + sigma (A xbar - b~)) followed by g = A^T q."""

    def __init__(self, solver, x):
        import torch
        s = self._solver = solver
        self._fused = s._op is not None
        if self._fused:
            self._A = lambda t: s._op._apply(t, s._op_shape)
            self._At = lambda t: s._op_adj._apply(t, s._op_adj_shape)
        else:
            self._A = BridgedCallable(s._A, s._dtype)
            self._At = BridgedCallable(s._A_adj, s._dtype)
        # q <- sigma A xbar + q as the epilogue of the one-pass blur, while it applies
        self._epilogue = self._fused and isinstance(s._op, ConvolutionOperator) and \
            s._m == s._n and linear_operators.USE_BLUR_EPILOGUE
        self._slot = torch.empty(1, dtype=torch.float64, device=x.device) \
            if self._epilogue else None

    def dual_step(self, xbar, q, bt, wt, sigma, lmbda, data_loss, background=0.):
        """q in place; returns g = A^T q (n values).  background: the scaled one."""
        s = self._solver
        if data_loss == "kl":
            def update(t):
                ops.pdl_dual_data_kl(q, t, bt, wt, sigma, lmbda, background)
        else:
            l1 = data_loss == "ell1"

            def update(t):
                ops.pdl_dual_data(q, t, bt, wt, sigma, lmbda, l1)
        if self._epilogue and s._op.apply_axpby(xbar, q, s._op_shape, sigma, 1.,
                                                result=self._slot) is None:
            self._epilogue = False     # the kernel declined: nothing ran, q is intact
        if self._epilogue:
            update(None)
        else:
            t = self._A(xbar)
            if t.numel() != s._m:
                raise ValueError("A returned %d values, b holds %d" %
                                 (t.numel(), s._m))
            update(t)
        g = self._At(q)
        if g.numel() != s._n:
            raise ValueError("A_adj returned %d values, x holds %d" % (g.numel(), s._n))
        return g

    def finish(self):
        """Records 'device' or 'host' for callables that are not this package's."""
        if not self._fused:
            A, At = self._A, self._At
            self._solver._execution = "device" if (
                A.on_device in (True, None) and At.on_device in (True, None)) else "host"


class _LinearDataTermSolver(Stopping, Solver):
    """What the solvers with a data term behind a linear operator A share, whatever
    their regulariser (PrimalDualLinearSolver below, tgv_solver.TGVPrimalDualLinearSolver):
    the checked arguments, the operators behind the caller's lambdas, the volume's shape,
    weights, the box, A_norm2 and the step sizes.  A subclass supplies _default_L2 (its
    bound of |K|^2) and _run, which takes the data side of an iteration from _DataSide."""

    def __init__(self, A, A_adj, b, x0, dimension, spacing=None, alpha=0.01,
                 iterations=10, isotropic=False, data_loss="ell2", weights=None,
                 bounds=None, A_norm2=None, L2=None, tau=None, sigma=None, x_scale=1.,
                 verbose=0, dtype=None, tolerance=None, check_every=10, shape=None,
                 background=0.):
        Solver.__init__(self, x0=x0, verbose=verbose, x_scale=x_scale, dtype=dtype)
        if data_loss not in DATA_LOSSES:
            raise ValueError("data_loss must be one of %r" % (DATA_LOSSES,))
        self._background = checked_background(background, data_loss)
        dimension = int(dimension)
        if dimension not in (1, 2, 3):
            raise ValueError("dimension must be 1, 2 or 3")
        self._A, self._A_adj, self._b = A, A_adj, b
        self._dimension = dimension
        self._spacing = np.ones(dimension) if spacing is None else \
            np.atleast_1d(spacing).astype(float)
        if self._spacing.size != dimension or not np.all(self._spacing > 0):
            raise ValueError("spacing must hold %d positive values" % dimension)
        self._alpha = float(alpha)
        if not self._alpha > 0:
            raise ValueError("alpha must be positive")
        self._iterations = iterations
        self._isotropic = bool(isotropic)
        self._data_loss = data_loss
        self._bounds = checked_bounds(bounds)
        self.set_tolerance(tolerance)
        self.set_check_every(check_every)

        n = int(x0.numel() if is_device_tensor(x0) else np.size(x0))
        m = int(b.numel() if is_device_tensor(b) else np.size(b))
        self._n, self._m = n, m
        # the operators behind the caller's lambdas
        dA, dAt = trace_operator(A, n), trace_operator(A_adj, m)
        self._op = self._op_adj = None
        if self._is_own(dA, n, m, dimension) and self._is_own(dAt, m, n, dimension):
            self._op, self._op_shape = dA[1], tuple(dA[2])
            self._op_adj, self._op_adj_shape = dAt[1], tuple(dAt[2])
        self._shape = self._volume_shape(shape, b, n)
        self._weights = weights
        if weights is not None:
            check_weights(weights, m)
        if data_loss == "kl":
            check_counts(b, weights)

        if A_norm2 is None:
            if not isinstance(self._op, (ConvolutionOperator,
                                         SampledConvolutionOperator)):
                raise ValueError("A_norm2 (an upper bound of ||A||^2) is required "
                                 "unless A is a ConvolutionOperator or a "
                                 "SampledConvolutionOperator of this package")
            # Young's bound, exact for non-negative taps; sampling is a restriction
            # (norm <= 1), so the bound holds for the sampled blur as well
            A_norm2 = float(np.sum(np.abs(self._op.kernel))) ** 2
        self._A_norm2 = float(A_norm2)
        if not (np.isfinite(self._A_norm2) and self._A_norm2 >= 0):
            raise ValueError("A_norm2 must be a finite number >= 0")
        if L2 is None:
            L2 = self._default_L2()
        self._L2 = float(L2)
        self._tau, self._sigma = step_sizes(self._L2, tau, sigma)
        self._theta = 1.
        self._execution = "fused" if self._op is not None else None

    def _default_L2(self):
        raise NotImplementedError

    @staticmethod
    def _is_own(desc, n_in, n_out, dimension):
        """desc is (kind, operator, in_shape) of a device operator of this package that
        maps n_in elements on `dimension` axes to n_out."""
        if desc is None or len(desc) < 3 or not isinstance(desc[1], DeviceOperator):
            return False
        shape = tuple(desc[2])
        return len(shape) == dimension and int(np.prod(shape)) == n_in and \
            int(np.prod(desc[1]._out_shape(shape))) == n_out

    def _volume_shape(self, shape, b, n):
        """The volume the gradient acts on: `shape`, else the traced operator's, else
        b's own when it is an array of `dimension` axes (1-D: the flat vector)."""
        d = self._dimension
        if shape is None and self._op is not None and len(self._op_shape) == d:
            shape = self._op_shape
        if shape is None and d == 1:
            shape = (n,)
        if shape is None and len(getattr(b, "shape", ())) == d:
            shape = tuple(b.shape)
        if shape is None:
            raise ValueError("the volume's shape is not known: pass shape=, or an A "
                             "of this package, or b with %d axes" % d)
        shape = tuple(int(s) for s in shape)
        if len(shape) != d or int(np.prod(shape)) != n or min(shape) < 1:
            raise ValueError("shape %r does not hold the %d values of x0 in %d-D" %
                             (shape, n, d))
        return shape

    def _scaled_background(self):
        """g = background / x_scale, the constant the kernels add to A xbar."""
        return self._background / float(self._x_scale)

    def _device_data(self, x):
        """(bt, wt): the scaled observation and the weights (or None) on x's device, checked
        (m values)."""
        bt = scaled_data_on_device(self._b, self._x_scale, x)
        if bt.numel() != self._m:
            raise ValueError("b holds %d values, not %d" % (bt.numel(), self._m))
        wt = None if self._weights is None else weights_on_device(self._weights, x)
        return bt, wt

    # ------------------------------------------------------------------
    def get_execution(self):
        """'fused' (known from construction), 'device' or 'host' after run()."""
        return self._execution

    def print_statistics(self, fmt="%.3e"):
        pass


class PrimalDualLinearSolver(_LinearDataTermSolver):

    def __init__(self, A, A_adj, b, x0, dimension, spacing=None, alpha=0.01,
                 iterations=10, reg_type="TV", huber_gamma=0.05, isotropic=False,
                 data_loss="ell2", weights=None, bounds=None, A_norm2=None, L2=None,
                 tau=None, sigma=None, x_scale=1., verbose=0, dtype=None,
                 tolerance=None, check_every=10, shape=None, background=0.):
        if reg_type not in REG_TYPES:
            raise ValueError("reg_type must be one of %r" % (REG_TYPES,))
        self._reg_type, self._huber_gamma = reg_type, float(huber_gamma)
        _LinearDataTermSolver.__init__(
            self, A, A_adj, b, x0, dimension, spacing=spacing, alpha=alpha,
            iterations=iterations, isotropic=isotropic, data_loss=data_loss,
            weights=weights, bounds=bounds, A_norm2=A_norm2, L2=L2, tau=tau, sigma=sigma,
            x_scale=x_scale, verbose=verbose, dtype=dtype, tolerance=tolerance,
            check_every=check_every, shape=shape, background=background)

    def _default_L2(self):
        """|grad|^2 + |A|^2 bounds |(grad, A)|^2."""
        return float(np.sum(4. / self._spacing ** 2)) + self._A_norm2

    # ------------------------------------------------------------------
    def _flags(self):
        flags = ops.PD_REG_HUBER if self._reg_type == "huber" else ops.PD_REG_TV
        if self._isotropic:
            flags |= ops.PD_REG_ISOTROPIC
        return flags

    def _run(self):
        import torch
        iters = max(int(self._iterations), 0)
        self._observe_start(iters)
        rule = self._start_rule(iters, _LinearStopRule)

        x = self._x0_device().clone()
        n, m = self._n, self._m
        xbar = [x.clone(), torch.empty_like(x)]
        p = [torch.empty(self._dimension * n, dtype=x.dtype, device=x.device)
             for _ in range(2)]
        q = torch.zeros(m, dtype=x.dtype, device=x.device)
        bt, wt = self._device_data(x)
        if rule is not None:
            rule.allocate(x)

        data = _DataSide(self, x)

        shape, w = self._shape, ops.inv_spacing(self._spacing, self._dimension)
        flags = self._flags()
        tau, sigma, theta = self._tau, self._sigma, self._theta
        hden = 1. + sigma * self._huber_gamma if self._reg_type == "huber" else 1.
        lmbda = 1. / self._alpha
        data_loss, bg = self._data_loss, self._scaled_background()
        lo, hi = self._bounds

        for i in range(iters):
            if self._verbose:
                print("Primal-Dual (linear) iteration %d/%d" % (i + 1, iters))
            k = i & 1
            check = rule is not None and rule.is_point(i + 1)
            if check:
                x_old, q_old = x.clone(), q.clone()
            g = data.dual_step(xbar[k], q, bt, wt, sigma, lmbda, data_loss, bg)
            if not ops.pdl_iter(xbar[k], xbar[1 - k], x, g, p[k], p[1 - k], shape, w,
                                sigma, hden, tau, theta, lo, hi, flags, has_p=i > 0):
                raise ValueError("nsol_pdl_iter does not take a volume of shape %r" %
                                 (tuple(shape),))
            if check:
                row = rule.row(i + 1)
                # (p's old slot is still intact: the kernel wrote the other one)
                ops.pd_change(x_old, x, None if i == 0 else p[k], p[1 - k], rule.ws,
                              row[:ops.PD_CHECK_SUMS])
                ops.pd_change(q_old, q, q_old, q, rule.ws, row[ops.PD_CHECK_SUMS:])
            self._x = x
            self._observe_iteration(i + 1, x)
            if self._stops_after(i + 1):
                break
        self._x = x
        if rule is None:
            self._iterations_done = iters
        data.finish()


add_accessors(_LinearDataTermSolver, ["alpha", "iterations", "data_loss"])
add_accessors(PrimalDualLinearSolver, ["huber_gamma", "reg_type"])
add_accessors(_LinearDataTermSolver,
              ["A", "A_adj", "dimension", "spacing", "isotropic", "bounds", "A_norm2",
               "L2", "tau", "sigma", "theta", "shape", "background"],
              setters=False)
