"""Second-order total generalised variation (TGV^2, Bredies / Kunisch / Pock) denoising
on MI355X:

    min over x and w   lambda D(x, b~) + |grad x - w|_1 + beta |E w|_1,   lambda = 1/alpha,

in the scaled variable x / x_scale (b~ = b / x_scale).  x holds n values, w one vector
of `dimension` values per voxel; grad is the zero-padded forward difference of
GradientOperator -- the one boundary convention of this package -- and E w the
symmetrised gradient of w, (E w)_aa = D_a w_a, (E w)_ab = (D_a w_b + D_b w_a) / 2, its
off-diagonals counted twice in every norm.  D is 1/2 |.|^2 (data_loss="ell2"), |.|_1
("ell1") or the Poisson (Kullback-Leibler) term sum (x - b~ log x) ("kl": counts b >= 0,
the prox of csrc/nsol_kl.hpp through ops.tgv_primal_kl, weighted or not); the norms are sums over the components, or with isotropic=True the per-voxel
Euclidean / Frobenius norms.  Where TV turns a smooth ramp into terraces, TGV keeps it:
w follows the gradient of x and only ITS variation is penalised (beta).

It cannot be written through PrimalDualSolver's callables, which know one primal
variable.  One iteration (constant steps, theta = 1; the problem is not strongly convex
in (x, w), so there is no accelerated schedule) is two launches (csrc/nsol_tgv.hip):

    p_a  <- P_1   (p_a  + sigma (D_a xbar - wbar_a))           ops.tgv_dual
    q_ab <- P_beta(q_ab + sigma (E wbar)_ab)
    x+   = prox_{tau lambda D}(x - tau sum_a D_a^T p_a)         ops.tgv_primal
    w_a+ = w_a - tau (-p_a + D_a^T q_aa + sum_{b != a} D_b^T q_ab)
    xbar = x+ + theta (x+ - x),   wbar = w+ + theta (w+ - w)

from x = xbar = x0 / x_scale, w = wbar = p = q = 0.  The steps default to tau = sigma =
1 / sqrt(L2) with L2 = (2 g + 1 + sqrt(4 g + 1)) / 2, g = 4 sum_a 1 / h_a^2, an upper
bound of |K|^2 (16 for unit spacing in 3-D).  The arithmetic is restated in NumPy in
nsol_amd/tgv_numpy.py.

Stopping rule: PrimalDualSolver's, with the primal ratio over the stacked (x, w) and the
dual ratio over (p, q); one read-back per check, none without a tolerance.  A device-mode
observer (keep_iterates=False) observes x where its points fall, as in the other solvers.
"""
import numpy as np

from . import ops, tgv_numpy
from .device import is_device_tensor, to_numpy
from .primal_dual_linear_solver import (DATA_LOSSES, _DataSide, _LinearDataTermSolver,
                                        _LinearStopRule, check_counts, step_sizes)
from .proximal_operators import (check_weights, scaled_data_on_device,
                                 weights_on_device)
from .solver import Solver
from .stopping import Stopping
from ._accessors import add_accessors


def _positive(v):
    return bool(np.isfinite(v) and v > 0)


class TGVPrimalDualSolver(Stopping, Solver):

    def __init__(self, b, x0, dimension, spacing=None, alpha=0.01, beta=2.0,
                 iterations=10, data_loss="ell2", isotropic=False, L2=None, tau=None,
                 sigma=None, x_scale=1., verbose=0, dtype=None, tolerance=None,
                 check_every=10, shape=None, weights=None):
        Solver.__init__(self, x0=x0, verbose=verbose, x_scale=x_scale, dtype=dtype)
        if data_loss not in DATA_LOSSES:
            raise ValueError("data_loss must be one of %r" % (DATA_LOSSES,))
        try:
            ok = int(dimension) == dimension and int(dimension) in (1, 2, 3)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("dimension must be 1, 2 or 3")
        dimension = int(dimension)
        self._b = b
        self._dimension = dimension
        self._spacing = np.ones(dimension) if spacing is None else \
            np.atleast_1d(spacing).astype(float)
        if self._spacing.size != dimension or \
                not all(_positive(s) for s in self._spacing):
            raise ValueError("spacing must hold %d positive, finite values" % dimension)
        self._alpha, self._beta = float(alpha), float(beta)
        if not _positive(self._alpha):
            raise ValueError("alpha must be positive and finite")
        if not _positive(self._beta):
            raise ValueError("beta must be positive and finite")
        self._iterations = iterations
        self._data_loss = data_loss
        self._isotropic = bool(isotropic)
        self.set_tolerance(tolerance)
        self.set_check_every(check_every)

        n = int(x0.numel() if is_device_tensor(x0) else np.size(x0))
        m = int(b.numel() if is_device_tensor(b) else np.size(b))
        if shape is None:
            if dimension == 1:
                shape = (m,)
            elif len(getattr(b, "shape", ())) == dimension:
                shape = tuple(b.shape)
            else:
                raise ValueError("the volume's shape is not known: pass shape=, or b "
                                 "with %d axes" % dimension)
        try:
            shape = tuple(int(s) for s in shape)
        except TypeError:
            raise ValueError("shape must be a sequence of %d extents" % dimension)
        if len(shape) != dimension or min(shape) < 1 or int(np.prod(shape)) != m:
            raise ValueError("shape %r does not hold the %d values of b in %d-D" %
                             (shape, m, dimension))
        if n != m:
            raise ValueError("x0 holds %d values, b %d" % (n, m))
        self._shape, self._n = shape, n
        # per-voxel weights >= 0 of the data term (a mask, a confidence map); None: all
        # 1, the unweighted kernel
        self._weights = weights
        if weights is not None:
            check_weights(weights, n)
        if data_loss == "kl":
            check_counts(b, weights)

        if L2 is None:
            L2 = tgv_numpy.norm_bound(dimension, self._spacing)
        self._L2 = float(L2)
        self._tau, self._sigma = step_sizes(self._L2, tau, sigma)
        self._theta = 1.
        self._w = None

    # ------------------------------------------------------------------
    def get_execution(self):
        """'fused': the two kernels of nsol_tgv.hip, whatever the arguments."""
        return "fused"

    def get_w(self):
        """The second primal variable times x_scale, dimension * n values (component 0
        along the last array axis first); zeros before run()."""
        if self._w is None:
            return np.zeros(self._dimension * self._n, dtype=np.float64)
        return to_numpy(ops.scale(self._w, self._x_scale))

    def print_statistics(self, fmt="%.3e"):
        print("TGV (%s, %s): alpha = %g, beta = %g, tau = %g, sigma = %g, L2 = %g" % (
            self._data_loss, "isotropic" if self._isotropic else "anisotropic",
            self._alpha, self._beta, self._tau, self._sigma, self._L2))
        if self._iterations_done is not None:
            print("  %d iterations (%s)" % (self._iterations_done, self._stop_reason))
        changes = self.get_changes()
        if len(changes):
            print(("  last change: primal " + fmt + ", dual " + fmt) %
                  (changes[-1, 1], changes[-1, 2]))

    # ------------------------------------------------------------------
    def _run(self):
        import torch
        iters = max(int(self._iterations), 0)
        self._observe_start(iters)
        rule = self._start_rule(iters)

        d, n = self._dimension, self._n
        M = tgv_numpy.components(d)
        x0 = self._x0_device()
        # x and w in one buffer [x; w], p and q in one [p; q]: the stopping rule's sums
        # run once over each
        primal = torch.zeros((1 + d) * n, dtype=x0.dtype, device=x0.device)
        dual = torch.zeros((d + M) * n, dtype=x0.dtype, device=x0.device)
        x, w = primal[:n], primal[n:]
        p, q = dual[:d * n], dual[d * n:]
        x.copy_(x0)
        xbar = x.clone()
        wbar = torch.zeros(d * n, dtype=x0.dtype, device=x0.device)
        bt = scaled_data_on_device(self._b, self._x_scale, x)
        if bt.numel() != n:
            raise ValueError("b holds %d values, not %d" % (bt.numel(), n))
        wt = None if self._weights is None else weights_on_device(self._weights, x)
        kl = self._data_loss == "kl"
        if rule is not None:
            rule.allocate(x)

        shape, iw = self._shape, ops.inv_spacing(self._spacing, d)
        tau, sigma, theta = self._tau, self._sigma, self._theta
        tl = tau / self._alpha
        dflags = ops.PD_REG_ISOTROPIC if self._isotropic else 0
        pflags = ops.PD_DATA_L1 if self._data_loss == "ell1" else 0

        self._x, self._w = x, w
        for i in range(iters):
            if self._verbose:
                print("TGV primal-dual iteration %d/%d" % (i + 1, iters))
            check = rule is not None and rule.is_point(i + 1)
            if check:
                primal_old, dual_old = primal.clone(), dual.clone()
            if not (ops.tgv_dual(xbar, wbar, p, q, shape, iw, sigma, self._beta, dflags)
                    and (ops.tgv_primal_kl(p, q, x, xbar, w, wbar, bt, wt, shape, iw, tau,
                                           tl, theta) if kl else
                         ops.tgv_primal(p, q, x, xbar, w, wbar, bt, shape, iw, tau, tl,
                                        theta, pflags) if wt is None else
                         ops.tgv_primal_w(p, q, x, xbar, w, wbar, bt, wt, shape, iw, tau,
                                          tl, theta, pflags))):
                raise ValueError("nsol_tgv does not take a volume of shape %r" %
                                 (tuple(shape),))
            if check:
                ops.pd_change(primal_old, primal, dual_old, dual, rule.ws,
                              rule.row(i + 1))
            self._observe_iteration(i + 1, x)
            if self._stops_after(i + 1):
                break
        if rule is None:
            self._iterations_done = iters


add_accessors(TGVPrimalDualSolver, ["alpha", "beta", "iterations", "data_loss"])
add_accessors(TGVPrimalDualSolver,
              ["b", "dimension", "spacing", "isotropic", "L2", "tau", "sigma", "theta",
               "shape", "weights"],
              setters=False)


class TGVPrimalDualLinearSolver(_LinearDataTermSolver):
    """TGV^2 as the regulariser of PrimalDualLinearSolver -- deconvolution and
    super-resolution that keep ramps, with weights, masks and an exact box:

        min over x (n values, the fine grid) and w (dimension * n)
            lambda D_wt(A x, b~) + |grad x - w|_1 + beta |E w|_1 + indicator_[lo, hi](x)

    in the scaled units, with TGVPrimalDualSolver's grad, E and norms and
    PrimalDualLinearSolver's D_wt (per-sample weights wt >= 0 on A's range, m values), box
    and treatment of A: this package's operators are recognised through the caller's
    lambdas (get_execution() 'fused', with the blur's axpby epilogue where m == n on a
    ConvolutionOperator, and SampledConvolutionOperator pairs with b, r and the weights on
    the coarse grid), other callables run as 'device' or 'host'.  The saddle-point map
    K(x, w) = (grad x - w, E w, A x) has a third dual variable r (m values) for the data
    term; one iteration (constant steps, theta = 1) is

        (p, q) <- ops.tgv_dual(xbar, wbar, p, q)
        r      <- ops.pdl_dual_data(r, A xbar, b~, wt, sigma, lambda)   (or the epilogue;
                   data_loss="kl": ops.pdl_dual_data_kl, with background=)
        g       = A^T r
        x+      = clip(x - tau (sum_a D_a^T p_a + g), lo, hi)           ops.tgv_primal_lin
        w+, xbar, wbar as in TGVPrimalDualSolver

    from x = xbar = x0 / x_scale, w = wbar = p = q = r = 0.  tau = sigma = 1 / sqrt(L2)
    with L2 = tgv_numpy.norm_bound_linear(dimension, spacing, A_norm2); A_norm2 defaults
    to Young's bound for this package's blurs and is required for any other callable.
    Restated in tgv_numpy.iterate_linear.

    Stopping rule: PrimalDualSolver's, the primal ratio over (x, w), the dual one over
    (p, q, r); one read-back per check, none without a tolerance."""

    def __init__(self, A, A_adj, b, x0, dimension, spacing=None, alpha=0.01, beta=2.0,
                 iterations=10, data_loss="ell2", isotropic=False, weights=None,
                 bounds=None, A_norm2=None, L2=None, tau=None, sigma=None, x_scale=1.,
                 verbose=0, dtype=None, tolerance=None, check_every=10, shape=None,
                 background=0.):
        try:
            ok = int(dimension) == dimension and int(dimension) in (1, 2, 3)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("dimension must be 1, 2 or 3")
        self._beta = float(beta)
        if not _positive(self._beta):
            raise ValueError("beta must be positive and finite")
        if not _positive(float(alpha)):
            raise ValueError("alpha must be positive and finite")
        _LinearDataTermSolver.__init__(
            self, A, A_adj, b, x0, dimension, spacing=spacing, alpha=alpha,
            iterations=iterations, isotropic=isotropic, data_loss=data_loss,
            weights=weights, bounds=bounds, A_norm2=A_norm2, L2=L2, tau=tau, sigma=sigma,
            x_scale=x_scale, verbose=verbose, dtype=dtype, tolerance=tolerance,
            check_every=check_every, shape=shape, background=background)
        if not all(_positive(s) for s in self._spacing):
            raise ValueError("spacing must hold %d positive, finite values" %
                             self._dimension)
        self._w = None

    def _default_L2(self):
        return float(tgv_numpy.norm_bound_linear(self._dimension, self._spacing,
                                                 self._A_norm2))

    def get_w(self):
        """The second primal variable times x_scale, dimension * n values (component 0
        along the last array axis first); zeros before run()."""
        if self._w is None:
            return np.zeros(self._dimension * self._n, dtype=np.float64)
        return to_numpy(ops.scale(self._w, self._x_scale))

    def print_statistics(self, fmt="%.3e"):
        print("TGV (linear; %s, %s): alpha = %g, beta = %g, tau = %g, sigma = %g, "
              "L2 = %g, execution %s" % (
                  self._data_loss, "isotropic" if self._isotropic else "anisotropic",
                  self._alpha, self._beta, self._tau, self._sigma, self._L2,
                  self._execution))
        if self._iterations_done is not None:
            print("  %d iterations (%s)" % (self._iterations_done, self._stop_reason))

    def _run(self):
        import torch
        iters = max(int(self._iterations), 0)
        self._observe_start(iters)
        rule = self._start_rule(iters, _LinearStopRule)

        d, n, m = self._dimension, self._n, self._m
        M = tgv_numpy.components(d)
        x0 = self._x0_device()
        # [x; w] and [p; q] are one buffer each, as in TGVPrimalDualSolver; r is the
        # data term's dual, on A's range
        primal = torch.zeros((1 + d) * n, dtype=x0.dtype, device=x0.device)
        dual = torch.zeros((d + M) * n, dtype=x0.dtype, device=x0.device)
        x, w = primal[:n], primal[n:]
        p, q = dual[:d * n], dual[d * n:]
        x.copy_(x0)
        xbar = x.clone()
        wbar = torch.zeros(d * n, dtype=x0.dtype, device=x0.device)
        r = torch.zeros(m, dtype=x0.dtype, device=x0.device)
        bt, wt = self._device_data(x)
        if rule is not None:
            rule.allocate(x)
        data = _DataSide(self, x)

        shape, iw = self._shape, ops.inv_spacing(self._spacing, d)
        tau, sigma, theta = self._tau, self._sigma, self._theta
        lmbda = 1. / self._alpha
        data_loss, bg = self._data_loss, self._scaled_background()
        lo, hi = self._bounds
        dflags = ops.PD_REG_ISOTROPIC if self._isotropic else 0

        self._x, self._w = x, w
        for i in range(iters):
            if self._verbose:
                print("TGV primal-dual (linear) iteration %d/%d" % (i + 1, iters))
            check = rule is not None and rule.is_point(i + 1)
            if check:
                primal_old, dual_old, r_old = primal.clone(), dual.clone(), r.clone()
            ok = ops.tgv_dual(xbar, wbar, p, q, shape, iw, sigma, self._beta, dflags)
            if ok:
                g = data.dual_step(xbar, r, bt, wt, sigma, lmbda, data_loss, bg)
                ok = ops.tgv_primal_lin(p, q, x, xbar, w, wbar, g, shape, iw, tau, theta,
                                        lo, hi)
            if not ok:
                raise ValueError("nsol_tgv does not take a volume of shape %r" %
                                 (tuple(shape),))
            if check:
                row = rule.row(i + 1)
                ops.pd_change(primal_old, primal, dual_old, dual, rule.ws,
                              row[:ops.PD_CHECK_SUMS])
                ops.pd_change(r_old, r, r_old, r, rule.ws, row[ops.PD_CHECK_SUMS:])
            self._observe_iteration(i + 1, x)
            if self._stops_after(i + 1):
                break
        if rule is None:
            self._iterations_done = iters
        data.finish()


add_accessors(TGVPrimalDualLinearSolver, ["beta"])
