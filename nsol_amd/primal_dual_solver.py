"""Chambolle-Pock primal-dual solver on MI355X (drop-in for
nsol/primal_dual_solver.py:26-403).

`run()` picks one of three execution forms:
  fused   B = grad, B_conj = grad_adj of nsol_amd.linear_operators, prox_g_conj
          in {prox_tv_conj, prox_huber_conj} or their isotropic forms
          {prox_tv_conj_isotropic, prox_huber_conj_isotropic} (one single-pass
          kernel per iteration, k_pd_fused_iso), prox_f in {prox_ell1_denoising,
          prox_ell2_denoising} or their per-voxel weighted forms
          {prox_ell1_denoising_weighted, prox_ell2_denoising_weighted} (masks,
          confidence maps: one single-pass kernel per iteration, k_pd_w, 48 bytes
          per voxel instead of 44) -- recognised THROUGH caller-side lambdas with
          a symbolic probe; nsol_pd_run_* enqueues the whole run: three
          iterations per pass over memory on large 3-D volumes (11 words of
          HBM traffic per voxel for all three; bit-identical to one
          iteration per launch), one single-pass kernel per iteration
          otherwise;
  device  any callables that work on torch HIP tensors (e.g.
          prox_linear_least_squares for deconvolution): the loop keeps all
          state in HBM and glues the callables with HIP axpy kernels; when
          only prox_f is foreign to the fused kernels, the regulariser side
          still runs fused (dual update in one pass, prox_f's argument in one
          pass: _run_native_dual);
  host    foreign NumPy-only callables: state stays in HBM, arguments are
          copied to the host for the callable only.

With a `tolerance` the run stops before `iterations` once its iterates have stopped
changing: after iteration k = check_every, 2 check_every, ... and the last,

    r_x = sqrt(sum (x_k - x_{k-1})^2 / sum x_k^2),   r_p likewise for the dual p

(p = 0 before the first iteration; a ratio whose numerator is exactly 0 counts as 0;
sums that are not finite never meet the criterion) and the run stops if
max(r_x, r_p) <= tolerance.  The fused forms run the check_every - 1 iterations
between two checks as before (multi-iteration and persistent kernels included) and
the checked iteration through k_pd_check (nsol_pdc.hip), which forms the four sums
from the values it holds in registers when it stores them; the other forms call
nsol_pd_change_* on the iterates before and after.  float32 rounding keeps r_x from
falling much below 1e-7: tolerances below about 1e-6 are not met in float32.
"""
import numpy as np

from . import ops
from .bridge import BridgedCallable
from .device import is_device_tensor
from .proximal_operators import (check_weights, scaled_data_on_device,
                                 weights_on_device)
from .solver import Solver
from ._accessors import add_accessors
from .symbolic import TauSym, trace_operator, trace_prox

# False: the "device" form glues every callable with separate axpy kernels even
# when the regulariser side is nsol_amd's own (the A/B reference of the tests)
USE_SEMI_FUSED = True
# 3-D volumes whose rows are not whole 16-byte vectors run with their arrays re-laid at
# a row pitch of whole vectors (nsol_pd_run_pitched_*), from this many voxels on
USE_ROW_PITCH = True
PITCH_MIN_VOXELS = 1 << 20


def step_schedule(alg_type, L2, lmbda, iterations):
    """Host-side step sizes; sigma[n], tau[n] are used inside iteration n and
    theta[n] in its over-relaxation (primal_dual_solver.py:222-253, 278-403).
    Unknown alg_type raises KeyError like the reference's dict lookup."""
    init = {"ALG2": _init_alg2, "ALG2_AHMOD": _init_alg2_ahmod,
            "ALG3": _init_alg3}[alg_type]
    tau, sigma, gamma = init(float(L2), lmbda)
    sig = np.empty(iterations)
    ta = np.empty(iterations)
    th = np.empty(iterations)
    for n in range(iterations):
        sig[n], ta[n] = sigma, tau
        if alg_type == "ALG3":
            theta = gamma            # constant steps; gamma carries theta
        else:
            theta = 1. / np.sqrt(1. + 2. * gamma * tau)
            tau = tau * theta
            sigma = sigma / theta
            if alg_type == "ALG2_AHMOD":
                theta = 0.
        th[n] = theta
    return sig, ta, th


def _init_alg2(L2, lmbda):
    tau0 = 1. / np.sqrt(L2)
    return tau0, 1. / (L2 * tau0), 0.35 * lmbda


def _init_alg2_ahmod(L2, lmbda):
    tau0 = 0.02
    return tau0, 4. / (L2 * tau0), 0.35 * lmbda


def _init_alg3(L2, lmbda, huber_alpha=0.05):
    mu = 2. * np.sqrt(lmbda * huber_alpha / L2)
    return mu / (2. * lmbda), mu / (2. * huber_alpha), 1. / (1. + mu)


def checked_tolerance(tolerance):
    """None, or the tolerance as a float >= 0 (ValueError for a negative one or NaN)."""
    if tolerance is None:
        return None
    tolerance = float(tolerance)
    if not tolerance >= 0.:
        raise ValueError("tolerance must be None or a number >= 0")
    return tolerance


def checked_check_every(check_every):
    """check_every as an int >= 1 (ValueError otherwise)."""
    try:
        k = int(check_every)
        ok = k >= 1 and k == check_every
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("check_every must be a positive integer")
    return k


def check_points(iterations, check_every):
    """Iterations after which the stopping rule is evaluated: check_every,
    2 check_every, ... and always the last."""
    iterations, check_every = int(iterations), int(check_every)
    if iterations < 1:
        return []
    pts = list(range(check_every, iterations + 1, check_every))
    if not pts or pts[-1] != iterations:
        pts.append(iterations)
    return pts


def relative_changes(sums):
    """(r_x, r_p) from the four sums {sum dx^2, sum x^2, sum dp^2, sum p^2}: a ratio
    whose numerator is exactly 0 is 0; NaN where a sum is not finite."""
    out = []
    for num, den in ((sums[0], sums[1]), (sums[2], sums[3])):
        num, den = float(num), float(den)
        if not (np.isfinite(num) and np.isfinite(den)):
            out.append(float("nan"))
        elif num == 0.:
            out.append(0.)
        elif den == 0.:
            out.append(float("inf"))
        else:
            out.append(float(np.sqrt(num / den)))
    return out[0], out[1]


def criterion_met(r_x, r_p, tolerance):
    """max(r_x, r_p) <= tolerance; never with a NaN among them."""
    return bool(np.isfinite(r_x) and np.isfinite(r_p) and
                max(r_x, r_p) <= tolerance)


class _StopRule(object):
    """The stopping rule of one run: its check points, the device workspace and
    board (one row of four sums per check) and the rows (k, r_x, r_p) read so far."""

    def __init__(self, tolerance, iterations, check_every):
        self.tolerance = float(tolerance)
        self.points = check_points(iterations, check_every)
        self._index = {p: j for j, p in enumerate(self.points)}
        self.ws = self.board = None
        self.rows = []

    def allocate(self, like, shape=None):
        """shape: the volume of the fused kernels (None: nsol_pd_change_* only)."""
        import torch
        if shape is not None:
            self.ws = ops.pd_check_workspace(like, shape)
        else:
            self.ws = torch.empty(ops.PD_CHECK_SUMS * 4096, dtype=torch.float64,
                                  device=like.device)
        self.board = torch.empty((max(len(self.points), 1), ops.PD_CHECK_SUMS),
                                 dtype=torch.float64, device=like.device)

    def is_point(self, it):
        return it in self._index

    def row(self, it):
        return self.board[self._index[it]]

    def decide(self, it):
        """Reads the row of check `it` back (this waits for the device) and says
        whether the run stops."""
        r_x, r_p = relative_changes(self.row(it).cpu().numpy())
        self.rows.append((float(it), r_x, r_p))
        return criterion_met(r_x, r_p, self.tolerance)


class PrimalDualSolver(Solver):

    def __init__(self, prox_f, prox_g_conj, B, B_conj, L2, x0, alpha=0.01,
                 iterations=10, x_scale=1., verbose=0, alg_type="ALG2",
                 dtype=None, tolerance=None, check_every=10):
        Solver.__init__(self, x0=x0, verbose=verbose, x_scale=x_scale,
                        dtype=dtype)
        self.set_tolerance(tolerance)
        self.set_check_every(check_every)
        self._iterations_done = None
        self._stop_reason = None
        self._rule = None
        self._prox_f = prox_f
        self._prox_g_conj = prox_g_conj
        self._B = B
        self._B_conj = B_conj
        self._L2 = float(L2)
        self._alpha = float(alpha)
        self._iterations = iterations
        self._alg_type = alg_type
        self._execution = None

    def get_execution(self):
        """'fused', 'device' or 'host' after run() (None before)."""
        return self._execution

    def print_statistics(self, fmt="%.3e"):
        pass

    # ---- the stopping rule -------------------------------------------
    def set_tolerance(self, tolerance):
        """None: run all `iterations`; else stop once max(r_x, r_p) <= tolerance."""
        self._tolerance = checked_tolerance(tolerance)

    def get_tolerance(self):
        return self._tolerance

    def set_check_every(self, check_every):
        self._check_every = checked_check_every(check_every)

    def get_check_every(self):
        return self._check_every

    def get_iterations_done(self):
        """Iterations the last run() did (None before one)."""
        return self._iterations_done

    def get_stop_reason(self):
        """'tolerance' or 'iterations' after run() (None before)."""
        return self._stop_reason

    def get_changes(self):
        """One row (k, r_x, r_p) per check of the last run()."""
        rows = self._rule.rows if self._rule is not None else []
        return np.array(rows, dtype=np.float64).reshape(-1, 3)

    # ------------------------------------------------------------------
    def _native_dual(self):
        """The regulariser side when it is nsol_amd's own: B = gradient, B_conj
        its adjoint, prox_g_conj = prox_tv_conj / prox_huber_conj.  Returns
        dict(shape, w, dim, flags, gamma) or None."""
        n = int(self._x0_host.size if self._x0_host is not None
                else self._x0_dev.numel())
        dB = trace_operator(self._B, n)
        if dB is None or dB[0] != "grad":
            return None
        gop, shape = dB[1], dB[2]
        if int(np.prod(shape)) != n or len(shape) != gop.dimension:
            return None
        dBt = trace_operator(self._B_conj, gop.dimension * n)
        if dBt is None or dBt[0] != "grad_adj":
            return None
        if tuple(dBt[1].w) != tuple(gop.w) or \
                dBt[1].dimension != gop.dimension or \
                tuple(dBt[2]) != tuple(gop._out_shape(shape)):
            return None
        dg = trace_prox(self._prox_g_conj, gop.dimension * n)
        if dg is None or dg[0] not in (
                "prox_tv_conj", "prox_huber_conj", "prox_tv_conj_iso",
                "prox_huber_conj_iso") or not isinstance(dg[1], TauSym):
            return None
        huber = dg[0].startswith("prox_huber_conj")
        flags = ops.PD_REG_HUBER if huber else ops.PD_REG_TV
        if dg[0].endswith("_iso"):
            # the vector norm is taken over the gradient operator's components
            if dg[-1] != gop.dimension:
                return None
            flags |= ops.PD_REG_ISOTROPIC
        return dict(shape=tuple(shape), w=gop.w, dim=gop.dimension, n=n,
                    flags=flags, gamma=(dg[2] if huber else 0.05))

    def plan(self):
        """Recognise a fully native configuration.  Returns a dict for the
        fused kernel or None."""
        dual = self._native_dual()
        if dual is None:
            return None
        n = dual["n"]
        df = trace_prox(self._prox_f, n)
        if df is None or df[0] not in ("prox_ell1", "prox_ell2", "prox_ell1_w",
                                       "prox_ell2_w") \
                or not isinstance(df[3], TauSym):
            return None
        data = df[1]
        dsize = data.numel() if is_device_tensor(data) else np.size(data)
        if dsize != n:
            return None
        flags = dual["flags"]
        flags |= ops.PD_DATA_L1 if df[0].startswith("prox_ell1") else ops.PD_DATA_L2
        plan = dict(shape=dual["shape"], w=dual["w"], dim=dual["dim"],
                    flags=flags, gamma=dual["gamma"], data=data,
                    data_scale=df[2])
        if df[0].endswith("_w"):
            # wrong weights are an error, not a reason for a slower path
            check_weights(df[4], n)
            plan["flags"] |= ops.PD_DATA_WEIGHTED
            plan["weights"] = df[4]
        return plan

    def _run(self):
        self._points = self._observe_start(self._iterations)
        lmbda = 1. / self._alpha
        sig, ta, th = step_schedule(self._alg_type, self._L2, lmbda,
                                    self._iterations)
        self._rule = None if self._tolerance is None else _StopRule(
            self._tolerance, self._iterations, self._check_every)
        self._iterations_done, self._stop_reason = 0, "iterations"
        plan = self.plan()
        if plan is not None:
            self._execution = "fused"
            self._run_fused(plan, lmbda, sig, ta, th)
        else:
            self._run_generic(lmbda, sig, ta, th)
        if self._rule is None:
            self._iterations_done = max(int(self._iterations), 0)

    def _stops_after(self, it):
        """Bookkeeping after iteration `it` of a run with a tolerance; True when the
        rule was evaluated there and the run stops."""
        self._iterations_done = it
        if self._rule.is_point(it) and self._rule.decide(it):
            self._stop_reason = "tolerance"
            return True
        return False

    # ------------------------------------------------------------------
    def _run_fused(self, plan, lmbda, sig, ta, th):
        import torch
        x = self._x0_device().clone()
        xbar = [x.clone(), torch.empty_like(x)]
        n = x.numel()
        p = [torch.empty(plan["dim"] * n, dtype=x.dtype, device=x.device)
             for _ in range(2)]
        bt = scaled_data_on_device(plan["data"], plan["data_scale"], x)
        if self._rule is not None:
            self._run_checked(plan, lmbda, sig, ta, th, x, xbar, p, bt)
            return
        if plan["flags"] & ops.PD_DATA_WEIGHTED:
            self._run_weighted(plan, lmbda, sig, ta, th, x, xbar, p, bt)
            return
        # a device-mode observer (observer.py) keeps the multi-iteration kernels
        # and the row pitch: the run is enqueued in chunks between its
        # observation points, nsol_observe_* reads the pitched x as it is
        unobserved = self._observer is None or self._points is not None
        pitch = ops.row_pitch(plan["shape"], x) if USE_ROW_PITCH and \
            n >= PITCH_MIN_VOXELS and self._iterations > 1 and \
            unobserved and not self._verbose else 0
        if pitch:
            # rows that are not whole 16-byte vectors (511^3, 181 x 217 x 181 ...): the
            # run's arrays hold them at a pitch of whole vectors -- aligned accesses
            # and whole stores instead of the ragged form's element-aligned ones (511^3:
            # the speed of 512^3 instead of +15...30 %); two re-layouts per run
            shape = plan["shape"]
            xq = ops.to_pitched(x, shape, pitch)
            np_ = xq.numel()
            xbq = [xq.clone(), torch.empty_like(xq)]
            pq = [torch.zeros(plan["dim"] * np_, dtype=x.dtype, device=x.device),
                  torch.empty(plan["dim"] * np_, dtype=x.dtype, device=x.device)]
            btq = ops.to_pitched(bt, shape, pitch)
            try:
                self._chunks(xbq, xq, btq, pq, plan, lmbda, sig, ta, th,
                             torch.zeros_like(xq), pitch)
                self._x = ops.from_pitched(xq, shape, pitch)
                return
            except ValueError:
                # the pitched entry declined (NSOL_EINVAL: the ragged-row form is
                # switched off, knob pd_rag): the contiguous arrays are untouched
                del xq, xbq, pq, btq
        if unobserved and not self._verbose:
            # scratch for the two-iterations-per-pass kernel (x ping-pong)
            x_alt = torch.empty_like(x) if self._iterations > 1 else None
            self._chunks(xbar, x, bt, p, plan, lmbda, sig, ta, th, x_alt, 0)
            self._x = x
            return
        for i in range(self._iterations):      # observed / verbose: stepwise
            if self._verbose:
                print("Primal-Dual iteration %d/%d" % (i + 1,
                                                       self._iterations))
            k = i & 1
            hden = 1. + sig[i] * plan["gamma"] \
                if plan["flags"] & ops.PD_REG_HUBER else 1.
            ops.pd_fused_iter(xbar[k], xbar[1 - k], x, bt,
                              None if i == 0 else p[k], p[1 - k],
                              plan["shape"], plan["w"], sig[i], hden, ta[i],
                              ta[i] * lmbda, th[i], plan["flags"])
            self._x = x
            self._observe_iteration(i + 1, x)
        self._x = x

    def _run_weighted(self, plan, lmbda, sig, ta, th, x, xbar, p, bt):
        """The fused run with a weighted data term (k_pd_w, nsol_pdw.hip): one
        iteration per launch, contiguous arrays -- no row pitch, no multi-iteration
        kernels and never the persistent kernel, which have no weighted form.  The
        weights are converted to the working dtype once per run."""
        wt = weights_on_device(plan["weights"], x)
        shape, w, flags = plan["shape"], plan["w"], plan["flags"]
        unobserved = self._observer is None or self._points is not None
        if unobserved and not self._verbose:
            # the whole run, or the stretches between a device-mode observer's points
            pts = self._points
            bounds = [0, self._iterations] if pts is None else pts
            k = 0
            for a, b in zip(bounds[:-1], bounds[1:]):
                slot = ops.pd_weighted_run(
                    xbar[k], xbar[1 - k], x, bt, wt, p[k], p[1 - k], 1, shape, w,
                    [lmbda], sig[a:b], ta[a:b], th[a:b], a == 0, plan["gamma"], flags)
                if slot is None:
                    raise ValueError("nsol_pd_weighted_run does not take a volume "
                                     "of shape %r" % (tuple(shape),))
                k = k if slot == 0 else 1 - k
                if pts is not None:
                    self._observe_at(b, x, None)
            self._x = x
            return
        tab = ops.pd_weighted_table(x, 1, [lmbda], sig, ta, th, True, plan["gamma"],
                                    flags)
        for i in range(self._iterations):      # observed / verbose: stepwise
            if self._verbose:
                print("Primal-Dual iteration %d/%d" % (i + 1,
                                                       self._iterations))
            k = i & 1
            if not ops.pd_weighted_iter(xbar[k], xbar[1 - k], x, bt, wt, p[k],
                                        p[1 - k], 1, shape, w, tab, i, flags):
                raise ValueError("nsol_pd_weighted_iter does not take a volume of "
                                 "shape %r" % (tuple(shape),))
            self._x = x
            self._observe_iteration(i + 1, x)
        self._x = x

    def _run_checked(self, plan, lmbda, sig, ta, th, x, xbar, p, bt):
        """The fused run with a tolerance, weighted or not: contiguous arrays (no row
        pitch).  The run is enqueued in stretches between the check points merged
        with a device-mode observer's points; a stretch that ends in a check runs
        all but its last iteration through ops.pd_run / ops.pd_weighted_run as an
        unchecked run does, and the last through k_pd_check, whose sums are read
        back for the decision.  With verbose or an observer that keeps iterates the
        stretches are single iterations (a weighted run then launches them from one
        table of scalars, as _run_weighted does)."""
        import torch
        rule = self._rule
        shape, w, flags = plan["shape"], plan["w"], plan["flags"]
        weighted = bool(flags & ops.PD_DATA_WEIGHTED)
        wt = weights_on_device(plan["weights"], x) if weighted else None
        rule.allocate(x, shape)
        iters = int(self._iterations)
        stepwise = bool(self._verbose) or not (
            self._observer is None or self._points is not None)
        if stepwise:
            bounds = list(range(iters + 1))
        else:
            bounds = sorted(set([0]) | set(self._points or []) | set(rule.points))
        x_alt = torch.empty_like(x) if not weighted and iters > 1 else None
        huber = bool(flags & ops.PD_REG_HUBER)
        # stepwise and weighted: one table for the whole run, as _run_weighted has
        tab = ops.pd_weighted_table(x, 1, [lmbda], sig, ta, th, True, plan["gamma"],
                                    flags) if stepwise and weighted else None
        k = 0
        for a, b in zip(bounds[:-1], bounds[1:]):
            if self._verbose:
                print("Primal-Dual iteration %d/%d" % (b, iters))
            check = rule.is_point(b)
            last = b - 1 if check else b
            if last > a and tab is not None:
                if not ops.pd_weighted_iter(xbar[k], xbar[1 - k], x, bt, wt, p[k],
                                            p[1 - k], 1, shape, w, tab, a, flags):
                    raise ValueError("nsol_pd_weighted_iter does not take a volume of "
                                     "shape %r" % (tuple(shape),))
                k = 1 - k
            elif last > a and weighted:
                slot = ops.pd_weighted_run(
                    xbar[k], xbar[1 - k], x, bt, wt, p[k], p[1 - k], 1, shape, w,
                    [lmbda], sig[a:last], ta[a:last], th[a:last], a == 0, plan["gamma"],
                    flags)
                if slot is None:
                    raise ValueError("nsol_pd_weighted_run does not take a volume "
                                     "of shape %r" % (tuple(shape),))
                k = k if slot == 0 else 1 - k
            elif last > a:
                slot = ops.pd_run(xbar[k], xbar[1 - k], x, bt, p[k], p[1 - k], shape, w,
                                  lmbda, sig[a:last], ta[a:last], th[a:last], a == 0,
                                  plan["gamma"], flags, x_alt=x_alt, swap_ok=True)
                k = k if slot == 0 else 1 - k
            if ops._pending_runs:
                # (a persistent stretch that timed out is repeated here, before the
                # checking kernel or the observer reads its x)
                ops.settle_persist_runs()
            if check:
                i = b - 1
                hden = 1. + sig[i] * plan["gamma"] if huber else 1.
                if not ops.pd_check_iter(xbar[k], xbar[1 - k], x, bt, wt,
                                         None if i == 0 else p[k], p[1 - k], shape, w,
                                         sig[i], hden, ta[i], ta[i] * lmbda, th[i],
                                         flags, rule.ws, rule.row(b)):
                    raise ValueError("nsol_pd_check_iter does not take a volume of "
                                     "shape %r" % (tuple(shape),))
                k = 1 - k
            self._x = x
            if stepwise:
                self._observe_iteration(b, x)
            elif self._points is not None:
                self._observe_at(b, x, None)
            if self._stops_after(b):
                break
        self._x = x

    _points = None

    def _chunks(self, xbar, x, bt, p, plan, lmbda, sig, ta, th, x_alt, pitch):
        """ops.pd_run over the whole run, or, with a device-mode observer, over
        the stretches between its observation points (the multi-iteration
        kernels are bit-identical to a launch per iteration, so the chunks
        change no bit of x): each chunk starts from the xbar / p slot the
        previous one ended in, p counts as zero in the first chunk only."""
        pts = self._points
        bounds = [0, self._iterations] if pts is None else pts
        layout = (plan["shape"], pitch) if pitch else None
        k, first = 0, True
        for a, b in zip(bounds[:-1], bounds[1:]):
            slot = ops.pd_run(xbar[k], xbar[1 - k], x, bt, p[k], p[1 - k],
                              plan["shape"], plan["w"], lmbda, sig[a:b], ta[a:b],
                              th[a:b], first, plan["gamma"], plan["flags"],
                              x_alt=x_alt, swap_ok=True, pitch=pitch)
            k = k if slot == 0 else 1 - k
            first = False
            if pts is not None:
                if ops._pending_runs:
                    # (a persistent chunk that timed out is repeated here, before
                    # its x is observed)
                    ops.settle_persist_runs()
                self._observe_at(b, x, layout)

    def _observe_iteration(self, it, x):
        if self._observer is None:
            return
        if self._points is None:
            self._observer.add_x(self.get_x())
        else:
            self._observe_at(it, x)

    # ------------------------------------------------------------------
    def _run_generic(self, lmbda, sig, ta, th):
        x = self._x0_device().clone()
        xbar = x.clone()
        pf = BridgedCallable(self._prox_f, self._dtype)
        dual = self._native_dual() if USE_SEMI_FUSED else None
        if dual is not None:
            self._run_native_dual(dual, pf, x, xbar, lmbda, sig, ta, th)
            return
        B = BridgedCallable(self._B, self._dtype)
        Bc = BridgedCallable(self._B_conj, self._dtype)
        pg = BridgedCallable(self._prox_g_conj, self._dtype)
        p = None
        rule = self._rule
        if rule is not None:
            rule.allocate(x)
        for i in range(self._iterations):
            if self._verbose:
                print("Primal-Dual iteration %d/%d" % (i + 1,
                                                       self._iterations))
            g = B(xbar)
            # p + sigma * B(xbar); p = 0 before the first iteration
            q = ops.scale(g, sig[i]) if p is None else \
                ops.lincomb2(1.0, p, sig[i], g)
            p_old, p = p, pg(q, float(sig[i]))
            u = ops.lincomb2(1.0, x, -ta[i], Bc(p))
            x_new = pf(u, float(ta[i] * lmbda))
            # x_new + theta * (x_new - x)
            d = ops.lincomb2(1.0, x_new, -1.0, x)
            xbar = ops.lincomb2(1.0, x_new, th[i], d)
            if rule is not None and rule.is_point(i + 1):
                ops.pd_change(x, x_new, p_old, p, rule.ws, rule.row(i + 1))
            x = x_new
            self._x = x
            self._observe_iteration(i + 1, x)
            if rule is not None and self._stops_after(i + 1):
                break
        self._x = x
        self._execution = "device" if all(
            c.on_device for c in (B, Bc, pg, pf)) else "host"

    def _run_native_dual(self, dual, pf, x, xbar, lmbda, sig, ta, th):
        """The loop of _run_generic when only prox_f is foreign to the fused
        kernels (e.g. prox_linear_least_squares: PD deconvolution, interface
        :257-280): the dual update in one pass (nsol_pd_dual_step_*: gradient,
        axpy and clamp, 28 bytes per voxel instead of 76), prox_f's argument
        x - tau K^T p in one pass (20 instead of 28) and the over-relaxation in
        one (12 instead of 24); the same values as the generic loop."""
        import torch
        shape, w = dual["shape"], dual["w"]
        p = torch.empty(dual["dim"] * x.numel(), dtype=x.dtype, device=x.device)
        huber = bool(dual["flags"] & ops.PD_REG_HUBER)
        rule = self._rule
        if rule is not None:
            rule.allocate(x)
        dual_step = ops.pd_dual_step_iso \
            if dual["flags"] & ops.PD_REG_ISOTROPIC else ops.pd_dual_step
        for i in range(self._iterations):
            if self._verbose:
                print("Primal-Dual iteration %d/%d" % (i + 1,
                                                       self._iterations))
            hden = 1. + sig[i] * dual["gamma"] if huber else 1.
            check = rule is not None and rule.is_point(i + 1)
            # (the dual step updates p in place: a checked iteration keeps the old)
            p_old = p.clone() if check and i > 0 else None
            dual_step(xbar, None if i == 0 else p, p, shape, w, sig[i], hden)
            u = ops.grad_adj_axpy(p, x, ta[i], shape, w)
            x_new = pf(u, float(ta[i] * lmbda))
            xbar = ops.extrapolate(x_new, x, th[i], out=xbar)
            if check:
                ops.pd_change(x, x_new, p_old, p, rule.ws, rule.row(i + 1))
            x = x_new
            self._x = x
            self._observe_iteration(i + 1, x)
            if rule is not None and self._stops_after(i + 1):
                break
        self._x = x
        self._execution = "device" if pf.on_device else "host"


add_accessors(PrimalDualSolver, ["alpha", "L2", "alg_type", "iterations"])
