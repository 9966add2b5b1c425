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
changing (the rule: stopping.py).  The fused forms run the check_every - 1 iterations
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
from .stopping import (Stopping, _StopRule, check_points, checked_check_every,  # noqa: F401
                       checked_tolerance, criterion_met, next_slot, relative_changes,
                       stretch_bounds)
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


def _taken(took, entry, shape):
    """What a launch returned, unless the library declined it (None / False)."""
    if took is None or took is False:
        raise ValueError("nsol_%s does not take a volume of shape %r" %
                         (entry, tuple(shape)))
    return took


class _PlainForm(object):
    """How PrimalDualSolver._run_stretches advances a fused run: ops.pd_run over a
    stretch (multi-iteration and persistent kernels included; pitch > 0: every array at
    that row pitch), ops.pd_check_iter for a checked iteration.  single: the stretches
    are single iterations of a run without a tolerance, launched through the
    one-iteration entry.  A new fused form supplies an object like this one."""
    wt = None

    def __init__(self, plan, lmbda, sig, ta, th, x, bt, x_alt=None, pitch=0,
                 single=False):
        self.shape, self.w, self.flags = plan["shape"], plan["w"], plan["flags"]
        self.gamma = plan["gamma"]
        self.lmbda, self.sig, self.ta, self.th = lmbda, sig, ta, th
        self.x, self.bt, self.x_alt, self.pitch, self.single = x, bt, x_alt, pitch, single
        # what the observer reads x as
        self.layout = (self.shape, pitch) if pitch else None

    def _hden(self, i):
        return 1. + self.sig[i] * self.gamma if self.flags & ops.PD_REG_HUBER else 1.

    def advance(self, xbar_in, xbar_out, p_in, p_out, a, last):
        """Iterations a ... last - 1 (p counts as zero before iteration 0); returns
        the slot of ops.pd_run."""
        sig, ta, th = self.sig, self.ta, self.th
        if self.single:
            ops.pd_fused_iter(xbar_in, xbar_out, self.x, self.bt,
                              None if a == 0 else p_in, p_out, self.shape, self.w,
                              sig[a], self._hden(a), ta[a], ta[a] * self.lmbda, th[a],
                              self.flags)
            return 1
        return ops.pd_run(xbar_in, xbar_out, self.x, self.bt, p_in, p_out, self.shape,
                          self.w, self.lmbda, sig[a:last], ta[a:last], th[a:last], a == 0,
                          self.gamma, self.flags, x_alt=self.x_alt, swap_ok=True,
                          pitch=self.pitch)

    def check(self, xbar_in, xbar_out, p_in, p_out, i, ws, row):
        """Iteration i through k_pd_check, its four sums into `row`."""
        _taken(ops.pd_check_iter(xbar_in, xbar_out, self.x, self.bt, self.wt,
                                 None if i == 0 else p_in, p_out, self.shape, self.w,
                                 self.sig[i], self._hden(i), self.ta[i],
                                 self.ta[i] * self.lmbda, self.th[i], self.flags, ws, row),
               "pd_check_iter", self.shape)


class _WeightedForm(_PlainForm):
    """The fused run with a weighted data term (k_pd_w, nsol_pdw.hip): one iteration
    per launch, contiguous arrays -- no row pitch, no multi-iteration kernels and never
    the persistent kernel, which have no weighted form.  stepwise: the stretches are
    single iterations, launched from one table of the run's scalars."""

    def __init__(self, plan, lmbda, sig, ta, th, x, bt, wt, stepwise):
        _PlainForm.__init__(self, plan, lmbda, sig, ta, th, x, bt)
        self.wt = wt
        self.tab = ops.pd_weighted_table(x, 1, [lmbda], sig, ta, th, True, self.gamma,
                                         self.flags) if stepwise else None

    def advance(self, xbar_in, xbar_out, p_in, p_out, a, last):
        if self.tab is not None:
            _taken(ops.pd_weighted_iter(xbar_in, xbar_out, self.x, self.bt, self.wt, p_in,
                                        p_out, 1, self.shape, self.w, self.tab, a,
                                        self.flags), "pd_weighted_iter", self.shape)
            return 1
        return _taken(ops.pd_weighted_run(
            xbar_in, xbar_out, self.x, self.bt, self.wt, p_in, p_out, 1, self.shape,
            self.w, [self.lmbda], self.sig[a:last], self.ta[a:last], self.th[a:last],
            a == 0, self.gamma, self.flags), "pd_weighted_run", self.shape)


class PrimalDualSolver(Stopping, Solver):

    def __init__(self, prox_f, prox_g_conj, B, B_conj, L2, x0, alpha=0.01,
                 iterations=10, x_scale=1., verbose=0, alg_type="ALG2",
                 dtype=None, tolerance=None, check_every=10):
        Solver.__init__(self, x0=x0, verbose=verbose, x_scale=x_scale,
                        dtype=dtype)
        self.set_tolerance(tolerance)
        self.set_check_every(check_every)
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
        self._start_rule(self._iterations)
        plan = self.plan()
        if plan is not None:
            self._execution = "fused"
            self._run_fused(plan, lmbda, sig, ta, th)
        else:
            self._run_generic(lmbda, sig, ta, th)
        if self._rule is None:
            self._iterations_done = max(int(self._iterations), 0)

    # ------------------------------------------------------------------
    def _run_fused(self, plan, lmbda, sig, ta, th):
        """The fused run: a form object (plain, pitched or weighted) driven by
        _run_stretches.  A run with a tolerance or weights gives up the row pitch."""
        import torch
        x = self._x0_device().clone()
        n, iters = x.numel(), int(self._iterations)
        bt = scaled_data_on_device(plan["data"], plan["data_scale"], x)
        rule = self._rule
        weighted = bool(plan["flags"] & ops.PD_DATA_WEIGHTED)
        bounds, stepwise = self._stretch_bounds(iters)
        if rule is not None:
            rule.allocate(x, plan["shape"])
        pitch = ops.row_pitch(plan["shape"], x) if USE_ROW_PITCH and \
            n >= PITCH_MIN_VOXELS and iters > 1 and \
            not (stepwise or weighted or rule is not None) else 0
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
            form = _PlainForm(plan, lmbda, sig, ta, th, xq,
                              ops.to_pitched(bt, shape, pitch), torch.zeros_like(xq),
                              pitch)
            try:
                self._run_stretches(form, xbq, pq, bounds)
                self._x = ops.from_pitched(xq, shape, pitch)
                return
            except ValueError:
                # the pitched entry declined (NSOL_EINVAL: the ragged-row form is
                # switched off, knob pd_rag): the contiguous arrays are untouched
                del xq, xbq, pq, form
        xbar = [x.clone(), torch.empty_like(x)]
        p = [torch.empty(plan["dim"] * n, dtype=x.dtype, device=x.device)
             for _ in range(2)]
        if weighted:
            # (the weights are converted to the working dtype once per run)
            form = _WeightedForm(plan, lmbda, sig, ta, th, x, bt,
                                 weights_on_device(plan["weights"], x), stepwise)
        else:
            # x_alt: scratch for the multi-iteration kernels (x ping-pong); none for
            # single iterations, checked or not: nsol_pd_run_* reads it only where two
            # or more iterations are left, so the launches are the same without it
            form = _PlainForm(
                plan, lmbda, sig, ta, th, x, bt,
                torch.empty_like(x) if iters > 1 and not stepwise else None,
                single=stepwise and rule is None)
        self._x = x
        self._run_stretches(form, xbar, p, bounds)

    _points = None

    def _stretch_bounds(self, iters):
        """(bounds of the stretches the run is enqueued in, stepwise).  Verbose, or an
        observer that keeps iterates: stepwise, the stretches are single iterations.  A
        device-mode observer (observer.py) keeps the multi-iteration kernels and the row
        pitch: the stretches end at its points (nsol_observe_* reads the pitched x as
        it is), merged with the rule's check points."""
        if self._verbose or not (self._observer is None or self._points is not None):
            return list(range(iters + 1)), True
        if self._rule is not None:
            return stretch_bounds(iters, self._check_every, self._points), False
        return ([0, iters] if self._points is None else self._points), False

    def _run_stretches(self, form, xbar, p, bounds):
        """The loop of every fused run: the run is enqueued in the stretches between
        `bounds` (check points, a device-mode observer's points, every iteration when
        stepwise), each starting from the xbar / p half the one before ended in.  A
        stretch that ends in a check runs all but its last iteration as an unchecked
        run does and the last in the checking form, whose sums are read back for the
        decision (the multi-iteration kernels are bit-identical to a launch per
        iteration, so the stretches change no bit of x).  Pending persistent runs are
        settled before every check and observation, whatever the form: only
        ops.pd_run leaves one, but a foreign one (an outer solver's) is then settled
        here too, before x is read.  form: _PlainForm's interface."""
        rule, iters = self._rule, int(self._iterations)
        observed = self._observer is not None
        k = 0
        for a, b in zip(bounds[:-1], bounds[1:]):
            if self._verbose:
                print("Primal-Dual iteration %d/%d" % (b, iters))
            check = rule is not None and rule.is_point(b)
            last = b - 1 if check else b
            if last > a:
                k = next_slot(k, form.advance(xbar[k], xbar[1 - k], p[k], p[1 - k], a,
                                              last))
            if ops._pending_runs and (check or observed):
                # (a persistent stretch that timed out is repeated here, before the
                # checking kernel or the observer reads its x)
                ops.settle_persist_runs()
            if check:
                form.check(xbar[k], xbar[1 - k], p[k], p[1 - k], b - 1, rule.ws,
                           rule.row(b))
                k = 1 - k
            if observed:
                self._observe_iteration(b, form.x, form.layout)
            if self._stops_after(b):
                break

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
            if self._stops_after(i + 1):
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
            if self._stops_after(i + 1):
                break
        self._x = x
        self._execution = "device" if pf.on_device else "host"


add_accessors(PrimalDualSolver, ["alpha", "L2", "alg_type", "iterations"])
