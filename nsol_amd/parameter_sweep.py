"""Parameter sweeps of the primal-dual solver on one observation (the job of the
reference's solver_parameter_study.py / primal_dual_solver_parameter_study.py,
without their SimpleITK / pysitk / natsort file handling).

    sweep = PrimalDualSweep(prox_f, prox_g_conj, B, B_conj, L2, x0,
                            parameters={"alpha": [...], "alg_type": [...]},
                            iterations=50, x_scale=xs)
    sweep.set_measures({"PSNR": lambda x: ...}, every=10)
    sweep.run()
    m, best = sweep.best("PSNR")

The members are the elements of itertools.product over the parameter lists in
the order the dictionary gives them (solver_parameter_study.py, _run).  Two
execution forms, the same results and the same interface:
  stacked     a natively fused configuration (PrimalDualSolver.plan()): the
              observation is uploaded and scaled once and all members advance
              together, ONE launch per iteration (nsol_pd_sweep_run_*; with a
              weighted data term nsol_pd_weighted_run_*, the weights shared), in
              groups that keep the state under ops.PD_SWEEP_GROUP_BYTES; the
              measures are taken on the device from each member's slice of the
              stacked iterate;
  sequential  anything else (foreign callables, deconvolution, members larger
              than ops.PD_SWEEP_MAX_VOXELS, a geometry the library declines, a
              `tolerance`: every member then stops at an iteration of its own,
              get_iterations_done()): one PrimalDualSolver after the other.

PrimalDualSweep(..., tolerance=, stacked_stopping=True) keeps a sweep with a
tolerance stacked: the members advance in one launch per iteration over a device
map of the members still running, observation and weights shared, and every member
leaves the map at the check that meets the tolerance
(nsol_amd/stacked_stopping.py, nsol_pdm.hip).  The default is off.
"""
import datetime
import itertools
import time

import numpy as np

from . import ops
from .observer import Observer
from .primal_dual_solver import PrimalDualSolver
from .stacked_run import run_stack
from .stopping import checked_check_every, checked_tolerance

PARAMETER_KEYS = ("alpha", "alg_type", "L2")


def member_parameters(parameters, keys=PARAMETER_KEYS):
    """The members of a sweep: one dict per element of itertools.product over the
    value lists, in the dictionary's own key order.  keys: the parameters the kind of
    sweep knows (tgv_stack.TGVPrimalDualSweep: alpha and beta)."""
    known = tuple(keys)
    keys = list(parameters.keys())
    for k in keys:
        if k not in known:
            raise ValueError("unknown sweep parameter '%s' (known: %s)" %
                             (k, ", ".join(known)))
    values = []
    for k in keys:
        v = parameters[k]
        v = [v] if isinstance(v, (str, bytes)) or np.ndim(v) == 0 else list(v)
        if len(v) == 0:
            raise ValueError("sweep parameter '%s' has no values" % k)
        values.append(v)
    if not keys:
        raise ValueError("a sweep needs at least one parameter")
    return [dict(zip(keys, combo)) for combo in itertools.product(*values)]


class PrimalDualSweep(object):

    def __init__(self, prox_f, prox_g_conj, B, B_conj, L2, x0, parameters,
                 iterations=50, x_scale=1., dtype=None, alpha=0.01,
                 alg_type="ALG2", tolerance=None, check_every=10,
                 stacked_stopping=False):
        self._callables = dict(prox_f=prox_f, prox_g_conj=prox_g_conj, B=B,
                               B_conj=B_conj)
        self._defaults = dict(alpha=alpha, alg_type=alg_type, L2=L2)
        # a tolerance (PrimalDualSolver's stopping rule): every member stops at an
        # iteration of its own, so the members run one after the other -- or, with
        # stacked_stopping, stacked over a map of the members still running
        self._init_state(x0, member_parameters(parameters), iterations,
                         checked_tolerance(tolerance), checked_check_every(check_every),
                         stacked_stopping, x_scale, dtype)

    def _init_state(self, x0, members, iterations, tolerance, check_every,
                    stacked_stopping, x_scale, dtype):
        """What every kind of sweep keeps, whatever solver its members are."""
        self._x0 = x0
        self._members = members
        self._iterations = int(iterations)
        self._tolerance = tolerance
        self._stacked_stopping = bool(stacked_stopping)
        self._check_every = check_every
        self._iterations_done = None
        self._x_scale = float(x_scale)
        self._dtype = dtype
        self._functions = {}
        self._every = None
        self._execution = None
        self._computational_time = datetime.timedelta(seconds=0)
        self._x_all = None          # stacked: (P * n) device tensor, solver units
        self._x_list = None         # sequential: per member, caller's units
        self._observers = []
        self._n = None

    # ------------------------------------------------------------------
    def set_measures(self, measures_dic, every=None):
        """Measures of every member's iterate x (caller's units), taken at
        iterations 0, every, 2 every, ... and the last; every=None: at the
        final iterate only."""
        if every is not None and int(every) < 1:
            raise ValueError("every must be a positive integer")
        self._functions = dict(measures_dic)
        self._every = None if every is None else int(every)

    def get_parameters(self):
        return [dict(m) for m in self._members]

    def get_execution(self):
        """'stacked' or 'sequential' after run() (None before)."""
        return self._execution

    def get_computational_time(self):
        return self._computational_time

    def _solver(self, member=None):
        kw = dict(self._defaults)
        kw.update(member or {})
        return PrimalDualSolver(
            x0=self._x0, iterations=self._iterations, x_scale=self._x_scale,
            dtype=self._dtype, alpha=kw["alpha"], alg_type=kw["alg_type"],
            L2=kw["L2"], tolerance=self._tolerance, check_every=self._check_every,
            **self._callables)

    def _observer(self):
        if not self._functions:
            return None
        obs = Observer(keep_iterates=False,
                       every=self._every or max(self._iterations, 1))
        obs.set_measures(self._functions)
        return obs

    # ------------------------------------------------------------------
    def run(self):
        import torch
        t0 = time.time()
        template = self._solver(self._members[0])
        if template._x0_ndim != 1:
            raise ValueError("Initial value x0 must be a 1D array")
        self._x_all = self._x_list = None
        self._observers = []
        self._iterations_done = None
        form = self._stack_form(template)
        stacked = form is not None and self._run_stacked(template, form)
        if not stacked:
            self._run_sequential()
        torch.cuda.synchronize()
        self._after_wait()
        for obs in self._observers:
            obs._finish()                 # every board, read after the one wait
        self._execution = "stacked" if stacked else "sequential"
        # the measure step: a measure that raised during the run fails here
        for obs in self._observers:
            obs.compute_measures()
        self._computational_time = datetime.timedelta(seconds=time.time() - t0)

    def _run_sequential(self):
        """One solver after the other, as the command-line tools loop."""
        self._x_list, self._observers = [], []
        self._iterations_done = []
        for member in self._members:
            solver = self._solver(member)
            obs = self._observer()
            if obs is not None:
                solver.set_observer(obs)
                self._observers.append(obs)
            solver.run()
            self._n = solver._x.numel()
            self._x_list.append(solver.get_x_device())
            self._iterations_done.append(solver.get_iterations_done())

    def _run_stacked(self, template, form):
        """All members together, observation, weights and start shared; False when the
        library declined (nothing has run then).  What differs from one kind of sweep
        to the other is behind three methods: _stack_form (whether the template
        stacks), _shared_operands and _advance."""
        import torch
        from .device import to_device
        iters, P = self._iterations, len(self._members)
        x0 = template._x0_device()
        n = x0.numel()
        bt, wt, G = self._shared_operands(template, form, x0)
        x_all = torch.empty(P * n, dtype=x0.dtype, device=x0.device)
        x_all.view(P, n).copy_(x0)
        # the observation of the start vector, as Solver._observe_at(0) makes it
        observers, points = [], None
        if self._functions:
            refs = {}
            for _ in range(P):
                obs = self._observer()
                points = obs._begin(n, iters, refs)
                observers.append(obs)
            if self._every is not None:
                if template._x0_host is not None:
                    start, scale = to_device(template._x0_host.reshape(-1),
                                             template._x0_host.dtype.type), 1.0
                else:
                    start, scale = x0, self._x_scale
                for obs in observers:
                    obs._observe(0, start, scale)
        res = self._advance(
            template, form, x_all, bt, wt, G, points,
            (lambda m, it: observers[m]._observe(
                it, x_all[m * n:(m + 1) * n], self._x_scale)) if observers else None, x0)
        if res is None:
            return False
        self._x_all, self._n, self._observers = x_all, n, observers
        self._group = G
        return True

    # ---- what PrimalDualLinearSweep replaces
    def _stack_form(self, template):
        """What the stacked run of sweeps like `template` is built from -- here the
        template's plan() -- or None where the members run one after the other."""
        plan = template.plan()
        if plan is not None and self._iterations > 0 and \
                (self._tolerance is None or self._stacked_stopping) and \
                int(np.prod(plan["shape"])) <= ops.PD_SWEEP_MAX_VOXELS:
            return plan
        return None

    def _after_wait(self):
        ops.settle_persist_runs(synchronize=False)

    def _shared_operands(self, template, plan, x0):
        """(bt, wt, members per group): the scaled observation and the weights (None:
        unweighted) that the members share, n elements each like x0."""
        from .proximal_operators import scaled_data_on_device, weights_on_device
        bt = scaled_data_on_device(plan["data"], plan["data_scale"], x0)
        wt = weights_on_device(plan["weights"], x0) \
            if plan["flags"] & ops.PD_DATA_WEIGHTED else None
        return bt, wt, ops.sweep_group_size(len(self._members), x0.numel(), plan["dim"],
                                            x0.element_size())

    def _advance(self, template, plan, x_all, bt, wt, group, points, observe, x0):
        """One launch per iteration and group (stacked_run.run_stack: ops.pd_sweep_run,
        with weights ops.pd_weighted_run, with a tolerance stacked_stopping.run_group).
        Returns None when the library declined."""
        iters = self._iterations
        kws = [dict(self._defaults, **member) for member in self._members]
        stopping = self._tolerance is not None      # (stacked_stopping)
        res = run_stack(
            x_all, bt, wt, False, plan,
            [(kw["alg_type"], float(kw["L2"]), kw["alpha"]) for kw in kws], iters, group,
            ops.pd_sweep_run, [0, iters] if points is None else points,
            observe=observe,
            tolerances=[self._tolerance] * len(kws) if stopping else None,
            check_every=self._check_every, start=x0)
        if res is not None and stopping:
            self._iterations_done = res.iterations_done
        return res

    _group = None

    def get_iterations_done(self):
        """Iterations every member did in the last run(): fewer than `iterations`
        where a tolerance stopped it (None before a run)."""
        if self._execution is None:
            return None
        if self._iterations_done is None:
            return [max(self._iterations, 0)] * len(self._members)
        return list(self._iterations_done)

    def get_group_size(self):
        """Members per stacked launch of the last run (None: sequential)."""
        return self._group if self._execution == "stacked" else None

    # ------------------------------------------------------------------
    def get_x_all_device(self):
        """(P, n) device tensor of all members' results in the caller's units."""
        import torch
        if self._x_all is not None:
            return ops.scale(self._x_all, self._x_scale).view(len(self._members), -1)
        if self._x_list is None:
            raise RuntimeError("run() first")
        return torch.stack(self._x_list)

    def get_x_device(self, m):
        if self._x_all is not None:
            n = self._n
            return ops.scale(self._x_all[m * n:(m + 1) * n], self._x_scale)
        if self._x_list is None:
            raise RuntimeError("run() first")
        return self._x_list[m].clone()

    def get_x(self, m):
        from .device import to_numpy
        return to_numpy(self.get_x_device(m))

    def get_observed_iterations(self):
        if not self._observers:
            return []
        pts = self._observers[0].get_observed_iterations()
        return pts if self._every is not None else pts[-1:]

    def get_measures(self):
        """{name: float64 array (members, observation points)}."""
        out = {}
        for name in self._functions:
            rows = np.array([np.asarray(obs.get_measures()[name], np.float64)
                             for obs in self._observers])
            out[name] = rows if self._every is not None else rows[:, -1:]
        return out

    def best(self, name, mode="max"):
        """(member index, its parameters) of the best final value of a measure."""
        if mode not in ("max", "min"):
            raise ValueError("mode must be 'max' or 'min'")
        last = self.get_measures()[name][:, -1]
        m = int(np.nanargmax(last) if mode == "max" else np.nanargmin(last))
        return m, dict(self._members[m])
