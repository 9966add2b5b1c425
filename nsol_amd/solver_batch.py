"""Many independent primal-dual problems of one shape in stacked device launches:
the slices of a stack denoised slice by slice, a batch of 2-D images, a set of small
volumes -- the job that is otherwise a Python loop of PrimalDualSolver objects.

    solvers = [PrimalDualSolver(...), ...]       # configured exactly as today
    batch = PrimalDualBatch(solvers)
    batch.run()
    x = solvers[3].get_x()                       # as if solvers[3].run() had run
    X = batch.get_x_all_device()                 # (P, n), callers' units

Solvers whose plans (PrimalDualSolver.plan()) agree in shape, inverse spacings,
dimension, flags, Huber gamma, dtype, device, iteration count and observation
points form a STACK: their observations and start vectors are uploaded together
(one page-locked (P, n) array each), scaled by every member's own x_scale in one
launch each (ops.scale_rows) and advanced together, ONE launch per iteration
(nsol_pd_batch_run_*; with a weighted data term nsol_pd_weighted_run_*, every
member bringing its own weights), in groups that keep the state under
ops.PD_BATCH_GROUP_BYTES.  The data, x_scale, alpha, alg_type and L2 may differ
from member to member.  Every member's result is bit-identical to its own run().

Everything else runs `solver.run()`, one after the other ("sequential"): a plan
that is None (foreign callables, deconvolution), a solver with a tolerance (it stops
at an iteration of its own), a stack of one, members above
ops.PD_BATCH_MAX_VOXELS, a geometry the library declines on its first launch, an
observer that keeps iterates on the host, a verbose solver.

PrimalDualBatch(solvers, stacked_stopping=True) also stacks the solvers that have a
tolerance, among themselves: members that agree in stopping_member_key() -- the
fields above and check_every; the tolerance may differ -- advance in one launch per
iteration over a device map of the members still running, and every member leaves
the map at the check that meets its own tolerance (nsol_amd/stacked_stopping.py,
nsol_pdm.hip).  Every member then answers get_x(), get_iterations_done(),
get_stop_reason() and get_changes() as after its own run().  The default is off.
"""
import datetime
import time

import numpy as np

from . import ops
from .device import device_index, is_device_tensor, torch_dtype
from .observer import observation_points
from .primal_dual_solver import PrimalDualSolver
from .stacked_run import run_stack
from .stacked_stopping import StoppedRule


def solver_key(solver):
    """The solver's own part of a stack key, whatever kind of solver it is: (dtype,
    iterations, a device-mode observer's points, ("x0", the device of x0)), or None for
    a solver that runs on its own: no iterations, verbose, a tolerance (its own stopping
    iteration: no stacked form), an observer that keeps iterates."""
    iters = int(solver._iterations)
    if iters < 1 or solver._verbose or solver._tolerance is not None:
        return None
    points = None
    obs = solver._observer
    if obs is not None:
        if obs.get_keep_iterates():
            return None
        points = tuple(observation_points(iters, obs.get_every()))
    x0_dev = None if solver._x0_host is not None else device_index(solver._x0_dev)
    return np.dtype(solver._dtype).name, iters, points, ("x0", x0_dev)


def member_key(solver, plan):
    """What the members of one stack share, or None for a solver that runs on its
    own: (shape, w, dim, flags, gamma, dtype, iterations, observation points,
    device of the data, device of x0, device of the weights).  The flags carry
    ops.PD_DATA_WEIGHTED: a weighted and an unweighted solver never share a stack."""
    if plan is None:
        return None
    own = solver_key(solver)
    if own is None or int(np.prod(plan["shape"])) > ops.PD_BATCH_MAX_VOXELS:
        return None
    return (tuple(int(s) for s in plan["shape"]),
            tuple(float(v) for v in plan["w"]), int(plan["dim"]),
            int(plan["flags"]), float(plan["gamma"])) + own[:3] + \
        (("data", device_index(plan["data"])), own[3],
         ("weights", device_index(plan.get("weights"))))


class _WithoutTolerance(object):
    """A solver as member_key() would see it without its tolerance."""
    _tolerance = None

    def __init__(self, solver):
        self._solver = solver

    def __getattr__(self, name):
        return getattr(self._solver, name)


def stopping_member_key(solver, plan):
    """What the members of one stack WITH per-member stopping share, or None:
    member_key's fields and check_every.  The tolerance itself may differ from
    member to member; a solver without one never has this key, so it never shares a
    stack with one that stops."""
    if solver._tolerance is None:
        return None
    key = member_key(_WithoutTolerance(solver), plan)
    if key is None:
        return None
    return key + (("check_every", int(solver._check_every)),)


def plan_stacks(keys):
    """[[member index, ...], ...]: the stacks of two or more members with equal
    keys, in order of their first member; every other index runs sequentially."""
    by_key = {}
    for i, k in enumerate(keys):
        if k is not None:
            by_key.setdefault(k, []).append(i)
    return [idx for idx in by_key.values() if len(idx) > 1]


class PrimalDualBatch(object):
    """The stacked front end of a list of solvers, and its form for PrimalDualSolver.
    __init__, run() and the upload of a stack's operands are the same for every kind
    of solver; a subclass (linear_stack.PrimalDualLinearBatch) replaces what is not:

        _solver_type        the solvers the batch takes
        _stops_members      whether stacked_stopping=True is on offer
        _stacks_to_try()    [(member indices, stopping), ...]
        _after_wait()       what follows the synchronisation behind a stack
        _operands(idx)      where a stack's observations and weights come from
        _advance(...)       the group size and the runner"""

    _solver_type = PrimalDualSolver
    _stops_members = True

    def __init__(self, solvers, stacked_stopping=False):
        solvers = list(solvers)
        if not solvers:
            raise ValueError("a batch needs at least one solver")
        if stacked_stopping and not self._stops_members:
            raise ValueError("%s has no stacked stopping" % type(self).__name__)
        seen = set()
        for s in solvers:
            if not isinstance(s, self._solver_type):
                raise ValueError("a batch takes %s objects, not %s" %
                                 (self._solver_type.__name__, type(s).__name__))
            if id(s) in seen:
                raise ValueError("the same solver object is in the batch twice")
            seen.add(id(s))
            if s._x0_ndim != 1:
                raise ValueError("Initial value x0 must be a 1D array")
        self._solvers = solvers
        # True: solvers with a tolerance stack among themselves and stop one by one
        self._stacked_stopping = bool(stacked_stopping)
        self._execution = None
        self._group = None
        self._stacks = []           # (member indices, (P * n) iterate, solver units)
        self._computational_time = datetime.timedelta(seconds=0)

    # ------------------------------------------------------------------
    def get_solvers(self):
        return list(self._solvers)

    def get_execution(self):
        """One of 'stacked' / 'sequential' per solver after run() (None before)."""
        return None if self._execution is None else list(self._execution)

    def get_group_size(self):
        """Members per stacked launch of the last run's largest stack (None: no
        stack ran)."""
        return self._group

    def get_computational_time(self):
        return self._computational_time

    # ------------------------------------------------------------------
    def run(self):
        import torch
        t0 = time.time()
        solvers = self._solvers
        for s in solvers:
            if s._x0_ndim != 1:
                raise ValueError("Initial value x0 must be a 1D array")
        execution = ["sequential"] * len(solvers)
        self._stacks, self._group = [], None
        self._staging = []
        for idx, stopping in self._stacks_to_try():
            t1 = time.time()
            ran = self._run_stack(idx, stopping)
            if ran is None:
                continue                       # declined: nothing was written
            x_all, stopped = ran
            torch.cuda.synchronize()
            self._after_wait()
            took = datetime.timedelta(seconds=time.time() - t1)
            n = x_all.numel() // len(idx)
            for m, i in enumerate(idx):
                s = solvers[i]
                s._x = x_all[m * n:(m + 1) * n]
                s._execution = "fused"
                s._iterations_done, s._stop_reason = int(s._iterations), "iterations"
                s._rule = None
                if stopping:
                    s._iterations_done = stopped.iterations_done[m]
                    s._stop_reason = stopped.stop_reason[m]
                    s._rule = StoppedRule(s._tolerance, stopped.changes[m])
                s._computational_time = took
                if s._observer is not None:
                    s._observer._finish()
                    s._observer.set_computational_time(took)
                execution[i] = "stacked"
            self._stacks.append((list(idx), x_all))
        del self._staging
        for i, s in enumerate(solvers):
            if execution[i] == "sequential":
                s.run()
        self._execution = execution
        self._computational_time = datetime.timedelta(seconds=time.time() - t0)

    def _stacks_to_try(self):
        """[(member indices, stopping), ...] of this run: the solvers that agree in
        member_key(), and with stacked_stopping those that agree in
        stopping_member_key() and stop one by one."""
        solvers = self._solvers
        self._plans = plans = [s.plan() for s in solvers]
        stacks = [(idx, False) for idx in plan_stacks(
            [member_key(s, p) for s, p in zip(solvers, plans)])]
        if self._stacked_stopping:
            stacks += [(idx, True) for idx in plan_stacks(
                [stopping_member_key(s, p) for s, p in zip(solvers, plans)])]
        return stacks

    def _after_wait(self):
        ops.settle_persist_runs(synchronize=False)

    def _upload_rows(self, rows, dtype):
        """One page-locked (P, n) array of `dtype`, filled row by row (NumPy casts
        as to_device does) and sent in one copy."""
        import torch
        from .device import device
        P, n = len(rows), int(np.size(rows[0]))
        host = torch.empty((P, n), dtype=torch_dtype(dtype), pin_memory=True)
        view = host.numpy()
        for m, r in enumerate(rows):
            np.copyto(view[m], np.asarray(r).reshape(-1), casting="unsafe")
        self._staging.append(host)       # alive until the run has synchronised
        return host.to(device(), non_blocking=True)

    def _scales(self, values):
        import torch
        from .device import device
        return torch.from_numpy(np.asarray(values, dtype=np.float64)).to(device())

    def _upload_stack(self, solvers, data, weights, device_weights):
        """(bt, x_all, wt) of the stack `solvers`: the scaled observations, the start
        vectors and the weights (None: unweighted), P * n elements each, member-major,
        in the working dtype.

        data: (observation, its scale) per member; weights: every member's own, or
        None; device_weights(w, like): a member's device-resident weights as the flat
        tensor that is copied into its row, `like` having the working dtype.  Where
        the first member's input lives decides the path (the members agree in it,
        member_key): host arrays travel together, one page-locked (P, n) array each
        (_upload_rows, kept in self._staging until run() has synchronised), and are
        scaled by every member's own scale in one launch (ops.scale_rows);
        device-resident inputs are converted and copied member by member."""
        import torch
        from .device import device
        from .proximal_operators import scaled_data_on_device
        s0 = solvers[0]
        P, td, dev = len(solvers), torch_dtype(s0._dtype), device()
        n = int(s0._x0_host.size if s0._x0_host is not None else s0._x0_dev.numel())

        def member_by_member(parts):
            out = torch.empty(P * n, dtype=td, device=dev)
            for m, part in enumerate(parts(out[:1])):
                out[m * n:(m + 1) * n].copy_(part)
            return out

        # ---- the scaled observations: float64 / scale, rounded once
        if is_device_tensor(data[0][0]):
            bt = member_by_member(lambda like: (scaled_data_on_device(d, scale, like)
                                                for d, scale in data))
        else:
            raw = self._upload_rows([d for d, _ in data], np.float64)
            bt = ops.scale_rows(raw, self._scales([scale for _, scale in data]), P,
                                divide=True, dtype=td).view(-1)
        # ---- the start vectors: rounded to the working dtype, then / x_scale
        if s0._x0_host is None:
            x_all = member_by_member(lambda like: (s._x0_device() for s in solvers))
        else:
            raw = self._upload_rows([s._x0_host for s in solvers], s0._dtype)
            x_all = ops.scale_rows(raw, self._scales([s._x_scale for s in solvers]),
                                   P, divide=True).view(-1)
        # ---- every member's own weights, converted to the working dtype
        wt = None
        if weights is not None:
            if is_device_tensor(weights[0]):
                wt = member_by_member(lambda like: (device_weights(w, like)
                                                    for w in weights))
            else:
                wt = self._upload_rows(weights, s0._dtype).view(-1)
        return bt, x_all, wt

    def _run_stack(self, idx, stopping=False):
        """The members `idx` together.  Returns (their stacked iterate (P * n, solver
        units), the runner's result), or None when the library declined on its first
        launch (nothing has been written to any solver then).  stopping: the members
        have tolerances and stop one by one; the result then holds what each did."""
        solvers = [self._solvers[i] for i in idx]
        iters = int(solvers[0]._iterations)
        bt, x_all, wt = self._upload_stack(solvers, *self._operands(idx))
        n = x_all.numel() // len(idx)
        # ---- device-mode observers share their points (member_key)
        obs = solvers[0]._observer
        points = None if obs is None else observation_points(iters, obs.get_every())

        def taken():
            # the library has taken the stack: the observation of the start
            # vectors, as Solver._observe_start makes it
            for s in solvers:
                s._x = None
                s._observe_start(iters)

        got = self._advance(
            idx, x_all, bt, wt, points,
            None if obs is None else (lambda m, it: solvers[m]._observe_at(
                it, x_all[m * n:(m + 1) * n])),
            None if obs is None else taken, stopping)
        if got is None:
            return None
        self._group = max(self._group or 0, got[0])
        return x_all, got[1]

    def _operands(self, idx):
        """(data, weights, device_weights) of the stack `idx` for _upload_stack: what
        the members' plans hold.  plan() has checked the weights; a device-resident
        member's are converted by the copy into its row."""
        plans = [self._plans[i] for i in idx]
        weighted = plans[0]["flags"] & ops.PD_DATA_WEIGHTED
        return [(p["data"], p["data_scale"]) for p in plans], \
            [p["weights"] for p in plans] if weighted else None, \
            lambda w, like: w.reshape(-1)

    def _advance(self, idx, x_all, bt, wt, points, observe, taken, stopping):
        """Run the stack `idx` in one launch per iteration and group
        (stacked_run.run_stack, in the stretches between the observers' points;
        stopping: stacked_stopping.run_group).  Returns (members per group, the
        runner's result), or None when the library declined."""
        solvers, plan = [self._solvers[i] for i in idx], self._plans[idx[0]]
        P, iters = len(solvers), int(solvers[0]._iterations)
        size = ops.batch_group_size if wt is None else ops.weighted_batch_group_size
        G = size(P, x_all.numel() // P, plan["dim"], x_all.element_size())
        res = run_stack(
            x_all, bt, wt, True, plan, [(s._alg_type, s._L2, s._alpha) for s in solvers],
            iters, G, ops.pd_batch_run, [0, iters] if points is None else points,
            observe=observe, taken=taken,
            tolerances=[s._tolerance for s in solvers] if stopping else None,
            check_every=solvers[0]._check_every)
        return None if res is None else (G, res)

    # ------------------------------------------------------------------
    def get_x_device(self, i):
        return self._solvers[i].get_x_device()

    def get_x(self, i):
        return self._solvers[i].get_x()

    def get_x_all_device(self):
        """(P, n) device tensor of every solver's result in its caller's units; one
        ops.scale_rows when the whole list ran as one stack."""
        import torch
        if self._execution is None:
            raise RuntimeError("run() first")
        solvers = self._solvers
        if len(self._stacks) == 1 and len(self._stacks[0][0]) == len(solvers):
            idx, x_all = self._stacks[0]
            s = self._scales([solvers[i]._x_scale for i in idx])
            return ops.scale_rows(x_all, s, len(idx)).view(len(idx), -1)
        rows = [s.get_x_device() for s in solvers]
        if len(set(r.numel() for r in rows)) != 1:
            raise ValueError("the solvers' results differ in length")
        return torch.stack(rows)
