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
from .device import is_device_tensor, torch_dtype
from .observer import observation_points
from .primal_dual_solver import PrimalDualSolver
from .stacked_run import run_stack
from .stacked_stopping import StoppedRule


def _dev_index(v):
    return v.device.index if is_device_tensor(v) else None


def member_key(solver, plan):
    """What the members of one stack share, or None for a solver that runs on its
    own: (shape, w, dim, flags, gamma, dtype, iterations, observation points,
    device of the data, device of x0, device of the weights).  The flags carry
    ops.PD_DATA_WEIGHTED: a weighted and an unweighted solver never share a stack."""
    if plan is None:
        return None
    iters = int(solver._iterations)
    n = int(np.prod(plan["shape"]))
    if iters < 1 or n > ops.PD_BATCH_MAX_VOXELS or solver._verbose:
        return None
    if solver._tolerance is not None:
        return None         # its own stopping iteration: no stacked form
    points = None
    obs = solver._observer
    if obs is not None:
        if obs.get_keep_iterates():
            return None
        points = tuple(observation_points(iters, obs.get_every()))
    x0_dev = None if solver._x0_host is not None else _dev_index(solver._x0_dev)
    return (tuple(int(s) for s in plan["shape"]),
            tuple(float(v) for v in plan["w"]), int(plan["dim"]),
            int(plan["flags"]), float(plan["gamma"]), np.dtype(solver._dtype).name,
            iters, points, ("data", _dev_index(plan["data"])), ("x0", x0_dev),
            ("weights", _dev_index(plan.get("weights"))))


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

    def __init__(self, solvers, stacked_stopping=False):
        solvers = list(solvers)
        if not solvers:
            raise ValueError("a batch needs at least one solver")
        seen = set()
        for s in solvers:
            if not isinstance(s, PrimalDualSolver):
                raise ValueError("a batch takes PrimalDualSolver objects, not %s" %
                                 type(s).__name__)
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
        plans = [s.plan() for s in solvers]
        keys = [member_key(s, p) for s, p in zip(solvers, plans)]
        execution = ["sequential"] * len(solvers)
        self._stacks, self._group = [], None
        self._staging = []
        stacks = [(idx, False) for idx in plan_stacks(keys)]
        if self._stacked_stopping:
            stacks += [(idx, True) for idx in plan_stacks(
                [stopping_member_key(s, p) for s, p in zip(solvers, plans)])]
        for idx, stopping in stacks:
            t1 = time.time()
            x_all = self._run_stack(idx, plans, stopping)
            if x_all is None:
                continue                       # declined: nothing was written
            stopped = self._stopped
            torch.cuda.synchronize()
            ops.settle_persist_runs(synchronize=False)
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

    _stopped = None     # GroupResult of the last stack that ran with stopping=True

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

    def _run_stack(self, idx, plans, stopping=False):
        """The members `idx` in one launch per iteration and group.  Returns their
        stacked iterate (P * n, solver units), or None when the library declined
        on its first launch (nothing has been written to any solver then).
        stopping: the members have tolerances and stop one by one
        (stacked_stopping.run_group); self._stopped then holds what each did."""
        import torch
        from .device import device
        from .proximal_operators import scaled_data_on_device
        solvers = [self._solvers[i] for i in idx]
        plan = plans[idx[0]]
        P, iters, dim = len(idx), int(solvers[0]._iterations), plan["dim"]
        n = int(np.prod(plan["shape"]))
        td = torch_dtype(solvers[0]._dtype)
        dev = device()
        # ---- the scaled observations: float64 / x_scale, rounded once
        datas = [plans[i]["data"] for i in idx]
        if is_device_tensor(datas[0]):
            bt = torch.empty(P * n, dtype=td, device=dev)
            like = bt[:1]
            for m, i in enumerate(idx):
                bt[m * n:(m + 1) * n].copy_(scaled_data_on_device(
                    datas[m], plans[i]["data_scale"], like))
        else:
            raw = self._upload_rows(datas, np.float64)
            bt = ops.scale_rows(
                raw, self._scales([plans[i]["data_scale"] for i in idx]), P,
                divide=True, dtype=td).view(-1)
        # ---- the start vectors: rounded to the working dtype, then / x_scale
        if solvers[0]._x0_host is None:
            x_all = torch.empty(P * n, dtype=td, device=dev)
            for m, s in enumerate(solvers):
                x_all[m * n:(m + 1) * n].copy_(s._x0_device())
        else:
            raw = self._upload_rows([s._x0_host for s in solvers], solvers[0]._dtype)
            x_all = ops.scale_rows(raw, self._scales([s._x_scale for s in solvers]),
                                   P, divide=True).view(-1)
        # ---- a weighted data term: every member's own weights, checked by plan(),
        # converted to the working dtype and uploaded once like the observations
        wt = None
        if plan["flags"] & ops.PD_DATA_WEIGHTED:
            wts = [plans[i]["weights"] for i in idx]
            if is_device_tensor(wts[0]):
                wt = torch.empty(P * n, dtype=td, device=dev)
                for m, v in enumerate(wts):
                    wt[m * n:(m + 1) * n].copy_(v.reshape(-1))
            else:
                wt = self._upload_rows(wts, solvers[0]._dtype).view(-1)
            G = ops.weighted_batch_group_size(P, n, dim, x_all.element_size())
        else:
            G = ops.batch_group_size(P, n, dim, x_all.element_size())
        # ---- device-mode observers share their points (member_key): the run is
        # enqueued in the stretches between them
        obs = solvers[0]._observer
        bounds = [0, iters] if obs is None else \
            observation_points(iters, obs.get_every())

        def taken():
            # the library has taken the stack: the observation of the start
            # vectors, as Solver._observe_start makes it
            for s in solvers:
                s._x = None
                s._observe_start(iters)

        res = run_stack(
            x_all, bt, wt, True, plan, [(s._alg_type, s._L2, s._alpha) for s in solvers],
            iters, G, ops.pd_batch_run, bounds,
            observe=None if obs is None else (lambda m, it: solvers[m]._observe_at(
                it, x_all[m * n:(m + 1) * n])),
            taken=None if obs is None else taken,
            tolerances=[s._tolerance for s in solvers] if stopping else None,
            check_every=solvers[0]._check_every)
        if res is None:
            return None
        if stopping:
            self._stopped = res
        self._group = max(self._group or 0, G)
        return x_all

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
