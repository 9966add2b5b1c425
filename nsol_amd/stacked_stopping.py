"""Stacked primal-dual runs whose members stop one by one: what stacked_run.run_stack
runs a group through for PrimalDualBatch(stacked_stopping=True) and
PrimalDualSweep(stacked_stopping=True).

A group of g members (stacked images with their own data, or the members of a sweep
that share one observation) advances in ONE launch per iteration
(ops.pd_stack_iter, nsol_pdm.hip) over a device map of the members still running.
The iteration that ends in a check point (stopping.check_points) runs in
the checking form and leaves the four sums of every active member in a device board;
ONE read-back of that board per check is the only synchronisation.  The decision is
PrimalDualSolver's own (stopping.relative_changes / criterion_met), taken per member
with the member's tolerance; a member that has met it is dropped from the map (a small
int32 upload) and is never touched again -- x is updated in place, so its result
stays where it is and no array is re-laid.  The run ends as soon as the map is empty.

The xbar / p slot alternates in lockstep for all active members; a retired member
needs only its x.
"""
from . import ops
from .stopping import (check_points, criterion_met, relative_changes,
                       stretch_bounds)  # noqa: F401 (stretch_bounds: its former home)


class StackDevice(object):
    """What run_group needs from the device: the launch, the board of sums with its
    workspace, the upload of a map and the read-back of the board."""

    def __init__(self, like, shape, members):
        import torch
        if ops._pending_runs:
            ops.settle_persist_runs()   # an earlier persistent run may feed this one
        self._device = like.device
        self.ws = ops.pd_stack_workspace(like, shape, members)
        self.rows = torch.zeros(ops.PD_CHECK_SUMS * int(members), dtype=torch.float64,
                                device=like.device)

    iter = staticmethod(ops.pd_stack_iter)

    def upload_map(self, active):
        import torch
        return torch.tensor(list(active), dtype=torch.int32, device=self._device)

    def read_rows(self):
        """(members, 4) float64 on the host; this waits for the device."""
        return self.rows.cpu().numpy().reshape(-1, ops.PD_CHECK_SUMS)


class GroupResult(object):
    """Per member of a group: iterations done, 'tolerance' / 'iterations', and the
    rows (k, r_x, r_p) of its checks."""

    def __init__(self, members):
        self.iterations_done = [0] * members
        self.stop_reason = ["iterations"] * members
        self.changes = [[] for _ in range(members)]

    def extend(self, other):
        """The members of the next group behind these."""
        self.iterations_done += other.iterations_done
        self.stop_reason += other.stop_reason
        self.changes += other.changes


def run_group(x, xbar, p, bt, wt, members, shape, w, tab, flags, tolerances,
              check_every, iterations, bounds, observe=None, device=None):
    """Advance a group of `members` stacked runs for at most `iterations` iterations,
    every member until its own tolerance is met.

    x (members * n), xbar[2] and p[2]: the group's state, xbar[0] holding the start
    vectors; bt and wt (None: unweighted) of n elements (shared, stride 0) or
    members * n (every member its own, stride n); tab: ops.pd_weighted_table's table
    of all `iterations` for the `members` (p zero before the first);
    tolerances[m]: member m's; bounds: stretch_bounds(); observe(m, it): called after
    iteration bounds[j] for every member still running then, before the decision --
    a retired member is not observed again.  device: a StackDevice (the tests pass a
    fake).  Returns a GroupResult, or None when the library declined on its first
    launch (nothing has been written then)."""
    members = int(members)
    if device is None:
        device = StackDevice(x, shape, members)
    points = set(check_points(iterations, check_every))
    res = GroupResult(members)
    active = list(range(members))
    dev_map = device.upload_map(active)
    k, first = 0, True
    for a, b in zip(bounds[:-1], bounds[1:]):
        check = b in points
        for it in range(a, b):
            with_rows = check and it == b - 1
            took = device.iter(xbar[k], xbar[1 - k], x, bt, wt, p[k], p[1 - k], members,
                               dev_map, len(active), shape, w, tab, it, flags,
                               ws=device.ws if with_rows else None,
                               rows=device.rows if with_rows else None)
            if not took:
                if first:
                    return None
                raise RuntimeError("nsol_pd_stack_iter declined in mid-run")
            first = False
            k = 1 - k
        for m in active:
            res.iterations_done[m] = b
            if observe is not None:
                observe(m, b)
        if not check:
            continue
        sums = device.read_rows()       # the one synchronisation of this check
        keep = []
        for m in active:
            r_x, r_p = relative_changes(sums[m])
            res.changes[m].append((float(b), r_x, r_p))
            if criterion_met(r_x, r_p, tolerances[m]):
                res.stop_reason[m] = "tolerance"
            else:
                keep.append(m)
        if len(keep) != len(active):
            active = keep
            if not active:
                break
            dev_map = device.upload_map(active)
    return res


class StoppedRule(object):
    """What PrimalDualSolver.get_changes() reads after a stacked run."""

    def __init__(self, tolerance, rows):
        self.tolerance = float(tolerance)
        self.rows = list(rows)
