"""What every stacked primal-dual run shares -- PrimalDualSweep's and PrimalDualBatch's
(run_stack, below) and PrimalDualLinearSolver's (linear_stack.run_linear_stack): P
members of one shape advance together in groups of at most `group` members.

    stack_groups    the group loop: the state of a group (two xbar, two p) allocated
                    once, every group's views of it, the copy of the start vectors and
                    the slices of operands that every member brings its own of
    Launches        the decline contract: the library may decline the very first launch
                    of a run (nothing has been written or called then), never a later one

A stacked caller supplies its operands and callbacks -- the stacked start vectors, the
scaled observations and weights with the way they are laid out (shared by the members
or one per member), its unweighted entry, observe(member, iteration) and an optional
hook for "the library has taken the stack" -- and run_stack owns the rest: the
members' schedules, the choice of entry (ops.pd_weighted_run, the caller's unweighted
entry, or stacked_stopping.run_group for members that stop one by one) and the slot
rule.
"""
import collections

import numpy as np

from . import ops
from .primal_dual_solver import step_schedule
from .stacked_stopping import GroupResult, run_group
from .stopping import next_slot, stretch_bounds

# The members [a, b) of a stack and the views their launches take: x (their part of the
# stacked iterate), xbar[2] and p[2] (the group's state, xbar[0] holding the start
# vectors), bt and wt (the whole shared operand, or the members' own part of it)
Group = collections.namedtuple("Group", "a b x xbar p bt wt")


def stack_groups(x_all, bt, wt, strided, members, dim, group, start=None):
    """The groups of a stacked run, one Group after the other: every member once, in
    order, `group` at a time (ops.sweep_groups; the last group may be smaller).

    x_all: the members' start vectors (members * n, member-major); bt, wt (None:
    unweighted): n elements each shared by the members, or, strided, members * n with
    every member's own; start: the n elements all members start from, where they share
    them (x_all holds them `members` times).  The two xbar and the two p (dim parts
    each) are allocated once, for `group` members, before the first group."""
    n = x_all.numel() // members
    xbar = [x_all.new_empty(group * n) for _ in range(2)]
    p = [x_all.new_empty(group * dim * n) for _ in range(2)]
    for a, b in ops.sweep_groups(members, group):
        g = b - a
        x = x_all[a * n:b * n]
        xb = [t[:g * n] for t in xbar]
        if start is None:
            xb[0].copy_(x)
        else:
            xb[0].view(g, n).copy_(start)
        bt_g, wt_g = bt, wt
        if strided:
            bt_g, wt_g = bt[a * n:b * n], None if wt is None else wt[a * n:b * n]
        yield Group(a, b, x, xb, [t[:g * dim * n] for t in p], bt_g, wt_g)


class Launches(object):
    """The decline contract of a stacked run.  The runner calls accepted() after every
    launch the library took: the first time, taken() is called (once, before the
    first observe).  Where the library declined a launch, the runner returns
    declined(entry): None on the very first launch -- nothing has been written or
    called, the caller runs its members one after the other -- and RuntimeError naming
    the entry on any later one."""

    def __init__(self, taken=None):
        self._first, self._taken = True, taken

    def accepted(self):
        if self._first:
            self._first = False
            if self._taken is not None:
                self._taken()

    def declined(self, entry):
        if self._first:
            return None
        raise RuntimeError("nsol_%s declined in mid-run" % entry)


def member_schedules(members, iterations):
    """lmbda (P,) and sigma, tau, theta (P, iterations) of the members
    [(alg_type, L2, alpha), ...]."""
    P = len(members)
    lmbda = np.empty(P)
    sig, ta, th = (np.empty((P, iterations)) for _ in range(3))
    for m, (alg_type, L2, alpha) in enumerate(members):
        lmbda[m] = 1. / float(alpha)
        sig[m], ta[m], th[m] = step_schedule(alg_type, L2, lmbda[m], iterations)
    return lmbda, sig, ta, th


def run_stack(x_all, bt, wt, strided, plan, members, iterations, group, entry, bounds,
              observe=None, taken=None, tolerances=None, check_every=None, start=None):
    """Advance the P = len(members) stacked runs whose start vectors x_all (P * n,
    member-major) holds, ONE launch per iteration and group; x_all holds the results
    afterwards.  x_all, bt, wt, strided, group and start: as stack_groups takes them.

    plan: PrimalDualSolver.plan() of a member; members: [(alg_type, L2, alpha), ...];
    entry: the unweighted launch, ops.pd_sweep_run's signature; bounds: the stretches
    without stopping ([0, iterations] or a device-mode observer's points);
    observe(m, it): called for member m after iteration `it` at the end of every
    stretch; taken(): called once, after the first launch the library accepted and
    before the first observe.  tolerances[m] with check_every: the members stop one by
    one (run_group), in the stretches between the check points merged with the
    observer's.

    Returns a GroupResult (filled with tolerances only), or None when the library
    declined on the very first launch: nothing has been written or called then.  A
    decline on any later launch raises RuntimeError (Launches)."""
    P = len(members)
    shape, w, gamma, flags = plan["shape"], plan["w"], plan["gamma"], plan["flags"]
    lmbda, sig, ta, th = member_schedules(members, iterations)
    if tolerances is not None:
        bounds = stretch_bounds(iterations, check_every,
                                None if observe is None else bounds)
    res, launches = GroupResult(0), Launches(taken)
    for grp in stack_groups(x_all, bt, wt, strided, P, plan["dim"], group, start):
        a, b, x, xb, pp = grp[:5]
        g = b - a
        if tolerances is not None:
            def group_observe(m, it, a=a):
                launches.accepted()
                observe(a + m, it)
            got = run_group(
                x, xb, pp, grp.bt, grp.wt, g, shape, w, ops.pd_weighted_table(
                    x, g, lmbda[a:b], sig[a:b], ta[a:b], th[a:b], True, gamma, flags),
                flags, tolerances[a:b], check_every, iterations, bounds,
                observe=None if observe is None else group_observe)
            if got is None:
                return launches.declined("pd_stack_iter")
            if iterations > 0:      # (no iterations: nothing was launched)
                launches.accepted()
            res.extend(got)
            continue
        k = 0
        for i0, i1 in zip(bounds[:-1], bounds[1:]):
            if wt is not None:
                slot = ops.pd_weighted_run(
                    xb[k], xb[1 - k], x, grp.bt, grp.wt, pp[k], pp[1 - k], g, shape, w,
                    lmbda[a:b], sig[a:b, i0:i1], ta[a:b, i0:i1], th[a:b, i0:i1], i0 == 0,
                    gamma, flags)
            else:
                slot = entry(
                    xb[k], xb[1 - k], x, grp.bt, pp[k], pp[1 - k], g, shape, w, lmbda[a:b],
                    sig[a:b, i0:i1], ta[a:b, i0:i1], th[a:b, i0:i1], i0 == 0, gamma, flags)
            if slot is None:
                return launches.declined("pd_weighted_run" if wt is not None else
                                         getattr(entry, "__name__", "pd_run"))
            launches.accepted()
            k = next_slot(k, slot)
            if observe is not None:
                for m in range(a, b):
                    observe(m, i1)
    return res
