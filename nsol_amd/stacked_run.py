"""The group runner behind PrimalDualSweep's and PrimalDualBatch's stacked form: P
members of one shape advance together, ONE launch per iteration, in groups of at most
`group` members whose state (two xbar, two p) is allocated once.

A stacked caller supplies its operands and callbacks -- the stacked start vectors, the
scaled observations and weights with the way they are laid out (shared by the members
or one per member), its unweighted entry, observe(member, iteration) and an optional
hook for "the library has taken the stack" -- and run_stack owns the rest: the
members' schedules, the group loop with its views and start copy, the choice of entry
(ops.pd_weighted_run, the caller's unweighted entry, or stacked_stopping.run_group for
members that stop one by one), the slot rule and the decline contract.
"""
import numpy as np

from . import ops
from .primal_dual_solver import step_schedule
from .stacked_stopping import GroupResult, run_group
from .stopping import next_slot, stretch_bounds


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
    member-major) holds; x_all holds the results afterwards.  start: the n elements
    all of them start from, where they share them (x_all holds them P times).

    bt, wt (None: unweighted): n elements each shared by the members, or, strided,
    P * n with every member's own; plan: PrimalDualSolver.plan() of a member;
    members: [(alg_type, L2, alpha), ...]; entry: the unweighted launch,
    ops.pd_sweep_run's signature; bounds: the stretches without stopping ([0,
    iterations] or a device-mode observer's points); observe(m, it): called for member
    m after iteration `it` at the end of every stretch; taken(): called once, after
    the first launch the library accepted and before the first observe.
    tolerances[m] with check_every: the members stop one by one (run_group), in the
    stretches between the check points merged with the observer's.

    Returns a GroupResult (filled with tolerances only), or None when the library
    declined on the very first launch: nothing has been written or called then.  A
    decline on any later launch raises RuntimeError."""
    P = len(members)
    n, dim = x_all.numel() // P, plan["dim"]
    shape, w, gamma, flags = plan["shape"], plan["w"], plan["gamma"], plan["flags"]
    lmbda, sig, ta, th = member_schedules(members, iterations)
    xbar = [x_all.new_empty(group * n) for _ in range(2)]
    p = [x_all.new_empty(group * dim * n) for _ in range(2)]
    if tolerances is not None:
        bounds = stretch_bounds(iterations, check_every,
                                None if observe is None else bounds)
    res, first = GroupResult(0), True

    def accepted():
        nonlocal first
        if first:
            first = False
            if taken is not None:
                taken()

    def declined(name):
        if first:
            return None
        raise RuntimeError("nsol_%s declined in mid-run" % name)

    for a, b in ops.sweep_groups(P, group):
        g = b - a
        x = x_all[a * n:b * n]
        xb = [t[:g * n] for t in xbar]
        pp = [t[:g * dim * n] for t in p]
        if start is None:
            xb[0].copy_(x)
        else:
            xb[0].view(g, n).copy_(start)
        bt_g, wt_g = bt, wt
        if strided:
            bt_g, wt_g = bt[a * n:b * n], None if wt is None else wt[a * n:b * n]
        if tolerances is not None:
            def group_observe(m, it, a=a):
                accepted()
                observe(a + m, it)
            got = run_group(
                x, xb, pp, bt_g, wt_g, g, shape, w, ops.pd_weighted_table(
                    x, g, lmbda[a:b], sig[a:b], ta[a:b], th[a:b], True, gamma, flags),
                flags, tolerances[a:b], check_every, iterations, bounds,
                observe=None if observe is None else group_observe)
            if got is None:
                return declined("pd_stack_iter")
            if iterations > 0:      # (no iterations: nothing was launched)
                accepted()
            res.extend(got)
            continue
        k = 0
        for i0, i1 in zip(bounds[:-1], bounds[1:]):
            if wt is not None:
                slot = ops.pd_weighted_run(
                    xb[k], xb[1 - k], x, bt_g, wt_g, pp[k], pp[1 - k], g, shape, w,
                    lmbda[a:b], sig[a:b, i0:i1], ta[a:b, i0:i1], th[a:b, i0:i1], i0 == 0,
                    gamma, flags)
            else:
                slot = entry(
                    xb[k], xb[1 - k], x, bt_g, pp[k], pp[1 - k], g, shape, w, lmbda[a:b],
                    sig[a:b, i0:i1], ta[a:b, i0:i1], th[a:b, i0:i1], i0 == 0, gamma, flags)
            if slot is None:
                return declined("pd_weighted_run" if wt is not None else
                                getattr(entry, "__name__", "pd_run"))
            if first:
                accepted()
            k = next_slot(k, slot)
            if observe is not None:
                for m in range(a, b):
                    observe(m, i1)
    return res
