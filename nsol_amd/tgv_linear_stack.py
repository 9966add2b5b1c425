"""Stacked forms of TGVPrimalDualLinearSolver -- TGV for blurred, thick-sliced, partly
missing data -- for the two jobs that are otherwise a Python loop of solvers:

    batch = TGVPrimalDualLinearBatch([TGVPrimalDualLinearSolver(...), ...])
    batch.run()                                  # the slices of a stack, small volumes
    x = batch.get_solvers()[3].get_x()           # as if that solver's run() had run
    w = batch.get_solvers()[3].get_w()

    sweep = TGVPrimalDualLinearSweep(A, A_adj, b, x0, dimension,
                                     parameters={"alpha": [...], "beta": [...]},
                                     iterations=200)
    sweep.set_measures({"PSNR": ...}, every=50)
    sweep.run()
    m, best = sweep.best("PSNR")

P members of one shape advance together in a host-driven loop of, per iteration,

    ops.tgv_stack_dual               every member's p and q, its own beta from a table
    the blur over the stack          ConvolutionOperator._apply_stacked, or the one-pass
                                     blur's epilogue r <- sigma A xbar + r per member
    ops.pdl_stack_dual_data          every member's r, its own lambda = 1 / alpha
    the adjoint blur over the stack
    ops.tgv_stack_primal_lin         every member's x, w and the bars; tau, theta and the
                                     box shared by value

in groups that keep the state under ops.TGV_STACK_GROUP_BYTES, without a read-back or a
synchronisation inside the loop.  The regulariser's side is tgv_stack.py's (k_tgv_dual_stack
and its table), the data term's linear_stack.py's (StackedDataSide); what joins them is
k_tgv_primal_lin_stack in nsol_tgv.hip.  A separable 1-D / 2-D blur runs in one launch per
pass over the whole stack: 7 launches per iteration for a stack of 2-D images instead of
7 P.  A 3-D blur runs member by member (2 P + 3 launches).  A sweep shares one scaled
observation, one set of weights and one start among its members; a batch uploads every
member's own together.  Every member's x and w are bit-identical to its own run().

Solvers form a stack when their A and A_adj are ConvolutionOperators and they agree in
what member_key() lists; alpha, beta, b, x0, x_scale and the weights may differ.
Everything else runs `solver.run()`, one after the other ("sequential"): a tolerance
(members do not stop one by one here), an observer that keeps iterates on the host, a
verbose solver, foreign or NumPy-only callables, a SampledConvolutionOperator pair (m != n,
which the stacked state does not hold), a stack of one, a geometry the library declines on
its first launch.

The two classes hold no front end of their own: they are solver_batch.PrimalDualBatch and
parameter_sweep.PrimalDualSweep with this solver's key, operands, group size and runner
(run_tgv_linear_stack, on stacked_run's decline contract).
"""
import numpy as np

from . import ops, tgv_numpy
from .device import device_index, is_device_tensor, to_numpy
from .linear_operators import ConvolutionOperator
from .linear_stack import (StackedDataSide, data_term_key, expects_epilogue,
                           operator_key)
from .parameter_sweep import PrimalDualSweep, member_parameters
from .solver_batch import PrimalDualBatch, plan_stacks, solver_key
from .stacked_run import Launches
from .tgv_stack import member_table_values
from .tgv_solver import TGVPrimalDualLinearSolver

SWEEP_KEYS = ("alpha", "beta")


def member_key(solver):
    """What the members of one stack share, or None for a solver that runs on its own:
    the operators (by value) and the shapes they are applied to, the volume's shape,
    spacing, dimension, isotropic, the data term (linear_stack.data_term_key: data_loss,
    with the KL term's scaled background), bounds, tau, sigma, theta, dtype, iteration
    count, a device-mode observer's points, whether the data term is weighted, and the
    devices of b, x0 and the weights."""
    if not isinstance(solver, TGVPrimalDualLinearSolver):
        return None
    op, op_adj = solver._op, solver._op_adj
    if not (isinstance(op, ConvolutionOperator) and
            isinstance(op_adj, ConvolutionOperator)):
        return None             # foreign or NumPy-only callables, other operators
    own = solver_key(solver)
    if own is None:
        return None             # (a tolerance, its own stopping iteration, among them)
    if solver._m != solver._n or solver._x0_ndim != 1:
        return None
    b = solver._b
    if int(b.numel() if is_device_tensor(b) else np.size(b)) != solver._m:
        return None             # (run() says what is wrong with it)
    w = solver._weights
    return (operator_key(op), tuple(solver._op_shape), operator_key(op_adj),
            tuple(solver._op_adj_shape), tuple(solver._shape),
            tuple(float(v) for v in solver._spacing), int(solver._dimension),
            bool(solver._isotropic), data_term_key(solver),
            tuple(float(v) for v in solver._bounds), float(solver._tau),
            float(solver._sigma), float(solver._theta)) + own[:3] + \
        (w is not None, ("b", device_index(b)), own[3], ("weights", device_index(w)))


def launches_per_iteration(solver, members):
    """(stacked, loop of solvers): kernel launches per iteration of `members` runs like
    `solver` -- the TGV dual step, the blur, the update of r, the adjoint blur, the
    primal step."""
    op, adj, P = solver._op, solver._op_adj, int(members)
    one = max(op._launches(solver._op_shape), 1) + \
        max(adj._launches(solver._op_adj_shape), 1) + 3
    return (op.stacked_launches(solver._op_shape, P) +
            adj.stacked_launches(solver._op_adj_shape, P) + 3, P * one)


def run_tgv_linear_stack(x_all, bt, wt, strided, template, alphas, betas, group, points,
                         observe=None, taken=None):
    """Advance the P = len(alphas) stacked runs whose start vectors x_all (P * n,
    member-major, solver units) holds; x_all holds the results afterwards.

    bt, wt (None: unweighted): n elements each shared by the members, or, strided,
    P * n with every member's own; template: a member, for everything the members share
    (member_key); alphas, betas: per member; group: members per launch; points: the
    iterations after which observe(m, it) is called for every member (None: never);
    taken(): called once, after the first launch the library accepted and before the
    first observe.

    Returns w_all (P * dimension * n, member-major, solver units), or None when the
    library declined the very first launch: x_all is as it was and nothing has been
    called.  A decline on any later launch raises RuntimeError."""
    import torch
    s = template
    P = len(alphas)
    n, d = x_all.numel() // P, s._dimension
    M = tgv_numpy.components(d)
    iters = int(s._iterations)
    shape, iw = s._shape, ops.inv_spacing(s._spacing, d)
    tau, sigma, theta = s._tau, s._sigma, s._theta
    dflags = ops.PD_REG_ISOTROPIC if s._isotropic else 0
    data_loss, bg = s._data_loss, s._scaled_background()
    lo, hi = s._bounds
    # (tl is unused by the kLin step; the table checks it as it checks beta)
    beta_all, tl_all = member_table_values(tau, alphas, betas)
    lm_all = ops.pdl_lambdas([1. / float(a) for a in alphas], x_all)
    points = set(points or ())
    w_all = x_all.new_zeros(P * d * n)
    # a group's xbar, wbar, p, q, r and g = A^T r, allocated once
    xbar_g, wbar_g = x_all.new_empty(group * n), x_all.new_empty(group * d * n)
    p_g, q_g = x_all.new_empty(group * d * n), x_all.new_empty(group * M * n)
    r_g, g_g = x_all.new_empty(group * n), x_all.new_empty(group * n)
    data = StackedDataSide(s, x_all, group, n)
    launches = Launches(taken)
    for a, b in ops.sweep_groups(P, group):
        g = b - a
        x, w = x_all[a * n:b * n], w_all[a * d * n:b * d * n]
        xbar, wbar = xbar_g[:g * n], wbar_g[:g * d * n]
        p, q = p_g[:g * d * n], q_g[:g * M * n]
        r, gq = r_g[:g * n], g_g[:g * n]
        bt_m, wt_m = bt, wt
        if strided:
            bt_m, wt_m = bt[a * n:b * n], None if wt is None else wt[a * n:b * n]
        tab = ops.tgv_stack_table(x_all, beta_all[a:b], tl_all[a:b])
        if tab is None:
            return launches.declined("tgv_stack_table")
        lm = lm_all[a:b]
        xbar.copy_(x)
        wbar.zero_()
        p.zero_()
        q.zero_()
        r.zero_()
        for i in range(iters):
            if not (ops.tgv_stack_dual(xbar, wbar, p, q, g, shape, iw, sigma, tab, dflags)
                    and data.dual_step(xbar, r, bt_m, wt_m, sigma, lm, g, data_loss, bg,
                                       gq)
                    and ops.tgv_stack_primal_lin(p, q, x, xbar, w, wbar, gq, g, shape, iw,
                                                 tau, theta, lo, hi)):
                return launches.declined("tgv_stack_primal_lin")
            launches.accepted()
            if observe is not None and (i + 1) in points:
                for m in range(a, b):
                    observe(m, i + 1)
        tab.record_stream(torch.cuda.current_stream())   # freed once the group is done
    return w_all


def _group_size(template, members, n, itemsize, own_data, own_weights):
    return ops.tgv_lin_stack_group_size(
        members, n, template._dimension, itemsize, own_data=own_data,
        own_weights=own_weights,
        with_t=not expects_epilogue(template._op, template._op_shape))


class TGVPrimalDualLinearBatch(PrimalDualBatch):
    """PrimalDualBatch's interface for TGVPrimalDualLinearSolver objects: its __init__,
    run() and upload, with this solver's key, operands and runner.  Every stacked member
    also answers get_w() as after its own run().  The members never stop one by one."""

    _solver_type = TGVPrimalDualLinearSolver
    _stops_members = False

    def _stacks_to_try(self):
        return [(idx, False) for idx in
                plan_stacks([member_key(s) for s in self._solvers])]

    def _after_wait(self):
        pass

    def _operands(self, idx):
        """What the members themselves hold; device-resident weights are checked and
        converted as the solver's own run() does it."""
        from .proximal_operators import weights_on_device
        solvers = [self._solvers[i] for i in idx]
        return [(s._b, s._x_scale) for s in solvers], \
            None if solvers[0]._weights is None else [s._weights for s in solvers], \
            weights_on_device

    def _advance(self, idx, x_all, bt, wt, points, observe, taken, stopping):
        solvers = [self._solvers[i] for i in idx]
        s0, P = solvers[0], len(solvers)
        n, d = x_all.numel() // P, s0._dimension
        G = _group_size(s0, P, n, x_all.element_size(), True, wt is not None)
        w_all = run_tgv_linear_stack(x_all, bt, wt, True, s0,
                                     [s._alpha for s in solvers],
                                     [s._beta for s in solvers], G, points,
                                     observe=observe, taken=taken)
        if w_all is None:
            return None
        for m, s in enumerate(solvers):
            s._w = w_all[m * d * n:(m + 1) * d * n]
        return G, None


class TGVPrimalDualLinearSweep(PrimalDualSweep):
    """PrimalDualSweep's interface for an (alpha, beta) sweep of TGVPrimalDualLinearSolver
    on one observation: TGVPrimalDualLinearSweep(A, A_adj, b, x0, dimension,
    parameters={"alpha": [...], "beta": [...]}, **solver_kwargs) with
    TGVPrimalDualLinearSolver's keyword arguments; the members are itertools.product over
    the lists in the dictionary's key order, and a parameter that is not swept keeps its
    keyword's value.  get_w(m) is member m's second primal variable.  A sweep with a
    `tolerance`, or one the library declines, runs its members one after the other
    through plain solvers."""

    def __init__(self, A, A_adj, b, x0, dimension, parameters, **solver_kwargs):
        members = member_parameters(parameters, keys=SWEEP_KEYS)
        kw = dict(solver_kwargs)
        self._defaults = dict(alpha=kw.pop("alpha", 0.01), beta=kw.pop("beta", 2.0))
        self._args = dict(A=A, A_adj=A_adj, b=b, x0=x0, dimension=dimension)
        self._kwargs = kw
        template = self._solver(members[0])          # the arguments' own refusals
        self._init_state(x0, members, template._iterations, template._tolerance,
                         template._check_every, False, template._x_scale,
                         template._dtype)
        self._w_all = self._w_list = None

    def _solver(self, member=None):
        kw = dict(self._defaults)
        kw.update(member or {})
        return TGVPrimalDualLinearSolver(alpha=kw["alpha"], beta=kw["beta"],
                                         **self._args, **self._kwargs)

    def run(self):
        self._w_all = self._w_list = None
        PrimalDualSweep.run(self)

    def _run_sequential(self):
        """One solver after the other; every member's w is kept beside its x."""
        self._x_list, self._observers = [], []
        self._iterations_done, self._w_list = [], []
        for member in self._members:
            solver = self._solver(member)
            obs = self._observer()
            if obs is not None:
                solver.set_observer(obs)
                self._observers.append(obs)
            solver.run()
            self._n = solver._x.numel()
            self._x_list.append(solver.get_x_device())
            self._w_list.append(solver.get_w())
            self._iterations_done.append(solver.get_iterations_done())

    def _stack_form(self, template):
        """The template itself, for everything the members share (member_key)."""
        return template if member_key(template) is not None else None

    def _after_wait(self):
        pass

    def _shared_operands(self, template, form, x0):
        from .proximal_operators import scaled_data_on_device, weights_on_device
        bt = scaled_data_on_device(template._b, template._x_scale, x0)
        wt = None if template._weights is None else \
            weights_on_device(template._weights, x0)
        return bt, wt, _group_size(template, len(self._members), x0.numel(),
                                   x0.element_size(), False, False)

    def _advance(self, template, form, x_all, bt, wt, group, points, observe, x0):
        kws = [dict(self._defaults, **member) for member in self._members]
        w_all = run_tgv_linear_stack(x_all, bt, wt, False, template,
                                     [kw["alpha"] for kw in kws],
                                     [kw["beta"] for kw in kws], group, points,
                                     observe=observe)
        if w_all is None:
            return None
        self._w_all = w_all
        return True

    def get_w(self, m):
        """Member m's second primal variable times x_scale, dimension * n values, as
        TGVPrimalDualLinearSolver.get_w() gives it."""
        if self._w_all is not None:
            dn = self._w_all.numel() // len(self._members)
            return to_numpy(ops.scale(self._w_all[m * dn:(m + 1) * dn], self._x_scale))
        if self._w_list is None:
            raise RuntimeError("run() first")
        return self._w_list[m].copy()
