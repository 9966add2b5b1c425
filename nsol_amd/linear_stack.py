"""Stacked forms of PrimalDualLinearSolver -- deconvolution with masks, weights, the l1
data term and an exact box -- for the two jobs that are otherwise a Python loop of
solvers:

    batch = PrimalDualLinearBatch([PrimalDualLinearSolver(...), ...])
    batch.run()                                  # a stack of images / small volumes
    x = batch.get_solvers()[3].get_x()           # as if that solver's run() had run

    sweep = PrimalDualLinearSweep(A, A_adj, b, x0, dimension,
                                  parameters={"alpha": [...]}, iterations=200)
    sweep.set_measures({"PSNR": ...}, every=50)
    sweep.run()
    m, best = sweep.best("PSNR")

P members of one shape advance together in a host-driven loop of, per iteration,

    the blur over the stack          ConvolutionOperator._apply_stacked, or the one-pass
                                     blur's epilogue q <- sigma A xbar + q per member
    ops.pdl_stack_dual_data          every member's q, its own lambda = 1 / alpha
                                     (data_loss="kl": ops.pdl_stack_dual_data_kl)
    the adjoint blur over the stack
    ops.pdl_stack_iter               the regulariser's dual update and the primal step

(nsol_pdls.hip) in groups that keep the state under ops.PDL_STACK_GROUP_BYTES, without
a read-back or a synchronisation inside the loop.  A separable 1-D / 2-D blur runs in
one launch per pass over the whole stack: 6 launches per iteration for a stack of 2-D
images instead of 6 P.  A 3-D blur runs member by member (2 P + 2 launches).  A sweep
shares one scaled observation, one set of weights and one start among its members; a
batch uploads every member's own together (one page-locked (P, n) array each, scaled by
every member's x_scale in one launch).  Every member's result is bit-identical to its
own run().

Solvers form a stack when they are `fused`, their A and A_adj are ConvolutionOperators
with equal taps, mode and dimension, and they agree in what member_key() lists; alpha,
b, x0, x_scale and the weights may differ.  Everything else runs `solver.run()`, one
after the other ("sequential"): a tolerance (members do not stop one by one here), an
observer that keeps iterates on the host, foreign callables, a verbose solver, a stack
of one, a geometry the library declines on its first launch, and every other operator
of the package -- a SampledConvolutionOperator pair keeps b and q on the coarse grid
and x on the fine one (m != n), which the stacked state does not hold.

The two classes hold no front end of their own: they are solver_batch.PrimalDualBatch and
parameter_sweep.PrimalDualSweep with this solver's key, operands, group size and runner
(run_linear_stack, on stacked_run's group loop and decline contract).
"""
import numpy as np

from . import linear_operators, ops
from .device import device_index, is_device_tensor
from .linear_operators import ConvolutionOperator
from .parameter_sweep import PrimalDualSweep, member_parameters
from .primal_dual_linear_solver import PrimalDualLinearSolver
from .solver_batch import PrimalDualBatch, plan_stacks, solver_key
from .stacked_run import Launches, stack_groups

SWEEP_KEYS = ("alpha",)


def operators_equal(a, b):
    """Two ConvolutionOperators that compute the same thing: the same object, or equal
    dimension, mode and taps (np.array_equal)."""
    if a is b:
        return True
    return isinstance(a, ConvolutionOperator) and isinstance(b, ConvolutionOperator) \
        and a.dimension == b.dimension and a.mode == b.mode and \
        a.kernel.shape == b.kernel.shape and np.array_equal(a.kernel, b.kernel)


def operator_key(op):
    """A hashable stand-in for operators_equal: dimension, mode and the taps by value."""
    return (int(op.dimension), op.mode, tuple(op.kernel.shape), op.kernel.tobytes())


def data_term_key(solver):
    """The data term's entry of a member key: data_loss itself, and for the KL term the
    pair of it and the background as the kernel sees it (background / x_scale, one value
    for the whole stack)."""
    if solver._data_loss == "kl":
        return ("kl", float(solver._scaled_background()))
    return solver._data_loss


def member_key(solver):
    """What the members of one stack share, or None for a solver that runs on its own:
    the operators (by value) and the shapes they are applied to, the volume's shape,
    spacing, dimension, reg_type, huber_gamma, isotropic, the data term (data_term_key:
    data_loss, with the KL term's scaled background), bounds, tau, sigma, dtype, iteration
    count, a device-mode observer's points, whether the data term is weighted, and the
    devices of b, x0 and the weights."""
    if not isinstance(solver, PrimalDualLinearSolver):
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
            solver._reg_type, float(solver._huber_gamma), bool(solver._isotropic),
            data_term_key(solver),
            tuple(float(v) for v in solver._bounds),
            float(solver._tau), float(solver._sigma)) + own[:3] + \
        (w is not None, ("b", device_index(b)), own[3], ("weights", device_index(w)))


def expects_epilogue(op, shape):
    """Whether the one-pass blur's epilogue is what a run on `shape` tries first."""
    return bool(linear_operators.USE_FUSED_BLUR3 and linear_operators.USE_BLUR_EPILOGUE
                and op._passes and len(shape) == 3 and op._fusable3())


def launches_per_iteration(solver, members):
    """(stacked, loop of solvers): kernel launches per iteration of `members` runs like
    `solver` -- the blur, the update of q, the adjoint blur, the tile."""
    op, adj, P = solver._op, solver._op_adj, int(members)
    one = max(op._launches(solver._op_shape), 1) + \
        max(adj._launches(solver._op_adj_shape), 1) + 2
    return (op.stacked_launches(solver._op_shape, P) +
            adj.stacked_launches(solver._op_adj_shape, P) + 2, P * one)


class StackedDataSide(object):
    """The data term's side of one stacked run (run_linear_stack below,
    tgv_linear_stack.run_tgv_linear_stack): the blur over the stack -- as the epilogue
    q <- sigma A xbar + q of the one-pass blur while it applies, else into t = A xbar,
    allocated when first needed -- every member's update of q and g = A^T q.  The
    template supplies the operators; `like` the element type, the device and, with
    `group`, the size of t and of the epilogue's slots."""

    def __init__(self, template, like, group, n):
        import torch
        s = template
        self._op, self._op_shape = s._op, s._op_shape
        self._adj, self._adj_shape = s._op_adj, s._op_adj_shape
        self._like, self._size = like, group * n
        self._t_all = None
        # q <- sigma A xbar + q as the epilogue of the one-pass blur, while it applies
        self._epilogue = bool(linear_operators.USE_BLUR_EPILOGUE)
        self._slots = torch.empty(group, dtype=torch.float64, device=like.device) \
            if self._epilogue else None

    def dual_step(self, xbar, q, bt, wt, sigma, lm, g, data_loss, background, out):
        """q (g members) in place, then out <- A^T q; background: the scaled one of the
        KL data term.  False when the library declined the update of q: the adjoint has
        not run then."""
        n = q.numel() // g
        if data_loss == "kl":
            def update(t):
                return ops.pdl_stack_dual_data_kl(q, t, bt, wt, sigma, lm, g, background)
        else:
            l1 = data_loss == "ell1"

            def update(t):
                return ops.pdl_stack_dual_data(q, t, bt, wt, sigma, lm, g, l1)
        if self._epilogue and self._op.apply_axpby_stacked(
                xbar, q, self._op_shape, g, sigma, 1., results=self._slots[:g]) is None:
            self._epilogue = False     # the kernel declined: nothing ran, q is intact
        if self._epilogue:
            ok = update(None)
        else:
            if self._t_all is None:
                self._t_all = self._like.new_empty(self._size)
            t = self._op._apply_stacked(xbar, self._op_shape, g, out=self._t_all[:g * n])
            ok = update(t)
        if ok:
            self._adj._apply_stacked(q, self._adj_shape, g, out=out)
        return ok


def run_linear_stack(x_all, bt, wt, strided, template, lmbda, group, points,
                     observe=None, taken=None, start=None):
    """Advance the P = len(lmbda) stacked runs whose start vectors x_all (P * n,
    member-major, solver units) holds; x_all holds the results afterwards.

    bt, wt (None: unweighted): n elements each shared by the members, or, strided,
    P * n with every member's own; template: a member, for everything the members
    share (member_key); lmbda: 1 / alpha per member; group: members per launch;
    points: the iterations after which observe(m, it) is called for every member
    (None: never); taken(): called once, after the first launch of the tile kernel
    and before the first observe; start: the n elements all members start from, where
    they share them (x_all holds them P times).

    Returns True, or None when the library declined the tile kernel's very first
    launch: x_all is as it was and nothing has been called.  A decline on any later
    launch raises RuntimeError."""
    s = template
    P = len(lmbda)
    n, dim = x_all.numel() // P, s._dimension
    iters = int(s._iterations)
    shape, w, flags = s._shape, ops.inv_spacing(s._spacing, dim), s._flags()
    tau, sigma, theta = s._tau, s._sigma, s._theta
    hden = 1. + sigma * s._huber_gamma if s._reg_type == "huber" else 1.
    data_loss, bg = s._data_loss, s._scaled_background()
    lo, hi = s._bounds
    lm_all = ops.pdl_lambdas(lmbda, x_all)
    points = set(points or ())
    # a group's q and g = A^T q, allocated once beside stack_groups' xbar and p (t = A
    # xbar, where the epilogue does not spare it, is the data side's)
    q_all, g_all = x_all.new_empty(group * n), x_all.new_empty(group * n)
    data = StackedDataSide(s, x_all, group, n)
    launches = Launches(taken)
    for a, b, x, xb, pp, bt_g, wt_g in stack_groups(x_all, bt, wt, strided, P, dim,
                                                    group, start):
        g = b - a
        q, gq = q_all[:g * n], g_all[:g * n]
        q.zero_()
        lm = lm_all[a:b]
        for i in range(iters):
            k = i & 1
            if not (data.dual_step(xb[k], q, bt_g, wt_g, sigma, lm, g, data_loss, bg,
                                   gq) and
                    ops.pdl_stack_iter(xb[k], xb[1 - k], x, gq, pp[k], pp[1 - k], g,
                                       shape, w, sigma, hden, tau, theta, lo, hi, flags,
                                       has_p=i > 0)):
                return launches.declined("pdl_stack")
            launches.accepted()
            if observe is not None and (i + 1) in points:
                for m in range(a, b):
                    observe(m, i + 1)
    return True


class PrimalDualLinearBatch(PrimalDualBatch):
    """PrimalDualBatch's interface for PrimalDualLinearSolver objects: its __init__,
    run() and upload, with this solver's key, operands and runner.  The members never
    stop one by one."""

    _solver_type = PrimalDualLinearSolver
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
        G = ops.pdl_group_size(P, x_all.numel() // P, s0._dimension,
                               x_all.element_size(), own_data=True,
                               own_weights=wt is not None,
                               with_t=not expects_epilogue(s0._op, s0._op_shape))
        res = run_linear_stack(x_all, bt, wt, True, s0, [1. / s._alpha for s in solvers],
                               G, points, observe=observe, taken=taken)
        return None if res is None else (G, None)


class PrimalDualLinearSweep(PrimalDualSweep):
    """PrimalDualSweep's interface for an alpha sweep of PrimalDualLinearSolver on one
    observation: PrimalDualLinearSweep(A, A_adj, b, x0, dimension,
    parameters={"alpha": [...]}, **solver_kwargs) with PrimalDualLinearSolver's keyword
    arguments.  A sweep with a `tolerance`, or one the library declines, runs its
    members one after the other through plain solvers."""

    def __init__(self, A, A_adj, b, x0, dimension, parameters, **solver_kwargs):
        for k in parameters:
            if k not in SWEEP_KEYS:
                raise ValueError("unknown sweep parameter '%s' (supported: %s)" %
                                 (k, ", ".join(SWEEP_KEYS)))
        members = member_parameters(parameters)
        kw = dict(solver_kwargs)
        self._defaults = dict(alpha=kw.pop("alpha", 0.01))
        self._args = dict(A=A, A_adj=A_adj, b=b, x0=x0, dimension=dimension)
        self._kwargs = kw
        template = self._solver(members[0])          # the arguments' own refusals
        # (no stacked stopping for this solver: DESIGN.md section 8)
        self._init_state(x0, members, template._iterations, template._tolerance,
                         template._check_every, False, template._x_scale,
                         template._dtype)

    def _solver(self, member=None):
        kw = dict(self._defaults)
        kw.update(member or {})
        return PrimalDualLinearSolver(alpha=kw["alpha"], **self._args, **self._kwargs)

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
        return bt, wt, ops.pdl_group_size(
            len(self._members), x0.numel(), template._dimension, x0.element_size(),
            own_data=False, own_weights=False,
            with_t=not expects_epilogue(template._op, template._op_shape))

    def _advance(self, template, form, x_all, bt, wt, group, points, observe, x0):
        alphas = [dict(self._defaults, **member)["alpha"] for member in self._members]
        return run_linear_stack(x_all, bt, wt, False, template,
                                [1. / float(a) for a in alphas], group, points,
                                observe=observe, start=x0)
