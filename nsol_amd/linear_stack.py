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
"""
import datetime
import time

import numpy as np

from . import linear_operators, ops
from .device import is_device_tensor, torch_dtype
from .linear_operators import ConvolutionOperator
from .observer import observation_points
from .parameter_sweep import PrimalDualSweep, member_parameters
from .primal_dual_linear_solver import PrimalDualLinearSolver
from .solver_batch import PrimalDualBatch, _dev_index, plan_stacks

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


def member_key(solver):
    """What the members of one stack share, or None for a solver that runs on its own:
    the operators (by value) and the shapes they are applied to, the volume's shape,
    spacing, dimension, reg_type, huber_gamma, isotropic, data_loss, bounds, tau,
    sigma, dtype, iteration count, a device-mode observer's points, whether the data
    term is weighted, and the devices of b, x0 and the weights."""
    if not isinstance(solver, PrimalDualLinearSolver):
        return None
    op, op_adj = solver._op, solver._op_adj
    if not (isinstance(op, ConvolutionOperator) and
            isinstance(op_adj, ConvolutionOperator)):
        return None             # foreign or NumPy-only callables, other operators
    iters = int(solver._iterations)
    if iters < 1 or solver._verbose or solver._tolerance is not None:
        return None             # (its own stopping iteration: no stacked form)
    if solver._m != solver._n or solver._x0_ndim != 1:
        return None
    b = solver._b
    if int(b.numel() if is_device_tensor(b) else np.size(b)) != solver._m:
        return None             # (run() says what is wrong with it)
    points = None
    obs = solver._observer
    if obs is not None:
        if obs.get_keep_iterates():
            return None
        points = tuple(observation_points(iters, obs.get_every()))
    x0_dev = None if solver._x0_host is not None else _dev_index(solver._x0_dev)
    w = solver._weights
    return (operator_key(op), tuple(solver._op_shape), operator_key(op_adj),
            tuple(solver._op_adj_shape), tuple(solver._shape),
            tuple(float(v) for v in solver._spacing), int(solver._dimension),
            solver._reg_type, float(solver._huber_gamma), bool(solver._isotropic),
            solver._data_loss, tuple(float(v) for v in solver._bounds),
            float(solver._tau), float(solver._sigma), np.dtype(solver._dtype).name,
            iters, points, w is not None, ("b", _dev_index(b)), ("x0", x0_dev),
            ("weights", _dev_index(w)))


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
    import torch
    s = template
    P = len(lmbda)
    n, dim = x_all.numel() // P, s._dimension
    iters = int(s._iterations)
    op, op_shape, adj, adj_shape = s._op, s._op_shape, s._op_adj, s._op_adj_shape
    shape, w, flags = s._shape, ops.inv_spacing(s._spacing, dim), s._flags()
    tau, sigma, theta = s._tau, s._sigma, s._theta
    hden = 1. + sigma * s._huber_gamma if s._reg_type == "huber" else 1.
    l1 = s._data_loss == "ell1"
    lo, hi = s._bounds
    lm_all = ops.pdl_lambdas(lmbda, x_all)
    points = set(points or ())
    # the state of a group, allocated once
    xbar = [x_all.new_empty(group * n) for _ in range(2)]
    p = [x_all.new_empty(group * dim * n) for _ in range(2)]
    q_all, g_all = x_all.new_empty(group * n), x_all.new_empty(group * n)
    t_all = None
    # q <- sigma A xbar + q as the epilogue of the one-pass blur, while it applies
    epilogue = bool(linear_operators.USE_BLUR_EPILOGUE)
    slots = torch.empty(group, dtype=torch.float64, device=x_all.device) \
        if epilogue else None
    first = True
    for a, b in ops.sweep_groups(P, group):
        g = b - a
        x = x_all[a * n:b * n]
        xb = [v[:g * n] for v in xbar]
        pp = [v[:g * dim * n] for v in p]
        q, gq = q_all[:g * n], g_all[:g * n]
        if start is None:
            xb[0].copy_(x)
        else:
            xb[0].view(g, n).copy_(start)
        q.zero_()
        bt_g, wt_g = bt, wt
        if strided:
            bt_g, wt_g = bt[a * n:b * n], None if wt is None else wt[a * n:b * n]
        lm = lm_all[a:b]
        for i in range(iters):
            k = i & 1
            if epilogue and op.apply_axpby_stacked(xb[k], q, op_shape, g, sigma, 1.,
                                                   results=slots[:g]) is None:
                epilogue = False       # the kernel declined: nothing ran, q is intact
            if epilogue:
                ok = ops.pdl_stack_dual_data(q, None, bt_g, wt_g, sigma, lm, g, l1)
            else:
                if t_all is None:
                    t_all = x_all.new_empty(group * n)
                t = op._apply_stacked(xb[k], op_shape, g, out=t_all[:g * n])
                ok = ops.pdl_stack_dual_data(q, t, bt_g, wt_g, sigma, lm, g, l1)
            if ok:
                adj._apply_stacked(q, adj_shape, g, out=gq)
                ok = ops.pdl_stack_iter(xb[k], xb[1 - k], x, gq, pp[k], pp[1 - k], g,
                                        shape, w, sigma, hden, tau, theta, lo, hi, flags,
                                        has_p=i > 0)
            if not ok:
                if first:
                    return None
                raise RuntimeError("nsol_pdl_stack declined in mid-run")
            if first:
                first = False
                if taken is not None:
                    taken()
            if observe is not None and (i + 1) in points:
                for m in range(a, b):
                    observe(m, i + 1)
    return True


class PrimalDualLinearBatch(PrimalDualBatch):
    """PrimalDualBatch's interface for PrimalDualLinearSolver objects."""

    def __init__(self, solvers):
        solvers = list(solvers)
        if not solvers:
            raise ValueError("a batch needs at least one solver")
        seen = set()
        for s in solvers:
            if not isinstance(s, PrimalDualLinearSolver):
                raise ValueError("a batch takes PrimalDualLinearSolver objects, not %s" %
                                 type(s).__name__)
            if id(s) in seen:
                raise ValueError("the same solver object is in the batch twice")
            seen.add(id(s))
            if s._x0_ndim != 1:
                raise ValueError("Initial value x0 must be a 1D array")
        self._solvers = solvers
        self._stacked_stopping = False      # (not for this solver: DESIGN.md section 8)
        self._execution = None
        self._group = None
        self._stacks = []
        self._computational_time = datetime.timedelta(seconds=0)

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
        for idx in plan_stacks([member_key(s) for s in solvers]):
            t1 = time.time()
            x_all = self._run_stack(idx)
            if x_all is None:
                continue                       # declined: nothing was written
            torch.cuda.synchronize()
            took = datetime.timedelta(seconds=time.time() - t1)
            n = x_all.numel() // len(idx)
            for m, i in enumerate(idx):
                s = solvers[i]
                s._x = x_all[m * n:(m + 1) * n]
                s._execution = "fused"
                s._iterations_done, s._stop_reason = int(s._iterations), "iterations"
                s._rule = None
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

    def _run_stack(self, idx):
        """The members `idx` together (run_linear_stack).  Returns their stacked
        iterate (P * n, solver units), or None when the library declined on its first
        launch (nothing has been written to any solver then)."""
        import torch
        from .device import device
        from .proximal_operators import scaled_data_on_device, weights_on_device
        solvers = [self._solvers[i] for i in idx]
        s0 = solvers[0]
        P, iters, n, dim = len(idx), int(s0._iterations), s0._n, s0._dimension
        td = torch_dtype(s0._dtype)
        dev = device()
        # ---- the scaled observations: float64 / x_scale, rounded once
        if is_device_tensor(s0._b):
            bt = torch.empty(P * n, dtype=td, device=dev)
            for m, s in enumerate(solvers):
                bt[m * n:(m + 1) * n].copy_(scaled_data_on_device(s._b, s._x_scale,
                                                                   bt[:1]))
        else:
            raw = self._upload_rows([s._b for s in solvers], np.float64)
            bt = ops.scale_rows(raw, self._scales([s._x_scale for s in solvers]), P,
                                divide=True, dtype=td).view(-1)
        # ---- the start vectors: rounded to the working dtype, then / x_scale
        if s0._x0_host is None:
            x_all = torch.empty(P * n, dtype=td, device=dev)
            for m, s in enumerate(solvers):
                x_all[m * n:(m + 1) * n].copy_(s._x0_device())
        else:
            raw = self._upload_rows([s._x0_host for s in solvers], s0._dtype)
            x_all = ops.scale_rows(raw, self._scales([s._x_scale for s in solvers]),
                                   P, divide=True).view(-1)
        # ---- every member's own weights, checked by the constructor
        wt = None
        if s0._weights is not None:
            if is_device_tensor(s0._weights):
                wt = torch.empty(P * n, dtype=td, device=dev)
                for m, s in enumerate(solvers):
                    wt[m * n:(m + 1) * n].copy_(weights_on_device(s._weights, wt[:1]))
            else:
                wt = self._upload_rows([s._weights for s in solvers], s0._dtype).view(-1)
        G = ops.pdl_group_size(P, n, dim, x_all.element_size(), own_data=True,
                               own_weights=wt is not None,
                               with_t=not expects_epilogue(s0._op, s0._op_shape))
        obs = s0._observer
        points = None if obs is None else observation_points(iters, obs.get_every())

        def taken():
            # the library has taken the stack: the observation of the start vectors,
            # as Solver._observe_start makes it
            for s in solvers:
                s._x = None
                s._observe_start(iters)

        res = run_linear_stack(
            x_all, bt, wt, True, s0, [1. / s._alpha for s in solvers], G, points,
            observe=None if obs is None else (lambda m, it: solvers[m]._observe_at(
                it, x_all[m * n:(m + 1) * n])),
            taken=None if obs is None else taken)
        if res is None:
            return None
        self._group = max(self._group or 0, G)
        return x_all


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
        self._members = member_parameters(parameters)
        kw = dict(solver_kwargs)
        self._defaults = dict(alpha=kw.pop("alpha", 0.01))
        self._args = dict(A=A, A_adj=A_adj, b=b, x0=x0, dimension=dimension)
        self._kwargs = kw
        template = self._solver(self._members[0])    # the arguments' own refusals
        self._x0 = x0
        self._iterations = int(template._iterations)
        self._tolerance = template._tolerance
        self._stacked_stopping = False      # (not for this solver: DESIGN.md section 8)
        self._check_every = template._check_every
        self._iterations_done = None
        self._x_scale = float(template._x_scale)
        self._dtype = template._dtype
        self._functions = {}
        self._every = None
        self._execution = None
        self._computational_time = datetime.timedelta(seconds=0)
        self._x_all = self._x_list = None
        self._observers = []
        self._n = None

    def _solver(self, member=None):
        kw = dict(self._defaults)
        kw.update(member or {})
        return PrimalDualLinearSolver(alpha=kw["alpha"], **self._args, **self._kwargs)

    def run(self):
        import torch
        t0 = time.time()
        template = self._solver(self._members[0])
        if template._x0_ndim != 1:
            raise ValueError("Initial value x0 must be a 1D array")
        self._x_all = self._x_list = None
        self._observers = []
        self._iterations_done = None
        stacked = False
        if member_key(template) is not None:
            stacked = self._run_stacked(template)
        if not stacked:
            self._run_sequential()
        torch.cuda.synchronize()
        for obs in self._observers:
            obs._finish()                 # every board, read after the one wait
        self._execution = "stacked" if stacked else "sequential"
        for obs in self._observers:
            obs.compute_measures()
        self._computational_time = datetime.timedelta(seconds=time.time() - t0)

    def _run_stacked(self, template, plan=None):
        """All members together (run_linear_stack, observation, weights and start
        shared); False when the library declined (nothing has run then)."""
        import torch
        from .device import to_device
        from .proximal_operators import scaled_data_on_device, weights_on_device
        iters = self._iterations
        alphas = [dict(self._defaults, **member)["alpha"] for member in self._members]
        P = len(alphas)
        x0 = template._x0_device()
        n = x0.numel()
        bt = scaled_data_on_device(template._b, template._x_scale, x0)
        wt = None if template._weights is None else \
            weights_on_device(template._weights, x0)
        G = ops.pdl_group_size(
            P, n, template._dimension, x0.element_size(), own_data=False,
            own_weights=False,
            with_t=not expects_epilogue(template._op, template._op_shape))
        x_all = torch.empty(P * n, dtype=x0.dtype, device=x0.device)
        x_all.view(P, n).copy_(x0)
        # the observation of the start vector, as Solver._observe_at(0) makes it
        observers, points = [], None
        if self._functions:
            refs = {}
            for _ in alphas:
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
        res = run_linear_stack(
            x_all, bt, wt, False, template, [1. / float(a) for a in alphas], G, points,
            observe=(lambda m, it: observers[m]._observe(
                it, x_all[m * n:(m + 1) * n], self._x_scale)) if observers else None,
            start=x0)
        if res is None:
            return False
        self._x_all, self._n, self._observers = x_all, n, observers
        self._group = G
        return True
