"""CPU-only side of the stacked front end that PrimalDualBatch, PrimalDualLinearBatch,
PrimalDualSweep and PrimalDualLinearSweep share: the inputs of
test_stack_front_gpu.py with their margins."""
import numpy as np
import pytest

from test_pd_stop_host import pd_stop_denoise
from test_pd_stretches_host import CHECKS, met_at_the_second_check
from test_pd_stretches_host import EVERY, ITERS, NEVER          # 3, 7, 1e-300
from test_pd_weighted_host import mixed_weights

# ------------------------------------------- inputs of test_stack_front_gpu.py
MEMBERS = 5
SHAPES = [(6, 8), (4, 5, 6)]
ALPHAS = [0.05, 0.02, 0.2, 0.01, 0.1]
STOP_SHAPE = (6, 8)
SECOND_CHECK = CHECKS[1]


def member_observation(shape, m):
    rng = np.random.default_rng(sum(shape) + 7 * m)
    return 50.0 + 30.0 * rng.standard_normal(shape)


def _stop_weights(weighted, m):
    return mixed_weights(STOP_SHAPE, 7 + m) if weighted else None


def stack_tolerances(weighted):
    """The members' tolerances: the even ones meet theirs at the second check with the
    restatement's 3 % margin, the odd ones never."""
    return [NEVER if m & 1 else met_at_the_second_check(
        member_observation(STOP_SHAPE, m), "TV", False, _stop_weights(weighted, m),
        ALPHAS[m])[0] for m in range(MEMBERS)]


def sweep_tolerance(weighted):
    """(a tolerance that some of the sweep's members meet at their second check and the
    others do not, the iterations every member does with it).  The tolerance is the
    geometric mean of the two neighbours that are furthest apart among the members'
    max(r_x, r_p) at the second check in the float64 restatement, which then asserts
    its 3 % margin at every check of every member."""
    obs, w = member_observation(STOP_SHAPE, 0), _stop_weights(weighted, 0)
    args = (4 * len(STOP_SHAPE), ITERS)
    kw = dict(check_every=EVERY, weights=w)
    second = sorted(max(pd_stop_denoise(
        obs, STOP_SHAPE, "TV", "L2", "ALG2", alpha, *args, NEVER, margin=0,
        **kw)["changes"][1, 1:]) for alpha in ALPHAS)
    lo, hi = max(zip(second[:-1], second[1:]), key=lambda pair: pair[1] / pair[0])
    tol = float(np.sqrt(lo * hi))
    done = [pd_stop_denoise(obs, STOP_SHAPE, "TV", "L2", "ALG2", alpha, *args, tol,
                            **kw)["done"] for alpha in ALPHAS]
    return tol, done


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_the_stopping_members_keep_their_margin(weighted):
    assert (ITERS, EVERY, SECOND_CHECK) == (7, 3, 6)
    tolerances = stack_tolerances(weighted)
    assert len(set(tolerances)) == 4 and all(0 < t < 1 for t in tolerances)
    tol, done = sweep_tolerance(weighted)
    assert set(done) == {SECOND_CHECK, ITERS}, done


# ----------------------------------------------------------- the group iterator
N, DIM, P, GROUP = 6, 2, 5, 2


def _stacked_operands(strided):
    """Member m's start vector holds m, its observation 10 + m, its weights 20 + m."""
    import torch
    x_all = torch.arange(P, dtype=torch.float64).repeat_interleave(N)
    if strided:
        return x_all, x_all + 10, x_all + 20
    return x_all, torch.full((N,), 10.0, dtype=torch.float64), \
        torch.full((N,), 20.0, dtype=torch.float64)


@pytest.mark.parametrize("strided", [True, False], ids=["own", "shared"])
def test_groups_are_views_of_state_that_is_allocated_once(strided):
    from nsol_amd.stacked_run import stack_groups
    x_all, bt, wt = _stacked_operands(strided)
    seen, state = [], set()
    for grp in stack_groups(x_all, bt, wt, strided, P, DIM, GROUP):
        a, b = grp.a, grp.b
        g = b - a
        seen.append((a, b))
        # views of the right lengths, also for the ragged last group
        assert grp.x.numel() == g * N and grp.x.data_ptr() == x_all[a * N:].data_ptr()
        assert [t.numel() for t in grp.xbar] == [g * N] * 2
        assert [t.numel() for t in grp.p] == [g * DIM * N] * 2
        # every member's own start vector is in xbar[0]
        assert grp.xbar[0].view(g, N)[:, 0].tolist() == list(range(a, b))
        if strided:
            assert grp.bt.numel() == grp.wt.numel() == g * N
            assert grp.bt.view(g, N)[:, 0].tolist() == [10. + m for m in range(a, b)]
            assert grp.wt.view(g, N)[:, 0].tolist() == [20. + m for m in range(a, b)]
            assert grp.bt.data_ptr() == bt[a * N:].data_ptr()
        else:
            assert grp.bt is bt and grp.wt is wt
        state.add(tuple(t.data_ptr() for t in grp.xbar + grp.p))
    assert seen == [(0, 2), (2, 4), (4, 5)]
    assert len(state) == 1 and len(set(next(iter(state)))) == 4


def test_groups_without_weights_and_with_a_shared_start():
    import torch
    from nsol_amd.stacked_run import stack_groups
    start = torch.arange(N, dtype=torch.float64) + 5
    x_all = start.repeat(P)
    sizes = []
    for grp in stack_groups(x_all, start + 10, None, False, P, DIM, GROUP, start=start):
        g = grp.b - grp.a
        sizes.append(g)
        assert grp.wt is None
        assert bool((grp.xbar[0].view(g, N) == start).all())
    assert sizes == [2, 2, 1]
    for grp in stack_groups(x_all, x_all + 10, None, True, P, DIM, GROUP):
        assert grp.wt is None and grp.bt.numel() == (grp.b - grp.a) * N


# ---------------------------------------------------------- the decline contract
def test_launches_is_the_decline_contract():
    from nsol_amd.stacked_run import Launches
    log = []
    launches = Launches(lambda: log.append("taken"))
    assert launches.declined("pd_batch_run") is None and log == []
    launches.accepted()
    launches.accepted()
    assert log == ["taken"]
    with pytest.raises(RuntimeError, match="nsol_pd_batch_run declined in mid-run"):
        launches.declined("pd_batch_run")
    Launches().accepted()                   # no hook: nothing to call


def _run_plain(log, decline_at):
    """run_stack on five members in groups of two with an entry that declines its
    call number decline_at."""
    from nsol_amd.stacked_run import run_stack
    from test_pd_stretches_host import PLAN, FakeEntry

    class pd_batch_run(FakeEntry):
        __name__ = "pd_batch_run"
    x_all, bt, _ = _stacked_operands(True)
    return run_stack(x_all, bt, None, True, PLAN, [("ALG2", 8, 0.05)] * P, 7, GROUP,
                     pd_batch_run(log, decline_at), [0, 4, 7],
                     observe=lambda m, it: log.append(("observe", m, it)),
                     taken=lambda: log.append(("taken",)))


def _run_linear(log, decline_at, monkeypatch):
    """run_linear_stack on five members in groups of two with a tile entry that
    declines its call number decline_at; the blurs and the update of q do nothing."""
    from nsol_amd import linear_operators, linear_stack, ops
    from test_pd_linear_stack_host import _solver
    from test_pd_linear_host import box_kernel
    template = _solver(shape=(2, 3), kernel=box_kernel(2), iterations=7)
    calls = []

    def pdl_stack_iter(xbar_in, xbar_out, x, g, p_in, p_out, members, *args, **kw):
        calls.append(members)
        if len(calls) == decline_at:
            return False
        assert xbar_in.numel() == xbar_out.numel() == x.numel() == g.numel() == members * N
        assert p_in.numel() == p_out.numel() == members * DIM * N
        assert kw["has_p"] == (not bool((xbar_in == x).all()))
        log.append(("launch", int(x[0]), members))
        xbar_out.copy_(xbar_in + 100)       # (no longer the start vectors)
        return True
    monkeypatch.setattr(linear_operators, "USE_BLUR_EPILOGUE", False)
    monkeypatch.setattr(linear_operators.ConvolutionOperator, "_apply_stacked",
                        lambda self, x, shape, members, out=None: out)
    monkeypatch.setattr(ops, "pdl_stack_dual_data", lambda *a, **kw: True)
    monkeypatch.setattr(ops, "pdl_stack_iter", pdl_stack_iter)
    x_all, bt, _ = _stacked_operands(True)
    return linear_stack.run_linear_stack(
        x_all, bt, None, True, template, [20.] * P, GROUP, [0, 4, 7],
        observe=lambda m, it: log.append(("observe", m, it)),
        taken=lambda: log.append(("taken",)))


RUNNERS = {"run_stack": (lambda log, at, mp: _run_plain(log, at), "nsol_pd_batch_run"),
           "run_linear_stack": (_run_linear, "nsol_pdl_stack")}


@pytest.mark.parametrize("runner", sorted(RUNNERS))
def test_both_runners_keep_the_decline_contract(runner, monkeypatch):
    run, entry = RUNNERS[runner]
    # the very first launch: None, and nothing has been called
    log = []
    assert run(log, 1, monkeypatch) is None and log == []
    # a later launch, in the first group or in the last
    for at in (2, 5):
        log = []
        with pytest.raises(RuntimeError, match=entry + " declined in mid-run"):
            run(log, at, monkeypatch)
        assert log.count(("taken",)) == 1
    # no decline: the hook once, after the first launch and before the first observe
    log = []
    assert run(log, None, monkeypatch) is not None
    assert [e[0] for e in log[:2]] == ["launch", "taken"]
    assert log.count(("taken",)) == 1
    first_observe = min(i for i, e in enumerate(log) if e[0] == "observe")
    assert log.index(("taken",)) < first_observe
    assert [e[1:] for e in log if e[0] == "observe"] == [
        (m, it) for a, b in [(0, 2), (2, 4), (4, 5)] for it in (4, 7) for m in range(a, b)]
    # (first member, members) of the launches: every group, the last one ragged
    assert sorted(set(e[1:3] for e in log if e[0] == "launch")) == \
        [(0, 2), (2, 2), (4, 1)]


# ----------------------------------------------------------- the operand upload
class _UploadSolver(object):
    """What _upload_stack reads of a solver; x0 on the host, or `on_device` as a
    tensor already divided by x_scale."""

    def __init__(self, x0, x_scale, dtype, on_device):
        import torch
        self._dtype, self._x_scale = dtype, x_scale
        self._x0_host = None if on_device else np.array(x0)
        self._x0_dev = torch.from_numpy(x0.astype(dtype) / dtype(x_scale)) \
            if on_device else None

    def _x0_device(self):
        return self._x0_dev


@pytest.fixture
def cpu_device(monkeypatch):
    """A CPU stand-in for the device: torch's CPU tensors count as device-resident, the
    page-locked transport is a plain copy with the same cast, and ops.scale_rows and
    scaled_data_on_device are restated with torch."""
    import torch
    import nsol_amd.device
    from nsol_amd import ops, proximal_operators, solver_batch

    def upload_rows(self, rows, dtype):
        host = np.empty((len(rows), np.size(rows[0])), dtype=dtype)
        for m, r in enumerate(rows):
            np.copyto(host[m], np.asarray(r).reshape(-1), casting="unsafe")
        self._staging.append(host)
        return torch.from_numpy(host)

    def scale_rows(x, s, members, divide=False, out=None, dtype=None):
        assert divide and s.dtype == torch.float64 and s.numel() == members
        rows = x.view(members, -1)
        return (rows.double() / s[:, None]).to(rows.dtype if dtype is None else dtype)

    def scaled_data(data, scale, like):
        return (data.double() / scale).to(like.dtype).view(-1)
    on_cpu = lambda v: isinstance(v, torch.Tensor)
    monkeypatch.setattr(nsol_amd.device, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(solver_batch, "is_device_tensor", on_cpu)
    monkeypatch.setattr(solver_batch.PrimalDualBatch, "_upload_rows", upload_rows)
    monkeypatch.setattr(ops, "scale_rows", scale_rows)
    monkeypatch.setattr(proximal_operators, "scaled_data_on_device", scaled_data)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_upload_scales_every_member_by_its_own_scale(cpu_device, weighted, where, dtype):
    import torch
    from nsol_amd.solver_batch import PrimalDualBatch
    on_device = where == "device"
    n = 11
    rng = np.random.default_rng(3)
    data = [50. + 30. * rng.standard_normal(n) for _ in range(P)]
    x0 = [d + rng.standard_normal(n) for d in data]
    weights = [3. * rng.random(n) for _ in range(P)] if weighted else None
    scales = [float(np.max(d)) * (1 + m) for m, d in enumerate(data)]
    data_scales = [1.5 * s for s in scales]     # (a plan's scale is its prox's own)
    solvers = [_UploadSolver(x, s, dtype, on_device) for x, s in zip(x0, scales)]
    place = torch.from_numpy if on_device else (lambda a: a)
    converted = []

    def device_weights(w, like):
        converted.append(w)
        assert like.dtype == torch.from_numpy(np.empty(0, dtype)).dtype
        return w.reshape(-1)
    batch = PrimalDualBatch.__new__(PrimalDualBatch)
    batch._staging = []
    bt, x_all, wt = batch._upload_stack(
        solvers, [(place(d), s) for d, s in zip(data, data_scales)],
        None if weights is None else [place(w) for w in weights], device_weights)
    for t in (bt, x_all) + ((wt,) if weighted else ()):
        assert t.shape == (P * n,) and t.numpy().dtype == dtype and t.is_contiguous()
    for m in range(P):
        row = slice(m * n, (m + 1) * n)
        # float64 / the member's own scale, rounded once
        assert np.array_equal(bt[row].numpy(), (data[m] / data_scales[m]).astype(dtype))
        # rounded to the working dtype, then / the member's own x_scale
        want = x0[m].astype(dtype) / dtype(scales[m]) if on_device else \
            (x0[m].astype(dtype).astype(np.float64) / scales[m]).astype(dtype)
        assert np.array_equal(x_all[row].numpy(), want)
        if weighted:
            assert np.array_equal(wt[row].numpy(), weights[m].astype(dtype))
    assert wt is None or weighted
    # host inputs travel in one staged array each, kept until run() has synchronised;
    # only device-resident weights go through the converter
    assert len(batch._staging) == (0 if on_device else 2 + weighted)
    assert len(converted) == (P if weighted and on_device else 0)


# ---------------------------------------------------------- the batch front end
class _FakeObserver(object):
    def __init__(self):
        self.finished, self.time = 0, None

    def _finish(self):
        self.finished += 1

    def set_computational_time(self, t):
        self.time = t


class _FakeSolver(object):
    _x0_ndim, _iterations, _tolerance = 1, 7, 1e-3

    def __init__(self, observed=False):
        self.runs = 0
        self._observer = _FakeObserver() if observed else None

    def run(self):
        self.runs += 1


def test_the_batch_front_end_writes_back_what_a_stack_did(monkeypatch):
    import datetime
    import torch
    from nsol_amd.solver_batch import PrimalDualBatch
    from nsol_amd.stacked_stopping import GroupResult, StoppedRule
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: log.append("synchronize"))
    log, n = [], 4
    stopped = GroupResult(2)
    stopped.iterations_done, stopped.stop_reason = [6, 7], ["tolerance", "iterations"]
    stopped.changes = [[(3., .5, .5), (6., .1, .1)], [(3., .5, .5)]]
    # solvers 0 and 3 stack, 1 and 5 form a stack that the library declines, 4 and 6
    # stack and stop one by one, 2 has no partner
    ran = {(0, 3): (torch.arange(2. * n), None), (1, 5): None,
           (4, 6): (torch.arange(2. * n) + 100, stopped)}

    class Batch(PrimalDualBatch):
        _solver_type = _FakeSolver

        def _stacks_to_try(self):
            return [([0, 3], False), ([1, 5], False), ([4, 6], True)]

        def _run_stack(self, idx, stopping):
            log.append(("stack", tuple(idx), stopping))
            assert self._staging == []
            return ran[tuple(idx)]

        def _after_wait(self):
            log.append("after")
    with pytest.raises(ValueError, match="a batch takes _FakeSolver objects, not int"):
        Batch([_FakeSolver(), 3])
    solvers = [_FakeSolver(observed=i in (3, 4, 5)) for i in range(7)]
    batch = Batch(solvers, stacked_stopping=True)
    batch.run()
    assert batch.get_execution() == ["stacked", "sequential", "sequential", "stacked",
                                     "stacked", "sequential", "stacked"]
    # one wait and one hook behind every stack that ran, none behind the declined one
    assert log == [("stack", (0, 3), False), "synchronize", "after",
                   ("stack", (1, 5), False),
                   ("stack", (4, 6), True), "synchronize", "after"]
    assert [s.runs for s in solvers] == [0, 1, 1, 0, 0, 1, 0]
    assert not hasattr(batch, "_staging")
    assert [idx for idx, _ in batch._stacks] == [[0, 3], [4, 6]]
    assert batch._stacks[0][1] is ran[(0, 3)][0] and batch._stacks[1][1] is ran[(4, 6)][0]
    for idx, stopping in (((0, 3), False), ((4, 6), True)):
        for m, i in enumerate(idx):
            s = solvers[i]
            assert s._x.tolist() == ran[idx][0][m * n:(m + 1) * n].tolist()
            assert s._execution == "fused"
            assert isinstance(s._computational_time, datetime.timedelta)
            if stopping:
                assert (s._iterations_done, s._stop_reason) == \
                    (stopped.iterations_done[m], stopped.stop_reason[m])
                assert isinstance(s._rule, StoppedRule)
                assert s._rule.tolerance == 1e-3 and s._rule.rows == stopped.changes[m]
            else:
                assert (s._iterations_done, s._stop_reason) == (7, "iterations")
                assert s._rule is None
            if s._observer is not None:
                assert s._observer.finished == 1
                assert s._observer.time == s._computational_time
    # a sequential solver is left to its own run(): nothing was written to it
    for i in (1, 2, 5):
        assert not hasattr(solvers[i], "_x") and not hasattr(solvers[i], "_execution")
    assert solvers[5]._observer.finished == 0


def test_the_linear_batch_is_the_same_class_body():
    from nsol_amd.linear_stack import PrimalDualLinearBatch
    from nsol_amd.solver_batch import PrimalDualBatch
    for name in ("__init__", "run", "_run_stack", "_upload_stack", "_upload_rows"):
        assert name not in vars(PrimalDualLinearBatch), name
        assert getattr(PrimalDualLinearBatch, name) is getattr(PrimalDualBatch, name)
    with pytest.raises(ValueError, match="no stacked stopping"):
        PrimalDualLinearBatch([object()], stacked_stopping=True)
