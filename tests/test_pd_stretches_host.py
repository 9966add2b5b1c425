"""CPU-only side of the two loops that enqueue fused primal-dual runs in stretches:
PrimalDualSolver._run_stretches against a recording form and a scripted rule,
stacked_run.run_stack against a fake entry, the group-size formula against a table,
and the inputs of test_pd_run_forms_gpu.py with their margins."""
import numpy as np
import pytest

from test_pd_stop_host import MARGIN, _wired, observation, pd_stop_denoise
from test_pd_weighted_host import mixed_weights

# ------------------------------------------- inputs of test_pd_run_forms_gpu.py
ITERS, EVERY = 7, 3
CHECKS = [3, 6, 7]
NEVER = 1e-300
# the smallest that reach every access form: ragged rows (pitched once
# PITCH_MIN_VOXELS allows it), rows of whole vectors, 2-D, 1-D
SHAPES = [(3, 5, 19), (2, 3, 16), (5, 9), (37,)]
ALPHA, ALG = 0.05, "ALG2"
STACK_SHAPE, STACK_ALPHAS = (5, 9), [0.05, 0.02, 0.2]
_restated = {}


def form_reg(shape):
    return "Huber" if shape in ((2, 3, 16), (37,)) else "TV"


def form_weights(shape, weighted, seed=None):
    return mixed_weights(shape, sum(shape) if seed is None else seed) \
        if weighted else None


def member_obs(m):
    return 50.0 + 30.0 * np.random.default_rng(11 + m).standard_normal(STACK_SHAPE)


def met_at_the_second_check(obs, reg, iso, weights, alpha=ALPHA):
    """The tolerance a run of ITERS iterations meets at its second check and not at its
    first: the geometric mean of max(r_x, r_p) at the two in the float64 restatement,
    which then asserts its 3 % margin at both.  Returns (tolerance, the restatement's
    result)."""
    key = (obs.tobytes(), reg, iso, None if weights is None else weights.tobytes(),
           alpha)
    if key not in _restated:
        shape = obs.shape
        args = (obs, shape, reg, "L2", ALG, alpha, 4 * len(shape), ITERS)
        rows = pd_stop_denoise(*args, NEVER, check_every=EVERY, iso=iso,
                               weights=weights, margin=0)["changes"]
        assert list(rows[:, 0]) == CHECKS
        first, second = max(rows[0, 1:]), max(rows[1, 1:])
        tol = float(np.sqrt(first * second))
        assert first >= (1 + MARGIN) * tol and second <= (1 - MARGIN) * tol, rows
        ref = pd_stop_denoise(*args, tol, check_every=EVERY, iso=iso, weights=weights,
                              margin=MARGIN)
        assert ref["done"] == CHECKS[1] and ref["reason"] == "tolerance"
        _restated[key] = tol, ref
    return _restated[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_the_single_runs_keep_their_margin(shape, iso, weighted):
    tol, ref = met_at_the_second_check(observation(shape), form_reg(shape), iso,
                                       form_weights(shape, weighted))
    assert 0 < tol < 1 and len(ref["changes"]) == 2


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_the_sweep_and_stack_members_keep_their_margin(weighted):
    obs, w = member_obs(0), form_weights(STACK_SHAPE, weighted)
    tol = met_at_the_second_check(obs, "TV", False, w, STACK_ALPHAS[0])[0]
    for alpha in STACK_ALPHAS[1:]:          # the sweep's other members, its tolerance
        pd_stop_denoise(obs, STACK_SHAPE, "TV", "L2", ALG, alpha, 8, ITERS, tol,
                        check_every=EVERY, weights=w)
    for m, alpha in enumerate(STACK_ALPHAS):
        met_at_the_second_check(member_obs(m), "TV", False,
                                form_weights(STACK_SHAPE, weighted, 7 + m), alpha)


# ------------------------------------------------------- the single-run loop
class RecordingForm(object):
    """Stands in for primal_dual_solver._PlainForm: logs what the loop asks for."""
    x, layout = "x", ("shape", 20)

    def __init__(self, log, slots=None):
        self.log, self.slots = log, list(slots or [])

    def advance(self, xbar_in, xbar_out, p_in, p_out, a, last):
        assert (xbar_in[-1], xbar_out[-1]) == (p_in[-1], p_out[-1])   # one half each
        assert xbar_in != xbar_out
        self.log.append(("advance", a, last, xbar_in, xbar_out))
        return self.slots.pop(0) if self.slots else 1

    def check(self, xbar_in, xbar_out, p_in, p_out, i, ws, row):
        assert (xbar_in[-1], xbar_out[-1]) == (p_in[-1], p_out[-1])
        assert (ws, row) == ("ws", "row%d" % (i + 1))
        self.log.append(("check", i, xbar_in, xbar_out))


class ScriptedRule(object):
    """Stands in for stopping._StopRule: fires at the check `fire_at`."""
    ws = "ws"

    def __init__(self, log, iterations, check_every, fire_at=None):
        from nsol_amd.stopping import check_points
        self.log, self.fire_at = log, fire_at
        self.points = check_points(iterations, check_every)

    def is_point(self, it):
        return it in self.points

    def row(self, it):
        return "row%d" % it

    def decide(self, it):
        self.log.append(("decide", it))
        return it == self.fire_at


def _stretches(iterations, check_every=None, points=None, stepwise=False, fire_at=None,
               slots=None):
    """The log of a run of _run_stretches; check_every None: no tolerance."""
    log = []
    s = _wired(observation((5, 6)))
    s._iterations = iterations
    s._iterations_done, s._stop_reason = 0, "iterations"       # as _run() starts
    if check_every is not None:
        s._check_every = check_every
        s._rule = ScriptedRule(log, iterations, check_every, fire_at)
    if points is not None or stepwise:
        s._observer, s._points = object(), points
        s._observe_iteration = lambda it, x, layout=None: log.append(
            ("observe", it, x, layout))
    bounds, is_stepwise = s._stretch_bounds(iterations)
    assert is_stepwise == stepwise
    s._run_stretches(RecordingForm(log, slots), ["xb0", "xb1"], ["p0", "p1"], bounds)
    return s, log


def _short(log):
    """Without the halves and the observer's operands."""
    return [e[:3] if e[0] == "advance" else e[:2] for e in log]


STRETCHES = [
    # (iterations, check_every, observer points, stepwise) -> the calls in order
    ((7, 3, None, False),
     [("advance", 0, 2), ("check", 2), ("decide", 3), ("advance", 3, 5), ("check", 5),
      ("decide", 6), ("check", 6), ("decide", 7)]),
    ((7, 3, [0, 2, 4, 6, 7], False),
     [("advance", 0, 2), ("observe", 2), ("check", 2), ("observe", 3), ("decide", 3),
      ("advance", 3, 4), ("observe", 4), ("advance", 4, 5), ("check", 5), ("observe", 6),
      ("decide", 6), ("check", 6), ("observe", 7), ("decide", 7)]),
    ((1, 10, None, False), [("check", 0), ("decide", 1)]),
    ((6, 3, None, True),
     [("advance", 0, 1), ("observe", 1), ("advance", 1, 2), ("observe", 2), ("check", 2),
      ("observe", 3), ("decide", 3), ("advance", 3, 4), ("observe", 4),
      ("advance", 4, 5), ("observe", 5), ("check", 5), ("observe", 6), ("decide", 6)]),
    ((0, 3, None, False), []),
]


@pytest.mark.parametrize("case,calls", STRETCHES,
                         ids=["-".join(map(str, c[0])) for c in STRETCHES])
def test_the_loop_asks_the_form_for_these_in_this_order(case, calls):
    iterations, check_every, points, stepwise = case
    s, log = _stretches(iterations, check_every, points, stepwise)
    assert _short(log) == calls
    assert s.get_iterations_done() == iterations
    assert s.get_stop_reason() == "iterations"
    # the observer is handed the form's x in the form's layout
    assert all(e[2:] == ("x", ("shape", 20)) for e in log if e[0] == "observe")
    # a stretch of one checked iteration makes no advance call: every advance covers
    # at least one iteration and ends before the checked one
    assert all(e[2] > e[1] for e in log if e[0] == "advance")
    # p counts as zero where a stretch starts at 0, and only the first one does
    assert [e[1] for e in log if e[0] in ("advance", "check")].count(0) == \
        (1 if iterations else 0)


def test_without_a_tolerance_the_run_is_one_stretch_or_the_observers():
    s, log = _stretches(7)
    assert _short(log) == [("advance", 0, 7)]
    s, log = _stretches(7, points=[0, 3, 6, 7])
    assert _short(log) == [("advance", 0, 3), ("observe", 3), ("advance", 3, 6),
                           ("observe", 6), ("advance", 6, 7), ("observe", 7)]
    s, log = _stretches(3, stepwise=True)
    assert _short(log) == [("advance", 0, 1), ("observe", 1), ("advance", 1, 2),
                           ("observe", 2), ("advance", 2, 3), ("observe", 3)]
    s, log = _stretches(0)
    assert log == []


def test_a_rule_that_fires_at_the_second_check_ends_the_run_there():
    s, log = _stretches(7, 3, [0, 2, 4, 6, 7], fire_at=6)
    assert _short(log)[-3:] == [("check", 5), ("observe", 6), ("decide", 6)]
    assert ("check", 6) not in _short(log)
    assert s.get_iterations_done() == 6 and s.get_stop_reason() == "tolerance"


def test_every_launch_starts_from_the_half_the_one_before_ended_in():
    # slot 0: the state is where the launch started; 1: in the other half
    s, log = _stretches(5, points=[0, 1, 2, 3, 4, 5], slots=[0, 1, 1, 0, 1])
    assert [e[3:] for e in log if e[0] == "advance"] == [
        ("xb0", "xb1"), ("xb0", "xb1"), ("xb1", "xb0"), ("xb0", "xb1"), ("xb0", "xb1")]
    # a checked iteration always ends in the other half
    s, log = _stretches(7, 3, slots=[0, 1])
    assert [e[-2:] for e in log if e[0] in ("advance", "check")] == [
        ("xb0", "xb1"), ("xb0", "xb1"), ("xb1", "xb0"), ("xb0", "xb1"), ("xb1", "xb0")]


def test_next_slot():
    from nsol_amd.stopping import next_slot
    assert [next_slot(k, s) for k in (0, 1) for s in (0, 1)] == [0, 1, 1, 0]


def test_the_moved_names_are_where_they_were():
    import nsol_amd.primal_dual_solver as pd
    import nsol_amd.stacked_stopping as ss
    import nsol_amd.stopping as st
    for name in ("checked_tolerance", "checked_check_every", "check_points",
                 "relative_changes", "criterion_met", "_StopRule"):
        assert getattr(pd, name) is getattr(st, name)
    assert ss.stretch_bounds is st.stretch_bounds
    assert ss.stretch_bounds(7, 3, [0, 2, 4, 6, 7]) == [0, 2, 3, 4, 6, 7]
    # stacked_stopping imports nothing from primal_dual_solver, at any level
    import ast
    imported = set()
    for node in ast.walk(ast.parse(open(ss.__file__).read())):
        if isinstance(node, ast.ImportFrom):
            imported.add(node.module or "")
            imported.update(a.name for a in node.names)
        elif isinstance(node, ast.Import):
            imported.update(a.name for a in node.names)
    assert imported and not any("primal_dual_solver" in name for name in imported)
    import nsol_amd.stopping as stopping_module
    assert not any("primal_dual_solver" in line for line in
                   open(stopping_module.__file__).read().splitlines()
                   if line.lstrip().startswith(("import ", "from ")))


# ----------------------------------------------------------- the group runner
N, DIM = 6, 2
PLAN = dict(shape=(2, 3), w=(1., 1., 1.), gamma=0.05, flags=0, dim=DIM)


class FakeEntry(object):
    """Stands in for ops.pd_batch_run: logs its operands' sizes, declines call number
    `decline_at` (from 1)."""

    def __init__(self, log, decline_at=None):
        self.log, self.decline_at, self.calls = log, decline_at, 0

    def __call__(self, xbar_in, xbar_out, x, bt, p_in, p_out, members, shape, w, lmbda,
                 sigma, tau, theta, p_is_zero, gamma_huber, flags):
        self.calls += 1
        if self.calls == self.decline_at:
            return None
        assert xbar_in.numel() == xbar_out.numel() == x.numel() == members * N
        assert p_in.numel() == p_out.numel() == members * DIM * N
        assert lmbda.shape == (members,) and sigma.shape == tau.shape == theta.shape
        assert sigma.shape[0] == members and (shape, w) == (PLAN["shape"], PLAN["w"])
        # p counts as zero in the stretch that starts the schedule, and that one
        # starts from the members' start vectors
        assert p_is_zero == (sigma[0, 0] == _first_sigma())
        assert not p_is_zero or bool((xbar_in == x).all())
        self.log.append(("launch", int(x[0]), members, bt.numel(), sigma.shape[1],
                         p_is_zero))
        return 1


def _stack(P, group, strided, bounds, decline_at=None, observed=True):
    import torch
    from nsol_amd.stacked_run import run_stack
    log = []
    # member m's start vector holds m, its observation 10 + m
    x_all = torch.arange(P, dtype=torch.float64).repeat_interleave(N)
    bt = x_all + 10 if strided else torch.full((N,), 10.0, dtype=torch.float64)
    entry = FakeEntry(log, decline_at)
    res = run_stack(
        x_all, bt, None, strided, PLAN, [("ALG2", 8, 0.05)] * P, bounds[-1], group, entry,
        bounds, observe=(lambda m, it: log.append(("observe", m, it))) if observed
        else None, taken=lambda: log.append(("taken",)))
    return res, log, entry


def _first_sigma():
    from nsol_amd.primal_dual_solver import step_schedule
    return step_schedule("ALG2", 8, 1. / 0.05, 1)[0][0]


def test_groups_cover_the_members_with_views_of_their_length():
    res, log, entry = _stack(5, 2, True, [0, 4, 7])
    # (first member, members, bt elements, iterations, p is zero) of every launch
    assert [e[1:] for e in log if e[0] == "launch"] == [
        (0, 2, 2 * N, 4, True), (0, 2, 2 * N, 3, False),
        (2, 2, 2 * N, 4, True), (2, 2, 2 * N, 3, False),
        (4, 1, N, 4, True), (4, 1, N, 3, False)]
    assert res is not None and res.iterations_done == []
    # every member is observed at the end of every stretch of its group
    assert [e[1:] for e in log if e[0] == "observe"] == [
        (0, 4), (1, 4), (0, 7), (1, 7), (2, 4), (3, 4), (2, 7), (3, 7), (4, 4), (4, 7)]
    # the hook fires once, after the first launch and before the first observation
    assert [e[0] for e in log[:3]] == ["launch", "taken", "observe"]
    assert log.count(("taken",)) == 1


def test_shared_operands_are_passed_whole():
    res, log, entry = _stack(5, 2, False, [0, 7], observed=False)
    assert [e[1:4] for e in log if e[0] == "launch"] == [(0, 2, N), (2, 2, N), (4, 1, N)]
    assert [e[0] for e in log] == ["launch", "taken", "launch", "launch"]


def test_a_shared_start_vector_is_copied_to_every_member_of_a_group():
    import torch
    from nsol_amd.stacked_run import run_stack
    log = []
    start = torch.arange(N, dtype=torch.float64) + 5
    x_all = start.repeat(5)
    run_stack(x_all, start + 10, None, False, PLAN, [("ALG2", 8, 0.05)] * 5, 7, 2,
              FakeEntry(log), [0, 7], start=start)
    # (FakeEntry has compared the group's xbar with its x at every first launch)
    assert [e[1:4] for e in log] == [(5, 2, N), (5, 2, N), (5, 1, N)]


def test_a_decline_on_the_first_launch_reports_nothing():
    res, log, entry = _stack(5, 2, True, [0, 4, 7], decline_at=1)
    assert res is None and log == [] and entry.calls == 1


def test_a_decline_on_a_later_launch_raises():
    with pytest.raises(RuntimeError):
        _stack(5, 2, True, [0, 4, 7], decline_at=3)


def test_member_schedules_are_each_members_own():
    from nsol_amd.primal_dual_solver import step_schedule
    from nsol_amd.stacked_run import member_schedules
    members = [("ALG2", 8, 0.05), ("ALG3", 16.0, 0.2), ("ALG2_AHMOD", 8, 0.01)]
    lmbda, sig, ta, th = member_schedules(members, 5)
    assert lmbda.tolist() == [1. / 0.05, 1. / 0.2, 1. / 0.01]
    for m, (alg, L2, alpha) in enumerate(members):
        want = step_schedule(alg, L2, 1. / alpha, 5)
        for got, w in zip((sig[m], ta[m], th[m]), want):
            assert np.array_equal(got, w)


# ------------------------------------------------------ the group-size formula
# (members, n, dim, element size) -> sweep_group_size, batch_group_size,
# weighted_batch_group_size as they were before they shared one formula.  By hand,
# with 256 MiB per group: row 1 has arrays of 4 MiB and 7, 8, 9 of them per member:
# 256 // 28 = 9, 256 // 32 = 8, 256 // 36 = 7; row 3 arrays of 1 MiB and 9, 10, 11 of
# them: 256 // 9 = 28, 256 // 10 = 25, 256 // 11 = 23.
GROUP_SIZES = [
    ((64, 1048576, 2, 4), 9, 8, 7),
    ((3, 1048576, 2, 4), 3, 3, 3),
    ((64, 262144, 3, 4), 28, 25, 23),
    ((64, 16777216, 3, 8), 1, 1, 1),
    ((4096, 2097152, 3, 4), 3, 3, 2),
    ((100000, 16, 1, 4), 100000, 65535, 65535),
    ((1000, 65536, 2, 4), 146, 128, 113),
    ((7, 45, 2, 8), 7, 7, 7),
    ((1, 1, 1, 4), 1, 1, 1),
    ((70000, 1000, 1, 4), 13421, 11184, 9586),
]


@pytest.mark.parametrize("args,sweep,batch,weighted", GROUP_SIZES)
def test_group_sizes_are_what_they_were(args, sweep, batch, weighted):
    from nsol_amd import ops
    assert ops.PD_SWEEP_GROUP_BYTES == ops.PD_BATCH_GROUP_BYTES == 256 << 20
    assert ops.sweep_group_size(*args) == sweep
    assert ops.batch_group_size(*args) == batch
    assert ops.weighted_batch_group_size(*args) == weighted
