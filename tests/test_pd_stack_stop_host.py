"""CPU-only side of the stacked runs that stop member by member: the declared symbols,
the stacking key of solvers with a tolerance, the opt-in keywords, and the map
bookkeeping of stacked_stopping.run_group against a fake device that fabricates the
sums."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from test_pd_stop_host import _wired

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ------------------------------------------------------------ the C interface
def test_header_library_and_binding_agree_on_the_stack_entries():
    from nsol_amd import _lib
    from nsol_amd.build import SOURCES, build_library
    assert "nsol_pdm.hip" in SOURCES
    decl = _lib.declared_symbols()
    raw = ctypes.CDLL(build_library())
    for name in ("nsol_pd_stack_iter_f32", "nsol_pd_stack_iter_f64",
                 "nsol_pd_stack_launches"):
        assert name in decl and hasattr(raw, name)
    assert hasattr(raw, "nsol_pd_stack_ws_doubles")
    # nsol_pd_weighted_iter's arguments + map, active, ws, ws_doubles, rows
    for suf in ("f32", "f64"):
        assert len(decl["nsol_pd_stack_iter_" + suf][1]) == \
            len(decl["nsol_pd_weighted_iter_" + suf][1]) + 5 == 26
    assert decl["nsol_pd_stack_launches"][1] == []
    text = open(os.path.join(ROOT, "include", "nsol_hip.h")).read()
    assert re.search(r"int64_t\s+nsol_pd_stack_ws_doubles\s*\(", text)
    ws = _lib.load().nsol_pd_stack_ws_doubles
    one = ws(4, 2, 1, 24, 40, 1)
    assert one >= 4 and one % 4 == 0
    assert ws(4, 2, 1, 24, 40, 7) == 7 * one          # one active member plans the most
    assert ws(8, 3, 9, 12, 21, 3) == 3 * ws(8, 3, 9, 12, 21, 1) > 0
    assert ws(4, 2, 1, 8192, 8192, 2) >= 2 * 4 * 32768   # one partial per workgroup
    assert ws(2, 1, 1, 1, 8, 1) == -1 and ws(4, 2, 64, 64, 64, 1) == -1
    assert ws(4, 1, 1, 1, 8, 0) == -1 and ws(4, 1, 1, 1, 8, 65536) == -1
    assert ws(4, 3, 1024, 1024, 1024, 3) == -1        # all members: more than 2^31 voxels
    from nsol_amd import ops
    for name in ("pd_stack_iter", "pd_stack_workspace", "pd_stack_launches"):
        assert callable(getattr(ops, name))


# ------------------------------------------------------------------ the keys
def test_stopping_member_key():
    from nsol_amd.solver_batch import member_key, plan_stacks, stopping_member_key
    obs = 1.0 + np.arange(30.0).reshape(5, 6)
    solvers = [_wired(obs),                                    # 0 no tolerance
               _wired(obs, tolerance=1e-3, check_every=5),     # 1
               _wired(obs, tolerance=1e-5, check_every=5),     # 2 another tolerance
               _wired(obs, tolerance=1e-3, check_every=4),     # 3 another check_every
               _wired(obs),                                    # 4 no tolerance
               _wired(obs, tolerance=1e-3, check_every=4),     # 5
               _wired(obs, tolerance=1e-3, check_every=5, verbose=1)]   # 6 verbose
    plans = [s.plan() for s in solvers]
    keys = [stopping_member_key(s, p) for s, p in zip(solvers, plans)]
    assert keys[0] is None and keys[4] is None          # no tolerance: never this key
    assert keys[1] == keys[2] is not None               # tolerances may differ
    assert keys[3] == keys[5] is not None and keys[3] != keys[1]   # check_every may not
    assert keys[6] is None                              # sequential for another reason
    assert plan_stacks(keys) == [[1, 2], [3, 5]]
    # a solver with a tolerance and one without never share a key of either kind
    plain = [member_key(s, p) for s, p in zip(solvers, plans)]
    assert all(plain[i] is None for i in (1, 2, 3, 5, 6))
    assert plain[0] == plain[4] is not None
    assert not set(k for k in keys if k is not None) & \
        set(k for k in plain if k is not None)
    assert solvers[1]._tolerance == 1e-3                # the key leaves the solver alone
    assert stopping_member_key(solvers[1], None) is None
    # member_key's own fields separate as before: another shape
    other = _wired(1.0 + np.arange(30.0).reshape(6, 5), tolerance=1e-3, check_every=5)
    assert stopping_member_key(other, other.plan()) != keys[1]


def test_the_option_is_accepted_and_off_by_default():
    from nsol_amd.parameter_sweep import PrimalDualSweep
    from nsol_amd.solver_batch import PrimalDualBatch
    obs = 1.0 + np.arange(30.0).reshape(5, 6)
    solvers = [_wired(obs, tolerance=1e-3), _wired(obs, tolerance=1e-3)]
    assert PrimalDualBatch(solvers, stacked_stopping=True)._stacked_stopping is True
    assert PrimalDualBatch(solvers)._stacked_stopping is False
    t = solvers[0]
    args = (t._prox_f, t._prox_g_conj, t._B, t._B_conj, 16, obs.flatten(),
            {"alpha": [0.1, 0.2]})
    sw = PrimalDualSweep(*args, tolerance=1e-3, check_every=5, stacked_stopping=True)
    assert sw._stacked_stopping is True
    assert PrimalDualSweep(*args, tolerance=1e-3)._stacked_stopping is False
    for cls in (PrimalDualBatch, PrimalDualSweep):
        par = inspect.signature(cls.__init__).parameters
        assert list(par)[-1] == "stacked_stopping"
        assert par["stacked_stopping"].default is False


# ------------------------------------------------- the group runner's bookkeeping
TOL = 1e-3


class FakeDevice(object):
    """Stands in for stacked_stopping.StackDevice.  stop_at[m]: the check (iteration
    count) from which member m's fabricated change is below TOL / 2; before it, and
    for members not listed, it is 2 TOL.  Rows of members outside the map are NaN."""

    def __init__(self, members, stop_at, decline=False):
        self.members, self.stop_at, self.decline = members, stop_at, decline
        self.ws, self.rows = object(), object()
        self.board = np.full((members, 4), np.nan)
        self.uploads, self.launches, self.reads = [], [], 0

    def upload_map(self, active):
        active = list(active)
        assert active == sorted(set(active)) and active    # strictly increasing
        assert 0 <= active[0] and active[-1] < self.members
        self.uploads.append(active)
        return active

    def iter(self, xbar_in, xbar_out, x, bt, wt, p_in, p_out, members, map, active,
             shape, w, tab, iteration, flags, ws=None, rows=None):
        if self.decline:
            return False
        assert members == self.members and active == len(map) >= 1
        assert (ws is None) == (rows is None)
        assert rows is None or (ws is self.ws and rows is self.rows)
        # the slots alternate in lockstep: iteration k reads slot k & 1
        assert (xbar_in, xbar_out) == ("xb%d" % (iteration & 1),
                                       "xb%d" % (1 - (iteration & 1)))
        assert (p_in, p_out) == ("p%d" % (iteration & 1), "p%d" % (1 - (iteration & 1)))
        self.launches.append((iteration, tuple(map), rows is not None))
        if rows is not None:
            self.board[:] = np.nan
            for m in map:
                r = TOL / 2 if iteration + 1 >= self.stop_at.get(m, 1 << 30) else 2 * TOL
                self.board[m] = [r * r, 1.0, r * r / 4, 1.0]      # r_x = r, r_p = r / 2
        return True

    def read_rows(self):
        self.reads += 1
        return self.board.copy()


def _run(members, stop_at, iters, every, tolerances=None, observer_points=None,
         observe=None, decline=False):
    from nsol_amd.stacked_stopping import run_group, stretch_bounds
    dev = FakeDevice(members, stop_at, decline)
    res = run_group("x", ["xb0", "xb1"], ["p0", "p1"], "bt", None, members, (5, 6),
                    (1., 1., 1.), "tab", 0, tolerances or [TOL] * members, every, iters,
                    stretch_bounds(iters, every, observer_points), observe=observe,
                    device=dev)
    return res, dev


def test_first_middle_and_last_member_retire():
    res, dev = _run(5, {0: 10, 2: 20, 4: 30}, 40, 10)
    assert dev.uploads == [[0, 1, 2, 3, 4], [1, 2, 3, 4], [1, 3, 4], [1, 3]]
    assert res.iterations_done == [10, 40, 20, 40, 30]
    assert res.stop_reason == ["tolerance", "iterations", "tolerance", "iterations",
                               "tolerance"]
    assert [len(c) for c in res.changes] == [1, 4, 2, 4, 3]
    assert res.changes[2] == [(10.0, 2 * TOL, TOL), (20.0, TOL / 2, TOL / 4)]
    assert dev.reads == 4                               # one read-back per check
    assert [l[0] for l in dev.launches] == list(range(40))      # one launch per iteration
    for it, active, checked in dev.launches:
        assert checked == ((it + 1) % 10 == 0)
        assert active == tuple(dev.uploads[it // 10])
    # a retired member is in no later map
    for m, k in ((0, 10), (2, 20), (4, 30)):
        assert all(m not in a for it, a, _ in dev.launches if it >= k)


def test_all_members_retire_at_one_check_and_the_loop_ends():
    res, dev = _run(4, {m: 15 for m in range(4)}, 400, 5)
    assert res.iterations_done == [15] * 4 and res.stop_reason == ["tolerance"] * 4
    assert len(dev.launches) == 15 and dev.reads == 3
    assert dev.uploads == [[0, 1, 2, 3]]                # nothing uploaded for an empty map
    assert [c[-1][0] for c in res.changes] == [15.0] * 4


def test_no_member_retires():
    res, dev = _run(3, {}, 23, 5)
    assert res.iterations_done == [23] * 3 and res.stop_reason == ["iterations"] * 3
    assert dev.uploads == [[0, 1, 2]] and len(dev.launches) == 23
    assert [it + 1 for it, _, chk in dev.launches if chk] == [5, 10, 15, 20, 23]
    assert [r[0] for r in res.changes[1]] == [5.0, 10.0, 15.0, 20.0, 23.0]
    assert dev.reads == 5


def test_the_last_member_to_run_ends_the_loop_when_it_retires():
    res, dev = _run(3, {0: 5, 1: 10, 2: 20}, 100, 5)
    assert res.iterations_done == [5, 10, 20]
    assert dev.uploads == [[0, 1, 2], [1, 2], [2]]
    assert len(dev.launches) == 20 and dev.launches[-1] == (19, (2,), True)


def test_every_member_is_held_to_its_own_tolerance():
    # the fabricated change is 2 TOL until check 10 and TOL / 2 from it
    res, dev = _run(4, {m: 10 for m in range(4)}, 30, 5,
                    tolerances=[3 * TOL, TOL, TOL / 4, 1e-300])
    assert res.iterations_done == [5, 10, 30, 30]
    assert res.stop_reason == ["tolerance", "tolerance", "iterations", "iterations"]
    assert dev.uploads == [[0, 1, 2, 3], [1, 2, 3], [2, 3]]


def test_observer_points_are_merged_and_a_retired_member_is_not_observed_again():
    from nsol_amd.stacked_stopping import stretch_bounds
    assert stretch_bounds(23, 5) == [0, 5, 10, 15, 20, 23]
    assert stretch_bounds(20, 10, [0, 4, 8, 12, 16, 20]) == [0, 4, 8, 10, 12, 16, 20]
    seen = []
    res, dev = _run(3, {1: 10}, 20, 10, observer_points=[0, 4, 8, 12, 16, 20],
                    observe=lambda m, it: seen.append((m, it)))
    assert res.iterations_done == [20, 10, 20]
    assert [it for m, it in seen if m == 0] == [4, 8, 10, 12, 16, 20]
    assert [it for m, it in seen if m == 1] == [4, 8, 10]       # observed at its stop
    # the checks fall where they fall without an observer
    assert [it + 1 for it, _, chk in dev.launches if chk] == [10, 20]
    assert len(dev.launches) == 20


def test_a_decline_on_the_first_launch_reports_nothing():
    res, dev = _run(3, {}, 20, 5, decline=True)
    assert res is None and dev.reads == 0
