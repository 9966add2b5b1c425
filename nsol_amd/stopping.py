"""The stopping rule of the primal-dual solvers: its arguments, check points and
ratios, the device board of one run (_StopRule), the bounds of the stretches a run is
enqueued in, and what a solver with the rule exposes (Stopping).

After iteration k = check_every, 2 check_every, ... and the last,

    r_x = sqrt(sum (x_k - x_{k-1})^2 / sum x_k^2),   r_p likewise for the dual p

(p = 0 before the first iteration; a ratio whose numerator is exactly 0 counts as 0;
sums that are not finite never meet the criterion) and the run stops if
max(r_x, r_p) <= tolerance.
"""
import numpy as np

from . import ops


def checked_tolerance(tolerance):
    """None, or the tolerance as a float >= 0 (ValueError for a negative one or NaN)."""
    if tolerance is None:
        return None
    tolerance = float(tolerance)
    if not tolerance >= 0.:
        raise ValueError("tolerance must be None or a number >= 0")
    return tolerance


def checked_check_every(check_every):
    """check_every as an int >= 1 (ValueError otherwise)."""
    try:
        k = int(check_every)
        ok = k >= 1 and k == check_every
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("check_every must be a positive integer")
    return k


def check_points(iterations, check_every):
    """Iterations after which the stopping rule is evaluated: check_every,
    2 check_every, ... and always the last."""
    iterations, check_every = int(iterations), int(check_every)
    if iterations < 1:
        return []
    pts = list(range(check_every, iterations + 1, check_every))
    if not pts or pts[-1] != iterations:
        pts.append(iterations)
    return pts


def stretch_bounds(iterations, check_every, observer_points=None):
    """The bounds of the stretches a run with the rule is enqueued in: the check points
    merged with a device-mode observer's points."""
    return sorted(set([0]) | set(observer_points or []) |
                  set(check_points(iterations, check_every)))


def next_slot(k, slot):
    """The half of the ping-pong arrays that holds the state after a launch that
    started from half k and reports `slot`: 0 where it started, 1 in the other."""
    return k if slot == 0 else 1 - k


def relative_changes(sums):
    """(r_x, r_p) from the four sums {sum dx^2, sum x^2, sum dp^2, sum p^2}: a ratio
    whose numerator is exactly 0 is 0; NaN where a sum is not finite."""
    out = []
    for num, den in ((sums[0], sums[1]), (sums[2], sums[3])):
        num, den = float(num), float(den)
        if not (np.isfinite(num) and np.isfinite(den)):
            out.append(float("nan"))
        elif num == 0.:
            out.append(0.)
        elif den == 0.:
            out.append(float("inf"))
        else:
            out.append(float(np.sqrt(num / den)))
    return out[0], out[1]


def criterion_met(r_x, r_p, tolerance):
    """max(r_x, r_p) <= tolerance; never with a NaN among them."""
    return bool(np.isfinite(r_x) and np.isfinite(r_p) and
                max(r_x, r_p) <= tolerance)


class _StopRule(object):
    """The stopping rule of one run: its check points, the device workspace and
    board (one row of four sums per check) and the rows (k, r_x, r_p) read so far."""

    def __init__(self, tolerance, iterations, check_every):
        self.tolerance = float(tolerance)
        self.points = check_points(iterations, check_every)
        self._index = {p: j for j, p in enumerate(self.points)}
        self.ws = self.board = None
        self.rows = []

    def allocate(self, like, shape=None):
        """shape: the volume of the fused kernels (None: nsol_pd_change_* only)."""
        import torch
        if shape is not None:
            self.ws = ops.pd_check_workspace(like, shape)
        else:
            self.ws = torch.empty(ops.PD_CHECK_SUMS * 4096, dtype=torch.float64,
                                  device=like.device)
        self.board = torch.empty((max(len(self.points), 1), ops.PD_CHECK_SUMS),
                                 dtype=torch.float64, device=like.device)

    def is_point(self, it):
        return it in self._index

    def row(self, it):
        return self.board[self._index[it]]

    def decide(self, it):
        """Reads the row of check `it` back (this waits for the device) and says
        whether the run stops."""
        r_x, r_p = relative_changes(self.row(it).cpu().numpy())
        self.rows.append((float(it), r_x, r_p))
        return criterion_met(r_x, r_p, self.tolerance)


class Stopping(object):
    """What a solver with the stopping rule exposes (mixed into the Solver classes):
    tolerance and check_every, and after run() the iterations done, the reason and the
    rows of the checks."""
    _tolerance = _rule = _iterations_done = _stop_reason = None
    _check_every = 10

    def set_tolerance(self, tolerance):
        """None: run all `iterations`; else stop once max(r_x, r_p) <= tolerance."""
        self._tolerance = checked_tolerance(tolerance)

    def get_tolerance(self):
        return self._tolerance

    def set_check_every(self, check_every):
        self._check_every = checked_check_every(check_every)

    def get_check_every(self):
        return self._check_every

    def get_iterations_done(self):
        """Iterations the last run() did (None before one)."""
        return self._iterations_done

    def get_stop_reason(self):
        """'tolerance' or 'iterations' after run() (None before)."""
        return self._stop_reason

    def get_changes(self):
        """One row (k, r_x, r_p) per check of the last run()."""
        rows = self._rule.rows if self._rule is not None else []
        return np.array(rows, dtype=np.float64).reshape(-1, 3)

    def _start_rule(self, iterations, rule=_StopRule):
        """The rule of the run that begins (None without a tolerance)."""
        self._rule = None if self._tolerance is None else rule(
            self._tolerance, iterations, self._check_every)
        self._iterations_done, self._stop_reason = 0, "iterations"
        return self._rule

    def _stops_after(self, it):
        """Bookkeeping after iteration `it`; True when the run has a tolerance, the
        rule was evaluated there and the run stops."""
        rule = self._rule
        if rule is None:
            return False
        self._iterations_done = it
        if rule.is_point(it) and rule.decide(it):
            self._stop_reason = "tolerance"
            return True
        return False
