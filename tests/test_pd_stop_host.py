"""CPU-only side of the stopping rule of the primal-dual solver: the float64 NumPy
restatement of the loop with the criterion that the GPU tests are held to (built from
oracle.nsol_oracle's functions), the cases with their margins, and the host logic:
check points, the ratios, argument checks, the stacking keys, the declared symbols."""
import os
import re

import numpy as np
import pytest

from test_pd_isotropic_host import project_iso
from test_pd_weighted_host import mixed_weights, prox_weighted

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# A case may not turn on rounding: at every check up to and including the stop,
# max(r_x, r_p) is at least this far (relative) from the tolerance.
MARGIN = 0.03
K = 5
ALLOWED = 400


def observation(shape):
    return 50.0 + 30.0 * np.random.default_rng(sum(shape)).standard_normal(shape)


def ratio(num, den):
    """sqrt(num / den); exactly 0 for a numerator that is exactly 0."""
    if num == 0.:
        return 0.
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sqrt(np.float64(num) / np.float64(den)))


def pd_stop_denoise(obs, shape, reg, data, alg, alpha, L2, iters, tolerance,
                    check_every=K, iso=False, weights=None, margin=MARGIN):
    """The loop of primal_dual_solver.py:232-261 on b = x0 = obs.flatten(), x_scale =
    max, unit spacing, with the criterion: after iteration k = K, 2K, ... and the last,
    r = sqrt(sum (v_k - v_{k-1})^2 / sum v_k^2) for the scaled primal x and the dual p
    (p = 0 before the first iteration); stop if max(r_x, r_p) <= tolerance.  Asserts
    the margin at every check.  Returns dict(x (times x_scale), done, reason,
    changes rows (k, r_x, r_p))."""
    from oracle import nsol_oracle as orc
    b = np.asarray(obs, dtype=np.float64).reshape(-1)
    xs = float(np.max(b))
    bt = b / xs
    w = np.ones(b.size) if weights is None else \
        np.asarray(weights, dtype=np.float64).reshape(-1)
    d = len(shape)
    lmbda = 1. / float(alpha)
    sig, ta, th = orc.pd_schedule(alg, L2, lmbda, iters)
    Z = (d * shape[0],) + tuple(shape[1:]) if d > 1 else shape
    x = bt.copy()
    xbar = x.copy()
    p = np.zeros(d * b.size)
    rows, reason, done = [], "iterations", 0
    for n in range(iters):
        q = p + sig[n] * orc.grad(xbar.reshape(shape), None).reshape(-1)
        if iso:
            pn = project_iso(q, d, 1. + sig[n] * 0.05 if reg == "Huber" else None)
        else:
            pn = orc.prox_huber_conj(q, sig[n]) if reg == "Huber" else \
                orc.prox_tv_conj(q, sig[n])
        u = x - ta[n] * orc.grad_adj(pn.reshape(Z), None).reshape(-1)
        if weights is None:
            xn = orc.prox_ell1_denoising(u, ta[n] * lmbda, bt) if data == "L1" else \
                orc.prox_ell2_denoising(u, ta[n] * lmbda, bt)
        else:
            xn = prox_weighted(u, ta[n] * lmbda, bt, w, data)
        xbar = xn + th[n] * (xn - x)
        k = n + 1
        stop = False
        if k % check_every == 0 or k == iters:
            r_x = ratio(np.sum((xn - x) ** 2), np.sum(xn ** 2))
            r_p = ratio(np.sum((pn - p) ** 2), np.sum(pn ** 2))
            rows.append((float(k), r_x, r_p))
            m = max(r_x, r_p)
            if tolerance > 0 and margin:
                assert abs(m / tolerance - 1.) >= margin, (k, m, tolerance)
            stop = np.isfinite(m) and m <= tolerance
        x, p, done = xn, pn, k
        if stop:
            reason = "tolerance"
            break
    return dict(x=x * xs, done=done, reason=reason,
                changes=np.array(rows).reshape(-1, 3))


# (shape, reg, data, alg, alpha, L2, iso, weighted, tolerance, iterations allowed,
#  stops at, max(r_x, r_p) at the check before, at the stop)
# every figure is this restatement's, in float64 on the CPU; the isotropic and weighted
# cases take their tolerance from {1e-2, 1e-3}, and the comment gives their smallest
# margin over all checks
CASES = [
    ((24, 40), "TV", "L2", "ALG2", 0.05, 8, False, False, 1e-2, ALLOWED, 20, 1.59e-2, 7.7e-3),
    ((24, 40), "TV", "L2", "ALG3", 0.05, 8, False, False, 1e-3, ALLOWED, 35, 1.065e-3, 6.4e-4),
    ((24, 40), "Huber", "L1", "ALG2", 0.6, 8, False, False, 1e-3, ALLOWED, 55, 1.04e-3, 5.5e-4),
    ((9, 12, 21), "TV", "L2", "ALG2", 0.05, 16, False, False, 1e-2, ALLOWED, 30, 1.195e-2, 8.2e-3),
    ((9, 12, 21), "Huber", "L2", "ALG2", 0.05, 16, False, False, 1e-4, ALLOWED, 40, 1.41e-4, 6.6e-5),
    ((70,), "TV", "L2", "ALG2", 0.05, 4, False, False, 1e-3, ALLOWED, 15, 6.0e-3, 7.1e-4),
    ((24, 40), "TV", "L2", "ALG2", 0.05, 8, True, False, 1e-3, ALLOWED, 30, 1.81e-3, 8.96e-4),      # 10.4 %
    ((24, 40), "Huber", "L2", "ALG2", 0.05, 8, False, True, 1e-3, ALLOWED, 30, 1.18e-3, 6.50e-4),   # 18.1 %
    ((24, 40), "Huber", "L1", "ALG2", 0.6, 8, True, True, 1e-2, ALLOWED, 30, 1.30e-2, 7.50e-3),     # 25.0 %
    ((9, 12, 21), "TV", "L2", "ALG2", 0.05, 16, True, False, 1e-2, ALLOWED, 15, 2.61e-2, 7.74e-3),  # 22.6 %
    ((9, 12, 21), "Huber", "L2", "ALG2", 0.05, 16, False, True, 1e-2, ALLOWED, 20, 1.95e-2, 6.81e-3),  # 31.9 %
    ((9, 12, 21), "Huber", "L1", "ALG2", 0.6, 16, True, True, 1e-3, ALLOWED, 60, 1.445e-3, 8.87e-4),   # 11.3 %
    ((33, 260), "TV", "L2", "ALG2", 0.05, 8, True, True, 1e-2, ALLOWED, 25, 1.36e-2, 8.19e-3),      # 18.1 %
]
NEVER = ((24, 40), "TV", "L2", "ALG2_AHMOD", 0.05, 8, False, False, 1e-3, 60)

_cache = {}


def case_weights(shape, weighted):
    return mixed_weights(shape, sum(shape)) if weighted else None


def reference(case, tolerance=None, iters=None):
    """The restatement's result for a case (computed once per session)."""
    shape, reg, data, alg, alpha, L2, iso, weighted, tol, allowed = case[:10]
    tol = tol if tolerance is None else tolerance
    allowed = allowed if iters is None else iters
    key = (shape, reg, data, alg, alpha, L2, iso, weighted, tol, allowed)
    if key not in _cache:
        _cache[key] = pd_stop_denoise(
            observation(shape), shape, reg, data, alg, alpha, L2, allowed, tol,
            iso=iso, weights=case_weights(shape, weighted))
    return _cache[key]


# ------------------------------------------------------------------- its check
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s%s-%s%s%s-%g" % (
    "x".join(map(str, c[0])), c[1], c[2], c[3], "-iso" if c[6] else "",
    "-w" if c[7] else "", c[8]))
def test_restatement_stops_where_the_table_says(case):
    ref = reference(case)             # (asserts the 3 % margin at every check)
    stop_at, before, at = case[10:13]
    assert ref["reason"] == "tolerance" and ref["done"] == stop_at
    rows = ref["changes"]
    assert list(rows[:, 0]) == list(range(K, stop_at + 1, K))
    # the table's figures are rounded to two to four digits
    assert max(rows[-2, 1:]) == pytest.approx(before, rel=2e-2)
    assert max(rows[-1, 1:]) == pytest.approx(at, rel=2e-2)
    assert max(rows[-2, 1:]) > case[8] >= max(rows[-1, 1:])


def test_restatement_runs_out_where_the_change_stays_large():
    ref = reference(NEVER)
    assert ref["reason"] == "iterations" and ref["done"] == 60
    rows = ref["changes"]
    assert list(rows[:, 0]) == list(range(5, 61, 5))
    assert rows[9, 0] == 50 and rows[9, 2] == pytest.approx(4.5e-2, rel=2e-2)


def test_restatement_without_a_stop_is_the_oracle_loop():
    from oracle import nsol_oracle as orc
    shape = (9, 12, 21)
    obs = observation(shape)
    ours = pd_stop_denoise(obs, shape, "Huber", "L2", "ALG2", 0.05, 16, 23, 1e-300,
                           margin=0)
    want = orc.primal_dual_denoise(obs.reshape(-1), shape, "Huber", "L2", 0.05, 23, 16,
                                   "ALG2")
    assert ours["done"] == 23 and ours["reason"] == "iterations"
    assert list(ours["changes"][:, 0]) == [5, 10, 15, 20, 23]
    assert np.linalg.norm(ours["x"] - want) / np.linalg.norm(want) <= 1e-12


# ------------------------------------------------------------------ host logic
def _wired(obs, **kw):
    import nsol_amd.linear_operators as LO
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd.proximal_operators import ProximalOperators as prox
    from nsol_amd.symbolic import Sym
    lo = {1: LO.LinearOperators1D, 2: LO.LinearOperators2D,
          3: LO.LinearOperators3D}[obs.ndim]()
    grad, grad_adj = lo.get_gradient_operators()
    X = obs.shape
    Z = grad(Sym(X)).shape
    b = obs.flatten()
    D = lambda x: grad(x.reshape(*X)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    pf = lambda x, tau: prox.prox_ell2_denoising(x, tau, x0=b, x_scale=3.)
    return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=prox.prox_tv_conj, B=D, B_conj=Da,
                               L2=16, x0=b, x_scale=3., alpha=0.05, iterations=7,
                               dtype=np.float64, **kw)


def test_check_points():
    from nsol_amd.primal_dual_solver import check_points
    assert check_points(23, 5) == [5, 10, 15, 20, 23]
    assert check_points(20, 5) == [5, 10, 15, 20]
    assert check_points(3, 10) == [3]
    assert check_points(4, 1) == [1, 2, 3, 4]
    assert check_points(0, 5) == []


def test_ratios_and_criterion():
    from nsol_amd.primal_dual_solver import criterion_met, relative_changes
    r_x, r_p = relative_changes([4.0, 16.0, 1.0, 100.0])
    assert r_x == 0.5 and r_p == 0.1
    # a numerator that is exactly 0 counts as 0, whatever the denominator
    assert relative_changes([0.0, 0.0, 0.0, 5.0]) == (0.0, 0.0)
    assert criterion_met(0.0, 0.0, 0.0)
    # a change from nothing: not met
    r_x, r_p = relative_changes([1.0, 0.0, 0.0, 1.0])
    assert r_x == float("inf") and not criterion_met(r_x, r_p, 1e300)
    # sums that are NaN or infinite never meet the criterion
    for bad in (float("nan"), float("inf")):
        for j in range(4):
            sums = [1e-12, 1.0, 1e-12, 1.0]
            sums[j] = bad
            assert not criterion_met(*relative_changes(sums), tolerance=float("inf"))
    assert criterion_met(1e-3, 9e-4, 1e-3) and not criterion_met(1e-3, 1.1e-3, 1e-3)


def test_arguments_and_accessors():
    obs = 1.0 + np.arange(30.0).reshape(5, 6)
    s = _wired(obs)
    assert s.get_tolerance() is None and s.get_check_every() == 10
    assert s.get_iterations_done() is None and s.get_stop_reason() is None
    assert s.get_changes().shape == (0, 3)
    s = _wired(obs, tolerance=1e-3, check_every=5)
    assert s.get_tolerance() == 1e-3 and s.get_check_every() == 5
    s.set_tolerance(0)
    s.set_check_every(1)
    assert s.get_tolerance() == 0.0 and s.get_check_every() == 1
    s.set_tolerance(None)
    assert s.get_tolerance() is None
    for bad in (-1e-3, float("nan"), -float("inf")):
        with pytest.raises(ValueError):
            _wired(obs, tolerance=bad)
        with pytest.raises(ValueError):
            s.set_tolerance(bad)
    for bad in (0, -3, 2.5, float("nan")):
        with pytest.raises(ValueError):
            _wired(obs, check_every=bad)
        with pytest.raises(ValueError):
            s.set_check_every(bad)
    # the keywords come after dtype
    import inspect
    import nsol_amd.primal_dual_solver as pd
    names = list(inspect.signature(pd.PrimalDualSolver.__init__).parameters)
    assert names[-3:] == ["dtype", "tolerance", "check_every"]


def test_a_solver_with_a_tolerance_does_not_join_a_stack():
    from nsol_amd.parameter_sweep import PrimalDualSweep
    from nsol_amd.solver_batch import member_key, plan_stacks
    obs = 1.0 + np.arange(30.0).reshape(5, 6)
    solvers = [_wired(obs), _wired(obs, tolerance=1e-3), _wired(obs),
               _wired(obs, tolerance=1e-3)]
    keys = [member_key(s, s.plan()) for s in solvers]
    assert keys[1] is None and keys[3] is None and keys[0] == keys[2] is not None
    assert plan_stacks(keys) == [[0, 2]]
    t = solvers[1]
    with pytest.raises(ValueError):
        PrimalDualSweep(t._prox_f, t._prox_g_conj, t._B, t._B_conj, 16, obs.flatten(),
                        {"alpha": [0.1, 0.2]}, tolerance=-1.0)
    with pytest.raises(ValueError):
        PrimalDualSweep(t._prox_f, t._prox_g_conj, t._B, t._B_conj, 16, obs.flatten(),
                        {"alpha": [0.1, 0.2]}, tolerance=1e-3, check_every=0)
    sw = PrimalDualSweep(t._prox_f, t._prox_g_conj, t._B, t._B_conj, 16, obs.flatten(),
                         {"alpha": [0.1, 0.2]}, tolerance=1e-3, check_every=5)
    member = sw._solver(sw._members[1])
    assert member.get_tolerance() == 1e-3 and member.get_check_every() == 5


def test_header_library_and_binding_agree_on_the_new_entries():
    import ctypes
    from nsol_amd import _lib
    from nsol_amd.build import SOURCES, build_library
    assert "nsol_pdc.hip" in SOURCES
    decl = _lib.declared_symbols()
    raw = ctypes.CDLL(build_library())
    for base in ("pd_check_iter", "pd_change"):
        for suf in ("f32", "f64"):
            name = "nsol_%s_%s" % (base, suf)
            assert name in decl and hasattr(raw, name)
    # nsol_pd_fused_iter's arguments + wt, ws, ws_doubles, row
    assert len(decl["nsol_pd_check_iter_f32"][1]) == \
        len(decl["nsol_pd_fused_iter_f32"][1]) + 4
    assert len(decl["nsol_pd_change_f64"][1]) == 10
    text = open(os.path.join(ROOT, "include", "nsol_hip.h")).read()
    assert re.search(r"int64_t\s+nsol_pd_check_ws_doubles\s*\(", text)
    ws = _lib.load().nsol_pd_check_ws_doubles
    assert ws(4, 3, 512, 512, 512) >= 4 * 4096 and ws(8, 1, 1, 1, 70) >= 4 * 4096
    assert ws(4, 2, 1, 8192, 8192) >= 4 * 32768        # one partial per workgroup
    assert ws(4, 2, 64, 64, 64) == -1 and ws(2, 1, 1, 1, 8) == -1
    assert ws(4, 3, 2048, 2048, 2048) == -1            # more than 2^31 voxels


def test_command_lines_take_the_tolerance(capsys):
    from nsol_amd.application import run_deconvolution, run_denoising
    for tool in (run_denoising, run_deconvolution):
        with pytest.raises(SystemExit):
            tool.main(["--help"])
        out = capsys.readouterr().out
        assert "--tolerance" in out and "--check-every" in out
    with pytest.raises(SystemExit):
        run_denoising.main(["--observation", "a", "--result", "b", "--tolerance", "-1"])
    with pytest.raises(SystemExit):
        run_deconvolution.main(["--observation", "a", "--result", "b", "--solver",
                                "ADMM", "--tolerance", "1e-3"])
    capsys.readouterr()
