"""Every way PrimalDualSolver.run() enqueues a fused run -- plain, pitched, weighted,
with a tolerance, observed on the device, observed with host copies, verbose -- against
a loop written out here from the one-iteration entries, through the public interface
only; and a sweep and a stack of three members, in one group and in two, against their
members' own runs.  Seven iterations with check_every = 3: the checks fall after 3, 6
and 7, the last stretch is a single checked iteration, and with an observer every 2 the
stretches are bounded by 0, 2, 3, 4, 6, 7."""
import itertools

import numpy as np
import pytest

from test_pd_stop_host import observation, pd_stop_denoise
from test_pd_stretches_host import (ALG, ALPHA, CHECKS, EVERY, ITERS, NEVER, SHAPES,
                                    STACK_ALPHAS, STACK_SHAPE, form_reg, form_weights,
                                    member_obs, met_at_the_second_check)

pytestmark = pytest.mark.gpu

OBSERVE_EVERY = 2
# a measure on the device differs from NumPy's on the same iterate by the rounding of
# x * x_scale to the working type (2^-24 per element in float32) and of float64 sums:
# orders below this, while consecutive iterates of these runs differ by more
MEASURE_RTOL = 1e-5


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _wiring(obs, reg, iso, weights):
    """Callables of run_denoising.py:95-154 on b = x0 = obs, x_scale = max(obs)."""
    import nsol_amd.linear_operators as LO
    from nsol_amd.proximal_operators import ProximalOperators as prox
    shape = obs.shape
    b = obs.flatten()
    xs = float(np.max(b))
    dim = len(shape)
    lo = {1: LO.LinearOperators1D, 2: LO.LinearOperators2D,
          3: LO.LinearOperators3D}[dim]()
    grad, grad_adj = lo.get_gradient_operators()
    Z = grad(b.reshape(shape)).shape
    D = lambda x: grad(x.reshape(*shape)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    if weights is None:
        pf = lambda x, tau: prox.prox_ell2_denoising(x, tau, x0=b, x_scale=xs)
    else:
        w = weights.flatten()
        pf = lambda x, tau: prox.prox_ell2_denoising_weighted(x, tau, x0=b, weights=w,
                                                              x_scale=xs)
    if not iso:
        pg = prox.prox_huber_conj if reg == "Huber" else prox.prox_tv_conj
    elif reg == "Huber":
        pg = lambda x, s: prox.prox_huber_conj_isotropic(x, s, dim)
    else:
        pg = lambda x, s: prox.prox_tv_conj_isotropic(x, s, dim)
    return dict(prox_f=pf, prox_g_conj=pg, B=D, B_conj=Da), b, xs


def _solver(obs, reg, iso, weights, dtype, alpha=ALPHA, **kw):
    import nsol_amd.primal_dual_solver as pd
    calls, b, xs = _wiring(obs, reg, iso, weights)
    return pd.PrimalDualSolver(L2=4 * obs.ndim, x0=b, alpha=alpha, iterations=ITERS,
                               x_scale=xs, alg_type=ALG, dtype=dtype, check_every=EVERY,
                               **dict(calls, **kw))


# ------------------------------------------------- the loop of one-iteration entries
def entries_loop(solver, obs, dtype, checks):
    """ITERS iterations launched one by one from the solver's plan(): pd_check_iter
    at the iterations in `checks`, else pd_fused_iter, or pd_weighted_iter from one
    pd_weighted_table.  Returns ([x_0, ... x_ITERS] device, solver units; rows
    (k, r_x, r_p) of the checks)."""
    import torch
    from nsol_amd import ops
    from nsol_amd.device import to_device
    from nsol_amd.primal_dual_solver import relative_changes, step_schedule
    from nsol_amd.proximal_operators import scaled_data_on_device, weights_on_device
    plan = solver.plan()
    shape, w, flags, gamma = plan["shape"], plan["w"], plan["flags"], plan["gamma"]
    xs = solver.get_x_scale()
    x = ops.scale(to_device(obs.reshape(-1), dtype), xs, divide=True)
    n, dim = x.numel(), plan["dim"]
    bt = scaled_data_on_device(plan["data"], plan["data_scale"], x)
    weighted = bool(flags & ops.PD_DATA_WEIGHTED)
    wt = weights_on_device(plan["weights"], x) if weighted else None
    lmbda = 1. / solver.get_alpha()
    sig, ta, th = step_schedule(solver.get_alg_type(), solver.get_L2(), lmbda, ITERS)
    xbar = [x.clone(), torch.empty_like(x)]
    p = [torch.empty(dim * n, dtype=x.dtype, device=x.device) for _ in range(2)]
    tab = ops.pd_weighted_table(x, 1, [lmbda], sig, ta, th, True, gamma, flags) \
        if weighted else None
    ws = ops.pd_check_workspace(x, shape)
    board = torch.zeros((ITERS, ops.PD_CHECK_SUMS), dtype=torch.float64, device=x.device)
    iterates = [x.clone()]
    for i in range(ITERS):
        k = i & 1
        hden = 1. + sig[i] * gamma if flags & ops.PD_REG_HUBER else 1.
        if i + 1 in checks:
            assert ops.pd_check_iter(xbar[k], xbar[1 - k], x, bt, wt,
                                     None if i == 0 else p[k], p[1 - k], shape, w,
                                     sig[i], hden, ta[i], ta[i] * lmbda, th[i], flags, ws,
                                     board[i])
        elif weighted:
            assert ops.pd_weighted_iter(xbar[k], xbar[1 - k], x, bt, wt, p[k], p[1 - k],
                                        1, shape, w, tab, i, flags)
        else:
            ops.pd_fused_iter(xbar[k], xbar[1 - k], x, bt, None if i == 0 else p[k],
                              p[1 - k], shape, w, sig[i], hden, ta[i], ta[i] * lmbda,
                              th[i], flags)
        iterates.append(x.clone())
    sums = board.cpu().numpy()
    rows = [(float(k),) + relative_changes(sums[k - 1]) for k in checks]
    return iterates, np.array(rows, dtype=np.float64).reshape(-1, 3)


def _caller_units(x, xs):
    from nsol_amd import ops
    from nsol_amd.device import to_numpy
    return to_numpy(ops.scale(x, xs))


OBSERVATIONS = ["none", "device", "host", "verbose"]
TOLERANCES = ["none", "never", "met"]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_every_form_of_a_run_is_the_loop_of_single_iterations(
        nsol, monkeypatch, capsys, weighted, iso, shape, dtype):
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd import ops
    from nsol_amd.observer import Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    obs, reg, weights = observation(shape), form_reg(shape), form_weights(shape, weighted)
    tol_met, restated = met_at_the_second_check(obs, reg, iso, weights)
    make = lambda **kw: _solver(obs, reg, iso, weights, dtype, **kw)
    xs = make().get_x_scale()
    unchecked, none = entries_loop(make(), obs, dtype, [])
    iterates, rows = entries_loop(make(), obs, dtype, CHECKS)
    assert none.shape == (0, 3)
    for a, b in zip(unchecked, iterates):       # the checking form changes no bit
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    print("rows", rows, "tolerance", tol_met, "restated", restated["changes"])
    # the device's decision is the restatement's: met at the second check, not before
    assert max(rows[0, 1:]) > tol_met >= max(rows[1, 1:])
    host = [_caller_units(x, xs) for x in iterates]
    ref_img = np.roll(obs.flatten(), 1)
    rmse = [float(np.sqrt(np.mean((h - ref_img) ** 2))) for h in host]

    monkeypatch.setattr(pd, "PITCH_MIN_VOXELS", 1)
    # (only a run that has completed on pitched arrays calls ops.from_pitched: an
    # attempt the library declined falls back to contiguous arrays before it)
    pitched = []
    from_pitched = ops.from_pitched
    monkeypatch.setattr(ops, "from_pitched",
                        lambda *a, **kw: pitched.append(1) or from_pitched(*a, **kw))
    for tolerance, observe in itertools.product(TOLERANCES, OBSERVATIONS):
        label = (tolerance, observe)
        done = CHECKS[1] if tolerance == "met" else ITERS
        want_rows = rows[:0] if tolerance == "none" else rows[rows[:, 0] <= done]
        s = make(tolerance={"none": None, "never": NEVER, "met": tol_met}[tolerance],
                 verbose=1 if observe == "verbose" else 0)
        o = None
        if observe in ("device", "host"):
            o = Observer(keep_iterates=False, every=OBSERVE_EVERY) \
                if observe == "device" else Observer()
            o.set_measures({"RMSE": lambda x: sm.similarity_measures["RMSE"](x, ref_img)})
            s.set_observer(o)
        del pitched[:]
        capsys.readouterr()
        before = ops.pd_weighted_launches(), ops.pd_check_launches()
        s.run()
        launched = (ops.pd_weighted_launches() - before[0],
                    ops.pd_check_launches() - before[1])
        printed = [line for line in capsys.readouterr().out.splitlines()
                   if line.startswith("Primal-Dual iteration")]
        assert s.get_execution() == "fused", label
        assert s.get_iterations_done() == done, label
        assert s.get_stop_reason() == ("tolerance" if tolerance == "met"
                                       else "iterations"), label
        assert np.array_equal(s.get_x(), host[done]), label
        assert np.array_equal(s.get_changes(), want_rows), (label, s.get_changes())
        # a checked iteration is a check launch and no weighted one
        assert launched == ((done - len(want_rows)) if weighted else 0,
                            len(want_rows)), label
        # the row pitch: ragged 3-D rows, and never with weights or a tolerance
        assert bool(pitched) == (shape == (3, 5, 19) and not weighted and
                                 tolerance == "none" and
                                 observe in ("none", "device")), label
        assert printed == (["Primal-Dual iteration %d/%d" % (k, ITERS)
                            for k in range(1, done + 1)]
                           if observe == "verbose" else []), label
        if observe == "device":
            o.compute_measures()
            pts = o.get_observed_iterations()
            assert pts == [0, 2, 4, 6, 7], label
            got = np.asarray(o.get_measures()["RMSE"], dtype=np.float64)
            seen = [j for j, k in enumerate(pts) if k <= done]
            print(label, "RMSE", got, [rmse[k] for k in pts])
            assert np.allclose(got[seen], [rmse[pts[j]] for j in seen],
                               rtol=MEASURE_RTOL, atol=0), label
            assert np.all(np.isnan(got[len(seen):])), label
        elif observe == "host":
            kept = o.get_x_list()
            assert len(kept) == done + 1, label
            assert np.array_equal(kept[0], obs.flatten()), label
            for k in range(1, done + 1):
                assert np.array_equal(kept[k], host[k]), (label, k)


# ------------------------------------------------------------- sweep and stack
ALPHAS, MEMBERS = STACK_ALPHAS, len(STACK_ALPHAS)


def _assert_member(label, x, done, changes, alone):
    assert alone.get_execution() == "fused", label
    assert done == alone.get_iterations_done(), label
    assert np.array_equal(x, alone.get_x()), label
    if changes is not None:
        own = alone.get_changes()
        assert changes.shape == own.shape, label
        assert np.array_equal(changes[:, 0], own[:, 0]), label
        # (the stacked kernel adds the same summands in another order)
        assert np.allclose(changes[:, 1:], own[:, 1:], rtol=1e-12, atol=0), label


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("group", [3, 2], ids=["one-group", "two-groups"])
@pytest.mark.parametrize("stopping", [False, True], ids=["all", "stopping"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_sweep_and_stack_members_are_their_own_runs(nsol, monkeypatch, weighted,
                                                    stopping, group, dtype):
    from nsol_amd import PrimalDualBatch, ops
    from nsol_amd.parameter_sweep import PrimalDualSweep
    n, dim, es = int(np.prod(STACK_SHAPE)), len(STACK_SHAPE), np.dtype(dtype).itemsize
    # the byte budget of `group` members' state; a third member does not fit
    monkeypatch.setattr(ops, "PD_SWEEP_GROUP_BYTES", group * (3 + 2 * dim) * n * es)
    monkeypatch.setattr(ops, "PD_BATCH_GROUP_BYTES", group * (5 + 2 * dim) * n * es)
    assert (group + 1) * (4 + 2 * dim) > group * (5 + 2 * dim)
    reg, iso = "TV", False
    # ---- the sweep: one observation, three alphas, one tolerance
    obs, weights = member_obs(0), form_weights(STACK_SHAPE, weighted)
    tol = None
    if stopping:
        tol = met_at_the_second_check(obs, reg, iso, weights, ALPHAS[0])[0]
        for alpha in ALPHAS[1:]:    # (asserts the margin at every member's checks)
            pd_stop_denoise(obs, STACK_SHAPE, reg, "L2", ALG, alpha, 4 * dim, ITERS, tol,
                            check_every=EVERY, weights=weights)
    calls, b, xs = _wiring(obs, reg, iso, weights)
    sweep = PrimalDualSweep(calls["prox_f"], calls["prox_g_conj"], calls["B"],
                            calls["B_conj"], 4 * dim, b, {"alpha": ALPHAS},
                            iterations=ITERS, x_scale=xs, dtype=dtype, alg_type=ALG,
                            tolerance=tol, check_every=EVERY, stacked_stopping=stopping)
    sweep.run()
    assert sweep.get_execution() == "stacked" and sweep.get_group_size() == group
    for m, alpha in enumerate(ALPHAS):
        alone = _solver(obs, reg, iso, weights, dtype, alpha=alpha, tolerance=tol)
        alone.run()
        _assert_member(("sweep", m), sweep.get_x(m), sweep.get_iterations_done()[m], None,
                       alone)
    if stopping:
        assert sweep.get_iterations_done()[0] == CHECKS[1]
    # ---- the stack: every member its own observation, weights, alpha and tolerance
    def members():
        out = []
        for m, alpha in enumerate(ALPHAS):
            o, w = member_obs(m), form_weights(STACK_SHAPE, weighted, 7 + m)
            t = met_at_the_second_check(o, reg, iso, w, alpha)[0] if stopping else None
            out.append(_solver(o, reg, iso, w, dtype, alpha=alpha, tolerance=t))
        return out
    solvers = members()
    batch = PrimalDualBatch(solvers, stacked_stopping=stopping)
    batch.run()
    assert batch.get_execution() == ["stacked"] * MEMBERS
    assert batch.get_group_size() == group
    for m, (s, alone) in enumerate(zip(solvers, members())):
        alone.run()
        _assert_member(("stack", m), s.get_x(), s.get_iterations_done(),
                       s.get_changes(), alone)
        assert s.get_stop_reason() == alone.get_stop_reason()
        if stopping:
            assert s.get_iterations_done() == CHECKS[1]
