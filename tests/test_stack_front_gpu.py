"""The stacked front ends -- PrimalDualBatch, PrimalDualLinearBatch, PrimalDualSweep,
PrimalDualLinearSweep -- against their members' own run(): five members in groups of
two (the last group ragged), inputs on the host or already on the device, with and
without weights, in both dtypes, with a device-mode observer every 3 of 7 iterations;
and one stack and one sweep whose members stop one by one.  Through the public interface
only: the test holds for any arrangement of the host code behind it."""
import numpy as np
import pytest

from test_pd_linear_stack_gpu import _bits, _kernel_for, _wrapped
from test_pd_weighted_host import mixed_weights
from test_stack_front_host import (ALPHAS, EVERY, ITERS, MEMBERS, NEVER, SECOND_CHECK,
                                   SHAPES, STOP_SHAPE, member_observation,
                                   stack_tolerances, sweep_tolerance)

pytestmark = pytest.mark.gpu

GROUP = 2
POINTS = [0, 3, 6, 7]
FRONTS = ["PrimalDualBatch", "PrimalDualLinearBatch", "PrimalDualSweep",
          "PrimalDualLinearSweep"]


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _budgets(monkeypatch, shape, dtype, weighted):
    """Byte budgets that hold GROUP members of each stack's state and no more: twice the
    most arrays a member can own.  GROUP * most // fewest is still GROUP wherever a
    member owns at least four arrays, and the fewest any of these owns is 3 + 2 dim."""
    from nsol_amd import ops
    n, dim, es = int(np.prod(shape)), len(shape), np.dtype(dtype).itemsize
    unit = GROUP * n * es
    monkeypatch.setattr(ops, "PD_SWEEP_GROUP_BYTES", unit * (3 + 2 * dim))
    monkeypatch.setattr(ops, "PD_BATCH_GROUP_BYTES",
                        unit * ((5 if weighted else 4) + 2 * dim))
    # x, two xbar, q, g, two p, the member's own b~ and weights, t = A xbar
    monkeypatch.setattr(ops, "PDL_STACK_GROUP_BYTES", unit * (8 + 2 * dim))


def _measures(shape):
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    truth = member_observation(shape, 99).flatten()
    return {"RMSE": lambda x: sm.similarity_measures["RMSE"](x, truth),
            "NCC": lambda x: sm.similarity_measures["NCC"](x, truth)}


def _observer(shape):
    from nsol_amd.observer import Observer
    o = Observer(keep_iterates=False, every=EVERY)
    o.set_measures(_measures(shape))
    return o


def _operands(obs, weights, dtype, where):
    """(b, x0, weights) as NumPy arrays, or on the device: b in float64, x0 in the
    working dtype and the weights in float64, so that the front end converts them."""
    from nsol_amd.device import to_device
    b = obs.flatten()
    w = None if weights is None else weights.flatten()
    if where == "host":
        return b, b, w
    return to_device(b, np.float64), to_device(b, dtype), \
        None if w is None else to_device(w, np.float64)


def _plain_wiring(obs, weights, dtype, where):
    """(callables, x0, L2, x_scale) of a TV-l2 denoising of obs, x_scale = max."""
    import nsol_amd.linear_operators as LO
    from nsol_amd.proximal_operators import ProximalOperators as prox
    shape, dim = obs.shape, obs.ndim
    b, x0, w = _operands(obs, weights, dtype, where)
    xs = float(obs.max())
    lo = {2: LO.LinearOperators2D, 3: LO.LinearOperators3D}[dim]()
    grad, grad_adj = lo.get_gradient_operators()
    Z = grad(obs).shape
    D = lambda x: grad(x.reshape(*shape)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    if w is None:
        pf = lambda x, tau: prox.prox_ell2_denoising(x, tau, x0=b, x_scale=xs)
    else:
        pf = lambda x, tau: prox.prox_ell2_denoising_weighted(x, tau, x0=b, weights=w,
                                                              x_scale=xs)
    return dict(prox_f=pf, prox_g_conj=prox.prox_tv_conj, B=D, B_conj=Da), x0, \
        4 * dim, xs


def _plain_solver(obs, weights, dtype, where, alpha, tolerance=None):
    import nsol_amd.primal_dual_solver as pd
    calls, x0, L2, xs = _plain_wiring(obs, weights, dtype, where)
    return pd.PrimalDualSolver(L2=L2, x0=x0, alpha=alpha, iterations=ITERS, x_scale=xs,
                               alg_type="ALG2", dtype=dtype, tolerance=tolerance,
                               check_every=EVERY, **calls)


def _linear_arguments(obs, weights, dtype, where):
    from nsol_amd.linear_operators import ConvolutionOperator
    shape = obs.shape
    b, x0, w = _operands(obs, weights, dtype, where)
    A = ConvolutionOperator(len(shape), _kernel_for(shape))
    return dict(A=_wrapped(A, shape), A_adj=_wrapped(A, shape), b=b, x0=x0,
                dimension=len(shape)), \
        dict(iterations=ITERS, x_scale=float(obs.max()), dtype=dtype, weights=w,
             reg_type="huber", isotropic=True)


def _linear_solver(nsol, obs, weights, dtype, where, alpha):
    args, kw = _linear_arguments(obs, weights, dtype, where)
    return nsol.PrimalDualLinearSolver(alpha=alpha, **args, **kw)


def _member_inputs(shape, weighted, m):
    """Member m of a batch: its own observation, weights, alpha and x_scale."""
    obs = (1. + 0.5 * m) * member_observation(shape, m)
    return obs, mixed_weights(shape, 7 + m) if weighted else None, ALPHAS[m]


def _same_measures(a, b, done, label):
    """Two observers hold the same values: numbers up to iteration `done`, NaN after."""
    a.compute_measures()
    b.compute_measures()
    assert a.get_observed_iterations() == b.get_observed_iterations() == POINTS, label
    for name in ("RMSE", "NCC"):
        got = np.asarray(a.get_measures()[name], dtype=np.float64)
        assert got.shape == (len(POINTS),), (label, name)
        assert list(np.isfinite(got)) == [k <= done for k in POINTS], (label, name)
        assert np.array_equal(got, b.get_measures()[name], equal_nan=True), (label, name)


def _check_batch(batch, solvers, own, label, changes=False):
    """A batch that has run against the same solvers run one by one."""
    assert batch.get_execution() == ["stacked"] * MEMBERS, label
    assert batch.get_group_size() == GROUP, label
    X = batch.get_x_all_device().cpu().numpy()
    assert X.shape == (MEMBERS, solvers[0]._x.numel()), label
    for m, (s, o) in enumerate(zip(solvers, own)):
        o.run()
        key = label + (m,)
        assert s.get_execution() == o.get_execution() == "fused", key
        assert np.array_equal(_bits(s), _bits(o)), key
        assert np.array_equal(s.get_x(), o.get_x()), key
        assert np.array_equal(X[m], o.get_x_device().cpu().numpy()), key
        assert s.get_iterations_done() == o.get_iterations_done(), key
        assert s.get_stop_reason() == o.get_stop_reason(), key
        _same_measures(s.get_observer(), o.get_observer(), o.get_iterations_done(), key)
        if changes:
            got, want = s.get_changes(), o.get_changes()
            assert got.shape == want.shape and np.array_equal(got[:, 0], want[:, 0]), key
            # (the stacked kernel adds the same summands in another order)
            assert np.allclose(got[:, 1:], want[:, 1:], rtol=1e-12, atol=0), key


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("front", FRONTS)
def test_a_front_end_is_its_members_own_runs(nsol, monkeypatch, front, shape, where,
                                             weighted, dtype):
    label = (front, shape, where, weighted, np.dtype(dtype).name)
    _budgets(monkeypatch, shape, dtype, weighted)
    linear = "Linear" in front
    if front.endswith("Batch"):
        def build():
            out = []
            for m in range(MEMBERS):
                obs, w, alpha = _member_inputs(shape, weighted, m)
                s = _linear_solver(nsol, obs, w, dtype, where, alpha) if linear else \
                    _plain_solver(obs, w, dtype, where, alpha)
                s.set_observer(_observer(shape))
                out.append(s)
            return out
        solvers, own = build(), build()
        batch = getattr(nsol, front)(solvers)
        batch.run()
        assert batch.get_solvers() == solvers
        _check_batch(batch, solvers, own, label)
        for s in solvers:
            assert s.get_iterations_done() == ITERS, label
            assert s.get_stop_reason() == "iterations", label
        return
    # ---- a sweep: one observation, one set of weights, five alphas
    obs, w, _ = _member_inputs(shape, weighted, 0)
    if linear:
        args, kw = _linear_arguments(obs, w, dtype, where)
        sweep = nsol.PrimalDualLinearSweep(parameters={"alpha": ALPHAS}, **args, **kw)
    else:
        from nsol_amd.parameter_sweep import PrimalDualSweep
        calls, x0, L2, xs = _plain_wiring(obs, w, dtype, where)
        sweep = PrimalDualSweep(calls["prox_f"], calls["prox_g_conj"], calls["B"],
                                calls["B_conj"], L2, x0, {"alpha": ALPHAS},
                                iterations=ITERS, x_scale=xs, dtype=dtype,
                                alg_type="ALG2", check_every=EVERY)
    sweep.set_measures(_measures(shape), every=EVERY)
    sweep.run()
    assert sweep.get_execution() == "stacked" and sweep.get_group_size() == GROUP, label
    assert sweep.get_iterations_done() == [ITERS] * MEMBERS, label
    assert sweep.get_observed_iterations() == POINTS, label
    got = sweep.get_measures()
    X = sweep.get_x_all_device().cpu().numpy()
    assert X.shape == (MEMBERS, int(np.prod(shape))), label
    for m, alpha in enumerate(ALPHAS):
        key = label + (m,)
        o = _linear_solver(nsol, obs, w, dtype, where, alpha) if linear else \
            _plain_solver(obs, w, dtype, where, alpha)
        o.set_observer(_observer(shape))
        o.run()
        o.get_observer().compute_measures()
        assert o.get_execution() == "fused", key
        assert np.array_equal(sweep.get_x(m), o.get_x()), key
        assert np.array_equal(X[m], o.get_x_device().cpu().numpy()), key
        assert o.get_observer().get_observed_iterations() == POINTS, key
        for name in ("RMSE", "NCC"):
            assert got[name].shape == (MEMBERS, len(POINTS)), key
            assert np.all(np.isfinite(got[name])), key
            assert np.array_equal(got[name][m], o.get_observer().get_measures()[name]), \
                (key, name)


# ------------------------------------------------- members that stop one by one
def test_a_stack_whose_members_stop_one_by_one(nsol, monkeypatch):
    """Every member its own tolerance: three that are met at the second check, two that
    never are."""
    shape, dtype, weighted = STOP_SHAPE, np.float32, True
    _budgets(monkeypatch, shape, dtype, weighted)
    tolerances = stack_tolerances(weighted)
    assert len(set(tolerances)) > 2 and NEVER in tolerances

    def build():
        out = []
        for m in range(MEMBERS):
            obs, w, alpha = member_observation(shape, m), \
                mixed_weights(shape, 7 + m), ALPHAS[m]
            s = _plain_solver(obs, w, dtype, "host", alpha, tolerance=tolerances[m])
            s.set_observer(_observer(shape))
            out.append(s)
        return out
    solvers, own = build(), build()
    batch = nsol.PrimalDualBatch(solvers, stacked_stopping=True)
    batch.run()
    _check_batch(batch, solvers, own, ("stopping",), changes=True)
    assert [s.get_iterations_done() for s in solvers] == \
        [ITERS if t == NEVER else SECOND_CHECK for t in tolerances]
    assert [s.get_stop_reason() for s in solvers] == \
        ["iterations" if t == NEVER else "tolerance" for t in tolerances]


def test_a_sweep_whose_members_stop_one_by_one(nsol, monkeypatch):
    """One tolerance, met at the second check by some alphas and never by others."""
    from nsol_amd.parameter_sweep import PrimalDualSweep
    shape, dtype, weighted = STOP_SHAPE, np.float32, True
    _budgets(monkeypatch, shape, dtype, weighted)
    tol, done = sweep_tolerance(weighted)
    assert len(set(done)) > 1
    obs, w = member_observation(shape, 0), mixed_weights(shape, 7)
    calls, x0, L2, xs = _plain_wiring(obs, w, dtype, "host")
    sweep = PrimalDualSweep(calls["prox_f"], calls["prox_g_conj"], calls["B"],
                            calls["B_conj"], L2, x0, {"alpha": ALPHAS}, iterations=ITERS,
                            x_scale=xs, dtype=dtype, alg_type="ALG2", tolerance=tol,
                            check_every=EVERY, stacked_stopping=True)
    sweep.set_measures(_measures(shape), every=EVERY)
    sweep.run()
    assert sweep.get_execution() == "stacked" and sweep.get_group_size() == GROUP
    assert sweep.get_iterations_done() == done
    assert sweep.get_observed_iterations() == POINTS
    got = sweep.get_measures()
    X = sweep.get_x_all_device().cpu().numpy()
    for m, alpha in enumerate(ALPHAS):
        o = _plain_solver(obs, w, dtype, "host", alpha, tolerance=tol)
        o.set_observer(_observer(shape))
        o.run()
        o.get_observer().compute_measures()
        assert o.get_iterations_done() == done[m], m
        assert np.array_equal(sweep.get_x(m), o.get_x()), m
        assert np.array_equal(X[m], o.get_x_device().cpu().numpy()), m
        for name in ("RMSE", "NCC"):
            assert list(np.isfinite(got[name][m])) == [k <= done[m] for k in POINTS]
            assert np.array_equal(got[name][m], o.get_observer().get_measures()[name],
                                  equal_nan=True), (m, name)
