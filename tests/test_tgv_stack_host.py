"""Host-side logic of the stacked forms of TGVPrimalDualSolver (nsol_amd/tgv_stack.py):
the declared C entry points, which solvers form a stack -- one field at a time --, the
group-size arithmetic, the sweep's members and the constructors' refusals.  No GPU."""
import itertools

import numpy as np
import pytest

SHAPE = (12, 19)


def _solver(shape=SHAPE, seed=0, scale=1.0, **kw):
    import nsol_amd
    rng = np.random.default_rng(seed)
    obs = scale * (50.0 + 10.0 * rng.standard_normal(shape))
    args = dict(b=obs.flatten(), x0=obs.flatten(), dimension=len(shape), shape=shape,
                alpha=0.05, beta=2.0, iterations=10, x_scale=float(obs.max()),
                dtype=np.float32)
    args.update(kw)
    return nsol_amd.TGVPrimalDualSolver(**args)


def _keys(solvers):
    from nsol_amd.tgv_stack import member_key
    return [member_key(s) for s in solvers]


# ------------------------------------------------------------------ the C ABI
def test_the_stacked_entries_are_declared():
    from nsol_amd import _lib
    syms = _lib.declared_symbols()
    assert syms["nsol_tgv_stack_launches"][1] == []
    for suf in ("f32", "f64"):
        for name, nargs in (("table", 7), ("dual", 16), ("primal", 21), ("primal_w", 23)):
            assert len(syms["nsol_tgv_stack_%s_%s" % (name, suf)][1]) == nargs, name
        assert "nsol_tgv_stack_primal_lin_" + suf not in syms     # out of scope
    # the member strides and the table travel as 64-bit integers and a pointer
    args = syms["nsol_tgv_stack_primal_w_f32"][1]
    assert args[7] is _lib.c_i64 and args[9] is _lib.c_i64 and args[20] is _lib.c_ptr


def test_the_package_exports_the_front_ends():
    import nsol_amd
    from nsol_amd import tgv_stack
    from nsol_amd.parameter_sweep import PrimalDualSweep
    from nsol_amd.solver_batch import PrimalDualBatch
    assert nsol_amd.TGVPrimalDualBatch is tgv_stack.TGVPrimalDualBatch
    assert nsol_amd.TGVPrimalDualSweep is tgv_stack.TGVPrimalDualSweep
    assert issubclass(tgv_stack.TGVPrimalDualBatch, PrimalDualBatch)
    assert issubclass(tgv_stack.TGVPrimalDualSweep, PrimalDualSweep)
    assert tgv_stack.TGVPrimalDualBatch._stops_members is False


# ------------------------------------------------------------------ the member key
def test_members_that_differ_in_data_alpha_beta_scale_and_weights_share_a_key():
    from nsol_amd.solver_batch import plan_stacks
    n = SHAPE[0] * SHAPE[1]
    w = np.ones(n)
    w[::7] = 0
    solvers = [_solver(seed=0, weights=np.ones(n)),
               _solver(seed=1, alpha=0.2, beta=0.7, scale=3.0, weights=w),
               _solver(seed=2, alpha=0.01, beta=5.0, weights=2.5 * w)]
    keys = _keys(solvers)
    assert None not in keys and len(set(keys)) == 1
    assert plan_stacks(keys) == [[0, 1, 2]]
    assert len({s.get_x_scale() for s in solvers}) == 3
    plain = _keys([_solver(seed=3, alpha=0.3), _solver(seed=4, beta=0.5, scale=2.0)])
    assert plain[0] == plain[1] and plain[0] != keys[0]


@pytest.mark.parametrize("kw", [
    dict(shape=(19, 12)), dict(shape=(228,)), dict(shape=(2, 6, 19)),
    dict(dtype=np.float64), dict(iterations=11), dict(isotropic=True),
    dict(data_loss="ell1"), dict(spacing=(1., 2.)), dict(tau=0.2), dict(sigma=0.2),
    dict(L2=20.), dict(weights=np.ones(228))], ids=lambda kw: "-".join(sorted(kw)))
def test_every_field_separates_a_stack(kw):
    from nsol_amd.solver_batch import plan_stacks
    keys = _keys([_solver(), _solver(seed=1, **kw)])
    assert None not in keys and keys[0] != keys[1]
    assert plan_stacks(keys) == []


def test_observation_points_join_and_separate():
    from nsol_amd.observer import Observer
    from nsol_amd.solver_batch import plan_stacks
    obs = [_solver(seed=k) for k in range(4)]
    for s, every in zip(obs[:3], (5, 5, 3)):
        s.set_observer(Observer(keep_iterates=False, every=every))
    keys = _keys(obs)
    assert keys[0] == keys[1] and len({keys[0], keys[2], keys[3]}) == 3
    assert plan_stacks(keys + _keys([_solver(seed=9)])) == [[0, 1], [3, 4]]


def test_what_runs_on_its_own():
    import nsol_amd
    from nsol_amd.observer import Observer
    from nsol_amd.tgv_stack import member_key
    assert member_key(_solver(tolerance=1e-3)) is None
    assert member_key(_solver(verbose=1)) is None
    assert member_key(_solver(iterations=0)) is None
    host = _solver()
    host.set_observer(Observer())                 # keeps iterates on the host
    assert member_key(host) is None
    assert member_key("not a solver") is None
    assert member_key(_solver()) is not None
    with pytest.raises(ValueError):
        nsol_amd.TGVPrimalDualBatch([])
    with pytest.raises(ValueError):
        nsol_amd.TGVPrimalDualBatch([_solver()], stacked_stopping=True)
    s = _solver()
    with pytest.raises(ValueError):
        nsol_amd.TGVPrimalDualBatch([s, s])
    obs = np.ones(20)
    lin = nsol_amd.TGVPrimalDualLinearSolver(
        A=lambda x: x, A_adj=lambda x: x, b=obs, x0=obs, dimension=1, A_norm2=1.)
    with pytest.raises(ValueError):
        nsol_amd.TGVPrimalDualBatch([lin])        # the linear form has no stack yet


# ------------------------------------------------------------------ groups
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_group_size_counts_what_a_member_owns(monkeypatch, dim):
    from nsol_amd import ops
    assert ops.TGV_STACK_GROUP_BYTES == 256 << 20 == ops.PD_BATCH_GROUP_BYTES
    n, es = 1 << 14, 4
    M = dim * (dim + 1) // 2
    state = (2 + 3 * dim + M) * n * es            # x, xbar, w, wbar, p, q
    monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", 4 * (state + 2 * n * es))
    # a batch member owns its observation, a weighted one its weights as well
    assert ops.tgv_stack_group_size(64, n, dim, es, True) == 4
    assert ops.tgv_stack_group_size(64, n, dim, es, False) == \
        4 * (state + 2 * n * es) // (state + n * es)
    assert ops.tgv_stack_group_size(3, n, dim, es, True) == 3
    # a sweep shares both
    assert ops.tgv_stack_group_size(64, n, dim, es, True, own_data=False) == \
        4 * (state + 2 * n * es) // state
    assert ops.tgv_stack_group_size(64, n, dim, 8, True) == 2
    monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", 1)
    assert ops.tgv_stack_group_size(64, n, dim, es, False) == 1      # at least one
    monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", 1 << 60)
    assert ops.tgv_stack_group_size(1 << 20, 1, dim, es, False) == 65535
    assert ops.sweep_groups(5, 2) == [(0, 2), (2, 4), (4, 5)]


# ------------------------------------------------------------------ the sweep's members
def test_member_parameters_take_the_sweeps_keys():
    from nsol_amd.parameter_sweep import PARAMETER_KEYS, member_parameters
    from nsol_amd.tgv_stack import SWEEP_KEYS
    assert SWEEP_KEYS == ("alpha", "beta")
    got = member_parameters({"alpha": [0.1, 0.2], "beta": [1., 2., 3.]}, keys=SWEEP_KEYS)
    assert got == [dict(alpha=a, beta=b)
                   for a, b in itertools.product([0.1, 0.2], [1., 2., 3.])]
    # the dictionary's own key order decides which parameter varies fastest
    got = member_parameters({"beta": [1., 2.], "alpha": [0.1, 0.2]}, keys=SWEEP_KEYS)
    assert [(m["beta"], m["alpha"]) for m in got] == \
        [(1., 0.1), (1., 0.2), (2., 0.1), (2., 0.2)]
    assert list(got[0]) == ["beta", "alpha"]
    assert member_parameters({"beta": 1.5}, keys=SWEEP_KEYS) == [dict(beta=1.5)]
    for bad in ({"alg_type": ["ALG2"]}, {"alpha": [0.1], "L2": [8.]}):
        with pytest.raises(ValueError, match="unknown sweep parameter"):
            member_parameters(bad, keys=SWEEP_KEYS)
    with pytest.raises(ValueError):
        member_parameters({"alpha": []}, keys=SWEEP_KEYS)
    # the default keys are PrimalDualSweep's, as before
    assert PARAMETER_KEYS == ("alpha", "alg_type", "L2")
    assert member_parameters({"alg_type": "ALG2", "L2": [8., 12.]}) == \
        [dict(alg_type="ALG2", L2=8.), dict(alg_type="ALG2", L2=12.)]
    with pytest.raises(ValueError, match="unknown sweep parameter"):
        member_parameters({"beta": [1.]})


def test_the_sweep_builds_its_members_and_refuses_as_the_solver_does():
    import nsol_amd
    obs = 50.0 + np.arange(SHAPE[0] * SHAPE[1], dtype=float)
    kw = dict(b=obs, x0=obs, dimension=2, shape=SHAPE, iterations=7, x_scale=3.,
              dtype=np.float32, data_loss="ell1", isotropic=True)
    sweep = nsol_amd.TGVPrimalDualSweep(parameters={"alpha": [0.1, 0.2], "beta": [1., 3.]},
                                        **kw)
    assert sweep.get_parameters() == [dict(alpha=a, beta=b)
                                      for a in (0.1, 0.2) for b in (1., 3.)]
    s = sweep._solver(sweep.get_parameters()[3])
    assert (s.get_alpha(), s.get_beta(), s.get_iterations()) == (0.2, 3., 7)
    assert s.get_data_loss() == "ell1" and s.get_isotropic() and s.get_x_scale() == 3.
    assert sweep.get_execution() is None
    with pytest.raises(RuntimeError):
        sweep.get_w(0)
    # a parameter that is not swept keeps its keyword's value
    one = nsol_amd.TGVPrimalDualSweep(parameters={"alpha": [0.1]}, beta=4., **kw)
    assert one._solver(one.get_parameters()[0]).get_beta() == 4.
    with pytest.raises(ValueError, match="unknown sweep parameter"):
        nsol_amd.TGVPrimalDualSweep(parameters={"L2": [8.]}, **kw)
    with pytest.raises(ValueError):
        nsol_amd.TGVPrimalDualSweep(parameters={"beta": [-1.]}, **kw)
    # a tolerance sends the sweep to sequential solvers
    tol = nsol_amd.TGVPrimalDualSweep(parameters={"alpha": [0.1]}, tolerance=1e-3, **kw)
    assert tol._stack_form(tol._solver(tol.get_parameters()[0])) is None
    assert sweep._stack_form(s) is s


def test_the_tables_values_are_the_solvers_own():
    """The table is rounded in the library; what Python hands it is the float64 tl =
    tau / alpha that TGVPrimalDualSolver._run passes to its own launches."""
    from nsol_amd.tgv_stack import member_table_values
    tau = 0.23570226039551584
    beta, tl = member_table_values(tau, [0.3, 0.01, 7], [2, 0.5, 1.7])
    assert beta.dtype == tl.dtype == np.float64
    assert list(beta) == [2., 0.5, 1.7]
    assert list(tl) == [tau / 0.3, tau / 0.01, tau / 7.]
