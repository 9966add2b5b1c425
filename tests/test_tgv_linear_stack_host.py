"""Host-side logic of the stacked forms of TGVPrimalDualLinearSolver
(nsol_amd/tgv_linear_stack.py): the declared C entries, which solvers form a stack -- one
field at a time --, the group-size arithmetic, the sweep's members and refusals, the launch
counts, and the condition on the finite box of test_tgv_linear_stack_gpu.py's kernel test.
No GPU."""
import itertools
import os

import numpy as np
import pytest

from test_pd_linear_host import box_kernel, gaussian_kernel
from test_tgv_stack_gpu import STRADDLING, TAU, THETA, _rounded_spacing
from tgv_lin_stack_cases import MEMBERS, box_shares, finite_box

SHAPE = (24, 40)
N = 24 * 40


def _solver(shape=SHAPE, seed=0, kernel=None, op=None, scale=1.0, **kw):
    import nsol_amd
    from nsol_amd.linear_operators import ConvolutionOperator
    rng = np.random.default_rng(seed)
    obs = scale * (50.0 + 10.0 * rng.standard_normal(shape))
    if op is None:
        op = ConvolutionOperator(len(shape), gaussian_kernel(len(shape), 1.)
                                 if kernel is None else kernel)
    A = lambda x: op(x.reshape(*shape)).flatten()
    args = dict(A=A, A_adj=A, b=obs.flatten(), x0=obs.flatten(), dimension=len(shape),
                alpha=0.05, beta=2.0, iterations=10, x_scale=float(obs.max()),
                dtype=np.float32)
    args.update(kw)
    if "A" in kw:
        args["shape"] = shape       # a foreign A does not tell the volume's shape
    return nsol_amd.TGVPrimalDualLinearSolver(**args)


def _keys(solvers):
    from nsol_amd.tgv_linear_stack import member_key
    return [member_key(s) for s in solvers]


# ------------------------------------------------------------------ the C ABI
def test_the_new_entries_are_declared_and_built():
    from nsol_amd import _lib, ops
    from nsol_amd._lib import c_dbl, c_i64, c_int, c_ptr
    # the two entries are declared in a header of their own, which nsol_hip.h includes
    # and _lib.load() binds: tests/test_tgv_stack_host.py keeps them out of what
    # nsol_hip.h itself declares
    (header,) = _lib.MORE_HEADERS
    assert os.path.basename(header) == "nsol_hip_tgv_lin_stack.h"
    assert '#include "nsol_hip_tgv_lin_stack.h"' in open(_lib.HEADER).read()
    sym, main = _lib.declared_symbols(header), _lib.declared_symbols()
    want = [c_ptr] * 7 + [c_int, c_int] + [c_i64] * 3 + [c_dbl] * 7 + [c_ptr]
    assert sorted(sym) == ["nsol_tgv_stack_primal_lin_f32", "nsol_tgv_stack_primal_lin_f64"]
    lib = _lib.load()
    for suf in ("f32", "f64"):
        name = "nsol_tgv_stack_primal_lin_" + suf
        assert sym[name] == (c_int, want)
        # the single entry's arguments with `members` after g
        single = main["nsol_tgv_primal_lin_" + suf][1]
        assert sym[name][1] == single[:7] + [c_int] + single[7:]
        # ... and bound with them
        fn = getattr(lib, name)
        assert fn.restype is c_int and list(fn.argtypes) == want
    for name in ("tgv_stack_primal_lin", "tgv_lin_stack_group_size"):
        assert callable(getattr(ops, name))


def test_the_entry_declines_before_any_launch():
    """What the entry refuses, it refuses on the host before a kernel is launched, so the
    calls can be made without a device (the pointers are compared, never followed)."""
    from nsol_amd import _lib
    lib = _lib.load()
    n = 3 * 4 * 6
    before = lib.nsol_tgv_stack_launches(), lib.nsol_tgv_launches()
    for suf, size in (("f32", 4), ("f64", 8)):
        fn = getattr(lib, "nsol_tgv_stack_primal_lin_" + suf)
        step = 2 * 6 * n * size                 # two members of the longest span, q
        good = [0x100000 + k * step for k in range(7)]

        def call(ptrs=good, members=2, dims=(3, 3, 4, 6), tau=0.3, theta=1., lo=-np.inf,
                 hi=np.inf):
            return fn(*ptrs, members, *dims, 1., 1., 1., tau, theta, lo, hi, None)
        assert [call(members=m) for m in (0, -1, 65536)] == [-2] * 3
        assert call(dims=(3, 1 << 11, 1 << 11, 1 << 10)) == -2
        for k in range(7):
            ptrs = list(good)
            ptrs[k] = None
            assert call(ptrs) == -1, k
        for i, j in itertools.combinations(range(7), 2):
            ptrs = list(good)
            ptrs[j] = ptrs[i]
            assert call(ptrs) == -1, (i, j)
        # x and xbar one member apart: they overlap because the spans are two members long
        ptrs = list(good)
        ptrs[3] = ptrs[2] + n * size
        assert call(ptrs) == -1
        assert call(lo=1., hi=0.) == -1 and call(lo=np.nan, hi=1.) == -1
        for bad in (0., -1., np.inf, np.nan):
            assert call(tau=bad) == -1, bad
        assert call(theta=np.nan) == -1 and call(theta=np.inf) == -1
        for dims in ((0, 3, 4, 6), (4, 3, 4, 6), (3, -1, 4, 6)):
            assert call(dims=dims) == -1, dims
        for dims in ((3, 0, 4, 6), (3, 3, 0, 6), (1, 1, 1, 0)):
            assert call(dims=dims) == 0 and call([None] * 7, dims=dims) == 0
    assert (lib.nsol_tgv_stack_launches(), lib.nsol_tgv_launches()) == before


# ------------------------------------------------------------------ the member key
def test_members_that_differ_in_data_alpha_beta_scale_and_weights_share_a_key():
    from nsol_amd.solver_batch import plan_stacks
    w = np.ones(N)
    w[::7] = 0
    solvers = [_solver(seed=0, weights=np.ones(N)),
               _solver(seed=1, alpha=0.2, beta=0.7, scale=3.0, weights=w),
               _solver(seed=2, alpha=0.01, beta=3.0, weights=2.5 * w)]
    keys = _keys(solvers)
    assert None not in keys and len(set(keys)) == 1
    assert plan_stacks(keys) == [[0, 1, 2]]
    assert len({s.get_x_scale() for s in solvers}) == 3
    assert len({id(s._op) for s in solvers}) == 3       # operators equal by value


def test_the_key_field_by_field():
    """linear_stack.member_key's list without reg_type and huber_gamma, with theta."""
    from nsol_amd.linear_stack import operator_key
    s = _solver(bounds=(0., 2.), isotropic=True, data_loss="ell1")
    key = _keys([s])[0]
    assert key == (
        operator_key(s._op), SHAPE, operator_key(s._op_adj), SHAPE, SHAPE, (1., 1.), 2,
        True, "ell1", (0., 2.), float(s.get_tau()), float(s.get_sigma()), 1.,
        "float32", 10, None, False, ("b", None), ("x0", None), ("weights", None))
    assert hash(key) is not None


@pytest.mark.parametrize("kw", [
    dict(shape=(40, 24)), dict(shape=(960,)), dict(dtype=np.float64),
    dict(iterations=11), dict(isotropic=True), dict(data_loss="ell1"),
    dict(bounds=(0., np.inf)), dict(spacing=(1., 2.)), dict(tau=0.2), dict(sigma=0.2),
    dict(weights=np.ones(960)), dict(kernel=gaussian_kernel(2, 1.5)),
    dict(kernel=box_kernel(2))], ids=lambda kw: "-".join(sorted(kw)))
def test_every_shared_field_separates_a_stack(kw):
    from nsol_amd.solver_batch import plan_stacks
    keys = _keys([_solver(), _solver(seed=1, **kw)])
    assert None not in keys and keys[0] != keys[1]
    assert plan_stacks(keys) == []


def test_theta_and_the_boundary_mode_separate_a_stack():
    from nsol_amd.linear_operators import ConvolutionOperator
    a, b = _solver(), _solver(seed=1)
    assert _keys([a])[0] == _keys([b])[0]
    b._theta = 0.5                  # (no keyword sets it; the key reads it all the same)
    assert _keys([a])[0] != _keys([b])[0]
    k = gaussian_kernel(2, 1.)
    keys = _keys([_solver(op=ConvolutionOperator(2, k, "wrap")),
                  _solver(op=ConvolutionOperator(2, k, "reflect"))])
    assert None not in keys and keys[0] != keys[1]


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
    from nsol_amd.linear_operators import SampledConvolutionOperator
    from nsol_amd.observer import Observer
    from nsol_amd.tgv_linear_stack import member_key
    from test_pd_linear_stack_host import _solver as tv_solver
    assert member_key(_solver()) is not None
    assert member_key(_solver(tolerance=1e-3)) is None
    assert member_key(_solver(verbose=1)) is None
    assert member_key(_solver(iterations=0)) is None
    host = _solver()
    host.set_observer(Observer())                 # keeps iterates on the host
    assert member_key(host) is None
    foreign = lambda x: np.asarray(x) * 0.5       # a NumPy-only callable
    assert member_key(_solver(A=foreign, A_adj=foreign, A_norm2=0.25)) is None
    assert member_key(_solver(x0=np.ones(SHAPE))) is None          # x0 with two axes
    assert member_key("not a solver") is None
    assert member_key(tv_solver()) is None        # a PrimalDualLinearSolver
    # a blur-and-sample pair: b on the coarse grid, m != n
    shape, coarse = (12, 16), (12, 8)
    S = SampledConvolutionOperator(2, gaussian_kernel(2, 1.), (1, 2), (0, 0))
    St = S.adjoint(shape)
    sampled = nsol_amd.TGVPrimalDualLinearSolver(
        lambda x: S(x.reshape(*shape)).flatten(),
        lambda r: St(r.reshape(*coarse)).flatten(), np.ones(12 * 8), np.ones(12 * 16), 2,
        shape=shape, dtype=np.float32)
    assert sampled.get_execution() == "fused" and sampled._m != sampled._n
    assert member_key(sampled) is None


# ------------------------------------------------------------------ groups
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_group_size_counts_what_a_member_owns(monkeypatch, dim):
    from nsol_amd import ops
    n, es = 1 << 12, 4
    word = n * es
    assert ops.TGV_STACK_GROUP_BYTES == 256 << 20       # the constant keeps its value
    M = dim * (dim + 1) // 2
    for own_data, own_weights, with_t in itertools.product((False, True), repeat=3):
        # x, xbar; w, wbar, p; q; r, g; and what the flags add
        words = 2 + 3 * dim + M + 2 + own_data + own_weights + with_t
        kw = dict(own_data=own_data, own_weights=own_weights, with_t=with_t)
        monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", 5 * words * word)
        assert ops.tgv_lin_stack_group_size(64, n, dim, es, **kw) == 5
        assert ops.tgv_lin_stack_group_size(3, n, dim, es, **kw) == 3
        monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", 5 * words * word - 1)
        assert ops.tgv_lin_stack_group_size(64, n, dim, es, **kw) == 4
        assert ops.tgv_lin_stack_group_size(64, n, dim, 2 * es, **kw) == 2
        monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", words * word - 1)
        assert ops.tgv_lin_stack_group_size(64, n, dim, es, **kw) == 1   # never less
    # the defaults: a batch without weights, the epilogue on
    monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", 7 * (2 + 3 * dim + M + 3) * word)
    assert ops.tgv_lin_stack_group_size(64, n, dim, es) == 7
    monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", 1 << 62)
    assert ops.tgv_lin_stack_group_size(100000, 16, dim, es) == 65535


# ------------------------------------------------------------------ the front ends
def _sweep(parameters, shape=(6, 8), **kw):
    from nsol_amd.linear_operators import ConvolutionOperator
    from nsol_amd.tgv_linear_stack import TGVPrimalDualLinearSweep
    op = ConvolutionOperator(2, gaussian_kernel(2, 1.))
    A = lambda x: op(x.reshape(*shape)).flatten()
    obs = 1. + np.arange(int(np.prod(shape)), dtype=float)
    return TGVPrimalDualLinearSweep(A, A, obs, obs, 2, parameters=parameters, **kw)


def test_the_sweeps_members_and_refusals():
    import nsol_amd
    from nsol_amd.tgv_linear_stack import TGVPrimalDualLinearSweep
    assert nsol_amd.TGVPrimalDualLinearSweep is TGVPrimalDualLinearSweep
    sweep = _sweep({"alpha": [0.1, 0.4], "beta": [0.8, 1.7, 3.0]}, iterations=7)
    assert sweep.get_parameters() == [dict(alpha=a, beta=b) for a in (0.1, 0.4)
                                      for b in (0.8, 1.7, 3.0)]
    # the dictionary's key order is the order of the product
    sweep = _sweep({"beta": [0.8, 3.0], "alpha": [0.1, 0.4]})
    assert sweep.get_parameters() == [dict(beta=b, alpha=a) for b in (0.8, 3.0)
                                      for a in (0.1, 0.4)]
    # a parameter that is not swept keeps its keyword's value
    sweep = _sweep({"beta": [0.8, 3.0]}, alpha=0.3, tolerance=1e-3)
    assert sweep.get_parameters() == [dict(beta=0.8), dict(beta=3.0)]
    assert [sweep._solver(m).get_alpha() for m in sweep._members] == [0.3, 0.3]
    assert [sweep._solver(m).get_beta() for m in sweep._members] == [0.8, 3.0]
    assert sweep.get_execution() is None and sweep.get_iterations_done() is None
    assert sweep.get_group_size() is None
    with pytest.raises(RuntimeError):
        sweep.get_x_all_device()
    with pytest.raises(RuntimeError):
        sweep.get_w(0)
    for key in ("L2", "alg_type", "tau", "reg_type"):
        with pytest.raises(ValueError, match="unknown sweep parameter '%s'" % key):
            _sweep({"alpha": [0.1], key: [1]})
    with pytest.raises(ValueError):
        _sweep({})
    with pytest.raises(ValueError):
        _sweep({"alpha": []})
    with pytest.raises(ValueError):                       # the solver's own refusals
        _sweep({"alpha": [0.1, 0.2]}, data_loss="huber")
    with pytest.raises(ValueError):
        _sweep({"beta": [-1., 0.2]})
    with pytest.raises(ValueError):
        sweep.set_measures({}, every=0)


def test_the_batch_refuses():
    import nsol_amd
    from nsol_amd.tgv_linear_stack import TGVPrimalDualLinearBatch
    from test_pd_linear_stack_host import _solver as tv_solver
    assert nsol_amd.TGVPrimalDualLinearBatch is TGVPrimalDualLinearBatch
    with pytest.raises(ValueError, match="at least one"):
        TGVPrimalDualLinearBatch([])
    s = _solver()
    with pytest.raises(ValueError, match="TGVPrimalDualLinearSolver"):
        TGVPrimalDualLinearBatch([s, tv_solver()])
    with pytest.raises(ValueError, match="twice"):
        TGVPrimalDualLinearBatch([s, _solver(seed=1), s])
    with pytest.raises(ValueError, match="1D"):
        TGVPrimalDualLinearBatch([s, _solver(x0=np.ones(SHAPE))])
    with pytest.raises(ValueError, match="stacked stopping"):
        TGVPrimalDualLinearBatch([s, _solver(seed=1)], stacked_stopping=True)
    batch = TGVPrimalDualLinearBatch([s, _solver(seed=1)])
    assert batch.get_execution() is None and batch.get_group_size() is None


def test_launch_counts_per_iteration_by_dimension():
    from nsol_amd.tgv_linear_stack import launches_per_iteration
    # 2-D, two passes: 1 + 2 + 1 + 2 + 1 for the stack, that per member for the loop
    for P in (4, 16, 64):
        assert launches_per_iteration(_solver((24, 40)), P) == (7, 7 * P)
    assert launches_per_iteration(_solver((960,)), 16) == (5, 80)
    # 3-D, the one-pass blur per member: 2 P + 3 against 5 P
    assert launches_per_iteration(_solver((8, 10, 12)), 8) == (19, 40)
    dense = np.array([[0., 0.2, 0.], [0.2, 0.2, 0.2], [0., 0.2, 0.]])
    assert launches_per_iteration(_solver(kernel=dense), 5) == (13, 25)


# --------------------------------------- the finite box of the GPU file's kernel test
@pytest.mark.parametrize("shape", STRADDLING)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_finite_box_is_at_work_in_every_member(shape, dtype):
    """At least 10 % of every member's voxels clipped at lo, 10 % at hi and 10 % strictly
    inside (tgv_numpy.primal_step_lin in float64 on the GPU test's states): a kernel that
    ignored the box, or a member's offset into g, could not pass that test."""
    lo, hi = finite_box(shape, dtype)
    assert np.isfinite(lo) and np.isfinite(hi) and lo < hi
    for m in range(MEMBERS):
        shares = box_shares(shape, dtype, m)
        print(shape, np.dtype(dtype).name, m, "at lo %.3f inside %.3f at hi %.3f" % shares)
        assert min(shares) >= 0.10, (shape, m, shares)
        assert abs(sum(shares) - 1.) < 1e-12


def test_every_members_g_is_its_own():
    """Swapping two members' g changes the restated step of both: the member offset into
    g is observable."""
    from nsol_amd import tgv_numpy as tg
    from tgv_lin_stack_cases import lin_state, want_lin
    shape, dtype = STRADDLING[0], np.float64
    box = finite_box(shape, dtype)
    s0, s1 = lin_state(shape, dtype, 0), lin_state(shape, dtype, 1)
    assert not np.array_equal(s0["g"], s1["g"])
    swapped = tg.primal_step_lin(s0["p"], s0["q"], s0["x"], s0["w"], s1["g"], TAU, THETA,
                                 box[0], box[1], _rounded_spacing(shape, dtype), dtype)
    same = tg.primal_step_lin(s0["p"], s0["q"], s0["x"], s0["w"], s0["g"], TAU, THETA,
                              box[0], box[1], _rounded_spacing(shape, dtype), dtype)
    assert np.array_equal(same[0], want_lin(shape, dtype, 0, box)[0])
    assert np.mean(swapped[0] != same[0]) > 0.3
