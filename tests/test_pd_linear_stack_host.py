"""Host-side logic of the stacked forms of PrimalDualLinearSolver
(nsol_amd/linear_stack.py): which solvers form a stack -- one field at a time --, operator
equality by value, the grouping and the group-size arithmetic, the constructors'
refusals, the declared C entry points and the command line.  No GPU."""
import numpy as np
import pytest

from test_pd_linear_host import box_kernel, gaussian_kernel


def _solver(shape=(24, 40), seed=0, kernel=None, op=None, scale=1.0, **kw):
    import nsol_amd
    from nsol_amd.linear_operators import ConvolutionOperator
    rng = np.random.default_rng(seed)
    obs = scale * (50.0 + 10.0 * rng.standard_normal(shape))
    if op is None:
        op = ConvolutionOperator(len(shape), gaussian_kernel(len(shape), 1.)
                                 if kernel is None else kernel)
    A = lambda x: op(x.reshape(*shape)).flatten()
    args = dict(A=A, A_adj=A, b=obs.flatten(), x0=obs.flatten(), dimension=len(shape),
                alpha=0.05, iterations=10, x_scale=float(obs.max()), dtype=np.float32)
    args.update(kw)
    if "A" in kw:
        args["shape"] = shape       # a foreign A does not tell the volume's shape
    return nsol_amd.PrimalDualLinearSolver(**args)


def _keys(solvers):
    from nsol_amd.linear_stack import member_key
    return [member_key(s) for s in solvers]


# ------------------------------------------------------------------ the member key
def test_members_that_differ_in_data_alpha_scale_and_weights_share_a_key():
    from nsol_amd.solver_batch import plan_stacks
    w = np.ones(24 * 40)
    w[::7] = 0
    solvers = [_solver(seed=0, weights=np.ones(24 * 40)),
               _solver(seed=1, alpha=0.2, scale=3.0, weights=w),
               _solver(seed=2, alpha=0.01, weights=2.5 * w)]
    keys = _keys(solvers)
    assert None not in keys and len(set(keys)) == 1
    assert plan_stacks(keys) == [[0, 1, 2]]
    assert len({s.get_x_scale() for s in solvers}) == 3
    # every solver here built an operator of its own: equal by value is enough
    assert len({id(s._op) for s in solvers}) == 3


@pytest.mark.parametrize("kw", [
    dict(shape=(40, 24)), dict(shape=(960,)), dict(dtype=np.float64),
    dict(iterations=11), dict(reg_type="huber"), dict(reg_type="huber", huber_gamma=0.1),
    dict(isotropic=True), dict(data_loss="ell1"), dict(bounds=(0., np.inf)),
    dict(spacing=(1., 2.)), dict(tau=0.2), dict(sigma=0.2),
    dict(weights=np.ones(960)), dict(kernel=gaussian_kernel(2, 1.5)),
    dict(kernel=box_kernel(2))], ids=lambda kw: "-".join(sorted(kw)))
def test_every_field_separates_a_stack(kw):
    from nsol_amd.solver_batch import plan_stacks
    base = _solver(reg_type="huber") if kw == dict(reg_type="huber", huber_gamma=0.1) \
        else _solver()
    keys = _keys([base, _solver(seed=1, **kw)])
    assert None not in keys and keys[0] != keys[1]
    assert plan_stacks(keys) == []


def test_the_boundary_mode_separates_a_stack():
    from nsol_amd.linear_operators import ConvolutionOperator
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
    from nsol_amd.linear_stack import member_key
    from nsol_amd.observer import Observer
    assert member_key(_solver(tolerance=1e-3)) is None
    assert member_key(_solver(verbose=1)) is None
    assert member_key(_solver(iterations=0)) is None
    host = _solver()
    host.set_observer(Observer())                 # keeps iterates on the host
    assert member_key(host) is None
    foreign = lambda x: np.asarray(x) * 0.5       # a NumPy-only callable
    assert member_key(_solver(A=foreign, A_adj=foreign, A_norm2=0.25)) is None
    assert member_key("not a solver") is None
    assert member_key(_solver()) is not None


# ------------------------------------------------------------------ operators
def test_operator_equality_is_by_value():
    from nsol_amd.linear_operators import ConvolutionOperator
    from nsol_amd.linear_stack import operator_key, operators_equal
    k = gaussian_kernel(2, 1.)
    a, b = ConvolutionOperator(2, k), ConvolutionOperator(2, k.copy())
    assert operators_equal(a, a) and operators_equal(a, b)
    assert operator_key(a) == operator_key(b) and hash(operator_key(a)) is not None
    other = k.copy()
    other[0, 0] = np.nextafter(other[0, 0], 1.)              # one bit of one tap
    for c in (ConvolutionOperator(2, other), ConvolutionOperator(2, k, "mirror"),
              ConvolutionOperator(2, k[1:]), ConvolutionOperator(1, k[3])):
        assert not operators_equal(a, c) and operator_key(a) != operator_key(c)
    assert not operators_equal(a, "not an operator")


def test_launch_counts_per_iteration_by_dimension():
    from nsol_amd.linear_stack import launches_per_iteration
    # 2-D separable: 2 + 1 + 2 + 1 for the stack, that per member for the loop
    assert launches_per_iteration(_solver((24, 40)), 16) == (6, 96)
    assert launches_per_iteration(_solver((960,)), 16) == (4, 64)
    # 3-D, the one-pass blur per member: 2 P + 2 against 4 P
    assert launches_per_iteration(_solver((8, 10, 12)), 8) == (18, 32)
    # dense taps: per member
    dense = np.array([[0., 0.2, 0.], [0.2, 0.2, 0.2], [0., 0.2, 0.]])
    assert launches_per_iteration(_solver(kernel=dense), 5) == (12, 20)


# ------------------------------------------------------------------ groups
def test_group_size_counts_what_a_member_owns(monkeypatch):
    from nsol_amd import ops
    n, dim, es = 1 << 16, 2, 4
    word = n * es
    # x, two xbar, q, g and two p of dim parts: 5 + 2 dim; + bt, + weights, + t
    monkeypatch.setattr(ops, "PDL_STACK_GROUP_BYTES", 4 * (5 + 2 * dim) * word)
    assert ops.pdl_group_size(64, n, dim, es, own_data=False, with_t=False) == 4
    assert ops.pdl_group_size(3, n, dim, es, own_data=False, with_t=False) == 3
    monkeypatch.setattr(ops, "PDL_STACK_GROUP_BYTES", 4 * 12 * word)
    assert ops.pdl_group_size(64, n, dim, es, own_data=False, with_t=False) == 5
    assert ops.pdl_group_size(64, n, dim, es, own_data=True, with_t=False) == 4
    assert ops.pdl_group_size(64, n, dim, es, own_data=True, with_t=True) == 4
    assert ops.pdl_group_size(64, n, dim, es, own_data=True, own_weights=True,
                              with_t=True) == 4
    assert ops.pdl_group_size(64, n, dim, es, own_data=True, own_weights=True,
                              with_t=True) == (4 * 12) // 12
    monkeypatch.setattr(ops, "PDL_STACK_GROUP_BYTES", 4 * 12 * word - 1)
    assert ops.pdl_group_size(64, n, dim, es, own_data=True, own_weights=True) == 3
    monkeypatch.setattr(ops, "PDL_STACK_GROUP_BYTES", 1)
    assert ops.pdl_group_size(64, n, dim, es) == 1          # never less than one
    # all members of a group within the kernels' 2^31 voxels and 65535 members
    monkeypatch.setattr(ops, "PDL_STACK_GROUP_BYTES", 1 << 62)
    assert ops.pdl_group_size(4096, 1 << 21, 3, 4) == 1024
    assert ops.pdl_group_size(100000, 16, 1, 4) == 65535
    assert ops.sweep_groups(5, 2) == [(0, 2), (2, 4), (4, 5)]


# ------------------------------------------------------------------ refusals
def test_the_batch_refuses():
    import nsol_amd
    from nsol_amd.application.run_denoising import build_solver
    from nsol_amd.linear_stack import PrimalDualLinearBatch
    assert nsol_amd.PrimalDualLinearBatch is PrimalDualLinearBatch
    with pytest.raises(ValueError, match="at least one"):
        PrimalDualLinearBatch([])
    s = _solver()
    with pytest.raises(ValueError, match="PrimalDualLinearSolver"):
        PrimalDualLinearBatch([s, build_solver(np.ones((6, 8)), "TVL2", 0.03, 5)])
    with pytest.raises(ValueError, match="PrimalDualLinearSolver"):
        PrimalDualLinearBatch([s, "not a solver"])
    with pytest.raises(ValueError, match="twice"):
        PrimalDualLinearBatch([s, _solver(seed=1), s])
    with pytest.raises(ValueError, match="1D"):
        PrimalDualLinearBatch([s, _solver(x0=np.ones((24, 40)))])
    batch = PrimalDualLinearBatch([s, _solver(seed=1)])
    assert batch.get_solvers() == [s, batch.get_solvers()[1]]
    assert batch.get_execution() is None and batch.get_group_size() is None
    with pytest.raises(RuntimeError):
        batch.get_x_all_device()


def test_the_sweep_refuses():
    import nsol_amd
    from nsol_amd.linear_operators import ConvolutionOperator
    from nsol_amd.linear_stack import PrimalDualLinearSweep
    assert nsol_amd.PrimalDualLinearSweep is PrimalDualLinearSweep
    shape = (6, 8)
    op = ConvolutionOperator(2, gaussian_kernel(2, 1.))
    A = lambda x: op(x.reshape(*shape)).flatten()
    obs = 1. + np.arange(48, dtype=float)
    make = lambda parameters, **kw: PrimalDualLinearSweep(A, A, obs, obs, 2,
                                                          parameters=parameters, **kw)
    for key in ("L2", "alg_type", "tau"):
        with pytest.raises(ValueError, match="alpha"):
            make({"alpha": [0.1], key: [1]})
    with pytest.raises(ValueError):
        make({})
    with pytest.raises(ValueError):
        make({"alpha": []})
    with pytest.raises(ValueError):                       # the solver's own refusals
        make({"alpha": [0.1, 0.2]}, data_loss="huber")
    with pytest.raises(ValueError):
        make({"alpha": [-1., 0.2]})
    sweep = make({"alpha": [0.1, 0.2, 0.4]}, iterations=7, reg_type="huber",
                 tolerance=1e-3)
    assert sweep.get_parameters() == [{"alpha": 0.1}, {"alpha": 0.2}, {"alpha": 0.4}]
    assert sweep.get_execution() is None and sweep.get_iterations_done() is None
    assert sweep.get_group_size() is None
    with pytest.raises(RuntimeError):
        sweep.get_x_all_device()
    with pytest.raises(ValueError):
        sweep.set_measures({}, every=0)


# ------------------------------------------------------------------ the C ABI
def test_the_new_symbols_are_declared_and_built():
    from nsol_amd import _lib, build, ops
    sym = _lib.declared_symbols()
    for name in ("nsol_pdl_stack_iter_f32", "nsol_pdl_stack_iter_f64",
                 "nsol_pdl_stack_dual_data_f32", "nsol_pdl_stack_dual_data_f64",
                 "nsol_pdl_stack_launches"):
        assert name in sym, name
    # the single entries' arguments plus `members`; the q update's plus two strides,
    # the lambdas as a pointer and `members`
    assert len(sym["nsol_pdl_stack_iter_f64"][1]) == len(sym["nsol_pdl_iter_f64"][1]) + 1
    assert len(sym["nsol_pdl_stack_dual_data_f32"][1]) == \
        len(sym["nsol_pdl_dual_data_f32"][1]) + 3
    assert sym["nsol_pdl_stack_launches"][1] == []
    assert "nsol_pdls.hip" in build.SOURCES and "nsol_pdl.hip" in build.SOURCES
    for name in ("pdl_stack_iter", "pdl_stack_dual_data", "pdl_stack_launches",
                 "pdl_group_size", "pdl_lambdas"):
        assert callable(getattr(ops, name))


def test_the_entries_decline_before_any_launch():
    """What the stacked entries refuse, they refuse on the host before a kernel is
    launched, so the calls can be made without a device (the pointers are compared,
    never followed).  -2: members < 1 or > 65535, members * n over 2^31, a geometry
    nsol_pdl_iter_* declines; -1: everything that is an invalid argument."""
    from nsol_amd import _lib
    lib = _lib.load()
    A = [0x1000 * (k + 1) for k in range(6)]
    n = 4 * 5 * 6
    for suf in ("f32", "f64"):
        it = getattr(lib, "nsol_pdl_stack_iter_" + suf)
        dd = getattr(lib, "nsol_pdl_stack_dual_data_" + suf)

        def call(members=2, dims=(3, 4, 5, 6), lo=-np.inf, hi=np.inf, flags=0,
                 sigma=0.3, ptrs=A):
            return it(*ptrs, members, *dims, 1., 1., 1., sigma, 1., 0.3, 1., lo, hi,
                      flags, 1, None)
        assert [call(m) for m in (0, -1, 65536)] == [-2] * 3
        assert call(3, (3, 1 << 10, 1 << 10, 1 << 10)) == -2
        assert call(2, (3, 1 << 10, 1 << 10, (1 << 10) + 1)) == -2
        for dims in ((4, 4, 5, 6), (0, 1, 1, n), (2, 4, 5, 6), (3, 0, 5, 6)):
            assert call(dims=dims) == -2, dims
        for k in range(6):
            ptrs = list(A)
            ptrs[k] = None
            assert call(ptrs=ptrs) == -1, k
        assert call(ptrs=[A[0], A[0]] + A[2:]) == -1            # xbar_in == xbar_out
        assert call(ptrs=A[:4] + [A[4], A[4]]) == -1            # p_in == p_out
        assert call(lo=1., hi=0.) == -1 and call(lo=np.nan, hi=1.) == -1
        assert call(flags=2) == -1 and call(flags=8) == -1      # data flags
        assert call(sigma=0.) == -1 and call(sigma=-1.) == -1

        def data(q=A[0], t=None, bt=A[1], bts=0, wt=None, wts=0, sigma=0.3, lm=A[2],
                 members=2, size=n):
            return dd(q, t, bt, bts, wt, wts, sigma, lm, 0, members, size, None)
        assert [data(members=m) for m in (0, -1, 65536)] == [-2] * 3
        assert data(size=(1 << 30) + 1) == -2 and data(size=-1) == -1
        assert data(size=0) == 0
        for bad in (1, n - 1, 2 * n, -n):
            assert data(bts=bad) == -1 and data(wt=A[3], wts=bad) == -1, bad
        assert data(q=None) == -1 and data(bt=None) == -1 and data(lm=None) == -1
        assert data(t=A[0]) == -1 and data(sigma=0.) == -1


# ------------------------------------------------------------------ command line
def _cli(argv, obs="o.nii.gz"):
    from nsol_amd.application import run_deconvolution
    return run_deconvolution.main(["--observation", obs, "--result", "r.nii.gz"] + argv)


@pytest.mark.parametrize("argv, word", [
    (["--solver", "PD", "--result-dir", "d"], "--solver PDL"),
    (["--solver", "ADMM", "--result-dir", "d"], "--solver PDL"),
    (["--solver", "PD", "--slice-wise"], "--solver PDL"),
    (["--solver", "ADMM", "--slice-wise"], "--solver PDL"),
    (["--result-dir", "d"], "--solver PDL"),                       # the default is PD
    (["--solver", "PDL", "--slice-wise", "--result-dir", "d"], "--slice-wise"),
    (["--solver", "PDL", "--slice-wise", "--alpha", "0.01", "0.1"], "--slice-wise"),
    (["--solver", "PDL", "--slice-wise", "--observe-every", "5"], "--slice-wise")])
def test_cli_refusals_exit_with_status_2(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        _cli(argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_cli_slice_wise_needs_a_3d_file(tmp_path, capsys):
    img = str(tmp_path / "img.npy")
    np.save(img, np.ones((8, 8)))
    with pytest.raises(SystemExit) as e:
        _cli(["--solver", "PDL", "--slice-wise"], obs=img)
    assert e.value.code == 2
    assert "--slice-wise needs a 3-D observation, not 2-D" in capsys.readouterr().err


def test_cli_new_options_pass_the_argument_checks(monkeypatch):
    """--tolerance composes with either, and so do the options of --solver PDL: the
    run gets as far as reading the observation."""
    from nsol_amd import data_reader

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(data_reader, "DataReader", stop)
    for extra in (["--result-dir", "d", "--alpha", "0.02", "0.05"],
                  ["--result-dir", "d", "--alpha", "0.02", "0.05", "--tolerance", "1e-3",
                   "--mask", "m.nii.gz", "--data-loss", "ell1", "--nonnegative",
                   "--isotropic", "--observe-every", "5"],
                  ["--slice-wise"],
                  ["--slice-wise", "--weights", "w.nii.gz", "--tolerance", "1e-3"]):
        with pytest.raises(Reached):
            _cli(["--solver", "PDL"] + extra)


class _FakeSolver(object):
    """What main() asks of a solver, without a device."""
    made = []

    def __init__(self, nda, alpha):
        self._nda, self.alpha, self.observer = nda, alpha, None
        _FakeSolver.made.append(self)

    def set_observer(self, obs):
        self.observer = obs

    def run(self):
        pass

    def get_x(self):
        return (self._nda * self.alpha).flatten()

    def get_computational_time(self):
        return "0:00:00"


def test_cli_without_the_new_options_is_the_loop_it_was(monkeypatch, tmp_path, capsys):
    """Several --alpha without --result-dir: one build_solver call per alpha with the
    arguments as before, one line each, every member written to --result so that the
    last survives."""
    from nsol_amd.application import run_deconvolution
    obs, out = str(tmp_path / "obs.npy"), str(tmp_path / "out.npy")
    vol = 1. + np.arange(48, dtype=float).reshape(6, 8)
    np.save(obs, vol)
    calls = []
    del _FakeSolver.made[:]

    def fake(nda, spacing, blur, rtype, tv_solver, alpha, iterations, *rest, **kw):
        calls.append((tv_solver, alpha, iterations, sorted(kw), len(rest)))
        return _FakeSolver(nda, alpha)
    monkeypatch.setattr(run_deconvolution, "build_solver", fake)

    def no_stack(*a, **k):
        raise AssertionError("the stacked forms ran without their options")
    monkeypatch.setattr(run_deconvolution, "run_sweep", no_stack)
    monkeypatch.setattr(run_deconvolution, "run_slice_wise", no_stack)
    assert run_deconvolution.main(["--observation", obs, "--result", out, "--solver",
                                   "PDL", "--alpha", "0.5", "2", "--iterations",
                                   "7"]) == 0
    kws = ["check_every", "isotropic", "nonnegative", "pdl_data_loss", "tolerance",
           "weights"]
    assert calls == [("PDL", 0.5, 7, kws, 8), ("PDL", 2.0, 7, kws, 8)]
    assert capsys.readouterr().out.splitlines() == ["TVL2 alpha=0.5: 0:00:00",
                                                    "TVL2 alpha=2: 0:00:00"]
    assert np.array_equal(np.load(out), 2. * vol)
    assert all(s.observer is None for s in _FakeSolver.made)


def test_cli_wiring_is_build_solvers():
    """pdl_wiring, which the sweep is built from, and build_solver configure the same
    solver."""
    import nsol_amd
    from nsol_amd.application import run_deconvolution as rd
    obs = 10. + np.arange(48, dtype=float).reshape(6, 8)
    w = np.ones((6, 8))
    w[-1] = 0
    junk = obs.copy()
    junk[-1] = np.nan
    kw = rd.pdl_wiring(junk, np.ones(2), 1.0, "HuberL2", 0.02, 7, dtype=np.float64,
                       isotropic=True, weights=w, pdl_data_loss="ell1",
                       nonnegative=True, tolerance=1e-3, check_every=4)
    a = nsol_amd.PrimalDualLinearSolver(**kw)
    b = rd.build_solver(junk, np.ones(2), 1.0, "HuberL2", "PDL", 0.02, 7,
                        dtype=np.float64, isotropic=True, weights=w,
                        pdl_data_loss="ell1", nonnegative=True, tolerance=1e-3,
                        check_every=4)
    for get in ("get_reg_type", "get_data_loss", "get_isotropic", "get_bounds",
                "get_x_scale", "get_tolerance", "get_check_every", "get_alpha",
                "get_iterations", "get_shape", "get_tau", "get_sigma", "get_dtype"):
        assert getattr(a, get)() == getattr(b, get)(), get
    assert np.array_equal(a.get_x0(), b.get_x0())
    assert a.get_x_scale() == obs[:-1].max()
