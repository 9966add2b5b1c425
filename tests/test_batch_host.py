"""Host-side logic of the image stack (nsol_amd/solver_batch.py): which solvers
form a stack, the group-size arithmetic with the per-member observation, the
validation, the declared C entry points and the --slice-wise command line.
No GPU."""
import numpy as np
import pytest


def _solver(shape, seed=0, kind="TVL2", alpha=0.03, iterations=10, dtype=np.float32,
            isotropic=False, alg_type="ALG2", L2=8, scale=1.0):
    from nsol_amd.application.run_denoising import build_solver
    rng = np.random.default_rng(seed)
    obs = scale * (50.0 + 10.0 * rng.standard_normal(shape))
    return build_solver(obs, kind, alpha, iterations, L2=L2, dtype=dtype,
                        alg_type=alg_type, isotropic=isotropic)


def _keys(solvers):
    from nsol_amd.solver_batch import member_key
    return [member_key(s, s.plan()) for s in solvers]


def test_members_that_differ_in_data_scale_and_steps_share_a_key():
    from nsol_amd.solver_batch import plan_stacks
    solvers = [_solver((24, 40), seed=0),
               _solver((24, 40), seed=1, alpha=0.1, scale=3.0),
               _solver((24, 40), seed=2, alg_type="ALG3", L2=16),
               _solver((24, 40), seed=3, alg_type="ALG2_AHMOD")]
    keys = _keys(solvers)
    assert None not in keys and len(set(keys)) == 1
    assert plan_stacks(keys) == [[0, 1, 2, 3]]
    assert len({s.get_x_scale() for s in solvers}) == 4


def test_what_separates_stacks():
    from nsol_amd.observer import Observer
    from nsol_amd.solver_batch import plan_stacks
    base = _solver((24, 40))
    others = [_solver((40, 24)),                        # shape
              _solver((24, 40), dtype=np.float64),      # dtype
              _solver((24, 40), iterations=11),         # iteration count
              _solver((24, 40), kind="TVL1"),           # flags: data term
              _solver((24, 40), kind="HuberL2"),        # flags: regulariser
              _solver((24, 40), isotropic=True),        # flags: isotropic bit
              _solver((960,))]                          # dimension
    keys = _keys([base] + others)
    assert None not in keys and len(set(keys)) == len(keys)
    assert plan_stacks(keys) == []
    # observation points: device-mode observers with the same points stack
    # together, other points or no observer stack apart
    obs = [_solver((24, 40), seed=k) for k in range(4)]
    for s, every in zip(obs[:3], (5, 5, 3)):
        s.set_observer(Observer(keep_iterates=False, every=every))
    keys = _keys(obs)
    assert keys[0] == keys[1] and len({keys[0], keys[2], keys[3]}) == 3
    assert plan_stacks(keys + _keys([base])) == [[0, 1], [3, 4]]


def test_what_runs_on_its_own(monkeypatch):
    from nsol_amd import ops
    from nsol_amd.observer import Observer
    from nsol_amd.primal_dual_solver import PrimalDualSolver
    from nsol_amd.solver_batch import member_key, plan_stacks
    f = lambda x, t: np.asarray(x) * 1.0          # foreign callables: no plan
    foreign = PrimalDualSolver(f, f, f, f, 8, np.zeros(16))
    assert foreign.plan() is None and member_key(foreign, None) is None
    host = _solver((24, 40))
    host.set_observer(Observer())                 # keeps iterates on the host
    assert member_key(host, host.plan()) is None
    none = _solver((24, 40), iterations=0)
    assert member_key(none, none.plan()) is None
    big = _solver((24, 40))
    assert member_key(big, big.plan()) is not None
    monkeypatch.setattr(ops, "PD_BATCH_MAX_VOXELS", 24 * 40 - 1)
    assert member_key(big, big.plan()) is None
    # a stack of one is no stack
    assert plan_stacks([("a",), None, ("b",), ("a",), ("c",)]) == [[0, 3]]


def test_group_size_counts_the_per_member_observation(monkeypatch):
    from nsol_amd import ops
    n, dim, es = 1 << 16, 2, 4
    per_member = (4 + 2 * dim) * n * es          # x, 2 xbar, bt, 2 p of dim parts
    monkeypatch.setattr(ops, "PD_BATCH_GROUP_BYTES", 5 * per_member + 1)
    assert ops.batch_group_size(64, n, dim, es) == 5
    assert ops.batch_group_size(3, n, dim, es) == 3
    # one word per voxel more than a sweep member under the same budget
    monkeypatch.setattr(ops, "PD_SWEEP_GROUP_BYTES", 8 * 7 * n * es)
    monkeypatch.setattr(ops, "PD_BATCH_GROUP_BYTES", 8 * 7 * n * es)
    assert ops.sweep_group_size(64, n, dim, es) == 8
    assert ops.batch_group_size(64, n, dim, es) == 7
    # 3-D: 12 words per voxel
    monkeypatch.setattr(ops, "PD_BATCH_GROUP_BYTES", 12 * (1 << 18) * 4 * 3)
    assert ops.batch_group_size(64, 1 << 18, 3, 4) == 3
    monkeypatch.setattr(ops, "PD_BATCH_GROUP_BYTES", 1)
    assert ops.batch_group_size(64, n, dim, es) == 1     # never less than one
    # all members of a group within the kernel's 2^31 voxels and 65535 members
    monkeypatch.setattr(ops, "PD_BATCH_GROUP_BYTES", 1 << 62)
    assert ops.batch_group_size(4096, 1 << 21, 3, 4) == 1024
    assert ops.batch_group_size(100000, 16, 1, 4) == 65535


def test_constants_start_at_the_sweeps():
    from nsol_amd import ops
    assert ops.PD_BATCH_GROUP_BYTES > 0 and ops.PD_BATCH_MAX_VOXELS > 0
    for name in ("pd_batch_run", "scale_rows", "batch_group_size",
                 "pd_batch_launches"):
        assert callable(getattr(ops, name))


def test_value_errors():
    import nsol_amd
    from nsol_amd.application.run_denoising import wiring
    from nsol_amd.primal_dual_solver import PrimalDualSolver
    from nsol_amd.solver_batch import PrimalDualBatch
    assert nsol_amd.PrimalDualBatch is PrimalDualBatch
    with pytest.raises(ValueError):
        PrimalDualBatch([])
    s = _solver((24, 40))
    with pytest.raises(ValueError):
        PrimalDualBatch([s, "not a solver"])
    with pytest.raises(ValueError):
        PrimalDualBatch([s, _solver((24, 40), seed=1), s])
    w = wiring(np.ones((6, 8)), "TVL2")
    w["x0"] = w["x0"].reshape(6, 8)
    with pytest.raises(ValueError):
        PrimalDualBatch([s, PrimalDualSolver(L2=8, **w)])
    batch = PrimalDualBatch([s, _solver((24, 40), seed=1)])
    assert batch.get_execution() is None and batch.get_group_size() is None
    with pytest.raises(RuntimeError):
        batch.get_x_all_device()


def test_batch_entry_points_are_declared_and_built():
    from nsol_amd import _lib, build
    assert "nsol_pdb.hip" in build.SOURCES
    decl = _lib.declared_symbols()
    for base in ("pd_batch_iter", "pd_batch_run", "scale_rows"):
        for suf in ("f32", "f64"):
            assert "nsol_%s_%s" % (base, suf) in decl
    assert "nsol_pd_batch_launches" in decl
    assert "nsol_scale_rows_f64_to_f32" in decl
    # the run entry has the sweep's signature, bt per member
    assert decl["nsol_pd_batch_run_f32"] == decl["nsol_pd_sweep_run_f32"]
    assert len(decl["nsol_pd_batch_run_f64"][1]) == 27
    # the one-launch entry: the sweep's and the flags that choose the kernel
    assert len(decl["nsol_pd_batch_iter_f32"][1]) == \
        len(decl["nsol_pd_sweep_iter_f32"][1]) + 1


def test_slice_wise_argument_errors(tmp_path, capsys):
    from nsol_amd.application import run_denoising
    vol, img = str(tmp_path / "vol.npy"), str(tmp_path / "img.npy")
    np.save(vol, np.ones((3, 8, 8)))
    np.save(img, np.ones((8, 8)))
    out = str(tmp_path / "out.npy")
    for argv in (["--observation", vol, "--result", out, "--slice-wise",
                  "--alpha", "0.01", "0.1"],
                 ["--observation", vol, "--result", out, "--slice-wise",
                  "--observe-every", "5"],
                 ["--observation", img, "--result", out, "--slice-wise"]):
        with pytest.raises(SystemExit) as e:
            run_denoising.main(argv)
        assert e.value.code == 2
        assert "--slice-wise" in capsys.readouterr().err


def test_slices_without_a_positive_maximum_are_copied_through():
    from nsol_amd.application.run_denoising import classify_slices
    vol = np.ones((5, 4, 6))
    vol[1] = 0.0                    # all zero: wiring() would divide by zero
    vol[3] = -2.0                   # nothing positive
    vol[4, 0, 0] = np.nan           # np.max is NaN: not positive
    assert classify_slices(vol) == ([0, 2], [1, 3, 4])
    assert classify_slices(np.zeros((2, 3, 3))) == ([], [0, 1])
