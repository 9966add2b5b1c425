"""The image stack (nsol_amd/solver_batch.py, nsol_pd_batch_run_*) on a real MI355X:
every member bit-identical to its own PrimalDualSolver.run(), the oracle anchors,
groups, the launch count, mixed lists, device-mode observers, scale_rows, the
declined geometry and the --slice-wise command line."""
import numpy as np
import pytest

from conftest import rel_l2
from test_pd_isotropic_host import pd_iso_denoise

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12     # float64 kernels vs the float64 reference / restatement
ITERS = 25
# rows of whole 16-byte vectors and not, in every dimension
SHAPES = [(1000,), (1027,), (72, 100), (37, 53), (24, 20, 32), (15, 17, 19)]
# what may differ from member to member, next to the data and its scale
MEMBERS = [dict(alpha=0.003, alg_type="ALG2", L2=16.0),
           dict(alpha=0.01, alg_type="ALG2_AHMOD", L2=16.0),
           dict(alpha=0.03, alg_type="ALG3", L2=24.0),
           dict(alpha=0.1, alg_type="ALG2", L2=32.0),
           dict(alpha=0.3, alg_type="ALG3", L2=16.0)]


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _image(shape, seed=0):
    """(clean, observed): every seed its own noise, level and hence x_scale."""
    rng = np.random.default_rng(seed)
    clean = np.full(shape, 20.0)
    clean[tuple(slice(s // 4, 3 * s // 4) for s in shape)] = 100.0
    clean = clean * (1.0 + 0.37 * seed)
    return clean, clean + 12.0 * rng.standard_normal(shape)


def _solver(obs, reg, data, dtype, member, iters=ITERS, iso=False):
    from nsol_amd.application.run_denoising import build_solver
    return build_solver(obs, reg + data, member["alpha"], iters, L2=member["L2"],
                        dtype=dtype, alg_type=member["alg_type"], isotropic=iso)


def _stack(shape, reg, data, dtype, iso=False, iters=ITERS, members=MEMBERS):
    obs = [_image(shape, seed=k)[1] for k in range(len(members))]
    make = lambda: [_solver(o, reg, data, dtype, m, iters, iso)
                    for o, m in zip(obs, members)]
    return obs, make


def _assert_same_bits(batch_solvers, single_solvers):
    for k, (got, one) in enumerate(zip(batch_solvers, single_solvers)):
        one.run()
        a, b = got.get_x_device(), one.get_x_device()
        assert a.dtype == b.dtype
        assert bool((a == b).all()), k
        assert np.array_equal(got.get_x(), one.get_x()), k


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("data", ["L2", "L1"])
@pytest.mark.parametrize("reg", ["TV", "Huber"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stacked_members_are_bit_identical_to_their_own_runs(nsol, shape, dtype, reg,
                                                             data, iso):
    from nsol_amd import PrimalDualBatch
    _, make = _stack(shape, reg, data, dtype, iso)
    solvers = make()
    assert len({s.get_x_scale() for s in solvers}) == len(solvers)
    batch = PrimalDualBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["stacked"] * len(solvers)
    assert batch.get_group_size() == len(solvers)
    assert all(s.get_execution() == "fused" for s in solvers)
    singles = make()
    _assert_same_bits(solvers, singles)
    assert all(s.get_execution() == "fused" for s in singles)
    allx = batch.get_x_all_device()
    assert tuple(allx.shape) == (len(solvers), int(np.prod(shape)))
    for k, one in enumerate(singles):
        assert bool((allx[k] == one.get_x_device()).all()), k
        assert np.array_equal(batch.get_x(k), one.get_x())


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(37, 53), (72, 100), (15, 17, 19)],
                         ids=lambda s: "x".join(map(str, s)))
def test_groups_of_two_equal_the_ungrouped_stack(nsol, shape, dtype, iso, monkeypatch):
    from nsol_amd import PrimalDualBatch, ops
    _, make = _stack(shape, "TV", "L2", dtype, iso)
    whole = PrimalDualBatch(make())
    whole.run()
    assert whole.get_group_size() == 5
    n, dim = int(np.prod(shape)), len(shape)
    # the byte budget of two members' state: x, two xbar, bt, two dim-component p
    monkeypatch.setattr(ops, "PD_BATCH_GROUP_BYTES",
                        2 * (4 + 2 * dim) * n * np.dtype(dtype).itemsize)
    before = ops.pd_batch_launches()
    solvers = make()
    grouped = PrimalDualBatch(solvers)
    grouped.run()
    assert grouped.get_execution() == ["stacked"] * 5
    assert grouped.get_group_size() == 2
    assert ops.pd_batch_launches() - before == 3 * ITERS
    assert bool((grouped.get_x_all_device() == whole.get_x_all_device()).all())
    _assert_same_bits(solvers, make())


@pytest.mark.parametrize("flags_iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(1027,), (37, 53), (24, 20, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_batch_iter_leaves_the_slices_of_fused_iter(nsol, shape, dtype, flags_iso):
    """x, xbar and p of every member after k nsol_pd_batch_iter calls against k
    nsol_pd_fused_iter calls on that member alone."""
    import ctypes
    import torch
    from nsol_amd import _lib, ops
    from nsol_amd.primal_dual_solver import step_schedule
    lib = _lib.load()
    K, P = 4, 3
    n, dim = int(np.prod(shape)), len(shape)
    ndim, nz, ny, nx = ops.dims3(shape)
    td = torch.float32 if dtype == np.float32 else torch.float64
    suf = "f32" if dtype == np.float32 else "f64"
    flags = ops.PD_REG_HUBER | ops.PD_DATA_L2 | (ops.PD_REG_ISOTROPIC if flags_iso else 0)
    gamma, w = 0.05, (1.0, 1.0, 1.0)
    rng = np.random.default_rng(11)
    bt = torch.from_numpy(rng.random((P, n)).astype(dtype)).cuda().view(-1)
    lm = np.array([1 / m["alpha"] for m in MEMBERS[:P]])
    sched = [step_schedule(m["alg_type"], m["L2"], l, K) for m, l in zip(MEMBERS, lm)]
    sig, ta, th = (np.ascontiguousarray([s[j] for s in sched]) for j in range(3))
    dev = lambda *size: torch.empty(*size, dtype=td, device="cuda")
    # the run entry fills the table (and runs K iterations on arrays of its own)
    entry = lib.nsol_pd_sweep_entry_bytes(np.dtype(dtype).itemsize)
    nbytes = entry * P * K
    tab_host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    tab = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    x_run, xb_run = bt.clone(), [bt.clone(), dev(P * n)]
    p_run = [dev(P * dim * n), dev(P * dim * n)]
    slot = ctypes.c_int(-1)
    run = getattr(lib, "nsol_pd_batch_run_" + suf)
    assert run(xb_run[0].data_ptr(), xb_run[1].data_ptr(), x_run.data_ptr(),
               bt.data_ptr(), p_run[0].data_ptr(), p_run[1].data_ptr(), P, ndim, nz,
               ny, nx, *w, lm.ctypes.data, sig.ctypes.data, ta.ctypes.data,
               th.ctypes.data, K, 1, gamma, flags, tab_host.data_ptr(),
               tab.data_ptr(), nbytes, ctypes.addressof(slot), None) == 0
    assert slot.value == K & 1
    torch.cuda.synchronize()
    # K one-launch calls on fresh arrays
    x, xb = bt.clone(), [bt.clone(), dev(P * n)]
    p = [dev(P * dim * n), dev(P * dim * n)]
    it = getattr(lib, "nsol_pd_batch_iter_" + suf)
    before = ops.pd_batch_launches()
    for i in range(K):
        k = i & 1
        assert it(xb[k].data_ptr(), xb[1 - k].data_ptr(), x.data_ptr(), bt.data_ptr(),
                  p[k].data_ptr(), p[1 - k].data_ptr(), P, ndim, nz, ny, nx, *w,
                  tab.data_ptr(), i, flags, None) == 0
    assert ops.pd_batch_launches() - before == K
    torch.cuda.synchronize()
    assert bool((x == x_run).all()) and bool((xb[K & 1] == xb_run[K & 1]).all())
    assert bool((p[K & 1] == p_run[K & 1]).all())
    for m in range(P):
        b1 = bt[m * n:(m + 1) * n].clone()
        x1, xb1 = b1.clone(), [b1.clone(), dev(n)]
        p1 = [dev(dim * n), dev(dim * n)]
        for i in range(K):
            k = i & 1
            ops.pd_fused_iter(xb1[k], xb1[1 - k], x1, b1, None if i == 0 else p1[k],
                              p1[1 - k], shape, w, sig[m, i],
                              1. + sig[m, i] * gamma, ta[m, i], ta[m, i] * lm[m],
                              th[m, i], flags)
        torch.cuda.synchronize()
        assert bool((x[m * n:(m + 1) * n] == x1).all()), m
        assert bool((xb[K & 1][m * n:(m + 1) * n] == xb1[K & 1]).all()), m
        assert bool((p[K & 1][m * dim * n:(m + 1) * dim * n] == p1[K & 1]).all()), m


def test_an_anisotropic_stack_matches_the_oracle_in_float64(nsol):
    from nsol_amd import PrimalDualBatch
    from oracle import nsol_oracle as orc
    shape = (72, 100)
    for reg, data in (("TV", "L2"), ("Huber", "L1")):
        obs, make = _stack(shape, reg, data, np.float64)
        solvers = make()
        batch = PrimalDualBatch(solvers)
        batch.run()
        assert batch.get_execution() == ["stacked"] * len(solvers)
        errs = []
        for k, (o, m) in enumerate(zip(obs, MEMBERS)):
            ref = orc.primal_dual_denoise(o.flatten(), shape, reg, data, m["alpha"],
                                          ITERS, m["L2"], m["alg_type"])
            assert np.all(np.isfinite(ref)), m
            errs.append(rel_l2(batch.get_x(k), ref, "%s%s %s" % (reg, data, m)))
        print("oracle rel-L2 per member:", errs)
        assert max(errs) <= F64_TOL, errs


def test_an_isotropic_stack_matches_the_restatement_in_float64(nsol):
    from nsol_amd import PrimalDualBatch
    for shape in ((37, 53), (15, 17, 19)):
        for reg, data in (("TV", "L2"), ("Huber", "L1")):
            obs, make = _stack(shape, reg, data, np.float64, iso=True)
            solvers = make()
            batch = PrimalDualBatch(solvers)
            batch.run()
            assert batch.get_execution() == ["stacked"] * len(solvers)
            errs = []
            for k, (o, m) in enumerate(zip(obs, MEMBERS)):
                ref = pd_iso_denoise(o.flatten(), shape, reg, data, m["alpha"], ITERS,
                                     m["L2"], m["alg_type"])
                errs.append(rel_l2(batch.get_x(k), ref,
                                   "iso %s %s%s %s" % (shape, reg, data, m)))
            print("restatement rel-L2 per member:", errs)
            assert max(errs) <= F64_TOL, errs


def test_one_launch_per_iteration_and_none_for_a_sequential_run(nsol):
    from nsol_amd import PrimalDualBatch, ops
    _, make = _stack((72, 100), "TV", "L2", np.float32)
    before = ops.pd_batch_launches()
    batch = PrimalDualBatch(make())
    batch.run()
    assert batch.get_execution() == ["stacked"] * 5
    assert ops.pd_batch_launches() - before == ITERS          # not 5 * 25
    # a stack of one runs as the solver itself
    before = ops.pd_batch_launches()
    alone = make()[:1]
    batch = PrimalDualBatch(alone)
    batch.run()
    assert batch.get_execution() == ["sequential"]
    assert batch.get_group_size() is None
    assert ops.pd_batch_launches() == before
    _assert_same_bits(alone, make()[:1])


def test_members_over_the_size_limit_run_sequentially(nsol, monkeypatch):
    from nsol_amd import PrimalDualBatch, ops
    shape = (24, 20, 32)
    _, make = _stack(shape, "TV", "L2", np.float32)
    monkeypatch.setattr(ops, "PD_BATCH_MAX_VOXELS", int(np.prod(shape)) - 1)
    before = ops.pd_batch_launches()
    solvers = make()
    batch = PrimalDualBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["sequential"] * 5
    assert ops.pd_batch_launches() == before
    _assert_same_bits(solvers, make())


def _foreign(obs, member, iters):
    """A prox the symbolic probe cannot see through: a host round trip."""
    from nsol_amd.application.run_denoising import wiring
    from nsol_amd.primal_dual_solver import PrimalDualSolver
    from nsol_amd.proximal_operators import ProximalOperators as prox
    w = wiring(obs, "TVL2")
    b, xs = obs.flatten(), w["x_scale"]
    w["prox_f"] = lambda x, tau: np.asarray(
        prox.prox_ell2_denoising(np.asarray(x), tau, x0=b, x_scale=xs))
    return PrimalDualSolver(L2=member["L2"], alpha=member["alpha"], iterations=iters,
                            alg_type=member["alg_type"], dtype=np.float32, **w)


def test_a_mixed_list_gives_two_stacks_and_one_sequential_member(nsol):
    from nsol_amd import PrimalDualBatch, ops
    iters = 8
    a = [_image((37, 53), seed=k)[1] for k in range(3)]
    b = [_image((24, 40), seed=k + 5)[1] for k in range(2)]
    f = _image((37, 53), seed=9)[1]

    def make():
        sa = [_solver(o, "TV", "L2", np.float32, m, iters) for o, m in zip(a, MEMBERS)]
        sb = [_solver(o, "Huber", "L1", np.float32, m, iters, iso=True)
              for o, m in zip(b, MEMBERS[3:])]
        # interleaved: the stacks are found by key, not by position
        return [sa[0], sb[0], sa[1], _foreign(f, MEMBERS[1], iters), sb[1], sa[2]]
    solvers = make()
    before = ops.pd_batch_launches()
    batch = PrimalDualBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["stacked", "stacked", "stacked", "sequential",
                                     "stacked", "stacked"]
    assert ops.pd_batch_launches() - before == 2 * iters
    assert solvers[3].get_execution() != "fused"
    _assert_same_bits(solvers, make())
    with pytest.raises(ValueError):
        batch.get_x_all_device()          # two lengths


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_observers_on_a_stack_equal_those_of_single_runs(nsol, dtype):
    from nsol_amd import PrimalDualBatch
    from nsol_amd.observer import Observer, observation_points
    from nsol_amd.prior_measures import PriorMeasures as PM
    from nsol_amd.similarity_measures import SimilarityMeasures as SM
    shape = (72, 100)
    pairs = [_image(shape, seed=k) for k in range(len(MEMBERS))]

    def make():
        out = []
        for (clean, obs), m in zip(pairs, MEMBERS):
            s = _solver(obs, "TV", "L2", dtype, m)
            x_ref = clean.flatten()
            measures = {k: (lambda x, k=k, r=x_ref: SM.similarity_measures[k](x, r))
                        for k in ("PSNR", "SSD", "NCC")}
            measures["TV"] = lambda x, D=s._B: PM.total_variation(x, D, 2)
            o = Observer(keep_iterates=False, every=5)
            o.set_measures(measures)
            s.set_observer(o)
            out.append(s)
        return out
    solvers = make()
    batch = PrimalDualBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["stacked"] * len(solvers)
    singles = make()
    _assert_same_bits(solvers, singles)
    for k, (got, one) in enumerate(zip(solvers, singles)):
        og, oo = got.get_observer(), one.get_observer()
        og.compute_measures()
        oo.compute_measures()
        assert set(oo.get_measure_classes().values()) == {"board"}
        assert og.get_measure_classes() == oo.get_measure_classes()
        assert og.get_observed_iterations() == observation_points(ITERS, 5)
        assert og.get_observed_iterations() == oo.get_observed_iterations()
        for name in ("PSNR", "SSD", "NCC", "TV"):
            a, b = og.get_measures()[name], oo.get_measures()[name]
            assert a.shape == (6,) and np.array_equal(a, b), (k, name, a, b)
    # other observation points: stacked apart, a host-mode observer: sequential
    solvers = make()
    solvers[4].get_observer().set_every(4)
    solvers[3].get_observer().set_every(4)
    solvers[2].set_observer(Observer())
    batch = PrimalDualBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["stacked", "stacked", "sequential", "stacked",
                                     "stacked"]
    assert solvers[3].get_observer().get_observed_iterations() == \
        observation_points(ITERS, 4)
    assert len(solvers[2].get_observer()._x_list) == ITERS + 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 77, 4096, 100003])
def test_scale_rows_equals_scale_row_by_row(nsol, n, dtype):
    import torch
    from nsol_amd import ops
    P = 7
    rng = np.random.default_rng(n)
    host = (50.0 + 30.0 * rng.standard_normal((P, n)))
    scales = np.array([3.0, 0.1, 117.3, 1.0, 1e-3, 7.0 / 3.0, 255.0])
    s = torch.from_numpy(scales).cuda()
    x = torch.from_numpy(host.astype(dtype)).cuda()
    for divide in (True, False):
        got = ops.scale_rows(x, s, P, divide=divide)
        assert got.dtype == x.dtype and tuple(got.shape) == (P, n)
        for m in range(P):
            want = ops.scale(x[m].contiguous(), scales[m], divide=divide)
            assert bool((got[m] == want).all()), (m, divide)
    # float64 data, divided in float64 and rounded once: the scaled observation
    x64 = torch.from_numpy(host).cuda()
    td = torch.float32 if dtype == np.float32 else torch.float64
    got = ops.scale_rows(x64, s, P, divide=True, dtype=td)
    assert got.dtype == td
    for m in range(P):
        want = ops.scale(x64[m].contiguous(), scales[m], divide=True).to(td)
        assert bool((got[m] == want).all()), m
    with pytest.raises(ValueError):
        ops.scale_rows(x, s[:3], P)
    with pytest.raises(ValueError):
        ops.scale_rows(x, s.float(), P)


def test_library_declines_with_minus_two_and_the_batch_falls_back(nsol, monkeypatch):
    import torch
    from nsol_amd import PrimalDualBatch, _lib, ops
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    one = np.ones(1)
    before = ops.pd_batch_launches()
    for flags in (0, ops.PD_REG_ISOTROPIC):
        for members, nx in ((0, 16), (3, 1 << 30), (65536, 16)):
            rc = lib.nsol_pd_batch_run_f32(
                t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                t.data_ptr(), members, 1, 1, 1, nx, 1.0, 1.0, 1.0, one.ctypes.data,
                one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 1, 0.05, flags,
                one.ctypes.data, t.data_ptr(), 64, None, None)
            assert rc == -2
            rc = lib.nsol_pd_batch_iter_f32(
                t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                t.data_ptr(), members, 1, 1, 1, nx, 1.0, 1.0, 1.0, t.data_ptr(), 0,
                flags, None)
            assert rc == -2
    assert ops.pd_batch_launches() == before
    # the existing stacked entry keeps declining the isotropic bit
    rc = lib.nsol_pd_sweep_run_f32(
        t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
        t.data_ptr(), 2, 1, 1, 1, 16, 1.0, 1.0, 1.0, one.ctypes.data,
        one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 1, 0.05,
        ops.PD_REG_ISOTROPIC, one.ctypes.data, t.data_ptr(), 64, None, None)
    assert rc == -2
    # a batch whose first launch is declined: sequential, nothing written before
    _, make = _stack((37, 53), "TV", "L2", np.float32)
    solvers = make()
    seen = []

    def declined(*args, **kw):
        seen.append([s._x for s in solvers])
        return None
    monkeypatch.setattr(ops, "pd_batch_run", declined)
    batch = PrimalDualBatch(solvers)
    batch.run()
    assert len(seen) == 1 and all(x is None for x in seen[0])
    assert batch.get_execution() == ["sequential"] * 5
    assert batch.get_group_size() is None
    assert ops.pd_batch_launches() == before
    _assert_same_bits(solvers, make())


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
def test_run_denoising_cli_slice_wise(nsol, tmp_path, capsys, iso):
    import re
    from nsol_amd.application import run_denoising
    vol = np.stack([_image((40, 48), seed=k)[1] for k in range(6)])
    ref = np.stack([_image((40, 48), seed=k)[0] for k in range(6)])
    vol[2] = 0.0                        # no positive maximum: copied through
    src, out, rf = (str(tmp_path / f) for f in ("vol.npy", "out.npy", "ref.npy"))
    np.save(src, vol)
    np.save(rf, ref)
    argv = ["--observation", src, "--result", out, "--reconstruction-type",
            "HuberL2", "--iterations", "30", "--alpha", "0.05", "--L2", "12",
            "--alg-type", "ALG3", "--slice-wise", "--reference", rf,
            "--measures", "PSNR", "NCC"] + (["--isotropic"] if iso else [])
    assert run_denoising.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 3
    assert re.match(r"^HuberL2 alpha=0.05 slice-wise: 30 iterations in \S+ "
                    r"\(5 slices stacked, 1 copied through, 0 sequential\)$",
                    lines[0]), lines[0]
    assert lines[1].startswith("  PSNR: ") and lines[2].startswith("  NCC: ")
    got = np.load(out)
    assert got.shape == vol.shape
    assert np.array_equal(got[2], vol[2])
    for k in (0, 1, 3, 4, 5):
        s = run_denoising.build_solver(vol[k], "HuberL2", 0.05, 30, L2=12.0,
                                       dtype=np.float32, alg_type="ALG3",
                                       isotropic=iso)
        s.run()
        want = s.get_x().reshape(40, 48)
        assert got.dtype == want.dtype and np.array_equal(got[k], want), k


def test_run_denoising_cli_slice_wise_keeps_the_nifti_header(nsol, tmp_path, capsys):
    from nsol_amd import data_reader, nifti
    from nsol_amd.application import run_denoising
    vol = np.stack([_image((24, 40), seed=k)[1] for k in range(4)])
    vol[0] = 0.0
    src, out = str(tmp_path / "vol.nii.gz"), str(tmp_path / "out.nii.gz")
    nifti.write(src, vol.astype(np.float32), (1.0, 2.0, 0.5))
    argv = ["--observation", src, "--result", out, "--reconstruction-type", "TVL1",
            "--iterations", "20", "--alpha", "0.5", "--slice-wise", "--isotropic"]
    assert run_denoising.main(argv) == 0
    line = capsys.readouterr().out.splitlines()
    assert len(line) == 1 and line[0].endswith(
        "(3 slices stacked, 1 copied through, 0 sequential)"), line
    reader = data_reader.DataReader(src)
    reader.read_data()
    observed = reader.get_data()
    assert observed.ndim == 3
    got, spacing, _ = nifti.read(out)
    assert tuple(spacing) == tuple(nifti.read(src)[1])
    res = data_reader.DataReader(out)
    res.read_data()
    got = res.get_data()
    assert got.shape == observed.shape
    copied = 0
    for k in range(observed.shape[0]):
        if not np.max(observed[k]) > 0:
            assert np.array_equal(got[k], observed[k])
            copied += 1
            continue
        s = run_denoising.build_solver(observed[k], "TVL1", 0.5, 20, L2=8.0,
                                       dtype=np.float32, isotropic=True)
        s.run()
        want = s.get_x().reshape(observed.shape[1:]).astype(got.dtype)
        assert np.array_equal(got[k], want), k
    assert copied == 1
