"""The member-stacked primal-dual sweep (nsol_amd/parameter_sweep.py,
nsol_pd_sweep_run_*) on a real MI355X: bit-identity to single solver runs, the
oracle, groups, measures, the sequential fallback, the launch count and the
command line."""
import os

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12     # float64 kernels vs float64 reference
F32_TOL = 1e-5      # BASELINE.json north_star: 1e-5 rel on the primal iterate

ALPHAS = [0.003, 0.01, 0.03, 0.1, 0.3]
ALGS = ["ALG2", "ALG2_AHMOD", "ALG3"]
PARAMS = {"alpha": ALPHAS, "alg_type": ALGS}
ITERS = 25
SHAPES = [(1000,), (72, 100), (37, 53), (24, 20, 32), (15, 17, 19)]


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _image(shape, seed=0):
    rng = np.random.default_rng(seed)
    clean = np.full(shape, 20.0)
    clean[tuple(slice(s // 4, 3 * s // 4) for s in shape)] = 100.0
    return clean, clean + 12.0 * rng.standard_normal(shape)


def _wiring(obs, reg, data, foreign=False):
    import nsol_amd.linear_operators as LO
    from nsol_amd.proximal_operators import ProximalOperators as prox
    b = obs.flatten()
    xs = float(np.max(obs))
    lo = getattr(LO, "LinearOperators%dD" % obs.ndim)()
    grad, grad_adj = lo.get_gradient_operators()
    X, Z = obs.shape, grad(obs).shape
    D = lambda x: grad(x.reshape(*X)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    inner = prox.prox_ell1_denoising if data == "L1" else prox.prox_ell2_denoising
    if foreign:
        # a prox the symbolic probe cannot see through: a host round trip
        pf = lambda x, tau: np.asarray(inner(np.asarray(x), tau, x0=b, x_scale=xs))
    else:
        pf = lambda x, tau: inner(x, tau, x0=b, x_scale=xs)
    pg = prox.prox_huber_conj if reg == "Huber" else prox.prox_tv_conj
    return dict(prox_f=pf, prox_g_conj=pg, B=D, B_conj=Da, x0=b, x_scale=xs), D


def _sweep(obs, reg, data, dtype, parameters=PARAMS, iters=ITERS, foreign=False):
    from nsol_amd.parameter_sweep import PrimalDualSweep
    w, D = _wiring(obs, reg, data, foreign)
    return PrimalDualSweep(L2=16.0, parameters=parameters, iterations=iters,
                           dtype=dtype, **w), D


def _single(obs, reg, data, dtype, member, iters=ITERS, foreign=False,
            one_launch=True):
    """The PrimalDualSolver of one member, one launch per iteration."""
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd import _lib
    if one_launch:
        _lib.set_param("pd2_enable", 0)
        _lib.set_param("pdk_enable", 0)
    w, _ = _wiring(obs, reg, data, foreign)
    return pd.PrimalDualSolver(L2=16.0, alpha=member["alpha"],
                               alg_type=member["alg_type"], iterations=iters,
                               dtype=dtype, **w)


@pytest.mark.parametrize("data", ["L2", "L1"])
@pytest.mark.parametrize("reg", ["TV", "Huber"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stacked_members_are_bit_identical_to_single_runs(nsol, shape, dtype, reg,
                                                          data):
    _, obs = _image(shape)
    sweep, _ = _sweep(obs, reg, data, dtype)
    sweep.run()
    assert sweep.get_execution() == "stacked"
    members = sweep.get_parameters()
    assert len(members) == 15
    allx = sweep.get_x_all_device()
    assert tuple(allx.shape) == (15, obs.size)
    for m, member in enumerate(members):
        s = _single(obs, reg, data, dtype, member)
        s.run()
        assert s.get_execution() == "fused"
        one = s.get_x_device()
        assert one.dtype == allx.dtype
        assert bool((allx[m] == one).all()), (m, member)
        assert np.array_equal(sweep.get_x(m), s.get_x())


@pytest.mark.parametrize("data", ["L2", "L1"])
@pytest.mark.parametrize("reg", ["TV", "Huber"])
@pytest.mark.parametrize("dtype,tol", [(np.float32, F32_TOL), (np.float64, F64_TOL)])
def test_stacked_members_match_the_oracle(nsol, dtype, tol, reg, data):
    from oracle import nsol_oracle as orc
    shape = (72, 100)
    _, obs = _image(shape)
    sweep, _ = _sweep(obs, reg, data, dtype)
    sweep.run()
    assert sweep.get_execution() == "stacked"
    errs = []
    for m, member in enumerate(sweep.get_parameters()):
        ref = orc.primal_dual_denoise(obs.flatten(), shape, reg, data,
                                      member["alpha"], ITERS, 16.0,
                                      member["alg_type"])
        assert np.all(np.isfinite(ref)), member
        errs.append(rel_l2(sweep.get_x(m), ref, "%s%s %s" % (reg, data, member)))
    print("oracle rel-L2 per member:", errs)
    assert max(errs) <= tol, errs


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_groups_of_four_equal_the_ungrouped_run(nsol, dtype, monkeypatch):
    from nsol_amd import ops
    _, obs = _image((37, 53))
    whole, _ = _sweep(obs, "TV", "L2", dtype)
    whole.run()
    assert whole.get_execution() == "stacked" and whole.get_group_size() == 15
    # the byte budget of four members' state (x, two xbar, two 2-component p)
    monkeypatch.setattr(ops, "PD_SWEEP_GROUP_BYTES",
                        4 * (3 + 2 * 2) * obs.size * np.dtype(dtype).itemsize)
    before = ops.pd_sweep_launches()
    grouped, _ = _sweep(obs, "TV", "L2", dtype)
    grouped.run()
    assert grouped.get_execution() == "stacked" and grouped.get_group_size() == 4
    assert ops.pd_sweep_launches() - before == 4 * ITERS
    assert bool((grouped.get_x_all_device() == whole.get_x_all_device()).all())


def test_groups_on_whole_vector_rows(nsol, monkeypatch):
    """The same on rows of whole 16-byte vectors (the aligned kernel form)."""
    from nsol_amd import ops
    _, obs = _image((72, 100))
    whole, _ = _sweep(obs, "Huber", "L1", np.float32)
    whole.run()
    monkeypatch.setattr(ops, "PD_SWEEP_GROUP_BYTES", 4 * (3 + 2 * 2) * obs.size * 4)
    grouped, _ = _sweep(obs, "Huber", "L1", np.float32)
    grouped.run()
    assert grouped.get_group_size() == 4
    assert bool((grouped.get_x_all_device() == whole.get_x_all_device()).all())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_measures_equal_the_single_solvers_device_observer(nsol, dtype):
    from nsol_amd.observer import Observer, observation_points
    from nsol_amd.prior_measures import PriorMeasures as PM
    from nsol_amd.similarity_measures import SimilarityMeasures as SM
    shape = (72, 100)
    clean, obs = _image(shape)
    x_ref = clean.flatten()
    sweep, D = _sweep(obs, "TV", "L2", dtype)
    measures = {k: (lambda x, k=k: SM.similarity_measures[k](x, x_ref))
                for k in ("PSNR", "SSD", "NCC")}
    measures["TV"] = lambda x: PM.total_variation(x, D, 2)
    sweep.set_measures(measures, every=5)
    sweep.run()
    assert sweep.get_execution() == "stacked"
    assert sweep.get_observed_iterations() == observation_points(ITERS, 5)
    got = sweep.get_measures()
    for m, member in enumerate(sweep.get_parameters()):
        s = _single(obs, "TV", "L2", dtype, member)
        o = Observer(keep_iterates=False, every=5)
        o.set_measures(measures)
        s.set_observer(o)
        s.run()
        o.compute_measures()
        assert set(o.get_measure_classes().values()) == {"board"}
        for name in measures:
            assert got[name].shape == (15, 6) and got[name].dtype == np.float64
            assert np.array_equal(got[name][m], o.get_measures()[name]), \
                (name, member, got[name][m], o.get_measures()[name])
    k, best = sweep.best("PSNR")
    assert k == int(np.argmax(got["PSNR"][:, -1]))
    assert best == sweep.get_parameters()[k]
    assert sweep.best("SSD", mode="min")[0] == int(np.argmin(got["SSD"][:, -1]))
    # every=None: the final iterate only
    last, _ = _sweep(obs, "TV", "L2", dtype)
    last.set_measures(measures)
    last.run()
    assert last.get_observed_iterations() == [ITERS]
    for name in measures:
        assert np.array_equal(last.get_measures()[name], got[name][:, -1:])


def test_a_measure_that_raises_fails_in_the_measure_step(nsol):
    _, obs = _image((37, 53))
    sweep, _ = _sweep(obs, "TV", "L2", np.float32,
                      parameters={"alpha": [0.01, 0.1]}, iters=6)

    def bad(x):
        raise KeyError("no such thing")
    sweep.set_measures({"bad": bad}, every=3)
    with pytest.raises(KeyError):
        sweep.run()
    # the members themselves ran to the end
    assert sweep.get_execution() == "stacked"
    assert np.all(np.isfinite(sweep.get_x(1)))


def test_foreign_prox_runs_sequentially_with_the_same_bits(nsol):
    _, obs = _image((37, 53))
    params = {"alpha": [0.01, 0.1], "alg_type": ["ALG2", "ALG3"]}
    from nsol_amd import ops
    before = ops.pd_sweep_launches()
    sweep, _ = _sweep(obs, "TV", "L2", np.float32, parameters=params, iters=8,
                      foreign=True)
    sweep.run()
    assert sweep.get_execution() == "sequential"
    assert sweep.get_group_size() is None
    assert ops.pd_sweep_launches() == before
    allx = sweep.get_x_all_device()
    for m, member in enumerate(sweep.get_parameters()):
        s = _single(obs, "TV", "L2", np.float32, member, iters=8, foreign=True,
                    one_launch=False)
        s.run()
        assert s.get_execution() != "fused"
        assert bool((allx[m] == s.get_x_device()).all())


def test_members_over_the_size_limit_run_sequentially(nsol, monkeypatch):
    from nsol_amd import ops
    _, obs = _image((24, 20, 32))
    whole, _ = _sweep(obs, "TV", "L2", np.float32, parameters={"alpha": ALPHAS})
    whole.run()
    assert whole.get_execution() == "stacked"
    monkeypatch.setattr(ops, "PD_SWEEP_MAX_VOXELS", obs.size - 1)
    seq, _ = _sweep(obs, "TV", "L2", np.float32, parameters={"alpha": ALPHAS})
    seq.run()
    assert seq.get_execution() == "sequential"
    assert bool((seq.get_x_all_device() == whole.get_x_all_device()).all())


def test_one_launch_per_iteration_for_all_members(nsol):
    from nsol_amd import ops
    _, obs = _image((72, 100))
    sweep, _ = _sweep(obs, "TV", "L2", np.float32)
    before = ops.pd_sweep_launches()
    sweep.run()
    assert sweep.get_execution() == "stacked"
    assert len(sweep.get_parameters()) == 15
    assert ops.pd_sweep_launches() - before == ITERS       # not 15 * 25


def test_library_declines_with_minus_two(nsol):
    """No members, or members over 2^31 voxels in total: the project's 'declined'
    code, nothing launched, never NSOL_EINVAL."""
    import torch
    from nsol_amd import _lib, ops
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    one = np.ones(1)
    before = ops.pd_sweep_launches()
    for members, nx in ((0, 16), (3, 1 << 30)):
        rc = lib.nsol_pd_sweep_run_f32(
            t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
            t.data_ptr(), members, 1, 1, 1, nx, 1.0, 1.0, 1.0, one.ctypes.data,
            one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 1, 0.05, 0,
            one.ctypes.data, t.data_ptr(), 64, None, None)
        assert rc == -2
    assert ops.pd_sweep_launches() == before


def _run_cli(argv, capsys):
    from nsol_amd.application import run_denoising
    rc = run_denoising.main(argv)
    return rc, capsys.readouterr().out


def test_run_denoising_cli_sweep(nsol, tmp_path, capsys):
    import re
    clean, obs = _image((64, 64), seed=3)
    src, ref = str(tmp_path / "obs.npy"), str(tmp_path / "ref.npy")
    np.save(src, obs)
    np.save(ref, clean)
    alphas = [0.01, 0.03, 0.1]
    rdir = str(tmp_path / "study")
    common = ["--observation", src, "--reconstruction-type", "TVL2",
              "--iterations", "30", "--L2", "8"]
    rc, out = _run_cli(common + ["--alpha"] + [str(a) for a in alphas] +
                       ["--result-dir", rdir, "--reference", ref], capsys)
    assert rc == 0
    lines = out.splitlines()
    heads = [ln for ln in lines if ln.startswith("TVL2 alpha=")]
    assert [float(re.match(r"TVL2 alpha=(\S+):", h).group(1)) for h in heads] == alphas
    assert all(h.endswith("(stacked)") for h in heads)
    assert lines[-1].startswith("best alpha: PSNR ")
    z = np.load(os.path.join(rdir, "sweep.npz"))
    assert list(z["parameter_names"]) == ["alpha"]
    assert np.array_equal(z["parameters"].reshape(-1), alphas)
    assert list(z["observed_iterations"]) == [0, 30]
    assert z["measure_PSNR"].shape == (3, 2)
    one_form = re.compile(
        r"^TVL2 alpha=\S+: 30 iterations in \d+:\d\d:\d\d(\.\d+)? \(fused\)$")
    for a in alphas:
        single = str(tmp_path / ("single_%g.npy" % a))
        rc, out = _run_cli(common + ["--alpha", str(a), "--result", single], capsys)
        assert rc == 0
        ln = out.splitlines()
        assert len(ln) == 1 and one_form.match(ln[0]), ln
        member = np.load(os.path.join(rdir, "obs_alpha%g.npy" % a))
        want = np.load(single)
        assert member.dtype == want.dtype and np.array_equal(member, want)
