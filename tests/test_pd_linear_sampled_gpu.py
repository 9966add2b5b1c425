"""PrimalDualLinearSolver on a SampledConvolutionOperator (super-resolution: b, q and the
weights on the coarse grid, x on the fine one) on the GPU: fused runs against the NumPy
restatement of tests/test_sampled_conv_host.py, `fused` against `device` mode with
callables composed from ConvolutionOperator, slicing and a zero-fill, masking, the
stopping rule, observers, the sequential batch and sweep, and the command line.
25 iterations; float64 at 1e-12, float32 at the project's standing 1e-5."""
import numpy as np
import pytest

from conftest import rel_l2
from test_pd_linear_gpu import _ratios
from test_pd_linear_host import gaussian_kernel
from test_pd_weighted_host import mixed_weights
from test_sampled_conv_host import (numpy_start, pd_linear_sampled_restatement,
                                    sampled_extent, sampled_forward)

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12
F32_TOL = 1e-5
ITERS = 25
BOTH = [np.float64, np.float32]


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _gate(dtype):
    return F64_TOL if np.dtype(dtype) == np.float64 else F32_TOL


def _factors_of(shape):
    """Per-axis ndimage.convolve factors, normalised: the 7-tap Gaussian of sigma 1, or
    (1/4, 1/2, 1/4) where the extent is below 7 -- different tap counts per axis."""
    return [gaussian_kernel(1, 1.) if s >= 7 else np.array([0.25, 0.5, 0.25])
            for s in shape]


def _dense(ks):
    out = ks[0]
    for k in ks[1:]:
        out = np.multiply.outer(out, k)
    return out


_CASES = {}


def _case(shape, factors, offsets):
    """(ks, obs, x0, coarse): a noisy sampled blur of a random fine image and the start
    A^T b / A^T 1; made once per geometry and left unchanged."""
    key = (shape, factors, offsets)
    if key not in _CASES:
        rng = np.random.default_rng(sum(shape) + sum(factors))
        ks = _factors_of(shape)
        truth = 50.0 + 30.0 * rng.standard_normal(shape)
        obs = sampled_forward(truth, ks, "wrap", factors, offsets)
        obs = obs + 2.0 * rng.standard_normal(obs.shape)
        x0 = numpy_start(obs, ks, "wrap", factors, offsets, shape)
        for a in (obs, x0, truth):
            a.setflags(write=False)
        _CASES[key] = (ks, obs, x0, truth)
    return _CASES[key]


def _operators(shape, factors, offsets):
    from nsol_amd.linear_operators import SampledConvolutionOperator
    ks = _factors_of(shape)
    A = SampledConvolutionOperator(len(shape), _dense(ks), factors, offsets)
    return A, A.adjoint(shape)


def _solver(nsol, fine, factors, offsets, dtype, obs=None, x0=None, **kw):
    ks, obs0, x00, _ = _case(fine, factors, offsets)
    obs = obs0 if obs is None else obs
    x0 = x00 if x0 is None else x0
    A, At = _operators(fine, factors, offsets)
    coarse = obs.shape
    args = dict(A=lambda x: A(x.reshape(*fine)).flatten(),
                A_adj=lambda q: At(q.reshape(*coarse)).flatten(), b=obs.flatten(),
                x0=x0.flatten(), dimension=len(fine), alpha=0.05, iterations=ITERS,
                x_scale=float(obs0.max()), dtype=dtype)
    args.update(kw)
    return nsol.PrimalDualLinearSolver(**args)


def _options(reg, iso, data, weighted, box, coarse):
    kw = dict(reg_type=reg, isotropic=iso, data_loss=data)
    ref = dict(reg=reg, iso=iso, data=data)
    if weighted:
        w = mixed_weights(coarse, 3)
        kw["weights"], ref["weights"] = w.flatten(), w
    if box:
        kw["bounds"] = ref["bounds"] = (0., np.inf)
    return kw, ref


# (fine shape, factors, offsets, reg, isotropic, data, weighted, bounds)
RUNS = [
    ((65,), (3,), (1,), "TV", False, "ell2", False, False),
    ((65,), (3,), (0,), "huber", True, "ell1", True, True),
    ((9, 130), (2, 3), (1, 2), "TV", False, "ell2", True, False),
    ((9, 130), (2, 3), (0, 0), "huber", True, "ell1", False, True),
    ((6, 9, 130), (3, 1, 2), (2, 0, 1), "TV", True, "ell1", True, True),
    ((6, 9, 130), (3, 1, 2), (0, 0, 0), "huber", False, "ell2", False, False),
    ((8, 16, 128), (4, 1, 1), (0, 0, 0), "TV", False, "ell2", False, False),
    ((8, 16, 128), (4, 1, 1), (3, 0, 0), "huber", True, "ell1", True, True),
]


def test_every_option_appears_in_2d_and_in_3d():
    for d in (2, 3):
        rows = [r for r in RUNS if len(r[0]) == d]
        for col, values in ((3, ("TV", "huber")), (4, (False, True)),
                            (5, ("ell2", "ell1")), (6, (False, True)),
                            (7, (False, True))):
            assert {r[col] for r in rows} == set(values), (d, col)


_REFS = {}


def _reference(i):
    if i not in _REFS:
        shape, factors, offsets, reg, iso, data, weighted, box = RUNS[i]
        ks, obs, x0, _ = _case(shape, factors, offsets)
        _, ref = _options(reg, iso, data, weighted, box, obs.shape)
        _REFS[i] = pd_linear_sampled_restatement(
            obs, ks, shape, factors, offsets, alpha=0.05, iters=ITERS, x0=x0,
            x_scale=obs.max(), **ref)
        _REFS[i].setflags(write=False)
    return _REFS[i]


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
@pytest.mark.parametrize("i", range(len(RUNS)))
def test_fused_runs_match_the_restatement(nsol, i, dtype):
    shape, factors, offsets, reg, iso, data, weighted, box = RUNS[i]
    coarse = _case(shape, factors, offsets)[1].shape
    kw, _ = _options(reg, iso, data, weighted, box, coarse)
    s = _solver(nsol, shape, factors, offsets, dtype, **kw)
    assert s.get_execution() == "fused" and s.get_shape() == shape
    assert s.get_A_norm2() == float(np.sum(np.abs(_dense(_factors_of(shape))))) ** 2
    s.run()
    assert s.get_execution() == "fused"
    x = s.get_x()
    assert x.shape == (int(np.prod(shape)),)
    err = rel_l2(x, _reference(i), np.dtype(dtype).name)
    print("run %d %s: rel. l2 %.3e" % (i, np.dtype(dtype).name, err))
    assert err <= _gate(dtype), err
    if box:
        assert x.min() >= 0


def _composed(shape, factors, offsets):
    """A and A^T on device tensors from the pieces the package had before the sampled
    operator: ConvolutionOperator plus torch slicing, and a zero-fill plus the adjoint
    blur (the convolution with the reversed kernel; odd taps, periodic)."""
    import torch
    from nsol_amd.device import is_device_tensor
    from nsol_amd.linear_operators import ConvolutionOperator
    kernel = _dense(_factors_of(shape))
    blur = ConvolutionOperator(len(shape), kernel)
    blur_adj = ConvolutionOperator(
        len(shape), kernel[tuple([slice(None, None, -1)] * kernel.ndim)])
    sl = tuple(slice(o, None, f) for o, f in zip(offsets, factors))
    coarse = tuple(sampled_extent(s, f, o) for s, f, o in zip(shape, factors, offsets))

    def A(t):
        if not is_device_tensor(t):
            raise TypeError("device tensors only")
        return blur(t.view(*shape))[sl].contiguous().reshape(-1)

    def At(q):
        if not is_device_tensor(q):
            raise TypeError("device tensors only")
        z = torch.zeros(shape, dtype=q.dtype, device=q.device)
        z[sl] = q.view(*coarse)
        return blur_adj(z).reshape(-1)
    return A, At


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
@pytest.mark.parametrize("i", [2, 4, 7])
def test_fused_agrees_with_device_mode_on_composed_callables(nsol, i, dtype):
    shape, factors, offsets, reg, iso, data, weighted, box = RUNS[i]
    coarse = _case(shape, factors, offsets)[1].shape
    kw, _ = _options(reg, iso, data, weighted, box, coarse)
    fused = _solver(nsol, shape, factors, offsets, dtype, **kw)
    fused.run()
    A, At = _composed(shape, factors, offsets)
    with pytest.raises(ValueError, match="A_norm2"):
        _solver(nsol, shape, factors, offsets, dtype, A=A, A_adj=At, shape=shape, **kw)
    dev = _solver(nsol, shape, factors, offsets, dtype, A=A, A_adj=At, A_norm2=1.,
                  shape=shape, **kw)
    dev.run()
    assert fused.get_execution() == "fused" and dev.get_execution() == "device"
    err = rel_l2(dev.get_x(), fused.get_x(), np.dtype(dtype).name)
    print("device against fused: %.3e" % err)
    assert err <= _gate(dtype), err
    assert rel_l2(dev.get_x(), _reference(i), "device " + np.dtype(dtype).name) <= \
        _gate(dtype)


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
@pytest.mark.parametrize("data", ["ell2", "ell1"])
def test_a_masked_block_never_shows_what_it_holds(nsol, dtype, data):
    shape, factors, offsets = (6, 9, 130), (3, 1, 2), (2, 0, 1)
    ks, obs, _, _ = _case(shape, factors, offsets)
    w = np.ones(obs.shape)
    w[0:2, 3:7, 20:45] = 0
    junk, zero = obs.copy(), obs.copy()
    junk[w == 0] = np.nan
    zero[w == 0] = 0
    x0 = numpy_start(zero, ks, "wrap", factors, offsets, shape)
    out = []
    for b in (junk, zero):
        s = _solver(nsol, shape, factors, offsets, dtype, obs=b, x0=x0,
                    weights=w.flatten(), data_loss=data)
        s.run()
        out.append(s.get_x())
    assert np.all(np.isfinite(out[0]))
    assert np.array_equal(out[0], out[1])
    ref = pd_linear_sampled_restatement(junk, ks, shape, factors, offsets, "TV", data,
                                        0.05, ITERS, x0, weights=w, x_scale=obs.max())
    assert rel_l2(out[0], ref, np.dtype(dtype).name) <= _gate(dtype)


def test_stopping_rule_stops_where_the_restatement_does(nsol):
    shape, factors, offsets = (8, 16, 128), (4, 1, 1), (0, 0, 0)
    ks, obs, x0, _ = _case(shape, factors, offsets)
    iters, every = 60, 5
    w = mixed_weights(obs.shape, 4)
    trace = []
    pd_linear_sampled_restatement(obs, ks, shape, factors, offsets, "huber", "ell2", 0.05,
                                  iters, x0, weights=w, x_scale=obs.max(), trace=trace)
    want = [(k,) + _ratios(trace, k) for k in range(every, iters + 1, every)]
    worst = [max(r[1:]) for r in want]
    # the first check whose change is below every earlier one, past the second
    stop = next(k for k in range(2, len(worst)) if worst[k] < min(worst[:k]))
    tol = float(np.sqrt(worst[stop] * min(worst[:stop])))
    kw = dict(reg_type="huber", weights=w.flatten(), iterations=iters)
    s = _solver(nsol, shape, factors, offsets, np.float64, tolerance=tol,
                check_every=every, **kw)
    s.run()
    assert s.get_iterations_done() == want[stop][0]
    assert s.get_stop_reason() == "tolerance"
    rows = s.get_changes()
    assert list(rows[:, 0]) == [float(r[0]) for r in want[:stop + 1]]
    for got, ref in zip(rows, want):
        assert np.allclose(got[1:], ref[1:], rtol=1e-9, atol=0), (got, ref)
    plain = _solver(nsol, shape, factors, offsets, np.float64,
                    **dict(kw, iterations=int(want[stop][0])))
    plain.run()
    assert np.array_equal(s.get_x(), plain.get_x())


def test_observers_see_the_same_final_iterate(nsol):
    from nsol_amd import observer as Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    shape, factors, offsets = (6, 9, 130), (3, 1, 2), (2, 0, 1)
    truth = _case(shape, factors, offsets)[3].flatten()
    iters, runs = 12, {}
    for name, o in (("none", None), ("host", Observer.Observer()),
                    ("device", Observer.Observer(keep_iterates=False, every=5))):
        s = _solver(nsol, shape, factors, offsets, np.float64, iterations=iters)
        if o is not None:
            o.set_measures({"RMSE": lambda x: sm.similarity_measures["RMSE"](x, truth)})
            s.set_observer(o)
        s.run()
        if o is not None:
            o.compute_measures()
        runs[name] = (s.get_x(), o)
    assert np.array_equal(runs["host"][0], runs["none"][0])
    assert np.array_equal(runs["device"][0], runs["none"][0])
    host, dev = runs["host"][1], runs["device"][1]
    assert host.get_observed_iterations() == list(range(iters + 1))
    points = dev.get_observed_iterations()
    assert points == [0, 5, 10, 12]
    hv, dv = host.get_measures()["RMSE"], dev.get_measures()["RMSE"]
    assert np.allclose(dv, np.asarray(hv)[points], rtol=1e-10, atol=0)
    assert dv[-1] == hv[-1] or abs(dv[-1] - hv[-1]) <= 1e-10 * abs(hv[-1])


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_batch_and_sweep_run_sequentially_with_the_members_own_bits(nsol, dtype):
    from nsol_amd.linear_stack import PrimalDualLinearBatch, PrimalDualLinearSweep
    shape, factors, offsets = (9, 130), (2, 3), (1, 2)
    ks, obs, x0, _ = _case(shape, factors, offsets)
    other = obs[::-1].copy()
    alphas = [0.02, 0.08]
    own = []
    for b, a in ((obs, alphas[0]), (other, alphas[1])):
        s = _solver(nsol, shape, factors, offsets, dtype, obs=b, alpha=a, iterations=10)
        s.run()
        own.append(s.get_x())
    members = [_solver(nsol, shape, factors, offsets, dtype, obs=b, alpha=a,
                       iterations=10) for b, a in ((obs, alphas[0]), (other, alphas[1]))]
    batch = PrimalDualLinearBatch(members)
    batch.run()
    assert batch.get_execution() == ["sequential", "sequential"]
    for s, x in zip(members, own):
        assert s.get_execution() == "fused" and np.array_equal(s.get_x(), x)
    # one observation under two alphas
    ref = []
    for a in alphas:
        s = _solver(nsol, shape, factors, offsets, dtype, alpha=a, iterations=10)
        s.run()
        ref.append(s.get_x())
    t = _solver(nsol, shape, factors, offsets, dtype)
    sweep = PrimalDualLinearSweep(t.get_A(), t.get_A_adj(), obs.flatten(), x0.flatten(), 2,
                                  parameters={"alpha": alphas}, iterations=10,
                                  x_scale=float(obs.max()), dtype=dtype)
    sweep.run()
    assert sweep.get_execution() == "sequential"
    for k, x in enumerate(ref):
        got = sweep.get_x(k)
        assert got.shape == (int(np.prod(shape)),) and np.array_equal(got, x)


def test_cli_upsample_equals_the_solver_built_by_hand(nsol, tmp_path, capsys):
    from nsol_amd import nifti
    from nsol_amd.application import run_deconvolution
    rng = np.random.default_rng(11)
    obs = 40. + 20. * rng.random((12, 20))
    npy, out = str(tmp_path / "obs.npy"), str(tmp_path / "out.npy")
    np.save(npy, obs)
    base = ["--solver", "PDL", "--iterations", "12", "--alpha", "0.03", "--blur", "1.0",
            "--upsample", "2", "2"]
    assert run_deconvolution.main(["--observation", npy, "--result", out] + base) == 0
    capsys.readouterr()
    s = run_deconvolution.build_solver(obs, np.ones(2), 1.0, "TVL2", "PDL", 0.03, 12,
                                       dtype=np.float32, upsample=[2, 2])
    assert s.get_execution() == "fused" and s.get_shape() == (24, 40)
    s.run()
    got = np.load(out)
    assert got.shape == (24, 40)
    assert np.array_equal(got, s.get_x().reshape(24, 40))
    # offsets, and a NIfTI result on the fine grid: spacing[0] belongs to the LAST axis
    nii, out_nii = str(tmp_path / "obs.nii.gz"), str(tmp_path / "out.nii.gz")
    nifti.write(nii, obs, (1.5, 3.0))
    assert run_deconvolution.main(
        ["--observation", nii, "--result", out_nii, "--solver", "PDL", "--iterations",
         "5", "--upsample", "3", "2", "--sample-offset", "2", "1"]) == 0
    arr, spacing, _ = nifti.read(out_nii)
    assert arr.shape == (36, 40)
    assert np.allclose(spacing, (1.5 / 2, 3.0 / 3))
    assert np.all(np.isfinite(arr))
