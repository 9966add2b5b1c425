"""Device-mode observer (keep_iterates=False) on the GPU: the histories equal
the host path's, the final iterate does not change, no iterate reaches the
host."""
import numpy as np
import pytest

from oracle import nsol_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _lo(dim):
    import nsol_amd.linear_operators as LO
    return {1: LO.LinearOperators1D, 2: LO.LinearOperators2D,
            3: LO.LinearOperators3D}[dim]()


def _volume(shape, seed=0):
    rng = np.random.default_rng(seed)
    v = np.zeros(shape)
    sl = tuple(slice(s // 4, 3 * s // 4) for s in shape)
    v[sl] = 100.0
    return v + 10.0 * rng.standard_normal(shape) + 20.0


def _pd(obs, iters, dtype, reg="TV", L2=16.0):
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd.proximal_operators import ProximalOperators as prox
    b = obs.flatten()
    xs = float(np.max(obs))
    grad, grad_adj = _lo(obs.ndim).get_gradient_operators()
    X, Z = obs.shape, grad(obs).shape
    D = lambda x: grad(x.reshape(*X)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    pf = lambda x, tau: prox.prox_ell2_denoising(x, tau, x0=b, x_scale=xs)
    pg = prox.prox_huber_conj if reg == "Huber" else prox.prox_tv_conj
    return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=pg, B=D, B_conj=Da, L2=L2,
                               x0=b, alpha=0.05, iterations=iters, x_scale=xs,
                               dtype=dtype), D


def _measures(x_ref, D, dim, shape, ssim=True, nmi=True):
    from nsol_amd.prior_measures import PriorMeasures as PM
    from nsol_amd.similarity_measures import SimilarityMeasures as SM
    m = {k: (lambda x, k=k: SM.similarity_measures[k](x, x_ref))
         for k in ("SSD", "SAD", "MAE", "MSE", "RMSE", "PSNR", "NCC")}
    if ssim:
        m["SSIM"] = lambda x: SM.structural_similarity(x.reshape(shape),
                                                       x_ref.reshape(shape))
    if nmi:
        m["NMI"] = lambda x: SM.similarity_measures["NMI"](x, x_ref)
    m["TK0"] = lambda x: PM.zeroth_order_tikhonov(x)
    m["TK1"] = lambda x: PM.first_order_tikhonov(x, D)
    m["TV"] = lambda x: PM.total_variation(x, D, dim)
    m["Huber"] = lambda x: PM.huber(x, D, dim, gamma=0.5)
    return m


def _observed(solver, measures, keep, every=1):
    from nsol_amd.observer import Observer
    o = Observer(keep_iterates=keep, every=every)
    o.set_measures(measures)
    solver.set_observer(o)
    solver.run()
    o.compute_measures()
    return o, {k: np.asarray(v) for k, v in o.get_measures().items()}


def _match(dev, host, tol=1e-10):
    for k, v in host.items():
        if k == "NMI":
            assert np.array_equal(dev[k], v), k
        elif k == "SSIM":
            np.testing.assert_allclose(dev[k], v, rtol=1e-12, atol=0, err_msg=k)
        else:
            np.testing.assert_allclose(dev[k], v, rtol=tol, atol=0, err_msg=k)


@pytest.mark.parametrize("shape", [(16, 20, 24), (128, 128, 128)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_histories_match_the_host_path(nsol, shape, dtype):
    obs = _volume(shape)
    ref = (obs - 20.0).astype(np.float32 if dtype == np.float32 else np.float64)
    iters = 6
    s_host, D = _pd(obs, iters, dtype)
    s_dev, _ = _pd(obs, iters, dtype)
    m = _measures(ref.flatten(), D, 3, shape)
    o_host, host = _observed(s_host, m, keep=True)
    o_dev, dev = _observed(s_dev, m, keep=False)
    assert s_dev.get_execution() == "fused"
    assert o_dev.get_x_list() == []
    assert o_dev.get_observed_iterations() == list(range(iters + 1))
    cls = o_dev.get_measure_classes()
    assert cls["SSIM"] == "ssim" and cls["NMI"] == "histogram"
    assert all(cls[k] == "board" for k in m if k not in ("SSIM", "NMI"))
    assert all(len(v) == iters + 1 for v in dev.values())
    _match(dev, host)
    assert np.array_equal(s_dev.get_x(), s_host.get_x())


def test_histories_match_the_oracle(nsol):
    shape = (12, 14, 16)
    obs = _volume(shape, 1)
    ref = obs - 20.0
    iters = 5
    s, D = _pd(obs, iters, np.float64)
    _, dev = _observed(s, _measures(ref.flatten(), D, 3, shape, ssim=False,
                                    nmi=False), keep=False)
    b = obs.flatten()
    xs = float(obs.max())
    Do, Dao = orc.flat_operators(shape)
    from oracle.nsol_oracle import prox_ell2_denoising, prox_tv_conj
    pf = lambda x, tau: prox_ell2_denoising(x, tau, x0=b, x_scale=xs)
    its = [b.copy()] + [orc.primal_dual(pf, prox_tv_conj, Do, Dao, 16.0, b,
                                        alpha=0.05, iterations=k, x_scale=xs)
                        for k in range(1, iters + 1)]
    r = ref.flatten()
    want = {"SSD": orc.sim_ssd, "SAD": orc.sim_sad, "MAE": orc.sim_mae,
            "MSE": orc.sim_mse, "RMSE": orc.sim_rmse, "PSNR": orc.sim_psnr,
            "NCC": orc.sim_ncc}
    for k, f in want.items():
        np.testing.assert_allclose(dev[k], [f(x, r) for x in its], rtol=1e-10,
                                   err_msg=k)
    np.testing.assert_allclose(dev["TK0"], [orc.prior_tk0(x) for x in its],
                               rtol=1e-10)
    np.testing.assert_allclose(dev["TK1"], [orc.prior_tk1(x, Do) for x in its],
                               rtol=1e-10)
    np.testing.assert_allclose(dev["TV"], [orc.prior_tv(x, Do, 3) for x in its],
                               rtol=1e-10)
    np.testing.assert_allclose(dev["Huber"],
                               [orc.prior_huber(x, Do, 3, 0.5) for x in its],
                               rtol=1e-10)


def _final_x_unchanged(make, measures_of, every):
    s0 = make()
    s0.run()
    s1 = make()
    from nsol_amd.observer import Observer
    o = Observer(keep_iterates=False, every=every)
    o.set_measures(measures_of(s1))
    s1.set_observer(o)
    s1.run()
    assert np.array_equal(s0.get_x(), s1.get_x())
    return s0, s1, o


@pytest.mark.parametrize("every", [1, 3, 5])
def test_final_x_bit_identical_fused(nsol, every):
    obs = _volume((128, 128, 128), 2)
    ref = obs.flatten() - 20.0
    holder = {}

    def make():
        s, holder["D"] = _pd(obs, 12, np.float32)
        return s
    _, s1, o = _final_x_unchanged(
        make, lambda s: _measures(ref, holder["D"], 3, obs.shape, False, False),
        every)
    assert o.get_observed_iterations()[-1] == 12
    assert all(len(v) == len(o.get_observed_iterations())
               for v in o.get_measures().values())


def test_final_x_bit_identical_pitched(nsol):
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd import ops
    shape = (64, 127, 131)                   # ragged rows, >= PITCH_MIN_VOXELS
    assert int(np.prod(shape)) >= pd.PITCH_MIN_VOXELS
    obs = _volume(shape, 3)
    ref = obs.flatten() - 20.0
    holder = {}

    def make():
        s, holder["D"] = _pd(obs, 7, np.float32)
        return s
    assert ops.row_pitch(shape, __import__("torch").empty(1)) > 0
    s0, s1, o = _final_x_unchanged(
        make, lambda s: _measures(ref, holder["D"], 3, shape, True, False), 3)
    # and the history matches the host path on the same iterates
    s2, D = _pd(obs, 7, np.float32)
    from nsol_amd.observer import Observer
    oh = Observer(every=1)
    m = _measures(ref, D, 3, shape, True, False)
    oh.set_measures(m)
    s2.set_observer(oh)
    s2.run()
    oh.compute_measures()
    pts = o.get_observed_iterations()
    host = {k: np.asarray(v)[pts] for k, v in oh.get_measures().items()}
    _match({k: np.asarray(v) for k, v in o.get_measures().items()}, host)


def test_final_x_bit_identical_persist_configs(nsol):
    from nsol_amd import ops
    obs = _volume((64, 64, 64), 4)
    ref = obs.flatten() - 20.0
    holder = {}

    def make():
        s, holder["D"] = _pd(obs, 200, np.float32)
        return s
    before = ops.pd_persist_launches()
    _, _, o = _final_x_unchanged(
        make, lambda s: _measures(ref, holder["D"], 3, obs.shape, False, False), 20)
    assert ops.pd_persist_launches() - before >= 11      # whole run + 10 chunks
    assert o.get_observed_iterations() == list(range(0, 201, 20))


def _admm(shape, dtype):
    import nsol_amd.admm_linear_solver as admm
    lo = _lo(3)
    A, Aa = lo.get_gaussian_blurring_operators(np.diag([0.8, 0.8, 0.8]))
    grad, grad_adj = lo.get_gradient_operators()
    Z = grad(np.zeros(shape)).shape
    y = _volume(shape, 5).flatten()
    A_ = lambda x: A(x.reshape(*shape)).flatten()
    Aa_ = lambda x: Aa(x.reshape(*shape)).flatten()
    D = lambda x: grad(x.reshape(*shape)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    s = admm.ADMMLinearSolver(A=A_, A_adj=Aa_, b=y, B=D, B_adj=Da, x0=y,
                              dimension=3, alpha=0.05, rho=0.5, iterations=5,
                              iter_max=8, x_scale=float(y.max()), dtype=dtype)
    return s, D, y


def test_admm_final_x_and_inner_log_unchanged(nsol):
    shape = (40, 40, 40)
    holder = {}

    def make():
        s, holder["D"], holder["y"] = _admm(shape, np.float32)
        return s
    s0, s1, o = _final_x_unchanged(
        make, lambda s: _measures(holder["y"] - 20.0, holder["D"], 3, shape,
                                  False, False), 1)
    assert s1.get_inner_log() == s0.get_inner_log()
    assert o.get_observed_iterations() == list(range(6))
    # the host path on the same iterates
    s2, D, y = _admm(shape, np.float32)
    _, host = _observed(s2, _measures(y - 20.0, D, 3, shape, False, False), True)
    _match({k: np.asarray(v) for k, v in o.get_measures().items()}, host)


def test_pd_deconvolution_native_dual_unchanged(nsol):
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd.proximal_operators import ProximalOperators as prox
    shape = (40, 48)
    lo = _lo(2)
    A, Aa = lo.get_gaussian_blurring_operators(np.diag([1.0, 1.0]))
    grad, grad_adj = lo.get_gradient_operators()
    Z = grad(np.zeros(shape)).shape
    y = _volume(shape, 6).flatten()
    A_ = lambda x: A(x.reshape(*shape)).flatten()
    Aa_ = lambda x: Aa(x.reshape(*shape)).flatten()
    D = lambda x: grad(x.reshape(*shape)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    xs = float(y.max())

    def make():
        pf = lambda x, tau: prox.prox_linear_least_squares(
            x=x, tau=tau, A=A_, A_adj=Aa_, b=y, x0=y, iter_max=6, x_scale=xs)
        return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=prox.prox_tv_conj, B=D,
                                   B_conj=Da, L2=8, alpha=0.05, x0=y,
                                   iterations=6, x_scale=xs, dtype=np.float64)
    m = lambda s: _measures(y - 20.0, D, 2, shape, True, True)
    s0, s1, o = _final_x_unchanged(make, m, 2)
    assert s1.get_execution() == "device"
    assert o.get_observed_iterations() == [0, 2, 4, 6]
    s2 = make()
    _, host = _observed(s2, m(s2), True)
    pts = o.get_observed_iterations()
    _match({k: np.asarray(v) for k, v in o.get_measures().items()},
           {k: v[pts] for k, v in host.items()})


def test_no_iterate_reaches_the_host(nsol, monkeypatch):
    import torch
    import nsol_amd.device as device
    shape = (32, 32, 32)
    n = int(np.prod(shape))
    obs = _volume(shape, 7)
    s, D = _pd(obs, 9, np.float32)
    from nsol_amd.observer import Observer
    o = Observer(keep_iterates=False, every=2)
    o.set_measures(_measures(obs.flatten() - 20.0, D, 3, shape, True, False))
    s.set_observer(o)
    seen = []
    real_dl, real_cpu, real_item = device._download, torch.Tensor.cpu, \
        torch.Tensor.item

    def dl(t, *a, **k):
        seen.append(("download", t.numel()))
        return real_dl(t, *a, **k)

    def cpu(t, *a, **k):
        seen.append(("cpu", t.numel(), t.data_ptr()))
        return real_cpu(t, *a, **k)

    def item(t, *a, **k):
        seen.append(("item", t.numel()))
        return real_item(t, *a, **k)
    monkeypatch.setattr(device, "_download", dl)
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    monkeypatch.setattr(torch.Tensor, "item", item)
    s.run()
    board = o._session.board
    monkeypatch.undo()
    assert all(e[1] < n for e in seen), seen
    assert sum(1 for e in seen if e[0] == "cpu" and e[2] == board.data_ptr()) == 1
    o.compute_measures()
    assert len(o.get_measures()["SSD"]) == 6              # 0 2 4 6 8 9


def test_fallbacks_repeatability_and_reuse(nsol):
    from nsol_amd.observer import Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as SM
    shape = (16, 20, 24)
    obs = _volume(shape, 8)
    ref = obs.flatten() - 20.0
    s, D = _pd(obs, 7, np.float32)
    m = _measures(ref, D, 3, shape, True, True)
    m["foreign"] = lambda x: orc.sim_ssd(x, ref)
    m["numpy"] = lambda x: SM.SSD(np.asarray(x) * 1.0, ref)
    o = Observer(keep_iterates=False, every=3)
    o.set_measures(m)
    s.set_observer(o)
    s.run()
    cls = o.get_measure_classes()
    assert cls["foreign"] == "host" and cls["numpy"] == "host"
    first = {k: np.array(v) for k, v in o.get_measures().items()}
    pts = o.get_observed_iterations()
    assert pts == [0, 3, 6, 7]
    np.testing.assert_allclose(first["foreign"], first["SSD"], rtol=1e-10)
    # the same observer for a second run of another length: reset
    s2, _ = _pd(obs, 4, np.float32)
    s2.set_observer(o)
    s2.run()
    assert o.get_observed_iterations() == [0, 3, 4]
    assert all(len(v) == 3 for v in o.get_measures().values())
    # a third, identical to the first: bit-identical histories
    s3, _ = _pd(obs, 7, np.float32)
    s3.set_observer(o)
    s3.run()
    for k, v in o.get_measures().items():
        assert np.array_equal(np.asarray(v), first[k], equal_nan=True), k
    # and the host path over the same callables
    s4, _ = _pd(obs, 7, np.float32)
    _, host = _observed(s4, m, True)
    _match(first, {k: v[pts] for k, v in host.items()})


def test_verbose_fused_run_observes_on_the_device(nsol, capsys):
    """verbose steps the fused run one launch per iteration: a device-mode
    observer still sees every point on the device, no host copies."""
    shape = (16, 20, 24)
    obs = _volume(shape, 9)
    ref = obs.flatten() - 20.0
    s_host, D = _pd(obs, 7, np.float32)
    s_dev, _ = _pd(obs, 7, np.float32)
    s_dev.set_verbose(1)
    m = _measures(ref, D, 3, shape, True, True)
    _, host = _observed(s_host, m, keep=True)
    o, dev = _observed(s_dev, m, keep=False, every=2)
    assert "Primal-Dual iteration 7/7" in capsys.readouterr().out
    assert o.get_x_list() == []
    pts = o.get_observed_iterations()
    assert pts == [0, 2, 4, 6, 7]
    assert all(not np.isnan(v).any() for v in dev.values())
    _match(dev, {k: v[pts] for k, v in host.items()})
    assert np.array_equal(s_dev.get_x(), s_host.get_x())


def test_anisotropic_spacing_matches_the_host_path(nsol):
    """w[0] / w[1] / w[2] belong to the x / y / z axes, as in nsol_grad_*."""
    import nsol_amd.linear_operators as LO
    from nsol_amd.prior_measures import PriorMeasures as PM
    shape = (12, 14, 16)
    obs = _volume(shape, 10)
    grad, _ = LO.LinearOperators3D(spacing=np.array([1.0, 2.0, 4.0])) \
        .get_gradient_operators()
    Da = lambda x: grad(x.reshape(*shape)).flatten()
    m = {"TV": lambda x: PM.total_variation(x, Da, 3),
         "TK1": lambda x: PM.first_order_tikhonov(x, Da),
         "Huber": lambda x: PM.huber(x, Da, 3, gamma=0.3)}
    for dtype in (np.float32, np.float64):
        s_host, _ = _pd(obs, 4, dtype)
        s_dev, _ = _pd(obs, 4, dtype)
        _, host = _observed(s_host, m, keep=True)
        o, dev = _observed(s_dev, m, keep=False)
        assert set(o.get_measure_classes().values()) == {"board"}
        _match(dev, host)
        # and the spacing matters: isotropic differences give other values
        assert not np.allclose(dev["TV"], _observed(
            _pd(obs, 4, dtype)[0],
            {"TV": lambda x: PM.total_variation(
                x, lambda v: _lo(3).get_gradient_operators()[0](
                    v.reshape(*shape)).flatten(), 3)}, keep=False)[1]["TV"])


def test_failing_measure_does_not_abort_the_run(nsol):
    """Dice of a float iterate raises, as it does on the host path: the run
    completes, the other measures are there, compute_measures() raises."""
    from nsol_amd.observer import Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as SM
    shape = (16, 20, 24)
    obs = _volume(shape, 11)
    mask = (obs > 60.0).flatten()
    s0, _ = _pd(obs, 5, np.float32)
    s0.run()
    s, _ = _pd(obs, 5, np.float32)
    o = Observer(keep_iterates=False, every=2)
    o.set_measures({"Dice": lambda x: SM.dice_score(x, mask),
                    "SSD": lambda x: SM.SSD(x, obs.flatten())})
    s.set_observer(o)
    s.run()
    assert np.array_equal(s.get_x(), s0.get_x())
    assert len(o.get_measures()["SSD"]) == 4
    with pytest.raises(ValueError):
        o.compute_measures()
    # the host path raises the same error where it evaluates the measure
    sh, _ = _pd(obs, 5, np.float32)
    oh = Observer()
    oh.set_measures({"Dice": lambda x: SM.dice_score(x, mask)})
    sh.set_observer(oh)
    sh.run()
    with pytest.raises(ValueError):
        oh.compute_measures()
