"""The stopping rule of the primal-dual solver on the GPU: the checking kernels
k_pd_check / k_pd_check_iso and nsol_pd_change_* through ops, the solver against the
float64 restatement of test_pd_stop_host.py, the identity of the execution forms,
sweeps and stacks, and the command line."""
import itertools

import numpy as np
import pytest

from conftest import rel_l2
from test_pd_stop_host import (CASES, K, NEVER, case_weights, observation, reference)

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-12     # identical non-negative float64 summands, another order
RATIO_TOL = 1e-9    # the sums behind a division and a root, on iterates gated at 1e-12
F64_TOL = 1e-12
F32_TOL = 1e-5


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _solver(shape, reg, data, alg, alpha, L2, iso, weighted, iters, dtype, **kw):
    """Wiring of run_denoising.py:95-154 on the case's observation."""
    import nsol_amd.linear_operators as LO
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd.proximal_operators import ProximalOperators as prox
    obs = observation(shape)
    b = obs.flatten()
    xs = float(np.max(b))
    dim = len(shape)
    lo = {1: LO.LinearOperators1D, 2: LO.LinearOperators2D,
          3: LO.LinearOperators3D}[dim]()
    grad, grad_adj = lo.get_gradient_operators()
    Z = grad(b.reshape(shape)).shape
    D = lambda x: grad(x.reshape(*shape)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    if not weighted:
        f = prox.prox_ell1_denoising if data == "L1" else prox.prox_ell2_denoising
        pf = lambda x, tau: f(x, tau, x0=b, x_scale=xs)
    else:
        w = case_weights(shape, True).flatten()
        f = prox.prox_ell1_denoising_weighted if data == "L1" else \
            prox.prox_ell2_denoising_weighted
        pf = lambda x, tau: f(x, tau, x0=b, weights=w, x_scale=xs)
    if not iso:
        pg = prox.prox_huber_conj if reg == "Huber" else prox.prox_tv_conj
    elif reg == "Huber":
        pg = lambda x, s: prox.prox_huber_conj_isotropic(x, s, dim)
    else:
        pg = lambda x, s: prox.prox_tv_conj_isotropic(x, s, dim)
    return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=pg, B=D, B_conj=Da, L2=L2, x0=b,
                               alpha=alpha, iterations=iters, x_scale=xs, alg_type=alg,
                               dtype=dtype, **kw)


def _case_solver(case, dtype, **kw):
    shape, reg, data, alg, alpha, L2, iso, weighted, tol, allowed = case[:10]
    kw.setdefault("tolerance", tol)
    kw.setdefault("check_every", K)
    kw.setdefault("iterations", allowed)
    iters = kw.pop("iterations")
    return _solver(shape, reg, data, alg, alpha, L2, iso, weighted, iters, dtype, **kw)


def _case_id(c):
    return "%s-%s%s-%s%s%s" % ("x".join(map(str, c[0])), c[1], c[2], c[3],
                               "-iso" if c[6] else "", "-w" if c[7] else "")


# ----------------------------------------------------- 1. kernel level, via ops
SHAPES = [(1,), (5,), (70,), (1031,),
          (7, 13), (5, 37), (24, 40), (33, 260),
          (2, 3, 5), (5, 6, 8), (9, 12, 21), (4, 20, 264)]


def _np_sums(x_old, x_new, p_old, p_new):
    f = lambda a: a.cpu().numpy().astype(np.float64)
    xo, xn, pn = f(x_old), f(x_new), f(p_new)
    po = np.zeros_like(pn) if p_old is None else f(p_old)
    return np.array([np.sum((xn - xo) ** 2), np.sum(xn ** 2),
                     np.sum((pn - po) ** 2), np.sum(pn ** 2)])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checking_kernel_writes_the_iteration_and_its_sums(nsol, shape, dtype):
    """Random x, xbar, bt, p (and weights); has_p x {TV, Huber} x {l2, l1} x
    {anisotropic, isotropic} x {unweighted, weighted}, and both rows-per-lane forms
    where the shape has rows: the arrays are the non-checking entry's bit for bit, the
    sums are NumPy's and nsol_pd_change's to 1e-12, two launches give the same bits."""
    import torch
    from nsol_amd import _lib, ops
    from nsol_amd.device import to_device
    rng = np.random.default_rng(sum(shape) + 7)
    n, dim = int(np.prod(shape)), len(shape)
    dev = lambda a: to_device(np.ascontiguousarray(a), dtype)
    x0, xbar0, bt = (dev(rng.standard_normal(n)) for _ in range(3))
    p0 = dev(rng.uniform(-1, 1, dim * n))
    wt = rng.uniform(0, 3, n)
    wt[rng.random(n) < 0.3] = 0.0
    wt = dev(wt)
    w = (1.0, 1.0, 1.0)
    sigma, tau, lmbda, theta, gamma = 0.31, 0.27, 20.0, 0.93, 0.05
    ws = ops.pd_check_workspace(x0, shape)
    rows = torch.zeros((3, 4), dtype=torch.float64, device=x0.device)
    worst = 0.0
    for ry in ((0,) if dim == 1 else (0, 2)):
        _lib.set_param("pd_ry", ry)
        for has_p, huber, l1, iso, wgt in itertools.product((False, True), repeat=5):
            flags = (ops.PD_REG_HUBER if huber else ops.PD_REG_TV) | \
                (ops.PD_DATA_L1 if l1 else ops.PD_DATA_L2) | \
                (ops.PD_REG_ISOTROPIC if iso else 0) | \
                (ops.PD_DATA_WEIGHTED if wgt else 0)
            hden = 1. + sigma * gamma if huber else 1.
            label = (ry, has_p, huber, l1, iso, wgt)
            # the non-checking one-iteration entry
            xr, xbr, pr = x0.clone(), torch.empty_like(x0), torch.empty_like(p0)
            if wgt:
                tab = ops.pd_weighted_table(x0, 1, [lmbda], [sigma], [tau], [theta],
                                            not has_p, gamma, flags)
                assert ops.pd_weighted_iter(xbar0, xbr, xr, bt, wt, p0, pr, 1, shape, w,
                                            tab, 0, flags)
            else:
                ops.pd_fused_iter(xbar0, xbr, xr, bt, p0 if has_p else None, pr, shape,
                                  w, sigma, hden, tau, tau * lmbda, theta, flags)
            got = []
            for j in range(2):
                xc, xbc, pc = x0.clone(), torch.empty_like(x0), torch.empty_like(p0)
                assert ops.pd_check_iter(xbar0, xbc, xc, bt, wt if wgt else None,
                                         p0 if has_p else None, pc, shape, w, sigma,
                                         hden, tau, tau * lmbda, theta, flags, ws,
                                         rows[j])
                got.append((xc, xbc, pc))
            ops.pd_change(x0, got[0][0], p0 if has_p else None, got[0][2], ws, rows[2])
            r = rows.cpu().numpy()
            for a, b in zip(got[0], (xr, xbr, pr)):
                assert torch.equal(a, b), label
            for a, b in zip(got[0], got[1]):
                assert torch.equal(a, b), label
            assert np.array_equal(r[0], r[1]), label          # the same bits twice
            want = _np_sums(x0, got[0][0], p0 if has_p else None, got[0][2])
            assert np.all(np.isfinite(r)) and np.all(want > 0), label
            err = max(np.max(np.abs(r[0] - want) / want),
                      np.max(np.abs(r[2] - want) / want),
                      np.max(np.abs(r[0] - r[2]) / want))
            worst = max(worst, err)
            assert err <= SUM_TOL, (label, err, r, want)
    print(shape, np.dtype(dtype).name, "worst relative error of a sum %.3g" % worst)


def test_checking_entries_refuse_what_they_cannot_index(nsol):
    import torch
    from nsol_amd import ops
    x = torch.zeros(30, dtype=torch.float64, device="cuda")
    p = torch.zeros(60, dtype=torch.float64, device="cuda")
    ws = ops.pd_check_workspace(x, (5, 6))
    row = torch.zeros(4, dtype=torch.float64, device="cuda")
    args = lambda **kw: dict(dict(xbar_in=x.clone(), xbar_out=x.clone(), x=x.clone(),
                                  bt=x, wt=None, p_in=None, p_out=p, shape=(5, 6),
                                  w=(1., 1., 1.), sigma=.3, hden=1., tau=.3, tl=1.,
                                  theta=1., flags=0, ws=ws, row=row), **kw)
    assert ops.pd_check_iter(**args())
    with pytest.raises(ValueError):
        ops.pd_check_iter(**args(p_out=p[:59]))
    with pytest.raises(ValueError):
        ops.pd_check_iter(**args(wt=x))                       # weights without the flag
    with pytest.raises(ValueError):
        ops.pd_check_iter(**args(flags=ops.PD_DATA_WEIGHTED))  # the flag without them
    with pytest.raises(ValueError):
        ops.pd_check_iter(**args(row=row[:3]))
    with pytest.raises(ValueError):
        ops.pd_check_iter(**args(ws=ws.float()))
    with pytest.raises(ValueError):
        ops.pd_check_iter(**args(shape=(5, 7)))
    a = args()
    with pytest.raises(ValueError):
        ops.pd_check_iter(**dict(a, xbar_out=a["xbar_in"]))    # NSOL_EINVAL
    with pytest.raises(ValueError):
        ops.pd_change(x, x, None, p, ws[:3], row)
    with pytest.raises(ValueError):
        ops.pd_change(x, x[:29], None, p, ws, row)
    # a workspace smaller than the grid: the pass fits its grid to it
    ops.pd_change(x, x + 1, None, p + 2, ws[:4], row)
    assert row.cpu().tolist() == [30.0, 30.0, 240.0, 240.0]
    with pytest.raises(ValueError):
        ops.pd_check_workspace(x, (5, 6, 7, 8))


# ------------------------------------------------ 2. solver vs the restatement
def _assert_matches(s, ref, dtype):
    rows = s.get_changes()
    print("done", s.get_iterations_done(), s.get_stop_reason())
    for got, want in zip(rows, ref["changes"]):
        print("  k=%d r_x %.6e (%.6e) r_p %.6e (%.6e)" % (got[0], got[1], want[1],
                                                          got[2], want[2]))
    assert s.get_iterations_done() == ref["done"]
    assert s.get_stop_reason() == ref["reason"]
    assert rows.shape == ref["changes"].shape
    assert np.array_equal(rows[:, 0], ref["changes"][:, 0])
    err = rel_l2(s.get_x(), ref["x"], np.dtype(dtype).name)
    print("  x", err)
    if np.dtype(dtype) == np.float64:
        assert np.allclose(rows[:, 1:], ref["changes"][:, 1:], rtol=RATIO_TOL, atol=0)
        assert err <= F64_TOL, err
    else:
        assert err <= F32_TOL, err


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_float64_run_stops_where_the_restatement_stops(nsol, case):
    from nsol_amd import ops
    before = ops.pd_check_launches()
    s = _case_solver(case, np.float64)
    s.run()
    assert s.get_execution() == "fused"
    ref = reference(case)
    _assert_matches(s, ref, np.float64)
    assert ops.pd_check_launches() == before + len(ref["changes"])


@pytest.mark.parametrize("case", [c for c in CASES if c[8] >= 1e-3], ids=_case_id)
def test_float32_run_stops_at_the_same_iteration(nsol, case):
    s = _case_solver(case, np.float32)
    s.run()
    assert s.get_execution() == "fused"
    _assert_matches(s, reference(case), np.float32)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_run_whose_change_stays_large_runs_out(nsol, dtype):
    s = _case_solver(NEVER, dtype)
    s.run()
    ref = reference(NEVER)
    _assert_matches(s, ref, dtype)
    assert s.get_iterations_done() == 60 and s.get_stop_reason() == "iterations"
    assert s.get_changes()[-1, 0] == 60


# ------------------------------------------------------- 3. identity of forms
FORM_CASES = [CASES[0], CASES[3], CASES[7], CASES[11]]      # tolerances >= 1e-3


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", FORM_CASES, ids=_case_id)
def test_stopped_run_is_the_plain_run_of_that_length(nsol, case, dtype):
    s = _case_solver(case, dtype)
    s.run()
    k = s.get_iterations_done()
    assert s.get_stop_reason() == "tolerance" and k == case[10]
    plain = _case_solver(case, dtype, tolerance=None, iterations=k)
    plain.run()
    assert plain.get_iterations_done() == k and plain.get_stop_reason() == "iterations"
    assert plain.get_changes().shape == (0, 3)
    assert np.array_equal(s.get_x(), plain.get_x())


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", FORM_CASES, ids=_case_id)
def test_tolerance_never_met_changes_no_bit(nsol, case, dtype):
    s = _case_solver(case, dtype, tolerance=1e-300, iterations=23)
    s.run()
    assert s.get_iterations_done() == 23 and s.get_stop_reason() == "iterations"
    assert list(s.get_changes()[:, 0]) == [5, 10, 15, 20, 23]
    plain = _case_solver(case, dtype, tolerance=None, iterations=23)
    plain.run()
    assert np.array_equal(s.get_x(), plain.get_x())


def test_persistent_stretches_between_checks_change_no_bit(nsol):
    """K = 20: the 19 iterations between two checks go through the persistent kernel,
    settled before the checking kernel reads x."""
    from nsol_amd import ops
    shape = (8, 12, 24)                               # rows of whole vectors
    kw = dict(reg="TV", data="L2", alg="ALG2", alpha=0.05, L2=16, iso=False,
              weighted=False)
    before = ops.pd_persist_launches()
    s = _solver(shape, iters=45, dtype=np.float32, tolerance=1e-300, check_every=20, **kw)
    s.run()
    assert ops.pd_persist_launches() > before
    assert list(s.get_changes()[:, 0]) == [20, 40, 45]
    old = ops.PD_PERSIST
    ops.PD_PERSIST = False
    try:
        plain = _solver(shape, iters=45, dtype=np.float32, **kw)
        plain.run()
    finally:
        ops.PD_PERSIST = old
    assert np.array_equal(s.get_x(), plain.get_x())


@pytest.mark.parametrize("case", [CASES[0], CASES[6], CASES[10]], ids=_case_id)
def test_fused_semi_fused_and_generic_forms_stop_together(nsol, case):
    import nsol_amd.primal_dual_solver as pd
    ref = reference(case)
    s = _case_solver(case, np.float64)
    s.run()
    assert s.get_execution() == "fused"
    old = pd.USE_SEMI_FUSED
    try:
        for semi in (False, True):
            pd.USE_SEMI_FUSED = semi
            g = _case_solver(case, np.float64)
            g.plan = lambda: None
            g.run()
            assert g.get_execution() == "device"
            assert g.get_iterations_done() == s.get_iterations_done() == ref["done"]
            assert g.get_stop_reason() == "tolerance"
            assert np.array_equal(g.get_x(), s.get_x()), semi
            assert np.allclose(g.get_changes(), s.get_changes(), rtol=RATIO_TOL, atol=0)
    finally:
        pd.USE_SEMI_FUSED = old


@pytest.mark.parametrize("case", [CASES[0], CASES[7]], ids=_case_id)
def test_device_observer_sees_the_same_values_up_to_the_stop(nsol, case):
    from nsol_amd.observer import Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    ref = observation(case[0]).flatten()

    def run(tolerance, keep):
        obs = Observer(keep_iterates=keep, every=1 if keep else 4)
        obs.set_measures({"RMSE": lambda x: sm.similarity_measures["RMSE"](x, ref)})
        s = _case_solver(case, np.float64, tolerance=tolerance, iterations=60)
        s.set_observer(obs)
        s.run()
        obs.compute_measures()
        return s, obs

    s, obs = run(case[8], False)
    plain, pobs = run(None, False)
    stop = case[10]
    assert s.get_iterations_done() == stop and plain.get_iterations_done() == 60
    pts = obs.get_observed_iterations()
    assert pts == pobs.get_observed_iterations() == list(range(0, 61, 4))
    got, want = obs.get_measures()["RMSE"], pobs.get_measures()["RMSE"]
    upto = [j for j, p in enumerate(pts) if p <= stop]
    assert len(upto) >= 2
    assert np.array_equal(got[upto], want[upto])
    assert np.all(np.isnan(got[len(upto):]))
    # an observer that keeps iterates: one host copy per iteration done
    h, hobs = run(case[8], True)
    assert h.get_iterations_done() == stop
    assert len(hobs.get_x_list()) == stop + 1
    assert np.array_equal(h.get_x(), s.get_x())
    assert np.allclose(h.get_changes(), s.get_changes(), rtol=RATIO_TOL, atol=0)


# ------------------------------------------------------------ 4. surroundings
def test_no_tolerance_leaves_the_run_as_it_was(nsol):
    from nsol_amd import ops
    case = CASES[3]
    before = ops.pd_check_launches()
    s = _case_solver(case, np.float32, tolerance=None, iterations=25)
    s.run()
    assert ops.pd_check_launches() == before
    assert s.get_execution() == "fused"
    assert s.get_iterations_done() == 25 and s.get_stop_reason() == "iterations"
    assert s.get_changes().shape == (0, 3)
    w = _case_solver(CASES[10], np.float32, tolerance=None, iterations=25)
    lw = ops.pd_weighted_launches()
    w.run()
    assert ops.pd_weighted_launches() == lw + 25 and ops.pd_check_launches() == before


def test_sweep_and_stack_give_what_the_solver_gives_alone(nsol):
    from nsol_amd.parameter_sweep import PrimalDualSweep
    from nsol_amd.solver_batch import PrimalDualBatch
    case = CASES[0]
    alone = _case_solver(case, np.float64)
    alone.run()
    t = _case_solver(case, np.float64)
    sweep = PrimalDualSweep(t._prox_f, t._prox_g_conj, t._B, t._B_conj, case[5],
                            observation(case[0]).flatten(),
                            {"alpha": [case[4], 2 * case[4]]}, iterations=case[9],
                            x_scale=t.get_x_scale(), dtype=np.float64,
                            tolerance=case[8], check_every=K)
    sweep.run()
    assert sweep.get_execution() == "sequential"
    assert sweep.get_iterations_done()[0] == case[10]
    assert np.array_equal(sweep.get_x(0), alone.get_x())
    members = [_case_solver(case, np.float64, tolerance=None, iterations=12),
               _case_solver(case, np.float64),
               _case_solver(case, np.float64, tolerance=None, iterations=12)]
    batch = PrimalDualBatch(members)
    batch.run()
    assert batch.get_execution() == ["stacked", "sequential", "stacked"]
    assert members[1].get_iterations_done() == case[10]
    assert np.array_equal(members[1].get_x(), alone.get_x())
    assert members[0].get_iterations_done() == 12
    assert members[0].get_stop_reason() == "iterations"


def test_bad_arguments_raise(nsol):
    for kw in (dict(tolerance=-1.0), dict(tolerance=float("nan")),
               dict(check_every=0), dict(check_every=-2)):
        with pytest.raises(ValueError):
            _case_solver(CASES[0], np.float32, **kw)


def test_run_denoising_cli_tolerance(tmp_path, capsys, nsol):
    from nsol_amd import nifti
    from nsol_amd.application import run_denoising
    from nsol_amd.data_reader import DataReader
    img = observation((24, 40))
    path, out = str(tmp_path / "img.nii.gz"), str(tmp_path / "out.nii.gz")
    nifti.write(path, img)
    rd = DataReader(path)
    rd.read_data()
    data = rd.get_data()
    args = ["--observation", path, "--result", out, "--reconstruction-type", "TVL2",
            "--alpha", "0.05", "--iterations", "400", "--dtype", "float64",
            "--tolerance", "1e-2", "--check-every", "5"]
    assert run_denoising.main(args) == 0
    s = run_denoising.build_solver(data, "TVL2", 0.05, 400, dtype=np.float64,
                                   tolerance=1e-2, check_every=5)
    s.run()
    text = capsys.readouterr().out
    assert "stopped after %d of 400 iterations (tolerance" % s.get_iterations_done() \
        in text
    assert s.get_iterations_done() < 400
    got, _, _ = nifti.read(out)
    assert rel_l2(got, s.get_x().reshape(data.shape)) < 1e-6      # float32 file


# r = |v_k - v_{k-1}| / |v_k| <= 1 + |v_{k-1}| / |v_k|: a tolerance of 10 is met at the
# first check of any run whose iterates keep their order of magnitude; 1e-300 never is
@pytest.mark.parametrize("tolerance,semi,done,reason", [
    ("10", True, 3, "tolerance"), ("1e-300", False, 7, "iterations")])
def test_run_deconvolution_cli_tolerance(tmp_path, capsys, nsol, tolerance, semi, done,
                                         reason):
    """--solver PD --tolerance: the semi-fused and the generic loop with
    nsol_pd_change_* on the deconvolution prox, the printed line and the file."""
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd import nifti
    from nsol_amd.application import run_deconvolution
    from nsol_amd.data_reader import DataReader
    img = observation((24, 40))
    path, out = str(tmp_path / "img.nii.gz"), str(tmp_path / "out.nii.gz")
    nifti.write(path, img)
    rd = DataReader(path)
    rd.read_data()
    data, info = rd.get_data(), rd.get_image_sitk()
    spacing = np.ones(data.ndim) if info is None else np.array(info.GetSpacing())
    args = ["--observation", path, "--result", out, "--reconstruction-type", "TVL2",
            "--solver", "PD", "--blur", "1.2", "--alpha", "0.05", "--iterations", "7",
            "--iter-max", "4", "--dtype", "float64", "--tolerance", tolerance,
            "--check-every", "3"]
    old = pd.USE_SEMI_FUSED
    pd.USE_SEMI_FUSED = semi
    try:
        assert run_deconvolution.main(args) == 0
        s = run_deconvolution.build_solver(
            data, spacing, 1.2, "TVL2", "PD", 0.05, 7, 4, dtype=np.float64,
            tolerance=float(tolerance), check_every=3)
        s.run()
    finally:
        pd.USE_SEMI_FUSED = old
    assert s.get_execution() != "fused"
    assert s.get_iterations_done() == done and s.get_stop_reason() == reason
    assert list(s.get_changes()[:, 0]) == [k for k in (3, 6, 7) if k <= done]
    assert np.all(np.isfinite(s.get_changes()))
    text = capsys.readouterr().out
    assert "stopped after %d of 7 iterations (%s" % (done, reason) in text
    got, _, _ = nifti.read(out)
    assert rel_l2(got, s.get_x().reshape(data.shape)) < 1e-6      # float32 file
