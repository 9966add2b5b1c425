"""The isotropic TV / Huber regulariser of the primal-dual solver on the GPU:
the stand-alone projection, the fused kernel k_pd_fused_iso against the NumPy
restatement of test_pd_isotropic_host.py, the bit-identity of every execution
form, the entries that must decline, and what the run minimises."""
import os

import numpy as np
import pytest

from conftest import rel_l2
from test_pd_isotropic_host import (disc_and_ramp, pd_iso_denoise, project_iso)

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12     # float64 kernels vs the float64 restatement
F32_TOL = 1e-5      # the project's standing gate on the primal iterate


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _lo(dim, spacing=None):
    import nsol_amd.linear_operators as LO
    cls = {1: LO.LinearOperators1D, 2: LO.LinearOperators2D,
           3: LO.LinearOperators3D}[dim]
    return cls() if spacing is None else cls(spacing=spacing)


def _solver(obs, reg, data, alpha, iters, L2, alg, dtype, spacing=None, iso=True,
            verbose=0):
    """Wiring of run_denoising.py:95-154 with the isotropic dual prox."""
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd.proximal_operators import ProximalOperators as prox
    b = obs.flatten()
    x_scale = np.max(obs)
    dim = obs.ndim
    grad, grad_adj = _lo(dim, spacing).get_gradient_operators()
    X_shape = obs.shape
    Z_shape = grad(obs).shape
    D = lambda x: grad(x.reshape(*X_shape)).flatten()
    D_adj = lambda x: grad_adj(x.reshape(*Z_shape)).flatten()
    if data == "L1":
        pf = lambda x, tau: prox.prox_ell1_denoising(x, tau, x0=b, x_scale=x_scale)
    else:
        pf = lambda x, tau: prox.prox_ell2_denoising(x, tau, x0=b, x_scale=x_scale)
    if not iso:
        pg = prox.prox_huber_conj if reg == "Huber" else prox.prox_tv_conj
    elif reg == "Huber":
        pg = lambda x, s: prox.prox_huber_conj_isotropic(x, s, dim)
    else:
        pg = lambda x, s: prox.prox_tv_conj_isotropic(x, s, dim)
    return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=pg, B=D, B_conj=D_adj, L2=L2,
                               x0=b, alpha=alpha, iterations=iters, x_scale=x_scale,
                               alg_type=alg, dtype=dtype, verbose=verbose)


# ------------------------------------------------------- 1. stand-alone prox
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 1000003])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_prox_dual_project_matches_the_restatement(nsol, n, dim):
    import torch
    from nsol_amd import ops
    from nsol_amd.proximal_operators import ProximalOperators as prox
    rng = np.random.default_rng(100 * dim + n % 97)
    q = 1.2 * rng.standard_normal(dim * n)
    q[::11] = 0.0
    sigma, gamma = 0.7, 0.05
    for huber in (False, True):
        den = 1. + sigma * gamma if huber else None
        call = (lambda v: prox.prox_huber_conj_isotropic(v, sigma, dim, gamma)) \
            if huber else (lambda v: prox.prox_tv_conj_isotropic(v, sigma, dim))
        # float64: the same operations in the same order, IEEE sqrt and division
        got = call(q)
        assert got.dtype == np.float64 and got.shape == q.shape
        assert np.array_equal(got, project_iso(q, dim, den))
        q32 = q.astype(np.float32)
        want32 = project_iso(q32, dim, None if den is None else np.float32(den))
        assert want32.dtype == np.float32
        got32 = call(q32)
        assert got32.dtype == np.float32
        err = rel_l2(got32, want32, "f32 dim%d n%d huber%d" % (dim, n, huber))
        print("prox_dual_project f32 dim %d n %d huber %d: %.3e" % (dim, n, huber, err))
        assert err <= 1e-6
        # device tensors, a view that starts one element behind a 16-byte boundary
        for dt, want in ((torch.float64, project_iso(q, dim, den)),
                         (torch.float32, want32)):
            buf = torch.zeros(dim * n + 5, dtype=dt, device="cuda")
            view = buf[1:1 + dim * n]
            view.copy_(torch.from_numpy(q).to(dt))
            out = call(view)
            assert out.data_ptr() != view.data_ptr() and out.shape == view.shape
            if dt == torch.float64:
                assert np.array_equal(out.cpu().numpy(), want)
            else:
                assert rel_l2(out.cpu().numpy(), want) <= 1e-6
            dst = torch.full((dim * n + 5,), 7.0, dtype=dt, device="cuda")
            ops.prox_dual_project(view, dim, 1.0 if den is None else den,
                                  out=dst[3:3 + dim * n])
            assert torch.equal(dst[3:3 + dim * n], out)
            assert float(dst[2]) == 7.0 and float(dst[3 + dim * n]) == 7.0


def test_prox_dual_project_refuses_a_length_the_dimension_does_not_divide(nsol):
    import torch
    from nsol_amd import ops
    from nsol_amd.proximal_operators import ProximalOperators as prox
    with pytest.raises(ValueError):
        ops.prox_dual_project(torch.zeros(7, device="cuda"), 2)
    with pytest.raises(ValueError):
        ops.prox_dual_project(torch.zeros(8, device="cuda"), 4)
    with pytest.raises(ValueError):
        prox.prox_tv_conj_isotropic(np.zeros(10), 0.5, 3)
    with pytest.raises(ValueError):
        prox.prox_huber_conj_isotropic(torch.zeros(10, device="cuda"), 0.5, 3)


# ------------------------------------------- 2. fused runs vs the restatement
ISO_CASES = [(reg, data, alg) for reg in ("TV", "Huber") for data in ("L2", "L1")
             for alg in ("ALG2", "ALG2_AHMOD", "ALG3")]


@pytest.mark.parametrize("shape", [(37, 50), (16, 20, 24)])
@pytest.mark.parametrize("reg,data,alg", ISO_CASES)
def test_fused_isotropic_run_matches_the_restatement(nsol, shape, reg, data, alg):
    rng = np.random.default_rng(len(shape))
    obs = 50.0 + 30.0 * rng.standard_normal(shape)
    alpha = 0.05 if data == "L2" else 0.6
    L2 = 8.0 * (len(shape) - 1)
    ref = pd_iso_denoise(obs.flatten(), shape, reg, data, alpha, 25, L2, alg)
    for dtype, tol in ((np.float64, F64_TOL), (np.float32, F32_TOL)):
        s = _solver(obs, reg, data, alpha, 25, L2, alg, dtype)
        s.run()
        assert s.get_execution() == "fused"
        err = rel_l2(s.get_x(), ref, np.dtype(dtype).name)
        print("iso %s %s %s %s %s: %.3e" % (shape, reg, data, alg,
                                             np.dtype(dtype).name, err))
        assert err <= tol
    # the two regularisers do differ here (the test would pass on the clamp else)
    s = _solver(obs, reg, data, alpha, 25, L2, alg, np.float64, iso=False)
    s.run()
    assert rel_l2(s.get_x(), ref, "anisotropic") > 1e-4


def test_fused_isotropic_run_with_spacing_matches_the_restatement(nsol):
    shape = (16, 20, 24)
    spacing = np.array([0.8, 1.3, 0.5])
    rng = np.random.default_rng(5)
    obs = 50.0 + 30.0 * rng.standard_normal(shape)
    ref = pd_iso_denoise(obs.flatten(), shape, "Huber", "L2", 0.05, 25, 32.0, "ALG2",
                         spacing=spacing)
    for dtype, tol in ((np.float64, F64_TOL), (np.float32, F32_TOL)):
        s = _solver(obs, "Huber", "L2", 0.05, 25, 32.0, "ALG2", dtype, spacing=spacing)
        s.run()
        assert s.get_execution() == "fused"
        err = rel_l2(s.get_x(), ref, np.dtype(dtype).name)
        print("iso spacing %s: %.3e" % (np.dtype(dtype).name, err))
        assert err <= tol


@pytest.mark.parametrize("n", [1, 2, 9, 77, 1024, 1031])
@pytest.mark.parametrize("reg,data", [("TV", "L2"), ("Huber", "L1")])
def test_isotropic_is_the_anisotropic_run_bit_for_bit_in_1d(nsol, n, reg, data):
    rng = np.random.default_rng(n)
    obs = 50.0 + 30.0 * rng.standard_normal((n,))
    alpha = 0.05 if data == "L2" else 0.6
    for dtype in (np.float64, np.float32):
        a = _solver(obs, reg, data, alpha, 25, 4.0, "ALG2", dtype)
        a.run()
        b = _solver(obs, reg, data, alpha, 25, 4.0, "ALG2", dtype, iso=False)
        b.run()
        assert a.get_execution() == b.get_execution() == "fused"
        assert np.array_equal(a.get_x(), b.get_x())


# --------------------------------------------- 3. all forms give the same bits
FORM_SHAPES = [(5, 7, 18), (4, 6, 19), (3, 5, 63), (6, 9, 64), (3, 21, 260),
               (1, 1, 7), (2, 2, 2), (1, 5, 9), (5, 1, 9), (7, 9, 1), (2, 9, 2),
               (40, 37), (9, 300), (1, 9), (2, 19), (30, 255), (9, 1), (13, 2),
               (77,), (2,), (1,), (1031,),
               (96, 150, 130)]


@pytest.mark.parametrize("shape", FORM_SHAPES)
def test_every_isotropic_form_gives_the_same_bits(nsol, shape):
    """nsol_pd_run_* == a launch per iteration through nsol_pd_fused_iter_* == the
    two-pass form (nsol_pd_dual_step_iso_* + the primal step) == the semi-fused
    loop == the generic device loop (nsol_grad_*, the stand-alone projection,
    nsol_grad_adj_*, the data prox) == the row-pitched entry, float64 and float32,
    with short z-chunks so that every halo path (left, above, plane before a seam,
    volume borders) lies inside the volume."""
    import torch
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd import _lib, ops
    big = int(np.prod(shape)) > 100000
    iters = 4 if big else 7
    rng = np.random.default_rng(sum(shape))
    obs = 50.0 + 30.0 * rng.standard_normal(shape)
    reg, data, alpha, L2 = "Huber", "L1", 0.5, 4.0 * len(shape)
    ref = pd_iso_denoise(obs.flatten(), shape, reg, data, alpha, iters, L2, "ALG2")
    old = (pd.USE_SEMI_FUSED, pd.PITCH_MIN_VOXELS)
    try:
        for dtype in (np.float64, np.float32):
            _lib.set_param("pd_zchunk", 0 if big else 3)
            pd.PITCH_MIN_VOXELS = 1 << 62
            s = _solver(obs, reg, data, alpha, iters, L2, "ALG2", dtype)
            s.run()
            assert s.get_execution() == "fused"
            fused = s.get_x()
            err = rel_l2(fused, ref, np.dtype(dtype).name)
            assert err <= (F64_TOL if dtype == np.float64 else F32_TOL), err
            # one launch per iteration (the verbose loop calls nsol_pd_fused_iter_*)
            s = _solver(obs, reg, data, alpha, iters, L2, "ALG2", dtype, verbose=1)
            s.run()
            assert np.array_equal(s.get_x(), fused)
            # other rows per lane, one z-chunk
            _lib.set_param("pd_zchunk", 1 << 20)
            for ry in (1, 2):
                _lib.set_param("pd_ry", ry)
                s = _solver(obs, reg, data, alpha, iters, L2, "ALG2", dtype)
                s.run()
                assert np.array_equal(s.get_x(), fused), ry
            _lib.set_param("pd_ry", 0)
            _lib.set_param("pd_zchunk", 0 if big else 3)
            # 4-byte accesses instead of the ragged vectors
            _lib.set_param("pd_rag", 0)
            s = _solver(obs, reg, data, alpha, iters, L2, "ALG2", dtype)
            s.run()
            assert np.array_equal(s.get_x(), fused)
            _lib.set_param("pd_rag", 1)
            # two passes: the isotropic dual step, then the primal step
            _lib.set_param("pd_two_pass", 1)
            s = _solver(obs, reg, data, alpha, iters, L2, "ALG2", dtype)
            s.run()
            _lib.set_param("pd_two_pass", 0)
            assert np.array_equal(s.get_x(), fused)
            # the semi-fused loop and the generic device loop
            for semi in (True, False):
                pd.USE_SEMI_FUSED = semi
                s = _solver(obs, reg, data, alpha, iters, L2, "ALG2", dtype)
                s.plan = lambda: None
                s.run()
                assert s.get_execution() == "device"
                assert np.array_equal(s.get_x(), fused), semi
            pd.USE_SEMI_FUSED = old[0]
            # rows at a pitch (3-D volumes whose rows are not whole vectors)
            like = torch.empty(1, dtype=torch.float64 if dtype == np.float64
                               else torch.float32)
            if ops.row_pitch(shape, like):
                pd.PITCH_MIN_VOXELS = 1
                s = _solver(obs, reg, data, alpha, iters, L2, "ALG2", dtype)
                s.run()
                assert s.get_execution() == "fused"
                assert np.array_equal(s.get_x(), fused)
            else:
                # rows of whole vectors, or too short for two
                assert shape[-1] % (16 // np.dtype(dtype).itemsize) == 0 or \
                    len(shape) != 3 or shape[-1] < 2 * (16 // np.dtype(dtype).itemsize)
    finally:
        pd.USE_SEMI_FUSED, pd.PITCH_MIN_VOXELS = old
        for k in ("pd_zchunk", "pd_ry", "pd_rag", "pd_two_pass"):
            _lib.set_param(k, _lib.PARAM_DEFAULTS[k])


# ------------------------------------------------------------------ 4. declines
def _state(shape, dtype, members=1):
    import torch
    n = int(np.prod(shape))
    dim = len(shape)
    g = torch.Generator(device="cpu").manual_seed(n)
    bt = torch.rand(n, generator=g, dtype=torch.float64).to(dtype).cuda()
    x = bt.repeat(members).contiguous()
    sent = -77.0
    return dict(bt=bt, x=x, xbar=x.clone(),
                xbar_out=torch.full_like(x, sent), x_out=torch.full_like(x, sent),
                p=torch.zeros(members * dim * n, dtype=dtype, device="cuda"),
                p_out=torch.full((members * dim * n,), sent, dtype=dtype,
                                 device="cuda"), sent=sent)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_multi_iteration_and_stacked_entries_decline_the_isotropic_bit(nsol, dtype):
    """nsol_pd_fused2_iter, nsol_pd_fusedk_iter, nsol_pd_persist_run and
    nsol_pd_sweep_run return -2 with the bit set and touch nothing."""
    import torch
    from nsol_amd import _lib, ops
    dt = getattr(torch, dtype)
    shape = (16, 32, 512)                  # a shape all four take without the bit
    w = (1.0, 1.0, 1.0)
    _lib.set_param("pdk_min_kvox", 0)
    for reg in (ops.PD_REG_TV, ops.PD_REG_HUBER):
        flags = reg | ops.PD_REG_ISOTROPIC | ops.PD_DATA_L2
        st = _state(shape, dt)

        def untouched(st=st):
            torch.cuda.synchronize()
            for k in ("xbar_out", "x_out", "p_out"):
                assert bool((st[k] == st["sent"]).all()), k
        two = [0.3, 0.31]
        assert ops.pd_fused2_iter(st["xbar"], st["xbar_out"], st["x"], st["x_out"],
                                  st["bt"], st["p"], st["p_out"], shape, w, two,
                                  [1.0, 1.0], two, two, [1.0, 1.0], flags) is False
        untouched()
        for k in (2, 3):
            a = [0.3] * k
            assert ops.pd_fusedk_iter(st["xbar"], st["xbar_out"], st["x"], st["x_out"],
                                      st["bt"], st["p"], st["p_out"], shape, w, a,
                                      [1.0] * k, a, a, [1.0] * k, flags) is False
            untouched()
        sig = np.full(20, 0.3)
        before = ops.pd_persist_launches()
        assert ops.pd_persist_run(st["xbar"], st["x"], st["bt"], st["p"], shape, w,
                                  30.0, sig, sig, sig, True, 0.05, flags,
                                  out=(st["xbar_out"], st["x_out"], st["p_out"])) \
            is False
        untouched()
        assert ops.pd_persist_launches() == before and not ops._pending_runs
        members = 3
        sw = _state(shape, dt, members)
        sched = np.full((members, 4), 0.3)
        launches = ops.pd_sweep_launches()
        x_before = sw["x"].clone()
        assert ops.pd_sweep_run(sw["xbar"], sw["xbar_out"], sw["x"], sw["bt"], sw["p"],
                                sw["p_out"], members, shape, w, np.full(members, 30.0),
                                sched, sched, sched, True, 0.05, flags) is None
        torch.cuda.synchronize()
        assert ops.pd_sweep_launches() == launches
        assert torch.equal(sw["x"], x_before)
        assert bool((sw["xbar_out"] == sw["sent"]).all())
        assert bool((sw["p_out"] == sw["sent"]).all())


def test_isotropic_sweep_runs_its_members_sequentially(nsol):
    from nsol_amd.parameter_sweep import PrimalDualSweep
    from nsol_amd import ops
    shape = (12, 20, 24)
    rng = np.random.default_rng(9)
    obs = 50.0 + 30.0 * rng.standard_normal(shape)
    alphas = [0.02, 0.05, 0.11]
    t = _solver(obs, "TV", "L2", 0.05, 12, 16.0, "ALG2", np.float32)
    launches = ops.pd_sweep_launches()
    sweep = PrimalDualSweep(prox_f=t._prox_f, prox_g_conj=t._prox_g_conj, B=t._B,
                            B_conj=t._B_conj, L2=16.0, x0=obs.flatten(),
                            parameters={"alpha": alphas}, iterations=12,
                            x_scale=np.max(obs), dtype=np.float32)
    sweep.run()
    assert sweep.get_execution() == "sequential"
    assert ops.pd_sweep_launches() == launches
    for k, alpha in enumerate(alphas):
        s = _solver(obs, "TV", "L2", alpha, 12, 16.0, "ALG2", np.float32)
        s.run()
        assert np.array_equal(sweep.get_x(k), s.get_x())
    # the same sweep with the component-wise clamp does stack
    a = _solver(obs, "TV", "L2", 0.05, 12, 16.0, "ALG2", np.float32, iso=False)
    sweep = PrimalDualSweep(prox_f=a._prox_f, prox_g_conj=a._prox_g_conj, B=a._B,
                            B_conj=a._B_conj, L2=16.0, x0=obs.flatten(),
                            parameters={"alpha": alphas}, iterations=12,
                            x_scale=np.max(obs), dtype=np.float32)
    sweep.run()
    assert sweep.get_execution() == "stacked"


def test_isotropic_run_stays_off_the_persist_kernel(nsol):
    """64^3, 50 iterations: inside the range persist_pays accepts (the fixture
    leaves ops.PD_PERSIST on for tests with 'persist' in their name)."""
    from nsol_amd import ops
    assert ops.PD_PERSIST and ops.persist_pays((64, 64, 64), 50)
    rng = np.random.default_rng(64)
    obs = 50.0 + 30.0 * rng.standard_normal((64, 64, 64))
    before = ops.pd_persist_launches()
    s = _solver(obs, "TV", "L2", 0.05, 50, 16.0, "ALG2", np.float32)
    s.run()
    assert s.get_execution() == "fused"
    assert ops.pd_persist_launches() == before and not ops._pending_runs
    ops.PD_PERSIST = False
    try:
        t = _solver(obs, "TV", "L2", 0.05, 50, 16.0, "ALG2", np.float32)
        t.run()
    finally:
        ops.PD_PERSIST = True
    assert np.array_equal(s.get_x(), t.get_x())
    a = _solver(obs, "TV", "L2", 0.05, 50, 16.0, "ALG2", np.float32, iso=False)
    a.run()
    assert ops.pd_persist_launches() == before + 1      # the clamp does go there


# ------------------------------------------- 5. it minimises what it claims to
def test_isotropic_run_minimises_the_isotropic_objective(nsol):
    """2-D 64 x 64, float64, TV-l2, alpha 0.03, 300 iterations on a disc plus an
    edge at 30 degrees plus noise.  In the solver's units F(x) = |x - b~|^2 / (2
    alpha) + TV_iso(x), F_aniso the same with sum_a |d_a x|.  The NumPy restatement
    gives F(x_aniso) - F(x_iso) = 14.45 of 465.66 and F_aniso(x_iso) -
    F_aniso(x_aniso) = 19.19 of 510.85 (3.1e-2 and 3.8e-2 relative)."""
    from nsol_amd.prior_measures import PriorMeasures
    img = disc_and_ramp()
    shape, alpha = img.shape, 0.03
    scale = img.max()
    bt = img.reshape(-1) / scale
    grad, _ = _lo(2).get_gradient_operators()
    D = lambda v: grad(v.reshape(*shape)).flatten()
    F = {}
    for iso in (True, False):
        s = _solver(img, "TV", "L2", alpha, 300, 8.0, "ALG2", np.float64, iso=iso)
        s.run()
        assert s.get_execution() == "fused"
        x = s.get_x() / scale
        fid = 0.5 * np.sum((x - bt) ** 2) / alpha
        tv_iso = PriorMeasures.total_variation(x, D, 2)
        tv_aniso = float(np.sum(np.abs(D(x))))
        F[iso] = (fid + tv_iso, fid + tv_aniso)
    print("F_iso: iso run %.6f, aniso run %.6f; F_aniso: iso run %.6f, aniso run %.6f"
          % (F[True][0], F[False][0], F[True][1], F[False][1]))
    assert F[True][0] < F[False][0]
    assert F[False][1] < F[True][1]
    ref = pd_iso_denoise(img.reshape(-1), shape, "TV", "L2", alpha, 300, 8.0, "ALG2")
    s = _solver(img, "TV", "L2", alpha, 300, 8.0, "ALG2", np.float64)
    s.run()
    assert rel_l2(s.get_x(), ref) <= 1e-11      # 300 iterations of rounding


# -------------------------------------------------------- 6. agreement with ADMM
def test_isotropic_primal_dual_agrees_with_admm(nsol):
    """min |x - b|^2 / 2 + alpha TV_iso(x) on a 48 x 48 image, A = identity, float64,
    alpha 0.05, rho 0.5: primal-dual after N = 500 iterations against ADMM after M =
    100 (LSMR iter_max 10).  On the CPU (the NumPy restatement against
    oracle.nsol_oracle.admm) the relative distance is 2.75e-4 for the isotropic run
    and 2.64e-2 for the anisotropic one; the GPU pair is gated at twice the first
    figure, 5.5e-4 (LSMR's truncation differs between the two ADMM
    implementations)."""
    from nsol_amd.admm_linear_solver import ADMMLinearSolver
    img = disc_and_ramp(48, seed=11)
    shape = img.shape
    b = img.reshape(-1)
    alpha, rho = 0.05, 0.5
    grad, grad_adj = _lo(2).get_gradient_operators()
    Z = grad(img).shape
    ident = lambda v: v.flatten()
    D = lambda v: grad(v.reshape(*shape)).flatten()
    Da = lambda v: grad_adj(v.reshape(*Z)).flatten()
    admm = ADMMLinearSolver(A=ident, A_adj=ident, b=b, B=D, B_adj=Da, x0=b,
                            dimension=2, alpha=alpha, rho=rho, iterations=100,
                            iter_max=10, x_scale=np.max(b), dtype=np.float64)
    admm.run()
    xad = admm.get_x()
    dist = {}
    for iso in (True, False):
        s = _solver(img, "TV", "L2", alpha, 500, 8.0, "ALG2", np.float64, iso=iso)
        s.run()
        dist[iso] = rel_l2(s.get_x(), xad, "iso" if iso else "aniso")
    print("|x_PD - x_ADMM| / |x_ADMM|: isotropic %.3e, anisotropic %.3e"
          % (dist[True], dist[False]))
    assert dist[True] <= 2 * 2.75e-4
    assert dist[False] > dist[True]


# ---------------------------------------------------------------------- 7. CLI
@pytest.mark.parametrize("rtype", ["TVL2", "HuberL1"])
def test_run_denoising_cli_isotropic_switch(tmp_path, golden, rtype, nsol):
    from nsol_amd import nifti
    from nsol_amd.data_writer import DataWriter
    from nsol_amd.data_reader import DataReader
    from nsol_amd.application import run_denoising
    g = golden("configs")
    png = str(tmp_path / "2D_Lena_256_noise.png")
    DataWriter(g["lena_noise_u8"].astype(np.float64), png).write_data()
    nii = str(tmp_path / "3D_SheppLoganPhantom_64.nii.gz")
    nifti.write(nii, g["phantom64"].astype(np.float64))
    for src, ext in ((png, "png"), (nii, "nii.gz")):
        obs = DataReader(src)
        obs.read_data()
        res = {}
        for iso in (True, False):
            out = str(tmp_path / ("out_%s_%d.%s" % (rtype, iso, ext)))
            rc = run_denoising.main(["--observation", src, "--result", out,
                                     "--reconstruction-type", rtype,
                                     "--iterations", "20", "--dtype", "float64"]
                                    + (["--isotropic"] if iso else []))
            assert rc == 0 and os.path.isfile(out)
            r = DataReader(out)
            r.read_data()
            s = run_denoising.build_solver(obs.get_data(), rtype, 0.03, 20,
                                           dtype=np.float64, isotropic=iso)
            s.run()
            assert s.get_execution() == "fused"
            want = s.get_x().reshape(obs.get_data().shape)
            res[iso] = want
            if ext == "png":
                assert np.array_equal(r.get_data(), np.round(want).astype(np.uint8))
            else:
                assert rel_l2(r.get_data(), want) < 1e-6      # float32 file
        # without the switch: what the tool has always written
        s = run_denoising.build_solver(obs.get_data(), rtype, 0.03, 20,
                                       dtype=np.float64)
        s.run()
        assert np.array_equal(s.get_x().reshape(obs.get_data().shape), res[False])
        if rtype.endswith("L2"):
            # (an l1 data term of this weight leaves the observation as it is,
            # whatever the regulariser)
            assert rel_l2(res[True], res[False]) > 1e-5


def test_run_denoising_cli_isotropic_sweep_is_sequential(tmp_path, golden, capsys,
                                                        nsol):
    from nsol_amd import nifti
    from nsol_amd.data_reader import DataReader
    from nsol_amd.application import run_denoising
    vol = golden("configs")["phantom64"][:24, :32, :40].astype(np.float64)
    nii = str(tmp_path / "vol.nii.gz")
    nifti.write(nii, vol)
    rdir = str(tmp_path / "members")
    os.makedirs(rdir)
    alphas = [0.02, 0.05, 0.1]
    rc = run_denoising.main(["--observation", nii, "--result-dir", rdir,
                             "--reconstruction-type", "TVL2", "--iterations", "10",
                             "--dtype", "float32", "--isotropic", "--alpha"]
                            + ["%g" % a for a in alphas])
    assert rc == 0
    assert capsys.readouterr().out.count("(sequential)") == len(alphas)
    obs = DataReader(nii)
    obs.read_data()
    for a in alphas:
        got, _, _ = nifti.read(run_denoising.member_result_path(rdir, nii, a))
        s = run_denoising.build_solver(obs.get_data(), "TVL2", a, 10,
                                       dtype=np.float32, isotropic=True)
        s.run()
        want = s.get_x().reshape(obs.get_data().shape)
        assert rel_l2(got, want) < 1e-6                       # float32 file
