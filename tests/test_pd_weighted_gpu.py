"""The weighted / masked data term of the primal-dual solver on the GPU: the
stand-alone prox, the fused kernels k_pd_w / k_pd_w_iso against the NumPy
restatement of test_pd_weighted_host.py, the bit-identity of the execution forms,
the stacked sweep and batch, the entries that must decline, inpainting, and the
command line."""
import os

import numpy as np
import pytest

from conftest import rel_l2
from test_pd_weighted_host import mixed_weights, pd_weighted_denoise, prox_weighted

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12     # float64 kernels vs the float64 restatement
F32_TOL = 1e-5      # the project's standing gate on the primal iterate
ITERS = 25


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


def _solver(obs, weights, reg, data, alpha, iters, L2, alg, dtype, iso=False,
            spacing=None, x_scale=None, x0=None, verbose=0):
    """Wiring of run_denoising.py:95-154 with the weighted data prox (weights None:
    the unweighted one)."""
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd.proximal_operators import ProximalOperators as prox
    b = obs.flatten()
    start = b if x0 is None else np.asarray(x0, np.float64).flatten()
    x_scale = float(np.max(start)) if x_scale is None else float(x_scale)
    dim = obs.ndim
    grad, grad_adj = _lo(dim, spacing).get_gradient_operators()
    X_shape = obs.shape
    Z_shape = grad(start.reshape(X_shape)).shape
    D = lambda x: grad(x.reshape(*X_shape)).flatten()
    D_adj = lambda x: grad_adj(x.reshape(*Z_shape)).flatten()
    if weights is None:
        f = prox.prox_ell1_denoising if data == "L1" else prox.prox_ell2_denoising
        pf = lambda x, tau: f(x, tau, x0=b, x_scale=x_scale)
    else:
        w = np.asarray(weights).flatten()
        f = prox.prox_ell1_denoising_weighted if data == "L1" else \
            prox.prox_ell2_denoising_weighted
        pf = lambda x, tau: f(x, tau, x0=b, weights=w, x_scale=x_scale)
    if not iso:
        pg = prox.prox_huber_conj if reg == "Huber" else prox.prox_tv_conj
    elif reg == "Huber":
        pg = lambda x, s: prox.prox_huber_conj_isotropic(x, s, dim)
    else:
        pg = lambda x, s: prox.prox_tv_conj_isotropic(x, s, dim)
    return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=pg, B=D, B_conj=D_adj, L2=L2,
                               x0=start, alpha=alpha, iterations=iters,
                               x_scale=x_scale, alg_type=alg, dtype=dtype,
                               verbose=verbose)


def _obs(shape, seed=None):
    rng = np.random.default_rng(sum(shape) if seed is None else seed)
    return 50.0 + 30.0 * rng.standard_normal(shape)


def _gate(dtype):
    return F64_TOL if np.dtype(dtype) == np.float64 else F32_TOL


# ------------------------------------------------------- 1. stand-alone prox
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1031])
@pytest.mark.parametrize("data", ["L2", "L1"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_weighted_prox_matches_numpy(nsol, n, data, dtype):
    from nsol_amd.proximal_operators import ProximalOperators as prox
    rng = np.random.default_rng(n)
    u = rng.standard_normal(n).astype(dtype)
    b = (3.0 * rng.standard_normal(n)).astype(dtype)
    w = mixed_weights((n,), n).astype(dtype)
    if n > 2:
        w[1] = 2.5
    tau, xs = 0.37, 3.0
    f = prox.prox_ell1_denoising_weighted if data == "L1" else \
        prox.prox_ell2_denoising_weighted
    got = f(u, tau, b, w, x_scale=xs)
    assert got.dtype == dtype and got.shape == u.shape
    bt = (b.astype(np.float64) / xs).astype(dtype)         # rounded once
    want = prox_weighted(u, dtype(tau), bt, w, data)       # in the working dtype
    assert want.dtype == dtype
    if dtype == np.float64 or data == "L1":
        # the same IEEE operations in the same order
        assert np.array_equal(got, want)
    else:
        assert rel_l2(got, want) <= 1e-6
    assert np.array_equal(got[w == 0], u[w == 0])
    # garbage where the weight is zero: u comes back bit for bit
    junk = b.copy()
    junk[w == 0] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype), int((w == 0).sum()))
    again = f(u, tau, junk, w, x_scale=xs)
    assert np.array_equal(again, got)
    # bool and integer weights, device tensors
    import torch
    mask = w > 0
    gm = f(u, tau, junk, mask, x_scale=xs)
    gi = f(torch.from_numpy(u).cuda(), tau, torch.from_numpy(junk).cuda(),
           torch.from_numpy(mask.astype(np.int32)).cuda(), x_scale=xs)
    ones = prox_weighted(u, dtype(tau), bt, mask.astype(dtype), data)
    assert np.array_equal(gm, gi.cpu().numpy())
    assert np.array_equal(gm[~mask], u[~mask])
    assert rel_l2(gm, ones) <= 1e-6


def test_weighted_prox_refuses_wrong_weights(nsol):
    import torch
    from nsol_amd.proximal_operators import ProximalOperators as prox
    u, b = np.zeros(8), np.ones(8)
    for w in (np.full(8, -1.0), np.full(8, np.nan), np.ones(7),
              torch.full((8,), -1.0, device="cuda"),
              torch.full((8,), float("inf"), device="cuda")):
        with pytest.raises(ValueError):
            prox.prox_ell2_denoising_weighted(u, 0.1, b, w)
        with pytest.raises(ValueError):
            prox.prox_ell1_denoising_weighted(torch.zeros(8, device="cuda",
                                                          dtype=torch.float64), 0.1, b, w)


# ------------------------------------------- 2. fused run vs the restatement
# (shape, reg, data, iso, alg, dtypes, iterations): every access form and boundary
# of the issue's list, {TV, Huber} x {l1, l2} x {anisotropic, isotropic}, every
# alg_type
BOTH = (np.float64, np.float32)
FUSED_CASES = [
    ((1,), "TV", "L2", False, "ALG2", BOTH, ITERS),
    ((2,), "Huber", "L1", True, "ALG2", BOTH, ITERS),
    ((65,), "TV", "L1", False, "ALG3", BOTH, ITERS),
    ((1031,), "Huber", "L2", True, "ALG2_AHMOD", BOTH, ITERS),
    ((37, 50), "TV", "L2", False, "ALG2", BOTH, ITERS),            # ragged
    ((37, 50), "Huber", "L1", True, "ALG3", BOTH, ITERS),
    ((16, 64), "TV", "L1", True, "ALG2", BOTH, ITERS),             # whole vectors
    ((16, 64), "Huber", "L2", False, "ALG2_AHMOD", BOTH, ITERS),
    ((5, 7, 9), "TV", "L2", True, "ALG2", BOTH, ITERS),            # single elements
    ((5, 7, 9), "Huber", "L1", False, "ALG2", BOTH, ITERS),
    ((16, 20, 24), "TV", "L1", False, "ALG2", BOTH, ITERS),        # vectors, 16 lanes
    ((16, 20, 24), "Huber", "L2", True, "ALG3", BOTH, ITERS),
    ((6, 9, 130), "TV", "L2", False, "ALG2", BOTH, ITERS),         # ragged vectors
    ((6, 9, 130), "Huber", "L2", True, "ALG2", BOTH, ITERS),
    ((3, 5, 256), "TV", "L2", True, "ALG2", BOTH, ITERS),          # 64 lanes, whole
    ((3, 5, 260), "Huber", "L1", False, "ALG2", BOTH, ITERS),      # 64 lanes, ragged
    ((3, 5, 260), "TV", "L2", True, "ALG2", BOTH, ITERS),
    # the smallest single volume with two rows per lane (16 tiles x 32 >= 512)
    ((64, 128, 256), "TV", "L2", False, "ALG2", (np.float32,), 10),
    ((64, 128, 256), "Huber", "L2", True, "ALG2", (np.float32,), 10),
]


@pytest.mark.parametrize("shape,reg,data,iso,alg,dtypes,iters", FUSED_CASES)
def test_fused_weighted_run_matches_the_restatement(nsol, shape, reg, data, iso, alg,
                                                    dtypes, iters):
    from nsol_amd import ops
    obs = _obs(shape)
    w = mixed_weights(shape, sum(shape))
    alpha = 0.6 if data == "L1" else 0.05
    L2 = 4.0 * len(shape)
    xs = float(np.max(obs))
    ref = pd_weighted_denoise(obs, w, shape, reg, data, alpha, iters, L2, alg, iso=iso,
                              x_scale=xs)
    for dtype in dtypes:
        before = ops.pd_weighted_launches()
        s = _solver(obs, w, reg, data, alpha, iters, L2, alg, dtype, iso=iso)
        s.run()
        assert s.get_execution() == "fused"
        assert ops.pd_weighted_launches() == before + iters
        err = rel_l2(s.get_x(), ref, np.dtype(dtype).name)
        print(shape, reg, data, iso, alg, np.dtype(dtype).name, err)
        assert err <= _gate(dtype), err


@pytest.mark.parametrize("dtype", BOTH)
def test_fused_weighted_run_with_spacing_and_scale_matches_the_restatement(nsol, dtype):
    shape, spacing = (6, 9, 130), np.array([0.7, 1.3, 2.0])
    obs = _obs(shape)
    w = mixed_weights(shape, 11)
    for iso in (False, True):
        ref = pd_weighted_denoise(obs, w, shape, "Huber", "L2", 0.05, ITERS, 30.0,
                                  "ALG2", iso=iso, spacing=spacing, x_scale=37.5)
        s = _solver(obs, w, "Huber", "L2", 0.05, ITERS, 30.0, "ALG2", dtype, iso=iso,
                    spacing=spacing, x_scale=37.5)
        s.run()
        assert s.get_execution() == "fused"
        err = rel_l2(s.get_x(), ref, "%s iso=%d" % (np.dtype(dtype).name, iso))
        assert err <= _gate(dtype), err


# --------------------------------------------------------------- 3. bit-identity
@pytest.mark.parametrize("shape", [(37, 50), (6, 9, 130)])
@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("dtype", BOTH)
def test_fused_weighted_run_is_the_generic_device_loop_bit_for_bit(nsol, shape, iso,
                                                                   dtype):
    """nsol_pd_weighted_run_* == nsol_grad_*, the dual prox, nsol_grad_adj_* and the
    stand-alone weighted prox glued by axpy kernels (USE_SEMI_FUSED off), and == the
    semi-fused loop: all of them go through prox_data_w."""
    import nsol_amd.primal_dual_solver as pd
    obs = _obs(shape)
    w = mixed_weights(shape, 3)
    old = pd.USE_SEMI_FUSED
    try:
        for data in ("L2", "L1"):
            alpha = 0.6 if data == "L1" else 0.05
            s = _solver(obs, w, "Huber", data, alpha, ITERS, 12.0, "ALG2", dtype, iso=iso)
            s.run()
            assert s.get_execution() == "fused"
            fused = s.get_x()
            for semi in (False, True):
                pd.USE_SEMI_FUSED = semi
                g = _solver(obs, w, "Huber", data, alpha, ITERS, 12.0, "ALG2", dtype,
                            iso=iso)
                g.plan = lambda: None
                g.run()
                assert g.get_execution() == "device"
                assert np.array_equal(g.get_x(), fused), (data, semi)
    finally:
        pd.USE_SEMI_FUSED = old


@pytest.mark.parametrize("shape", [(16, 20, 24), (37, 50)])
@pytest.mark.parametrize("iso", [False, True])
def test_unit_weights_give_the_unweighted_bits_in_float64(nsol, shape, iso):
    obs = _obs(shape)
    for data in ("L2", "L1"):
        alpha = 0.6 if data == "L1" else 0.05
        a = _solver(obs, np.ones(shape), "TV", data, alpha, ITERS, 12.0, "ALG2",
                    np.float64, iso=iso)
        b = _solver(obs, None, "TV", data, alpha, ITERS, 12.0, "ALG2", np.float64,
                    iso=iso)
        a.run()
        b.run()
        assert a.get_execution() == b.get_execution() == "fused"
        assert np.array_equal(a.get_x(), b.get_x())
        # float32 divides where the unweighted kernels multiply by a reciprocal
        a = _solver(obs, np.ones(shape), "TV", data, alpha, ITERS, 12.0, "ALG2",
                    np.float32, iso=iso)
        b = _solver(obs, None, "TV", data, alpha, ITERS, 12.0, "ALG2", np.float32,
                    iso=iso)
        a.run()
        b.run()
        assert rel_l2(a.get_x(), b.get_x(), data) <= F32_TOL


@pytest.mark.parametrize("dtype", BOTH)
def test_garbage_under_a_zero_weight_changes_no_bit(nsol, dtype):
    shape = (6, 9, 130)
    obs = _obs(shape)
    w = mixed_weights(shape, 4)
    zeroed = np.where(w == 0, 0.0, obs)
    junk = np.where(w == 0, np.nan, obs)
    junk[0, 0, 0] = np.inf
    xs = float(np.max(obs))
    for data, iso in (("L2", False), ("L1", True)):
        alpha = 0.6 if data == "L1" else 0.05
        a = _solver(zeroed, w, "TV", data, alpha, ITERS, 12.0, "ALG2", dtype, iso=iso,
                    x_scale=xs, x0=obs)
        b = _solver(junk, w, "TV", data, alpha, ITERS, 12.0, "ALG2", dtype, iso=iso,
                    x_scale=xs, x0=obs)
        a.run()
        b.run()
        assert np.all(np.isfinite(b.get_x()))
        assert np.array_equal(a.get_x(), b.get_x())


@pytest.mark.parametrize("dtype", BOTH)
def test_stepwise_weighted_path_is_the_enqueued_run_bit_for_bit(nsol, dtype):
    """A host observer (every iterate kept) and the verbose loop go through
    nsol_pd_weighted_iter_*, a device-mode observer through chunks of the run."""
    from nsol_amd.observer import Observer
    shape = (6, 9, 130)
    obs = _obs(shape)
    w = mixed_weights(shape, 5)
    s = _solver(obs, w, "Huber", "L2", 0.05, ITERS, 12.0, "ALG2", dtype, iso=True)
    s.run()
    want = s.get_x()
    t = _solver(obs, w, "Huber", "L2", 0.05, ITERS, 12.0, "ALG2", dtype, iso=True)
    o = Observer()
    o.set_measures({"mean": lambda x: float(np.mean(x))})
    t.set_observer(o)
    t.run()
    assert t.get_execution() == "fused"
    assert np.array_equal(t.get_x(), want)
    o.compute_measures()
    assert len(o.get_measures()["mean"]) == ITERS + 1
    v = _solver(obs, w, "Huber", "L2", 0.05, ITERS, 12.0, "ALG2", dtype, iso=True,
                verbose=1)
    v.run()
    assert np.array_equal(v.get_x(), want)
    d = _solver(obs, w, "Huber", "L2", 0.05, ITERS, 12.0, "ALG2", dtype, iso=True)
    od = Observer(keep_iterates=False, every=7)
    od.set_measures({"mean": lambda x: float(np.mean(x))})
    d.set_observer(od)
    d.run()
    assert np.array_equal(d.get_x(), want)


# ------------------------------------------------------------- 4. stacked forms
@pytest.mark.parametrize("iso", [False, True])
def test_weighted_sweep_is_stacked_and_every_member_has_its_own_runs_bits(nsol, iso):
    from nsol_amd import ops
    from nsol_amd.parameter_sweep import PrimalDualSweep
    shape = (12, 20, 24)
    obs = _obs(shape)
    w = mixed_weights(shape, 6)
    alphas, algs, iters = [0.02, 0.05, 0.11], ["ALG2", "ALG3"], ITERS
    for dtype in BOTH:
        t = _solver(obs, w, "TV", "L2", 0.05, iters, 16.0, "ALG2", dtype, iso=iso)
        sweep = PrimalDualSweep(prox_f=t._prox_f, prox_g_conj=t._prox_g_conj, B=t._B,
                                B_conj=t._B_conj, L2=16.0, x0=obs.flatten(),
                                parameters={"alpha": alphas, "alg_type": algs},
                                iterations=iters, x_scale=np.max(obs), dtype=dtype)
        counts = (ops.pd_sweep_launches(), ops.pd_batch_launches(),
                  ops.pd_weighted_launches())
        sweep.run()
        assert sweep.get_execution() == "stacked"
        assert (ops.pd_sweep_launches(), ops.pd_batch_launches()) == counts[:2]
        groups = -(-6 // sweep.get_group_size())
        assert ops.pd_weighted_launches() == counts[2] + groups * iters
        for k, member in enumerate(sweep.get_parameters()):
            s = _solver(obs, w, "TV", "L2", member["alpha"], iters, 16.0,
                        member["alg_type"], dtype, iso=iso)
            s.run()
            assert np.array_equal(sweep.get_x(k), s.get_x()), (k, member)


def _batch_members(shape, P, dtype, iso, weighted=None):
    solvers = []
    for m in range(P):
        obs = _obs(shape, 100 + m) * (1.0 + 0.25 * (m % 5))
        w = mixed_weights(shape, 200 + m)
        if weighted is not None and not weighted[m]:
            w = None
        solvers.append(dict(obs=obs, w=w, alpha=0.03 + 0.01 * (m % 7),
                            alg=("ALG2", "ALG3")[m % 2]))
    make = lambda c: _solver(c["obs"], c["w"], "TV", "L2", c["alpha"], ITERS, 12.0,
                             c["alg"], dtype, iso=iso)
    return solvers, make


@pytest.mark.parametrize("shape,P,dtypes", [((37, 50), 5, BOTH),
                                            ((8, 16, 64), 128, (np.float32,))])
@pytest.mark.parametrize("iso", [False, True])
def test_weighted_batch_is_stacked_and_every_member_has_its_own_runs_bits(
        nsol, shape, P, dtypes, iso):
    """Data, weights, x_scale (the member's own maximum) and alpha differ from member
    to member; 128 members of (8, 16, 64) push the stack to two rows per lane."""
    from nsol_amd import ops
    from nsol_amd.solver_batch import PrimalDualBatch
    for dtype in dtypes:
        cfg, make = _batch_members(shape, P, dtype, iso)
        solvers = [make(c) for c in cfg]
        counts = (ops.pd_sweep_launches(), ops.pd_batch_launches(),
                  ops.pd_weighted_launches())
        batch = PrimalDualBatch(solvers)
        batch.run()
        assert batch.get_execution() == ["stacked"] * P
        assert (ops.pd_sweep_launches(), ops.pd_batch_launches()) == counts[:2]
        groups = -(-P // batch.get_group_size())
        assert ops.pd_weighted_launches() == counts[2] + groups * ITERS
        check = range(P) if P <= 8 else (0, 1, 63, 64, 126, 127)
        for m in check:
            s = make(cfg[m])
            s.run()
            assert np.array_equal(solvers[m].get_x(), s.get_x()), m


def test_mixed_batch_forms_a_weighted_and_an_unweighted_stack(nsol):
    from nsol_amd import ops
    from nsol_amd.solver_batch import PrimalDualBatch
    shape, P = (37, 50), 6
    weighted = [True, False, True, False, True, False]
    cfg, make = _batch_members(shape, P, np.float32, False, weighted)
    solvers = [make(c) for c in cfg]
    counts = (ops.pd_batch_launches(), ops.pd_weighted_launches())
    batch = PrimalDualBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["stacked"] * P
    assert ops.pd_batch_launches() == counts[0] + ITERS
    assert ops.pd_weighted_launches() == counts[1] + ITERS
    assert sorted(sorted(idx) for idx, _ in batch._stacks) == [[0, 2, 4], [1, 3, 5]]
    for m in range(P):
        s = make(cfg[m])
        s.run()
        assert np.array_equal(solvers[m].get_x(), s.get_x()), m


# ------------------------------------------------------------------ 5. declines
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
def test_entries_without_a_weights_pointer_decline_the_weighted_bit(nsol, dtype):
    """nsol_pd_fused_iter, nsol_pd_fused2_iter, nsol_pd_fusedk_iter,
    nsol_pd_persist_run, nsol_pd_run, nsol_pd_run_pitched, nsol_pd_sweep_run and
    nsol_pd_batch_iter / _run return -2 with the bit set and write nothing."""
    import ctypes
    import torch
    from nsol_amd import _lib, ops
    from nsol_amd.device import stream_ptr
    dt = getattr(torch, dtype)
    suf = "f32" if dtype == "float32" else "f64"
    lib = _lib.load()
    shape = (16, 32, 512)                  # a shape all of them take without the bit
    w = (1.0, 1.0, 1.0)
    _lib.set_param("pdk_min_kvox", 0)
    for extra in (0, ops.PD_REG_HUBER, ops.PD_REG_ISOTROPIC, ops.PD_DATA_L1):
        flags = extra | ops.PD_DATA_WEIGHTED
        st = _state(shape, dt)

        def untouched(st=st, also=()):
            torch.cuda.synchronize()
            for k in ("xbar_out", "x_out", "p_out") + tuple(also):
                assert bool((st[k] == st["sent"]).all()), k
        rc = getattr(lib, "nsol_pd_fused_iter_" + suf)(
            st["xbar"].data_ptr(), st["xbar_out"].data_ptr(), st["x_out"].data_ptr(),
            st["bt"].data_ptr(), st["p"].data_ptr(), st["p_out"].data_ptr(), 3, 16, 32,
            512, 1.0, 1.0, 1.0, 0.3, 1.0, 0.3, 0.3, 1.0, flags, stream_ptr())
        assert rc == -2
        untouched()
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
        slot = ctypes.c_int(0)
        for name, pitch in (("nsol_pd_run_", None), ("nsol_pd_run_pitched_", 512)):
            args = [st["xbar_out"].data_ptr(), st["xbar_out"].data_ptr(),
                    st["x_out"].data_ptr(), None, st["bt"].data_ptr(),
                    st["p_out"].data_ptr(), st["p_out"].data_ptr(), 3, 16, 32, 512]
            if pitch is not None:
                args.append(pitch)
            args += [1.0, 1.0, 1.0, 30.0, sig.ctypes.data, sig.ctypes.data,
                     sig.ctypes.data, 20, 1, 0.05, flags, ctypes.addressof(slot),
                     stream_ptr()]
            assert getattr(lib, name + suf)(*args) == -2, name
            untouched()
        members = 3
        sw = _state(shape, dt, members)
        sched = np.full((members, 4), 0.3)
        counts = (ops.pd_sweep_launches(), ops.pd_batch_launches())
        x_before = sw["x"].clone()
        assert ops.pd_sweep_run(sw["xbar"], sw["xbar_out"], sw["x"], sw["bt"], sw["p"],
                                sw["p_out"], members, shape, w, np.full(members, 30.0),
                                sched, sched, sched, True, 0.05, flags) is None
        assert ops.pd_batch_run(sw["xbar"], sw["xbar_out"], sw["x"], sw["x"].clone(),
                                sw["p"], sw["p_out"], members, shape, w,
                                np.full(members, 30.0), sched, sched, sched, True, 0.05,
                                flags) is None
        tab = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        rc = getattr(lib, "nsol_pd_batch_iter_" + suf)(
            sw["xbar"].data_ptr(), sw["xbar_out"].data_ptr(), sw["x"].data_ptr(),
            sw["x"].data_ptr(), sw["p"].data_ptr(), sw["p_out"].data_ptr(), members, 3,
            16, 32, 512, 1.0, 1.0, 1.0, tab.data_ptr(), 0, flags, stream_ptr())
        assert rc == -2
        torch.cuda.synchronize()
        assert (ops.pd_sweep_launches(), ops.pd_batch_launches()) == counts
        assert torch.equal(sw["x"], x_before)
        assert bool((sw["xbar_out"] == sw["sent"]).all())
        assert bool((sw["p_out"] == sw["sent"]).all())


def test_weighted_entries_refuse_what_they_cannot_index(nsol):
    """Without the bit, with a member stride other than 0 or n: NSOL_EINVAL, nothing
    launched."""
    import torch
    from nsol_amd import ops
    shape = (4, 8, 16)
    st = _state(shape, torch.float32)
    wt = torch.ones_like(st["bt"])
    sig = np.full((1, 3), 0.3)
    before = ops.pd_weighted_launches()
    with pytest.raises(ValueError):
        ops.pd_weighted_run(st["xbar"], st["xbar_out"], st["x"], st["bt"], wt, st["p"],
                            st["p_out"], 1, shape, (1., 1., 1.), [30.0], sig, sig, sig,
                            True, 0.05, ops.PD_DATA_L2)
    with pytest.raises(ValueError):
        ops.pd_weighted_run(st["xbar"], st["xbar_out"], st["x"], st["bt"], wt[:-1],
                            st["p"], st["p_out"], 1, shape, (1., 1., 1.), [30.0], sig,
                            sig, sig, True, 0.05, ops.PD_DATA_WEIGHTED)
    torch.cuda.synchronize()
    assert ops.pd_weighted_launches() == before
    assert bool((st["xbar_out"] == st["sent"]).all())


def test_weighted_run_stays_off_the_persist_kernel(nsol):
    """64^3, 50 iterations: inside the range persist_pays accepts (the fixture
    leaves ops.PD_PERSIST on for tests with 'persist' in their name)."""
    from nsol_amd import ops
    assert ops.PD_PERSIST and ops.persist_pays((64, 64, 64), 50)
    shape = (64, 64, 64)
    obs = _obs(shape)
    w = mixed_weights(shape, 8)
    before = ops.pd_persist_launches()
    s = _solver(obs, w, "TV", "L2", 0.05, 50, 16.0, "ALG2", np.float32)
    s.run()
    assert s.get_execution() == "fused"
    assert ops.pd_persist_launches() == before and not ops._pending_runs
    a = _solver(obs, None, "TV", "L2", 0.05, 50, 16.0, "ALG2", np.float32)
    a.run()
    assert ops.pd_persist_launches() == before + 1      # the unweighted run does go


# ------------------------------------------------ 6. inpainting does what it says
def _objective(x, bt, w, shape, alpha):
    from oracle import nsol_oracle as orc
    g = orc.grad(np.asarray(x, np.float64).reshape(shape))
    parts = np.array_split(g, len(shape))
    s = parts[0] * parts[0]
    for a in range(1, len(shape)):
        s = s + parts[a] * parts[a]
    d = np.where(w == 0, 0.0, x - bt)
    return float(0.5 / alpha * np.sum(w * d * d) + np.sum(np.sqrt(s)))


def test_weighted_isotropic_tv_inpaints_a_masked_hole(nsol):
    """2-D 64 x 64 piecewise-constant image, an 8 x 8 hole in the mask, TV-l2,
    300 iterations, float64."""
    shape, alpha, iters = (64, 64), 0.05, 300
    img = np.full(shape, 0.3)
    img[:, 32:] = 0.9
    img[40:, :20] = 0.6
    rng = np.random.default_rng(12)
    obs = img + 0.03 * rng.standard_normal(shape)
    w = np.ones(shape)
    w[28:36, 28:36] = 0.0                           # across the vertical edge
    hole = (w == 0).reshape(-1)
    filled = obs.copy()
    filled[28:36, 28:36] = 5.0                      # what the file holds in the hole
    ref = pd_weighted_denoise(filled, w, shape, "TV", "L2", alpha, iters, 8.0, "ALG2",
                              iso=True, x_scale=1.0, x0=obs)
    s = _solver(filled, w, "TV", "L2", alpha, iters, 8.0, "ALG2", np.float64, iso=True,
                x_scale=1.0, x0=obs)
    s.run()
    x = s.get_x()
    bt, wf = filled.reshape(-1), w.reshape(-1)
    F, Fref = _objective(x, bt, wf, shape, alpha), _objective(ref, bt, wf, shape, alpha)
    F0 = _objective(obs.reshape(-1), bt, wf, shape, alpha)
    print("objective: run %.9g, restatement %.9g, observation %.9g" % (F, Fref, F0))
    assert abs(F - Fref) <= 1e-3 * Fref
    assert F < F0
    # the hole is filled from its surroundings, not from the file
    other = obs.copy()
    other[28:36, 28:36] = np.nan
    t = _solver(other, w, "TV", "L2", alpha, iters, 8.0, "ALG2", np.float64, iso=True,
                x_scale=1.0, x0=obs)
    t.run()
    assert np.array_equal(t.get_x(), x)
    assert np.all(x[hole] > 0.2) and np.all(x[hole] < 1.0)


# ---------------------------------------------------------------------- 7. CLI
@pytest.mark.parametrize("mode", ["plain", "isotropic", "alpha", "slice-wise"])
def test_run_denoising_cli_mask(tmp_path, golden, capsys, mode, nsol):
    from nsol_amd import nifti
    from nsol_amd.data_reader import DataReader
    from nsol_amd.application import run_denoising
    vol = golden("configs")["phantom64"][20:32, :32, :40].astype(np.float64)
    vol = vol + 0.02 * np.random.default_rng(1).standard_normal(vol.shape)
    mask = np.ones(vol.shape)
    mask[:, 10:16, 12:20] = 0
    mask[5] = 0                                     # a slice that is copied through
    nii, mnii = str(tmp_path / "vol.nii.gz"), str(tmp_path / "mask.nii.gz")
    nifti.write(nii, vol)
    nifti.write(mnii, mask)
    obs = DataReader(nii)
    obs.read_data()
    data = obs.get_data()
    weights = (mask > 0).astype(np.float64)
    out = str(tmp_path / "out.nii.gz")
    base = ["--observation", nii, "--mask", mnii, "--reconstruction-type", "TVL2",
            "--iterations", "10", "--dtype", "float32", "--L2", "12"]
    kw = dict(L2=12, dtype=np.float32)
    if mode in ("plain", "isotropic"):
        iso = mode == "isotropic"
        assert run_denoising.main(base + ["--result", out] +
                                  (["--isotropic"] if iso else [])) == 0
        assert "(fused)" in capsys.readouterr().out
        s = run_denoising.build_solver(data, "TVL2", 0.03, 10, weights=weights,
                                       isotropic=iso, **kw)
        s.run()
        got, _, _ = nifti.read(out)
        assert rel_l2(got, s.get_x().reshape(data.shape)) < 1e-6     # float32 file
    elif mode == "alpha":
        rdir = str(tmp_path / "members")
        os.makedirs(rdir)
        alphas = [0.02, 0.05]
        assert run_denoising.main(base + ["--result-dir", rdir, "--alpha"] +
                                  ["%g" % a for a in alphas]) == 0
        assert capsys.readouterr().out.count("(stacked)") == len(alphas)
        for a in alphas:
            got, _, _ = nifti.read(run_denoising.member_result_path(rdir, nii, a))
            s = run_denoising.build_solver(data, "TVL2", a, 10, weights=weights, **kw)
            s.run()
            assert rel_l2(got, s.get_x().reshape(data.shape)) < 1e-6
    else:
        assert run_denoising.main(base + ["--result", out, "--slice-wise"]) == 0
        assert "11 slices stacked, 1 copied through, 0 sequential" in \
            capsys.readouterr().out
        got, _, _ = nifti.read(out)
        for k in range(data.shape[0]):
            if k == 5:
                assert rel_l2(got[k], data[k]) < 1e-6
                continue
            s = run_denoising.build_solver(data[k], "TVL2", 0.03, 10,
                                           weights=weights[k], **kw)
            s.run()
            assert rel_l2(got[k], s.get_x().reshape(data[k].shape)) < 1e-6, k
