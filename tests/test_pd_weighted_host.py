"""CPU-only side of the weighted / masked data term of the primal-dual solver: the
NumPy float64 restatement the GPU tests are held to (the oracle's Chambolle-Pock
loop with per-voxel weights in the data prox), its own check, and the host logic:
the probe descriptors, the plan, the refusal of wrong weights, the stacking keys and
the command-line arguments."""
import os
import re

import numpy as np
import pytest

from nsol_amd import vector_numpy as vn
from test_pd_isotropic_host import project_iso

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ------------------------------------------------------------------ yardstick
def prox_weighted(u, tl, bt, w, data):
    """nsol_amd.vector_numpy.prox_data_w (the restatement of the kernels' helper) in the
    argument order of the loops here."""
    return vn.prox_data_w(u, bt, w, tl, data == "L1")


def pd_weighted_denoise(obs, weights, shape, reg, data, alpha, iters, L2, alg,
                        iso=False, spacing=None, x_scale=1., x0=None, scaled=False):
    """The reference loop (primal_dual_solver.py:232-261, as
    oracle.nsol_oracle.primal_dual_denoise states it) with prox_weighted as prox_f
    and, with iso, the per-voxel projection as the dual prox.  x0: the start, default
    the observation.  Returns x * x_scale (scaled: x)."""
    from oracle import nsol_oracle as orc
    b = np.asarray(obs, dtype=np.float64).reshape(-1)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    x_scale = float(x_scale)
    bt = b / x_scale
    start = b if x0 is None else np.asarray(x0, np.float64).reshape(-1)
    d = len(shape)
    lmbda = 1. / float(alpha)
    sig, ta, th = orc.pd_schedule(alg, L2, lmbda, iters)
    Zshape = (d * shape[0],) + tuple(shape[1:]) if d > 1 else shape
    x = start / x_scale
    xbar = x.copy()
    p = 0
    for n in range(iters):
        q = p + sig[n] * orc.grad(xbar.reshape(shape), spacing).reshape(-1)
        if iso:
            p = project_iso(q, d, 1. + sig[n] * 0.05 if reg == "Huber" else None)
        else:
            p = orc.prox_huber_conj(q, sig[n]) if reg == "Huber" else \
                orc.prox_tv_conj(q, sig[n])
        u = x - ta[n] * orc.grad_adj(p.reshape(Zshape), spacing).reshape(-1)
        xn = prox_weighted(u, ta[n] * lmbda, bt, w, data)
        xbar = xn + th[n] * (xn - x)
        x = xn
    return x if scaled else x * x_scale


def mixed_weights(shape, seed=0):
    """About 30 % exact zeros -- among them one whole row, one whole plane (where
    the shape has them) and the first and last voxel -- ones, and values in (0, 3]."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    kind = rng.random(n)
    w = np.where(kind < 0.3, 0.0, np.where(kind < 0.6, 1.0,
                                           3.0 - 3.0 * rng.random(n)))
    w = w.reshape(shape)
    if len(shape) >= 2:
        w[..., shape[-2] // 2, :] = 0.0            # a whole row (of every plane)
    if len(shape) == 3:
        w[shape[0] // 2] = 0.0                     # a whole plane
    w.reshape(-1)[0] = 0.0
    w.reshape(-1)[-1] = 0.0
    assert np.all(w >= 0) and np.all(w <= 3)
    return w


# ------------------------------------------------------------------- its check
@pytest.mark.parametrize("reg", ["TV", "Huber"])
@pytest.mark.parametrize("data", ["L2", "L1"])
@pytest.mark.parametrize("alg", ["ALG2", "ALG2_AHMOD", "ALG3"])
@pytest.mark.parametrize("shape", [(257,), (13, 17), (5, 6, 7)])
def test_restatement_with_unit_weights_is_the_oracle_loop(reg, data, alg, shape):
    from oracle import nsol_oracle as orc
    rng = np.random.default_rng(3)
    b = 50.0 + 30.0 * rng.standard_normal(int(np.prod(shape)))
    alpha = 0.05 if data == "L2" else 0.6
    xs = float(np.max(b))
    ours = pd_weighted_denoise(b, np.ones(b.size), shape, reg, data, alpha, 25, 12.0,
                               alg, x_scale=xs)
    ref = orc.primal_dual_denoise(b, shape, reg, data, alpha, 25, 12.0, alg)
    err = np.linalg.norm(ours - ref) / np.linalg.norm(ref)
    assert err <= 1e-12, err


def test_restatement_ignores_the_observation_where_the_weight_is_zero():
    rng = np.random.default_rng(5)
    shape = (9, 11)
    b = 1.0 + rng.random(99)
    w = mixed_weights(shape, 1).reshape(-1)
    junk = b.copy()
    junk[w == 0] = np.nan
    for data in ("L2", "L1"):
        a = pd_weighted_denoise(b, w, shape, "TV", data, 0.1, 20, 8.0, "ALG2")
        c = pd_weighted_denoise(junk, w, shape, "TV", data, 0.1, 20, 8.0, "ALG2", x0=b)
        assert np.array_equal(a, c) and np.all(np.isfinite(a))


# ------------------------------------------------------------------ host logic
def _wired(obs, weights, data="L2", reg="TV", iso=False, alpha=0.05):
    import nsol_amd.linear_operators as LO
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd.proximal_operators import ProximalOperators as prox
    from nsol_amd.symbolic import Sym
    lo = {1: LO.LinearOperators1D, 2: LO.LinearOperators2D,
          3: LO.LinearOperators3D}[obs.ndim]()
    grad, grad_adj = lo.get_gradient_operators()
    X = obs.shape
    Z = grad(Sym(X)).shape
    b = obs.flatten()
    D = lambda x: grad(x.reshape(*X)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    if weights is None:
        pf = lambda x, tau: prox.prox_ell2_denoising(x, tau, x0=b, x_scale=3.)
    elif data == "L2":
        pf = lambda x, tau: prox.prox_ell2_denoising_weighted(
            x, tau, x0=b, weights=weights, x_scale=3.)
    else:
        pf = lambda x, tau: prox.prox_ell1_denoising_weighted(
            x, tau, x0=b, weights=weights, x_scale=3.)
    if iso:
        pg = lambda x, s: prox.prox_tv_conj_isotropic(x, s, obs.ndim)
    else:
        pg = prox.prox_huber_conj if reg == "Huber" else prox.prox_tv_conj
    return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=pg, B=D, B_conj=Da, L2=16,
                               x0=b, x_scale=3., alpha=alpha, iterations=7,
                               dtype=np.float64)


def test_probe_descriptors_of_the_weighted_proxes():
    from nsol_amd.proximal_operators import ProximalOperators as prox
    from nsol_amd.symbolic import Sym
    b, w = np.arange(24.0), np.ones(24, dtype=bool)
    out = prox.prox_ell2_denoising_weighted(Sym((24,)), 0.25, b, w, x_scale=2)
    assert isinstance(out, Sym) and out.shape == (24,)
    assert out.desc[0] == "prox_ell2_w" and out.desc[1] is b
    assert out.desc[2:4] == (2.0, 0.25) and out.desc[4] is w
    out = prox.prox_ell1_denoising_weighted(Sym((24,)), 0.25, b, w)
    assert out.desc[0] == "prox_ell1_w" and out.desc[2] == 1.0 and out.desc[4] is w


def test_plan_carries_the_bit_and_the_weights_through_caller_lambdas():
    from nsol_amd import ops
    assert ops.PD_DATA_WEIGHTED == 8
    w = mixed_weights((4, 5, 6), 2)
    s = _wired(np.ones((4, 5, 6)), w.reshape(-1), "L1", "Huber")
    plan = s.plan()
    assert plan["flags"] == ops.PD_REG_HUBER | ops.PD_DATA_L1 | ops.PD_DATA_WEIGHTED
    assert plan["weights"].shape == (120,) and np.array_equal(plan["weights"], w.ravel())
    assert plan["shape"] == (4, 5, 6) and plan["data_scale"] == 3.0
    mask = (w > 0).reshape(-1)                     # a bool mask is a weight array
    s = _wired(np.ones((4, 5, 6)), mask, "L2", "TV", iso=True)
    plan = s.plan()
    assert plan["flags"] == ops.PD_REG_ISOTROPIC | ops.PD_DATA_WEIGHTED
    assert plan["weights"] is mask
    plain = _wired(np.ones((4, 5, 6)), None).plan()
    assert "weights" not in plain and not plain["flags"] & ops.PD_DATA_WEIGHTED


@pytest.mark.parametrize("bad", ["negative", "nan", "inf", "size", "complex"])
def test_wrong_weights_raise_instead_of_falling_back(bad):
    from nsol_amd.proximal_operators import check_weights
    w = np.ones(30)
    if bad == "negative":
        w[7] = -1e-9
    elif bad == "nan":
        w[7] = np.nan
    elif bad == "inf":
        w[7] = np.inf
    elif bad == "size":
        w = np.ones(29)
    else:
        w = np.ones(30, dtype=np.complex128)
    with pytest.raises(ValueError):
        check_weights(w, 30)
    # plan() is where a solver first sees them: an error, not None (the generic loop)
    with pytest.raises(ValueError):
        _wired(np.ones((5, 6)), w).plan()
    check_weights(np.ones(30, dtype=np.int16), 30)
    check_weights(np.zeros(30, dtype=bool), 30)
    check_weights(np.zeros(30, dtype=np.float32), 30)


def test_batch_key_separates_weighted_from_unweighted_solvers():
    from nsol_amd.solver_batch import member_key, plan_stacks
    obs = 1.0 + np.arange(30.0).reshape(5, 6)
    w = np.ones(30)
    solvers = [_wired(obs, w), _wired(obs, None), _wired(obs, w * 2),
               _wired(obs, None), _wired(obs, w, data="L1")]
    keys = [member_key(s, s.plan()) for s in solvers]
    assert keys[0] == keys[2] and keys[1] == keys[3]
    assert keys[0] != keys[1] and keys[4] not in (keys[0], keys[1])
    assert plan_stacks(keys) == [[0, 2], [1, 3]]


def test_sweep_takes_the_weighted_entry_for_a_weighted_plan():
    src = open(os.path.join(ROOT, "nsol_amd", "parameter_sweep.py")).read()
    assert "pd_weighted_run" in src and "PD_DATA_WEIGHTED" in src
    from nsol_amd import ops
    # a sweep shares its weights: the group size is the unweighted sweep's; a stack
    # of images counts the member's own weights
    assert ops.weighted_batch_group_size(1000, 1 << 16, 2, 4) < \
        ops.batch_group_size(1000, 1 << 16, 2, 4)
    assert ops.weighted_batch_group_size(3, 100, 2, 4) == 3


def test_header_declares_the_weighted_entries():
    from nsol_amd import _lib
    decl = _lib.declared_symbols()
    for base in ("prox_ell2_weighted", "prox_ell1_weighted", "pd_weighted_iter",
                 "pd_weighted_run", "pd_weighted_table"):
        for suf in ("f32", "f64"):
            assert "nsol_%s_%s" % (base, suf) in decl
    assert "nsol_pd_weighted_launches" in decl
    assert len(decl["nsol_prox_ell2_weighted_f32"][1]) == 7
    # bt_stride, wt, wt_stride on top of the image stack's arguments
    assert len(decl["nsol_pd_weighted_run_f64"][1]) == \
        len(decl["nsol_pd_batch_run_f64"][1]) + 3
    text = open(os.path.join(ROOT, "include", "nsol_hip.h")).read()
    assert re.search(r"#define\s+NSOL_PD_DATA_WEIGHTED\s+8\b", text)
    from nsol_amd.build import SOURCES
    assert "nsol_pdw.hip" in SOURCES


def test_every_flagged_entry_without_weights_declines_the_bit_in_the_source():
    """The GPU test calls them; here: each unit that takes flags names the bit."""
    for unit in ("nsol_pd.hip", "nsol_pd2.hip", "nsol_pdk.hip", "nsol_pdp.hip",
                 "nsol_pds.hip", "nsol_pdb.hip"):
        src = open(os.path.join(ROOT, "nsol_amd", "csrc", unit)).read()
        assert "NSOL_PD_DATA_WEIGHTED" in src, unit


# ------------------------------------------------------------------------- CLI
def test_cli_mask_and_weights_exclude_each_other(capsys):
    from nsol_amd.application import run_denoising
    with pytest.raises(SystemExit) as e:
        run_denoising.main(["--observation", "o.nii.gz", "--result", "r.nii.gz",
                            "--mask", "m.nii.gz", "--weights", "w.nii.gz"])
    assert e.value.code == 2
    assert "not allowed with" in capsys.readouterr().err


@pytest.mark.parametrize("opt", ["--mask", "--weights"])
def test_cli_deconvolution_refuses_mask_and_weights(capsys, opt):
    from nsol_amd.application import run_deconvolution
    with pytest.raises(SystemExit) as e:
        run_deconvolution.main(["--observation", "o.nii.gz", "--result", "r.nii.gz",
                                opt, "m.nii.gz"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "run_denoising" in err and "operator A" in err


def test_cli_wiring_takes_weights_and_scales_by_the_voxels_that_count():
    from nsol_amd import ops
    from nsol_amd.application import run_denoising
    obs = 10.0 + np.arange(6 * 8, dtype=float).reshape(6, 8)
    w = np.ones((6, 8))
    w[-1] = 0
    junk = obs.copy()
    junk[-1] = np.nan
    for rtype in ("TVL1", "TVL2", "HuberL1", "HuberL2"):
        for iso in (False, True):
            s = run_denoising.build_solver(junk, rtype, 0.03, 5, dtype=np.float64,
                                           weights=w, isotropic=iso)
            plan = s.plan()
            assert plan["flags"] & ops.PD_DATA_WEIGHTED
            assert bool(plan["flags"] & ops.PD_REG_ISOTROPIC) == iso
            assert bool(plan["flags"] & ops.PD_DATA_L1) == rtype.endswith("L1")
            assert plan["data_scale"] == float(np.max(obs[:-1]))
            assert np.all(np.isfinite(s._x0_host))
    with pytest.raises(ValueError):
        run_denoising.wiring(obs, "TVL2", weights=np.ones((6, 7)))
    # a slice without a voxel that counts is copied through
    vol = np.stack([obs, obs, obs])
    wv = np.ones(vol.shape)
    wv[1] = 0
    assert run_denoising.classify_slices(vol, wv) == ([0, 2], [1])
    assert run_denoising.classify_slices(vol) == ([0, 1, 2], [])
