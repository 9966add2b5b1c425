"""CPU-only side of the isotropic primal-dual regulariser: the NumPy float64
restatement the GPU tests are held to (the oracle's Chambolle-Pock loop with the
per-voxel projection in the place of prox_tv_conj), its own checks, and the host
logic that recognises the new prox descriptors."""
import os
import re

import numpy as np
import pytest

# the projection itself is stated once, beside the rest of the kernels' arithmetic
# (the other test modules take it from here)
from nsol_amd.vector_numpy import project_iso    # noqa: F401

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ------------------------------------------------------------------ yardstick
def pd_iso_denoise(b, shape, reg="TV", data="L2", alpha=0.03, iterations=10,
                   L2=8., alg_type="ALG2", x_scale=None, spacing=None,
                   gamma=0.05, scaled=False):
    """oracle.nsol_oracle.primal_dual_denoise with project_iso in the place of
    prox_tv_conj / prox_huber_conj; nothing else differs.  scaled: return the
    iterate in the solver's units (x / x_scale)."""
    from oracle import nsol_oracle as orc
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x_scale = float(np.max(b)) if x_scale is None else float(x_scale)
    d = len(shape)
    lmbda = 1. / float(alpha)
    sig, ta, th = orc.pd_schedule(alg_type, L2, lmbda, iterations)
    x = b / x_scale
    xbar = x.copy()
    p = 0
    for n in range(iterations):
        q = p + sig[n] * orc.grad(xbar.reshape(shape), spacing).reshape(-1)
        p = project_iso(q, d, 1. + sig[n] * gamma if reg == "Huber" else None)
        Zshape = (d * shape[0],) + tuple(shape[1:]) if d > 1 else shape
        u = x - ta[n] * orc.grad_adj(p.reshape(Zshape), spacing).reshape(-1)
        if data == "L2":
            xn = orc.prox_ell2_denoising(u, ta[n] * lmbda, b, x_scale)
        else:
            xn = orc.prox_ell1_denoising(u, ta[n] * lmbda, b, x_scale)
        xbar = xn + th[n] * (xn - x)
        x = xn
    return x if scaled else x * x_scale


def disc_and_ramp(n=64, seed=7, noise=0.08):
    """A disc plus an edge at 30 degrees plus seeded Gaussian noise: oblique
    edges, where the two total variations part."""
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    c = (n - 1) / 2.0
    img = 0.2 + 0.6 * ((xx - 0.62 * n) ** 2 + (yy - 0.4 * n) ** 2 < (0.2 * n) ** 2)
    t = np.deg2rad(30.0)
    img = img + 0.5 * (np.cos(t) * (yy - c) - np.sin(t) * (xx - c) > 0.18 * n)
    rng = np.random.default_rng(seed)
    return img + noise * rng.standard_normal((n, n))


def tv_values(x, shape):
    """(isotropic, anisotropic) total variation of the flat image x."""
    from oracle import nsol_oracle as orc
    g = orc.grad(np.asarray(x, np.float64).reshape(shape))
    parts = np.array_split(g, len(shape))
    s = parts[0] * parts[0]
    for a in range(1, len(shape)):
        s = s + parts[a] * parts[a]
    return float(np.sum(np.sqrt(s))), float(np.sum(np.abs(g)))


# ------------------------------------------------------------------- its checks
@pytest.mark.parametrize("reg", ["TV", "Huber"])
@pytest.mark.parametrize("data", ["L2", "L1"])
@pytest.mark.parametrize("alg", ["ALG2", "ALG2_AHMOD", "ALG3"])
def test_restatement_is_the_oracle_loop_in_1d(reg, data, alg):
    """sqrt(q q) = |q| exactly, so in 1-D the isotropic loop is the oracle's
    anisotropic one, array for array."""
    from oracle import nsol_oracle as orc
    rng = np.random.default_rng(3)
    b = 50.0 + 30.0 * rng.standard_normal(257)
    alpha = 0.05 if data == "L2" else 0.6
    ours = pd_iso_denoise(b, (257,), reg, data, alpha, 25, 4.0, alg)
    ref = orc.primal_dual_denoise(b, (257,), reg, data, alpha, 25, 4.0, alg)
    assert np.array_equal(ours, ref)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_projection_is_moreau_complement_of_the_reference_shrinkage(d):
    """t - shrink(t, 1) is the projection of t onto the unit ball (Moreau);
    the shrinkage is the reference's own isotropic arithmetic
    (admm_linear_solver.py:239-253)."""
    from oracle import nsol_oracle as orc
    rng = np.random.default_rng(10 + d)
    t = 1.5 * rng.standard_normal(d * 4001)
    t[:7] = 0.0
    want = t - orc.admm_prox_g(t, 1.0, d)
    assert np.max(np.abs(project_iso(t, d) - want)) <= 1e-14


def test_isotropic_and_anisotropic_minimisers_part_on_oblique_edges():
    """The separation the GPU test relies on, on the CPU (2-D 64 x 64, TV-l2,
    alpha 0.03, 300 iterations, float64).  Observed: F_iso(x_aniso) - F_iso(x_iso)
    = 14.45 of 465.66 (3.1e-2 relative), F_aniso(x_iso) - F_aniso(x_aniso) = 19.19
    of 510.85 (3.8e-2 relative) -- ten orders above float64 rounding."""
    from oracle import nsol_oracle as orc
    img = disc_and_ramp()
    shape, alpha = img.shape, 0.03
    bt = img.reshape(-1) / img.max()
    xi = pd_iso_denoise(img.reshape(-1), shape, "TV", "L2", alpha, 300, 8.0, "ALG2",
                        scaled=True)
    xa = orc.primal_dual_denoise(img.reshape(-1), shape, "TV", "L2", alpha, 300, 8.0,
                                 "ALG2") / img.max()
    F = {}
    for name, x in (("iso", xi), ("aniso", xa)):
        fid = 0.5 * np.sum((x - bt) ** 2) / alpha
        ti, ta = tv_values(x, shape)
        F[name] = (fid + ti, fid + ta)
    gap_iso = F["aniso"][0] - F["iso"][0]
    gap_aniso = F["iso"][1] - F["aniso"][1]
    print("F_iso gap %.6g of %.6g, F_aniso gap %.6g of %.6g" %
          (gap_iso, F["iso"][0], gap_aniso, F["aniso"][1]))
    assert gap_iso > 1e-6 * F["iso"][0]
    assert gap_aniso > 1e-6 * F["aniso"][1]


# ------------------------------------------------------------------ host logic
def _wired(obs, data="L2", reg="TV", dimension=None, gamma=None):
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
    if data == "L2":
        pf = lambda x, tau: prox.prox_ell2_denoising(x, tau, x0=b, x_scale=3.)
    else:
        pf = lambda x, tau: prox.prox_ell1_denoising(x, tau, x0=b, x_scale=3.)
    dim = obs.ndim if dimension is None else dimension
    if reg == "Huber":
        kw = {} if gamma is None else {"gamma": gamma}
        pg = lambda x, s: prox.prox_huber_conj_isotropic(x, s, dim, **kw)
    else:
        pg = lambda x, s: prox.prox_tv_conj_isotropic(x, s, dim)
    return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=pg, B=D, B_conj=Da,
                               L2=16, x0=b, x_scale=3.)


def test_probe_descriptors_of_the_isotropic_proxes():
    from nsol_amd.proximal_operators import ProximalOperators as prox
    from nsol_amd.symbolic import Sym
    out = prox.prox_tv_conj_isotropic(Sym((24,)), 0.25, 3)
    assert isinstance(out, Sym) and out.shape == (24,)
    assert out.desc == ("prox_tv_conj_iso", 0.25, 3)
    out = prox.prox_huber_conj_isotropic(Sym((24,)), 0.25, 2, gamma=0.1)
    assert out.desc == ("prox_huber_conj_iso", 0.25, 0.1, 2)
    assert prox.prox_huber_conj_isotropic(Sym((24,)), 0.25, 2).desc[2] == 0.05
    for bad in (lambda: prox.prox_tv_conj_isotropic(Sym((25,)), 0.25, 3),
                lambda: prox.prox_huber_conj_isotropic(Sym((25,)), 0.25, 2),
                lambda: prox.prox_tv_conj_isotropic(np.zeros(25), 0.25, 3),
                lambda: prox.prox_tv_conj_isotropic(np.zeros(24), 0.25, 4)):
        with pytest.raises(ValueError):
            bad()


def test_plan_recognises_the_isotropic_descriptors():
    from nsol_amd import ops
    assert ops.PD_REG_ISOTROPIC == 4
    s = _wired(np.ones((4, 5, 6)), "L1", "Huber", gamma=0.125)
    dual = s._native_dual()
    assert dual["flags"] == ops.PD_REG_HUBER | ops.PD_REG_ISOTROPIC
    assert dual["gamma"] == 0.125 and dual["dim"] == 3
    plan = s.plan()
    assert plan["flags"] == ops.PD_REG_HUBER | ops.PD_REG_ISOTROPIC | ops.PD_DATA_L1
    assert plan["shape"] == (4, 5, 6)
    s = _wired(np.ones((7, 9)), "L2", "TV")
    assert s.plan()["flags"] == ops.PD_REG_ISOTROPIC and s.plan()["dim"] == 2
    assert s._native_dual()["gamma"] == 0.05
    s = _wired(np.ones(11), "L2", "TV")
    assert s.plan()["flags"] == ops.PD_REG_ISOTROPIC and s.plan()["dim"] == 1


def test_plan_refuses_a_dimension_other_than_the_gradients():
    # 4 x 6 x 6 voxels: a field of 3 blocks also splits into 2 -- the vector norm
    # would pair components of different voxels
    s = _wired(np.ones((4, 6, 6)), "L2", "TV", dimension=2)
    assert s._native_dual() is None and s.plan() is None
    s = _wired(np.ones((4, 6)), "L2", "Huber", dimension=1)
    assert s._native_dual() is None and s.plan() is None
    s = _wired(np.ones((4, 6)), "L2", "Huber", dimension=2)
    assert s.plan() is not None


def test_persistent_kernel_is_not_chosen_for_isotropic_plans(monkeypatch):
    """ops.pd_run must not try the persistent kernel (which declines) for an
    isotropic request: no workspace, no error-word slot, no pending-run record."""
    from nsol_amd import ops
    src = open(os.path.join(ROOT, "nsol_amd", "ops.py")).read()
    m = re.search(r"if PD_PERSIST and (.*?):\n", src, re.S)
    assert m and "PD_REG_ISOTROPIC" in m.group(1)
    assert ops.persist_pays((64, 64, 64), 50)      # the range the GPU test uses


def test_header_declares_the_isotropic_entries():
    from nsol_amd import _lib
    decl = _lib.declared_symbols()
    for base in ("prox_dual_project", "pd_dual_step_iso"):
        for suf in ("f32", "f64"):
            assert "nsol_%s_%s" % (base, suf) in decl
    assert len(decl["nsol_prox_dual_project_f64"][1]) == 6
    assert len(decl["nsol_pd_dual_step_iso_f32"][1]) == \
        len(decl["nsol_pd_dual_step_f32"][1])
    text = open(os.path.join(ROOT, "include", "nsol_hip.h")).read()
    assert re.search(r"#define\s+NSOL_PD_REG_ISOTROPIC\s+4\b", text)
    assert "admm_linear_solver.py:239-253" in text
    assert "prior_measures.py:27-52" in text
    from nsol_amd.build import SOURCES
    assert "nsol_pdi.hip" in SOURCES


def test_cli_build_solver_takes_isotropic_as_a_trailing_keyword():
    import inspect
    from nsol_amd import ops
    from nsol_amd.application import run_denoising, run_deconvolution
    for mod in (run_denoising, run_deconvolution):
        params = list(inspect.signature(mod.build_solver).parameters.values())
        assert params[-1].name == "isotropic" and params[-1].default is False
    obs = 10.0 + np.arange(6 * 8, dtype=float).reshape(6, 8)
    for rtype, reg in (("TVL1", ops.PD_REG_TV), ("TVL2", ops.PD_REG_TV),
                       ("HuberL1", ops.PD_REG_HUBER), ("HuberL2", ops.PD_REG_HUBER)):
        data = ops.PD_DATA_L1 if rtype.endswith("L1") else ops.PD_DATA_L2
        s = run_denoising.build_solver(obs, rtype, 0.03, 5, dtype=np.float64)
        assert s.plan()["flags"] == reg | data
        s = run_denoising.build_solver(obs, rtype, 0.03, 5, dtype=np.float64,
                                       isotropic=True)
        assert s.plan()["flags"] == reg | data | ops.PD_REG_ISOTROPIC
    s = run_deconvolution.build_solver(obs, np.ones(2), 1.2, "HuberL2", isotropic=True)
    assert s._native_dual()["flags"] == ops.PD_REG_HUBER | ops.PD_REG_ISOTROPIC
    s = run_deconvolution.build_solver(obs, np.ones(2), 1.2, "TVL2")
    assert s._native_dual()["flags"] == ops.PD_REG_TV
