"""The float64 restatement of the generic vector kernels (nsol_amd/vector_numpy.py)
against the CPU oracle (oracle/nsol_oracle.py) and the reference's golden vectors: the
reference of tests/test_vector_ops_gpu.py, anchored where it can run without a GPU.
Also the CPU side of that file's inputs: the share of elements on either side of every
branch, and the planted values."""
import math

import numpy as np
import pytest

import vector_cases as vc
from nsol_amd import vector_numpy as vn
from oracle import nsol_oracle as orc

SPACING = (0.8, 1.3, 2.0)           # spacing[0] belongs to the last array axis
SHAPES = [(1,), (5,), (259,), (5, 7), (6, 259), (1, 9), (9, 1),
          (3, 5, 7), (4, 6, 259), (2, 1, 5), (3, 5, 8), (5, 4, 64)]


def _w(d, spacing=SPACING):
    return [1. / spacing[a] if a < d else 1. for a in range(3)]


# ------------------------------------------------------------------------ goldens
def test_proxes_match_oracle_and_goldens(golden):
    g = golden("ops")
    v, b = g["prox_in"], g["prox_b"]
    bt = vn.scale(b, 50.0, divide=True)
    for got, name, want in (
            (vn.prox_dual_clamp(v, 1.0), "prox_tv_conj", orc.prox_tv_conj(v, 0.7)),
            (vn.prox_dual_clamp(v, 1. + 0.7 * 0.05), "prox_huber_conj",
             orc.prox_huber_conj(v, 0.7)),
            (vn.prox_ell1(v, bt, 0.3), "prox_ell1",
             orc.prox_ell1_denoising(v, 0.3, b, 50.0)),
            (vn.prox_ell2(v, bt, 0.3), "prox_ell2",
             orc.prox_ell2_denoising(v, 0.3, b, 50.0))):
        assert np.array_equal(got, want), name
        assert np.array_equal(got, g[name]), name


def test_losses_match_oracle_and_goldens(golden):
    g = golden("ops")
    f2 = g["loss_f2"]
    for name in vn.LOSSES:
        for fs in (1.0, 1.7):
            rho, drho = vn.loss_eval(name, f2, fs)
            assert np.array_equal(rho, orc.loss(name, f2, fs)), (name, fs)
            assert np.array_equal(drho, orc.gradient_loss(name, f2, fs)), (name, fs)
            assert np.allclose(rho, g["loss_%s_%g" % (name, fs)], rtol=1e-14, atol=0)
            assert np.allclose(drho, g["gradloss_%s_%g" % (name, fs)], rtol=1e-14,
                               atol=0)
    # Huber's gamma is a parameter: the prior's form of it (prior_measures.py:40-52)
    gm = 0.7
    rho, drho = vn.loss_eval("huber", f2, 1.0, gm)
    assert np.array_equal(rho, np.where(f2 < gm * gm, f2, 2. * gm * np.sqrt(f2) - gm * gm))
    assert np.any(f2 < gm * gm) and np.any(f2 > gm * gm)


def test_shrink_matches_oracle_and_golden(golden):
    g = golden("ops")
    got = vn.vector_shrink(g["shrink_in"], 3, 0.9)
    assert np.array_equal(got, g["shrink_out"])
    assert np.array_equal(got, orc.admm_prox_g(g["shrink_in"], 0.9, 3))
    for ndim in (1, 2, 3):
        t = vc.inputs("shrink%d" % ndim, 257, np.float64)["t"]
        for thr in (vc.THR, 0.):
            got = vn.vector_shrink(t, ndim, thr)
            assert np.all(np.isfinite(got))
            assert np.array_equal(got.reshape(-1),
                                  orc.admm_prox_g(t.reshape(-1), thr, ndim))
        # on the threshold and at the zero vector: 0
        got = vn.vector_shrink(t, ndim, vc.THR)
        assert not got[:, 0].any() and not got[:, 2].any() and not got[:, 3].any()
        assert got[0, 1] > 0.


@pytest.mark.parametrize("k", ["1d", "2d", "3d"])
@pytest.mark.parametrize("tag", ["unit", "sp"])
def test_differences_match_oracle_and_goldens(golden, k, tag):
    g = golden("ops")
    x, p = g["x_" + k], g["p_" + k]
    d = x.ndim
    sp = np.ones(d) if tag == "unit" else g["spacing_" + k]
    w = [1. / sp[a] if a < d else 1. for a in range(3)]
    pp = p.reshape((d,) + x.shape)
    got = vn.grad(x, w).reshape(p.shape)
    assert np.array_equal(got, g["grad_%s_%s" % (k, tag)])
    assert np.array_equal(got, orc.grad(x, sp))
    got = vn.grad_adj(pp, w)
    assert np.array_equal(got, orc.grad_adj(p, sp))
    assert np.allclose(got, g["gradadj_%s_%s" % (k, tag)], rtol=0, atol=1e-14)
    tau = 0.37
    assert np.array_equal(vn.grad_adj_axpy(pp, x, tau, w), x - tau * orc.grad_adj(p, sp))
    for a, nm in enumerate(["dx", "dy", "dz"][:d]):
        assert np.array_equal(vn.diff_axis(x, a, False, w[a]),
                              g["%s_%s_%s" % (nm, k, tag)])
        assert np.array_equal(vn.diff_axis(x, a, True, w[a]),
                              g["%sadj_%s_%s" % (nm, k, tag)])


# ------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("shape", SHAPES)
def test_stencils_match_the_oracle_and_are_adjoint(shape):
    rng = np.random.default_rng(5 + sum(shape))
    d = len(shape)
    x, p = rng.standard_normal(shape), rng.standard_normal((d,) + shape)
    y = rng.standard_normal(shape)
    sp, w = SPACING[:d], _w(d)
    flat = p.reshape((d * shape[0],) + shape[1:])
    assert np.array_equal(vn.grad(x, w).reshape(flat.shape), orc.grad(x, sp))
    assert np.array_equal(vn.grad_adj(p, w), orc.grad_adj(flat, sp))
    lhs = math.fsum((vn.grad(x, w) * p).reshape(-1))
    rhs = math.fsum((x * vn.grad_adj(p, w)).reshape(-1))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    x3 = x.reshape((1,) * (3 - d) + shape)
    y3 = y.reshape(x3.shape)
    for a in range(3):
        ax = 2 - a
        assert np.array_equal(vn.diff_axis(x3, a, False, 1.3),
                              orc.d_forward(x3, ax, 1. / 1.3))
        assert np.array_equal(vn.diff_axis(x3, a, True, 1.3),
                              orc.d_forward_adj(x3, ax, 1. / 1.3))
        lhs = math.fsum((vn.diff_axis(x3, a, False, 1.3) * y3).reshape(-1))
        rhs = math.fsum((x3 * vn.diff_axis(y3, a, True, 1.3)).reshape(-1))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-300)


def test_float32_weights_are_rounded_as_the_library_rounds_them():
    x = vc.normal(35, np.float32, 1).reshape(5, 7)
    w = _w(2)
    w32 = [float(np.float32(v)) for v in w]
    assert w32[1] != w[1]                       # (1 / 1.3; 1 / 0.8 is exact)
    assert np.array_equal(vn.grad(x, w, np.float32), vn.grad(x, w32))
    assert not np.array_equal(vn.grad(x, w, np.float32), vn.grad(x, w))
    p = np.stack([x, x[::-1]])
    assert np.array_equal(vn.grad_adj_axpy(p, x, 0.3, w, np.float32),
                          x - float(np.float32(0.3)) * vn.grad_adj(p, w32))


def test_reductions_match_oracle_measures():
    n = 1021
    x, y = vc.cancelling_pair(n, np.float64)
    terms = vn.dot_terms(x, y)
    assert abs(vn.dot(x, y)) < 0.05 * np.sum(np.abs(terms))      # heavy cancellation
    assert vn.dot(x, y) == pytest.approx(float(np.dot(x, y)), abs=1e-12 * np.sum(np.abs(terms)))
    assert vn.norm2(x) == pytest.approx(np.linalg.norm(x), rel=1e-14)
    mx, my = float(x.mean()), float(y.mean())
    st = vn.pair_stats(x, y, mx, my)
    assert st[3] == pytest.approx(orc.sim_sad(x, y), rel=1e-13)
    assert st[4] == pytest.approx(orc.sim_ssd(x, y), rel=1e-13)
    assert st[5] == np.max(y)
    assert st[6] == pytest.approx(np.sum(x), abs=1e-12 * np.sum(np.abs(x)))
    assert st[7] == pytest.approx(np.sum(y), abs=1e-12 * np.sum(np.abs(y)))
    ncc = st[0] / (n * np.sqrt(st[1] / (n - 1)) * np.sqrt(st[2] / (n - 1)))
    assert ncc == pytest.approx(orc.sim_ncc(x, y), rel=1e-12)
    for ndim in (1, 2, 3):
        t = vc.field(n, ndim, np.float64)
        ident = lambda u: u
        assert vn.vector_norm_sum(t, ndim, 0) == pytest.approx(
            orc.prior_tv(t.reshape(-1), ident, ndim), rel=1e-13)
        assert vn.vector_norm_sum(t, ndim, 1, vc.NORM_GAMMA) == pytest.approx(
            orc.prior_huber(t.reshape(-1), ident, ndim, vc.NORM_GAMMA), rel=1e-13)
    r, b = vc.residual_inputs(n, np.float64)
    for name in vn.LOSSES:
        cost, g = vn.loss_cost_grad(r, name, 1.7, minus=b)
        assert cost == pytest.approx(0.5 * np.sum(orc.loss(name, (r - b) ** 2, 1.7)),
                                     rel=1e-13)
        assert np.array_equal(g, orc.gradient_loss(name, (r - b) ** 2, 1.7) * (r - b))
        cost0, g0 = vn.loss_cost_grad(r, name, 1.7)
        assert np.array_equal(g0, orc.gradient_loss(name, r * r, 1.7) * r)


def test_elementwise_restatements_and_float32_scalars():
    n = 257
    v = vc.inputs("lincomb3", n, np.float32)
    x, y, z = v["x"], v["y"], v["z"]
    assert np.array_equal(vn.lincomb2(vc.A, x, vc.B, y), vc.A * x + vc.B * y)
    assert np.array_equal(vn.lincomb3(vc.A, x, vc.B, y, vc.C, z),
                          vc.A * x + vc.B * y + vc.C * z)
    a32 = float(np.float32(vc.A))
    assert np.array_equal(vn.lincomb2(vc.A, x, 1.0, y, np.float32), a32 * x + y)
    assert np.array_equal(vn.extrapolate(x, y, 0.9), x + 0.9 * (x - y))
    assert np.array_equal(vn.scale(x, 3.0, True), x / 3.0)
    assert np.array_equal(vn.clip(x, -np.inf, np.inf, np.float32), x)
    assert np.array_equal(vn.clip(x, vc.LO, vc.HI), np.clip(x, vc.LO, vc.HI))
    # float32: reciprocals formed in double on the host, rounded once
    tau = 0.3
    r32 = float(np.float32(1. / (1. + tau)))
    assert np.array_equal(vn.prox_ell2(x, y, tau, np.float32),
                          (x + float(np.float32(tau)) * y) * r32)
    d32 = float(np.float32(1. / vc.DEN))
    assert np.array_equal(vn.prox_dual_clamp(x, vc.DEN, np.float32),
                          np.clip(x * d32, -1., 1.))
    # ... and both stay within float32 rounding of the float64 forms
    assert np.allclose(vn.prox_ell2(x, y, tau, np.float32), vn.prox_ell2(x, y, tau),
                       rtol=0, atol=4 * vc.U32 * 3)
    assert np.allclose(vn.prox_dual_clamp(x, vc.DEN, np.float32),
                       vn.prox_dual_clamp(x, vc.DEN), rtol=0, atol=2 * vc.U32)


# ------------------------------------------------- the GPU tests' inputs, on the CPU
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_inputs_fall_on_both_sides_of_every_branch(dtype):
    for k, f in vc.branch_fractions(1021, dtype).items():
        assert 0.1 <= f <= 0.9, (k, f)
    # at the length that needs a second and a third trip as well
    for k, f in vc.branch_fractions(2 * 256 * 2 + 37, dtype).items():
        assert 0.1 <= f <= 0.9, (k, f)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_values_sit_on_the_branches(dtype):
    n = 257
    x = vc.inputs("clip", n, dtype)["x"]
    assert x[0] == vc.LO and x[1] == vc.HI and x[-1] == vc.LO and x[-2] == vc.HI
    assert x[2] < vc.LO < x[3] and x[4] < vc.HI < x[5]
    v = vc.inputs("prox_ell1", n, dtype)
    d = v["x"] - v["bt"]
    assert d[0] == vc.TAU1 and d[1] == -vc.TAU1 and d[2] == 0.
    assert d[3] > vc.TAU1 > d[4] and d[5] < -vc.TAU1
    got = vn.prox_ell1(v["x"], v["bt"], vc.TAU1, dtype)
    assert got[0] == got[1] == got[2] == got[4] == 0.25 and got[3] > 0.25 > got[5]
    for ndim in (1, 2, 3):
        t = vc.inputs("shrink%d" % ndim, n, dtype)["t"]
        nrm = np.sqrt(np.sum(t * t, axis=0))
        assert nrm[0] == vc.THR and nrm[1] > vc.THR > nrm[2] and nrm[3] == 0.
        assert nrm[-1] == vc.THR                        # ... and in the tail
    f2 = vc.inputs("loss_eval", n, dtype)["f2"]
    z = f2 / vc.c(vc.F_SCALE * vc.F_SCALE, dtype)
    assert z[0] == vc.GAMMA ** 2 and f2[1] == 0. and z[2] > vc.GAMMA ** 2 > z[3]
    for name in vn.LOSSES:
        rho, drho = vn.loss_eval(name, f2, vc.F_SCALE, vc.GAMMA, dtype)
        assert np.all(np.isfinite(rho)) and np.all(np.isfinite(drho))
        assert rho[1] == 0. and drho[1] == 1.
    r, b = vc.residual_inputs(n, dtype)
    assert r[0] == 0. and (r - b)[1] == 0. and (r - b)[0] == 0.


def test_bounds_dominate_the_float32_restatement_run_in_float32():
    """The derived R u S bounds against NumPy's own float32 arithmetic (correctly
    rounded, so well inside): a bound that a CPU float32 run already exceeds would be
    wrong before any kernel is measured against it."""
    n, dt = 1021, np.float32
    f = lambda a: np.asarray(a, dtype=np.float32)
    v = vc.inputs("lincomb3", n, dt)
    want, R, S = vc.expected("lincomb3", v, dt)
    got = f(vc.A) * f(v["x"]) + f(vc.B) * f(v["y"]) + f(vc.C) * f(v["z"])
    assert got.dtype == np.float32 and np.all(np.abs(got - want) <= R * vc.U32 * S)
    v = vc.inputs("shrink3", n, dt)
    want, R, S = vc.expected("shrink3", v, dt)
    t = f(v["t"])
    nrm = np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        got = np.where(nrm > f(vc.THR), (nrm - f(vc.THR)) * t / nrm, f(0))
    assert got.dtype == np.float32 and np.all(np.abs(got - want) <= R * vc.U32 * S)
    f2 = vc.inputs("loss_eval", n, dt)["f2"]
    for name in ("soft_l1", "huber"):
        want = vn.loss_eval(name, f2, vc.F_SCALE, vc.GAMMA, dt)
        S = vc.loss_S(name, f2, vc.F_SCALE, vc.GAMMA, dt)
        z = f(f2) / f(4.)
        if name == "soft_l1":
            q = np.sqrt(f(1) + z)
            got = f(2) * (q - f(1)) * f(4.), f(1) / q
        else:
            q = np.sqrt(z)
            gm = f(vc.GAMMA)
            with np.errstate(divide="ignore"):
                got = (np.where(z < gm * gm, z * f(4.), (f(2) * gm * q - gm * gm) * f(4.)),
                       np.where(z < gm * gm, f(1), gm / q))
        for k in range(2):
            assert got[k].dtype == np.float32
            assert np.all(np.abs(got[k] - want[k]) <= vc.LOSS_R[name][k] * vc.U32 * S[k])
