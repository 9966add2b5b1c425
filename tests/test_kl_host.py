"""CPU-only side of the Poisson (Kullback-Leibler) data term: the two closed-form proxes
of nsol_amd/vector_numpy.py (kl_dual_prox, prox_kl) on a stress vector that tells the
branched forms from the one-line ones, their reductions and edge values, the restated
iteration against SciPy's L-BFGS-B, and the host logic -- arguments, member keys, the
command line and the declared symbols."""
import numpy as np
import pytest

from nsol_amd import vector_numpy as vn
from kl_cases import (KL_BACKGROUND, dual_one_line, dual_scaled_error, kl_convergence_case,
                      kl_minimiser_of, pd_linear_kl_restatement, primal_one_line,
                      relative_error, stress_vector)
from test_pd_linear_host import gaussian_kernel, rel

F32_TOL = 1e-5


@pytest.fixture(scope="module")
def stress():
    return stress_vector()


def _f64(s):
    return {k: a.astype(np.float64) for k, a in s.items()}


# ------------------------------------------------------------------ the stress vector
def test_the_stress_vector_is_what_the_issue_describes(stress):
    s = stress
    assert all(a.dtype == np.float32 and a.size == 200000 for a in s.values())
    assert 1e-3 * 0.999 <= s["c"].min() and s["c"].max() <= 1e3 * 1.001
    assert 1e-2 * 0.999 <= s["sigma"].min() and s["sigma"].max() <= 1e1 * 1.001
    assert np.sum(s["bt"] == 0) == 20000 and s["bt"].max() <= 1e4 * 1.001
    assert s["bt"][s["bt"] > 0].min() >= 1e-4 * 0.999
    for k in ("v", "u"):
        ratio = np.abs(s[k].astype(np.float64)) / s["c"]
        assert 1e-3 * 0.99 <= ratio.min() and ratio.max() <= 1e6 * 1.01
        assert 0.4 < np.mean(s[k] < 0) < 0.6


def test_float32_dual_prox_is_within_the_gate_and_the_one_line_form_is_not(stress):
    s, d = stress, _f64(stress)
    ref = vn.kl_dual_prox(d["v"], d["c"], d["sigma"], d["bt"])
    got = vn.kl_dual_prox(s["v"], s["c"], s["sigma"], s["bt"])
    assert got.dtype == np.float32 and ref.dtype == np.float64
    err = dual_scaled_error(got, ref, d["c"])
    one = dual_scaled_error(dual_one_line(s["v"], s["c"], s["sigma"], s["bt"]), ref,
                            d["c"])
    print("dual prox float32: branched %.3g, one-line %.3g" % (err, one))
    assert err <= F32_TOL, err
    assert one > F32_TOL, one          # the vector tells the two forms apart
    # in float64 the two forms are the same number
    assert dual_scaled_error(dual_one_line(d["v"], d["c"], d["sigma"], d["bt"]), ref,
                             d["c"]) <= 1e-8


def test_float32_primal_prox_is_within_the_gate_and_the_one_line_form_is_not(stress):
    s, d = stress, _f64(stress)
    t32, t64 = s["c"] / s["sigma"], None
    t64 = t32.astype(np.float64)                   # the same float32-rounded t
    ref = vn.prox_kl(d["u"], d["bt"], t64)
    got = vn.prox_kl(s["u"], s["bt"], t32)
    assert got.dtype == np.float32
    err = relative_error(got, ref)
    wrong = primal_one_line(s["u"], s["bt"], t32).astype(np.float64)
    ok = ref != 0
    one = float(np.max(np.abs(wrong[ok] - ref[ok]) / np.abs(ref[ok])))
    print("primal prox float32: branched %.3g, one-line %.3g" % (err, one))
    assert err <= F32_TOL, err
    assert one > F32_TOL, one


def test_moreau_identity(stress):
    d = _f64(stress)
    v, c, sg, bt = d["v"], d["c"], d["sigma"], d["bt"]
    lhs = vn.kl_dual_prox(v, c, sg, bt)
    rhs = v - sg * vn.prox_kl(v / sg, bt, c / sg)
    err = dual_scaled_error(rhs, lhs, c)
    print("Moreau identity, scaled by max(|q|, c): %.3g" % err)
    # (v - sigma x cancels where v >> c: float64 keeps 1e-16 |v| <= 1e-10 c of it)
    assert err <= 1e-8, err


# ------------------------------------------------------- reductions and edge values
def test_reductions_and_edge_values(stress):
    d = _f64(stress)
    v, u, c, sg, bt = d["v"], d["u"], d["c"], d["sigma"], d["bt"]
    t = c / sg
    zero = bt == 0
    q = vn.kl_dual_prox(v, c, sg, bt)
    x = vn.prox_kl(u, bt, t)
    assert np.array_equal(q[zero], np.minimum(v, c)[zero])
    assert np.array_equal(x[zero], np.maximum(u - t, 0.)[zero])
    assert np.all(q <= c) and np.all(x >= 0)
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(x))
    for s in (stress,):          # float32 as well
        q32 = vn.kl_dual_prox(s["v"], s["c"], s["sigma"], s["bt"])
        x32 = vn.prox_kl(s["u"], s["bt"], s["c"] / s["sigma"])
        assert np.all(q32 <= s["c"]) and np.all(x32 >= 0)
        assert np.all(np.isfinite(q32)) and np.all(np.isfinite(x32))
    # weight 0 over NaN: +0 and u itself
    w = np.ones_like(v)
    w[::3] = 0.
    junk = bt.copy()
    junk[::3] = np.nan
    qw = vn.kl_dual_prox(v, c * w, sg, junk, w)
    xw = vn.prox_kl(u, junk, t * w, w)
    assert np.all(qw[::3] == 0) and not np.any(np.signbit(qw[::3]))
    assert np.array_equal(xw[::3], u[::3])
    keep = w > 0
    assert np.array_equal(qw[keep], q[keep]) and np.array_equal(xw[keep], x[keep])
    # the composed restatements: t = None with q holding q + sigma A xbar, a background
    qq, tt = v[:64], u[:64]
    a = vn.pdl_dual_data_kl(qq, tt, bt[:64], w[:64], 0.3, 20., 0.25)
    b = vn.pdl_dual_data_kl(qq + 0.3 * tt, None, bt[:64], w[:64], 0.3, 20., 0.25)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-12)
    assert np.array_equal(a, vn.kl_dual_prox(qq + 0.3 * (tt + 0.25), 20. * w[:64], 0.3,
                                              bt[:64], w[:64]))
    assert np.array_equal(vn.prox_kl_w(u[:64], bt[:64], None, 0.7),
                          vn.prox_kl(u[:64], bt[:64], np.full(64, 0.7)))


def test_the_proxes_minimise_what_they_stand_for():
    """x = prox_kl(u) zeroes the derivative of t (x - bt log x) + (x - u)^2 / 2, and
    q = kl_dual_prox(v) that of the conjugate's prox, q = v - sigma x(v / sigma)."""
    rng = np.random.default_rng(3)
    u = rng.uniform(-5., 5., 1000)
    bt = rng.uniform(0.1, 10., 1000)
    t = rng.uniform(0.01, 5., 1000)
    x = vn.prox_kl(u, bt, t)
    assert np.all(x > 0)
    assert np.max(np.abs(t * (1. - bt / x) + (x - u))) <= 1e-10


# ------------------------------------------------------------------ convergence
@pytest.mark.parametrize("mixed, iters", [(False, 4000), (True, 8000)])
def test_restatement_reaches_the_kl_minimiser(mixed, iters):
    """The 24 x 20 block image under Poisson noise, alpha = 0.05, anisotropic Huber with
    gamma = 0.05, x >= 0, background 2: relative L2 distance of the restated iteration
    to SciPy's L-BFGS-B minimiser of the same energy.  Reached by the committed
    restatement: 4.1e-7 after 4 000 iterations with all weights 1, 1.1e-7 after 8 000
    with rows 7-8 of weight 0 over NaN and column 15 of weight 2.5 (L-BFGS-B's own
    floor is of that order)."""
    obs, kernel, shape, w, s = kl_convergence_case(mixed)
    start = np.where(np.isfinite(obs), obs, 0.)
    x = pd_linear_kl_restatement(obs, kernel, shape, "huber", 0.05, iters,
                                 weights=w if mixed else None, bounds=(0., np.inf),
                                 x_scale=s, background=KL_BACKGROUND, x0=start)
    assert np.all(np.isfinite(x)) and np.all(x >= 0)
    err = rel(x, kl_minimiser_of(mixed))
    print("mixed weights" if mixed else "all weights 1", iters,
          "iterations: rel. l2 to the L-BFGS-B minimiser", err)
    assert err <= 1e-5, err


# ------------------------------------------------------------------ host logic
def _solver(cls=None, **kw):
    import nsol_amd
    from nsol_amd.linear_operators import ConvolutionOperator
    shape = (6, 8)
    A = ConvolutionOperator(2, gaussian_kernel(2, 1.))
    obs = 1. + np.arange(48, dtype=float)
    A1 = lambda x: A(x.reshape(*shape)).flatten()
    args = dict(A=A1, A_adj=A1, b=obs, x0=obs, dimension=2, data_loss="kl")
    args.update(kw)
    return (cls or nsol_amd.PrimalDualLinearSolver)(**args)


def _classes():
    import nsol_amd
    from nsol_amd.tgv_solver import TGVPrimalDualLinearSolver
    return [nsol_amd.PrimalDualLinearSolver, TGVPrimalDualLinearSolver]


def test_kl_is_a_data_loss_with_a_background():
    from nsol_amd import primal_dual_linear_solver as pdl, tgv_numpy
    assert "kl" in pdl.DATA_LOSSES and "kl" in tgv_numpy.DATA_LOSSES
    for cls in _classes():
        s = _solver(cls)
        assert s.get_data_loss() == "kl" and s.get_background() == 0.
        s = _solver(cls, background=1.5, x_scale=3.)
        assert s.get_background() == 1.5 and s._scaled_background() == 0.5
        assert _solver(cls, data_loss="ell2").get_background() == 0.
        assert _solver(cls, data_loss="ell1", background=0.).get_background() == 0.


@pytest.mark.parametrize("kw", [
    dict(background=-1.), dict(background=np.nan), dict(background=np.inf),
    dict(background="much"), dict(background=1., data_loss="ell2"),
    dict(background=0.5, data_loss="ell1"),
    dict(b=np.r_[-1., np.ones(47)]), dict(b=np.r_[np.nan, np.ones(47)]),
    dict(b=np.r_[-1., np.ones(47)], weights=np.ones(48)),
    dict(b=np.r_[np.nan, np.ones(47)], weights=np.r_[0.5, np.zeros(47)])])
def test_bad_arguments_raise(kw):
    for cls in _classes():
        with pytest.raises(ValueError):
            _solver(cls, **kw)


def test_what_weight_zero_hides_is_accepted():
    w = np.r_[0., 0., np.ones(46)]
    b = np.r_[np.nan, -3., np.ones(46)]
    for cls in _classes():
        _solver(cls, b=b, weights=w, x0=np.ones(48))
        # the other data terms take negative observations, as before
        _solver(cls, b=-np.ones(48), data_loss="ell2")
    import nsol_amd
    nsol_amd.TGVPrimalDualSolver(b=b.reshape(6, 8), x0=np.ones(48), dimension=2,
                                 data_loss="kl", weights=w)
    with pytest.raises(ValueError):
        nsol_amd.TGVPrimalDualSolver(b=b.reshape(6, 8), x0=np.ones(48), dimension=2,
                                     data_loss="kl")
    with pytest.raises(ValueError):
        nsol_amd.TGVPrimalDualSolver(b=b.reshape(6, 8), x0=np.ones(48), dimension=2,
                                     data_loss="huber")


def test_member_keys_separate_the_background_and_the_data_loss():
    from nsol_amd import linear_stack, tgv_linear_stack
    from nsol_amd.solver_batch import plan_stacks
    for cls, key in zip(_classes(), (linear_stack.member_key,
                                     tgv_linear_stack.member_key)):
        kl = [_solver(cls, alpha=a) for a in (0.01, 0.02)]
        keys = [key(s) for s in kl]
        assert keys[0] is not None and keys[0] == keys[1]
        other = key(_solver(cls, background=0.5))
        ell2 = key(_solver(cls, data_loss="ell2"))
        assert other is not None and ell2 is not None
        assert other != keys[0] and ell2 != keys[0] and ell2 != other
        # the kernel sees background / x_scale: equal scaled backgrounds share a group
        assert key(_solver(cls, background=1., x_scale=2.)) == other
        assert key(_solver(cls, background=1., x_scale=4.)) != other
        solvers = kl + [_solver(cls, background=0.5), _solver(cls, data_loss="ell2"),
                        _solver(cls, background=0.5, alpha=0.3),
                        _solver(cls, data_loss="ell2", alpha=0.3)]
        stacks = sorted(sorted(idx) for idx in plan_stacks([key(s) for s in solvers]))
        assert stacks == [[0, 1], [2, 4], [3, 5]]


def test_tgv_denoising_stacks_run_kl_members_on_their_own():
    import nsol_amd
    from nsol_amd import tgv_stack
    from nsol_amd.solver_batch import plan_stacks
    b = 1. + np.arange(48, dtype=float).reshape(6, 8)

    def make(loss, **kw):
        return nsol_amd.TGVPrimalDualSolver(b=b, x0=b.flatten(), dimension=2,
                                            data_loss=loss, **kw)
    assert tgv_stack.member_key(make("ell2")) is not None
    assert tgv_stack.member_key(make("ell1")) is not None
    assert tgv_stack.member_key(make("kl")) is None
    assert tgv_stack.member_key(make("kl", weights=np.ones(48))) is None
    solvers = [make("kl"), make("ell2"), make("kl", alpha=0.2), make("ell2", alpha=0.2)]
    assert [sorted(i) for i in
            plan_stacks([tgv_stack.member_key(s) for s in solvers])] == [[1, 3]]
    batch = tgv_stack.TGVPrimalDualBatch(solvers)
    assert [sorted(idx) for idx, _ in batch._stacks_to_try()] == [[1, 3]]
    sweep = tgv_stack.TGVPrimalDualSweep(b, b.flatten(), 2, {"alpha": [0.1, 0.2]},
                                         data_loss="kl")
    assert sweep._stack_form(sweep._solver(sweep._members[0])) is None
    ell2 = tgv_stack.TGVPrimalDualSweep(b, b.flatten(), 2, {"alpha": [0.1, 0.2]})
    assert ell2._stack_form(ell2._solver(ell2._members[0])) is not None
    # a kl template never reaches the stacked kernels, whoever calls the runner
    with pytest.raises(ValueError, match="kl"):
        tgv_stack.run_tgv_stack(None, None, None, False, make("kl"), [0.1], [2.], 1, None)


def test_tgv_numpy_takes_the_kl_data_loss():
    """One step of tgv_numpy with "kl" is the step with the prox swapped; w and wbar do
    not depend on the data term."""
    from nsol_amd import tgv_numpy
    rng = np.random.default_rng(1)
    shape = (5, 6)
    b = rng.poisson(20., shape).astype(float) / 30.
    x = rng.uniform(0.1, 1., shape)
    w = rng.standard_normal((2,) + shape)
    p = rng.uniform(-1, 1, (2,) + shape)
    q = rng.uniform(-1, 1, (3,) + shape)
    wt = rng.uniform(0., 2., shape)
    wt[1] = 0.
    xk, xbk, wk, wbk = tgv_numpy.primal_step(p, q, x, w, b, 0.3, 0.7, data_loss="kl")
    x2, _, w2, wb2 = tgv_numpy.primal_step(p, q, x, w, b, 0.3, 0.7, data_loss="ell2")
    assert np.array_equal(wk, w2) and np.array_equal(wbk, wb2)
    kx, _ = tgv_numpy.K_adj(p, q)
    assert np.array_equal(xk, vn.prox_kl(x - 0.3 * kx, b, np.full(shape, 0.7)))
    assert np.all(xk >= 0) and np.array_equal(xbk, xk + (xk - x))
    xw = tgv_numpy.primal_step_weighted(p, q, x, w, b, wt, 0.3, 0.7, data_loss="kl")[0]
    assert np.array_equal(xw, vn.prox_kl(x - 0.3 * kx, b, 0.7 * wt, wt))
    assert np.array_equal(xw[1], (x - 0.3 * kx)[1])
    out = tgv_numpy.iterate(b, b, 5, 0.1, data_loss="kl", weights=wt)
    assert np.all(np.isfinite(out["x"]))
    ident = lambda v: v
    lin = tgv_numpy.iterate_linear(ident, ident, b, b, 5, 0.1, data_loss="kl",
                                   A_norm2=1., background=0.1, bounds=(0., np.inf))
    assert np.all(np.isfinite(lin["x"])) and np.all(lin["x"] >= 0)
    assert np.all(lin["r"] <= 1. / 0.1)            # q <= c
    with pytest.raises(ValueError):
        tgv_numpy.iterate(b, b, 1, 0.1, data_loss="huber")
    # the energies know the term: the iteration lowers it, and both functions agree
    long = tgv_numpy.iterate(b, b, 300, 0.1, data_loss="kl")
    zero = np.zeros((2,) + shape)
    e0 = tgv_numpy.energy(b, zero, b, 10., 2., data_loss="kl")
    e1 = tgv_numpy.energy(long["x"], long["w"], b, 10., 2., data_loss="kl")
    assert e1 < e0
    assert np.isclose(e1, tgv_numpy.energy_linear(long["x"], long["w"], long["x"], b, 10.,
                                                  2., data_loss="kl"), rtol=1e-13)
    assert tgv_numpy.energy_linear(x, zero, x, np.where(wt == 0, np.nan, b), 10., 2.,
                                   data_loss="kl", weights=wt, background=0.3) == \
        tgv_numpy.energy_linear(x, zero, x, b, 10., 2., data_loss="kl", weights=wt,
                                background=0.3)


def test_the_new_symbols_are_declared():
    from nsol_amd import _lib
    sym = _lib.declared_symbols()
    counts = {"nsol_pdl_dual_data_kl": 9, "nsol_pdl_stack_dual_data_kl": 12,
              "nsol_prox_kl": 7, "nsol_tgv_primal_kl": 19}
    for stem, n in counts.items():
        for suf in ("_f32", "_f64"):
            assert stem + suf in sym, stem + suf
            assert len(sym[stem + suf][1]) == n, (stem + suf, len(sym[stem + suf][1]))
    # the entries they stand beside are what they were
    assert len(sym["nsol_pdl_dual_data_f32"][1]) == 9
    assert len(sym["nsol_pdl_stack_dual_data_f32"][1]) == 12
    assert len(sym["nsol_tgv_primal_w_f64"][1]) == 20
    # background is a double between lmbda and n
    assert sym["nsol_pdl_dual_data_kl_f64"][1][4:8] == [_lib.c_dbl] * 3 + [_lib.c_i64]


# ------------------------------------------------------------------ command line
def _parse(argv):
    from nsol_amd.application import run_deconvolution
    return run_deconvolution.parse_args(
        ["--observation", "o.nii.gz", "--result", "r.nii.gz"] + argv)


@pytest.mark.parametrize("extra", [
    [], ["--background", "0.5"], ["--background", "0"],
    ["--mask", "m.nii.gz", "--nonnegative", "--isotropic", "--tolerance", "1e-3",
     "--check-every", "5", "--reconstruction-type", "HuberL2", "--background", "2"],
    ["--weights", "w.nii.gz", "--upsample", "2", "1"],
    ["--reconstruction-type", "TGVL2", "--beta", "1.5", "--background", "0.5"],
    ["--alpha", "0.01", "0.02", "--result-dir", "d", "--background", "0.5"],
    ["--slice-wise"]])
def test_cli_takes_kl(extra):
    from nsol_amd.application import run_deconvolution
    args = _parse(["--solver", "PDL", "--data-loss", "kl"] + extra)
    assert args.data_loss == "kl"
    want = float(extra[extra.index("--background") + 1]) if "--background" in extra else 0.
    assert args.background == want
    kw = run_deconvolution._pdl_arguments(args)
    assert kw["pdl_data_loss"] == "kl" and kw.get("background", 0.) == want


@pytest.mark.parametrize("argv", [
    ["--solver", "PDL", "--background", "0.5"],
    ["--solver", "PDL", "--data-loss", "ell1", "--background", "0.5"],
    ["--solver", "PD", "--data-loss", "kl", "--background", "0.5"],
    ["--solver", "PDL", "--data-loss", "kl", "--background", "-1"],
    ["--solver", "PDL", "--data-loss", "kl", "--background", "nan"],
    ["--solver", "PDL", "--data-loss", "huber"],
    ["--solver", "PDL", "--data-loss", "cauchy"],
    ["--solver", "PDL", "--data-loss", "kl", "--reconstruction-type", "TK1L2"]])
def test_cli_refusals_exit_with_status_2(capsys, argv):
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2
    assert capsys.readouterr().err


def test_cli_without_kl_is_what_it_was():
    from nsol_amd.application import run_deconvolution
    for loss, want in (("linear", "ell2"), ("ell2", "ell2"), ("ell1", "ell1")):
        args = _parse(["--solver", "PDL", "--data-loss", loss])
        kw = run_deconvolution._pdl_arguments(args)
        assert kw["pdl_data_loss"] == want and "background" not in kw


def test_cli_build_solver_wires_kl():
    import nsol_amd
    from nsol_amd.application import run_deconvolution
    from nsol_amd.tgv_solver import TGVPrimalDualLinearSolver
    obs = 10. + np.arange(48, dtype=float).reshape(6, 8)
    w = np.ones((6, 8))
    w[-1] = 0
    junk = obs.copy()
    junk[-1] = np.nan
    s = run_deconvolution.build_solver(junk, np.ones(2), 1.0, "HuberL2", "PDL", 0.02, 7,
                                       dtype=np.float64, weights=w, pdl_data_loss="kl",
                                       nonnegative=True, background=0.5)
    assert isinstance(s, nsol_amd.PrimalDualLinearSolver)
    assert s.get_data_loss() == "kl" and s.get_background() == 0.5
    assert s.get_bounds() == (0., np.inf) and s.get_x_scale() == obs[:-1].max()
    t = run_deconvolution.build_solver(obs, np.ones(2), 1.0, "TGVL2", "PDL", 0.02, 7,
                                       pdl_data_loss="kl", background=0.25, beta=1.5)
    assert isinstance(t, TGVPrimalDualLinearSolver)
    assert t.get_data_loss() == "kl" and t.get_background() == 0.25
    with pytest.raises(ValueError):
        run_deconvolution.build_solver(obs, np.ones(2), 1.0, "TVL2", "PD", 0.02, 7,
                                       background=0.5)
    with pytest.raises(ValueError):
        run_deconvolution.build_solver(obs, np.ones(2), 1.0, "TVL2", "PDL", 0.02, 7,
                                       pdl_data_loss="ell1", background=0.5)
