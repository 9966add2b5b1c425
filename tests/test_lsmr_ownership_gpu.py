"""Who owns what the LSMR solvers are handed: every device tensor a caller passes in
(b, b_reg / x, x0) is bit-identical after the call, a solver's own b_reg survives its
run(), and a second run() repeats the first bit for bit.  Needs a real MI355X.

k_lsmr_u (nsol_lsmr.hip) overwrites the lower block of u on every step of the
bidiagonalisation, so that form has to work in a copy of any lower block it is not given
to keep; the normal-equations form only reads.  The cases where the factor that rides
with the block is exactly 1 (x_scale = 2 with tau = 0.25: sqrt(1 / tau) / x_scale = 1;
alpha = 1) are the ones in which no scaled copy is made on the way.

How a case reaches a form (asserted through lsmr.LAST_FORM, which only the
normal-equations form sets):
  bidiagonalisation      iter_max = 40 > lsmr.NE_MAX_ITER, or
                         lsmr.USE_NORMAL_EQUATIONS = False at iter_max = 6
  normal equations       iter_max = 6 with the flag as it is
  promoted to float64    float32, alpha = 1e-3 (below the weight guard), iter_max = 12 >
                         lsmr.PROMOTE_FROM_ITERATIONS; asserted through lsmr.LAST_PROMOTED

Volumes: (9, 10, 16) and 1-D 257, float64 and float32, B = identity and B = gradient.

Gates.  Results of two solvers that differ only in where x_scale is applied: rel-L2
2e-6 (float32) / 1e-12 (float64), those of
test_gpu_parity.test_prox_least_squares_folds_x_scale_into_coefficients; their costs:
relative 1e-6 / 1e-12.  The regularisation cost against NumPy: the reference is evaluated
in float64 at the very iterate the solver holds, so only the roundings of B x and of the
products remain: relative 1e-6 / 1e-12.

Observed on an MI355X: the prox against the plain solver 0 in both types (x_scale = 2
scales exactly); costs of the deferred against the plain solver at most 2.0e-7 (float32)
and 3.9e-15 (float64).  Before the lower block had an owner of its own, the factor-1
cases failed as written (the caller's x held u's lower block after the call, and so did
the solver's b_reg behind get_b_reg()), and so did the cost case on the 3-D
volume, evaluated at x * x_scale; the 1-D signal never takes the form that assembles
x * x_scale, so its cost case passed then as now."""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
SHAPES = ((9, 10, 16), (257,))
SHAPE_IDS = ("9x10x16", "257")
# (how the solve is sent to the bidiagonalisation)
WAYS = ("iter_max_40", "flag_off")


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()                      # fails loudly if the .so is missing
    return nsol_amd


def _tol(dtype):
    return 2e-6 if dtype == np.float32 else 1e-12


def _cost_tol(dtype):
    return 1e-6 if dtype == np.float32 else 1e-12


class _Problem(object):
    """A blurred, noisy volume on the device with the flat operators around it."""

    def __init__(self, shape, dtype, reg):
        import torch
        import nsol_amd.linear_operators as LO
        self.shape, self.dtype, self.reg = shape, dtype, reg
        self.n = n = int(np.prod(shape))
        nd = len(shape)
        rng = np.random.default_rng(21 + nd)
        clean = np.clip(rng.standard_normal(shape).cumsum(axis=nd - 1), -5, 5) + 10.0
        if nd == 3:
            lo = LO.LinearOperators3D()
            A, A_adj = lo.get_gaussian_blurring_operators(np.diag([1.0, 1.0, 1.0]))
        else:
            lo = LO.LinearOperators1D()
            A, A_adj = lo.get_gaussian_blurring_operators(1.0)
        self.td = td = torch.float32 if dtype == np.float32 else torch.float64
        self.A = lambda v: A(v.reshape(*shape)).flatten()
        self.A_adj = lambda v: A_adj(v.reshape(*shape)).flatten()
        self.b = A(torch.from_numpy(clean).to("cuda", td)).flatten().clone()
        gen = torch.Generator(device="cuda").manual_seed(3)
        self.noisy = self.b + 0.3 * torch.randn(n, device="cuda", dtype=td, generator=gen)
        if reg == "identity":
            self.B = self.B_adj = lambda v: v.flatten()
            self.rows = n
        else:
            grad, grad_adj = lo.get_gradient_operators()
            zshape = (nd * shape[0],) + tuple(shape[1:])
            self.B = lambda v: grad(v.reshape(*shape)).flatten()
            self.B_adj = lambda v: grad_adj(v.reshape(*zshape)).flatten()
            self.rows = nd * n
        # a lower block of the regulariser's size, of the data's magnitude
        self.b_reg = (self.noisy if reg == "identity" else
                      0.3 * torch.randn(self.rows, device="cuda", dtype=td, generator=gen))

    def reg_cost(self, x):
        """1/2 |B x|^2 in float64 NumPy (the solvers' regularisation cost)."""
        from oracle import nsol_oracle as orc
        x = np.asarray(x, np.float64).reshape(self.shape)
        Bx = x if self.reg == "identity" else orc.grad(x)
        return 0.5 * float(np.sum(Bx.astype(np.float64) ** 2))


class _Snapshots(object):
    def __init__(self, **tensors):
        self.live = tensors
        self.before = dict((k, t.clone()) for k, t in tensors.items())

    def check(self, what):
        import torch
        torch.cuda.synchronize()
        for k, t in self.live.items():
            assert torch.equal(t, self.before[k]), "%s: %s was written" % (what, k)


def _route(monkeypatch, way):
    """(iter_max, expected form) with the module flag set for `way`."""
    from nsol_amd import lsmr
    lsmr.LAST_FORM[0] = None
    lsmr.LAST_PROMOTED[0] = False
    if way == "iter_max_40":
        assert 40 > lsmr.NE_MAX_ITER
        return 40
    if way == "flag_off":
        monkeypatch.setattr(lsmr, "USE_NORMAL_EQUATIONS", False)
        return 6
    assert way == "normal" and lsmr.USE_NORMAL_EQUATIONS and 6 <= lsmr.NE_MAX_ITER
    return 6


def _assert_form(way):
    from nsol_amd import lsmr
    if way == "normal":
        assert lsmr.LAST_FORM[0] in ("lanczos", "lanczos-in-blur"), lsmr.LAST_FORM[0]
    else:
        assert lsmr.LAST_FORM[0] is None, lsmr.LAST_FORM[0]     # (never tried)
    assert not lsmr.LAST_PROMOTED[0]


def _prox_case(monkeypatch, P, way, tau, x_scale):
    import nsol_amd.tikhonov_linear_solver as tk
    from nsol_amd.proximal_operators import ProximalOperators as prox
    iter_max = _route(monkeypatch, way)
    snap = _Snapshots(x=P.noisy, b=P.b)
    got = prox.prox_linear_least_squares(P.noisy, tau, P.A, P.A_adj, P.b, P.b,
                                         iter_max=iter_max, x_scale=x_scale)
    _assert_form(way)
    snap.check("prox_linear_least_squares %s tau %g" % (way, tau))
    assert got.data_ptr() != P.noisy.data_ptr()
    plain = tk.TikhonovLinearSolver(
        A=P.A, A_adj=P.A_adj, B=P.B, B_adj=P.B_adj, x0=P.b / x_scale, b=P.b / x_scale,
        b_reg=snap.before["x"].clone(), alpha=1.0 / tau, iter_max=iter_max,
        x_scale=x_scale, dtype=P.dtype)
    plain.run()
    err = rel_l2(got.cpu().numpy(), plain.get_x())
    print("prox %s %s tau %g: rel-L2 against the plain solver %.3e" %
          (way, np.dtype(P.dtype).name, tau, err))
    assert err < _tol(P.dtype), (way, tau, err)
    snap.check("the plain solver, %s tau %g" % (way, tau))


def _tikhonov_case(monkeypatch, P, way, alpha):
    import nsol_amd.tikhonov_linear_solver as tk
    iter_max = _route(monkeypatch, way)
    snap = _Snapshots(b=P.b, b_reg=P.b_reg, x0=P.noisy)
    s = tk.TikhonovLinearSolver(A=P.A, A_adj=P.A_adj, B=P.B, B_adj=P.B_adj, b=P.b,
                                x0=P.noisy, alpha=alpha, b_reg=P.b_reg,
                                iter_max=iter_max, dtype=P.dtype)
    b_reg_before = s.get_b_reg()
    assert np.array_equal(b_reg_before, snap.before["b_reg"].cpu().numpy().astype(np.float64))
    s.run()
    _assert_form(way)
    what = "TikhonovLinearSolver %s %s alpha %g" % (P.reg, way, alpha)
    snap.check(what)
    assert np.array_equal(s.get_b_reg(), b_reg_before), what + ": the solver's b_reg"
    x1 = s.get_x()
    assert np.all(np.isfinite(x1)) and np.linalg.norm(x1) > 0
    ref = P.reg_cost(x1)
    got = s.get_cost_regularization_term()
    print("%s %s: regularisation cost %.17g against %.17g" %
          (what, np.dtype(P.dtype).name, got, ref))
    assert abs(got - ref) <= _cost_tol(P.dtype) * abs(ref), (what, got, ref)
    s.run()
    assert np.array_equal(s.get_x(), x1), what + ": the second run() differs"
    snap.check(what + ", second run")
    assert np.array_equal(s.get_b_reg(), b_reg_before)


# --------------------------------------------- cases 1 and 3: the prox on a device x
@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_prox_least_squares_keeps_x_when_the_factor_is_one(nsol, monkeypatch, shape, dtype,
                                                            way):
    """x_scale = 2, tau = 0.25: the lazy lower block is the caller's x itself and its
    factor sqrt(1 / tau) / x_scale is exactly 1 -- the bidiagonalisation must not work
    in it."""
    assert np.sqrt(1.0 / 0.25) / 2.0 == 1.0
    _prox_case(monkeypatch, _Problem(shape, dtype, "identity"), way, 0.25, 2.0)


@pytest.mark.parametrize("way", WAYS + ("normal",))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_prox_least_squares_reads_only(nsol, monkeypatch, shape, dtype, way):
    """The factor not 1 (tau = 0.5) in all three forms, and the factor 1 through the
    normal equations."""
    P = _Problem(shape, dtype, "identity")
    _prox_case(monkeypatch, P, way, 0.5, 2.0)
    if way == "normal":
        _prox_case(monkeypatch, P, way, 0.25, 2.0)


# ------------------------------------- cases 2 and 3: a solver around a device b_reg
@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("reg", ("identity", "gradient"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_tikhonov_keeps_b_reg_when_alpha_is_one(nsol, monkeypatch, shape, dtype, reg, way):
    """alpha = 1: the solver's own b_reg is handed over with the factor sqrt(alpha) = 1.
    It must still be there for get_b_reg() and for a second run()."""
    _tikhonov_case(monkeypatch, _Problem(shape, dtype, reg), way, 1.0)


@pytest.mark.parametrize("way", WAYS + ("normal",))
@pytest.mark.parametrize("reg", ("identity", "gradient"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_tikhonov_reads_only(nsol, monkeypatch, shape, dtype, reg, way):
    P = _Problem(shape, dtype, reg)
    _tikhonov_case(monkeypatch, P, way, 2.0)
    if way == "normal":
        _tikhonov_case(monkeypatch, P, way, 1.0)


# ---------------------------------------------------- case 4: promoted to float64
@pytest.mark.parametrize("reg", ("identity", "gradient"))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_promoted_float32_solve_reads_only(nsol, shape, reg):
    """float32, a regulariser below the normal equations' weight guard and more than
    PROMOTE_FROM_ITERATIONS iterations: the solve runs in float64 on widened copies."""
    import nsol_amd.tikhonov_linear_solver as tk
    from nsol_amd import lsmr
    from nsol_amd.proximal_operators import ProximalOperators as prox
    P = _Problem(shape, np.float32, reg)
    iter_max = 12
    assert lsmr.PROMOTE_FROM_ITERATIONS < iter_max <= lsmr.NE_MAX_ITER
    lsmr.LAST_PROMOTED[0] = False
    snap = _Snapshots(b=P.b, b_reg=P.b_reg, x0=P.noisy)
    s = tk.TikhonovLinearSolver(A=P.A, A_adj=P.A_adj, B=P.B, B_adj=P.B_adj, b=P.b,
                                x0=P.noisy, alpha=1e-3, b_reg=P.b_reg, iter_max=iter_max,
                                dtype=np.float32)
    b_reg_before = s.get_b_reg()
    s.run()
    assert lsmr.LAST_PROMOTED[0], "the solve was not promoted: the case proves nothing"
    snap.check("promoted TikhonovLinearSolver")
    assert np.array_equal(s.get_b_reg(), b_reg_before)
    x1 = s.get_x()
    s.run()
    assert np.array_equal(s.get_x(), x1)
    if reg == "identity":
        # the lazy block (the caller's x) with sqrt(alpha) / x_scale = 1 / 64
        lsmr.LAST_PROMOTED[0] = False
        snap = _Snapshots(x=P.noisy, b=P.b)
        prox.prox_linear_least_squares(P.noisy, 1024.0, P.A, P.A_adj, P.b, P.b,
                                       iter_max=iter_max, x_scale=2.0)
        assert lsmr.LAST_PROMOTED[0]
        snap.check("promoted prox_linear_least_squares")


# ------------------------------------------------------------------- case 5: ADMM
@pytest.mark.parametrize("way", WAYS + ("normal",))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_admm_keeps_b_and_x0(nsol, monkeypatch, shape, dtype, way):
    """rho = 1 (sqrt(rho) = 1 rides with the inner solves' lower block) and rho = 0.5,
    without and with a device b_reg."""
    import nsol_amd.admm_linear_solver as admm
    P = _Problem(shape, dtype, "gradient")
    for rho, with_b_reg in ((1.0, False), (0.5, False), (1.0, True)):
        iter_max = _route(monkeypatch, way)
        snap = _Snapshots(b=P.b, x0=P.noisy, b_reg=P.b_reg)
        s = admm.ADMMLinearSolver(A=P.A, A_adj=P.A_adj, b=P.b, B=P.B, B_adj=P.B_adj,
                                  x0=P.noisy, dimension=len(shape),
                                  b_reg=P.b_reg if with_b_reg else 0, alpha=0.05, rho=rho,
                                  iterations=3, iter_max=iter_max, dtype=dtype)
        s.run()
        x = s.get_x()
        assert np.all(np.isfinite(x)) and np.linalg.norm(x) > 0
        snap.check("ADMMLinearSolver %s rho %g b_reg %s" % (way, rho, with_b_reg))


# ------------------------------------------------- case 6: costs of a deferred solver
@pytest.mark.parametrize("reg", ("identity", "gradient"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_costs_of_a_deferred_solver_are_those_of_the_plain_one(nsol, shape, dtype, reg):
    """A _defer_scaling solver may hold its solution as x * x_scale; b and b_reg stay in
    the solver's units, and so must the point the cost getters evaluate at."""
    import nsol_amd.tikhonov_linear_solver as tk
    P = _Problem(shape, dtype, reg)
    xs = float(P.b.max())
    snap = _Snapshots(b=P.b, b_reg=P.b_reg)
    costs = {}
    for defer in (True, False):
        s = tk.TikhonovLinearSolver(A=P.A, A_adj=P.A_adj, B=P.B, B_adj=P.B_adj,
                                    x0=P.b / xs, b=P.b / xs, b_reg=P.b_reg, alpha=2.0,
                                    iter_max=4, x_scale=xs, dtype=dtype,
                                    _defer_scaling=defer)
        s.run()
        if defer:
            print("solution held in the caller's units: %s" % s._x_in_callers_units)
            # (the form that assembles x * x_scale takes 3-D volumes: there the case
            # evaluates the costs of a solver that holds its iterate in other units)
            assert s._x_in_callers_units or len(shape) != 3
            before = s.get_x()
        else:
            assert not s._x_in_callers_units
        costs[defer] = (s.get_total_cost(), s.get_cost_data_term(),
                        s.get_cost_regularization_term())
        if defer:
            # ... and asking changed nothing the solver hands out
            assert np.array_equal(s.get_x(), before)
            assert np.array_equal(before,
                                  s.get_x_device().cpu().numpy().astype(np.float64))
    snap.check("deferred and plain solver")
    for name, got, ref in zip(("total", "data", "regularisation"), costs[True], costs[False]):
        print("%s %s %s cost: deferred %.17g plain %.17g rel %.3e" %
              (SHAPE_IDS[SHAPES.index(shape)], np.dtype(dtype).name, name, got, ref,
               abs(got - ref) / abs(ref)))
    for name, got, ref in zip(("total", "data", "regularisation"), costs[True], costs[False]):
        assert abs(got - ref) <= _cost_tol(dtype) * abs(ref), (name, got, ref)
