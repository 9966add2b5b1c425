"""The Poisson (Kullback-Leibler) data term on the GPU: the four new entries of the C ABI
against the NumPy restatements (nsol_amd/vector_numpy.py, nsol_amd/tgv_numpy.py) and
against each other bit for bit, the solvers that take data_loss="kl" against the restated
iterations, the stacked front ends against every member's own run, and the command
line."""
import numpy as np
import pytest

from conftest import rel_l2
from device_arena import Arena
from kl_cases import (dual_scaled_error, pd_linear_kl_restatement, relative_error,
                      stress_vector)
from nsol_amd import tgv_numpy as tg
from nsol_amd import vector_numpy as vn
from test_pd_linear_host import gaussian_kernel, grad, grad_adj
from test_pd_weighted_host import mixed_weights
from test_tgv_gpu import SHAPES as TGV_SHAPES
from test_tgv_gpu import (TAU, THETA, TL, _call_primal, _dims, _iw, _rounded_spacing,
                          _state)

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12     # float64 kernels vs the float64 restatement
F32_TOL = 1e-5      # the project's standing gate
ITERS = 25
BOTH = [np.float64, np.float32]
SIZES = [1, 255, 256, 257, 4099]


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


def _fn(name, dtype):
    from nsol_amd import _lib
    return getattr(_lib.load(), "nsol_%s_%s" % (
        name, "f64" if np.dtype(dtype) == np.float64 else "f32"))


def _stream():
    from nsol_amd.device import stream_ptr
    return stream_ptr()


def _sync():
    import torch
    torch.cuda.synchronize()


def _rounded(a, dtype):
    return np.asarray(a).astype(dtype).astype(np.float64)


# ------------------------------------------------------------ 1. entries 1 and 3
def _element_case(n, dtype, seed=0):
    """Moderate values, rounded to dtype and held in float64: q, t, bt >= 0 with a few
    exact zeros, weights with exact zeros, and bt = NaN under weight 0 (junk)."""
    rng = np.random.default_rng(100 + n + seed)
    q = _rounded(3. * rng.standard_normal(n), dtype)
    t = _rounded(np.abs(rng.standard_normal(n)) + 0.1, dtype)
    bt = _rounded(rng.uniform(0., 3., n), dtype)
    bt[rng.random(n) < 0.1] = 0.
    w = _rounded(mixed_weights((n,), n + seed), dtype)
    junk = bt.copy()
    junk[w == 0] = np.nan
    x = _rounded(2. * rng.standard_normal(n), dtype)
    return dict(q=q, t=t, bt=bt, wt=w, junk=junk, x=x)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", BOTH)
def test_dual_data_kl_matches_the_restatement(nsol, n, dtype):
    c = _element_case(n, dtype)
    sigma, lmbda = 0.3, 20.
    lm_t = vn.as_scalar(lmbda, dtype)
    for offset in (0, 1):
        for with_t in (True, False):
            for with_w in (True, False):
                for bg in (0., 0.37):
                    bt = c["junk"] if with_w else c["bt"]
                    ar = Arena(dict(q=c["q"], t=c["t"], bt=bt, wt=c["wt"]), dtype, offset)
                    rc = _fn("pdl_dual_data_kl", dtype)(
                        ar.ptr("q"), ar.ptr("t") if with_t else None, ar.ptr("bt"),
                        ar.ptr("wt") if with_w else None, sigma, lmbda, bg, n, _stream())
                    assert rc == 0
                    _sync()
                    key = (n, offset, with_t, with_w, bg)
                    w = c["wt"] if with_w else np.ones(n)
                    want = vn.pdl_dual_data_kl(c["q"], c["t"] if with_t else None, bt,
                                               c["wt"] if with_w else None, sigma, lmbda,
                                               bg, dtype)
                    got = ar.get("q", (n,))
                    assert np.all(np.isfinite(got)), key
                    assert np.all(got[w == 0] == 0), key
                    assert np.all(got <= _rounded(lm_t * w, dtype)), key   # q <= c
                    err = dual_scaled_error(got, want, np.maximum(lm_t * w, 1e-300))
                    assert err <= _gate(dtype), (key, err)
                    assert ar.guards_intact(), key
                    for k in ("t", "wt"):                 # the inputs are only read
                        assert np.array_equal(ar.get(k, (n,)), c[k]), (key, k)
                    assert np.array_equal(ar.get("bt", (n,)), bt, equal_nan=True), key


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", BOTH)
def test_prox_kl_matches_the_restatement(nsol, n, dtype):
    c = _element_case(n, dtype, seed=1)
    # bt == 0 gives max(x - t, 0), which cancels where x is close to t: a relative gate
    # on it needs the kernel's t = tl * w to be the reference's, so tl is a power of two
    tl = 0.5
    for offset in (0, 1):
        for with_w in (True, False):
            for in_place in (False, True):
                bt = c["junk"] if with_w else c["bt"]
                ar = Arena(dict(x=c["x"], out=np.zeros(n), bt=bt, wt=c["wt"]), dtype,
                           offset)
                rc = _fn("prox_kl", dtype)(
                    ar.ptr("x" if in_place else "out"), ar.ptr("x"), ar.ptr("bt"),
                    ar.ptr("wt") if with_w else None, tl, n, _stream())
                assert rc == 0
                _sync()
                key = (n, offset, with_w, in_place)
                want = vn.prox_kl_w(c["x"], bt, c["wt"] if with_w else None, tl, dtype)
                got = ar.get("x" if in_place else "out", (n,))
                assert np.all(np.isfinite(got)), key
                keep = (c["wt"] == 0) if with_w else np.zeros(n, bool)
                assert np.array_equal(got[keep], c["x"][keep]), key
                assert np.all(got[~keep] >= 0), key
                err = relative_error(got, want)
                assert err <= _gate(dtype), (key, err)
                assert ar.guards_intact(), key
                if not in_place:
                    assert np.array_equal(ar.get("x", (n,)), c["x"]), key


@pytest.mark.parametrize("dtype", BOTH)
def test_both_proxes_on_the_stress_vector(nsol, dtype):
    """The CPU stress vector cut to 4099 elements: v in q's place with t null and no
    background (v = q exactly) and c as the weights under lmbda = 1; for the primal prox
    t = c / sigma as the weights under tl = 1."""
    n = 4099
    s = {k: a[:n].astype(np.float64) for k, a in stress_vector().items()}
    worst = [0., 0.]
    for sigma in (1e-2, 0.3, 10.):
        sg = vn.as_scalar(sigma, dtype)
        t = _rounded(s["c"] / sg, dtype)           # t = c / sigma, as in the CPU test
        ar = Arena(dict(q=s["v"], bt=s["bt"], wt=s["c"], x=s["u"], t=t), dtype, 1)
        assert _fn("pdl_dual_data_kl", dtype)(ar.ptr("q"), None, ar.ptr("bt"),
                                              ar.ptr("wt"), sigma, 1., 0., n,
                                              _stream()) == 0
        assert _fn("prox_kl", dtype)(ar.ptr("x"), ar.ptr("x"), ar.ptr("bt"), ar.ptr("t"),
                                     1., n, _stream()) == 0
        _sync()
        q, x = ar.get("q", (n,)), ar.get("x", (n,))
        want_q = vn.kl_dual_prox(s["v"], s["c"], sg, s["bt"])
        want_x = vn.prox_kl(s["u"], s["bt"], t)
        assert np.all(q <= s["c"]) and np.all(x >= 0)
        zero = s["bt"] == 0
        if dtype is np.float64:                    # (float32 rounds c + (v - c))
            assert np.array_equal(q[zero], np.minimum(s["v"], s["c"])[zero])
        eq, ex = dual_scaled_error(q, want_q, s["c"]), relative_error(x, want_x)
        worst = [max(worst[0], eq), max(worst[1], ex)]
        assert eq <= _gate(dtype) and ex <= _gate(dtype), (sigma, eq, ex)
        assert ar.guards_intact()
    print("stress vector %s: dual %.3g, primal %.3g" % (np.dtype(dtype).name, *worst))


@pytest.mark.parametrize("dtype", BOTH)
def test_the_element_entries_check_their_arguments(nsol, dtype):
    import torch
    from nsol_amd import ops
    from nsol_amd.device import to_device
    n = 300
    mk = lambda v: to_device(np.full(n, v), dtype)
    q, t, bt, wt, out = mk(0.25), mk(0.5), mk(1.), mk(2.), mk(7.)
    P = lambda a: None if a is None else a.data_ptr()
    dual, prox = _fn("pdl_dual_data_kl", dtype), _fn("prox_kl", dtype)

    def d(q=q, t=t, bt=bt, wt=wt, sigma=0.3, lmbda=2., bg=0.1, n=n):
        return dual(P(q), P(t), P(bt), P(wt), sigma, lmbda, bg, n, _stream())

    def p(out=out, x=q, bt=bt, wt=wt, tl=0.5, n=n):
        return prox(P(out), P(x), P(bt), P(wt), tl, n, _stream())
    assert d(n=0) == 0 and d(q=None, bt=None, n=0) == 0 and p(n=0) == 0
    assert p(out=None, x=None, bt=None, n=0) == 0
    for bad in (dict(q=None), dict(bt=None), dict(t=q), dict(sigma=0.), dict(sigma=-1.),
                dict(sigma=np.nan), dict(lmbda=-1.), dict(lmbda=np.nan), dict(n=-1),
                dict(bg=-0.1), dict(bg=np.nan), dict(bg=np.inf)):
        assert d(**bad) == -1, bad
    for bad in (dict(out=None), dict(x=None), dict(bt=None), dict(tl=-1.),
                dict(tl=np.nan), dict(tl=np.inf), dict(n=-1)):
        assert p(**bad) == -1, bad
    _sync()
    for a, v in ((q, 0.25), (t, 0.5), (bt, 1.), (wt, 2.), (out, 7.)):
        assert torch.equal(a, torch.full_like(a, v))      # refused before any launch
    assert d() == 0 and d(t=None, wt=None) == 0 and p() == 0 and p(wt=None) == 0
    _sync()
    # the Python wrappers check their operands before the library sees them
    with pytest.raises(ValueError):
        ops.pdl_dual_data_kl(q, None, q[:7], None, 0.3, 1.)
    with pytest.raises(ValueError):
        ops.pdl_dual_data_kl(q, q, bt, None, 0.3, 1.)
    with pytest.raises(ValueError):
        ops.pdl_dual_data_kl(q, None, bt, None, 0.3, 1., -1.)
    with pytest.raises(ValueError):
        ops.prox_kl(q, bt[:7], None, 0.5)
    with pytest.raises(ValueError):
        ops.prox_kl(q, bt, None, -0.5)


# ------------------------------------------------------------ 2. the stacked entry
@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("dtype", BOTH)
def test_stacked_dual_data_kl_is_the_single_entry_per_member(nsol, P, dtype):
    from nsol_amd import ops
    from nsol_amd.device import to_device, to_numpy
    n = 257
    cases = [_element_case(n, dtype, seed=10 + m) for m in range(P)]
    lmbda = np.array([20., 3.5, 0.75][:P])
    sigma, bg = 0.3, 0.21
    up = lambda a: to_device(np.ascontiguousarray(a).reshape(-1), dtype)
    q0 = np.stack([c["q"] for c in cases])
    t = np.stack([c["t"] for c in cases])
    lam = ops.pdl_lambdas(lmbda, up(q0))
    for own_b in (False, True):                           # bt at stride 0 or n
        for w_mode in ("none", "shared", "own"):          # no weights, stride 0, stride n
            W = {"none": np.ones((P, n)), "shared": np.stack([cases[0]["wt"]] * P),
                 "own": np.stack([c["wt"] for c in cases])}[w_mode]
            B = np.stack([c["bt"] for c in cases]) if own_b else \
                np.stack([cases[0]["bt"]] * P)
            if own_b:
                B[W == 0] = np.nan
            else:
                B[:, np.all(W == 0, axis=0)] = np.nan
            b_in = B if own_b else B[:1]
            w_in = None if w_mode == "none" else (W if w_mode == "own" else W[:1])
            for with_t in (True, False):
                q = up(q0)
                assert ops.pdl_stack_dual_data_kl(
                    q, up(t) if with_t else None, up(b_in),
                    None if w_in is None else up(w_in), sigma, lam, P, bg)
                got = to_numpy(q, dtype).reshape(P, n)
                for m in range(P):
                    one = up(q0[m])
                    ops.pdl_dual_data_kl(one, up(t[m]) if with_t else None, up(B[m]),
                                         None if w_in is None else up(W[m]), sigma,
                                         lmbda[m], bg)
                    key = (own_b, w_mode, with_t, m)
                    assert np.array_equal(got[m], to_numpy(one, dtype)), key
                    assert np.all(np.isfinite(got[m])) and np.all(got[m][W[m] == 0] == 0)
                    want = vn.pdl_dual_data_kl(q0[m], t[m] if with_t else None, B[m],
                                               W[m], sigma, lmbda[m], bg, dtype)
                    c = vn.as_scalar(lmbda[m], dtype) * W[m]
                    assert dual_scaled_error(got[m], want, np.maximum(c, 1e-300)) <= \
                        _gate(dtype), key
    # the contract of nsol_pdl_stack_dual_data_*: -2 declines, a stride is 0 or n
    entry = _fn("pdl_stack_dual_data_kl", dtype)
    q, b = up(q0), up(B)
    call = lambda members=P, bts=n, bg_=bg, sg=sigma: entry(
        q.data_ptr(), None, b.data_ptr(), bts, None, 0, sg, lam.data_ptr(), bg_, members,
        n, _stream())
    assert call(members=0) == -2 and call(members=65536) == -2
    assert call(bts=n + 1) == -1 and call(bg_=-1.) == -1 and call(bg_=np.nan) == -1
    assert call(sg=0.) == -1
    _sync()
    assert np.array_equal(to_numpy(q, dtype).reshape(P, n), q0.astype(dtype))
    with pytest.raises(ValueError):
        ops.pdl_stack_dual_data_kl(q, None, b, None, sigma, lam, P + 1)


# ------------------------------------------------------------ 3. the TGV primal step
OFF_16 = [s for s in TGV_SHAPES if s in ((259,), (6, 259), (3, 5, 7), (5, 4, 64),
                                         (3, 5, 8))]
KL_ARRAYS = ("p", "q", "x", "xbar", "w", "wbar", "bt")


def _kl_state(shape, dtype):
    """test_tgv_gpu's state with counts in b's place (|bt|) and weights with zeros."""
    s = dict(_state(shape, dtype))
    s["bt"] = np.abs(s["bt"])
    s["wt"] = _rounded(mixed_weights(shape, sum(shape)), dtype)
    s["junk"] = np.where(s["wt"] == 0, np.nan, s["bt"])
    return s


def _check_tgv_primal_kl(shape, dtype, weighted, offset=0):
    s = _kl_state(shape, dtype)
    d = len(shape)
    c = lambda v: float(np.dtype(dtype).type(v))
    bt = s["junk"] if weighted else s["bt"]
    arrays = {k: s[k] for k in KL_ARRAYS}
    arrays["bt"] = bt
    if weighted:
        arrays["wt"] = s["wt"]
    ar = Arena(arrays, dtype, offset)
    rc = _fn("tgv_primal_kl", dtype)(
        *[ar.ptr(k) for k in KL_ARRAYS], ar.ptr("wt") if weighted else None,
        *_dims(shape), *_iw(d), TAU, TL, THETA, _stream())
    assert rc == 0
    _sync()
    sp = _rounded_spacing(shape, dtype)
    if weighted:
        want = tg.primal_step_weighted(s["p"], s["q"], s["x"], s["w"], bt, s["wt"], c(TAU),
                                       c(TL), c(THETA), sp, "kl")
    else:
        want = tg.primal_step(s["p"], s["q"], s["x"], s["w"], bt, c(TAU), c(TL), c(THETA),
                              sp, "kl")
    label = "tgv primal kl %r weighted=%d off=%d" % (shape, weighted, offset)
    got = {k: ar.get(k, v.shape) for k, v in zip(("x", "xbar", "w", "wbar"), want)}
    assert all(np.all(np.isfinite(v)) for v in got.values()), label
    errs = [rel_l2(got[k], v, label + " " + k)
            for k, v in zip(("x", "xbar", "w", "wbar"), want)]
    assert max(errs) <= _gate(dtype), (label, errs)
    if weighted:
        keep = s["wt"] == 0
        assert np.all(got["x"][~keep] >= 0), label
    else:
        assert np.all(got["x"] >= 0), label
    assert ar.guards_intact(), label
    for k in ("p", "q"):
        assert np.array_equal(ar.get(k, s[k].shape), s[k]), (label, k)
    # w and wbar: the bits nsol_tgv_primal_* gives them on the same inputs
    ref = Arena({k: s[k] for k in KL_ARRAYS}, dtype, offset)
    assert _call_primal(shape, dtype, 0, ref) == 0
    _sync()
    for k in ("w", "wbar"):
        a = ar.t[k].cpu().numpy()
        assert np.array_equal(a.view(np.uint8), ref.t[k].cpu().numpy().view(np.uint8)), \
            (label, k)


@pytest.mark.parametrize("shape", TGV_SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_tgv_primal_kl_matches_numpy(nsol, shape, dtype):
    from nsol_amd import ops
    before = ops.tgv_launches()
    for weighted in (False, True):
        _check_tgv_primal_kl(shape, dtype, weighted)
    assert ops.tgv_launches() - before == 4       # the same counter, the plain calls too


@pytest.mark.parametrize("shape", OFF_16)
@pytest.mark.parametrize("dtype", BOTH)
def test_tgv_primal_kl_off_16_byte_alignment(nsol, shape, dtype):
    assert len(OFF_16) == 5
    for weighted in (False, True):
        _check_tgv_primal_kl(shape, dtype, weighted, offset=3)


def test_tgv_primal_kl_checks_its_arguments(nsol):
    import torch
    from nsol_amd.device import to_device
    dtype, shape = np.float32, (3, 4, 6)
    n = 72
    mk = lambda k: to_device(np.full(k * n, 0.25), dtype)
    p, q, x, xbar, w, wbar, bt, wt = mk(3), mk(6), mk(1), mk(1), mk(3), mk(3), mk(1), mk(1)
    good = [p, q, x, xbar, w, wbar, bt, wt]
    entry = _fn("tgv_primal_kl", dtype)

    def call(a=good, dims=(3,) + shape, tau=0.3, tl=0.5, theta=1.):
        return entry(*[None if t is None else t.data_ptr() for t in a], *dims, 1., 1., 1.,
                     tau, tl, theta, _stream())
    for k in range(7):
        a = list(good)
        a[k] = None
        assert call(a) == -1, k
    assert call(good[:7] + [x]) == -1                      # wt overlaps x
    for bad in (dict(tau=0.), dict(tau=np.nan), dict(tl=-1.), dict(tl=np.inf),
                dict(theta=np.nan), dict(dims=(4,) + shape)):
        assert call(**bad) == -1, bad
    assert call(dims=(3, 1 << 11, 1 << 11, 1 << 10)) == -2
    assert call(dims=(3, 0, 4, 6)) == 0
    _sync()
    for t in good:
        assert torch.equal(t, torch.full_like(t, 0.25))
    assert call() == 0 and call(good[:7] + [None]) == 0
    _sync()


# ------------------------------------------------------------ 4. the solvers
def _counts(shape, seed=None):
    """Poisson counts of a smooth positive image on `shape`."""
    rng = np.random.default_rng(sum(shape) if seed is None else seed)
    grid = np.indices(shape).sum(axis=0)
    return rng.poisson(12. + 8. * np.sin(0.7 * grid)).astype(np.float64)


def _kernel_for(shape):
    """A 5-tap Gaussian (sigma 0.6): it fits the extents of 6."""
    return gaussian_kernel(len(shape), 0.6)


def _weights_over_nan(shape, obs):
    """(weights with a block of zeros, the observation with NaN under it)."""
    w = np.ones(shape)
    w[tuple(slice(1, 3) for _ in shape)] = 0.
    w.reshape(-1)[-1] = 2.5
    junk = obs.copy()
    junk[w == 0] = np.nan
    return w, junk


def _wrapped(op, shape):
    return lambda x: op(x.reshape(*shape)).flatten()


def _pdl(nsol, obs, kernel, dtype, op=None, **kw):
    from nsol_amd.linear_operators import ConvolutionOperator
    shape = obs.shape
    A = ConvolutionOperator(len(shape), kernel) if op is None else op
    args = dict(A=_wrapped(A, shape), A_adj=_wrapped(A, shape), b=obs.flatten(),
                x0=np.nan_to_num(obs).flatten(), dimension=len(shape), alpha=0.05,
                iterations=ITERS, x_scale=float(np.nanmax(obs)), dtype=dtype,
                data_loss="kl")
    args.update(kw)
    return nsol.PrimalDualLinearSolver(**args)


PDL_SHAPES = [(12, 10), (6, 7, 8)]
_REF = {}


def _pdl_reference(shape, reg, iso, bg):
    key = (shape, reg, iso, bg)
    if key not in _REF:
        obs = _counts(shape)
        w, junk = _weights_over_nan(shape, obs)
        _REF[key] = pd_linear_kl_restatement(
            junk, _kernel_for(shape), shape, reg, 0.05, ITERS, weights=w,
            bounds=(0., np.inf), iso=iso, x_scale=obs.max(), background=bg,
            x0=np.nan_to_num(junk))
    return _REF[key]


@pytest.mark.parametrize("shape", PDL_SHAPES)
@pytest.mark.parametrize("reg", ["TV", "huber"])
@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("bg", [0., 1.5])
@pytest.mark.parametrize("dtype", BOTH)
def test_pdl_runs_match_the_restatement(nsol, shape, reg, iso, bg, dtype):
    from nsol_amd import ops
    obs = _counts(shape)
    w, junk = _weights_over_nan(shape, obs)
    s = _pdl(nsol, junk, _kernel_for(shape), dtype, reg_type=reg, isotropic=iso,
             weights=w.flatten(), bounds=(0., np.inf), background=bg,
             x_scale=float(obs.max()))
    before = ops.pdl_launches()
    s.run()
    assert ops.pdl_launches() - before == ITERS
    assert s.get_execution() == "fused" and s.get_iterations_done() == ITERS
    x = s.get_x()
    assert np.all(np.isfinite(x)) and np.all(x >= 0)
    err = rel_l2(x, _pdl_reference(shape, reg, iso, bg), np.dtype(dtype).name)
    print(shape, reg, iso, bg, np.dtype(dtype).name, err)
    assert err <= _gate(dtype), err


@pytest.mark.parametrize("dtype", BOTH)
def test_pdl_without_weights_or_bounds(nsol, dtype):
    shape = (12, 10)
    obs = _counts(shape)
    s = _pdl(nsol, obs, _kernel_for(shape), dtype, background=0.5)
    s.run()
    ref = pd_linear_kl_restatement(obs, _kernel_for(shape), shape, "TV", 0.05, ITERS,
                                   x_scale=obs.max(), background=0.5)
    assert rel_l2(s.get_x(), ref) <= _gate(dtype)


@pytest.mark.parametrize("shape, var, dtype", [((9, 5, 16), 4., np.float64),
                                               ((20, 37, 64), 2., np.float32)])
def test_pdl_on_the_blur_epilogue_path(nsol, monkeypatch, shape, var, dtype):
    from nsol_amd import linear_operators as LO, ops
    from test_pd_linear_host import separable_taps
    A, _ = LO.LinearOperators3D().get_gaussian_blurring_operators(np.diag([var] * 3))
    obs = _counts(shape)
    w, junk = _weights_over_nan(shape, obs)
    ran, real = [], ops.corr3_wrap_axpby

    def counted(*a, **k):
        out = real(*a, **k)
        ran.append(out is not None)
        return out
    monkeypatch.setattr(ops, "corr3_wrap_axpby", counted)
    got = {}
    for on in (True, False):
        monkeypatch.setattr(LO, "USE_BLUR_EPILOGUE", on)
        del ran[:]
        s = _pdl(nsol, junk, None, dtype, op=A, reg_type="huber", weights=w.flatten(),
                 background=1.5, bounds=(0., np.inf), x_scale=float(obs.max()))
        s.run()
        assert ran == ([True] * ITERS if on else [])
        got[on] = s.get_x()
    from test_pd_linear_host import blur
    taps = separable_taps(A.kernel)
    ref = pd_linear_kl_restatement(
        junk, None, shape, "huber", 0.05, ITERS, weights=w, bounds=(0., np.inf),
        x_scale=obs.max(), background=1.5, x0=np.nan_to_num(junk),
        A=lambda v: blur(v, taps), At=lambda v: blur(v, taps, adjoint=True), A_norm2=1.)
    for on in (True, False):
        err = rel_l2(got[on], ref, "%s epilogue=%d" % (np.dtype(dtype).name, on))
        print(shape, np.dtype(dtype).name, on, err)
        assert err <= _gate(dtype), err


@pytest.mark.parametrize("dtype", BOTH)
def test_the_three_execution_forms_agree(nsol, dtype):
    from scipy.ndimage import convolve
    from nsol_amd.device import is_device_tensor
    from nsol_amd.linear_operators import ConvolutionOperator
    shape = (6, 7, 8)
    obs, kernel = _counts(shape), _kernel_for(shape)
    w, junk = _weights_over_nan(shape, obs)
    op = ConvolutionOperator(3, kernel)

    def on_device(t):
        if not is_device_tensor(t):
            raise TypeError("device tensors only")
        return op(t.view(*shape)).reshape(-1)

    def on_host(v):
        return convolve(np.asarray(v, np.float64).reshape(shape), kernel,
                        mode="wrap").reshape(-1)
    kw = dict(weights=w.flatten(), shape=shape, background=1.5, bounds=(0., np.inf),
              x_scale=float(obs.max()))
    ref = _pdl_reference(shape, "TV", False, 1.5)
    for name, f in (("fused", None), ("device", on_device), ("host", on_host)):
        extra = {} if f is None else dict(A=f, A_adj=f, A_norm2=1.)
        s = _pdl(nsol, junk, kernel, dtype, **dict(kw, **extra))
        s.run()
        assert s.get_execution() == name
        err = rel_l2(s.get_x(), ref, "%s %s" % (name, np.dtype(dtype).name))
        assert err <= _gate(dtype), (name, err)


@pytest.mark.parametrize("dtype", BOTH)
def test_pdl_on_a_sampled_operator_pair(nsol, dtype):
    from test_pd_linear_sampled_gpu import _case, _operators
    from test_sampled_conv_host import sampled_adjoint, sampled_forward
    fine, factors, offsets = (12, 10), (2, 1), (0, 0)
    ks, obs0, x0, _ = _case(fine, factors, offsets)
    obs = np.round(np.abs(obs0))                  # counts
    coarse = obs.shape
    assert coarse == (6, 10)
    A, At = _operators(fine, factors, offsets)
    s = nsol.PrimalDualLinearSolver(
        A=lambda x: A(x.reshape(*fine)).flatten(),
        A_adj=lambda q: At(q.reshape(*coarse)).flatten(), b=obs.flatten(),
        x0=np.abs(x0).flatten(), dimension=2, alpha=0.05, iterations=ITERS,
        x_scale=float(obs.max()), dtype=dtype, data_loss="kl", background=1.5,
        bounds=(0., np.inf), reg_type="huber")
    s.run()
    assert s.get_execution() == "fused" and s.get_shape() == fine
    norm2 = float(np.prod([np.sum(np.abs(k)) for k in ks])) ** 2
    assert abs(s.get_A_norm2() - norm2) <= 1e-12
    ref = pd_linear_kl_restatement(
        obs, None, fine, "huber", 0.05, ITERS, bounds=(0., np.inf), x_scale=obs.max(),
        background=1.5, x0=np.abs(x0),
        A=lambda v: sampled_forward(v, ks, "wrap", factors, offsets),
        At=lambda v: sampled_adjoint(v, ks, "wrap", factors, offsets, fine),
        A_norm2=norm2)
    err = rel_l2(s.get_x(), ref.reshape(-1), np.dtype(dtype).name)
    assert err <= _gate(dtype), err


@pytest.mark.parametrize("dtype", BOTH)
def test_a_tolerance_stops_where_the_restatement_stops(nsol, dtype):
    shape, iters, every = (12, 10), 400, 10
    obs, kernel = _counts(shape), _kernel_for(shape)
    kw = dict(x_scale=obs.max(), background=1.5, bounds=(0., np.inf))
    trace = []
    pd_linear_kl_restatement(obs, kernel, shape, "huber", 0.05, iters, trace=trace, **kw)

    def worst(k):
        (x1, p1, q1), (x0, p0, q0) = trace[k - 1], trace[k - 2]
        return max(np.sqrt(np.sum((x1 - x0) ** 2) / np.sum(x1 ** 2)),
                   np.sqrt((np.sum((p1 - p0) ** 2) + np.sum((q1 - q0) ** 2)) /
                           (np.sum(p1 ** 2) + np.sum(q1 ** 2))))
    changes = [worst(k) for k in range(every, iters + 1, every)]
    # a tolerance between the changes of two neighbouring checks, a factor 1.2 or more
    # apart, both larger than float32 resolves
    j = next(j for j in range(3, len(changes) - 1)
             if changes[j + 1] < changes[j] / 1.2 and
             min(changes[:j + 1]) > changes[j + 1] and changes[j + 1] > 1e-4)
    tol = float(np.sqrt(changes[j] * changes[j + 1]))
    stop = every * (j + 2)
    want, done = pd_linear_kl_restatement(obs, kernel, shape, "huber", 0.05, iters,
                                          tolerance=tol, check_every=every, **kw)
    assert done == stop < iters
    s = _pdl(nsol, obs, kernel, dtype, reg_type="huber", iterations=iters, tolerance=tol,
             check_every=every, background=1.5, bounds=(0., np.inf))
    s.run()
    assert s.get_iterations_done() == stop and s.get_stop_reason() == "tolerance"
    assert rel_l2(s.get_x(), want) <= _gate(dtype)


def test_a_device_mode_observer_sees_the_kl_run(nsol):
    from nsol_amd import observer as Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    shape, iters = (12, 10), 12
    obs, kernel = _counts(shape), _kernel_for(shape)
    truth = _counts(shape, 99).flatten()
    runs = {}
    for name, o in (("none", None), ("host", Observer.Observer()),
                    ("device", Observer.Observer(keep_iterates=False, every=5))):
        s = _pdl(nsol, obs, kernel, np.float64, iterations=iters, background=1.5)
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
    points = dev.get_observed_iterations()
    assert points == [0, 5, 10, 12]
    hv, dv = host.get_measures()["RMSE"], dev.get_measures()["RMSE"]
    assert np.allclose(dv, np.asarray(hv)[points], rtol=1e-10, atol=0)


def test_negative_counts_are_refused_on_the_device_too(nsol):
    from nsol_amd.device import to_device
    shape = (12, 10)
    obs = _counts(shape)
    bad = obs.copy()
    bad[3, 4] = -1.
    w = np.ones(shape)
    w[3, 4] = 0.
    with pytest.raises(ValueError, match="kl"):
        _pdl(nsol, bad, _kernel_for(shape), np.float32, b=to_device(bad.flatten(),
                                                                   np.float64))
    junk = bad.copy()
    junk[3, 4] = np.nan
    for b in (bad, junk):
        s = _pdl(nsol, obs, _kernel_for(shape), np.float32,
                 b=to_device(b.flatten(), np.float64),
                 weights=to_device(w.flatten(), np.float32), iterations=3)
        s.run()
        assert np.all(np.isfinite(s.get_x()))


# ---- the TGV solvers and the denoising prox
def _blur_of(kernel, shape):
    from scipy.ndimage import convolve
    return lambda x: convolve(np.asarray(x, np.float64).reshape(shape), kernel,
                              mode="wrap")


@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("dtype", BOTH)
def test_tgv_linear_solver_matches_the_restatement(nsol, iso, dtype):
    from nsol_amd.linear_operators import ConvolutionOperator
    shape = (12, 10)
    obs, kernel = _counts(shape), _kernel_for(shape)
    w, junk = _weights_over_nan(shape, obs)
    scale, bg = float(obs.max()), 1.5
    op = ConvolutionOperator(2, kernel)
    s = nsol.TGVPrimalDualLinearSolver(
        A=_wrapped(op, shape), A_adj=_wrapped(op, shape), b=junk.flatten(),
        x0=np.nan_to_num(junk).flatten(), dimension=2, alpha=0.05, beta=1.7,
        iterations=ITERS, x_scale=scale, dtype=dtype, data_loss="kl", background=bg,
        weights=w.flatten(), bounds=(0., np.inf), isotropic=iso)
    s.run()
    assert s.get_execution() == "fused" and s.get_background() == bg
    A = _blur_of(kernel, shape)
    want = tg.iterate_linear(A, A, junk / scale, np.nan_to_num(junk) / scale, ITERS, 0.05,
                             1.7, data_loss="kl", isotropic=iso, weights=w,
                             bounds=(0., np.inf), A_norm2=s.get_A_norm2(),
                             background=bg / scale)
    ex = rel_l2(s.get_x(), want["x"] * scale, "x")
    ew = rel_l2(s.get_w(), want["w"] * scale, "w")
    print("tgv linear kl", iso, np.dtype(dtype).name, ex, ew)
    assert ex <= _gate(dtype) and ew <= _gate(dtype)
    assert np.all(s.get_x() >= 0)


@pytest.mark.parametrize("shape", [(12, 10), (6, 7, 8)])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", BOTH)
def test_tgv_denoising_with_kl_matches_the_restatement(nsol, shape, weighted, dtype):
    from nsol_amd import ops
    obs = _counts(shape)
    w, junk = _weights_over_nan(shape, obs)
    b = junk if weighted else obs
    scale = float(obs.max())
    s = nsol.TGVPrimalDualSolver(b=b, x0=np.nan_to_num(b).flatten(), dimension=len(shape),
                                 alpha=0.05, beta=1.7, iterations=ITERS, x_scale=scale,
                                 dtype=dtype, data_loss="kl",
                                 weights=w.flatten() if weighted else None)
    before = ops.tgv_launches()
    s.run()
    assert ops.tgv_launches() - before == 2 * ITERS
    want = tg.iterate(b / scale, np.nan_to_num(b) / scale, ITERS, 0.05, 1.7,
                      data_loss="kl", weights=w if weighted else None)
    ex = rel_l2(s.get_x(), want["x"] * scale, "x")
    ew = rel_l2(s.get_w(), want["w"].reshape(-1) * scale, "w")
    print("tgv kl", shape, weighted, np.dtype(dtype).name, ex, ew)
    assert ex <= _gate(dtype) and ew <= _gate(dtype)
    x = s.get_x().reshape(shape)
    assert np.all(np.isfinite(x)) and np.all(x[w > 0] >= 0 if weighted else x >= 0)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", BOTH)
def test_primal_dual_solver_with_prox_kl_denoising(nsol, weighted, dtype):
    """PrimalDualSolver does not plan this prox: the run goes through the loop of
    separate kernels, against that loop restated."""
    import nsol_amd.linear_operators as LO
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd.proximal_operators import ProximalOperators as prox
    shape = (12, 10)
    obs = _counts(shape)
    w, junk = _weights_over_nan(shape, obs)
    b = (junk if weighted else obs).flatten()
    scale, alpha, L2 = float(obs.max()), 0.05, 8.
    grad_op, grad_adj_op = LO.LinearOperators2D().get_gradient_operators()
    Z = grad_op(obs).shape
    D = lambda x: grad_op(x.reshape(*shape)).flatten()
    D_adj = lambda x: grad_adj_op(x.reshape(*Z)).flatten()
    if weighted:
        pf = lambda x, tau: prox.prox_kl_denoising_weighted(x, tau, b, w.flatten(),
                                                            x_scale=scale)
    else:
        pf = lambda x, tau: prox.prox_kl_denoising(x, tau, x0=b, x_scale=scale)
    s = pd.PrimalDualSolver(prox_f=pf, prox_g_conj=prox.prox_tv_conj, B=D, B_conj=D_adj,
                            L2=L2, x0=np.nan_to_num(b), alpha=alpha, iterations=ITERS,
                            x_scale=scale, dtype=dtype)
    assert s.plan() is None
    s.run()
    assert s.get_execution() == "device"
    sig, ta, th = pd.step_schedule("ALG2", L2, 1. / alpha, ITERS)
    bt = b.reshape(shape) / scale
    x = np.nan_to_num(b).reshape(shape) / scale
    xbar, p = x.copy(), np.zeros((2,) + shape)
    for i in range(ITERS):
        p = np.clip(p + sig[i] * grad(xbar), -1., 1.)
        t = ta[i] * (1. / alpha)
        xn = vn.prox_kl(x - ta[i] * grad_adj(p), bt, t * w if weighted else t,
                        w if weighted else None)
        xbar = xn + th[i] * (xn - x)
        x = xn
    err = rel_l2(s.get_x(), (x * scale).reshape(-1), np.dtype(dtype).name)
    print("prox_kl_denoising", weighted, np.dtype(dtype).name, err)
    assert err <= _gate(dtype), err
    # NumPy in, NumPy out: the same prox through the host round trip
    u = np.linspace(-1., 2., 120)
    got = prox.prox_kl_denoising(u, 0.7, x0=obs.flatten(), x_scale=scale)
    assert isinstance(got, np.ndarray)
    assert relative_error(got, vn.prox_kl(u, obs.flatten() / scale, 0.7)) <= F64_TOL


# ------------------------------------------------------------ 5. the stacks
@pytest.fixture
def data_side(monkeypatch):
    """Calls of the data term's update per wrapper, those the library took."""
    from nsol_amd import ops
    calls = dict(stacked_kl=0, single_kl=0, stacked=0, single=0)

    def count(name, key):
        real = getattr(ops, name)

        def counted(*a, **k):
            out = real(*a, **k)
            calls[key] += 1 if key.startswith("single") else bool(out)
            return out
        monkeypatch.setattr(ops, name, counted)
    count("pdl_stack_dual_data_kl", "stacked_kl")
    count("pdl_dual_data_kl", "single_kl")
    count("pdl_stack_dual_data", "stacked")
    count("pdl_dual_data", "single")
    return calls


def _bits(t):
    return t.cpu().numpy().view(np.uint8)


def _members(shape, P=3, bg=1.5):
    """(observation, weights, alpha) per member: one common x_scale, so that the members
    meet one scaled background."""
    out = []
    for m in range(P):
        obs = _counts(shape, seed=sum(shape) + 7 * m)
        w, junk = _weights_over_nan(shape, obs)
        out.append((junk, w, [0.05, 0.02, 0.2][m]))
    return out


STACK_CASES = [((12, 10), None, np.float64), ((12, 10), None, np.float32),
               ((9, 5, 16), 4., np.float64)]


def _stack_operator(shape, var):
    from nsol_amd import linear_operators as LO
    from nsol_amd.linear_operators import ConvolutionOperator
    if var is None:
        return ConvolutionOperator(len(shape), gaussian_kernel(len(shape), 1.))
    return LO.LinearOperators3D().get_gaussian_blurring_operators(np.diag([var] * 3))[0]


@pytest.mark.parametrize("shape, var, dtype", STACK_CASES)
def test_linear_batch_of_kl_members(nsol, data_side, shape, var, dtype):
    from nsol_amd import ops
    from nsol_amd.linear_stack import launches_per_iteration
    members = _members(shape)
    P = len(members)

    def make(bg=1.5):
        return [_pdl(nsol, junk, None, dtype, op=_stack_operator(shape, var), alpha=a,
                     weights=w.flatten(), background=bg, bounds=(0., np.inf),
                     reg_type="huber", x_scale=30.)
                for junk, w, a in members]
    own, solvers = make(), make()
    for f in own:
        f.run()
    assert data_side == dict(stacked_kl=0, single_kl=P * ITERS, stacked=0, single=0)
    want = (6, 6 * P) if var is None else (2 * P + 2, 4 * P)
    assert launches_per_iteration(solvers[0], P) == want
    batch = nsol.PrimalDualLinearBatch(solvers)
    stack0, single0 = ops.pdl_stack_launches(), ops.pdl_launches()
    batch.run()
    assert batch.get_execution() == ["stacked"] * P and batch.get_group_size() == P
    assert ops.pdl_stack_launches() - stack0 == ITERS and ops.pdl_launches() == single0
    assert data_side == dict(stacked_kl=ITERS, single_kl=P * ITERS, stacked=0, single=0)
    for m, (s, f) in enumerate(zip(solvers, own)):
        assert np.array_equal(_bits(s._x), _bits(f._x)), m
        assert np.array_equal(s.get_x(), f.get_x()) and np.all(s.get_x() >= 0)
    # a member with another background is a group of its own: it runs on its own
    mixed = make()[:2] + make(bg=0.5)[2:]
    batch = nsol.PrimalDualLinearBatch(mixed)
    batch.run()
    assert batch.get_execution() == ["stacked"] * 2 + ["sequential"]
    lone = make(bg=0.5)[2]
    lone.run()
    assert np.array_equal(_bits(mixed[2]._x), _bits(lone._x))
    assert np.array_equal(_bits(mixed[0]._x), _bits(own[0]._x))


@pytest.mark.parametrize("shape, var, dtype", STACK_CASES)
def test_linear_sweep_of_kl_members(nsol, data_side, shape, var, dtype):
    from nsol_amd import ops
    junk, w, _ = _members(shape)[0]
    op = _stack_operator(shape, var)
    alphas = [0.02, 0.05, 0.2]
    kw = dict(weights=w.flatten(), background=1.5, bounds=(0., np.inf), data_loss="kl",
              iterations=ITERS, x_scale=30., dtype=dtype)
    sweep = nsol.PrimalDualLinearSweep(_wrapped(op, shape), _wrapped(op, shape),
                                       junk.flatten(), np.nan_to_num(junk).flatten(),
                                       len(shape), parameters={"alpha": alphas}, **kw)
    stack0 = ops.pdl_stack_launches()
    sweep.run()
    assert sweep.get_execution() == "stacked" and sweep.get_group_size() == 3
    assert ops.pdl_stack_launches() - stack0 == ITERS
    assert data_side == dict(stacked_kl=ITERS, single_kl=0, stacked=0, single=0)
    X = sweep.get_x_all_device()
    for m, alpha in enumerate(alphas):
        s = _pdl(nsol, junk, None, dtype, op=op, alpha=alpha, **{
            k: v for k, v in kw.items() if k not in ("data_loss", "dtype")})
        s.run()
        assert np.array_equal(sweep.get_x(m), s.get_x()), m
        assert np.array_equal(_bits(X[m]), _bits(s.get_x_device())), m


def _tgv_lin(nsol, junk, w, op, dtype, alpha, beta, bg=1.5):
    shape = junk.shape
    return nsol.TGVPrimalDualLinearSolver(
        A=_wrapped(op, shape), A_adj=_wrapped(op, shape), b=junk.flatten(),
        x0=np.nan_to_num(junk).flatten(), dimension=len(shape), alpha=alpha, beta=beta,
        iterations=ITERS, x_scale=30., dtype=dtype, data_loss="kl", background=bg,
        weights=w.flatten(), bounds=(0., np.inf))


@pytest.mark.parametrize("shape, var, dtype", STACK_CASES)
def test_tgv_linear_batch_and_sweep_of_kl_members(nsol, data_side, shape, var, dtype):
    from nsol_amd import ops
    from nsol_amd.tgv_linear_stack import launches_per_iteration
    members = _members(shape)
    P = len(members)
    betas = [1.7, 0.8, 3.0]

    def make(bg=1.5):
        return [_tgv_lin(nsol, junk, w, _stack_operator(shape, var), dtype, a, betas[m], bg)
                for m, (junk, w, a) in enumerate(members)]
    own, solvers = make(), make()
    for f in own:
        f.run()
    want = (7, 7 * P) if var is None else (2 * P + 3, 5 * P)
    assert launches_per_iteration(solvers[0], P) == want
    calls0 = dict(data_side)
    batch = nsol.TGVPrimalDualLinearBatch(solvers)
    before = ops.tgv_stack_launches(), ops.tgv_launches()
    batch.run()
    assert batch.get_execution() == ["stacked"] * P and batch.get_group_size() == P
    assert ops.tgv_stack_launches() - before[0] == 2 * ITERS
    assert ops.tgv_launches() == before[1]
    assert data_side == dict(calls0, stacked_kl=ITERS)
    for m, (s, f) in enumerate(zip(solvers, own)):
        assert np.array_equal(_bits(s._x), _bits(f._x)), m
        assert np.array_equal(_bits(s._w), _bits(f._w)), m
        assert np.array_equal(s.get_w(), f.get_w()) and np.abs(s.get_w()).max() > 0
    mixed = make()[:2] + make(bg=0.5)[2:]
    batch = nsol.TGVPrimalDualLinearBatch(mixed)
    batch.run()
    assert batch.get_execution() == ["stacked"] * 2 + ["sequential"]
    # the sweep: one observation, (alpha, beta) pairs
    junk, w, _ = members[0]
    op = _stack_operator(shape, var)
    grid = {"alpha": [0.05, 0.2], "beta": [0.8, 1.7]}
    sweep = nsol.TGVPrimalDualLinearSweep(
        A=_wrapped(op, shape), A_adj=_wrapped(op, shape), b=junk.flatten(),
        x0=np.nan_to_num(junk).flatten(), dimension=len(shape), parameters=grid,
        iterations=ITERS, x_scale=30., dtype=dtype, data_loss="kl", background=1.5,
        weights=w.flatten(), bounds=(0., np.inf))
    before = ops.tgv_stack_launches()
    sweep.run()
    assert sweep.get_execution() == "stacked" and sweep.get_group_size() == 4
    assert ops.tgv_stack_launches() - before == 2 * ITERS
    for m, par in enumerate(sweep.get_parameters()):
        s = _tgv_lin(nsol, junk, w, op, dtype, par["alpha"], par["beta"])
        s.run()
        assert np.array_equal(sweep.get_x(m), s.get_x()), m
        assert np.array_equal(sweep.get_w(m), s.get_w()), m


def test_tgv_denoising_stacks_send_kl_members_to_their_own_runs(nsol):
    """Their stacked kernels hold ell2 and ell1 only: a kl member that reached them would
    run as ell2."""
    from nsol_amd import ops
    shape = (12, 10)
    obs = [_counts(shape, seed=40 + m) for m in range(3)]

    def make(loss):
        return [nsol.TGVPrimalDualSolver(b=o, x0=o.flatten(), dimension=2, alpha=0.05,
                                         iterations=ITERS, x_scale=30., dtype=np.float64,
                                         data_loss=loss) for o in obs]
    own, solvers = make("kl"), make("kl")
    for f in own:
        f.run()
    batch = nsol.TGVPrimalDualBatch(solvers)
    before = ops.tgv_stack_launches()
    batch.run()
    assert batch.get_execution() == ["sequential"] * 3
    assert ops.tgv_stack_launches() == before
    ell2 = make("ell2")
    for f in ell2:
        f.run()
    for s, f, e in zip(solvers, own, ell2):
        assert np.array_equal(s.get_x(), f.get_x())
        assert not np.array_equal(s.get_x(), e.get_x())
    sweep = nsol.TGVPrimalDualSweep(obs[0], obs[0].flatten(), 2,
                                    {"alpha": [0.05, 0.2]}, iterations=ITERS, x_scale=30.,
                                    dtype=np.float64, data_loss="kl")
    sweep.run()
    assert sweep.get_execution() == "sequential" and ops.tgv_stack_launches() == before
    assert np.array_equal(sweep.get_x(0), own[0].get_x())


# ------------------------------------------------------------ 6. the command line
def test_cli_kl_equals_the_api_run(nsol, tmp_path, capsys):
    from nsol_amd import nifti
    from nsol_amd.application import run_deconvolution
    from nsol_amd.data_reader import DataReader
    vol = _counts((12, 16, 20), seed=3)
    nii, out = str(tmp_path / "obs.nii.gz"), str(tmp_path / "out.nii.gz")
    nifti.write(nii, vol)
    reader = DataReader(nii)
    reader.read_data()
    data = reader.get_data()
    base = ["--observation", nii, "--result", out, "--solver", "PDL", "--iterations", "12",
            "--blur", "1.0", "--data-loss", "kl", "--background", "0.5", "--nonnegative"]
    assert run_deconvolution.main(base + ["--alpha", "0.03"]) == 0
    capsys.readouterr()
    s = run_deconvolution.build_solver(data, np.ones(3), 1.0, "TVL2", "PDL", 0.03, 12,
                                       dtype=np.float32, pdl_data_loss="kl",
                                       background=0.5, nonnegative=True)
    assert s.get_data_loss() == "kl" and s.get_background() == 0.5
    s.run()
    got, _, _ = nifti.read(out)
    assert got.min() >= 0
    assert rel_l2(got, s.get_x().reshape(data.shape)) < 1e-6         # float32 file
    # TGV
    assert run_deconvolution.main(base + ["--alpha", "0.03", "--reconstruction-type",
                                          "TGVL2", "--beta", "1.5"]) == 0
    capsys.readouterr()
    t = run_deconvolution.build_solver(data, np.ones(3), 1.0, "TGVL2", "PDL", 0.03, 12,
                                       dtype=np.float32, pdl_data_loss="kl",
                                       background=0.5, nonnegative=True, beta=1.5)
    t.run()
    got, _, _ = nifti.read(out)
    assert rel_l2(got, t.get_x().reshape(data.shape)) < 1e-6
    # a sweep over two alphas
    rdir = tmp_path / "sweep"
    assert run_deconvolution.main(base + ["--alpha", "0.03", "0.1", "--result-dir",
                                          str(rdir)]) == 0
    text = capsys.readouterr().out
    assert "stacked" in text and "sequentially" not in text
    first = run_deconvolution.member_result_path(str(rdir), out, 0.03)
    got, _, _ = nifti.read(first)
    assert rel_l2(got, s.get_x().reshape(data.shape)) < 1e-6
