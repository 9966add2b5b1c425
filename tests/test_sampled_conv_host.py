"""CPU-only side of the blur-and-sample operator pair (SampledConvolutionOperator,
nsol_corr_axis_down_* / nsol_corr_axis_up_*): the NumPy restatement of the per-axis
semantics that the GPU tests are held to, its own check against the dense matrix and
scipy.ndimage, the restatement of PrimalDualLinearSolver's iteration on the sampled
operator, and the host logic -- shapes, refusals, tracing, the operator norm, the
declared symbols and the command-line arguments."""
import numpy as np
import pytest

from test_pd_isotropic_host import project_iso
from test_pd_linear_host import _widths, dual_data, gaussian_kernel, grad, grad_adj

MODES = ("wrap", "constant")


# ------------------------------------------------------------------ yardstick
def sampled_extent(length, f, o):
    return -((o - length) // f)


def sampled_down(x, w, c, mode, f, o, axis, dtype=np.float64):
    """out[j] = sum_t w[t] x[map(o + j f - c + t)] along `axis`, j in [0, m): the sum
    over t upwards, every product and sum rounded to `dtype`."""
    x = np.moveaxis(np.asarray(x, dtype=dtype), axis, -1)
    w = np.asarray(w, dtype=dtype)
    length = x.shape[-1]
    m = sampled_extent(length, f, o)
    j = np.arange(m)
    acc = np.zeros(x.shape[:-1] + (m,), dtype=dtype)
    for t in range(w.size):
        pos = o + j * f - c + t
        if mode == "wrap":
            ok, pos = np.ones(m, bool), pos % length
        else:
            ok = (pos >= 0) & (pos < length)
            pos = np.clip(pos, 0, length - 1)
        acc = acc + w[t] * np.where(ok, x[..., pos], dtype(0))
    return np.moveaxis(acc, -1, axis)


def sampled_up(q, w, c, mode, f, o, axis, length, dtype=np.float64):
    """out[i] = sum_t w[t] q[(P - o) / f] over the t with P >= o, f | P - o and
    (P - o) / f < m, P = (i + c - t) mod length (wrap) or i + c - t inside [0, length)
    (constant); i in [0, length)."""
    q = np.moveaxis(np.asarray(q, dtype=dtype), axis, -1)
    w = np.asarray(w, dtype=dtype)
    m = sampled_extent(length, f, o)
    assert q.shape[-1] == m
    i = np.arange(length)
    acc = np.zeros(q.shape[:-1] + (length,), dtype=dtype)
    for t in range(w.size):
        P = i + c - t
        if mode == "wrap":
            ok, P = np.ones(length, bool), P % length
        else:
            ok = (P >= 0) & (P < length)
        ok = ok & (P >= o) & ((P - o) % f == 0) & ((P - o) // f < m)
        k = np.clip((P - o) // f, 0, m - 1)
        acc = acc + w[t] * np.where(ok, q[..., k], dtype(0))
    return np.moveaxis(acc, -1, axis)


def convolve_params(kernel):
    """(per-axis correlation taps, centres) of a rank-1 ndimage.convolve kernel whose
    per-axis factors are `kernel` (a list of 1-D arrays): the flipped taps and the
    centre ConvolutionOperator derives."""
    taps = [np.asarray(k, np.float64)[::-1] for k in kernel]
    centres = [k.size // 2 - (1 if k.size % 2 == 0 else 0) for k in taps]
    return taps, centres


def pass_order(factors):
    """Axes with f > 1 by falling factor (ties in axis order), then the others."""
    d = len(factors)
    return sorted((a for a in range(d) if factors[a] > 1),
                  key=lambda a: (-factors[a], a)) + \
        [a for a in range(d) if factors[a] == 1]


def sampled_forward(x, kernel, mode, factors, offsets, dtype=np.float64):
    """A x for per-axis ndimage.convolve factors `kernel` (list of 1-D arrays), in the
    operator's pass order."""
    taps, centres = convolve_params(kernel)
    for a in pass_order(factors):
        x = sampled_down(x, taps[a], centres[a], mode, factors[a], offsets[a], a, dtype)
    return x


def sampled_adjoint(q, kernel, mode, factors, offsets, fine_shape, dtype=np.float64):
    taps, centres = convolve_params(kernel)
    for a in reversed(pass_order(factors)):
        q = sampled_up(q, taps[a], centres[a], mode, factors[a], offsets[a], a,
                       fine_shape[a], dtype)
    return q


def sampled_steps(fine_shape, kernel, spacing=None):
    norm = float(np.prod([np.sum(np.abs(k)) for k in kernel]))
    L2 = sum(4. * w * w for w in _widths(fine_shape, spacing)) + norm ** 2
    return L2, 1. / np.sqrt(L2), 1. / np.sqrt(L2)


def change_ratios(new, old):
    """(r_x, r_dual) of PrimalDualLinearSolver's stopping rule between two states
    (x, p, q); old = None: the start (p = q = 0; x0 given as old_x)."""
    (x1, p1, q1), (x0, p0, q0) = new, old
    return (np.sqrt(np.sum((x1 - x0) ** 2) / np.sum(x1 ** 2)),
            np.sqrt((np.sum((p1 - p0) ** 2) + np.sum((q1 - q0) ** 2)) /
                    (np.sum(p1 ** 2) + np.sum(q1 ** 2))))


def pd_linear_sampled_restatement(obs, kernel, fine_shape, factors, offsets, reg, data,
                                  alpha, iters, x0, mode="wrap", weights=None,
                                  bounds=None, iso=False, spacing=None, x_scale=1.,
                                  gamma=0.05, trace=None):
    """NumPy float64 statement of PrimalDualLinearSolver's iteration with A the sampled
    blur (sampled_forward) and A^T its transpose (sampled_adjoint).  obs, weights: the
    coarse data; x0: the start on the fine grid.  trace: receives (x, p, q) per
    iteration.  Returns x * x_scale with the fine shape."""
    fine_shape = tuple(fine_shape)
    d = len(fine_shape)
    coarse = tuple(sampled_extent(s, f, o)
                   for s, f, o in zip(fine_shape, factors, offsets))
    A = lambda v: sampled_forward(v, kernel, mode, factors, offsets)
    At = lambda v: sampled_adjoint(v, kernel, mode, factors, offsets, fine_shape)
    x_scale = float(x_scale)
    bt = np.asarray(obs, np.float64).reshape(coarse) / x_scale
    w = np.ones(coarse) if weights is None else \
        np.asarray(weights, np.float64).reshape(coarse)
    lo, hi = (-np.inf, np.inf) if bounds is None else bounds
    _, tau, sigma = sampled_steps(fine_shape, kernel, spacing)
    lmbda, theta = 1. / float(alpha), 1.
    c = lmbda * w
    x = np.asarray(x0, np.float64).reshape(fine_shape) / x_scale
    xbar = x.copy()
    p = np.zeros((d,) + fine_shape)
    q = np.zeros(coarse)
    hden = 1. + sigma * gamma if reg == "huber" else None
    for _ in range(iters):
        pq = p + sigma * grad(xbar, spacing)
        if iso:
            p = project_iso(pq.reshape(-1), d, hden).reshape(pq.shape)
        else:
            p = np.clip(pq / hden if hden is not None else pq, -1., 1.)
        with np.errstate(invalid="ignore"):
            v = q + sigma * (A(xbar) - bt)
        q = dual_data(v, c, sigma, w, data)
        xn = np.clip(x - tau * (grad_adj(p, spacing) + At(q)), lo, hi)
        xbar = xn + theta * (xn - x)
        x = xn
        if trace is not None:
            trace.append((x.copy(), p.copy(), q.copy()))
    return x * x_scale


def numpy_start(obs, kernel, mode, factors, offsets, fine_shape):
    """A^T b / A^T 1, 0 where A^T 1 == 0."""
    num = sampled_adjoint(obs, kernel, mode, factors, offsets, fine_shape)
    den = sampled_adjoint(np.ones_like(obs), kernel, mode, factors, offsets, fine_shape)
    out = np.zeros_like(num)
    np.divide(num, den, out=out, where=den != 0)
    return out


# ------------------------------------------------------------------ the semantics
LENGTHS = (1, 2, 3, 5, 7, 8, 13, 16)


def _centres(ntaps):
    """The centre ndimage.convolve gives, and the two ends (off-centre taps)."""
    return sorted({ntaps // 2 - (1 if ntaps % 2 == 0 else 0), 0, ntaps - 1})


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("length", LENGTHS)
def test_up_is_the_transpose_of_down_and_down_is_correlate_then_slice(length, mode):
    from scipy.ndimage import correlate1d
    rng = np.random.default_rng(length)
    x = rng.standard_normal((3, length))
    worst = 0.
    for f in range(1, 5):
        for o in range(min(f, length)):
            m = sampled_extent(length, f, o)
            assert m == len(range(o, length, f))
            for ntaps in range(1, 20):
                w = rng.standard_normal(ntaps)
                for c in _centres(ntaps):
                    D = sampled_down(np.eye(length), w, c, mode, f, o, 0)
                    U = sampled_up(np.eye(m), w, c, mode, f, o, 0, length)
                    assert D.shape == (m, length) and U.shape == (length, m)
                    assert np.array_equal(U, D.T), (f, o, ntaps, c)
                    # the restatement applied to data is that matrix
                    got = sampled_down(x, w, c, mode, f, o, 1)
                    worst = max(worst, np.max(np.abs(got - x.dot(D.T))))
                    ref = correlate1d(x, w, axis=1, mode=mode,
                                      origin=c - ntaps // 2)[:, o::f]
                    worst = max(worst, np.max(np.abs(got - ref)))
    print("worst difference", worst)
    assert worst <= 1e-13


def test_nd_restatement_is_convolve_then_slice():
    from scipy.ndimage import convolve
    rng = np.random.default_rng(3)
    shape, factors, offsets = (6, 9, 13), (3, 1, 2), (2, 0, 1)
    kernel = [rng.standard_normal(n) for n in (5, 4, 3)]
    dense = np.einsum("i,j,k->ijk", *kernel)
    x = rng.standard_normal(shape)
    for mode in MODES:
        got = sampled_forward(x, kernel, mode, factors, offsets)
        ref = convolve(x, dense, mode=mode)[2::3, 0::1, 1::2]
        assert got.shape == ref.shape == (2, 9, 6)
        assert np.max(np.abs(got - ref)) <= 1e-13
        y = rng.standard_normal(got.shape)
        lhs = np.vdot(got, y)
        rhs = np.vdot(x, sampled_adjoint(y, kernel, mode, factors, offsets, shape))
        assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(got) * np.linalg.norm(y)


# ------------------------------------------------------------------ the library
def test_the_new_symbols_are_declared_and_the_library_cross_compiles():
    import os
    from nsol_amd import _lib, build
    sym = _lib.declared_symbols()
    for name in ("nsol_corr_axis_down_f32", "nsol_corr_axis_down_f64",
                 "nsol_corr_axis_up_f32", "nsol_corr_axis_up_f64"):
        assert name in sym, name
        assert len(sym[name][1]) == 13
    assert "nsol_sample.hip" in build.SOURCES
    lib = build.build_library()
    assert os.path.exists(lib)
    import ctypes
    so = ctypes.CDLL(lib)
    for name in sym:
        assert hasattr(so, name), name


# ------------------------------------------------------------------ the operators
def _op(dim=2, factors=(2, 3), offsets=None, mode="wrap", kernel=None):
    from nsol_amd.linear_operators import SampledConvolutionOperator
    kernel = gaussian_kernel(dim, 1.) if kernel is None else kernel
    return SampledConvolutionOperator(dim, kernel, factors, offsets, mode)


def test_out_shapes():
    A = _op()
    assert A._out_shape((9, 130)) == (5, 44)
    assert A._out_shape((8, 129)) == (4, 43)
    A = _op(offsets=(1, 2))
    assert A._out_shape((9, 130)) == (4, 43)
    assert A._out_shape((2, 3)) == (1, 1)
    with pytest.raises(ValueError):
        A._out_shape((1, 130))                  # the offset is outside the axis
    A = _op(3, (3, 1, 2), (2, 0, 1))
    assert A._out_shape((6, 9, 130)) == (2, 9, 65)
    assert A.factors == (3, 1, 2) and A.offsets == (2, 0, 1)
    # the adjoint is built with the fine shape; without one it maps to f * m
    assert A.adjoint()._out_shape((2, 9, 65)) == (6, 9, 130)
    assert A.adjoint((6, 9, 129))._out_shape((2, 9, 64)) == (6, 9, 129)
    with pytest.raises(ValueError):
        A.adjoint((6, 9, 129))._out_shape((2, 9, 65))
    with pytest.raises(ValueError):
        _op().adjoint((9, 131))._out_shape((5, 45))


def test_the_operator_is_no_convolution_operator():
    from nsol_amd.linear_operators import (ConvolutionOperator, DeviceOperator,
                                           SampledConvolutionAdjointOperator)
    A = _op()
    At = A.adjoint((9, 130))
    assert isinstance(A, DeviceOperator) and isinstance(At, DeviceOperator)
    assert not isinstance(A, ConvolutionOperator)
    assert not isinstance(At, ConvolutionOperator)
    assert isinstance(At, SampledConvolutionAdjointOperator)
    assert A.kind == "sampled_conv" and At.kind == "sampled_conv_adj"
    from nsol_amd.linear_stack import member_key
    assert member_key(_solver()) is None


@pytest.mark.parametrize("kw", [
    dict(mode="nearest"), dict(mode="reflect"), dict(mode="mirror"),
    dict(factors=(2,)), dict(factors=(2, 3, 1)), dict(factors=(0, 1)),
    dict(factors=(2, -1)), dict(factors=(2.5, 1)), dict(factors=None, offsets=(1, 0)),
    dict(offsets=(2, 0)), dict(offsets=(0, -1)), dict(offsets=(0,)),
    dict(kernel=np.array([[1., 2.], [3., 5.]])),                  # not separable
    dict(kernel=np.multiply.outer(np.ones(131), np.ones(3))),     # over 129 taps
    dict(kernel=np.ones(3)),                                      # wrong rank
], ids=lambda kw: "-".join("%s" % k for k in kw))
def test_bad_operator_arguments_raise(kw):
    args = dict(dim=2, factors=(2, 3))
    args.update(kw)
    with pytest.raises(ValueError):
        _op(**args)


def test_factories():
    from nsol_amd.linear_operators import (LinearOperators2D,
                                           SampledConvolutionAdjointOperator,
                                           SampledConvolutionOperator)
    lo = LinearOperators2D()
    A, At = lo.get_sampled_convolution_operators(gaussian_kernel(2, 1.), (2, 2))
    assert isinstance(A, SampledConvolutionOperator) and A.mode == "wrap"
    assert isinstance(At, SampledConvolutionAdjointOperator) and At.forward is A
    A, At = lo.get_sampled_gaussian_blurring_operators(np.diag([1., 1.]), (2, 1), (1, 0))
    assert A.factors == (2, 1) and A.offsets == (1, 0)
    assert A.kernel.shape == (7, 7) and abs(A.kernel.sum() - 1.) <= 1e-14
    with pytest.raises(ValueError):
        lo.get_sampled_convolution_operators(gaussian_kernel(2, 1.), (2, 2),
                                             mode="reflect")


def test_trace_operator_sees_the_pair_through_lambdas():
    from nsol_amd.symbolic import trace_operator
    fine, coarse = (9, 130), (5, 44)
    A = _op()
    At = A.adjoint(fine)
    d = trace_operator(lambda x: A(x.reshape(fine)).flatten(), 9 * 130)
    assert d[0] == "sampled_conv" and d[1] is A and tuple(d[2]) == fine
    d = trace_operator(lambda q: At(q.reshape(*coarse)).flatten(), 5 * 44)
    assert d[0] == "sampled_conv_adj" and d[1] is At and tuple(d[2]) == coarse


# ------------------------------------------------------------------ the solver
def _solver(fine=(9, 130), factors=(2, 3), offsets=None, **kw):
    import nsol_amd
    A = _op(len(fine), factors, offsets)
    At = A.adjoint(fine)
    coarse = A._out_shape(fine)
    b = 1. + np.arange(int(np.prod(coarse)), dtype=float)
    x0 = np.ones(int(np.prod(fine)))
    args = dict(A=lambda x: A(x.reshape(*fine)).flatten(),
                A_adj=lambda q: At(q.reshape(*coarse)).flatten(), b=b, x0=x0,
                dimension=len(fine))
    args.update(kw)
    return nsol_amd.PrimalDualLinearSolver(**args)


def test_solver_on_the_sampled_operator_needs_no_A_norm2():
    s = _solver()
    assert s.get_execution() == "fused"
    k = gaussian_kernel(2, 1.)
    assert s.get_A_norm2() == float(np.sum(np.abs(k))) ** 2
    assert s.get_shape() == (9, 130)
    assert abs(s.get_L2() - (8. + s.get_A_norm2())) <= 1e-12
    # signed taps: Young's bound is the sum of the absolute values
    taps = np.multiply.outer(np.array([1., -3., 1.]), np.array([0.5, 0.5, -2.]))
    from nsol_amd.linear_operators import SampledConvolutionOperator
    import nsol_amd
    A = SampledConvolutionOperator(2, taps, (1, 2))
    At = A.adjoint((4, 6))
    s = nsol_amd.PrimalDualLinearSolver(
        lambda x: A(x.reshape(4, 6)).flatten(), lambda q: At(q.reshape(4, 3)).flatten(),
        np.ones(12), np.ones(24), 2)
    assert s.get_A_norm2() == 225. and s.get_execution() == "fused"
    # weights live on the m sampled values
    _solver(weights=np.ones(5 * 44))
    with pytest.raises(ValueError):
        _solver(weights=np.ones(9 * 130))
    # a foreign callable still needs the bound
    with pytest.raises(ValueError):
        nsol_amd.PrimalDualLinearSolver(lambda x: x[::2], lambda q: np.repeat(q, 2),
                                        np.ones(4), np.ones(8), 1)


def test_sampled_start_is_refused_on_the_wrong_grid():
    from nsol_amd.linear_operators import sampled_start
    A = _op()
    with pytest.raises(ValueError):
        sampled_start(A.adjoint((9, 130)), np.ones((5, 44)), (10, 132))


# ------------------------------------------------------------------ command line
def _cli(argv):
    from nsol_amd.application import run_deconvolution
    return run_deconvolution.main(["--observation", "o.nii.gz", "--result", "r.nii.gz"] +
                                  argv)


@pytest.mark.parametrize("argv", [
    ["--solver", "PDL", "--upsample", "2", "2", "--slice-wise"],
    ["--solver", "PDL", "--upsample", "2", "2", "--result-dir", "d"],
    ["--solver", "PD", "--upsample", "2", "2"],
    ["--solver", "ADMM", "--upsample", "2", "2"],
    ["--solver", "PDL", "--sample-offset", "1", "1"],
    ["--solver", "PDL", "--upsample", "2", "2", "--sample-offset", "2", "0"],
    ["--solver", "PDL", "--upsample", "2", "2", "--sample-offset", "1"],
    ["--solver", "PDL", "--upsample", "0", "2"],
], ids=lambda a: " ".join(a))
def test_cli_refusals_exit_with_status_2(capsys, argv):
    with pytest.raises(SystemExit) as e:
        _cli(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--upsample" in err or "--sample-offset" in err


def test_cli_wrong_number_of_factors(tmp_path, capsys):
    from nsol_amd.application import run_deconvolution
    path = str(tmp_path / "obs.npy")
    np.save(path, np.ones((4, 6)))
    with pytest.raises(SystemExit) as e:
        run_deconvolution.main(["--observation", path, "--result",
                                str(tmp_path / "r.npy"), "--solver", "PDL", "--upsample",
                                "2", "2", "2"])
    assert e.value.code == 2 and "one factor per axis" in capsys.readouterr().err


def test_fine_grid_handles_the_axis_order():
    from nsol_amd.application.run_deconvolution import fine_grid
    # spacing[0] belongs to the LAST array axis, the factors are per array axis
    shape, spacing = fine_grid((4, 6, 8), (1., 2., 3.), (4, 1, 2))
    assert shape == (16, 6, 16)
    assert np.allclose(spacing, (0.5, 2., 0.75))
    with pytest.raises(ValueError):
        fine_grid((4, 6), (1., 1.), (2,))
