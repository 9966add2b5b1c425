"""The convolution kernels of nsol_amd/csrc/nsol_conv.hip at every boundary mode, tap
count and extent, through `ConvolutionOperator` and `ops.corr_axis` / `ops.corr_dense`
(ctypes -> C ABI), against `oracle.nsol_oracle.convolve_nd` in float64.  The oracle, the
case grid and the Python statement of the index rule are pinned against scipy.ndimage
in tests/test_conv_host.py.  Needs a real MI355X.

Which kernel a case reaches:
  k_corr_dense              kernels that are no outer product, or with an axis over 129 taps
  k_corr_axis               outer products under constant / nearest / reflect / mirror; under
                            wrap with an even or long (> 25) tap count, rows that are not
                            whole 16-byte vectors, or operands off the 16-byte grid
  k_corr_strided_wrap<NT>   wrap, odd centred NT in 3..25, array axis 0 or 1
  k_corr_x_wrap<NT>         the same along the rows
  the one-pass blur         3-D, wrap, the same odd tap count <= 17 on all three axes

Bounds: float64 rel-L2 <= 1e-12 everywhere.  float32 Gaussians 1e-6 (2e-6 from 17 taps).
float32 random kernels: at most 4 x the error of the oracle evaluated in float32
(test_conv_host.convolve_f32), floor 1e-6.  Observed over the module's 696 float32
comparisons: largest GPU / reference ratio 1.60 (1.7e-7 against 1.1e-7, an 8 x 9-tap outer
product on a 3 x 2 image); largest GPU error 3.4e-7, so the floor is the gate that binds;
the float32 reference itself reaches 1.0e-6 (it rounds more terms than the passes do).
Largest float64 error 2.0e-15.  One-hot kernels and guard elements: exact."""
import numpy as np
import pytest

from conftest import rel_l2
from test_conv_host import (GRID, GRID_IDS, MODES, all_hot_positions, convolve_f32,
                            expect_separable, make_case, map_index_py, rank1_edge_kernels,
                            take_mapped, wrap_adjoint_pair)

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12
F32_FLOOR = 1e-6
F32_FACTOR = 4.0
DTYPES = (np.float64, np.float32)
ODD_NT = tuple(range(3, 26, 2))


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()                      # fails loudly if the .so is missing
    return nsol_amd


def _conv(kernel, mode):
    import nsol_amd.linear_operators as LO
    return LO.ConvolutionOperator(np.ndim(kernel), kernel, mode)


def _lo3():
    import nsol_amd.linear_operators as LO
    return LO.LinearOperators3D()


def _torch_dtype(dtype):
    import torch
    return torch.float32 if dtype == np.float32 else torch.float64


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda().view(-1)


def _axis_kernel(taps, axis3):
    """The 3-D kernel ndimage.convolve needs for a correlation with `taps` along one
    axis (convolve reverses it; an odd kernel keeps its centre)."""
    shp = [1, 1, 1]
    shp[axis3] = len(taps)
    return np.asarray(taps, dtype=np.float64)[::-1].reshape(shp)


def _check_float32(got, x, kernel, mode, ref, what):
    """The float32 gate for random kernels: the GPU's error against the float64 oracle is
    at most F32_FACTOR x the error of the oracle evaluated in float32, floor F32_FLOOR."""
    assert got.dtype == np.float32
    e_ref = rel_l2(convolve_f32(x, kernel, mode), ref, label="ref32 " + what)
    e_gpu = rel_l2(got, ref, label="gpu32 " + what)
    print("%s: float32 gpu %.3e reference %.3e ratio %.2f" %
          (what, e_gpu, e_ref, e_gpu / e_ref if e_ref > 0 else float("inf")))
    assert e_gpu <= max(F32_FACTOR * e_ref, F32_FLOOR), (what, e_gpu, e_ref)


# ------------------------------------------------------------------ the grid
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", GRID, ids=GRID_IDS)
def test_grid_matches_oracle(nsol, case, mode):
    from oracle import nsol_oracle as orc
    x, kernel = make_case(*case)
    A = _conv(kernel, mode)
    # a case that silently took the other kernel would prove nothing
    assert A.separable == expect_separable(case[2], case[3])
    ref = orc.convolve_nd(x, kernel, mode)
    got = A(x)
    assert got.dtype == np.float64 and got.shape == x.shape
    e64 = rel_l2(got, ref, label="gpu64")
    print("%s %s: float64 %.3e" % (case[0], mode, e64))
    assert e64 <= F64_TOL
    _check_float32(A(x.astype(np.float32)), x, kernel, mode, ref,
                   "%s %s" % (case[0], mode))


@pytest.mark.parametrize("name,kernel,separable", rank1_edge_kernels(),
                         ids=[e[0] for e in rank1_edge_kernels()])
def test_rank1_edge_kernels_match_oracle(nsol, name, kernel, separable):
    """Whichever path `_rank1_factors` chooses for a kernel at its edges (zero, negative
    and tiny sums, size-1 factors, nearly rank-1 taps) meets the float64 bound."""
    from oracle import nsol_oracle as orc
    rng = np.random.default_rng(17)
    x = rng.standard_normal((6, 9, 16)[3 - kernel.ndim:])
    for mode in MODES:
        A = _conv(kernel, mode)
        if separable is not None:
            assert A.separable == separable
        ref = orc.convolve_nd(x, kernel, mode)
        assert rel_l2(A(x), ref, label=mode) <= F64_TOL, mode
        _check_float32(A(x.astype(np.float32)), x, kernel, mode, ref,
                       "%s %s" % (name, mode))


# ------------------------------------------------ the vectorised wrap passes
def _wrap_shapes(axis3, vec, ntaps, ra):
    """Volumes for a wrap pass along axis3: rows of one vector and of 70 vectors (two
    blocks along x, the second partly empty; three for 8-byte elements' 140); axis
    lengths below the kernel's reach R, equal to RA, RA + 1 and no multiple of RA; the
    other slow axis no multiple of 4."""
    reach = ntaps // 2
    lens = sorted({max(1, reach - 1), ra, ra + 1, 2 * ra + 5})
    out = []
    if axis3 == 2:
        return [(3, 5, vec), (3, 5, 2 * vec), (1, 7, 280), (2, 3, 4 * 67)]
    for n in lens:
        for other, nx in ((5, vec), (3, 280)):
            out.append((n, other, nx) if axis3 == 0 else (other, n, nx))
    return out


def _run_wrap_pass(dtype, ntaps, axis3, shape, rng, symmetric=False):
    from nsol_amd import ops
    from oracle import nsol_oracle as orc
    taps = rng.uniform(-0.5, 1.0, ntaps)
    if symmetric:
        taps = taps + taps[::-1]
    x = rng.standard_normal(shape)
    ref = orc.convolve_nd(x, _axis_kernel(taps, axis3), "wrap")
    xd = _dev(x, dtype)
    assert xd.data_ptr() % 16 == 0
    got = ops.corr_axis(xd, shape, axis3, taps, ntaps // 2, "wrap")
    assert got.data_ptr() % 16 == 0
    got = got.cpu().numpy().reshape(shape)
    what = "nt%d axis%d %s" % (ntaps, axis3, "x".join(map(str, shape)))
    if dtype == np.float64:
        assert rel_l2(got, ref, label=what) <= F64_TOL, what
    else:
        _check_float32(got, x, _axis_kernel(taps, axis3), "wrap", ref, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ntaps", ODD_NT)
def test_wrap_pass_every_tap_count(nsol, ntaps, dtype):
    """nsol_corr_axis_* one axis at a time with odd centred taps, aligned operands and
    rows of whole vectors: k_corr_strided_wrap<NT, 8> along z and y, k_corr_x_wrap<NT, 1>
    along x, for every NT the library instantiates.  Asymmetric taps (the
    specialisation does not need symmetry), then symmetric ones."""
    vec = 16 // np.dtype(dtype).itemsize
    rng = np.random.default_rng(1000 + ntaps)
    for axis3 in (0, 1, 2):
        for shape in _wrap_shapes(axis3, vec, ntaps, 8):
            _run_wrap_pass(dtype, ntaps, axis3, shape, rng)
    for axis3, shape in ((0, (9, 3, 4 * vec)), (1, (3, 9, 4 * vec)), (2, (2, 3, 4 * vec))):
        _run_wrap_pass(dtype, ntaps, axis3, shape, rng, symmetric=True)


@pytest.mark.parametrize("ntaps", [3, 9, 25])
@pytest.mark.parametrize("knob,value", [("corr_ra", 2), ("corr_ra", 4), ("corr_xv", 2)])
def test_wrap_pass_knob_variants(nsol, knob, value, ntaps):
    """k_corr_strided_wrap<NT, 2>, <NT, 4> and k_corr_x_wrap<NT, 2> (experiment knobs)."""
    from nsol_amd import _lib
    rng = np.random.default_rng(2000 + ntaps + value)
    _lib.set_param(knob, value)
    try:
        for dtype in DTYPES:
            vec = 16 // np.dtype(dtype).itemsize
            for axis3 in ((0, 1) if knob == "corr_ra" else (2,)):
                for shape in _wrap_shapes(axis3, vec, ntaps, value):
                    _run_wrap_pass(dtype, ntaps, axis3, shape, rng)
            if knob == "corr_xv":
                # an odd number of vectors per row: the lane's second vector is past the row
                _run_wrap_pass(dtype, ntaps, 2, (2, 3, 129 * vec), rng)
    finally:
        _lib.set_param(knob, _lib.PARAM_DEFAULTS[knob])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ntaps", [5, 9, 19, 26, 27])
def test_wrap_pass_off_the_16_byte_grid(nsol, ntaps, dtype):
    """x and out as views at element offset 1 and 3 into larger buffers: the generic
    k_corr_axis takes over from the vectorised passes (another kernel: the bound, not
    bit-equality), and the guard elements around `out` keep their fill value.  26 and 27
    taps go to the generic kernel in any case."""
    import torch
    from nsol_amd import ops
    from oracle import nsol_oracle as orc
    td = _torch_dtype(dtype)
    vec = 16 // np.dtype(dtype).itemsize
    shape = (6, 9, 8 * vec)
    n = int(np.prod(shape))
    rng = np.random.default_rng(3000 + ntaps)
    centre = ntaps // 2 - (1 if ntaps % 2 == 0 else 0)
    for off in (1, 3):
        for axis3 in (0, 1, 2):
            taps = rng.uniform(-0.5, 1.0, ntaps)
            x = rng.standard_normal(shape)
            ref = orc.convolve_nd(x, _axis_kernel(taps, axis3), "wrap")
            xbuf = torch.full((n + 8,), 555.0, device="cuda", dtype=td)
            obuf = torch.full((n + 8,), 777.0, device="cuda", dtype=td)
            x_off, out_off = xbuf[off:off + n], obuf[off:off + n]
            x_off.copy_(_dev(x, dtype))
            assert x_off.data_ptr() % 16 != 0 and out_off.data_ptr() % 16 != 0
            ops.corr_axis(x_off, shape, axis3, taps, centre, "wrap", out=out_off)
            got = out_off.cpu().numpy().reshape(shape)
            what = "nt%d axis%d off%d" % (ntaps, axis3, off)
            if dtype == np.float64:
                assert rel_l2(got, ref, label=what) <= F64_TOL, what
            else:
                _check_float32(got, x, _axis_kernel(taps, axis3), "wrap", ref, what)
            assert bool((obuf[:off] == 777.0).all().item()), what
            assert bool((obuf[off + n:] == 777.0).all().item()), what
            assert bool((xbuf[:off] == 555.0).all().item()), what
            assert bool((xbuf[off + n:] == 555.0).all().item()), what


# ------------------------------------------------ anisotropic Gaussian blurs
ANISO_COV = np.diag([0.3, 4.0, 16.0])      # half widths ceil(3 sigma) = 2, 6, 12


def _aniso_blur(cov=ANISO_COV):
    A, _ = _lo3().get_gaussian_blurring_operators(cov)
    assert A.separable and not A._fusable3()
    return A


def test_anisotropic_blur_has_three_tap_counts(nsol):
    A = _aniso_blur()
    assert A.kernel.shape == (5, 13, 25)
    assert [(a, t.size, c) for a, t, c in A._passes] == [(0, 5, 2), (1, 13, 6), (2, 25, 12)]
    B = _aniso_blur(np.diag([9.0, 0.2, 2.0]))
    assert [(a, t.size, c) for a, t, c in B._passes] == [(0, 19, 9), (1, 5, 2), (2, 11, 5)]


@pytest.mark.parametrize("shape,dtype,cov", [
    ((64, 96, 128), np.float32, (0.3, 4.0, 16.0)),
    ((33, 40, 66), np.float64, (0.3, 4.0, 16.0)),
    ((64, 96, 128), np.float32, (9.0, 0.2, 2.0)),
    ((33, 40, 66), np.float64, (9.0, 0.2, 2.0)),
    # rows that are no whole vectors: the generic kernel
    ((20, 31, 67), np.float32, (0.3, 4.0, 16.0)),
    ((20, 31, 67), np.float64, (0.3, 4.0, 16.0))],
    ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_anisotropic_blur_matches_oracle(nsol, shape, dtype, cov):
    """A slice-acquisition PSF: a different tap count per axis, three vectorised passes
    with three NT, against the oracle's dense sum."""
    from oracle import nsol_oracle as orc
    A = _aniso_blur(np.diag(cov))
    rng = np.random.default_rng(41)
    x = rng.standard_normal(shape).astype(dtype)
    ref = orc.convolve_nd(x.astype(np.float64), A.kernel, "wrap")
    got = A(x)
    assert got.dtype == dtype
    # 19 and 25 taps: the gate of float32 Gaussians from 17 taps up
    assert rel_l2(got, ref) <= (F64_TOL if dtype == np.float64 else 2e-6)


def test_anisotropic_blur_256_cubed_matches_generic_kernel(nsol):
    """256^3 float32, where the oracle's dense sum is too slow: the vectorised passes
    (aligned operands) against the generic k_corr_axis on the same input (operands one
    element off the 16-byte grid), which the smaller cases hold to the oracle."""
    import torch
    from nsol_amd import ops
    A = _aniso_blur()
    shape = (256, 256, 256)
    n = int(np.prod(shape))
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(n, device="cuda", dtype=torch.float32, generator=gen)
    got = A(x.view(shape)).view(-1)
    bufs = [torch.full((n + 8,), 777.0, device="cuda", dtype=torch.float32)
            for _ in range(2)]
    cur = bufs[0][1:1 + n]
    cur.copy_(x)
    for i, (axis3, taps, centre) in enumerate(A._passes):
        nxt = bufs[(i + 1) % 2][1:1 + n]
        assert cur.data_ptr() % 16 != 0 and nxt.data_ptr() % 16 != 0
        ops.corr_axis(cur, shape, axis3, taps, centre, "wrap", out=nxt)
        cur = nxt
    assert rel_l2(got.cpu().numpy(), cur.cpu().numpy()) <= 2e-6
    for b in bufs:
        assert float(b[0]) == 777.0 and bool((b[1 + n:] == 777.0).all().item())


# -------------------------------------------- structure, without a reference
def _expected_one_hot(x, kshape, hot, mode):
    """ndimage.convolve with a one-hot kernel: tap j of an s-tap axis sits on
    x[i - j + s // 2], mapped into the array by the boundary rule."""
    idx = [[map_index_py(i - hot[ax] + kshape[ax] // 2, x.shape[ax], mode)
            for i in range(x.shape[ax])] for ax in range(x.ndim)]
    return take_mapped(x, idx).astype(x.dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
def test_one_hot_kernel_reproduces_the_folded_input_1d(nsol, mode, dtype):
    """Every tap position of 1- to 9-tap kernels on extents 1, 2, 3, 5, 8: the output is
    the input sampled through the Python index rule, bit for bit (k_corr_axis; for
    wrap, whole-vector rows and odd sizes k_corr_x_wrap)."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 5, 8):
        x = rng.standard_normal(n).astype(dtype)
        for s in (1, 2, 3, 4, 5, 8, 9):
            for hot in range(s):
                k = np.zeros(s)
                k[hot] = 1.0
                got = _conv(k, mode)(x)
                want = _expected_one_hot(x, (s,), (hot,), mode)
                assert np.array_equal(got, want), (n, s, hot)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,kshape", [((2, 3, 5), (3, 4, 2)), ((1, 2, 8), (2, 5, 3)),
                                          ((4, 8), (8, 3))],
                         ids=["2x3x5_k3x4x2", "1x2x8_k2x5x3", "4x8_k8x3"])
def test_one_hot_kernel_reproduces_the_folded_input_nd(nsol, shape, kshape, mode, dtype):
    """The same in 2-D / 3-D, through both paths: a one-hot array is an outer product
    (the separable passes), and nsol_corr_dense_* is called with it directly."""
    from nsol_amd import ops
    rng = np.random.default_rng(6)
    x = rng.standard_normal(shape).astype(dtype)
    xd = _dev(x, dtype)
    for hot in all_hot_positions(kshape):
        k = np.zeros(kshape)
        k[hot] = 1.0
        want = _expected_one_hot(x, kshape, hot, mode)
        A = _conv(k, mode)
        assert A.separable
        assert np.array_equal(A(x), want), hot
        k3 = (1,) * (3 - len(kshape)) + tuple(kshape)
        c3 = (0,) * (3 - len(kshape)) + tuple(A._centre)
        got = ops.corr_dense(xd, shape, _dev(A._flipped, dtype), k3, c3, mode)
        assert np.array_equal(got.cpu().numpy().reshape(shape), want), hot


@pytest.mark.parametrize("mode", MODES)
def test_linearity_in_the_kernel(nsol, mode):
    """C_{a k1 + b k2} x = a C_k1 x + b C_k2 x.  With k1, k2 outer products the left
    side runs the dense kernel and the right side the separable passes."""
    rng = np.random.default_rng(8)
    for shape, kshape in [((23,), (6,)), ((7, 18), (4, 5)), ((5, 6, 16), (3, 3, 3)),
                          ((3, 2, 9), (5, 8, 4))]:
        x = rng.standard_normal(shape)
        k1, k2 = (make_case("lin%d" % i, shape, kshape, True)[1] for i in (1, 2))
        a, b = 0.75, -1.5
        A1, A2, A12 = _conv(k1, mode), _conv(k2, mode), _conv(a * k1 + b * k2, mode)
        assert A1.separable and A2.separable
        assert A12.separable == (len(kshape) == 1)
        assert rel_l2(A12(x), a * A1(x) + b * A2(x)) <= F64_TOL


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_constant_equals_wrap_inside_a_zero_border(nsol, dtype):
    """On an input whose border of kernel width is zero no tap ever reaches a sample
    through the boundary: "constant" and "wrap" add the same products in the same
    order (or a product with zero) -- equal bit for bit, dense and separable."""
    rng = np.random.default_rng(9)
    for shape, kshape, outer in [((40,), (7,), True), ((20, 32), (4, 5), False),
                                 ((20, 32), (4, 5), True), ((16, 18, 32), (3, 4, 5), False),
                                 ((16, 18, 32), (3, 4, 5), True),
                                 ((16, 18, 32), (3, 5, 7), True)]:
        _, k = make_case("zb", shape, kshape, outer)
        x = np.zeros(shape, dtype=dtype)
        inner = tuple(slice(s, n - s) for s, n in zip(kshape, shape))
        x[inner] = rng.standard_normal(x[inner].shape)
        got_c, got_w = _conv(k, "constant")(x), _conv(k, "wrap")(x)
        assert np.any(got_c != 0)
        assert np.array_equal(got_c, got_w), (shape, kshape, outer)


def test_wrap_adjoint_is_the_flipped_kernel_shifted_for_even_sizes(nsol):
    """<C_k x, y> = <x, roll(C_k' y, +1 along every even-sized axis)> under "wrap", k'
    the kernel reversed along every axis (test_conv_host.wrap_adjoint_pair derives it:
    ndimage.convolve puts tap j on x[i - j + s // 2]; reversing an even-sized kernel
    moves that centre by one sample, an odd one keeps it)."""
    rng = np.random.default_rng(10)
    for shape, kshape, outer in [((16,), (3,), True), ((16,), (4,), True), ((9,), (8,), True),
                                 ((6, 16), (2, 5), False), ((6, 16), (4, 3), True),
                                 ((6, 7, 16), (4, 3, 2), False), ((6, 7, 16), (3, 5, 7), True),
                                 ((6, 7, 16), (2, 8, 4), True), ((2, 3, 3), (8, 9, 8), True)]:
        _, k = make_case("adj", shape, kshape, outer)
        x, y = rng.standard_normal(shape), rng.standard_normal(shape)
        kf, shifts, axes = wrap_adjoint_pair(k)
        lhs = np.vdot(_conv(k, "wrap")(x), y)
        rhs = np.vdot(x, np.roll(_conv(kf, "wrap")(y), shifts, axes))
        assert abs(lhs - rhs) < 1e-10, (shape, kshape, lhs, rhs)


# ------------------------------------------------------------ error behaviour
def test_dimension_mismatch_raises(nsol):
    import torch
    A = _conv(np.ones((3, 3, 3)) / 27.0, "wrap")
    with pytest.raises(RuntimeError, match="3D convolution applied to 2 axes"):
        A(np.ones((4, 5)))
    with pytest.raises(RuntimeError, match="3D convolution applied to 2 axes"):
        A(torch.ones((4, 5), device="cuda", dtype=torch.float64))
    B = _conv(np.array([[1., 2.], [3., 5.]]), "reflect")      # the dense kernel
    with pytest.raises(RuntimeError, match="2D convolution applied to 3 axes"):
        B(np.ones((4, 5, 6)))
