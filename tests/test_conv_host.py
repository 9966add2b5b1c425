"""The convolution reference and the case grid the HIP kernels are held to
(tests/test_conv_gpu.py), pinned on the host.

* `oracle.nsol_oracle.convolve_nd` (float64, np.pad + slicing) against
  scipy.ndimage.convolve over the whole grid: five modes, 1-D / 2-D / 3-D, even
  and odd tap counts, kernels several periods longer than the extent, extents of
  1 and 2.  ndimage is the authority.
* `map_index_py`: the boundary rule in ten lines of Python, checked against ndimage
  position by position -- what a reader compares map_index() of
  nsol_amd/csrc/nsol_conv.hip with.
* `correlate_model`: the dense kernel restated in Python on top of map_index_py with
  the flip and centre that `_ndimage_convolve_params` hands to the library.
* `_rank1_factors`, which chooses between the separable passes and the dense kernel,
  at its edges.

No GPU, no library."""
import itertools

import numpy as np
import pytest
from scipy import ndimage

from conftest import rel_l2
from oracle import nsol_oracle as orc

MODES = ("constant", "wrap", "nearest", "reflect", "mirror")

# the separable form holds at most this many taps per axis (kMaxTaps)
MAX_SEPARABLE_TAPS = 129


# ----------------------------------------------------------------- the grid
# (name, array shape, kernel shape, outer product?)  Every case runs under all five
# modes.  Kernel sizes per axis: 1, 2, 3, 4, 5, 8, 9 and the long 27 (beyond the 25-tap
# specialisation) and 131 (beyond the separable form's 129).  Extents: 1, 2, 3,
# kernel - 1, kernel, 2 * kernel + 1 and ordinary ones; extents 2 and 3 under 8 and 9
# taps fold the window three times and more; rows of 16, 18, 19, 63, 64.
GRID = [
    # 1-D (one factor: the separable form whatever the taps, up to 129 of them)
    ("1d_n1_k1", (1,), (1,), True),
    ("1d_n1_k3", (1,), (3,), True),
    ("1d_n1_k8", (1,), (8,), True),
    ("1d_n2_k8", (2,), (8,), True),
    ("1d_n3_k9", (3,), (9,), True),
    ("1d_n2_k5", (2,), (5,), True),
    ("1d_n7_k8", (7,), (8,), True),
    ("1d_n8_k8", (8,), (8,), True),
    ("1d_n17_k8", (17,), (8,), True),
    ("1d_n4_k5", (4,), (5,), True),
    ("1d_n5_k5", (5,), (5,), True),
    ("1d_n11_k5", (11,), (5,), True),
    ("1d_n64_k4", (64,), (4,), True),
    ("1d_n63_k2", (63,), (2,), True),
    ("1d_n19_k3", (19,), (3,), True),
    ("1d_n16_k27", (16,), (27,), True),
    ("1d_n300_k27", (300,), (27,), True),
    ("1d_n300_k131", (300,), (131,), False),
    ("1d_n40_k131", (40,), (131,), False),
    # 2-D dense
    ("2d_dense_5x16_k3x4", (5, 16), (3, 4), False),
    ("2d_dense_2x3_k8x5", (2, 3), (8, 5), False),
    ("2d_dense_1x9_k2x3", (1, 9), (2, 3), False),
    ("2d_dense_9x1_k3x2", (9, 1), (3, 2), False),
    ("2d_dense_7x18_k8x2", (7, 18), (8, 2), False),
    ("2d_dense_11x63_k5x5", (11, 63), (5, 5), False),
    # 2-D outer products
    ("2d_sep_5x16_k3x4", (5, 16), (3, 4), True),
    ("2d_sep_3x2_k9x8", (3, 2), (9, 8), True),
    ("2d_sep_12x19_k5x2", (12, 19), (5, 2), True),
    ("2d_sep_1x64_k1x5", (1, 64), (1, 5), True),
    ("2d_sep_30x63_k27x3", (30, 63), (27, 3), True),
    ("2d_sep_6x140_k2x131", (6, 140), (2, 131), False),
    # 3-D dense
    ("3d_dense_4x5x16_k2x3x4", (4, 5, 16), (2, 3, 4), False),
    ("3d_dense_2x3x3_k3x8x5", (2, 3, 3), (3, 8, 5), False),
    ("3d_dense_1x1x7_k2x2x3", (1, 1, 7), (2, 2, 3), False),
    ("3d_dense_3x1x2_k4x2x5", (3, 1, 2), (4, 2, 5), False),
    ("3d_dense_6x7x18_k1x4x3", (6, 7, 18), (1, 4, 3), False),
    ("3d_dense_5x9x64_k3x3x3", (5, 9, 64), (3, 3, 3), False),
    ("3d_dense_9x4x19_k5x2x2", (9, 4, 19), (5, 2, 2), False),
    # 3-D outer products
    ("3d_sep_4x5x16_k2x3x4", (4, 5, 16), (2, 3, 4), True),
    ("3d_sep_2x3x3_k9x8x5", (2, 3, 3), (9, 8, 5), True),
    ("3d_sep_1x2x3_k4x5x8", (1, 2, 3), (4, 5, 8), True),
    ("3d_sep_7x8x17_k8x8x8", (7, 8, 17), (8, 8, 8), True),
    ("3d_sep_6x63x18_k3x27x1", (6, 63, 18), (3, 27, 1), True),
    ("3d_sep_5x6x64_k1x1x27", (5, 6, 64), (1, 1, 27), True),
    ("3d_sep_3x4x300_k1x1x131", (3, 4, 300), (1, 1, 131), False),
    # under wrap: three vectorised passes with three tap counts / the one-pass blur
    ("3d_sep_8x12x64_k3x5x7", (8, 12, 64), (3, 5, 7), True),
    ("3d_sep_9x10x32_k9x15x21", (9, 10, 32), (9, 15, 21), True),
    ("3d_sep_8x12x16_k5x5x5", (8, 12, 16), (5, 5, 5), True),
    ("3d_sep_6x5x19_k3x3x3", (6, 5, 19), (3, 3, 3), True),
]
GRID_IDS = [g[0] for g in GRID]


def make_case(name, shape, kshape, outer):
    """(x, kernel) of a grid case, float64, from a generator seeded by the name.
    Outer products are built from random vectors (asymmetric, mixed signs); the others
    are random arrays with at least two axes longer than 1, or a single long axis that
    the separable form cannot hold."""
    seed = int.from_bytes(name.encode(), "little") % (2 ** 32)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    if outer or len(kshape) == 1 or sum(s > 1 for s in kshape) < 2:
        kernel = np.ones(())
        for s in kshape:
            # (a sum well away from zero, so that the product's own sum is: an outer
            # product must be recognised as one)
            v = rng.uniform(-0.5, 1.0, s)
            while abs(v.sum()) < 0.2 * np.abs(v).sum():
                v = rng.uniform(-0.5, 1.0, s)
            kernel = np.multiply.outer(kernel, v)
    else:
        kernel = rng.uniform(-1.0, 1.0, kshape)
    return x, kernel.reshape(kshape)


def expect_separable(kshape, outer):
    return outer and max(kshape) <= MAX_SEPARABLE_TAPS


# ------------------------------------------------------------ the index rule
def map_index_py(i, n, mode):
    """Index in [0, n) of the sample that position i refers to under `mode`, -1 for
    the zero of "constant" (scipy.ndimage's boundary modes)."""
    if 0 <= i < n:
        return i
    if mode == "constant":
        return -1
    if mode == "wrap":
        return i % n
    if mode == "nearest":
        return 0 if i < 0 else n - 1
    if mode == "reflect":                 # d c b a | a b c d | d c b a
        j = i % (2 * n)
        return j if j < n else 2 * n - 1 - j
    if n == 1:                            # mirror:  d c b | a b c d | c b a
        return 0
    j = i % (2 * n - 2)
    return j if j < n else 2 * n - 2 - j


def take_mapped(x, index_lists):
    """x sampled at one list of mapped indices per axis (-1: zero)."""
    out = x
    for ax, idx in enumerate(index_lists):
        idx = np.asarray(idx)
        out = np.take(out, np.where(idx < 0, 0, idx), axis=ax)
        shp = [1] * x.ndim
        shp[ax] = idx.size
        out = np.where((idx < 0).reshape(shp), 0.0, out)
    return out


def ndimage_params(kernel):
    """What ndimage.convolve(x, kernel) means as a correlation: the reversed kernel
    and, per axis, the tap that sits on the output position."""
    kernel = np.asarray(kernel, dtype=np.float64)
    w = kernel[tuple([slice(None, None, -1)] * kernel.ndim)]
    return w, [s // 2 - (1 if s % 2 == 0 else 0) for s in kernel.shape]


def correlate_model(x, w, centre, mode, dtype=np.float64):
    """out[i] = sum_t w[t] * x[map(i + t - centre)], taps in row-major order, products
    and sum in `dtype`: k_corr_dense restated."""
    x = np.asarray(x, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    out = np.zeros(x.shape, dtype=dtype)
    for t in np.ndindex(*w.shape):
        idx = [[map_index_py(i + t[ax] - centre[ax], x.shape[ax], mode)
                for i in range(x.shape[ax])] for ax in range(x.ndim)]
        out += w[t] * take_mapped(x, idx).astype(dtype)
    return out


def convolve_f32(x, kernel, mode):
    """oracle.convolve_nd with float32 data, float32 products and float32 accumulation
    in tap order: the error a correct single-precision kernel is expected to make
    (ndimage accumulates in double whatever the input, so it cannot stand in)."""
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(kernel, dtype=np.float32)
    w = w[tuple([slice(None, None, -1)] * w.ndim)]
    xp = x
    for ax in range(x.ndim):
        s = w.shape[ax]
        c = s // 2 - (1 if s % 2 == 0 else 0)
        xp = orc._pad_axis(xp, ax, c, s - 1 - c, mode)
    assert xp.dtype == np.float32
    out = np.zeros(x.shape, dtype=np.float32)
    for idx in np.ndindex(*w.shape):
        sl = tuple(slice(idx[ax], idx[ax] + x.shape[ax]) for ax in range(x.ndim))
        out += w[idx] * xp[sl]
    assert out.dtype == np.float32
    return out


# ------------------------------------------------------------------- tests
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_index_map_matches_ndimage(n, mode):
    """Every position from -3n - 1 to 4n + 1: a one-hot correlation kernel whose tap
    sits d samples from the output position reads x[map(i + d)].  The ramp starts at 1
    so that the zero of "constant" is no sample."""
    x = np.arange(1.0, n + 1.0)
    half = 4 * n + 1
    for d in range(-half, half + 1):
        w = np.zeros(2 * half + 1)
        w[half + d] = 1.0
        got = ndimage.correlate(x, w, mode=mode)
        for i in range(n):
            p = i + d
            if not -3 * n - 1 <= p <= 4 * n + 1:
                continue
            j = map_index_py(p, n, mode)
            want = 0.0 if j < 0 else x[j]
            assert got[i] == want, (n, mode, p, j)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", GRID, ids=GRID_IDS)
def test_oracle_convolve_matches_ndimage(case, mode):
    """convolve_nd and ndimage.convolve sum the same float64 products; another order at
    the most."""
    x, kernel = make_case(*case)
    want = ndimage.convolve(x, kernel, mode=mode)
    got = orc.convolve_nd(x, kernel, mode)
    assert got.shape == want.shape
    assert rel_l2(got, want) <= 1e-13


SMALL = [g for g in GRID if np.prod(g[1]) * np.prod(g[2]) <= 20000]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", SMALL, ids=[g[0] for g in SMALL])
def test_flip_and_centre_handed_to_the_library(case, mode):
    """The taps and centres `_ndimage_convolve_params` passes to nsol_corr_dense_* /
    nsol_corr_axis_*, applied by the Python model of the kernel, are ndimage.convolve."""
    import nsol_amd.linear_operators as LO
    x, kernel = make_case(*case)
    flipped, centre = LO._ndimage_convolve_params(kernel)
    w, c = ndimage_params(kernel)
    assert np.array_equal(flipped, w) and list(centre) == c
    got = correlate_model(x, flipped, centre, mode)
    assert rel_l2(got, ndimage.convolve(x, kernel, mode=mode)) <= 1e-13


def test_float32_reference_is_the_oracle_in_single_precision():
    x, kernel = make_case("f32ref", (6, 7, 9), (3, 4, 5), False)
    for mode in MODES:
        ref = orc.convolve_nd(x, kernel, mode)
        got = convolve_f32(x, kernel, mode)
        assert got.dtype == np.float32
        err = rel_l2(got, ref)
        # 60 products of rounded operands: a few float32 epsilons, and not float64
        assert 1e-9 < err < 60 * 2.0 ** -24
        assert np.array_equal(
            got, correlate_model(x, *ndimage_params(kernel), mode, dtype=np.float32))


def test_grid_kernels_are_what_they_claim():
    import nsol_amd.linear_operators as LO
    for case in GRID:
        _, kernel = make_case(*case)
        assert kernel.shape == case[2]
        A = LO.ConvolutionOperator(kernel.ndim, kernel, "reflect")
        assert A.separable == expect_separable(case[2], case[3]), case[0]


# ------------------------------------------------------------ _rank1_factors
def _outer(*vs):
    k = np.ones(())
    for v in vs:
        k = np.multiply.outer(k, np.asarray(v, dtype=np.float64))
    return k


def rank1_edge_kernels():
    """(name, kernel, separable?) -- None where either path is right and only the
    result counts (tests/test_conv_gpu.py runs them all)."""
    rng = np.random.default_rng(5)
    a, b, c = rng.uniform(0.2, 1.0, 3), rng.uniform(0.2, 1.0, 5), rng.uniform(0.2, 1.0, 4)
    exact = _outer(a, b, c)
    noise = rng.uniform(-1.0, 1.0, exact.shape)
    tiny = rng.uniform(-1.0, 1.0, 5)
    tiny[-1] = 1e-9 - tiny[:-1].sum()
    return [
        ("sobel", _outer([1., 2., 1.], [1., 0., -1.]), False),
        ("sobel_3d", _outer([1., 2., 1.], [1., 2., 1.], [1., 0., -1.]), False),
        ("negative_sum_2d", _outer([1., -3., 1.], [1., 2., 1.]), True),
        ("negative_sum_3d", _outer([1., -3., 1.], [1., 2., 1.], [0.5, 0.25]), True),
        ("size1_factor", _outer(a, [2.5], c), True),
        ("size1_factor_unit_sum", _outer(a / a.sum(), [1.0], c / c.sum()), True),
        ("one_axis_1x1xk", _outer([1.0], [1.0], b), True),
        ("one_axis_kx1x1_negative", _outer(-b, [1.0], [1.0]), True),
        ("exact", exact, True),
        ("perturbed_1e-15", exact * (1.0 + 1e-15 * noise), True),
        ("perturbed_1e-11", exact * (1.0 + 1e-11 * noise), False),
        ("tiny_sum_exact_factors", _outer([1.0, -1.0 + 1e-9], [1.0, 1.0]), None),
        ("tiny_sum_random", _outer(a, tiny), None),
        ("tiny_sum_random_3d", _outer(tiny, a, c), None),
    ]


@pytest.mark.parametrize("name,kernel,separable", rank1_edge_kernels(),
                         ids=[e[0] for e in rank1_edge_kernels()])
def test_rank1_factors_edges(name, kernel, separable):
    import nsol_amd.linear_operators as LO
    A = LO.ConvolutionOperator(kernel.ndim, kernel, "mirror")
    if separable is not None:
        assert A.separable == separable
    facs = LO._rank1_factors(A._flipped)      # (the reversed taps: what the passes apply)
    assert (facs is not None) == A.separable
    if facs is not None:
        # the product of the factors is the kernel itself, to the tolerance of the test
        assert [f.size for f in facs] == list(kernel.shape)
        assert np.max(np.abs(_outer(*facs) - A._flipped)) <= \
            2e-13 * np.max(np.abs(kernel))
        # passes whose only tap is exactly 1 are dropped, nothing else
        want = [ax + 3 - kernel.ndim for ax, f in enumerate(facs)
                if not (f.size == 1 and f[0] == 1.0)]
        assert [p[0] for p in A._passes] == want


def test_rank1_factors_takes_every_1d_kernel_and_no_long_axis():
    import nsol_amd.linear_operators as LO
    assert LO.ConvolutionOperator(1, np.array([1., 0., -1.])).separable
    assert LO.ConvolutionOperator(1, np.ones(129)).separable
    assert not LO.ConvolutionOperator(1, np.ones(130)).separable
    assert LO.ConvolutionOperator(2, _outer(np.ones(129), [1., 2.])).separable
    assert not LO.ConvolutionOperator(2, _outer(np.ones(131), [1., 2.])).separable


# ------------------------------------------------------------ error behaviour
def test_constructor_errors():
    import nsol_amd.linear_operators as LO
    with pytest.raises(RuntimeError, match="filter weights array has incorrect shape"):
        LO.ConvolutionOperator(3, np.ones((3, 3)))
    with pytest.raises(RuntimeError, match="filter weights array has incorrect shape"):
        LO.ConvolutionOperator(1, np.ones((3, 1)))
    with pytest.raises(RuntimeError, match="boundary mode not supported"):
        LO.ConvolutionOperator(2, np.ones((3, 3)), mode="symmetric")
    with pytest.raises(RuntimeError, match="boundary mode not supported"):
        LO.LinearOperators2D().get_dx_operators(mode="edge")


def test_adjoint_shift_for_even_sizes_on_the_host():
    """The identity test_conv_gpu.py checks on the GPU, on the oracle first (see
    wrap_adjoint_pair)."""
    rng = np.random.default_rng(3)
    for kshape in [(3,), (4,), (2, 5), (4, 3, 2)]:
        shape = tuple(s + 3 for s in kshape)
        k = rng.standard_normal(kshape)
        x, y = rng.standard_normal(shape), rng.standard_normal(shape)
        kf, shift, axes = wrap_adjoint_pair(k)
        lhs = np.vdot(orc.convolve_nd(x, k, "wrap"), y)
        rhs = np.vdot(x, np.roll(orc.convolve_nd(y, kf, "wrap"), shift, axes))
        assert abs(lhs - rhs) < 1e-12 * (1 + abs(lhs))


def wrap_adjoint_pair(kernel):
    """(flipped kernel k', shifts, axes) with
         <C_k x, y> = <x, roll(C_k' y, shifts, axes)>      (mode "wrap").
    ndimage.convolve puts tap j of an s-tap axis on x[i - j + s // 2] (odd and even s
    alike), so (C_k^T y)[m] = sum_j k[j] y[m + j - s // 2], while C_k' with
    k'[j] = k[s - 1 - j] gives sum_j k[j] y[m + j - (s - 1 - s // 2)].  For odd s the
    two offsets agree and C_k^T = C_k'; for even s they differ by one and
    (C_k^T y)[m] = (C_k' y)[m - 1]: a roll by +1 along every even-sized axis."""
    kernel = np.asarray(kernel)
    kf = kernel[tuple([slice(None, None, -1)] * kernel.ndim)]
    axes = tuple(range(kernel.ndim))
    shifts = tuple(1 if s % 2 == 0 else 0 for s in kernel.shape)
    return kf, shifts, axes


def all_hot_positions(kshape):
    return list(itertools.product(*[range(s) for s in kshape]))
