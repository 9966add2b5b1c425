"""CPU side of the tiled dense correlation and of ConvolutionOperator.transpose():

  * the planner (nsol_amd/csrc/nsol_convd_plan.hpp) through tests/host/convd_plan_check.cpp,
    built with the host compiler alone, once plain and once with the address and
    undefined-behaviour sanitizers, and run as a child process;
  * the transposed kernel against scipy.ndimage.convolve: <A x, y> = <x, A^T y>;
  * exact_adjoint= of the factory; the new entries in the header.

No GPU: the operators' taps are applied by scipy here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "convd_plan_check.cpp")
BUILDS = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined",
                                     "-fno-sanitize-recover=all"]}
KERNEL_SHAPES = [(4,), (3,), (2, 3), (2, 3, 4), (4, 1, 2), (4, 5)]
# float64 dot products of a few hundred terms of size O(1): 1e-12 relative is four orders
# above their rounding
ADJOINT_TOL = 1e-12


def _clangxx():
    """The clang++ that hipcc drives."""
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for root in filter(None, roots):
        for sub in ("llvm/bin", "lib/llvm/bin"):
            exe = os.path.join(root, sub, "clang++")
            if os.path.exists(exe):
                return exe
    return None


@pytest.mark.parametrize("build", list(BUILDS))
def test_planner_grid(tmp_path, build):
    """Every plan covers the volume exactly once, its LDS bytes are the ring formula and
    fit a CU, the lane layout is consistent, and the declines are the documented ones."""
    cxx = _clangxx()
    assert cxx is not None, "ROCm's clang++ not found"
    exe = tmp_path / ("convd_plan_check_" + build)
    subprocess.run([cxx, "-std=c++17", "-ffp-contract=off", "-O1"] + BUILDS[build] +
                   [SOURCE, "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True)
    assert got.returncode == 0, got.stdout
    word, plans, declines, invalid = got.stdout.split()
    assert word == "ok" and min(int(plans), int(declines), int(invalid)) > 1000


def _image_shape(kshape):
    """A 2 x 3 image (the issue's), with the axes a 1-D / 3-D kernel needs."""
    return {1: (6,), 2: (2, 3), 3: (2, 2, 3)}[len(kshape)]


@pytest.mark.parametrize("mode", ["wrap", "constant"])
@pytest.mark.parametrize("kshape", KERNEL_SHAPES, ids=str)
def test_transpose_is_the_adjoint_under_ndimage(kshape, mode):
    """<A x, y> = <x, A^T y> with both sides evaluated by scipy.ndimage.convolve on the
    operators' kernels; the image is smaller than the kernel on some axes, so windows
    fold.  A second, larger image with odd and even extents as well."""
    from scipy import ndimage
    import nsol_amd.linear_operators as LO
    rng = np.random.default_rng(sum(kshape) + len(mode))
    kernel = rng.standard_normal(kshape)
    A = LO.ConvolutionOperator(len(kshape), kernel, mode)
    At = A.transpose()
    assert isinstance(At, LO.ConvolutionOperator) and At.mode == mode
    assert At.kernel.shape == tuple(s + (s % 2 == 0) for s in kshape)
    assert A.separable == At.separable
    for shape in (_image_shape(kshape), tuple(range(5, 5 + len(kshape)))):
        x, y = rng.standard_normal(shape), rng.standard_normal(shape)
        lhs = np.vdot(ndimage.convolve(x, A.kernel, mode=mode), y)
        rhs = np.vdot(x, ndimage.convolve(y, At.kernel, mode=mode))
        scale = np.linalg.norm(ndimage.convolve(x, A.kernel, mode=mode)) * np.linalg.norm(y)
        print(kshape, mode, shape, abs(lhs - rhs) / scale)
        assert abs(lhs - rhs) <= ADJOINT_TOL * scale
        # the transpose of the transpose computes A x again
        Att = At.transpose()
        np.testing.assert_allclose(ndimage.convolve(x, Att.kernel, mode=mode),
                                   ndimage.convolve(x, A.kernel, mode=mode),
                                   rtol=0, atol=1e-13 * np.abs(kernel).sum() * np.abs(x).max())


def test_transpose_is_the_documented_roll_in_taps():
    """test_conv_host.wrap_adjoint_pair states the rule as 'flip, then roll by one along
    every even-sized axis'; the prepended zero is that roll."""
    from scipy import ndimage
    from test_conv_host import wrap_adjoint_pair
    import nsol_amd.linear_operators as LO
    rng = np.random.default_rng(5)
    kernel = rng.standard_normal((2, 3, 4))
    y = rng.standard_normal((5, 4, 7))
    kf, shifts, axes = wrap_adjoint_pair(kernel)
    want = np.roll(ndimage.convolve(y, kf, mode="wrap"), shifts, axes)
    got = ndimage.convolve(y, LO.ConvolutionOperator(3, kernel, "wrap").transpose().kernel,
                           mode="wrap")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("mode", ["nearest", "reflect", "mirror"])
def test_transpose_of_the_other_modes_raises(mode):
    import nsol_amd.linear_operators as LO
    A = LO.ConvolutionOperator(2, np.arange(6.).reshape(2, 3), mode)
    with pytest.raises(ValueError, match="transpose"):
        A.transpose()
    with pytest.raises(ValueError, match="transpose"):
        LO.LinearOperators2D().get_convolution_and_adjoint_convolution_operators(
            np.arange(6.).reshape(2, 3), mode, exact_adjoint=True)


def test_exact_adjoint_switch_of_the_factory():
    import nsol_amd.linear_operators as LO
    kernel = np.arange(1., 7.).reshape(2, 3)
    lo = LO.LinearOperators2D()
    A, At = lo.get_convolution_and_adjoint_convolution_operators(kernel)
    assert A is At
    A, At = lo.get_convolution_and_adjoint_convolution_operators(kernel, exact_adjoint=False)
    assert A is At
    A, At = lo.get_convolution_and_adjoint_convolution_operators(kernel, "constant",
                                                                 exact_adjoint=True)
    assert A is not At and At.mode == "constant"
    np.testing.assert_array_equal(At.kernel, A.transpose().kernel)
    np.testing.assert_array_equal(At.kernel, np.pad(kernel[::-1, ::-1], [(1, 0), (0, 0)]))
    # a separable asymmetric PSF keeps its 1-D passes; an odd point-symmetric kernel is
    # its own transpose
    sep = np.multiply.outer([1., 2., 4.], [1., 3.])
    S = LO.ConvolutionOperator(2, sep, "wrap")
    assert S.separable and S.transpose().separable and S.dense_form((8, 8)) is None
    sym = np.array([[1., 2., 1.], [3., 5., 3.], [1., 2., 1.]])
    np.testing.assert_array_equal(LO.ConvolutionOperator(2, sym).transpose().kernel, sym)
    assert LO.USE_TILED_DENSE is True


def test_oriented_gaussian_is_dense():
    """The thick-slice PSF rotated against the grid: 7 x 13 x 17 taps, no outer product."""
    import nsol_amd.linear_operators as LO
    from nsol_amd import kernels as K
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    R = np.array([[1., 0., 0.], [0., c, -s], [0., s, c]])
    cov = R @ np.diag([1., 1., 9.]) @ R.T
    kernel = K.Kernels3D().get_gaussian(cov=cov)
    assert sorted(kernel.shape) == [7, 13, 17]
    assert LO._rank1_factors(kernel) is None
    A = LO.ConvolutionOperator(3, kernel)
    assert not A.separable
    # the planner is host code: the form is known without a device
    assert A.dense_form((20, 24, 40)) == "tiled"
    assert A.dense_form((20, 24, 40), np.float32) == "tiled"
    long = LO.ConvolutionOperator(1, np.arange(1., 132.))
    assert not long.separable and long.dense_form((300,)) == "plain"


def test_new_entries_are_declared():
    from nsol_amd import _lib
    decl = _lib.declared_symbols()
    for name in ("nsol_corr_dense_tiled_f32", "nsol_corr_dense_tiled_f64",
                 "nsol_corr_dense_tiled_plan"):
        assert name in decl
    assert len(decl["nsol_corr_dense_tiled_f32"][1]) == 17
    assert len(decl["nsol_corr_dense_tiled_plan"][1]) == 11
