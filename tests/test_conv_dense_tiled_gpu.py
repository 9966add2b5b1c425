"""The tiled dense correlation k_corr_dense_tile (nsol_amd/csrc/nsol_convd.hip) on a real
MI355X, through ops.corr_dense_tiled (ctypes -> C ABI) and ConvolutionOperator.

Its contract is BIT IDENTITY with ops.corr_dense (k_corr_dense): the same accumulation
order with a separate multiply and add.  Every forced case reads the plan back and asserts
the seams it is there for -- at least two tiles and a ragged last one along every tiled
axis, at least two slabs along z -- so that no case passes by running as a single tile.
Three cases are also held against oracle.nsol_oracle.convolve_nd (float64 at
test_conv_gpu's F64_TOL, float32 through its _check_float32), which excludes identity
with a plain kernel that is wrong in the same way.

Then ConvolutionOperator's switch (dense_form), its exact transpose on the device, and
the linear primal-dual solvers and their batch on an (A, A.transpose()) pair."""
import ctypes

import numpy as np
import pytest

from conftest import rel_l2
from test_conv_gpu import F64_TOL, _check_float32

pytestmark = pytest.mark.gpu

MODES = ("constant", "wrap", "nearest", "reflect", "mirror")
DTYPES = (np.float64, np.float32)
AUTO = (0, 0, 0)


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda().view(-1)


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _pad3(t):
    t = tuple(t)
    return (1,) * (3 - len(t)) + t


def _ndimage_centre(kshape):
    return tuple(s // 2 - (1 if s % 2 == 0 else 0) for s in kshape)


def _assert_seams(shape, k3, dtype, tile, axes):
    """axes: (z, y, x) booleans -- the axes this case is there to cut."""
    from nsol_amd import ops
    plan = ops.corr_dense_tiled_plan(shape, k3, np.dtype(dtype).itemsize, tile)
    assert plan is not None, (shape, k3, tile)
    nz, ny, nx = _pad3(shape)
    assert tile[0] == 0 or plan["ty"] == tile[0]
    assert tile[1] == 0 or plan["tx"] == tile[1]
    assert tile[2] == 0 or plan["slab"] == min(tile[2], nz)
    if axes[2]:
        assert plan["ntx"] >= 2 and nx % plan["tx"] != 0, (shape, plan)
    if axes[1]:
        assert plan["nty"] >= 2 and ny % plan["ty"] != 0, (shape, plan)
    if axes[0]:
        assert plan["nslab"] >= 2, (shape, plan)
    assert plan["blocks"] == plan["ntx"] * plan["nty"] * plan["nslab"] >= 2
    return plan


def _identical(x, taps, centre, mode, dtype, tile, axes=None):
    """Runs both kernels on x (N-D) with correlation taps (N-D) and asserts equal bits;
    returns the tiled result as an array of x's shape.  tile AUTO: the planner's choice,
    which may decline -- then the plan says so too, and the plain result is returned."""
    from nsol_amd import ops
    shape = x.shape
    k3, c3 = _pad3(taps.shape), (0,) * (3 - taps.ndim) + tuple(centre)
    xd, td = _dev(x, dtype), _dev(taps, dtype)
    plain = ops.corr_dense(xd, shape, td, k3, c3, mode)
    if tile != AUTO:
        _assert_seams(shape, k3, dtype, tile, axes)
    tiled = ops.corr_dense_tiled(xd, shape, td, k3, c3, mode, tile=tile)
    planned = ops.corr_dense_tiled_plan(shape, k3, np.dtype(dtype).itemsize, tile)
    assert (tiled is None) == (planned is None)
    if tiled is None:
        assert tile == AUTO, "a forced tile must run"
        return plain.cpu().numpy().reshape(shape)
    assert tiled.dtype == plain.dtype
    assert np.array_equal(_bits(tiled), _bits(plain)), (shape, taps.shape, centre, mode, tile)
    return tiled.cpu().numpy().reshape(shape)


def _case(shape, kshape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), rng.standard_normal(kshape)


# ------------------------------------------------------------- bit identity
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mode", MODES)
def test_small_extents_fold_more_than_once(nsol, mode, dtype):
    """Extents 1, 2, 3, k - 1, k and 2 k + 1 on each axis in turn under a 3 x 4 x 5
    kernel; the two other axes stay cut by the forced tile (3, 8, 2)."""
    kshape, base, tile = (3, 4, 5), [5, 7, 13], (3, 8, 2)
    for axis in range(3):
        k = kshape[axis]
        for e in sorted({1, 2, 3, k - 1, k, 2 * k + 1}):
            shape = list(base)
            shape[axis] = e
            x, taps = _case(shape, kshape, 100 * axis + e)
            cut = [shape[0] > tile[2], shape[1] > tile[0] and shape[1] % tile[0] != 0,
                   shape[2] > tile[1] and shape[2] % tile[1] != 0]
            assert all(cut[a] for a in range(3) if a != axis)
            _identical(x, taps, _ndimage_centre(kshape), mode, dtype, tile, cut)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mode", MODES)
def test_volume_with_every_centre(nsol, mode, dtype):
    """(5, 19, 70) under 3 x 4 x 5 taps: the centre where ndimage has it, at 0 and at
    k - 1 (the C ABI takes any centre inside the kernel); forced tile and the planner's."""
    shape, kshape = (5, 19, 70), (3, 4, 5)
    x, taps = _case(shape, kshape, 7)
    for centre in (_ndimage_centre(kshape), (0, 0, 0), (2, 3, 4)):
        _identical(x, taps, centre, mode, dtype, (6, 16, 2), (True, True, True))
        _identical(x, taps, centre, mode, dtype, AUTO)
    # ... and the planner's own choice on a volume large enough for it to take
    big, _ = _case((9, 35, 70), kshape, 8)
    from nsol_amd import ops
    assert ops.corr_dense_tiled_plan(big.shape, kshape, np.dtype(dtype).itemsize) is not None
    _identical(big, taps, _ndimage_centre(kshape), mode, dtype, AUTO)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mode", MODES)
def test_kernel_larger_than_the_tile_and_lower_dimensions(nsol, mode, dtype):
    # 1 x 9 x 21 taps on tiles of 4 x 16: the halo is larger than the tile itself
    x, taps = _case((19, 70), (9, 21), 11)
    _identical(x, taps, (4, 10), mode, dtype, (4, 16, 1), (False, True, True))
    _identical(x, taps, (4, 10), mode, dtype, AUTO)
    # 1-D, 6 taps
    x, taps = _case((70,), (6,), 12)
    _identical(x, taps, (2,), mode, dtype, (1, 16, 1), (False, False, True))
    _identical(x, taps, (2,), mode, dtype, AUTO)
    # 2-D, 5 x 2 taps
    x, taps = _case((19, 70), (5, 2), 13)
    _identical(x, taps, (2, 0), mode, dtype, (4, 16, 1), (False, True, True))
    _identical(x, taps, (2, 0), mode, dtype, AUTO)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("nx,offset", [(63, 0), (63, 1), (64, 0), (64, 1)])
def test_ragged_rows_and_operands_off_the_16_byte_grid(nsol, dtype, nx, offset):
    """Rows of 63 (no whole vectors) and of 64, operands on the 16-byte grid and one
    element off it: the scalar store form of the same kernel.  The elements before and
    after `out` keep their bits."""
    import torch
    from nsol_amd import ops
    kshape, guard = (3, 3, 5), 8
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    k3, c3 = kshape, _ndimage_centre(kshape)
    # a forced tile on a tiny volume; the planner's own on one large enough for it to take
    for shape, tile in (((3, 5, nx), (2, 24, 2)), ((12, 33, nx), AUTO)):
        n = int(np.prod(shape))
        x, taps = _case(shape, kshape, nx + offset)
        td = _dev(taps, dtype)
        if tile != AUTO:
            _assert_seams(shape, k3, dtype, tile, (True, True, True))
        else:
            plan = ops.corr_dense_tiled_plan(shape, k3, np.dtype(dtype).itemsize)
            assert plan is not None and plan["blocks"] >= 30 and plan["ntx"] >= 2
        for mode in ("wrap", "reflect"):
            xbuf = torch.zeros(n + 4, dtype=tdt, device="cuda")
            xd = xbuf[offset:offset + n]
            xd.copy_(_dev(x, dtype))
            assert xd.data_ptr() % 16 == (offset * xd.element_size()) % 16
            plain = ops.corr_dense(xd.clone(), shape, td, k3, c3, mode)
            obuf = torch.full((n + 2 * guard + 4,), -7.25, dtype=tdt, device="cuda")
            lo = guard + offset
            got = ops.corr_dense_tiled(xd, shape, td, k3, c3, mode, tile=tile,
                                       out=obuf[lo:lo + n])
            assert got is not None
            assert np.array_equal(_bits(obuf[lo:lo + n]), _bits(plain)), (mode, tile)
            rest = torch.cat([obuf[:lo], obuf[lo + n:]]).cpu().numpy()
            assert rest.size == 2 * guard + 4 and np.all(rest == -7.25), (mode, tile)


def test_131_taps_decline_and_the_operator_still_answers(nsol):
    from oracle import nsol_oracle as orc
    from nsol_amd import ops
    import nsol_amd.linear_operators as LO
    rng = np.random.default_rng(3)
    kernel = rng.standard_normal(131)
    x = rng.standard_normal(300)
    A = LO.ConvolutionOperator(1, kernel, "reflect")
    assert not A.separable and A.dense_form(x.shape) == "plain"
    k3, c3 = A._dense3()
    assert ops.corr_dense_tiled(_dev(x, np.float64), x.shape, _dev(A._flipped, np.float64),
                                k3, c3, "reflect") is None
    assert ops.corr_dense_tiled(_dev(x, np.float64), x.shape, _dev(A._flipped, np.float64),
                                k3, c3, "reflect", tile=(1, 16, 1)) is None
    assert rel_l2(A(x), orc.convolve_nd(x, kernel, "reflect")) <= F64_TOL


def test_bad_arguments_are_value_errors(nsol):
    import torch
    from nsol_amd import _lib, ops
    shape, kshape = (4, 6, 16), (3, 3, 3)
    n = int(np.prod(shape))
    x, taps = _case(shape, kshape, 1)
    buf = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    buf[:n].copy_(_dev(x, np.float64))
    td = _dev(taps, np.float64)
    for out in (buf[:n], buf[n // 2:n // 2 + n], buf[n - 1:2 * n - 1]):
        with pytest.raises(ValueError):
            ops.corr_dense_tiled(buf[:n], shape, td, kshape, (1, 1, 1), "wrap", out=out)
    assert torch.all(buf[n:] == 0)
    # (a volume this small is below the planner's workgroup threshold: a forced tile)
    assert ops.corr_dense_tiled(buf[:n], shape, td, kshape, (1, 1, 1), "wrap",
                                out=buf[n:]) is None
    assert torch.all(buf[n:] == 0)
    assert ops.corr_dense_tiled(buf[:n], shape, td, kshape, (1, 1, 1), "wrap",
                                tile=(2, 8, 2), out=buf[n:]) is not None
    for centre in ((3, 1, 1), (1, -1, 1), (1, 1, 3)):
        with pytest.raises(ValueError):
            ops.corr_dense_tiled(buf[:n], shape, td, kshape, centre, "wrap")
        with pytest.raises(ValueError):
            ops.corr_dense_tiled(buf[:n], shape, td, kshape, centre, "wrap", tile=(2, 8, 2),
                                 out=buf[n:])
    # ... and through the C ABI itself
    assert _lib.load().nsol_corr_dense_tiled_f64(
        buf[:n].data_ptr(), buf[n:].data_ptr(), 4, 6, 16, td.data_ptr(), 3, 3, 3, 3, 1, 1, 1,
        2, 8, 2, None) == -1
    # forced tiles the kernel cannot run: tx no multiple of 4, a ring over 160 KiB
    for tile in ((2, 6, 1), (4096, 4096, 1)):
        with pytest.raises(ValueError):
            ops.corr_dense_tiled(buf[:n], shape, td, kshape, (1, 1, 1), "wrap", tile=tile)
    # a null pointer, through the C ABI itself
    lib = _lib.load()
    assert lib.nsol_corr_dense_tiled_f64(None, buf[n:].data_ptr(), 4, 6, 16, td.data_ptr(),
                                         3, 3, 3, 1, 1, 1, 1, 0, 0, 0, None) == -1
    assert lib.nsol_corr_dense_tiled_plan(4, 6, 16, 3, 3, 3, 8, 0, 0, 0, None) == -1
    plan = (ctypes.c_int64 * 8)()
    assert lib.nsol_corr_dense_tiled_plan(4, 6, 16, 3, 3, 131, 8, 0, 0, 0,
                                          ctypes.addressof(plan)) == -2


# ---------------------------------------------------- against the float64 oracle
ORACLE_CASES = [((5, 19, 70), (3, 4, 5), (6, 16, 2), (True, True, True), "reflect"),
                ((19, 70), (9, 21), (4, 16, 1), (False, True, True), "wrap"),
                ((7, 3, 13), (3, 4, 5), (3, 8, 2), (True, False, True), "constant")]


@pytest.mark.parametrize("shape,kshape,tile,axes,mode", ORACLE_CASES,
                         ids=[str(c[0]) for c in ORACLE_CASES])
def test_against_the_oracle(nsol, shape, kshape, tile, axes, mode):
    from oracle import nsol_oracle as orc
    import nsol_amd.linear_operators as LO
    x, kernel = _case(shape, kshape, 21)
    A = LO.ConvolutionOperator(len(shape), kernel, mode)
    assert not A.separable
    ref = orc.convolve_nd(x, kernel, mode)
    got = _identical(x, A._flipped, A._centre, mode, np.float64, tile, axes)
    e64 = rel_l2(got, ref, label="tiled64")
    print(shape, mode, "float64 %.3e" % e64)
    assert e64 <= F64_TOL
    got32 = _identical(x, A._flipped, A._centre, mode, np.float32, tile, axes)
    _check_float32(got32, x, kernel, mode, ref, "tiled %r %s" % (shape, mode))


# ------------------------------------------------------------ the operator
def _oriented_gaussian():
    from nsol_amd import kernels as K
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    R = np.array([[1., 0., 0.], [0., c, -s], [0., s, c]])
    return K.Kernels3D().get_gaussian(cov=R @ np.diag([1., 1., 9.]) @ R.T)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_operator_runs_the_oriented_gaussian_tiled(nsol, dtype):
    from nsol_amd import ops
    from nsol_amd.device import to_device
    import nsol_amd.linear_operators as LO
    kernel = _oriented_gaussian()
    assert kernel.size == 1547
    shape = (20, 24, 40)
    A = LO.ConvolutionOperator(3, kernel)
    assert A.dense_form(shape, dtype) == "tiled"
    assert A._launches(shape) == 1 and A.stacked_launches(shape, 3) == 3
    x = np.random.default_rng(2).standard_normal(shape)
    xd = to_device(x, dtype)
    got = A(xd)
    k3, c3 = A._dense3()
    plain = ops.corr_dense(xd.view(-1), shape, _dev(A._flipped, dtype), k3, c3, "wrap")
    assert np.array_equal(_bits(got.reshape(-1)), _bits(plain))
    # the switch: the plain kernel, the same bits
    LO.USE_TILED_DENSE = False
    try:
        assert A.dense_form(shape, dtype) == "plain"
        assert np.array_equal(_bits(A(xd).reshape(-1)), _bits(plain))
    finally:
        LO.USE_TILED_DENSE = True
    # member by member over a stack, through the same switch
    stack = to_device(np.stack([x, 2 * x, x[::-1]]), dtype).view(-1)
    out = A._apply_stacked(stack, shape, 3)
    n = x.size
    assert np.array_equal(_bits(out[:n]), _bits(plain))
    assert np.array_equal(_bits(out[2 * n:]),
                          _bits(A(to_device(x[::-1].copy(), dtype)).reshape(-1)))


@pytest.mark.parametrize("mode", ["wrap", "constant"])
def test_transpose_on_the_device(nsol, mode):
    import torch
    from nsol_amd.device import to_device
    import nsol_amd.linear_operators as LO
    rng = np.random.default_rng(4)
    kernel = rng.standard_normal((3, 4, 2))
    shape = (6, 7, 9)
    A = LO.ConvolutionOperator(3, kernel, mode)
    At = A.transpose()
    x, y = (to_device(rng.standard_normal(shape), np.float64) for _ in range(2))
    Ax, Aty = A(x), At(y)
    lhs, rhs = float(torch.sum(Ax * y)), float(torch.sum(x * Aty))
    scale = float(torch.linalg.norm(Ax) * torch.linalg.norm(y))
    print(mode, "adjoint mismatch %.3e" % (abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-12 * scale


# ------------------------------------------------------------ the solvers
PSF = np.array([[0.00, 0.02, 0.05, 0.01],
                [0.01, 0.06, 0.12, 0.03],
                [0.03, 0.15, 0.20, 0.04],
                [0.02, 0.08, 0.09, 0.02],
                [0.00, 0.03, 0.03, 0.01]])
SHAPE2 = (24, 40)


def _observation(seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:SHAPE2[0], :SHAPE2[1]]
    return 1. + ((yy // 6 + xx // 8) % 2) + 0.05 * rng.standard_normal(SHAPE2)


def _linear_solver(nsol, cls, obs, A=None, A_adj=None, alpha=0.05, **kw):
    import nsol_amd.linear_operators as LO
    if A is None:
        op, op_adj = LO.LinearOperators2D().get_convolution_and_adjoint_convolution_operators(
            PSF, exact_adjoint=True)
        assert not op.separable and op_adj is not op
        A = lambda v: op(v.reshape(*SHAPE2)).flatten()
        A_adj = lambda v: op_adj(v.reshape(*SHAPE2)).flatten()
    return cls(A=A, A_adj=A_adj, b=obs.flatten(), x0=obs.flatten(), dimension=2,
               alpha=alpha, iterations=15, dtype=np.float64, x_scale=obs.max(), **kw)


@pytest.mark.parametrize("which", ["PrimalDualLinearSolver", "TGVPrimalDualLinearSolver"])
def test_solvers_recognise_the_exact_pair(nsol, which):
    """Through the caller's lambdas the solver finds (A, A.transpose()) and runs fused;
    the same two operators hidden in foreign device callables give the same x."""
    from nsol_amd.device import is_device_tensor
    import nsol_amd.linear_operators as LO
    cls = getattr(nsol, which)
    obs = _observation()
    fused = _linear_solver(nsol, cls, obs)
    fused.run()
    assert fused.get_execution() == "fused"
    assert fused._op is not fused._op_adj
    np.testing.assert_array_equal(fused._op_adj.kernel, fused._op.transpose().kernel)
    op, op_adj = LO.LinearOperators2D().get_convolution_and_adjoint_convolution_operators(
        PSF, exact_adjoint=True)

    def opaque(o):
        def f(t):
            if not is_device_tensor(t):
                raise TypeError("device tensors only")
            return o(t.view(*SHAPE2)).reshape(-1)
        return f
    dev = _linear_solver(nsol, cls, obs, A=opaque(op), A_adj=opaque(op_adj),
                         A_norm2=float(np.abs(PSF).sum()) ** 2, shape=SHAPE2)
    dev.run()
    assert dev.get_execution() == "device"
    err = rel_l2(dev.get_x(), fused.get_x(), which)
    print(which, "fused against device callables: %.3e, bits equal: %s" %
          (err, np.array_equal(dev.get_x(), fused.get_x())))
    assert err <= 1e-12
    assert np.all(np.isfinite(fused.get_x()))
    # the exact transpose matters: the reference's (A, A) pair is another problem
    same = LO.ConvolutionOperator(2, PSF)
    other = _linear_solver(nsol, cls, obs,
                           A=lambda v: same(v.reshape(*SHAPE2)).flatten(),
                           A_adj=lambda v: same(v.reshape(*SHAPE2)).flatten())
    other.run()
    assert rel_l2(other.get_x(), fused.get_x()) > 1e-6


def test_a_batch_of_exact_pairs_stacks(nsol):
    solvers = [_linear_solver(nsol, nsol.PrimalDualLinearSolver, _observation(k))
               for k in range(3)]
    own = [_linear_solver(nsol, nsol.PrimalDualLinearSolver, _observation(k))
           for k in range(3)]
    batch = nsol.PrimalDualLinearBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["stacked"] * 3
    for s, o in zip(solvers, own):
        o.run()
        assert np.array_equal(s.get_x(), o.get_x())
