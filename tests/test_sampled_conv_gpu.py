"""The blur-and-sample kernels of nsol_amd/csrc/nsol_sample.hip -- nsol_corr_axis_down_*
and its exact transpose nsol_corr_axis_up_* -- through `ops.corr_axis_down` /
`ops.corr_axis_up` and `SampledConvolutionOperator`, against the NumPy restatement of
tests/test_sampled_conv_host.py (pinned there against the dense matrix and
scipy.ndimage).  Needs a real MI355X.

Which kernel a case reaches:
  k_sample_x<UP>            array axis 2 (lanes along the outputs of a row)
  k_sample_rows<VEC, UP>    array axis 0 or 1; VEC = 16 bytes where the rows are whole
                            vectors and both pointers are on the 16-byte grid, else 1
(a 1-D shape is axis 2, a 2-D shape axes 1 and 2 of the padded volume).

Bounds: float64 rel-L2 <= 1e-12.  float32: the rule of tests/test_conv_gpu.py -- at most
4 x the error of the same sums evaluated in float32 NumPy, floor 1e-6.  One-hot inputs
and one-hot taps, and the guard elements around `out`: exact.
Observed over the module's 7000-odd comparisons (one MI355X run):
largest float64 error 4.7e-16; largest float32 error 2.1e-6 (27 random-signed taps)
with the float32 NumPy sums at the same size -- the largest GPU / NumPy ratio is 2.13,
so the factor 4 is the gate that binds there and the floor elsewhere; the adjoint
identity holds to 3e-17 of |Ax| |y|."""
import numpy as np
import pytest

from conftest import rel_l2
from test_pd_linear_host import gaussian_kernel
from test_sampled_conv_host import (MODES, sampled_adjoint, sampled_down,
                                    sampled_extent, sampled_forward, sampled_up)

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12
F32_FLOOR = 1e-6
F32_FACTOR = 4.0
DTYPES = (np.float64, np.float32)
SHAPES = [(5,), (64,), (65,), (1031,), (7, 10), (9, 130), (16, 128), (3, 5, 7),
          (6, 9, 130), (8, 16, 128), (13, 4, 66), (1, 1, 1)]
SENTINEL = -777.25
GUARD = 8


def _taps_set():
    """(name, forward correlation taps, centre): 1, 3, 4 (even, off-centre), 5, 13 and
    27 random-signed taps, and a 13-tap Gaussian."""
    rng = np.random.default_rng(2024)
    out = []
    for n, c in ((1, 0), (3, 1), (4, 0), (5, 2), (13, 6), (27, 13)):
        out.append(("r%d" % n, rng.standard_normal(n), c))
    out.append(("g13", gaussian_kernel(1, 2.), 6))
    assert out[-1][1].size == 13
    return out


TAPS = _taps_set()


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _err(a, b):
    a = np.asarray(a, np.float64).reshape(-1)
    b = np.asarray(b, np.float64).reshape(-1)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda().view(-1)


def _call(up, src, shape, axis, taps, c, mode, f, o, dtype, off=0):
    """The kernel's result on `src` (NumPy, the shape of its side) written into a
    guarded buffer at GUARD + off elements (off = 1: off the 16-byte grid); asserts
    that the guards are untouched."""
    import torch
    from nsol_amd import ops
    d = len(shape)
    out_shape = list(shape)
    if not up:
        out_shape[axis] = sampled_extent(shape[axis], f, o)
    n_out = int(np.prod(out_shape))
    buf = torch.full((n_out + 2 * GUARD + 1,), SENTINEL,
                     dtype=torch.float32 if dtype == np.float32 else torch.float64,
                     device="cuda")
    lo = GUARD + off
    out = buf[lo:lo + n_out]
    fn = ops.corr_axis_up if up else ops.corr_axis_down
    res = fn(_dev(src, dtype), shape, axis + 3 - d, taps, c, mode, f, o, out=out)
    assert res is out
    host = buf.cpu().numpy()
    assert np.all(host[:lo] == SENTINEL) and np.all(host[lo + n_out:] == SENTINEL), \
        "guard elements were written"
    return host[lo:lo + n_out].reshape(out_shape)


class _Worst(object):
    """The worst float64 error, float32 error and float32 GPU / NumPy ratio of a test,
    logged once through conftest.rel_l2 at its end."""

    def __init__(self):
        self.e64 = self.e32 = self.ratio = 0.
        self.count = 0

    def check(self, got, ref64, ref32, dtype, what):
        self.count += 1
        e = _err(got, ref64)
        if dtype == np.float64:
            self.e64 = max(self.e64, e)
            assert e <= F64_TOL, (what, e)
            return
        assert got.dtype == np.float32
        e_ref = _err(ref32, ref64)
        self.e32 = max(self.e32, e)
        if e_ref > 0:
            self.ratio = max(self.ratio, e / e_ref)
        assert e <= max(F32_FACTOR * e_ref, F32_FLOOR), (what, e, e_ref)

    def report(self, what):
        print("%s: %d comparisons, float64 %.3e, float32 %.3e, largest float32 "
              "gpu / numpy ratio %.2f" % (what, self.count, self.e64, self.e32,
                                          self.ratio))
        for label, v in (("e64", self.e64), ("e32", self.e32), ("ratio32", self.ratio)):
            rel_l2(np.array([v]), np.array([0.]), label=label)      # (records v itself)


def _factors(length):
    return [f for f in (1, 2, 3, 4, 5) if f <= length]


# ------------------------------------------------------------------ per axis
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_down_and_up_match_the_restatement(nsol, shape, dtype):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape)
    worst = _Worst()
    k = 0
    for axis in range(len(shape)):
        length = shape[axis]
        for f in _factors(length):
            for o in sorted({0, f - 1}):
                m = sampled_extent(length, f, o)
                qshape = list(shape)
                qshape[axis] = m
                q = rng.standard_normal(qshape)
                for name, w, c in TAPS:
                    for mode in MODES:
                        k += 1
                        off = 1 if k % 3 == 0 else 0       # out off the 16-byte grid
                        what = "%s axis %d f %d o %d %s %s" % (shape, axis, f, o, name,
                                                               mode)
                        got = _call(False, x, shape, axis, w, c, mode, f, o, dtype, off)
                        ref = sampled_down(x, w, c, mode, f, o, axis)
                        ref32 = None if dtype == np.float64 else \
                            sampled_down(x, w, c, mode, f, o, axis, np.float32)
                        worst.check(got, ref, ref32, dtype, "down " + what)
                        got = _call(True, q, shape, axis, w, c, mode, f, o, dtype, off)
                        ref = sampled_up(q, w, c, mode, f, o, axis, length)
                        ref32 = None if dtype == np.float64 else \
                            sampled_up(q, w, c, mode, f, o, axis, length, np.float32)
                        worst.check(got, ref, ref32, dtype, "up " + what)
    worst.report(str(shape))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_one_hot_inputs_and_one_hot_taps_are_exact(nsol, dtype):
    rng = np.random.default_rng(5)
    for shape in ((65,), (9, 130), (8, 16, 128), (3, 5, 7)):
        for axis in range(len(shape)):
            length = shape[axis]
            for f in (1, 2, 3):
                o = f - 1
                m = sampled_extent(length, f, o)
                qshape = list(shape)
                qshape[axis] = m
                for mode in MODES:
                    # one-hot taps: the pass copies (shifted, sampled) values
                    w = np.zeros(5)
                    w[3] = 1.
                    x = rng.standard_normal(shape).astype(dtype)
                    q = rng.standard_normal(qshape).astype(dtype)
                    got = _call(False, x, shape, axis, w, 2, mode, f, o, dtype)
                    assert np.array_equal(got, sampled_down(x, w, 2, mode, f, o, axis,
                                                            dtype))
                    got = _call(True, q, shape, axis, w, 2, mode, f, o, dtype)
                    assert np.array_equal(got, sampled_up(q, w, 2, mode, f, o, axis,
                                                          length, dtype))
                    # one-hot inputs: the pass writes the taps themselves
                    w = rng.standard_normal(7)
                    hot = np.zeros(shape, dtype=dtype)
                    hot[tuple(s // 2 for s in shape)] = 1
                    got = _call(False, hot, shape, axis, w, 3, mode, f, o, dtype)
                    assert np.array_equal(got, sampled_down(hot, w, 3, mode, f, o, axis,
                                                            dtype))
                    hot = np.zeros(qshape, dtype=dtype)
                    hot[tuple(s // 2 for s in qshape)] = 1
                    got = _call(True, hot, shape, axis, w, 3, mode, f, o, dtype)
                    assert np.array_equal(got, sampled_up(hot, w, 3, mode, f, o, axis,
                                                          length, dtype))


# ------------------------------------------------------------------ N-D operators
def _nd_cases():
    """(fine shape, factors, offsets): 2-D and 3-D, mixed factors, extents that are no
    multiples of the factor."""
    return [((7, 10), (2, 3), (1, 2)), ((9, 130), (2, 3), (0, 0)),
            ((16, 128), (4, 2), (3, 1)), ((3, 5, 7), (1, 2, 3), (0, 1, 2)),
            ((6, 9, 130), (3, 1, 2), (2, 0, 1)), ((8, 16, 128), (4, 1, 1), (0, 0, 0)),
            ((13, 4, 66), (2, 2, 2), (1, 0, 1))]


def _factor_kernels(d, rng):
    """Per-axis ndimage.convolve factors: random-signed, different tap counts, one even."""
    sizes = (5, 4, 3)[:d] if d < 3 else (5, 4, 3)
    ks = [rng.standard_normal(n) for n in sizes]
    for k in ks:
        k += np.sign(k.sum()) * 0.5          # a non-zero sum: _rank1_factors needs one
    return ks


def _dense(ks):
    out = ks[0]
    for k in ks[1:]:
        out = np.multiply.outer(out, k)
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _nd_cases(), ids=lambda c: "x".join(map(str, c[0])))
def test_the_operator_is_convolve_then_slice_and_its_adjoint_the_transpose(nsol, case,
                                                                           mode):
    from scipy.ndimage import convolve
    from nsol_amd.linear_operators import SampledConvolutionOperator
    shape, factors, offsets = case
    rng = np.random.default_rng(sum(shape) + len(mode))
    ks = _factor_kernels(len(shape), rng)
    kernel = _dense(ks)
    A = SampledConvolutionOperator(len(shape), kernel, factors, offsets, mode)
    At = A.adjoint(shape)
    x = rng.standard_normal(shape)
    sl = tuple(slice(o, None, f) for o, f in zip(offsets, factors))
    ref = convolve(x, kernel, mode=mode)[sl]
    assert np.max(np.abs(ref - sampled_forward(x, ks, mode, factors, offsets))) <= 1e-12
    worst = _Worst()
    Ax = A(x)
    assert Ax.dtype == np.float64 and Ax.shape == ref.shape == A._out_shape(shape)
    worst.check(Ax, ref, None, np.float64, "A f64")
    got32 = A(x.astype(np.float32))
    worst.check(got32, ref, sampled_forward(x, ks, mode, factors, offsets, np.float32),
                np.float32, "A f32")
    y = rng.standard_normal(ref.shape)
    Aty = At(y)
    assert Aty.shape == tuple(shape)
    ref_t = sampled_adjoint(y, ks, mode, factors, offsets, shape)
    worst.check(Aty, ref_t, None, np.float64, "At f64")
    worst.check(At(y.astype(np.float32)), ref_t,
                sampled_adjoint(y, ks, mode, factors, offsets, shape, np.float32),
                np.float32, "At f32")
    # the adjoint identity, float64
    lhs, rhs = np.vdot(Ax, y), np.vdot(x, Aty)
    gap = abs(lhs - rhs) / (np.linalg.norm(Ax) * np.linalg.norm(y))
    print("adjoint identity: relative gap %.3e" % gap)
    assert gap <= 1e-12
    # device tensors in, device tensors out, the same bits
    import torch
    xd = torch.from_numpy(x).cuda()
    assert np.array_equal(A(xd).cpu().numpy(), Ax)
    worst.report("%s %s" % (shape, mode))


def test_sampled_start_on_the_device(nsol):
    import torch
    from nsol_amd.linear_operators import SampledConvolutionOperator, sampled_start
    from test_sampled_conv_host import numpy_start
    shape, factors, offsets = (6, 9, 130), (3, 1, 2), (2, 0, 1)
    ks = [gaussian_kernel(1, 1.), np.array([0.25, 0.5, 0.25]), np.ones(1)]
    for mode in MODES:
        A = SampledConvolutionOperator(3, _dense(ks), factors, offsets, mode)
        At = A.adjoint(shape)
        b = np.random.default_rng(1).random(A._out_shape(shape)) + 1.
        ref = numpy_start(b, ks, mode, factors, offsets, shape)
        # the one-tap x axis with f = 2: every other fine voxel is seen by no sample
        assert np.count_nonzero(ref == 0) == ref.size // 2
        got = sampled_start(At, b, shape)
        assert got.shape == shape and rel_l2(got, ref, mode) <= F64_TOL
        assert np.array_equal(got == 0, ref == 0)
        dev = sampled_start(At, torch.from_numpy(b).cuda(), shape)
        assert np.array_equal(dev.cpu().numpy(), got)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_every_einval_leaves_out_untouched(nsol, dtype, up):
    import torch
    from nsol_amd import _lib
    from nsol_amd.device import stream_ptr
    lib = _lib.load()
    fn = getattr(lib, "nsol_corr_axis_%s_%s" % ("up" if up else "down",
                                                "f64" if dtype == np.float64 else "f32"))
    td = torch.float64 if dtype == np.float64 else torch.float32
    src = torch.ones(4 * 5 * 6, dtype=td, device="cuda")
    out = torch.full((4 * 5 * 6,), SENTINEL, dtype=td, device="cuda")
    taps = np.array([0.25, 0.5, 0.25])

    def call(s=src, o=out, axis=1, dims=(4, 5, 6), t=taps.ctypes.data, ntaps=3, centre=1,
             mode=1, factor=2, offset=1):
        return fn(None if s is None else s.data_ptr(), None if o is None else o.data_ptr(),
                  axis, *dims, t, ntaps, centre, mode, factor, offset, stream_ptr())
    bad = [dict(s=None), dict(o=None), dict(o=src), dict(t=None),
           dict(dims=(0, 5, 6)), dict(dims=(4, 0, 6)), dict(dims=(4, 5, 0)),
           dict(dims=(-1, 5, 6)), dict(axis=-1), dict(axis=3), dict(ntaps=0),
           dict(ntaps=130), dict(centre=-1), dict(centre=3), dict(mode=2), dict(mode=3),
           dict(mode=4), dict(mode=-1), dict(mode=5), dict(factor=0), dict(factor=-2),
           dict(offset=-1), dict(offset=2), dict(factor=9, offset=5),   # offset >= len
           dict(axis=0, factor=7, offset=4)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL) and torch.all(src == 1)
    assert call() == 0                                   # and the good call runs
    torch.cuda.synchronize()
    n_out = 4 * 5 * 6 if up else 4 * 2 * 6
    assert torch.all(out[:n_out] != SENTINEL)
    # the Python wrappers refuse before the library sees the call
    from nsol_amd import ops
    f = ops.corr_axis_up if up else ops.corr_axis_down
    x = torch.ones(4 * (2 if up else 5) * 6, dtype=td, device="cuda")
    for kw in (dict(mode="reflect"), dict(mode="nearest"), dict(mode="mirror"),
               dict(factor=0), dict(offset=2), dict(offset=-1), dict(axis3=3)):
        args = dict(axis3=1, taps=taps, centre=1, mode="wrap", factor=2, offset=1)
        args.update(kw)
        with pytest.raises(ValueError):
            f(x, (4, 5, 6), **args)
    with pytest.raises(ValueError):
        f(x[:-1], (4, 5, 6), 1, taps, 1, "wrap", 2, 1)
    with pytest.raises(ValueError):
        f(x, (4, 5, 6), 1, taps, 1, "wrap", 2, 1, out=out[:7])


# ------------------------------------------------------------------ 64-bit indexing
def test_a_row_beyond_2_to_the_31_elements(nsol):
    """One float32 row of 2^31 + 64 elements, f = 4, o = 3, 5 taps: the first and last
    256 outputs of `down`, and of `up` writing a row of that length, against NumPy on
    the matching ends."""
    import torch
    from nsol_amd import ops
    n, f, o, c = (1 << 31) + 64, 4, 3, 2
    m = sampled_extent(n, f, o)
    w = np.array([0.1, -0.3, 0.5, 0.4, 0.2])
    ends = 256
    try:
        x = torch.empty(n, dtype=torch.float32, device="cuda")
        q = torch.empty(m, dtype=torch.float32, device="cuda")
        step = 1 << 27
        for a in range(0, n, step):                     # x[i] = (i mod 251) / 8 - 15
            b = min(a + step, n)
            i = torch.arange(a, b, dtype=torch.int64, device="cuda")
            x[a:b] = (i % 251).to(torch.float32) / 8 - 15
            del i
        for a in range(0, m, step):                     # q[k] = (k mod 241) / 4 - 30
            b = min(a + step, m)
            i = torch.arange(a, b, dtype=torch.int64, device="cuda")
            q[a:b] = (i % 241).to(torch.float32) / 4 - 30
            del i
        down = ops.corr_axis_down(x, (n,), 2, w, c, "constant", f, o)
        assert down.numel() == m
        d_lo, d_hi = down[:ends].cpu().numpy(), down[-ends:].cpu().numpy()
        del down, x
        up = ops.corr_axis_up(q, (n,), 2, w, c, "constant", f, o)
        assert up.numel() == n
        u_lo, u_hi = up[:ends].cpu().numpy(), up[-ends:].cpu().numpy()
        del up, q
    except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
        if "out of memory" not in str(e).lower():
            raise
        pytest.skip("no room for a row of 2^31 + 64 float32: %s" % e)
    fx = lambda i: ((i % 251) / 8. - 15.).astype(np.float32)
    fq = lambda k: ((k % 241) / 4. - 30.).astype(np.float32)
    # down: outputs j read x[o + j f - c .. + 4]; constant mode = zero outside the row
    j = np.concatenate([np.arange(ends), np.arange(m - ends, m)])
    ref = np.zeros(j.size, np.float32)
    for t in range(5):
        pos = o + j * f - c + t
        ok = (pos >= 0) & (pos < n)
        ref = ref + np.float32(w[t]) * np.where(ok, fx(pos), np.float32(0))
    assert np.array_equal(np.concatenate([d_lo, d_hi]), ref)
    # up: output i gathers q[(i + c - t - o) / f] where that is a kept sample
    i = np.concatenate([np.arange(ends), np.arange(n - ends, n)])
    ref = np.zeros(i.size, np.float32)
    for t in range(5):
        P = i + c - t
        ok = (P >= 0) & (P < n) & (P >= o) & ((P - o) % f == 0) & ((P - o) // f < m)
        ref = ref + np.float32(w[t]) * np.where(ok, fq(np.clip((P - o) // f, 0, m - 1)),
                                               np.float32(0))
    assert np.array_equal(np.concatenate([u_lo, u_hi]), ref)
    assert np.any(u_hi != 0) and np.any(d_hi != 0)
