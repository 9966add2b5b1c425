"""Member-stacked TGV on the GPU: k_tgv_dual_stack / k_tgv_primal_stack /
k_tgv_primal_w_stack through the C ABI, bit for bit against the single entries on every
member's arrays and against the NumPy restatement (nsol_amd/tgv_numpy.py); members that do
not see each other, guard bands, the entries that must decline; TGVPrimalDualBatch and
TGVPrimalDualSweep against the members' own runs."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from device_arena import Arena
from nsol_amd import tgv_numpy as tg

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12     # float64 kernels vs the float64 restatement
F32_TOL = 1e-5      # the project's standing gate
BOTH = [np.float64, np.float32]
SPACING = (0.8, 1.3, 2.0)          # spacing[0] belongs to the last array axis
BETA, SIGMA, TAU, TL, THETA = 1.7, 0.3, 0.4, 0.6, 0.9
ISO, L1 = 4, 2                      # NSOL_PD_REG_ISOTROPIC, NSOL_PD_DATA_L1
# every member its own beta and tl
BETAS = (0.6 * BETA, BETA, 1.5 * BETA)
TLS = (0.25, TL, 1.9)

# a row shorter than a vector, ragged rows that cross an x tile, a row count that is no
# multiple of ROWS, extents of 1, whole aligned rows
SHAPES = [(5,), (259,), (6, 259), (5, 7), (1, 9), (9, 1), (2, 1, 5), (3, 5, 7),
          (4, 6, 259), (5, 4, 64)]
STRADDLING = ((6, 259), (4, 6, 259), (5, 4, 64))
DUAL_ARRAYS = ("xbar", "wbar", "p", "q")
PRIMAL_ARRAYS = ("p", "q", "x", "xbar", "w", "wbar", "bt")


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


def _suffix(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _iw(d):
    return [1. / SPACING[a] if a < d else 1. for a in range(3)]


def _dims(shape):
    return (len(shape),) + (1,) * (3 - len(shape)) + tuple(shape)


def _fn(name, dtype):
    from nsol_amd import _lib
    return getattr(_lib.load(), "nsol_%s_%s" % (name, _suffix(dtype)))


def _raw(t):
    """The tensor's bytes."""
    return t.detach().cpu().numpy().view(np.uint8).copy()


@functools.lru_cache(maxsize=None)
def _state(shape, dtype, m):
    """Member m's random state, rounded to dtype and held in float64, as test_tgv_gpu.py
    builds its own: dual variables on both sides of both projections, weights in [0, 2)
    with a fifth of them 0.  Never modified."""
    rng = np.random.default_rng(2000 + sum(shape) + len(shape) + 101 * m)
    d, M = len(shape), tg.components(len(shape))
    r = lambda *s, scale=1.: (scale * rng.standard_normal(s)).astype(dtype).astype(
        np.float64)
    st = dict(xbar=r(*shape), wbar=r(d, *shape), p=r(d, *shape, scale=0.7),
              q=r(M, *shape, scale=0.7 * BETA), x=r(*shape), w=r(d, *shape),
              bt=r(*shape))
    wt = 2. * rng.random(shape) * (rng.random(shape) > 0.2)
    st["wt"] = wt.astype(dtype).astype(np.float64)
    for v in st.values():
        v.setflags(write=False)
    return st


def _rounded_spacing(shape, dtype):
    """The spacing whose inverse is the inverse the kernels use (1/h rounded to dtype)."""
    return tuple(1. / float(np.dtype(dtype).type(1. / h)) for h in SPACING[:len(shape)])


def _c(dtype, v):
    return float(np.dtype(dtype).type(v))


@functools.lru_cache(maxsize=None)
def _inside(shape, dtype, m):
    """Fractions of member m's p and q components that its projections leave alone."""
    s = _state(shape, dtype, m)
    g, e = tg.K(s["xbar"], s["wbar"], _rounded_spacing(shape, dtype))
    return (float(np.mean(np.abs(s["p"] + _c(dtype, SIGMA) * g) <= 1.)),
            float(np.mean(np.abs(s["q"] + _c(dtype, SIGMA) * e) <= _c(dtype, BETAS[m]))))


def _assert_straddles(shape, dtype, P):
    """Every member has at least 2 % of its p components inside its projection and 2 %
    outside, and the same of its q: asserted on the CPU, before any launch."""
    if shape in STRADDLING:
        for m in range(P):
            for f in _inside(shape, dtype, m):
                assert 0.02 <= f <= 0.98, (shape, m, _inside(shape, dtype, m))


@functools.lru_cache(maxsize=None)
def _want_dual(shape, dtype, m, iso):
    s = _state(shape, dtype, m)
    return tg.dual_step(s["xbar"], s["wbar"], s["p"], s["q"], _c(dtype, SIGMA),
                        _c(dtype, BETAS[m]), _rounded_spacing(shape, dtype), iso)


@functools.lru_cache(maxsize=None)
def _want_primal(shape, dtype, m, l1, weighted, data):
    """data: the member whose bt and wt member m reads (0 where they are shared)."""
    s, sd = _state(shape, dtype, m), _state(shape, dtype, data)
    args = (_c(dtype, TAU), _c(dtype, TLS[m]), _c(dtype, THETA),
            _rounded_spacing(shape, dtype), "ell1" if l1 else "ell2")
    if weighted:
        return tg.primal_step_weighted(s["p"], s["q"], s["x"], s["w"], sd["bt"], sd["wt"],
                                       *args)
    return tg.primal_step(s["p"], s["q"], s["x"], s["w"], sd["bt"], *args)


# ---- the single entries on one member's arrays: what every stacked member must equal
@functools.lru_cache(maxsize=None)
def _single_dual(shape, dtype, m, iso):
    import torch
    from nsol_amd.device import stream_ptr
    s = _state(shape, dtype, m)
    ar = Arena({k: s[k] for k in DUAL_ARRAYS}, dtype)
    assert _fn("tgv_dual", dtype)(
        *[ar.ptr(k) for k in DUAL_ARRAYS], *_dims(shape), *_iw(len(shape)), SIGMA,
        BETAS[m], ISO if iso else 0, stream_ptr()) == 0
    torch.cuda.synchronize()
    return {k: _raw(ar.t[k]) for k in ("p", "q")}


def _single_primal_on(shape, dtype, m, l1, arrays):
    import torch
    from nsol_amd.device import stream_ptr
    weighted = "wt" in arrays
    ar = Arena(arrays, dtype)
    names = PRIMAL_ARRAYS + (("wt",) if weighted else ())
    assert _fn("tgv_primal_w" if weighted else "tgv_primal", dtype)(
        *[ar.ptr(k) for k in names], *_dims(shape), *_iw(len(shape)), TAU, TLS[m], THETA,
        L1 if l1 else 0, stream_ptr()) == 0
    torch.cuda.synchronize()
    return {k: _raw(ar.t[k]) for k in ("x", "xbar", "w", "wbar")}


@functools.lru_cache(maxsize=None)
def _single_primal(shape, dtype, m, l1, weighted, data):
    s, sd = _state(shape, dtype, m), _state(shape, dtype, data)
    arrays = {k: (sd if k == "bt" else s)[k] for k in PRIMAL_ARRAYS}
    if weighted:
        arrays["wt"] = sd["wt"]
    return _single_primal_on(shape, dtype, m, l1, arrays)


def _stacked(shape, dtype, P, names, strided=True, poison=None):
    """The members' arrays one after the other; bt and wt of member 0 alone where they
    are shared.  poison: the member whose whole state is NaN."""
    out = {}
    for k in names:
        if k in ("bt", "wt") and not strided:
            out[k] = _state(shape, dtype, 0)[k].reshape(-1).copy()
            continue
        parts = [_state(shape, dtype, m)[k].reshape(-1).copy() for m in range(P)]
        if poison is not None:
            parts[poison][:] = np.nan
        out[k] = np.concatenate(parts)
    return out


def _table(like, P):
    from nsol_amd import ops
    tab = ops.tgv_stack_table(like, BETAS[:P], TLS[:P])
    assert tab is not None
    return tab


def _member(raw, m, P):
    size = raw.size // P
    return raw[m * size:(m + 1) * size]


def _bytes_of(values, dtype):
    """The bytes of float64-held values that are exact in dtype."""
    return values.astype(dtype).view(np.uint8)


def _as_f64(raw, dtype, shape):
    return raw.view(dtype).astype(np.float64).reshape(shape)


def _check_dual(shape, dtype, P, iso, offset=0, last=None, poison=None):
    import torch
    from nsol_amd.device import stream_ptr
    _assert_straddles(shape, dtype, P)
    d, M = len(shape), tg.components(len(shape))
    host = _stacked(shape, dtype, P, DUAL_ARRAYS, poison=poison)
    ar = Arena(host, dtype, offset, last)
    tab = _table(ar.buf, P)
    assert _fn("tgv_stack_dual", dtype)(
        *[ar.ptr(k) for k in DUAL_ARRAYS], P, *_dims(shape), *_iw(d), SIGMA,
        tab.data_ptr(), ISO if iso else 0, stream_ptr()) == 0
    torch.cuda.synchronize()
    got = {k: _raw(ar.t[k]) for k in DUAL_ARRAYS}
    label = "dual %r P=%d iso=%d off=%d last=%s" % (shape, P, iso, offset, last)
    for m in range(P):
        if m == poison:
            continue
        want = _single_dual(shape, dtype, m, iso)
        for k in ("p", "q"):
            assert np.array_equal(_member(got[k], m, P), want[k]), (label, m, k)
    assert ar.guards_intact(), label
    if poison is None:
        for k in ("xbar", "wbar"):                      # the inputs are only read
            assert np.array_equal(got[k], _bytes_of(host[k], dtype)), (label, k)
        m = P - 1                                       # the last member, restated
        p, q = _want_dual(shape, dtype, m, iso)
        ep = rel_l2(_as_f64(_member(got["p"], m, P), dtype, (d,) + shape), p, label + " p")
        eq = rel_l2(_as_f64(_member(got["q"], m, P), dtype, (M,) + shape), q, label + " q")
        print("%s %s: p %.3g q %.3g" % (label, _suffix(dtype), ep, eq))
        assert ep <= _gate(dtype) and eq <= _gate(dtype)


def _check_primal(shape, dtype, P, l1, weighted, strided, offset=0, last=None,
                  poison=None):
    import torch
    from nsol_amd.device import stream_ptr
    d = len(shape)
    names = PRIMAL_ARRAYS + (("wt",) if weighted else ())
    host = _stacked(shape, dtype, P, names, strided, poison)
    ar = Arena(host, dtype, offset, last)
    tab = _table(ar.buf, P)
    n = int(np.prod(shape))
    stride = n if strided else 0
    args = [ar.ptr(k) for k in PRIMAL_ARRAYS] + [stride]
    if weighted:
        args += [ar.ptr("wt"), stride]
    assert _fn("tgv_stack_primal_w" if weighted else "tgv_stack_primal", dtype)(
        *args, P, *_dims(shape), *_iw(d), TAU, THETA, tab.data_ptr(), L1 if l1 else 0,
        stream_ptr()) == 0
    torch.cuda.synchronize()
    got = {k: _raw(ar.t[k]) for k in names}
    label = "primal %r P=%d l1=%d w=%d stride=%d off=%d last=%s" % (
        shape, P, l1, weighted, stride, offset, last)
    for m in range(P):
        if m == poison:
            continue
        want = _single_primal(shape, dtype, m, l1, weighted, m if strided else 0)
        for k in ("x", "xbar", "w", "wbar"):
            assert np.array_equal(_member(got[k], m, P), want[k]), (label, m, k)
    assert ar.guards_intact(), label
    if poison is None:
        for k in ("p", "q", "bt") + (("wt",) if weighted else ()):
            assert np.array_equal(got[k], _bytes_of(host[k], dtype)), (label, k)
        m = P - 1
        want = _want_primal(shape, dtype, m, l1, weighted, m if strided else 0)
        errs = [rel_l2(_as_f64(_member(got[k], m, P), dtype, v.shape), v, label + " " + k)
                for k, v in zip(("x", "xbar", "w", "wbar"), want)]
        print("%s %s: x %.3g xbar %.3g w %.3g wbar %.3g" % ((label, _suffix(dtype)) +
                                                           tuple(errs)))
        assert max(errs) <= _gate(dtype)


# ------------------------------------------------------------ 1. the stacked kernels
@pytest.mark.parametrize("dtype", BOTH)
def test_every_member_straddles_both_projections(dtype):
    for shape in STRADDLING:
        _assert_straddles(shape, dtype, 3)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_dual_stack_has_the_single_entrys_bits(nsol, shape, dtype):
    for P in (1, 2, 3):
        for iso in (False, True):
            _check_dual(shape, dtype, P, iso)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_primal_stacks_have_the_single_entries_bits(nsol, shape, dtype):
    for P in (1, 2, 3):
        for l1 in (False, True):
            for weighted in (False, True):
                for strided in (False, True):
                    _check_primal(shape, dtype, P, l1, weighted, strided)


@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (5, 4, 64)])
@pytest.mark.parametrize("dtype", BOTH)
def test_arrays_off_16_byte_alignment(nsol, shape, dtype):
    """Every base one element (three for the primal step) off alignment: the ragged
    kernels, or the element kernels for short rows, whatever the row length."""
    for P in (2, 3):
        _check_dual(shape, dtype, P, False, offset=1)
        _check_primal(shape, dtype, P, False, False, True, offset=3)
        _check_primal(shape, dtype, P, True, True, P == 2, offset=1)


@pytest.mark.parametrize("shape", [(259,), (6, 259), (4, 6, 259), (3, 5, 7), (5, 4, 64)])
@pytest.mark.parametrize("dtype", BOTH)
def test_stacks_that_end_with_their_allocation(nsol, shape, dtype):
    """Every stacked array in turn ends exactly where the device allocation ends: the last
    rows of the LAST member's last component have nothing of the array behind them."""
    for last in DUAL_ARRAYS:
        _check_dual(shape, dtype, 3, True, last=last)
    for last in ("x", "w", "wbar", "p", "q", "bt"):
        _check_primal(shape, dtype, 3, True, False, last != "w", last=last)
    for last in ("wt", "bt", "q"):
        _check_primal(shape, dtype, 2, False, True, last != "q", last=last)


@pytest.mark.parametrize("shape", [(6, 259), (3, 5, 7), (5, 4, 64)])
@pytest.mark.parametrize("dtype", BOTH)
def test_a_zero_weight_hides_a_nan_in_the_observation(nsol, shape, dtype):
    """Member 1's observation is NaN wherever its weight is 0: the member stays finite and
    keeps the single entry's bits."""
    import torch
    from nsol_amd.device import stream_ptr
    P, n, d = 3, int(np.prod(shape)), len(shape)
    names = PRIMAL_ARRAYS + ("wt",)
    for l1 in (False, True):
        host = _stacked(shape, dtype, P, names)
        hidden = host["wt"][n:2 * n] == 0
        assert 0.1 < hidden.mean() < 0.4
        host["bt"][n:2 * n][hidden] = np.nan
        ar = Arena(host, dtype)
        tab = _table(ar.buf, P)
        assert _fn("tgv_stack_primal_w", dtype)(
            *[ar.ptr(k) for k in PRIMAL_ARRAYS], n, ar.ptr("wt"), n, P, *_dims(shape),
            *_iw(d), TAU, THETA, tab.data_ptr(), L1 if l1 else 0, stream_ptr()) == 0
        torch.cuda.synchronize()
        mine = {k: _state(shape, dtype, 1)[k] for k in names}
        mine["bt"] = host["bt"][n:2 * n]
        want = _single_primal_on(shape, dtype, 1, l1, mine)
        for k in ("x", "xbar", "w", "wbar"):
            got = _raw(ar.t[k])
            assert np.all(np.isfinite(got.view(dtype))), k
            assert np.array_equal(_member(got, 1, P), want[k]), k
        assert ar.guards_intact()


# ---------------------------------------------------------------------- 2. isolation
@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (5, 4, 64)])
@pytest.mark.parametrize("dtype", BOTH)
def test_a_member_of_nans_leaves_its_neighbours_alone(nsol, shape, dtype):
    """NaN throughout member 1's state: members 0 and 2 keep the bits of their clean run
    and the guard bands their sentinels."""
    _check_dual(shape, dtype, 3, False, poison=1)
    _check_dual(shape, dtype, 3, True, poison=1, offset=1)
    _check_primal(shape, dtype, 3, False, False, True, poison=1)
    _check_primal(shape, dtype, 3, True, True, True, poison=1, offset=1)


# ------------------------------------------------------------------------ 3. declines
@pytest.mark.parametrize("dtype", BOTH)
def test_the_entries_decline(nsol, dtype):
    import torch
    from nsol_amd import ops
    from nsol_amd.device import stream_ptr, to_device
    dual, primal = _fn("tgv_stack_dual", dtype), _fn("tgv_stack_primal", dtype)
    primal_w, table = _fn("tgv_stack_primal_w", dtype), _fn("tgv_stack_table", dtype)
    shape, P = (3, 4, 6), 2
    n = 3 * 4 * 6
    mk = lambda k: to_device(np.full(k * P * n, 0.25), dtype)
    xbar, wbar, p, q = mk(1), mk(3), mk(3), mk(6)
    x, w, bt, wt = mk(1), mk(3), mk(1), mk(1)
    every = (xbar, wbar, p, q, x, w, bt, wt)
    tab = ops.tgv_stack_table(x, [2., 1.], [0.5, 0.])
    ptr = lambda t: None if t is None else t.data_ptr()
    good_d, good_p = (xbar, wbar, p, q), (p, q, x, xbar, w, wbar, bt)
    good_w = good_p + (wt,)

    def cd(a=good_d, members=P, dims=(3,) + shape, sigma=0.3, tab=tab, flags=0):
        return dual(*[ptr(t) for t in a], members, *dims, 1., 1., 1., sigma, ptr(tab),
                    flags, stream_ptr())

    def cp(a=good_p, stride=n, members=P, dims=(3,) + shape, tau=0.3, theta=1., tab=tab,
           flags=0):
        return primal(*[ptr(t) for t in a], stride, members, *dims, 1., 1., 1., tau, theta,
                      ptr(tab), flags, stream_ptr())

    def cw(a=good_w, stride=n, wstride=n, members=P, dims=(3,) + shape, tau=0.3, theta=1.,
           tab=tab, flags=0):
        return primal_w(*[ptr(t) for t in a[:7]], stride, ptr(a[7]), wstride, members,
                        *dims, 1., 1., 1., tau, theta, ptr(tab), flags, stream_ptr())

    before = ops.tgv_stack_launches(), ops.tgv_launches()
    for members in (0, 65536, -1):                       # declined, nothing launched
        assert cd(members=members) == -2 and cp(members=members) == -2
        assert cw(members=members) == -2
    for dims in ((3, 1 << 11, 1 << 11, 1 << 10), (1, 1, 1, (1 << 31) + 1)):
        assert cd(dims=dims) == -2 and cp(dims=dims) == -2 and cw(dims=dims) == -2
    for k in range(4):                                   # a missing pointer
        a = list(good_d)
        a[k] = None
        assert cd(a) == -1, k
    for k in range(8):
        a = list(good_w)
        a[k] = None
        assert cw(a) == -1, k
        if k < 7:
            assert cp(a[:7]) == -1, k
    assert cd(tab=None) == -1 and cp(tab=None) == -1 and cw(tab=None) == -1
    for i in range(4):                                   # two arguments that alias
        for j in range(i):
            a = list(good_d)
            a[i] = a[j]
            assert cd(a) == -1, (i, j)
    for i in range(8):
        for j in range(i):
            a = list(good_w)
            a[i] = a[j]
            assert cw(a) == -1, (i, j)
            if i < 7:
                assert cp(a[:7]) == -1, (i, j)
    # ... or overlap only because the spans are `members` times as long: what one member
    # leaves of an array given as the next argument
    halves = (xbar, wbar, q[:3 * n], q[3 * n:])          # p: 3 n per member, q: 6 n
    assert cd(halves) == -1
    assert cp((p, q, x[:n], x[n:], w, wbar, bt)) == -1
    # shared bt and wt are n values long: they may sit right behind one another
    shared = (p, q, x, xbar, w, wbar, bt[:n], bt[n:])
    assert cw(shared, stride=n, wstride=0) == -1
    for stride in (1, n - 1, 2 * n, -n):                 # a stride that is neither 0 nor n
        assert cp(stride=stride) == -1 and cw(stride=stride) == -1
        assert cw(wstride=stride) == -1
    for bad in (0., -0.3, np.inf, np.nan):
        assert cd(sigma=bad) == -1 and cp(tau=bad) == -1 and cw(tau=bad) == -1, bad
    assert cp(theta=np.nan) == -1 and cw(theta=np.nan) == -1
    for flags in (1, 8, 0x100, ISO | 1, L1 | 8):         # Huber, weighted, run flags
        assert cd(flags=flags) == -1 and cp(flags=flags) == -1, flags
    assert cw(flags=ISO) == -1
    for dims in ((0,) + shape, (4,) + shape, (2,) + shape, (3, -1, 4, 6)):
        assert cd(dims=dims) == -1 and cp(dims=dims) == -1 and cw(dims=dims) == -1, dims
    # an extent of 0: nothing to do, whatever else is passed
    for dims in ((3, 0, 4, 6), (3, 3, 0, 6), (1, 1, 1, 0)):
        assert cd(dims=dims) == 0 and cp(dims=dims) == 0 and cw(dims=dims) == 0
        assert cd((None,) * 4, dims=dims, tab=None) == 0
    # the table checks its values as the single entries check their scalars
    host = torch.empty(64, dtype=torch.uint8).pin_memory()
    dev = torch.zeros(64, dtype=torch.uint8, device=x.device)

    def ct(beta, tl, members=2, nbytes=64):
        b, t = np.asarray(beta, np.float64), np.asarray(tl, np.float64)
        return table(members, b.ctypes.data, t.ctypes.data, host.data_ptr(),
                     dev.data_ptr(), nbytes, stream_ptr())
    for bad in (0., -1., np.inf, np.nan):
        assert ct([2., bad], [0.5, 0.5]) == -1, bad
    for bad in (-0.1, np.nan, np.inf):
        assert ct([2., 2.], [0.5, bad]) == -1, bad
    assert ct([2., 2.], [0.5, 0.5], nbytes=8 * np.dtype(dtype).itemsize - 1) == -1
    assert ct([2., 2.], [0.5, 0.5], members=0) == -2
    assert ct([2., 2.], [0.5, 0.5], members=65536) == -2
    torch.cuda.synchronize()
    assert not dev.any()                                 # nothing was uploaded
    with pytest.raises(ValueError):
        ops.tgv_stack_table(x, [2., -1.], [0.5, 0.5])
    assert ops.tgv_stack_table(x, [], []) is None
    assert (ops.tgv_stack_launches(), ops.tgv_launches()) == before
    torch.cuda.synchronize()
    for t in every:
        assert torch.equal(t, torch.full_like(t, 0.25))
    assert cd() == 0 and cp() == 0 and cw() == 0         # and the good calls run
    assert cd(halves, members=1) == 0 and cw(shared, stride=0, wstride=0) == 0
    assert cd(flags=ISO) == 0 and cp(flags=L1) == 0 and cw(flags=L1, stride=0) == 0
    torch.cuda.synchronize()
    assert (ops.tgv_stack_launches(), ops.tgv_launches()) == (before[0] + 8, before[1])
    # the Python wrappers check their operands before the library sees them
    iw = (1., 1., 1.)
    with pytest.raises(ValueError):
        ops.tgv_stack_dual(xbar, wbar[:3 * n], p, q, P, shape, iw, 0.3, tab)
    with pytest.raises(ValueError):
        ops.tgv_stack_primal(p, q, x, xbar, w, wbar, bt[:n + 1], P, shape, iw, 0.3, tab)
    with pytest.raises(ValueError):
        ops.tgv_stack_dual(xbar, wbar, p, q, P, shape, iw, 0.3, tab[:8])
    with pytest.raises(ValueError):
        ops.tgv_stack_dual(xbar, wbar, p, q, P, shape, iw, -1., tab)
    assert ops.tgv_stack_dual(xbar, wbar, p, q, 0, shape, iw, 0.3, tab) is False


# --------------------------------------------------------------------------- 4. batch
X_SCALES = (2.0, 1.0, 3.5, 0.8, 1.7, 2.2)
ALPHAS = (0.3, 0.1, 0.7, 0.2, 0.4, 0.25)
MEMBER_BETAS = (1.7, 1.0, 2.6, 0.6, 2.0, 1.3)
ITERS = 25


def _obs(shape, seed=0):
    """A ramp with a step and noise, in [0, 2] or so."""
    rng = np.random.default_rng(7 + sum(shape) + 31 * seed)
    grids = np.meshgrid(*[np.arange(s) / float(s) for s in shape], indexing="ij")
    v = sum((k + 1) * 0.4 * g for k, g in enumerate(grids)) + 0.6 * (grids[-1] > 0.5)
    return v + 0.1 * rng.standard_normal(shape)


def _weights(shape, seed):
    rng = np.random.default_rng(900 + seed)
    return (2. * rng.random(shape) * (rng.random(shape) > 0.2)).flatten()


def _solver(nsol, shape, dtype, k, **kw):
    """Member k of a list: its own observation, alpha, beta and x_scale."""
    obs = _obs(shape, k)
    args = dict(b=obs.flatten(), x0=obs.flatten(), dimension=len(shape), shape=shape,
                spacing=SPACING[:len(shape)], alpha=ALPHAS[k], beta=MEMBER_BETAS[k],
                iterations=ITERS, x_scale=X_SCALES[k], dtype=dtype)
    args.update(kw)
    return nsol.TGVPrimalDualSolver(**args)


def _six(nsol, dtype, iso, data):
    """Four of (12, 19), one of another shape, one with a tolerance."""
    kw = dict(isotropic=iso, data_loss=data)
    return [_solver(nsol, (12, 19), dtype, k, **kw) for k in range(4)] + \
        [_solver(nsol, (19, 12), dtype, 4, **kw),
         _solver(nsol, (12, 19), dtype, 5, tolerance=1e-3, check_every=5, **kw)]


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("iso, data", [(False, "ell2"), (True, "ell1")])
def test_batch_members_are_single_solvers(nsol, dtype, iso, data):
    from nsol_amd import ops
    fresh = _six(nsol, dtype, iso, data)
    own = []
    for s in fresh:
        before = ops.tgv_launches()
        s.run()
        own.append(ops.tgv_launches() - before)
    assert own[:5] == [2 * ITERS] * 5
    solvers = _six(nsol, dtype, iso, data)
    batch = nsol.TGVPrimalDualBatch(solvers)
    before = ops.tgv_stack_launches(), ops.tgv_launches()
    batch.run()
    assert batch.get_execution() == ["stacked"] * 4 + ["sequential"] * 2
    assert ops.tgv_stack_launches() - before[0] == 2 * ITERS
    assert ops.tgv_launches() - before[1] == own[4] + own[5]
    assert batch.get_group_size() == 4
    for k, (s, f) in enumerate(zip(solvers, fresh)):
        assert np.array_equal(s.get_x(), f.get_x()), k
        assert np.array_equal(s.get_w(), f.get_w()), k
        assert s.get_iterations_done() == f.get_iterations_done()
        assert s.get_stop_reason() == f.get_stop_reason()
        assert s.get_execution() == f.get_execution() == "fused"
        assert np.abs(s.get_w()).max() > 0
    assert solvers[0].get_iterations_done() == ITERS
    assert solvers[0].get_stop_reason() == "iterations"
    X = batch.get_x_all_device().cpu().numpy()
    for k, f in enumerate(fresh):
        assert np.array_equal(X[k], f.get_x_device().cpu().numpy())
    if dtype is np.float64:
        for k in range(4):
            obs = _obs((12, 19), k)
            want = tg.iterate(obs / X_SCALES[k], obs / X_SCALES[k], ITERS, ALPHAS[k],
                              MEMBER_BETAS[k], SPACING[:2], data, iso)
            ex = rel_l2(solvers[k].get_x(), want["x"] * X_SCALES[k], "x")
            ew = rel_l2(solvers[k].get_w(), want["w"] * X_SCALES[k], "w")
            print("batch member %d iso=%d %s: x %.3g w %.3g" % (k, iso, data, ex, ew))
            assert ex <= F64_TOL and ew <= F64_TOL


@pytest.mark.parametrize("dtype", BOTH)
def test_weighted_members_stack_among_themselves(nsol, dtype):
    from nsol_amd import ops
    shape = (12, 19)
    def make():
        return [_solver(nsol, shape, dtype, k,
                        weights=_weights(shape, k) if k % 2 else None) for k in range(4)]
    fresh, solvers = make(), make()
    for f in fresh:
        f.run()
    batch = nsol.TGVPrimalDualBatch(solvers)
    before = ops.tgv_stack_launches(), ops.tgv_launches()
    batch.run()
    assert batch.get_execution() == ["stacked"] * 4 and batch.get_group_size() == 2
    assert ops.tgv_stack_launches() - before[0] == 2 * 2 * ITERS
    assert ops.tgv_launches() == before[1]
    for k, (s, f) in enumerate(zip(solvers, fresh)):
        assert np.array_equal(s.get_x(), f.get_x()), k
        assert np.array_equal(s.get_w(), f.get_w()), k
    assert not np.array_equal(solvers[1].get_x(), _solver(nsol, shape, dtype, 1).get_x())


def test_batch_of_device_tensors_with_device_mode_observers(nsol):
    from nsol_amd.device import to_device
    from nsol_amd.observer import Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    shape, dtype = (12, 19), np.float32
    truth = _obs(shape, 99).flatten()

    def make():
        out = []
        for k in range(3):
            obs = _obs(shape, k).flatten()
            s = _solver(nsol, shape, dtype, k, b=to_device(obs, np.float64),
                        x0=to_device(obs, dtype),
                        weights=to_device(_weights(shape, k), dtype))
            o = Observer(keep_iterates=False, every=10)
            o.set_measures({"RMSE": lambda x: sm.similarity_measures["RMSE"](x, truth),
                            "NCC": lambda x: sm.similarity_measures["NCC"](x, truth)})
            s.set_observer(o)
            out.append(s)
        return out
    fresh, solvers = make(), make()
    for f in fresh:
        f.run()
    batch = nsol.TGVPrimalDualBatch(solvers)
    batch.run()
    assert batch.get_execution() == ["stacked"] * 3
    for s, f in zip(solvers, fresh):
        assert np.array_equal(s.get_x(), f.get_x())
        assert np.array_equal(s.get_w(), f.get_w())
        a, b = s.get_observer(), f.get_observer()
        a.compute_measures()
        b.compute_measures()
        assert a.get_observed_iterations() == b.get_observed_iterations() == [0, 10, 20, 25]
        for name in ("RMSE", "NCC"):
            assert np.array_equal(a.get_measures()[name], b.get_measures()[name]), name
            assert np.all(np.isfinite(a.get_measures()[name]))


def test_groups_leave_the_same_bits(nsol, monkeypatch):
    from nsol_amd import ops
    shape, dtype = (12, 19), np.float32
    fresh = [_solver(nsol, shape, dtype, k) for k in range(5)]
    for f in fresh:
        f.run()
    n = 12 * 19
    per_member = (2 + 3 * 2 + 3 + 1) * n * 4            # the state and its own bt
    monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", 2 * per_member + per_member // 2)
    solvers = [_solver(nsol, shape, dtype, k) for k in range(5)]
    batch = nsol.TGVPrimalDualBatch(solvers)
    before = ops.tgv_stack_launches()
    batch.run()
    assert batch.get_group_size() == 2 and batch.get_execution() == ["stacked"] * 5
    assert ops.tgv_stack_launches() - before == 3 * 2 * ITERS       # 2 + 2 + 1
    for k, (s, f) in enumerate(zip(solvers, fresh)):
        assert np.array_equal(s.get_x(), f.get_x()), k
        assert np.array_equal(s.get_w(), f.get_w()), k


# --------------------------------------------------------------------------- 5. sweep
@pytest.mark.parametrize("dtype, weighted", [(np.float64, False), (np.float32, True)])
def test_sweep_members_are_single_solvers(nsol, dtype, weighted):
    from nsol_amd import ops
    from nsol_amd.observer import Observer, observation_points
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    shape = (3, 10, 13)
    obs, truth = _obs(shape).flatten(), _obs(shape, 99).flatten()
    measures = {k: (lambda x, k=k: sm.similarity_measures[k](x, truth))
                for k in ("PSNR", "SSD")}
    kw = dict(b=obs, x0=obs, dimension=3, shape=shape, spacing=SPACING, iterations=ITERS,
              x_scale=2.0, dtype=dtype, isotropic=True,
              weights=_weights(shape, 3) if weighted else None)
    grid = {"alpha": [0.1, 0.4], "beta": [0.8, 1.7, 3.0]}
    sweep = nsol.TGVPrimalDualSweep(parameters=grid, **kw)
    sweep.set_measures(measures, every=10)
    before = ops.tgv_stack_launches(), ops.tgv_launches()
    sweep.run()
    assert sweep.get_execution() == "stacked" and sweep.get_group_size() == 6
    assert ops.tgv_stack_launches() - before[0] == 2 * ITERS
    assert ops.tgv_launches() == before[1]
    members = [dict(alpha=a, beta=b) for a in grid["alpha"] for b in grid["beta"]]
    assert sweep.get_parameters() == members
    assert sweep.get_iterations_done() == [ITERS] * 6
    assert sweep.get_observed_iterations() == observation_points(ITERS, 10)
    got = sweep.get_measures()
    X = sweep.get_x_all_device().cpu().numpy()
    for m, member in enumerate(members):
        s = nsol.TGVPrimalDualSolver(**dict(kw, **member))
        o = Observer(keep_iterates=False, every=10)
        o.set_measures(measures)
        s.set_observer(o)
        s.run()
        o.compute_measures()
        assert np.array_equal(sweep.get_x(m), s.get_x()), member
        assert np.array_equal(sweep.get_w(m), s.get_w()), member
        assert np.array_equal(X[m], s.get_x_device().cpu().numpy())
        for name in measures:
            assert got[name].shape == (6, 4)
            assert np.array_equal(got[name][m], o.get_measures()[name]), (name, member)
    k, best = sweep.best("PSNR")
    assert k == int(np.argmax(got["PSNR"][:, -1])) and best == members[k]
    assert sweep.best("SSD", mode="min")[0] == int(np.argmin(got["SSD"][:, -1]))
    # alpha and beta both act: the members at the ends of either list differ
    last = got["PSNR"][:, -1]
    assert last[0] != last[3] and last[0] != last[2] and last[3] != last[5]


def test_sweep_with_a_tolerance_runs_sequentially(nsol):
    from nsol_amd import ops
    shape, dtype = (3, 10, 13), np.float64
    obs = _obs(shape).flatten()
    kw = dict(b=obs, x0=obs, dimension=3, shape=shape, spacing=SPACING, iterations=40,
              x_scale=2.0, dtype=dtype, tolerance=1e-3, check_every=5)
    grid = {"beta": [0.8, 3.0], "alpha": [0.1, 0.4]}
    sweep = nsol.TGVPrimalDualSweep(parameters=grid, **kw)
    before = ops.tgv_stack_launches()
    sweep.run()
    assert sweep.get_execution() == "sequential" and sweep.get_group_size() is None
    assert ops.tgv_stack_launches() == before
    members = sweep.get_parameters()
    assert members == [dict(beta=b, alpha=a) for b in grid["beta"] for a in grid["alpha"]]
    done = sweep.get_iterations_done()
    for m, member in enumerate(members):
        s = nsol.TGVPrimalDualSolver(**dict(kw, **member))
        s.run()
        assert np.array_equal(sweep.get_x(m), s.get_x()), member
        assert np.array_equal(sweep.get_w(m), s.get_w()), member
        assert done[m] == s.get_iterations_done()
