"""The observation kernels of csrc/nsol_observe.hip -- k_observe, k_observe_final and
k_observe_widen, the sums behind PSNR, NCC, SSD, TV, Huber, TK0 and TK1 of an observed
run -- called on their own beside a float64 reference (observe_cases.py, anchored on the
oracle by test_observe_kernels_host.py).

Through the C ABI on arrays in a guard-band arena (device_arena.py): 1-D, 2-D and 3-D
volumes with extents of 1, with two workgroups so that every thread takes several voxels
and the division-free advance of (ix, iy, iz) carries and wraps, contiguous and pitched
rows with the sentinel in the gaps, every flag set, the reference in the element type
and in float64, scales that float32 rounds, both Huber branches, the flat path's second
unrolled step, the 64-bit coordinates once, and every argument the entry refuses.  The
gates are derived in observe_cases.py, per sum.
"""
import itertools

import numpy as np
import pytest

import observe_cases as oc
import vector_cases as vc
from device_arena import Arena, SENTINEL

pytestmark = pytest.mark.gpu

BOTH = [np.float64, np.float32]
FILL = -7.5                         # what the row and the widened output hold before a call
DEFAULT_GRID = 2048                 # max_grid_blocks as the library is built
ALL = oc.PAIR | oc.GRAD | oc.SQ | oc.HUBER
WORST = {}                          # sum -> (largest |got - want| / gate, where)


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    yield nsol_amd
    for k in sorted(WORST):
        print("k_observe %-18s largest |got - want| / gate = %.3g  (%s)"
              % ((oc.NAMES[k],) + WORST[k]))


@pytest.fixture(scope="module")
def ws(nsol):
    import torch
    from nsol_amd import _lib
    return torch.empty(_lib.load().nsol_hip_reduce_ws_doubles(), dtype=torch.float64,
                       device="cuda")


def _suffix(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _fn(name, dtype):
    from nsol_amd import _lib
    return getattr(_lib.load(), "nsol_%s_%s" % (name, _suffix(dtype)))


def _sync():
    import torch
    torch.cuda.synchronize()


def _stream():
    from nsol_amd.device import stream_ptr
    return stream_ptr()


def _two_workgroups(fn):
    """Runs fn with max_grid_blocks = 2 (a stride of 512 voxels) and puts the knob back."""
    from nsol_amd import _lib
    _lib.set_param("max_grid_blocks", 2)
    try:
        fn()
    finally:
        _lib.reset_params()


# ====================================================================== 1. k_observe
def _check_observe(ws, x, dtype, shape, flags, x_scale=1.0, y=None, y_f64=False, ybar=0.0,
                   w=(1., 1., 1.), gamma=0.5, pitch=0, offset=0, grid=DEFAULT_GRID):
    """One call of nsol_observe_* on x (float64 values of dtype, contiguous) laid out at
    `pitch`, against observe_sums_ref; the row in a float64 arena of its own."""
    ndim, nz, ny, nx = oc.dims3(shape)
    n = nz * ny * nx
    xlay = oc.pitched(x, shape, pitch, SENTINEL) if pitch else np.asarray(x).reshape(-1)
    pair = bool(flags & oc.PAIR)
    here = dict(x=xlay)
    if pair and not y_f64:
        here["y"] = y
    ax = Arena(here, dtype, offset)
    ay = Arena(dict(y=y), np.float64, offset) if pair and y_f64 else None
    ar = Arena(dict(row=np.full(oc.SUMS, FILL)), np.float64, offset)
    yp = (ay if y_f64 else ax).ptr("y") if pair else None
    rc = _fn("observe", dtype)(ax.ptr("x"), x_scale, yp, int(y_f64), ybar, ndim, nz, ny, nx,
                               pitch, w[0], w[1], w[2], gamma, flags, ar.ptr("row"),
                               ws.data_ptr(), _stream())
    label = "%r %s flags=%d scale=%g y=%s ybar=%g w=%r pitch=%d off=%d grid=%d" % (
        shape, _suffix(dtype), flags, x_scale, "f64" if y_f64 else "T", ybar, w, pitch,
        offset, grid)
    assert rc == 0, label
    _sync()
    got = ar.get("row", (oc.SUMS,))
    want, terms = oc.observe_sums_ref(x, x_scale, y, ybar, shape, w, gamma, flags, ndim,
                                      dtype)
    n_trips = oc.obs_trips(n, grid)
    for k in range(oc.SUMS):
        if terms[k] is None:                             # not asked for: exactly +0.0
            assert got[k] == 0.0 and not np.signbit(got[k]), (label, k, got[k])
            continue
        bound = oc.gate(k, terms[k], n_trips, ndim)
        err = abs(got[k] - want[k])
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
        if ratio > WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (ratio, label)
        assert err <= bound, "%s: %s got %.17g want %.17g err %.3g gate %.3g" % (
            label, oc.NAMES[k], got[k], want[k], err, bound)
    assert ar.guards_intact() and ax.guards_intact(), label      # nine doubles, no more
    assert np.array_equal(ax.get("x", xlay.shape), xlay), label
    if pair:
        assert np.array_equal((ay if y_f64 else ax).get("y", (n,)), y.reshape(-1)), label
        assert ay is None or ay.guards_intact(), label
    return got


def _combos():
    """Every combination of flag set, pitch kind, scale, spacing, reference type, ybar
    and alignment, in a fixed shuffled order: each (shape, type) case takes the next 48,
    so that all 1152 run somewhere and every case meets every value of every factor."""
    every = list(itertools.product(oc.FLAG_SETS, range(4), oc.SCALES, oc.SPACINGS,
                                   (False, True), (False, True), (0, 1)))
    order = np.random.default_rng(2024).permutation(len(every))
    return [every[i] for i in order]


COMBOS = _combos()
PER_CASE = 48
assert PER_CASE * len(oc.SHAPES) * 2 >= len(COMBOS)


def _case_combos(shape, dtype):
    i = (2 * oc.SHAPES.index(shape) + int(np.dtype(dtype) == np.float32)) * PER_CASE
    picked = [COMBOS[(i + j) % len(COMBOS)] for j in range(PER_CASE)]
    # and every case: all sums at once on every pitch
    picked += [(ALL, p, 37.5, oc.SPACINGS[1], p % 2 == 1, True, p % 2) for p in range(4)]
    return picked


@pytest.mark.parametrize("shape", oc.SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_observe_sums_with_two_workgroups_walking_the_coordinates(nsol, ws, shape, dtype):
    """A stride of 512 voxels: a thread takes up to 13 voxels and (ix, iy, iz) advance by
    a stride that is no multiple of nx (7, 259, 13) or is one (64), carrying into iy and
    wrapping into iz."""
    ndim, nx = len(shape), shape[-1]
    x = oc.smooth_field(shape, dtype)

    def run():
        for flags, pk, scale, spacing, y_f64, ybar0, offset in _case_combos(shape, dtype):
            w = oc.weights(spacing)
            y = oc.reference_for(x, scale, np.float64 if y_f64 else dtype)
            ybar = 0.0 if ybar0 else float(np.mean(y)) + 0.01
            gamma = oc.median_gamma(x, scale, shape, w, ndim, dtype)
            pitch = 0 if pk == 0 else oc.pitches(nx, dtype)[pk - 1]
            _check_observe(ws, x, dtype, shape, flags, scale, y, y_f64, ybar, w, gamma,
                           pitch, offset, grid=2)
    _two_workgroups(run)


@pytest.mark.parametrize("dtype", BOTH)
def test_observe_sums_with_the_grid_the_library_launches(nsol, ws, dtype):
    for i, shape in enumerate(oc.SHAPES):
        x = oc.smooth_field(shape, dtype)
        w = oc.weights(oc.SPACINGS[i % 2])
        scale = oc.SCALES[i % 3]
        y = oc.reference_for(x, scale, np.float64 if i % 2 else dtype)
        gamma = oc.median_gamma(x, scale, shape, w, len(shape), dtype)
        for flags in oc.FLAG_SETS:
            for pitch in (0,) + oc.pitches(shape[-1], dtype):
                _check_observe(ws, x, dtype, shape, flags, scale, y, bool(i % 2), 0.3, w,
                               gamma, pitch, offset=(i + pitch) % 2)


@pytest.mark.parametrize("dtype", BOTH)
def test_huber_term_on_both_branches_on_the_corner_and_on_zero(nsol, ws, dtype):
    """The planted field of observe_cases.huber_field (its shares are asserted on the CPU
    by test_observe_kernels_host.py): a swapped or one-sided branch moves sum 6 by far
    more than its gate."""
    shapes = [s for s in oc.SHAPES if int(np.prod(s)) >= 35]
    for shape in shapes:
        x = oc.huber_field(shape)
        sh = oc.huber_shares(x, shape)
        assert sh["below"] >= 0.2 and sh["above"] >= 0.2 and sh["on"] and sh["zero"]
        for flags in (oc.GRAD | oc.HUBER, ALL):
            y = oc.reference_for(x, 1.0, dtype)
            for pitch, offset in ((0, 0), (shape[-1] + 1, 1)):
                _check_observe(ws, x, dtype, shape, flags, 1.0, y, False, 0.25,
                               gamma=oc.HUBER_GAMMA, pitch=pitch, offset=offset)
                _two_workgroups(lambda: _check_observe(
                    ws, x, dtype, shape, flags, 1.0, y, False, 0.25, gamma=oc.HUBER_GAMMA,
                    pitch=pitch, offset=offset, grid=2))


@pytest.mark.parametrize("dtype", BOTH)
def test_signed_sums_under_cancellation(nsol, ws, dtype):
    """sum c and sum (c - ybar)(y - ybar) next to nothing against their terms: the gate
    is on sum |term|."""
    for shape in [(1031,), (6, 259), (7, 10, 13)]:
        for ybar in (0.0, 1024.0):
            for y_f64 in (False, True):
                x, y = oc.cancelling_field(shape, dtype, ybar)
                _check_observe(ws, x, dtype, shape, oc.PAIR, 1.0, y, y_f64, ybar)
                _two_workgroups(lambda: _check_observe(
                    ws, x, dtype, shape, oc.PAIR | oc.SQ, 1.0, y, y_f64, ybar,
                    pitch=shape[-1] + 3, grid=2))


@pytest.mark.parametrize("dtype", BOTH)
def test_the_flat_path_takes_a_second_unrolled_step(nsol, ws, dtype):
    """2048 * 256 * 4 + 5 voxels without coordinates: one full step of four strides, then
    five threads start a second one."""
    n = 2048 * 256 * 4 + 5
    x = oc.smooth_field((n,), dtype)
    y_f64 = np.dtype(dtype) == np.float32
    y = oc.reference_for(x, 37.5, np.float64 if y_f64 else dtype)
    _check_observe(ws, x, dtype, (n,), oc.PAIR | oc.SQ, 37.5, y, y_f64, 0.5,
                   offset=int(y_f64))


@pytest.mark.parametrize("dtype", BOTH)
def test_a_default_stride_that_is_no_multiple_of_the_row(nsol, ws, dtype):
    """(33, 127, 131): the stride of 524 288 voxels is no multiple of 131, so the second
    voxel of a thread is reached through a carry (contiguous and pitched)."""
    shape = (33, 127, 131)
    x = oc.smooth_field(shape, dtype)
    w = oc.weights(oc.SPACINGS[1])
    y = oc.reference_for(x, 0.1, dtype)
    gamma = oc.median_gamma(x, 0.1, shape, w, 3, dtype)
    _check_observe(ws, x, dtype, shape, ALL, 0.1, y, False, 0.02, w, gamma)
    _check_observe(ws, x, dtype, shape, oc.GRAD, 0.1, None, False, 0.0, w, gamma,
                   pitch=132, offset=1)


class _Row(object):
    """Nine doubles for the sums between sentinels, in a tensor of their own."""

    def __init__(self, k=oc.SUMS):
        import torch
        self.k = k
        self.t = torch.full((k + 16,), FILL, dtype=torch.float64, device="cuda")

    def ptr(self):
        return self.t[8:].data_ptr()

    def get(self):
        h = self.t.cpu().numpy()
        assert np.all(h[:8] == FILL) and np.all(h[8 + self.k:] == FILL)
        return h[8:8 + self.k].copy()


def test_the_64_bit_coordinates_on_a_line_beyond_2_30_voxels(nsol, ws):
    """nx = 2^30 + 5 with the gradient: the one case in which k_observe<float, float,
    int64_t, true> runs.  x and y repeat a period of 1000, so the sums follow in closed
    form (observe_cases.periodic_sums, checked on the CPU against a line summed term by
    term)."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory, %.1f GiB are free"
                    % (free / 2.0 ** 30))
    n, p = (1 << 30) + 5, 1000
    rng = np.random.default_rng(31)
    px = vc.rounded(0.4 + rng.standard_normal(p), np.float32)
    py = vc.rounded(15.0 + 33.0 * rng.standard_normal(p), np.float32)
    x_scale, ybar, wx = 37.5, 14.75, 1.0 / 1.3
    dev = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    reps = n // p
    x = dev(px).repeat(reps + 1)[:n]
    y = dev(py).repeat(reps + 1)[:n]
    assert x.numel() == n and x.is_contiguous() and y.is_contiguous()
    row = _Row()
    flags = oc.PAIR | oc.GRAD | oc.SQ
    rc = _fn("observe", np.float32)(x.data_ptr(), x_scale, y.data_ptr(), 0, ybar, 1, 1, 1,
                                    n, 0, wx, 1., 1., 1.0, flags, row.ptr(), ws.data_ptr(),
                                    _stream())
    assert rc == 0
    _sync()
    got = row.get()
    want, mags = oc.periodic_sums(px, py, n, x_scale, ybar, wx, np.float32)
    n_trips = oc.obs_trips(n)
    for k in range(oc.SUMS):
        if not (flags & oc.GROUP[k]) == oc.GROUP[k]:
            assert got[k] == 0.0, k
            continue
        # the gate of observe_cases.gate on the closed form's sum of magnitudes
        bound = (n_trips + 32 + oc.term_ops(k, 1)) * vc.U64 * mags[k]
        err = abs(got[k] - want[k])
        print("2^30 + 5 voxels, %s: got %.17g want %.17g err %.3g gate %.3g"
              % (oc.NAMES[k], got[k], want[k], err, bound))
        assert err <= bound, k
    tail = np.arange(n - 5, n) % p                       # the inputs are as they were
    assert np.array_equal(x[-5:].cpu().numpy(), px[tail].astype(np.float32))
    assert np.array_equal(y[-5:].cpu().numpy(), py[tail].astype(np.float32))
    del x, y
    torch.cuda.empty_cache()


def test_observe_declines(nsol, ws):
    """ValueError from ops.observe, NSOL_EINVAL (-1) from the entry, and the row left as
    it was; then the same arguments made good run."""
    import torch
    from nsol_amd import ops
    shape, dtype = (3, 5, 7), np.float32
    n = 105
    x = oc.smooth_field(shape, dtype)
    y = oc.reference_for(x, 1.0, dtype)
    ax = Arena(dict(x=x, y=y, xp=oc.pitched(x, shape, 8, SENTINEL)), dtype)
    ar = Arena(dict(row=np.full(oc.SUMS, FILL), short=np.full(8, FILL)), np.float64)
    xt, yt, row = ax.t["x"], ax.t["y"], ar.t["row"]

    def entry(flags, yp=ax.ptr("y"), gamma=0.5, pitch=0, xp=ax.ptr("x"), rowp=ar.ptr("row"),
              wsp=ws.data_ptr(), dims=(3, 3, 5, 7)):
        return _fn("observe", dtype)(xp, 1.0, yp, 0, 0.0, *dims, pitch, 1., 1., 1., gamma,
                                     flags, rowp, wsp, _stream())

    assert entry(16) == -1 and entry(ALL | 32) == -1 and entry(-1) == -1   # unknown bits
    assert entry(oc.PAIR, yp=None) == -1
    for gamma in (0.0, -0.5, float("nan")):
        assert entry(oc.GRAD, gamma=gamma) == -1
        assert entry(oc.GRAD | oc.HUBER, gamma=gamma) == -1
    assert entry(oc.SQ, pitch=6, xp=ax.ptr("xp")) == -1                    # pitch < nx
    assert entry(oc.SQ, xp=None) == -1 and entry(oc.SQ, rowp=None) == -1
    assert entry(oc.SQ, wsp=None) == -1
    for dims in ((0, 3, 5, 7), (4, 3, 5, 7), (2, 3, 5, 7), (1, 1, 5, 7), (3, 0, 5, 7),
                 (3, 3, 0, 7), (3, 3, 5, 0)):
        assert entry(oc.SQ, dims=dims) == -1, dims

    with pytest.raises(ValueError):
        ops.observe(xt, 1.0, row, shape, flags=16)
    with pytest.raises(ValueError):
        ops.observe(xt, 1.0, row, shape, flags=oc.GRAD, gamma=0.0)
    with pytest.raises(ValueError):
        ops.observe(ax.t["xp"], 1.0, row, shape, flags=oc.SQ, pitch=6)
    with pytest.raises(ValueError):
        ops.observe(xt, 1.0, row, shape, flags=oc.SQ, pitch=8)   # x holds pitch 7 only
    with pytest.raises(ValueError):
        ops.observe(xt, 1.0, ar.t["short"], shape, flags=oc.SQ)  # a row of 8
    with pytest.raises(ValueError):
        ops.observe(xt, 1.0, row.to(torch.float32), shape, flags=oc.SQ)
    with pytest.raises(ValueError):
        ops.observe(xt, 1.0, row, shape, y=yt[:n - 1], flags=oc.PAIR)
    with pytest.raises(ValueError):
        ops.observe(xt, 1.0, row, shape, y=yt.to(torch.float16), flags=oc.PAIR)
    with pytest.raises((ValueError, TypeError)):                  # no y at all
        ops.observe(xt, 1.0, row, shape, flags=oc.PAIR)
    _sync()
    assert np.all(ar.get("row", (oc.SUMS,)) == FILL) and np.all(ar.get("short", (8,)) == FILL)
    assert ar.guards_intact() and ax.guards_intact()

    # ... and the good calls run, the wrapper handing its arguments on in order
    w = oc.weights(oc.SPACINGS[1])
    for pitch, xk in ((0, "x"), (8, "xp")):
        ar.t["row"].fill_(FILL)
        assert ops.observe(ax.t[xk], 0.1, row, shape, y=yt, ybar=0.3, w=w, gamma=0.4,
                           flags=ALL, pitch=pitch) is row
        _sync()
        want, terms = oc.observe_sums_ref(x, 0.1, y, 0.3, shape, w, 0.4, ALL, 3, dtype)
        got = ar.get("row", (oc.SUMS,))
        for k in range(oc.SUMS):
            assert abs(got[k] - want[k]) <= oc.gate(k, terms[k], oc.obs_trips(n), 3), k
    assert ar.guards_intact() and ax.guards_intact()


# ================================================================ 2. k_observe_widen
def _check_widen(x, dtype, shape, x_scale, pitch=0, offset=0, through_ops=False):
    _, nz, ny, nx = oc.dims3(shape)
    n = nz * ny * nx
    xlay = oc.pitched(x, shape, pitch, SENTINEL) if pitch else np.asarray(x).reshape(-1)
    ax = Arena(dict(x=xlay), dtype, offset)
    ao = Arena(dict(out=np.full(n, FILL)), np.float64, offset)
    if through_ops:
        from nsol_amd import ops
        assert ops.observe_widen(ax.t["x"], x_scale, shape, pitch, out=ao.t["out"]) is \
            ao.t["out"]
    else:
        assert _fn("observe_widen", dtype)(ao.ptr("out"), ax.ptr("x"), x_scale, nz, ny, nx,
                                           pitch, _stream()) == 0
    _sync()
    label = "widen %r %s scale=%g pitch=%d off=%d" % (shape, _suffix(dtype), x_scale, pitch,
                                                      offset)
    want = oc.widen(x, x_scale, dtype).reshape(-1)
    got = ao.get("out", (n,))
    assert np.array_equal(got, want), "%s: %d of %d differ" % (label, np.sum(got != want), n)
    assert ao.guards_intact() and ax.guards_intact(), label
    assert np.array_equal(ax.get("x", xlay.shape), xlay), label


@pytest.mark.parametrize("dtype", BOTH)
def test_widen_is_the_scaled_iterate_bit_for_bit(nsol, dtype):
    """out[j] == float64(T(x) * T(s)) for every shape, contiguous and on all three
    pitches, with one trip per thread and, on two workgroups, with several."""
    def run(through_ops):
        for i, shape in enumerate(oc.SHAPES):
            x = oc.smooth_field(shape, dtype)
            for j, pitch in enumerate((0,) + oc.pitches(shape[-1], dtype)):
                for scale in (1.0, 0.1):
                    _check_widen(x, dtype, shape, scale, pitch, (i + j) % 2, through_ops)
    run(False)
    _two_workgroups(lambda: run(True))
    n = 2048 * 256 + 5                                   # the default grid cap crossed
    _check_widen(oc.smooth_field((n,), dtype), dtype, (n,), 0.1, offset=1)
    _check_widen(oc.smooth_field((2, n // 2), dtype), dtype, (2, n // 2), 0.1,
                 pitch=n // 2 + 3)


def test_widen_declines(nsol):
    from nsol_amd import ops
    dtype, shape = np.float32, (3, 5, 7)
    x = oc.smooth_field(shape, dtype)
    ax = Arena(dict(x=x), dtype)
    ao = Arena(dict(out=np.full(105, FILL)), np.float64)
    fn = _fn("observe_widen", dtype)
    s = _stream()
    assert fn(None, ax.ptr("x"), 1.0, 3, 5, 7, 0, s) == -1
    assert fn(ao.ptr("out"), None, 1.0, 3, 5, 7, 0, s) == -1
    assert fn(ao.ptr("out"), ax.ptr("x"), 1.0, 3, 5, 7, 6, s) == -1       # pitch < nx
    for dims in ((0, 5, 7), (3, 0, 7), (3, 5, 0), (3, -5, 7)):
        assert fn(ao.ptr("out"), ax.ptr("x"), 1.0, *dims, 0, s) == -1, dims
    with pytest.raises(ValueError):
        ops.observe_widen(ax.t["x"], 1.0, shape, pitch=6)
    with pytest.raises(ValueError):
        ops.observe_widen(ax.t["x"], 1.0, shape, pitch=8)
    with pytest.raises(ValueError):
        ops.observe_widen(ax.t["x"], 1.0, shape, out=ao.t["out"][:104])
    _sync()
    assert np.all(ao.get("out", (105,)) == FILL)
    assert ao.guards_intact() and ax.guards_intact()
