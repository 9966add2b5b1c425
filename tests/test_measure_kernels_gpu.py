"""The kernels of csrc/nsol_measures.hip at their edges: SSIM in every window it is built
for (3, 5, 7, 9, 11; line, 2-D and 3-D; both element types) with the output extent on
and one past a tile seam (16 x 16 windows) and a z-chunk seam (64 planes), the item loop's
second trip, explicit data_range and the population covariance; the histograms across
the LDS limit of 16384 bins and in the global-memory form, with several trips of the
grid-stride loop and runs of equal values that start inside a wave; the range pass with
its extremes and non-finite values in every workgroup.

SSIM against the restatement of test_measures_host.py (checked there against one window
at a time for every window size) at the SSIM_TOL of test_measures_gpu.py; histograms and
ranges equal to NumPy's.  Arrays live in a guard-band arena (device_arena.py), on and
off 16-byte alignment.
"""
import itertools

import numpy as np
import pytest

from device_arena import Arena
from test_measures_gpu import SSIM_TOL
from test_measures_host import ssim_brute, ssim_direct_1d, ssim_restated

pytestmark = pytest.mark.gpu

BOTH = [np.float64, np.float32]
WINDOWS = [3, 5, 7, 9, 11]
BRUTE_AT_MOST = 20000               # elements up to which every window is also summed alone
K_SSIM_MAX_PARTS = 8192             # kSsimMaxParts
K_LDS_BINS = 16384                  # kLdsBins


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


@pytest.fixture(scope="module")
def sm(nsol):
    from nsol_amd.similarity_measures import SimilarityMeasures
    return SimilarityMeasures


def _f32(a):
    """Values of float32 held in float64: the same numbers for both element types."""
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _pair(shape, seed):
    """uniform(-1, 1) and 0.6 x + 0.4 noise, the conditioning SSIM_TOL was set for."""
    rng = np.random.default_rng(seed)
    x = _f32(rng.uniform(-1, 1, shape))
    y = _f32(0.6 * x + 0.4 * rng.uniform(-1, 1, shape))
    return x, y


def _count(shape, win):
    return int(np.prod([s - win + 1 for s in shape]))


# ============================================================================ 1. SSIM
def _ssim_shapes(win, ndim):
    xy = (win, win + 15, win + 16)                       # 1, 16 and 17 windows
    if ndim == 1:
        return [(win,), (win + 1023,), (win + 1024,), (5000,)]   # 1, 1024, 1025 windows
    if ndim == 2:
        return list(itertools.product(xy, xy))
    return list(itertools.product((win, win + 63, win + 64), xy, xy))   # 1, 64, 65 planes


def _check_ssim(sm, x, y, win, dtype, offset, label, sample_cov=True, data_range=2.0,
                through_measure=True):
    from nsol_amd import ops
    from nsol_amd.similarity_measures import ssim_params
    shape = x.shape
    want = (ssim_direct_1d if x.ndim == 1 else ssim_restated)(
        x, y, win, data_range, sample_cov=sample_cov)
    _, C1, C2, cov_norm, count = ssim_params(shape, shape, np.float64, win_size=win,
                                             data_range=data_range)
    assert count == _count(shape, win)
    if not sample_cov:
        cov_norm = 1.0
    ar = Arena(dict(x=x, y=y), dtype, offset)
    got = ops.ssim_sum(ar.t["x"], ar.t["y"], shape, win, C1, C2, cov_norm) / count
    assert abs(got - want) <= SSIM_TOL, (label, got, want, got - want)
    assert ar.guards_intact(), label
    assert np.array_equal(ar.get("x", shape), x) and np.array_equal(ar.get("y", shape), y)
    if x.size <= BRUTE_AT_MOST:
        brute = ssim_brute(x, y, win, data_range, sample_cov=sample_cov)
        assert abs(got - brute) <= SSIM_TOL, (label, "brute", got, brute)
    if through_measure and sample_cov:
        kw = {} if data_range == 2.0 else dict(data_range=data_range)
        m = sm.structural_similarity(x.astype(dtype), y.astype(dtype), win_size=win, **kw)
        assert m == got, (label, m, got)                 # the same kernel, the same bits
    return got


@pytest.mark.parametrize("ndim", [1, 2, 3])
@pytest.mark.parametrize("win", WINDOWS)
def test_ssim_every_window_on_and_past_the_tile_and_chunk_seams(sm, win, ndim):
    """1, 16 and 17 windows along x and y (one tile, a full tile, a tile and a column),
    1, 64 and 65 output planes (one z-march, a full one, a second of one plane); the line
    form with 1, 1024 and 1025 outputs.  Both element types on the same float32 values:
    everything after the load is float64, so the two must agree bit for bit."""
    for i, shape in enumerate(_ssim_shapes(win, ndim)):
        x, y = _pair(shape, 1000 * win + 10 * ndim + i)
        got = [_check_ssim(sm, x, y, win, dtype, (i + j) % 2,
                           "W=%d %r %s" % (win, shape, np.dtype(dtype).name))
               for j, dtype in enumerate(BOTH)]
        assert got[0] == got[1], (win, shape, got)


@pytest.mark.parametrize("case", ["line", "tiles", "planes"])
def test_ssim_item_loop_takes_a_second_trip(sm, case):
    """More work items than kSsimMaxParts workgroups, float32: 8193 chunks of a line,
    91 x 91 = 8281 tiles, and 8281 tiles of a 3-D volume of one output plane, where the
    ring of plane sums must start afresh with every item."""
    shape, win = {"line": ((K_SSIM_MAX_PARTS * 1024 + 7,), 7),
                  "tiles": ((1462, 1462), 7),
                  "planes": ((3, 1458, 1458), 3)}[case]
    items = {"line": -(-(shape[0] - win + 1) // 1024),
             "tiles": (-(-(1462 - 6) // 16)) ** 2,
             "planes": (-(-(1458 - 2) // 16)) ** 2}[case]
    assert K_SSIM_MAX_PARTS < items <= 2 * K_SSIM_MAX_PARTS
    x, y = _pair(shape, 77 + len(shape))
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    got = sm.structural_similarity(x32, y32, win_size=win)
    want = (ssim_direct_1d if len(shape) == 1 else ssim_restated)(x, y, win)
    assert abs(got - want) <= SSIM_TOL, (case, got, want, got - want)
    assert sm.structural_similarity(x32, y32, win_size=win) == got   # and repeatable


@pytest.mark.parametrize("dtype", BOTH)
def test_ssim_explicit_data_range_and_population_covariance(sm, dtype):
    rng = np.random.default_rng(255)
    for win, shape in ((7, (40, 23)), (3, (19,)), (5, (9, 21, 20)), (11, (27, 26)),
                       (9, (1033,))):
        u8 = rng.integers(0, 256, shape).astype(np.uint8)
        v8 = np.clip(u8 + 12.0 * rng.standard_normal(shape), 0, 255).astype(np.uint8)
        x, y = u8.astype(np.float64), v8.astype(np.float64)
        label = "u8 values W=%d %r" % (win, shape)
        # uint8-valued data in a float type: the default range would be 2
        a = _check_ssim(sm, x, y, win, dtype, 1, label, data_range=255.0)
        b = _check_ssim(sm, x, y, win, dtype, 0, label + " default range")
        assert abs(a - b) > 1e-6
        # ... and uint8 itself, whose default is 255: the same bits either way
        assert sm.structural_similarity(u8, v8, win_size=win, data_range=255) == a
        assert sm.structural_similarity(u8, v8, win_size=win) == a
        # use_sample_covariance=False of the published algorithm: cov_norm = 1
        c = _check_ssim(sm, x, y, win, dtype, 0, label + " population", sample_cov=False,
                        data_range=255.0)
        assert abs(a - c) > 1e-9
        xf, yf = _pair(shape, win)
        _check_ssim(sm, xf, yf, win, dtype, 1, "population W=%d %r" % (win, shape),
                    sample_cov=False)


def test_ssim_declines(sm):
    import torch
    from nsol_amd import ops
    x, y = _pair((12, 14), 3)
    for win in (4, 6, 12):                               # even
        with pytest.raises(ValueError):
            sm.structural_similarity(x, y, win_size=win)
    for win in (13, 1):                                  # odd, but not built
        with pytest.raises((ValueError, NotImplementedError)):
            sm.structural_similarity(np.zeros((13, 14)), np.ones((13, 14)), win_size=win)
    for shape, win in (((12, 8), 9), ((8, 12), 9), ((10,), 11), ((7, 7, 6), 7),
                       ((6, 7, 7), 7), ((2, 9), 3)):      # an extent below the window
        with pytest.raises(ValueError):
            sm.structural_similarity(np.zeros(shape), np.zeros(shape), win_size=win)
    # the entry itself: NSOL_EINVAL, and the result left alone
    ar = Arena(dict(x=x, y=y), np.float32)
    out = torch.full((1,), -7.5, dtype=torch.float64, device="cuda")
    for shape, win in (((12, 14), 4), ((12, 14), 13), ((12, 14), 1), ((12, 14), 0),
                       ((14, 12), 13), ((2, 84), 3), ((84, 2), 3), ((168,), 13),
                       ((2, 7, 12), 3), ((7, 2, 12), 3), ((7, 12, 2), 3)):
        with pytest.raises(ValueError):
            ops.ssim_sum(ar.t["x"], ar.t["y"], shape, win, 1e-4, 9e-4, 1.0, out=out)
    with pytest.raises(ValueError):                      # a line shorter than its window
        ops.ssim_sum(ar.t["x"][:10], ar.t["y"][:10], (10,), 11, 1e-4, 9e-4, 1.0, out=out)
    with pytest.raises(ValueError):                      # a shape of another size
        ops.ssim_sum(ar.t["x"], ar.t["y"], (12, 13), 7, 1e-4, 9e-4, 1.0, out=out)
    torch.cuda.synchronize()
    assert out.item() == -7.5 and ar.guards_intact()
    assert ops.ssim_sum(ar.t["x"], ar.t["y"], (12, 14), 11, 1e-4, 9e-4, 1.0, out=out) is out
    torch.cuda.synchronize()
    assert out.item() != -7.5


# ====================================================================== 2. histograms
N_TRIPS = 2048 * 256 * 2 + 37       # the grid cap of 2048: two trips and part of a third


def _check_hist1d(x, dtype, bins, offset=0):
    from nsol_amd import ops
    x = np.asarray(x, dtype)
    ar = Arena(dict(x=x), dtype, offset)
    got, edges = ops.histogram1d(ar.t["x"], bins)
    want, wedges = np.histogram(x, bins)
    label = "hist1d n=%d %s bins=%d off=%d" % (x.size, np.dtype(dtype).name, bins, offset)
    assert edges.dtype == wedges.dtype and edges.tobytes() == wedges.tobytes(), label
    assert got.dtype == np.int64 and np.array_equal(got, want), (
        label, int(np.sum(got != want)), int(got.sum()), x.size)
    assert ar.guards_intact() and np.array_equal(ar.get("x", x.shape), x), label


def _check_hist2d(x, y, dtype, bins, offset=0):
    from nsol_amd import ops
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    ar = Arena(dict(x=x, y=y), dtype, offset)
    got, ex, ey, hx, hy = ops.histogram2d(ar.t["x"], ar.t["y"], bins, marginals=True)
    want, wx, wy = np.histogram2d(x, y, bins)
    label = "hist2d n=%d %s bins=%r off=%d" % (x.size, np.dtype(dtype).name, bins, offset)
    assert ex.tobytes() == wx.tobytes() and ey.tobytes() == wy.tobytes(), label
    assert np.array_equal(got, want.astype(np.int64)), (label, int(np.sum(got != want)))
    bx, by = (bins, bins) if np.ndim(bins) == 0 else bins
    assert np.array_equal(hx, np.histogram(x, bx)[0]), label
    assert np.array_equal(hy, np.histogram(y, by)[0]), label
    assert ar.guards_intact(), label
    assert np.array_equal(ar.get("x", x.shape), x) and np.array_equal(ar.get("y", y.shape), y)


@pytest.mark.parametrize("bins", [K_LDS_BINS, K_LDS_BINS + 1, 20000])
@pytest.mark.parametrize("dtype", BOTH)
def test_hist1d_across_the_lds_limit_with_several_trips(nsol, dtype, bins):
    """16384 bins: the last grid that counts in LDS; 16385 and 20000: straight into global
    memory, the form no other test runs in 1-D.  2048 * 256 * 2 + 37 values: every
    thread makes two trips, 37 a third."""
    rng = np.random.default_rng(bins)
    _check_hist1d(rng.standard_normal(N_TRIPS), dtype, bins, offset=bins % 2)


@pytest.mark.parametrize("bins", [(128, 128), (128, 129), (129, 128)])
@pytest.mark.parametrize("dtype", BOTH)
def test_hist2d_across_the_lds_limit_with_several_trips(nsol, dtype, bins):
    rng = np.random.default_rng(sum(bins))
    x = rng.standard_normal(N_TRIPS)
    _check_hist2d(x, 0.5 * x + rng.uniform(-1, 1, N_TRIPS), dtype, bins, offset=bins[1] % 2)


@pytest.mark.parametrize("dtype", BOTH)
def test_hist_lengths_of_one_value_and_one_past_whole_waves(nsol, dtype):
    rng = np.random.default_rng(64)
    for n in (1, 2, 65, 64 * 4 + 1, 64 * 37 + 1):
        x, y = rng.standard_normal(n), rng.uniform(0, 3, n)
        for bins in (1, 100, K_LDS_BINS + 1):
            _check_hist1d(x, dtype, bins, offset=n % 2)
        for bins in (100, (7, 3), (128, 129)):
            _check_hist2d(x, y, dtype, bins, offset=n % 2)


@pytest.mark.parametrize("dtype", BOTH)
def test_hist_runs_of_equal_values_that_start_inside_a_wave(nsol, dtype):
    """count_bin adds a wave's lanes at once when they share a bin.  Runs of 64 equal
    values from lane 0 (a uniform wave between mixed ones) and from lane 32 (two waves
    half uniform, half random), and a last, partial wave that is uniform."""
    rng = np.random.default_rng(32)
    for n, starts in ((64 * 6 + 17, (64, 224)), (256 * 3 + 40, (0, 256 + 32, 512 + 96)),
                      (64 + 5, (0,)), (64 * 2 + 32, (96,))):
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        for k, s in enumerate(starts):
            x[s:s + 64] = 0.125 * (k + 1)
            y[s:s + 64] = -0.25 * (k + 1)
        tail = n - n % 64
        x[tail:], y[tail:] = 1.5, -1.5                   # the partial wave: one bin
        for bins in (100, 7, K_LDS_BINS + 1):            # (LDS and global counters)
            _check_hist1d(x, dtype, bins)
            _check_hist1d(y, dtype, bins, offset=1)
        for bins in (100, (128, 129)):
            _check_hist2d(x, y, dtype, bins)
        # uniform in x only: the joint bin differs from lane to lane
        _check_hist2d(x, rng.standard_normal(n), dtype, 100, offset=1)


def test_hist_of_a_narrow_range_at_a_large_offset(nsol):
    """(v - e[0]) * scale loses most of its bits here; the search on the edges that
    follows the guess has to put every value where NumPy does."""
    rng = np.random.default_rng(10000)
    n = 20011
    x32 = (10000.0 + rng.uniform(0, 1, n)).astype(np.float32)
    y32 = (20000.0 - rng.uniform(0, 2, n)).astype(np.float32)
    x64 = 1e15 + 60.0 * rng.uniform(0, 1, n)
    y64 = -1e15 + 30.0 * rng.uniform(0, 1, n)
    for bins in (100, 37):      # (about 1000 float32 and 480 float64 values apart in all)
        _check_hist1d(x32, np.float32, bins)
        _check_hist1d(x64, np.float64, bins, offset=1)
    for bins in (100, (100, 37)):
        _check_hist2d(x32, y32, np.float32, bins, offset=1)
        _check_hist2d(x64, y64, np.float64, bins)


def test_hist_of_a_range_too_narrow_for_its_bins_raises_as_numpy_does(nsol):
    from nsol_amd import ops
    x = (2.0 ** 24 + 2.0 * np.arange(33)).astype(np.float32)     # [2^24, 2^24 + 64]
    with pytest.raises(ValueError):
        np.histogram(x, 100)
    ar = Arena(dict(x=x), np.float32)
    with pytest.raises(ValueError):
        ops.histogram1d(ar.t["x"], 100)
    assert ar.guards_intact()
    _check_hist1d(x, np.float32, 32)                     # 32 bins of width 2 fit


# =========================================================================== 3. range
def _check_range(x, y, dtype, offset, label):
    from nsol_amd import ops
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    ar = Arena(dict(x=x, y=y), dtype, offset)
    got = ops.pair_range(ar.t["x"], ar.t["y"])
    fx, fy = x[np.isfinite(x)].astype(np.float64), y[np.isfinite(y)].astype(np.float64)
    want = (fx.min() if fx.size else np.inf, fx.max() if fx.size else -np.inf,
            fy.min() if fy.size else np.inf, fy.max() if fy.size else -np.inf,
            2 * x.size - fx.size - fy.size)
    assert got == tuple(want), (label, got, want)
    assert isinstance(got[4], int)
    assert ar.guards_intact(), label
    assert np.array_equal(ar.get("x", x.shape), x, equal_nan=True), label
    assert np.array_equal(ar.get("y", y.shape), y, equal_nan=True), label


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256 + 5])
@pytest.mark.parametrize("dtype", BOTH)
def test_pair_range_extremes_and_non_finite_values_wherever_they_sit(nsol, dtype, n):
    """Minimum and maximum of x and y at the first element, the last, the start of the
    last wave, the middle and inside the second workgroup, whose partial results
    k_pair_range_final takes up first (n = 257: a second workgroup of one element;
    2048 * 256 + 5: five threads make a second trip), with non-finite values beside them:
    x only, y only, both."""
    rng = np.random.default_rng(n)
    places = sorted({0, n - 1, ((n - 1) // 64) * 64, (n - 1) // 2, min(n - 1, 300)})
    bad = (np.nan, np.inf, -np.inf)
    for i, (p, q) in enumerate(itertools.product(places, places)):
        for where in ("none", "x", "y", "both"):
            x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
            x[p], y[q] = -5.0, 9.0                       # min x at p, max y at q
            x[q] = 7.0 if q != p else x[q]               # max x at q
            y[p] = -3.0 if q != p else y[p]              # min y at p
            if where in ("x", "both"):
                for k, j in enumerate(places):
                    if j not in (p, q):
                        x[j] = bad[k % 3]
            if where in ("y", "both"):
                for k, j in enumerate(places):
                    if j not in (p, q):
                        y[j] = bad[(k + 1) % 3]
                if n > 3:
                    y[1] = np.nan
            _check_range(x, y, dtype, (i + len(where)) % 2, "n=%d p=%d q=%d bad in %s"
                         % (n, p, q, where))


@pytest.mark.parametrize("dtype", BOTH)
def test_pair_range_of_nothing_finite(nsol, dtype):
    rng = np.random.default_rng(8)
    for n in (1, 257, 2048 * 256 + 5):
        x = rng.choice([np.nan, np.inf, -np.inf], n)
        y = rng.uniform(-1, 1, n)
        _check_range(x, y, dtype, 0, "x not finite n=%d" % n)     # (inf, -inf, ..., n)
        _check_range(y, x, dtype, 1, "y not finite n=%d" % n)
        _check_range(x, x, dtype, 0, "neither finite n=%d" % n)
        assert _range_of(x, y, dtype)[:2] == (np.inf, -np.inf)
        assert _range_of(x, y, dtype)[4] == n


def _range_of(x, y, dtype):
    from nsol_amd import ops
    ar = Arena(dict(x=np.asarray(x, dtype), y=np.asarray(y, dtype)), dtype)
    return ops.pair_range(ar.t["x"], ar.t["y"])
