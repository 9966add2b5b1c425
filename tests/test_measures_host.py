"""Host-side pieces of SSIM / MI / NMI / Dice (no GPU needed): the test-local
restatement of skimage's SSIM that the GPU tests gate against, NumPy-exact
histogram edges, the C ABI of nsol_measures.hip and the deconvolution CLI's
new options."""
import ctypes
import itertools

import numpy as np
import pytest
from scipy.ndimage import uniform_filter

K1, K2 = 0.01, 0.03


def ssim_restated(x, y, win=7, data_range=2.0, sample_cov=True):
    """skimage compare_ssim (box window, sample covariance unless sample_cov is false) as
    published."""
    X = np.asarray(x, np.float64)
    Y = np.asarray(y, np.float64)
    npix = win ** X.ndim
    cov_norm = npix / (npix - 1.0) if sample_cov else 1.0
    ux = uniform_filter(X, size=win)
    uy = uniform_filter(Y, size=win)
    uxx = uniform_filter(X * X, size=win)
    uyy = uniform_filter(Y * Y, size=win)
    uxy = uniform_filter(X * Y, size=win)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
    B1, B2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    pad = (win - 1) // 2
    return S[tuple(slice(pad, n - pad) for n in S.shape)].mean()


def ssim_direct_1d(x, y, win=7, data_range=2.0, sample_cov=True):
    """The 1-D form with every window summed on its own (no running sum).
    SciPy's uniform_filter1d carries one running sum along the whole line;
    on a flattened volume that sum drifts (5e-9 on the mean SSIM of the
    flattened phantom64), so long 1-D lines are also checked against this."""
    from numpy.lib.stride_tricks import sliding_window_view
    X = np.asarray(x, np.float64)
    Y = np.asarray(y, np.float64)
    cov_norm = win / (win - 1.0) if sample_cov else 1.0

    def box(a):
        return sliding_window_view(a, win).sum(axis=-1) / win
    ux, uy, uxx, uyy, uxy = box(X), box(Y), box(X * X), box(Y * Y), box(X * Y)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / \
        ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return S.mean()


def ssim_brute(x, y, win=7, data_range=2.0, sample_cov=True):
    """One window at a time, straight from the definition."""
    X = np.asarray(x, np.float64)
    Y = np.asarray(y, np.float64)
    npix = win ** X.ndim
    div = npix - 1 if sample_cov else npix
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    vals = []
    for corner in itertools.product(*[range(n - win + 1) for n in X.shape]):
        sl = tuple(slice(c, c + win) for c in corner)
        a, b = X[sl].ravel(), Y[sl].ravel()
        mx, my = a.mean(), b.mean()
        vx = ((a - mx) ** 2).sum() / div
        vy = ((b - my) ** 2).sum() / div
        vxy = ((a - mx) * (b - my)).sum() / div
        vals.append(((2 * mx * my + C1) * (2 * vxy + C2)) /
                    ((mx * mx + my * my + C1) * (vx + vy + C2)))
    return float(np.mean(vals))


@pytest.mark.parametrize("shape", [(9, 11), (8, 9, 10), (40,)])
def test_restated_ssim_matches_brute_force_windows(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape)
    y = 0.7 * x + 0.3 * rng.standard_normal(shape)
    for dr in (2.0, 255.0):
        assert abs(ssim_restated(x, y, data_range=dr) -
                   ssim_brute(x, y, data_range=dr)) < 1e-13
    assert abs(ssim_restated(x, x) - 1.0) < 1e-13
    if x.ndim == 1:
        assert abs(ssim_direct_1d(x, y) - ssim_brute(x, y)) < 1e-13
    # every window the kernel is built for (7: above), on extents grown with the window
    for win in (3, 5, 9, 11):
        grown = tuple(s + max(0, win - 7) for s in shape)
        rng = np.random.default_rng(sum(grown) + win)
        x = rng.standard_normal(grown)
        y = 0.7 * x + 0.3 * rng.standard_normal(grown)
        for dr in (2.0, 255.0):
            want = ssim_brute(x, y, win, dr)
            assert abs(ssim_restated(x, y, win, dr) - want) < 1e-13, (win, dr)
            if x.ndim == 1:
                assert abs(ssim_direct_1d(x, y, win, dr) - want) < 1e-13, (win, dr)
        assert abs(ssim_restated(x, y, win, sample_cov=False) -
                   ssim_brute(x, y, win, sample_cov=False)) < 1e-13, win
        assert abs(ssim_restated(x, x, win) - 1.0) < 1e-13


def _edge_cases():
    rng = np.random.default_rng(3)
    r32 = rng.standard_normal(5000).astype(np.float32)
    r64 = rng.uniform(-3.0, 7.0, 5000)
    return [
        (r32, r32[::-1].copy()), (r64, r64[::-1].copy()), (r32, r64),
        (r64, r32), (np.full(100, 2.5, np.float32), r32[:100]),
        (np.full(100, -1.0), np.full(100, 3.0)),
        (np.full(100, 7, np.uint8), (r64[:100] * 10).astype(np.int16)),
        (rng.integers(0, 256, 500).astype(np.uint8), r32[:500]),
        (np.array([0.1, 1e-7, 3e5], np.float32), np.array([1, 2, 3], np.uint8)),
    ]


@pytest.mark.parametrize("case", range(9))
@pytest.mark.parametrize("bins", [1, 100, (100, 37), 200])
def test_host_edges_are_numpys_bit_for_bit(case, bins):
    from nsol_amd import ops
    x, y = _edge_cases()[case]
    bx, by = (bins, bins) if np.ndim(bins) == 0 else bins
    # what the device range pass delivers: min / max as float64
    rx = (float(x.min()), float(x.max()))
    ry = (float(y.min()), float(y.max()))
    for a, r, b in ((x, rx, bx), (y, ry, by)):
        want = np.histogram_bin_edges(a, b)
        got = ops.hist_edges(r[0], r[1], a.dtype, b)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        assert got.tobytes() == want.tobytes()
    _, wx, wy = np.histogram2d(x, y, (bx, by))
    gx, gy = ops.hist2d_edges(rx, ry, x.dtype, y.dtype, (bx, by))
    for g, w in ((gx, wx), (gy, wy)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


def test_measures_abi_declared_and_exported():
    from nsol_amd.build import build_library
    from nsol_amd import _lib
    path = build_library()
    decl = _lib.declared_symbols()
    raw = ctypes.CDLL(path)
    for base in ("ssim", "pair_range", "hist2d", "hist1d"):
        for suf in ("f32", "f64"):
            name = "nsol_%s_%s" % (base, suf)
            assert name in decl
            assert hasattr(raw, name)
    assert len(decl["nsol_ssim_f32"][1]) == 13
    assert len(decl["nsol_hist2d_f64"][1]) == 11
    assert _lib.load().nsol_hip_abi_version() == 1


def test_run_deconvolution_help_lists_reference_and_measures(capsys):
    from nsol_amd.application import run_deconvolution
    with pytest.raises(SystemExit) as e:
        run_deconvolution.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--reference" in out and "--measures" in out


def test_measure_tables_list_the_reference_keys():
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    keys = {"SSD", "MAE", "MSE", "RMSE", "PSNR", "SSIM", "NCC", "MI", "NMI"}
    assert set(sm.similarity_measures) >= keys
    assert set(sm.UNDEF) == keys and all(np.isnan(v) for v in sm.UNDEF.values())
