"""SSIM, histograms, entropies / MI / NMI and Dice on the device
(nsol_measures.hip) against a test-local NumPy / SciPy restatement of the
reference's formulas.  Needs a real MI355X."""
import os
import re

import numpy as np
import pytest

from conftest import rel_l2
from test_measures_host import ssim_direct_1d, ssim_restated

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-9
# 1-D: SciPy's running sum along the whole (flattened) line drifts by itself
# (5e-9 measured on the flattened phantom64, where every window summed on its
# own agrees with the kernel to 1e-12): gate against the direct sums at
# SSIM_TOL and against SciPy at this bound
SSIM_TOL_SCIPY_1D = 2e-8


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()                      # fails loudly if the .so is missing
    return nsol_amd


@pytest.fixture(scope="module")
def sm(nsol):
    from nsol_amd.similarity_measures import SimilarityMeasures
    return SimilarityMeasures


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _noisy(a, sigma, seed):
    rng = np.random.default_rng(seed)
    return a.astype(np.float64) + sigma * rng.standard_normal(a.shape)


def _check_ssim(sm, x, y, label):
    got = sm.structural_similarity(x, y)
    dr = 2.0 if np.asarray(x).dtype.kind == "f" else \
        float(np.iinfo(x.dtype).max) - float(np.iinfo(x.dtype).min)
    want = ssim_restated(x, y, data_range=dr)
    err = abs(got - want)
    rel_l2([got], [want], label)           # logged with the other observed errors
    if np.ndim(x) == 1:
        direct = ssim_direct_1d(x, y, data_range=dr)
        rel_l2([got], [direct], label + " (direct sums)")
        assert abs(got - direct) <= SSIM_TOL, (label, got, direct)
        assert err <= SSIM_TOL_SCIPY_1D, (label, got, want, err)
    else:
        assert err <= SSIM_TOL, (label, got, want, err)
    return got


# ------------------------------------------------------------------- SSIM
def test_ssim_brainweb_2d_and_flat(sm, golden):
    bw = golden("measures")["brainweb_u8"]
    noisy = _noisy(bw, 12.0, 0)
    _check_ssim(sm, bw, noisy, "brainweb u8 vs f64")
    _check_ssim(sm, bw.astype(np.float64), noisy, "brainweb f64")
    _check_ssim(sm, bw.astype(np.float32), noisy.astype(np.float32), "brainweb f32")
    _check_ssim(sm, bw.astype(np.float32).flatten(), noisy.flatten(), "brainweb 1-D mixed")


def test_ssim_phantom_3d_and_flat(sm, golden):
    ph = golden("configs")["phantom64"]
    noisy = _noisy(ph, 0.1, 1).astype(np.float32)
    _check_ssim(sm, ph, noisy, "phantom f32")
    _check_ssim(sm, ph, noisy.astype(np.float64), "phantom mixed")
    _check_ssim(sm, ph.flatten(), noisy.flatten(), "phantom 1-D")
    got = sm.structural_similarity(_dev(ph), _dev(noisy))
    assert abs(got - ssim_restated(ph, noisy)) <= SSIM_TOL
    got = sm.structural_similarity(_dev(ph.flatten()),
                                   _dev(noisy.astype(np.float64).flatten()))
    assert abs(got - ssim_direct_1d(ph.flatten(), noisy.flatten())) <= SSIM_TOL


@pytest.mark.parametrize("shape", [(40, 37, 33), (7, 7), (7, 7, 7), (7,),
                                   (7, 30), (9, 7, 20), (5000,), (300, 17)])
def test_ssim_shapes(sm, shape):
    rng = np.random.default_rng(len(shape) * 100 + shape[0])
    x = rng.uniform(-1, 1, shape)
    y = 0.6 * x + 0.4 * rng.uniform(-1, 1, shape)
    _check_ssim(sm, x, y, "f64 %s" % (shape,))
    _check_ssim(sm, x.astype(np.float32), y.astype(np.float32), "f32 %s" % (shape,))


def test_ssim_f32_bit_identical_to_f64_cast_and_repeatable(sm, golden):
    ph = golden("configs")["phantom64"]
    noisy = _noisy(ph, 0.1, 2).astype(np.float32)
    a = sm.structural_similarity(ph, noisy)
    b = sm.structural_similarity(ph.astype(np.float64), noisy.astype(np.float64))
    c = sm.structural_similarity(ph, noisy)
    assert a == b == c
    f = sm.structural_similarity(ph.flatten(), noisy.flatten())
    g = sm.structural_similarity(ph.flatten().astype(np.float64),
                                 noisy.flatten().astype(np.float64))
    assert f == g
    assert abs(sm.structural_similarity(noisy, noisy) - 1.0) <= 1e-12
    assert abs(sm.structural_similarity(noisy.flatten(), noisy.flatten()) - 1.0) <= 1e-12


def test_ssim_rejects_small_extents_and_mismatched_shapes(sm):
    x = np.zeros((6, 20))
    with pytest.raises(ValueError):
        sm.structural_similarity(x, x)
    with pytest.raises(ValueError):
        sm.structural_similarity(np.zeros(6), np.zeros(6))
    with pytest.raises(ValueError):
        sm.structural_similarity(np.zeros((8, 9)), np.zeros((9, 8)))
    with pytest.raises(NotImplementedError):
        sm.structural_similarity(np.zeros((8, 9)), np.zeros((8, 9)),
                                 gaussian_weights=True)


def test_ssim_256_cubed_float32(sm):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((256, 256, 256), dtype=np.float32)
    y = (0.8 * x + 0.2 * rng.standard_normal((256, 256, 256), dtype=np.float32))
    _check_ssim(sm, x, y, "256^3 f32")


# ------------------------------------------------------------- histograms
def _on_edges(dtype, bins=100):
    """Data whose values include every edge NumPy builds for it."""
    rng = np.random.default_rng(7)
    base = rng.uniform(-2.0, 5.0, 3000).astype(dtype)
    e = np.histogram_bin_edges(base, bins)
    return np.concatenate([base, e.astype(dtype), e.astype(dtype)[::-1]])


def _hist_cases():
    rng = np.random.default_rng(11)
    r32 = rng.standard_normal(20011).astype(np.float32)
    r64 = rng.standard_normal(20011) * 3 + 1
    sparse = np.where(rng.uniform(size=20011) < 0.9, 0.0,
                      rng.uniform(0, 100, 20011)).astype(np.float32)
    e32, e64 = _on_edges(np.float32), _on_edges(np.float64)
    return {
        "edges32": (e32, e32[::-1].copy()),
        "edges64": (e64, e64[::-1].copy()),
        "edges_mixed": (e32, e64),
        "f32": (r32, r32 * 2 + 1),
        "f64": (r64, np.sin(r64)),
        "mixed": (r32, r64),
        "mixed_rev": (r64, r32),
        "zeros90": (sparse, sparse[::-1].copy()),
        "const": (np.full(5000, 3.0, np.float32), r32[:5000]),
        "both_const": (np.full(5000, -1.5), np.full(5000, 2.0)),
        "u8": (np.round(sparse).astype(np.uint8), r64.astype(np.float32)),
    }


HIST = sorted(_hist_cases())


@pytest.mark.parametrize("case", HIST)
@pytest.mark.parametrize("bins", [1, 100, (100, 37), 200])
def test_histograms_integer_equal_to_numpy(nsol, case, bins):
    from nsol_amd import ops
    x, y = _hist_cases()[case]
    dx = _dev(x.astype(np.float64) if x.dtype.kind != "f" else x)
    dy = _dev(y.astype(np.float64) if y.dtype.kind != "f" else y)
    counts, ex, ey, hx, hy = ops.histogram2d(dx, dy, bins, dtypes=(x.dtype, y.dtype),
                                             marginals=True)
    want, wx, wy = np.histogram2d(x, y, bins)
    assert ex.tobytes() == wx.tobytes() and ey.tobytes() == wy.tobytes()
    assert np.array_equal(counts, want.astype(np.int64))
    bx, by = (bins, bins) if np.ndim(bins) == 0 else bins
    assert np.array_equal(hx, np.histogram(x, bx)[0])
    assert np.array_equal(hy, np.histogram(y, by)[0])
    c1, e1 = ops.histogram1d(dx, bx, dtype=x.dtype)
    w1, we1 = np.histogram(x, bx)
    assert e1.tobytes() == we1.tobytes() and np.array_equal(c1, w1)


def test_histograms_beyond_2_31_elements(nsol):
    import torch
    from nsol_amd import ops
    n = (1 << 31) + 64
    rng = np.random.default_rng(13)
    px = rng.standard_normal(1000).astype(np.float32)
    py = np.where(rng.uniform(size=1000) < 0.5, 0.0,
                  rng.uniform(0, 9, 1000)).astype(np.float32)
    reps, rem = divmod(n, 1000)
    x = _dev(px).repeat(reps + 1)[:n]
    y = _dev(py).repeat(reps + 1)[:n]
    assert x.numel() == n
    counts, ex, ey, hx, hy = ops.histogram2d(x, y, 100, marginals=True)
    want = reps * np.histogram2d(px, py, [ex, ey])[0] + \
        np.histogram2d(px[:rem], py[:rem], [ex, ey])[0]
    assert np.array_equal(counts, want.astype(np.int64))
    assert counts.sum() == n
    wx = reps * np.histogram(px, ex)[0] + np.histogram(px[:rem], ex)[0]
    assert np.array_equal(hx, wx)
    c1, e1 = ops.histogram1d(y, 100)
    wy = reps * np.histogram(py, e1)[0] + np.histogram(py[:rem], e1)[0]
    assert np.array_equal(c1, wy) and np.array_equal(hy, wy)
    del x, y
    torch.cuda.empty_cache()


# ---------------------------------------------------- entropies / MI / NMI
def _ref_entropy(hist):
    prob = hist / float(np.sum(hist))
    return - sum([p * np.log(p) for p in prob.flatten() if p != 0])


def _ref_h(x, bins=100):
    return _ref_entropy(np.histogram(x, bins=bins)[0])


def _ref_hxy(x, y, bins=100):
    return _ref_entropy(np.histogram2d(x.flatten(), y.flatten(), bins=bins)[0])


def _close(a, b):
    return abs(a - b) <= 1e-13 * max(abs(b), 1e-300)


@pytest.mark.parametrize("case", HIST)
def test_entropies_mi_nmi_match_reference_expressions(sm, case):
    x, y = _hist_cases()[case]
    for bins in (1, 100, 200):
        hx, hy, hxy = _ref_h(x, bins), _ref_h(y, bins), _ref_hxy(x, y, bins)
        assert _close(sm.shannon_entropy(x, bins), hx)
        assert _close(sm.joint_entropy(x, y, bins), hxy)
        assert _close(sm.mutual_information(x, y, bins), hx + hy - hxy)
        # symmetric up to the order of the entropy sums: the reference's
        # expressions differ by up to 5e-13 between (x, y) and (y, x) here
        mxy, myx = sm.mutual_information(x, y, bins), sm.mutual_information(y, x, bins)
        assert _close(myx, hy + hx - _ref_hxy(y, x, bins))
        assert abs(mxy - myx) <= 1e-11 * max(abs(mxy), 1e-300)
        if hxy != 0:
            assert _close(sm.normalized_mutual_information(x, y, bins),
                          (hx + hy) / hxy)
    assert _close(sm.joint_entropy(x, y, (100, 37)), _ref_hxy(x, y, (100, 37)))
    # device tensors in, the same histograms
    if x.dtype.kind == "f" and y.dtype.kind == "f" and _ref_hxy(x, y) != 0:
        assert _close(sm.normalized_mutual_information(_dev(x), _dev(y)),
                      (_ref_h(x) + _ref_h(y)) / _ref_hxy(x, y))


def test_entropy_measures_on_images(sm, golden):
    bw = golden("measures")["brainweb_u8"]
    noisy = _noisy(bw, 12.0, 3).astype(np.float32)
    ph = golden("configs")["phantom64"]
    phn = _noisy(ph, 0.1, 4)
    for x, y in ((bw, noisy), (ph, phn), (ph.flatten(), phn.flatten().astype(np.float32))):
        hx, hy, hxy = _ref_h(x), _ref_h(y), _ref_hxy(x, y)
        assert _close(sm.mutual_information(x, y), hx + hy - hxy)
        assert _close(sm.normalized_mutual_information(x, y), (hx + hy) / hxy)


def test_constant_inputs_give_nan_nmi_and_nonfinite_raises(sm):
    c = np.full(1000, 4.0, np.float32)
    h = sm.shannon_entropy(c)
    assert h == 0.0 and np.signbit(h)
    assert np.isnan(sm.normalized_mutual_information(c, c))
    for bad in (np.nan, np.inf, -np.inf):
        x = np.linspace(0, 1, 500)
        x[123] = bad
        with pytest.raises(ValueError):
            sm.mutual_information(x, np.linspace(0, 1, 500))
        with pytest.raises(ValueError):
            sm.normalized_mutual_information(np.linspace(0, 1, 500), x)
        with pytest.raises(ValueError):
            sm.shannon_entropy(x.astype(np.float32))


# --------------------------------------------------------------------- Dice
def test_dice_score(sm):
    rng = np.random.default_rng(17)
    for p, q in ((0.3, 0.6), (0.01, 0.9), (0.5, 0.5)):
        a = rng.uniform(size=(30, 41, 17)) < p
        b = rng.uniform(size=(30, 41, 17)) < q
        want = 2 * np.sum(a & b) / float(np.sum(a) + np.sum(b))
        assert sm.dice_score(a, b) == want
        assert sm.dice_score(_dev(a), _dev(b)) == want
    with pytest.raises(ValueError):
        sm.dice_score(a.astype(np.float32), b)
    with pytest.raises(ValueError):
        sm.dice_score(a, b.astype(np.uint8))
    z = np.zeros(100, bool)
    assert np.isnan(sm.dice_score(z, z))


# ---------------------------------------------------------------------- CLI
_LINE = re.compile(r"^  (\w+): (\S+) -> (\S+)$", re.M)


def _printed(out):
    return {m: (float(a), float(b)) for m, a, b in _LINE.findall(out)}


def _restated(m, x, ref):
    if m == "SSIM":
        return ssim_restated(x, ref)
    if m == "PSNR":
        return 10 * np.log10(np.max(ref) ** 2 / np.mean((x - ref) ** 2))
    if m == "MI":
        return _ref_h(x) + _ref_h(ref) - _ref_hxy(x, ref)
    if m == "NMI":
        return (_ref_h(x) + _ref_h(ref)) / _ref_hxy(x, ref)
    raise KeyError(m)


def _check_printed(out, result, ref, measures):
    got = _printed(out)
    assert set(got) == set(measures), out
    x = np.load(result).flatten()
    for m in measures:
        want = float("%.6g" % _restated(m, x, ref))
        assert abs(got[m][1] - want) <= 1e-5 * abs(want), (m, got[m], want)


def test_run_denoising_cli_new_measures(tmp_path, golden, capsys):
    from nsol_amd.data_writer import DataWriter
    from nsol_amd.application import run_denoising
    g = golden("configs")
    lena = g["lena_noise_u8"].astype(np.float64)
    src = str(tmp_path / "lena.png")
    DataWriter(lena, src).write_data()
    out = str(tmp_path / "recon.npy")
    measures = ["PSNR", "SSIM", "MI", "NMI"]
    assert run_denoising.main(["--observation", src, "--result", out,
                               "--reference", src, "--iterations", "10",
                               "--measures"] + measures) == 0
    _check_printed(capsys.readouterr().out, out, lena.flatten(), measures)


@pytest.mark.parametrize("rtype,solver", [("TK0L2", "PD"), ("TVL2", "ADMM")])
def test_run_deconvolution_cli_measures(tmp_path, golden, capsys, rtype, solver):
    from nsol_amd.data_writer import DataWriter
    from nsol_amd.application import run_deconvolution
    g = golden("configs")
    lena = g["lena_noise_u8"][:96, :128].astype(np.float64)
    src = str(tmp_path / "lena.png")
    DataWriter(lena, src).write_data()
    out = str(tmp_path / "dec.npy")
    measures = ["PSNR", "SSIM", "NMI"]
    assert run_deconvolution.main([
        "--observation", src, "--result", out, "--blur", "1.2",
        "--reconstruction-type", rtype, "--solver", solver,
        "--iterations", "3", "--iter-max", "4", "--reference", src,
        "--measures"] + measures) == 0
    _check_printed(capsys.readouterr().out, out, lena.flatten(), measures)
    # without --reference nothing is printed but the timing line
    assert run_deconvolution.main([
        "--observation", src, "--result", out, "--blur", "1.2",
        "--reconstruction-type", rtype, "--solver", solver,
        "--iterations", "3", "--iter-max", "4"]) == 0
    assert not _printed(capsys.readouterr().out)
    assert os.path.getsize(out) > 0
