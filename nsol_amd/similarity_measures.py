"""Evaluation measures on the GPU (drop-in for
nsol/similarity_measures.py): SSD, SAD, MAE, MSE, RMSE, PSNR, NCC, SSIM, the
Shannon and joint entropies, MI, NMI and Dice.  x, x_ref: NumPy arrays or torch
HIP tensors of equal shape.

One fused pass (nsol_pair_stats_*) yields the sums of the reduction-type
measures; NCC takes a second, mean-centred pass for accuracy.  SSIM is
skimage's compare_ssim with its defaults (box window of 7 along every axis of
the input as given, K1 = 0.01, K2 = 0.03, sample covariance, data_range from
the dtype of x) in one pass (nsol_ssim_*).  The entropies take NumPy's integer
histogram counts from the device (nsol_pair_range_* fixes the edges,
nsol_hist2d_* / nsol_hist1d_* count) and evaluate the reference's expression
on the host.  The histogram measures keep the callers' dtypes: NumPy's bins
depend on them.

Every measure answers the solvers' symbolic probe (symbolic.Sym) with a
descriptor of itself (symbolic.MeasureDesc) instead of a value: that is how
observer.py recognises the measure lambdas callers write and evaluates them on
the device.
"""
import numpy as np
import torch

from . import ops
from .device import is_device_tensor, to_device
from .symbolic import TraceAbort, is_probe, measure_probe


def _pair(x, x_ref):
    shape_x = tuple(x.shape)
    if shape_x != tuple(x_ref.shape):
        raise ValueError("Input data shapes do not match")
    if is_device_tensor(x) and is_device_tensor(x_ref):
        a = x.contiguous().view(-1)
        return a, x_ref.to(a.dtype).contiguous().view(-1)
    dx = x if is_device_tensor(x) else to_device(
        np.asarray(x, dtype=np.float64).reshape(-1), np.float64)
    dr = x_ref if is_device_tensor(x_ref) else to_device(
        np.asarray(x_ref, dtype=np.float64).reshape(-1), np.float64)
    dx = dx.contiguous().view(-1)
    return dx, dr.to(dx.dtype).contiguous().view(-1)


def _upload(x):
    """Device tensor of x: float32 stays float32, everything else float64
    (exact for the integer types)."""
    if is_device_tensor(x):
        t = x.contiguous()
        return t if t.dtype in (torch.float32, torch.float64) \
            else t.to(torch.float64)
    a = np.asarray(x)
    return to_device(a, np.float32 if a.dtype == np.float32 else np.float64)


def _common(a, b):
    """Both tensors in one dtype: float32 if both are, else float64 (exact)."""
    if a.dtype == b.dtype:
        return a, b
    f64 = torch.float64
    return a.to(f64).contiguous(), b.to(f64).contiguous()


def _dtype_range(dt):
    """skimage's dtype_range[dt][1] - dtype_range[dt][0]."""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return 1.0
    if dt.kind == "f":
        return 2.0
    if dt.kind in "iu":
        info = np.iinfo(dt)
        return float(info.max) - float(info.min)
    raise ValueError("no default data_range for dtype %s" % dt)


def _entropy(hist):
    """The reference's expression (similarity_measures.py:157-161)."""
    prob = hist / float(np.sum(hist))
    return - sum([p * np.log(p) for p in prob.flatten() if p != 0])


def _histograms(x, x_ref, bins):
    """NumPy's histogram counts (x, x_ref, joint) of the two arrays, each in
    its own dtype, from one joint pass (plus 1-D passes where the dtypes
    give the 1-D histograms other edges than the joint one)."""
    if tuple(x.shape) != tuple(x_ref.shape):
        raise ValueError("Input data shapes do not match")
    if np.ndim(bins) != 0:
        raise ValueError("bins: only an integer number of bins is supported")
    dx, dy = ops.numpy_dtype(x), ops.numpy_dtype(x_ref)
    return _histograms_dev(_upload(x), _upload(x_ref), dx, dy, bins)


def _histograms_dev(ux, uy, dx, dy, bins):
    joint, _, _, hx, hy = ops.histogram2d(ux, uy, bins, dtypes=(dx, dy),
                                          marginals=True)
    return hx, hy, joint


def histogram_measure(kind, ux, dx, uy=None, dy=None, bins=100):
    """Measure `kind` ("entropy", "joint_entropy", "MI", "NMI") of device
    tensors ux, uy (as _upload leaves them) that hold arrays of NumPy dtypes
    dx, dy: the measures below and the observer's histogram class share it."""
    if kind == "entropy":
        counts, _ = ops.histogram1d(ux.view(-1), bins, dtype=dx)
        return _entropy(counts)
    if kind == "joint_entropy":
        joint, _, _ = ops.histogram2d(ux, uy, bins, dtypes=(dx, dy))
        return _entropy(joint)
    hx, hy, joint = _histograms_dev(ux, uy, dx, dy, bins)
    if kind == "MI":
        mi = _entropy(hx)
        mi += _entropy(hy)
        mi -= _entropy(joint)
        return mi
    if kind == "NMI":
        nmi = _entropy(hx)
        nmi += _entropy(hy)
        with np.errstate(invalid="ignore", divide="ignore"):
            nmi /= _entropy(joint)       # constant inputs: 0/0 = nan
        return nmi
    raise ValueError("not a histogram measure: %s" % kind)


def ssim_params(shape, ref_shape, dtype, win_size=7, data_range=None,
                gaussian_weights=False, gradient=False, full=False):
    """(win_size, C1, C2, cov_norm, number of windows) of SSIM of arrays of
    `shape` (x of NumPy dtype `dtype`); raises what structural_similarity
    raises for unsupported arguments."""
    if gaussian_weights or gradient or full:
        raise NotImplementedError(
            "SSIM: gaussian_weights, gradient and full are not supported")
    shape = tuple(shape)
    if shape != tuple(ref_shape):
        raise ValueError("Input images must have the same dimensions.")
    if not 1 <= len(shape) <= 3:
        raise NotImplementedError("SSIM: 1-D, 2-D and 3-D inputs only")
    if win_size % 2 != 1:
        raise ValueError("Window size must be odd.")
    if any(n < win_size for n in shape):
        raise ValueError("win_size exceeds image extent.")
    if not 3 <= win_size <= 11:
        raise NotImplementedError("SSIM: win_size 3, 5, 7, 9 or 11 only")
    if data_range is None:
        data_range = _dtype_range(dtype)
    npix = win_size ** len(shape)
    cov_norm = npix / (npix - 1.0)
    C1 = (0.01 * data_range) ** 2
    C2 = (0.03 * data_range) ** 2
    count = 1
    for n in shape:
        count *= n - win_size + 1
    return win_size, C1, C2, cov_norm, count


class SimilarityMeasures(object):

    @staticmethod
    def sum_of_absolute_differences(x, x_ref):
        if is_probe(x, x_ref):
            return measure_probe("SAD", x, x_ref)
        a, b = _pair(x, x_ref)
        return float(ops.pair_stats(a, b)[3])

    @staticmethod
    def mean_absolute_error(x, x_ref):
        if is_probe(x, x_ref):
            return measure_probe("MAE", x, x_ref)
        a, b = _pair(x, x_ref)
        return float(ops.pair_stats(a, b)[3]) / float(a.numel())

    @staticmethod
    def sum_of_squared_differences(x, x_ref):
        if is_probe(x, x_ref):
            return measure_probe("SSD", x, x_ref)
        a, b = _pair(x, x_ref)
        return float(ops.pair_stats(a, b)[4])

    @staticmethod
    def mean_squared_error(x, x_ref):
        if is_probe(x, x_ref):
            return measure_probe("MSE", x, x_ref)
        a, b = _pair(x, x_ref)
        return float(ops.pair_stats(a, b)[4]) / float(a.numel())

    @staticmethod
    def root_mean_square_error(x, x_ref):
        if is_probe(x, x_ref):
            return measure_probe("RMSE", x, x_ref)
        return float(np.sqrt(SimilarityMeasures.mean_squared_error(x, x_ref)))

    @staticmethod
    def peak_signal_to_noise_ratio(x, x_ref):
        if is_probe(x, x_ref):
            return measure_probe("PSNR", x, x_ref)
        a, b = _pair(x, x_ref)
        st = ops.pair_stats(a, b)
        mse = st[4] / float(a.numel())
        return float(10 * np.log10(st[5] ** 2 / mse))

    @staticmethod
    def normalized_cross_correlation(x, x_ref):
        if is_probe(x, x_ref):
            return measure_probe("NCC", x, x_ref)
        a, b = _pair(x, x_ref)
        n = float(a.numel())
        st = ops.pair_stats(a, b)
        st = ops.pair_stats(a, b, st[6] / n, st[7] / n)   # centred pass
        sx = np.sqrt(st[1] / (n - 1.0))
        sy = np.sqrt(st[2] / (n - 1.0))
        return float(st[0] / (n * sx * sy))

    @staticmethod
    def structural_similarity(x, x_ref, win_size=7, data_range=None,
                              gaussian_weights=False, gradient=False,
                              full=False):
        """skimage.measure.compare_ssim(x, x_ref) (the reference's call):
        mean SSIM over the valid box windows of win_size along every axis."""
        kw = dict(win_size=win_size, data_range=data_range,
                  gaussian_weights=gaussian_weights, gradient=gradient,
                  full=full)
        if is_probe(x, x_ref):
            # (the observer hands the measures float64 iterates, as get_x() does)
            try:
                ssim_params(x.shape, x_ref.shape, np.float64, **kw)
            except Exception:
                raise TraceAbort("SSIM arguments the measure refuses")
            return measure_probe("SSIM", x, x_ref, ssim=kw)
        shape = tuple(x.shape)
        win_size, C1, C2, cov_norm, count = ssim_params(
            shape, tuple(x_ref.shape), ops.numpy_dtype(x), **kw)
        a, b = _common(_upload(x), _upload(x_ref))
        total = ops.ssim_sum(a.view(-1), b.view(-1), shape, win_size, C1, C2,
                             cov_norm)
        return total / count

    @staticmethod
    def shannon_entropy(x, bins=100):
        if np.ndim(bins) != 0:
            raise ValueError("bins: only an integer number of bins is supported")
        if is_probe(x):
            return measure_probe("entropy", x, bins=bins)
        return histogram_measure("entropy", _upload(x), ops.numpy_dtype(x),
                                 bins=bins)

    @staticmethod
    def joint_entropy(x, x_ref, bins=100):
        if is_probe(x, x_ref):
            return measure_probe("joint_entropy", x, x_ref, bins=bins)
        if tuple(x.shape) != tuple(x_ref.shape):
            raise ValueError("Input data shapes do not match")
        return histogram_measure("joint_entropy", _upload(x), ops.numpy_dtype(x),
                                 _upload(x_ref), ops.numpy_dtype(x_ref), bins)

    @staticmethod
    def mutual_information(x, x_ref, bins=100):
        if is_probe(x, x_ref):
            if np.ndim(bins) != 0:
                raise TraceAbort("bins")
            return measure_probe("MI", x, x_ref, bins=bins)
        hx, hy, joint = _histograms(x, x_ref, bins)
        mi = _entropy(hx)
        mi += _entropy(hy)
        mi -= _entropy(joint)
        return mi

    @staticmethod
    def normalized_mutual_information(x, x_ref, bins=100):
        if is_probe(x, x_ref):
            if np.ndim(bins) != 0:
                raise TraceAbort("bins")
            return measure_probe("NMI", x, x_ref, bins=bins)
        hx, hy, joint = _histograms(x, x_ref, bins)
        nmi = _entropy(hx)
        nmi += _entropy(hy)
        with np.errstate(invalid="ignore", divide="ignore"):
            nmi /= _entropy(joint)       # constant inputs: 0/0 = nan
        return nmi

    @staticmethod
    def dice_score(x, x_ref):
        """2 |x and x_ref| / (|x| + |x_ref|) of two boolean masks."""
        if is_probe(x, x_ref):
            return measure_probe("Dice", x, x_ref)
        if ops.numpy_dtype(x) != np.bool_ or ops.numpy_dtype(x_ref) != np.bool_:
            raise ValueError("x and x_ref need to be of type boolean")
        if tuple(x.shape) != tuple(x_ref.shape):
            raise ValueError("Input data shapes do not match")
        f32 = torch.float32

        def mask(m):
            if is_device_tensor(m):
                return m.contiguous().view(-1).to(f32)
            return to_device(np.asarray(m, dtype=np.float32).reshape(-1),
                             np.float32)
        st = ops.pair_stats(mask(x), mask(x_ref))   # exact integer sums
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.float64(2.0 * st[0]) / np.float64(st[6] + st[7])

    SSD = sum_of_squared_differences
    SAD = sum_of_absolute_differences
    MAE = mean_absolute_error
    MSE = mean_squared_error
    RMSE = root_mean_square_error
    PSNR = peak_signal_to_noise_ratio
    NCC = normalized_cross_correlation
    SSIM = structural_similarity
    MI = mutual_information
    NMI = normalized_mutual_information


SimilarityMeasures.similarity_measures = {
    "SSD": SimilarityMeasures.sum_of_squared_differences,
    "SAD": SimilarityMeasures.sum_of_absolute_differences,
    "MAE": SimilarityMeasures.mean_absolute_error,
    "MSE": SimilarityMeasures.mean_squared_error,
    "RMSE": SimilarityMeasures.root_mean_square_error,
    "PSNR": SimilarityMeasures.peak_signal_to_noise_ratio,
    "SSIM": SimilarityMeasures.structural_similarity,
    "NCC": SimilarityMeasures.normalized_cross_correlation,
    "MI": SimilarityMeasures.mutual_information,
    "NMI": SimilarityMeasures.normalized_mutual_information,
}

# values that stand for an undefined measure (the reference's UNDEF)
SimilarityMeasures.UNDEF = {k: np.nan for k in (
    "SSD", "MAE", "MSE", "RMSE", "PSNR", "SSIM", "NCC", "MI", "NMI")}
