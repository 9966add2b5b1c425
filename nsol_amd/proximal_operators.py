"""Proximal operators (drop-in for nsol/proximal_operators.py).

Static methods with the reference's names/arguments.  `x` may be a NumPy
array (host round trip through the GPU), a torch HIP tensor (device path used
by the solvers) or the solvers' symbolic probe.  All arithmetic is done by
libnsol_hip.so.
"""
import numpy as np

from . import _caches, ops
from .device import is_device_tensor, to_device, to_numpy
from .symbolic import Sym, TraceAbort, TauSym


# b / x_scale on the device for host arrays, keyed by the identity of the array the
# caller's lambda closes over (run_denoising.py:109-131 pass x0=b on every call) AND
# by a fingerprint of its contents, so that an array the caller changed in place
# between runs is uploaded again instead of served stale.
_bt_cache = []
_caches._registered.append(_bt_cache)
# the same for device tensors: nsol_amd/_caches.py says when an entry may be served
_bt_dev_cache = _caches.DataCache(4)


def _fingerprint(arr):
    """Cheap content signature: up to 4096 evenly spaced elements plus the
    ends.  Catches in-place rescaling, re-noising, refilling; a change confined
    to elements between the samples is not seen (copy the array instead)."""
    flat = arr.reshape(-1)
    if flat.size <= 4096:
        return flat.tobytes()
    step = flat.size // 4096
    return flat[::step].tobytes() + flat[-1:].tobytes()


def scaled_data_on_device(x0, x_scale, like):
    """b~ = x0 / x_scale as a device tensor with the dtype of `like`."""
    if is_device_tensor(x0):
        return scaled_tensor(x0, x_scale, like.dtype)
    arr = np.asarray(x0)
    key = (id(x0), arr.__array_interface__["data"][0], arr.size,
           float(x_scale), like.dtype, like.device.index, _fingerprint(arr))
    for k, ref, val in _bt_cache:
        if k == key and ref is x0:
            return val
    dev = to_device(arr.reshape(-1), np.float64)
    bt = ops.scale(dev, float(x_scale), divide=True)   # divide in float64
    bt = bt.to(like.dtype)                             # then round once
    _bt_cache.append((key, x0, bt))
    del _bt_cache[:-4]
    return bt


def scaled_tensor(src, x_scale, dtype):
    """src / x_scale for a device tensor, remembered while src is unchanged (the
    reference divides on every call, proximal_operators.py:117-120) -- a data term b
    or a start x0 that a caller's lambda hands over on every call
    (prox_linear_least_squares inside a primal-dual loop builds a Tikhonov solver per
    iteration) is divided once, not once per call."""
    flat = src.to(dtype).contiguous().view(-1)
    if flat.data_ptr() != src.data_ptr():      # converted / compacted: a temporary
        return ops.scale(flat, float(x_scale), divide=True)
    extra = float(x_scale)
    val = _bt_dev_cache.lookup((src,), extra)
    if val is None:
        val = _bt_dev_cache.store((src,), extra,
                                  ops.scale(flat, extra, divide=True))
    return val


# validated weights of the weighted data terms on the device, per working dtype
_wt_cache = []
_caches._registered.append(_wt_cache)
_wt_dev_cache = _caches.DataCache(4)


def check_weights(weights, n):
    """ValueError unless `weights` holds n finite, non-negative real (or bool)
    values.  Device tensors are checked on the device (one reduction, one
    synchronisation)."""
    if is_device_tensor(weights):
        size = int(weights.numel())
        kind = "b" if str(weights.dtype) == "torch.bool" else \
            ("c" if weights.is_complex() else "f")
    else:
        weights = np.asarray(weights)
        size, kind = int(weights.size), weights.dtype.kind
    if kind not in "biuf":
        raise ValueError("weights must be real or bool, not %s" % (weights.dtype,))
    if size != int(n):
        raise ValueError("weights hold %d values for %d voxels" % (size, int(n)))
    if size == 0 or kind == "b":
        return
    if is_device_tensor(weights):
        import torch
        flat = weights.contiguous().view(-1)
        if flat.dtype not in (torch.float32, torch.float64):
            flat = flat.to(torch.float64)
        lo, _, _, _, bad = ops.pair_range(flat, flat)
    else:
        bad = int(weights.size - np.count_nonzero(np.isfinite(weights)))
        lo = float(np.min(weights)) if not bad else 0.
    if bad:
        raise ValueError("weights must be finite (%d are not)" % bad)
    if lo < 0:
        raise ValueError("weights must not be negative (minimum %g)" % lo)


def weights_on_device(weights, like):
    """The weights (NumPy array or device tensor of any real or bool dtype), checked
    (check_weights) and converted once to a flat device tensor with the dtype of
    `like`; remembered like the scaled observation while the caller's array is
    unchanged."""
    n = int(weights.numel() if is_device_tensor(weights) else np.size(weights))
    if is_device_tensor(weights):
        val = _wt_dev_cache.lookup((weights,), str(like.dtype))
        if val is None:
            check_weights(weights, n)
            flat = weights.to(like.dtype).contiguous().view(-1)
            # (the caller's own memory is not kept alive by the cache: only that
            # it has been checked is remembered)
            own = flat.data_ptr() == weights.data_ptr()
            val = _wt_dev_cache.store((weights,), str(like.dtype),
                                      True if own else flat)
        return weights.contiguous().view(-1) if val is True else val
    arr = np.asarray(weights)
    key = (id(weights), arr.__array_interface__["data"][0], arr.size, str(arr.dtype),
           like.dtype, like.device.index, _fingerprint(arr))
    for k, ref, val in _wt_cache:
        if k == key and ref is weights:
            return val
    check_weights(arr, n)
    dt = np.float32 if "32" in str(like.dtype) else np.float64
    wt = to_device(arr.reshape(-1).astype(dt), dt)
    _wt_cache.append((key, weights, wt))
    del _wt_cache[:-4]
    return wt


def _weighted(x, tau, x0, weights, x_scale, op, name):
    if isinstance(x, Sym):
        # (the probe is answered unchecked: PrimalDualSolver.plan() checks the
        # weights, where a ValueError reaches the caller instead of the tracer)
        return _elementwise(x, None, (name, x0, float(x_scale), tau, weights))
    n = int(x0.numel() if is_device_tensor(x0) else np.size(x0))
    size = int(x.numel() if is_device_tensor(x) else np.size(x))
    if size != n:
        raise ValueError("x holds %d values, x0 %d" % (size, n))
    check = int(weights.numel() if is_device_tensor(weights) else np.size(weights))
    if check != n:
        raise ValueError("weights hold %d values for %d voxels" % (check, n))
    return _elementwise(
        x, lambda d: op(d, scaled_data_on_device(x0, x_scale, d),
                        weights_on_device(weights, d), tau), None)


def _elementwise(x, fn, desc):
    if isinstance(x, Sym):
        if x.desc is not None:
            raise TraceAbort("prox applied to a transformed probe")
        return Sym(x.shape, desc)
    if is_device_tensor(x):
        shape = tuple(x.shape)
        return fn(x.contiguous().view(-1)).view(shape)
    arr = np.asarray(x)
    dt = arr.dtype.type if arr.dtype in (np.float32, np.float64) \
        else np.float64
    return to_numpy(fn(to_device(arr, dt).view(-1)), dt).reshape(arr.shape)


def _project(x, dimension, den, desc):
    """The isotropic dual prox of a stacked gradient field x."""
    dimension = int(dimension)
    if dimension not in (1, 2, 3):
        raise ValueError("dimension must be 1, 2 or 3, not %r" % (dimension,))
    if isinstance(x, Sym):
        size = x.size
    else:
        size = int(x.numel()) if is_device_tensor(x) else int(np.size(x))
    if size == 0 or size % dimension:
        raise ValueError("a gradient field of %d elements is not %d blocks of "
                         "equal length" % (size, dimension))
    return _elementwise(
        x, lambda d: ops.prox_dual_project(d, dimension, den), desc)


class ProximalOperators(object):

    @staticmethod
    def prox_linear_least_squares(x, tau, A, A_adj, b, x0, iter_max=10,
                                  verbose=0, data_loss="linear",
                                  data_loss_scale=1, minimizer="lsmr",
                                  x_scale=1, bounds=(0, np.inf)):
        """Tikhonov solve with B = I, b_reg = x, alpha = 1/tau
        (proximal_operators.py:43-78)."""
        from . import tikhonov_linear_solver as tk
        if isinstance(x, Sym):
            raise TraceAbort("prox_linear_least_squares is not fused")
        identity = lambda v: v.flatten()
        if is_device_tensor(x):
            # the solvers' device path: b / x_scale and x0 / x_scale are formed
            # on the device once and remembered (scaled_data_on_device)
            b_s = scaled_data_on_device(b, x_scale, x)
            x0_s = scaled_data_on_device(x0, x_scale, x)
        else:
            b_s = to_numpy(b) / float(x_scale) if is_device_tensor(b) \
                else np.asarray(b) / float(x_scale)
            x0_s = to_numpy(x0) / float(x_scale) if is_device_tensor(x0) \
                else np.asarray(x0) / float(x_scale)
        tikhonov = tk.TikhonovLinearSolver(
            A=A, A_adj=A_adj, B=identity, B_adj=identity, x0=x0_s, b=b_s,
            b_reg=x, alpha=1. / tau, iter_max=iter_max, verbose=verbose,
            x_scale=x_scale, data_loss=data_loss,
            data_loss_scale=data_loss_scale, minimizer=minimizer,
            bounds=bounds,
            dtype=(np.float32 if is_device_tensor(x) and "32" in str(x.dtype)
                   else (np.float64 if is_device_tensor(x) else None)),
            _defer_scaling=is_device_tensor(x))
        # (on the solvers' device path the caller is a loop that goes on enqueueing and
        # synchronises at the end of its own run)
        tikhonov._sync_after_run = not is_device_tensor(x)
        tikhonov.run()
        if is_device_tensor(x):
            return tikhonov.take_x_device()       # (the solver is dropped here)
        return tikhonov.get_x()

    @staticmethod
    def prox_ell1_denoising(x, tau, x0, x_scale=1.):
        # proximal_operators.py:95-98
        return _elementwise(
            x, lambda d: ops.prox_ell1(
                d, scaled_data_on_device(x0, x_scale, d), tau),
            ("prox_ell1", x0, float(x_scale), tau))

    @staticmethod
    def prox_ell2_denoising(x, tau, x0, x_scale=1.):
        # proximal_operators.py:117-120
        return _elementwise(
            x, lambda d: ops.prox_ell2(
                d, scaled_data_on_device(x0, x_scale, d), tau),
            ("prox_ell2", x0, float(x_scale), tau))

    @staticmethod
    def prox_ell1_denoising_weighted(x, tau, x0, weights, x_scale=1.):
        """prox of tau * lambda sum_i w_i |x_i - x0_i|: the soft threshold of
        proximal_operators.py:95-98 with the per-voxel threshold tau * w_i.
        weights: NumPy array or device tensor of any real or bool dtype with x0's
        size, finite and >= 0 (ValueError otherwise), not scaled by x_scale.  Where
        w_i == 0 the result is x_i exactly, whatever x0 holds there."""
        return _weighted(x, tau, x0, weights, x_scale, ops.prox_ell1_weighted,
                         "prox_ell1_w")

    @staticmethod
    def prox_ell2_denoising_weighted(x, tau, x0, weights, x_scale=1.):
        """prox of tau * lambda / 2 sum_i w_i (x_i - x0_i)^2:
        (x + tau w x0 / x_scale) / (1 + tau w), proximal_operators.py:117-120 with
        per-voxel weights (see prox_ell1_denoising_weighted)."""
        return _weighted(x, tau, x0, weights, x_scale, ops.prox_ell2_weighted,
                         "prox_ell2_w")

    @staticmethod
    def prox_kl_denoising(x, tau, x0, x_scale=1.):
        """prox of tau * lambda sum_i (x_i - b~_i log x_i), b~ = x0 / x_scale >= 0: the
        Poisson (Kullback-Leibler) data term, the negative log-likelihood of photon
        counts x0 up to a constant.  In closed form (csrc/nsol_kl.hpp): with e = x - tau,
        s = sqrt(e^2 + 4 tau b~), (e + s) / 2 where e >= 0 and 2 tau b~ / (s - e) elsewhere;
        never negative.  The fused kernels do not hold this prox: a PrimalDualSolver run
        with it goes through the loop of separate kernels."""
        return ProximalOperators.prox_kl_denoising_weighted(x, tau, x0, None, x_scale)

    @staticmethod
    def prox_kl_denoising_weighted(x, tau, x0, weights, x_scale=1.):
        """prox_kl_denoising with per-voxel weights w_i >= 0 on the terms of the sum (see
        prox_ell1_denoising_weighted; None: all 1).  Where w_i == 0 the result is x_i
        exactly, whatever x0 holds there."""
        if isinstance(x, Sym):
            raise TraceAbort("prox_kl_denoising is not fused")
        n = int(x0.numel() if is_device_tensor(x0) else np.size(x0))
        size = int(x.numel() if is_device_tensor(x) else np.size(x))
        if size != n:
            raise ValueError("x holds %d values, x0 %d" % (size, n))
        if weights is not None:
            check = int(weights.numel() if is_device_tensor(weights)
                        else np.size(weights))
            if check != n:
                raise ValueError("weights hold %d values for %d voxels" % (check, n))
        return _elementwise(
            x, lambda d: ops.prox_kl(
                d, scaled_data_on_device(x0, x_scale, d),
                None if weights is None else weights_on_device(weights, d), tau), None)

    @staticmethod
    def prox_tv_conj(x, sigma):
        # proximal_operators.py:138-140
        return _elementwise(x, lambda d: ops.prox_dual_clamp(d, 1.0),
                            ("prox_tv_conj", sigma))

    @staticmethod
    def prox_huber_conj(x, sigma, gamma=0.05):
        # proximal_operators.py:156-159; the reference divides its argument
        # in place, here the argument is left untouched
        return _elementwise(
            x, lambda d: ops.prox_dual_clamp(d, 1. + sigma * gamma),
            ("prox_huber_conj", sigma, float(gamma)))

    @staticmethod
    def prox_tv_conj_isotropic(x, sigma, dimension):
        """prox_tv_conj for the isotropic total variation: x is the stacked
        gradient field of linear_operators.py:121-137 (`dimension` blocks), and
        every voxel's vector is divided by max(1, its Euclidean norm) -- the norm
        prior_measures.py:27-52 sums and admm_linear_solver.py:239-253 shrinks
        by -- where proximal_operators.py:138-140 clamps component by component."""
        return _project(x, dimension, 1.0,
                        ("prox_tv_conj_iso", sigma, int(dimension)))

    @staticmethod
    def prox_huber_conj_isotropic(x, sigma, dimension, gamma=0.05):
        """prox_huber_conj (proximal_operators.py:156-159) with the per-voxel
        vector norm: (x / (1 + sigma gamma)) / max(1, |x / (1 + sigma gamma)|_2)."""
        return _project(x, dimension, 1. + sigma * gamma,
                        ("prox_huber_conj_iso", sigma, float(gamma),
                         int(dimension)))
