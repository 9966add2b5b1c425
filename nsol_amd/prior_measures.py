"""Regulariser values for reporting (drop-in for nsol/prior_measures.py:17-52),
evaluated with HIP reductions.  x: NumPy array or device tensor (flat);
D: a gradient callable as handed to the solvers.

Every measure answers the solvers' symbolic probe (symbolic.Sym) with a
descriptor of itself (symbolic.MeasureDesc) when D is nsol_amd's gradient
(recognised through the caller's lambda by trace_operator): observer.py
evaluates such measures on the device."""
import numpy as np

from . import ops
from .bridge import BridgedCallable
from .device import is_device_tensor, to_device
from .symbolic import TraceAbort, is_probe, measure_probe, trace_operator


def _dev(x):
    if is_device_tensor(x):
        return x.contiguous().view(-1)
    return to_device(np.asarray(x, dtype=np.float64).reshape(-1), np.float64)


def _apply(D, x):
    x = _dev(x)
    return BridgedCallable(D, np.float32 if "32" in str(x.dtype)
                           else np.float64)(x)


def _grad_probe(kind, x, D, dimension=None, gamma=None):
    if not is_probe(x):
        return None
    n = x.size
    g = trace_operator(D, n)
    if g is None or g[0] != "grad":
        raise TraceAbort("D is not nsol_amd's gradient")
    op, shape = g[1], tuple(g[2])
    if int(np.prod(shape)) != n or len(shape) != op.dimension or \
            (dimension is not None and int(dimension) != op.dimension):
        raise TraceAbort("gradient of another shape or dimension")
    return measure_probe(kind, x, grad=g, gamma=gamma)


class PriorMeasures(object):

    @staticmethod
    def zeroth_order_tikhonov(x):
        if is_probe(x):
            return measure_probe("TK0", x)
        x = _dev(x)
        return 0.5 * ops.dot(x, x)

    @staticmethod
    def first_order_tikhonov(x, D):
        if is_probe(x):
            return _grad_probe("TK1", x, D)
        g = _apply(D, x)
        return 0.5 * ops.dot(g, g)

    @staticmethod
    def total_variation(x, D, dimension):
        if is_probe(x):
            return _grad_probe("TV", x, D, dimension)
        return ops.vector_norm_sum(_apply(D, x), dimension, 0)

    @staticmethod
    def huber(x, D, dimension, gamma=0.05):
        if is_probe(x):
            if not float(gamma) > 0.0:
                raise TraceAbort("gamma")
            return _grad_probe("Huber", x, D, dimension, float(gamma))
        return ops.vector_norm_sum(_apply(D, x), dimension, 1, gamma)
