"""The states and the finite box of the stacked LIN tests (k_tgv_primal_lin_stack), shared
by test_tgv_linear_stack_gpu.py, which launches on them, and test_tgv_linear_stack_host.py,
which asserts on the CPU that the box is at work in every member.  No GPU."""
import functools

import numpy as np

from nsol_amd import tgv_numpy as tg
from test_tgv_stack_gpu import TAU, THETA, _c, _rounded_spacing
from test_tgv_stack_gpu import _state as _stack_state

MEMBERS = 3
OPEN = (-np.inf, np.inf)
# the finite box sits at these quantiles of the members' unclipped steps, pooled: about
# 30 % of every member's voxels below it, 40 % inside, 30 % above
QUANTILES = (0.3, 0.7)


@functools.lru_cache(maxsize=None)
def lin_state(shape, dtype, m):
    """Member m's state of test_tgv_stack_gpu.py (rounded to dtype, held in float64) with
    its own g = A^T r.  Never modified."""
    rng = np.random.default_rng(5000 + sum(shape) + len(shape) + 101 * m)
    st = dict(_stack_state(shape, dtype, m))
    st["g"] = (0.8 * rng.standard_normal(shape)).astype(dtype).astype(np.float64)
    st["g"].setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def want_lin(shape, dtype, m, box):
    """(x+, xbar, w+, wbar) of member m, restated: float64 arithmetic on the state that
    dtype can hold, the scalars and the box as a kernel of dtype sees them."""
    s = lin_state(shape, dtype, m)
    return tg.primal_step_lin(s["p"], s["q"], s["x"], s["w"], s["g"], _c(dtype, TAU),
                              _c(dtype, THETA), box[0], box[1],
                              _rounded_spacing(shape, dtype), dtype)


@functools.lru_cache(maxsize=None)
def finite_box(shape, dtype):
    """(lo, hi): the QUANTILES of the unclipped x+ of all members together."""
    u = np.concatenate([want_lin(shape, dtype, m, OPEN)[0].reshape(-1)
                        for m in range(MEMBERS)])
    lo, hi = (float(v) for v in np.quantile(u, QUANTILES))
    assert lo < hi
    return lo, hi


def box_shares(shape, dtype, m):
    """Fractions of member m's voxels that the finite box puts at lo, strictly inside, at
    hi (float64 restatement)."""
    lo, hi = finite_box(shape, dtype)
    x = want_lin(shape, dtype, m, (lo, hi))[0]
    # (float32 rounds the box towards its inside: the clipped values sit at the ends of
    # the rounded box)
    lo_in, hi_in = x.min(), x.max()
    assert lo <= lo_in < hi_in <= hi
    return (float(np.mean(x == lo_in)), float(np.mean((x > lo_in) & (x < hi_in))),
            float(np.mean(x == hi_in)))
