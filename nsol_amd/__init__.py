"""nsol_amd -- MI355X-native primal-dual / ADMM hot path with NSoL's callable API.

Module and class names mirror gift-surg/NSoL (nsol.linear_operators,
nsol.proximal_operators, nsol.primal_dual_solver, nsol.admm_linear_solver,
nsol.tikhonov_linear_solver, ...), so caller code switches by changing the
import.  All arithmetic runs in hand-written HIP kernels (libnsol_hip.so, C ABI
in include/nsol_hip.h); there is no CPU fallback.
"""
from .device import set_default_dtype, get_default_dtype  # noqa: F401
from ._caches import invalidate_caches  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # nsol_amd.PrimalDualBatch / PrimalDualLinearSolver: resolved on first use, so that importing the package
    # stays as light as it was
    if name == "PrimalDualBatch":
        from .solver_batch import PrimalDualBatch
        return PrimalDualBatch
    if name == "PrimalDualLinearSolver":
        from .primal_dual_linear_solver import PrimalDualLinearSolver
        return PrimalDualLinearSolver
    if name == "TGVPrimalDualSolver":
        from .tgv_solver import TGVPrimalDualSolver
        return TGVPrimalDualSolver
    if name == "TGVPrimalDualLinearSolver":
        from .tgv_solver import TGVPrimalDualLinearSolver
        return TGVPrimalDualLinearSolver
    if name in ("PrimalDualLinearBatch", "PrimalDualLinearSweep"):
        from . import linear_stack
        return getattr(linear_stack, name)
    if name in ("TGVPrimalDualBatch", "TGVPrimalDualSweep"):
        from . import tgv_stack
        return getattr(tgv_stack, name)
    if name in ("TGVPrimalDualLinearBatch", "TGVPrimalDualLinearSweep"):
        from . import tgv_linear_stack
        return getattr(tgv_linear_stack, name)
    raise AttributeError("module 'nsol_amd' has no attribute '%s'" % name)
