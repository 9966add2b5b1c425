"""TVL1 / TVL2 / HuberL1 / HuberL2 denoising from the command line
(nsol_run_denoising of the reference, nsol/application/run_denoising.py:33-195,
without plotting).

    python -m nsol_amd.application.run_denoising --observation in.nii.gz \\
        --result out.nii.gz --reconstruction-type TVL2 --alpha 0.03 \\
        --iterations 50 [--reference gt.nii.gz] [--L2 8] [--dtype float32]
        [--isotropic] [--mask mask.nii.gz | --weights w.nii.gz]
        [--tolerance 1e-3 [--check-every 10]]

--tolerance T: stop before --iterations once the iterates have stopped changing --
max(r_x, r_p) <= T with r the relative change of the primal and of the dual iterate
in one iteration, evaluated every --check-every iterations and at the last
(PrimalDualSolver); the iterations actually done are printed.  Tolerances below
about 1e-6 are not met in float32.  Several --alpha and --slice-wise then keep their
members stacked, one launch per iteration for those still running, and every member
stops at its own iteration (stacked_stopping of PrimalDualSweep / PrimalDualBatch).

--isotropic: the regulariser is the isotropic TV / Huber norm -- the per-voxel
vector norm that PriorMeasures reports and ADMM minimises -- instead of the
reference's sum over the components (one fused launch per iteration).

Several values of --alpha are a parameter sweep (nsol_amd/parameter_sweep.py): the
members run stacked, one launch per iteration for all of them; --result-dir DIR
keeps every member (<stem>_alpha<value><ext>) next to a sweep.npz.

--mask FILE / --weights FILE: a weighted data term, sum_i w_i (x_i - b_i)^2 or
sum_i w_i |x_i - b_i| (prox_ell*_denoising_weighted).  --mask uses voxels > 0 as
weight 1 and the rest as weight 0 (the result is inpainted there, whatever the
observation holds); --weights takes the image's values as they are (finite, >= 0).
The image must have the observation's shape.  Both compose with --isotropic, several
--alpha and --slice-wise (the weights are sliced with the data; a slice whose
weights are all zero is copied through).

--reconstruction-type TGVL2 | TGVL1 [--beta B]: second-order total generalised
variation (TGVPrimalDualSolver, nsol_amd/tgv_solver.py), which keeps the smooth ramps
that TV turns into terraces; B (default 2) weighs the second-order term.  Composes
with --isotropic, --tolerance / --check-every, --dtype, --reference / --measures and
--observe-every; several --alpha, --slice-wise, --mask / --weights and --alg-type are
refused.  --L2 defaults to the bound of the operator's norm for these types.

--slice-wise: a 3-D observation is shape[0] independent 2-D images, each with its
own x_scale = max(slice), run together through PrimalDualBatch
(nsol_amd/solver_batch.py) -- one launch per iteration for all slices -- and
reassembled; a slice without a positive maximum is copied through unchanged.
"""
import argparse
import os
import sys

import numpy as np

from .. import linear_operators as LinearOperators
from .. import primal_dual_solver as pd
from .. import data_reader as dr
from .. import data_writer as dw
from .. import observer as Observer
from ..proximal_operators import ProximalOperators as prox
from ..similarity_measures import SimilarityMeasures


DEFAULT_ALG_TYPE = "ALG2"


def wiring(observed_nda, reconstruction_type, isotropic=False, weights=None):
    """Wiring of run_denoising.py:95-154: the callables, start and scale that
    PrimalDualSolver / PrimalDualSweep are built from.  isotropic: the dual prox
    projects every voxel's gradient vector (prox_*_conj_isotropic).  weights: an
    array of the observation's shape, the per-voxel weights of the data term; the
    scale is then the maximum over the voxels that count, and the start is zero
    where a voxel that does not count holds no finite value."""
    dimension = observed_nda.ndim
    b = observed_nda.flatten()
    x0 = observed_nda.flatten()
    x_scale = np.max(observed_nda)
    if weights is not None:
        weights = np.asarray(weights)
        if weights.shape != observed_nda.shape:
            raise ValueError("the weights have shape %s, the observation %s" %
                             (weights.shape, observed_nda.shape))
        w = weights.flatten()
        counted = w > 0
        x_scale = np.max(b[counted]) if counted.any() else 1.
        x0[~counted & ~np.isfinite(x0)] = 0
    linear_operators = getattr(
        LinearOperators, "LinearOperators%dD" % dimension)()
    grad, grad_adj = linear_operators.get_gradient_operators()
    X_shape = observed_nda.shape
    Z_shape = (dimension * X_shape[0],) + tuple(X_shape[1:]) \
        if dimension > 1 else X_shape
    D_1D = lambda x: grad(x.reshape(*X_shape)).flatten()
    D_adj_1D = lambda x: grad_adj(x.reshape(*Z_shape)).flatten()
    if reconstruction_type in ("TVL1", "HuberL1"):
        prox_f = lambda x, tau: prox.prox_ell1_denoising(
            x, tau, x0=b, x_scale=x_scale)
        if weights is not None:
            prox_f = lambda x, tau: prox.prox_ell1_denoising_weighted(
                x, tau, x0=b, weights=w, x_scale=x_scale)
    elif reconstruction_type in ("TVL2", "HuberL2"):
        prox_f = lambda x, tau: prox.prox_ell2_denoising(
            x, tau, x0=b, x_scale=x_scale)
        if weights is not None:
            prox_f = lambda x, tau: prox.prox_ell2_denoising_weighted(
                x, tau, x0=b, weights=w, x_scale=x_scale)
    else:
        raise ValueError("Denoising type '%s' not known" %
                         reconstruction_type)
    prox_g_conj = prox.prox_huber_conj \
        if reconstruction_type.startswith("Huber") else prox.prox_tv_conj
    if isotropic:
        if reconstruction_type.startswith("Huber"):
            prox_g_conj = lambda x, sigma: prox.prox_huber_conj_isotropic(
                x, sigma, dimension)
        else:
            prox_g_conj = lambda x, sigma: prox.prox_tv_conj_isotropic(
                x, sigma, dimension)
    return dict(prox_f=prox_f, prox_g_conj=prox_g_conj, B=D_1D, B_conj=D_adj_1D,
                x0=x0, x_scale=x_scale)


def build_solver(observed_nda, reconstruction_type, alpha, iterations, L2=8,
                 verbose=0, dtype=None, alg_type="ALG2", weights=None,
                 tolerance=None, check_every=10, isotropic=False):
    return pd.PrimalDualSolver(
        L2=L2, alpha=alpha, iterations=iterations, verbose=verbose,
        alg_type=alg_type, dtype=dtype, tolerance=tolerance, check_every=check_every,
        **wiring(observed_nda, reconstruction_type, isotropic, weights))


def read_weights(args, shape):
    """The weights that --mask / --weights name (None without either): the mask
    as 1 where its voxel is > 0 and 0 elsewhere, the weights as they are."""
    path = args.mask if args.mask is not None else args.weights
    if path is None:
        return None
    reader = dr.DataReader(path)
    reader.read_data()
    nda = np.asarray(reader.get_data())
    if nda.shape != tuple(shape):
        raise ValueError("'%s' has shape %s, the observation %s" %
                         (path, nda.shape, tuple(shape)))
    if args.mask is not None:
        return (nda > 0).astype(np.float64)
    return nda.astype(np.float64)


def member_result_path(result_dir, like, alpha):
    """<result_dir>/<stem>_alpha<value><ext> with stem and extension (".nii.gz"
    counts as one) of the file name `like`."""
    base = os.path.basename(like)
    stem, _, ext = base.partition(".")
    return os.path.join(result_dir, "%s_alpha%g%s" % (stem, alpha,
                                                     "." + ext if ext else ""))


def run_sweep(args, observed_nda, x_ref, reader, weights=None):
    """Several alphas: the members stacked through PrimalDualSweep."""
    from ..parameter_sweep import PrimalDualSweep
    sweep = PrimalDualSweep(
        L2=args.L2, parameters={"alpha": list(args.alpha)},
        iterations=args.iterations, alg_type=args.alg_type,
        dtype=np.dtype(args.dtype).type, tolerance=args.tolerance,
        check_every=args.check_every, stacked_stopping=args.tolerance is not None,
        **wiring(observed_nda, args.reconstruction_type, args.isotropic, weights))
    if x_ref is not None:
        sweep.set_measures({
            m: (lambda x, m=m:
                SimilarityMeasures.similarity_measures[m](x, x_ref))
            for m in args.measures},
            every=args.observe_every or max(args.iterations, 1))
    sweep.run()
    measures = sweep.get_measures()
    like = args.result if args.result is not None else args.observation
    for k, alpha in enumerate(args.alpha):
        print("%s alpha=%g: %d iterations in %s (%s)" % (
            args.reconstruction_type, alpha, args.iterations,
            sweep.get_computational_time(), sweep.get_execution()))
        if args.tolerance is not None:
            print("  stopped after %d of %d iterations" % (
                sweep.get_iterations_done()[k], args.iterations))
        for m, vals in measures.items():
            print("  %s: %.6g -> %.6g" % (m, vals[k, 0], last_observed(vals[k])))
        if args.result is not None or args.result_dir is not None:
            recon = np.array(sweep.get_x(k).reshape(*observed_nda.shape))
        if args.result is not None:
            dw.DataWriter(recon, args.result,
                          reader.get_image_sitk()).write_data()
        if args.result_dir is not None:
            dw.DataWriter(recon, member_result_path(args.result_dir, like, alpha),
                          reader.get_image_sitk()).write_data()
    if measures:
        lower = ("RMSE", "MSE", "MAE", "SSD", "SAD")
        print("best alpha: " + ", ".join(
            "%s %g" % (m, sweep.best(m, "min" if m in lower else "max")[1]["alpha"])
            for m in measures))
    if args.result_dir is not None:
        os.makedirs(args.result_dir, exist_ok=True)
        np.savez(os.path.join(args.result_dir, "sweep.npz"),
                 parameter_names=np.array(["alpha"]),
                 parameters=np.array(args.alpha, dtype=np.float64).reshape(-1, 1),
                 observed_iterations=np.array(sweep.get_observed_iterations(),
                                              dtype=np.int64),
                 **{"measure_" + m: v for m, v in measures.items()})
    return 0


def last_observed(vals):
    """The last value a measure took: a run that a tolerance stopped leaves the
    observation points behind its stop empty (NaN) in a device-mode observer."""
    vals = np.asarray(vals, dtype=np.float64)
    seen = np.flatnonzero(~np.isnan(vals))
    return vals[seen[-1]] if seen.size else vals[-1]


def print_stop(solver, iterations):
    """The line a run with --tolerance adds: the iterations actually done."""
    changes = solver.get_changes()
    print("  stopped after %d of %d iterations (%s%s)" % (
        solver.get_iterations_done(), iterations, solver.get_stop_reason(),
        "; last change %.3g" % max(changes[-1, 1:]) if len(changes) else ""))


def classify_slices(observed_nda, weights=None):
    """(indices of the slices to solve, indices copied through unchanged): a slice
    whose maximum is not positive has no x_scale to divide by (wiring()); with
    weights the maximum is taken over the voxels whose weight is positive, and a
    slice without any is copied through."""
    solve, copy = [], []
    for k in range(observed_nda.shape[0]):
        vals = observed_nda[k] if weights is None else \
            observed_nda[k][np.asarray(weights[k]) > 0]
        m = np.max(vals) if np.size(vals) else 0.
        (solve if np.isfinite(m) and m > 0 else copy).append(k)
    return solve, copy


def run_slice_wise(args, observed_nda, x_ref, reader, weights=None):
    """--slice-wise: one solver per slice, all through PrimalDualBatch."""
    from ..solver_batch import PrimalDualBatch
    solve, copy = classify_slices(observed_nda, weights)
    solvers = [build_solver(observed_nda[k], args.reconstruction_type,
                            args.alpha[0], args.iterations, L2=args.L2,
                            dtype=np.dtype(args.dtype).type,
                            alg_type=args.alg_type, isotropic=args.isotropic,
                            weights=None if weights is None else weights[k],
                            tolerance=args.tolerance, check_every=args.check_every)
               for k in solve]
    recon = np.array(observed_nda, dtype=np.float64)
    execution = []
    if solvers:
        batch = PrimalDualBatch(solvers, stacked_stopping=args.tolerance is not None)
        batch.run()
        execution = batch.get_execution()
        for k, solver in zip(solve, solvers):
            recon[k] = solver.get_x().reshape(*observed_nda.shape[1:])
        took = batch.get_computational_time()
    else:
        import datetime
        took = datetime.timedelta(seconds=0)
    print("%s alpha=%g slice-wise: %d iterations in %s (%d slices stacked, "
          "%d copied through, %d sequential)" % (
              args.reconstruction_type, args.alpha[0], args.iterations, took,
              execution.count("stacked"), len(copy),
              execution.count("sequential")))
    if args.tolerance is not None and solvers:
        done = [s.get_iterations_done() for s in solvers]
        print("  stopped after %d to %d of %d iterations" % (
            min(done), max(done), args.iterations))
    if x_ref is not None:
        flat = recon.flatten()
        for m in args.measures:
            print("  %s: %.6g" % (
                m, SimilarityMeasures.similarity_measures[m](flat, x_ref)))
    dw.DataWriter(recon, args.result, reader.get_image_sitk()).write_data()
    return 0


TGV_TYPES = ("TGVL2", "TGVL1")


def build_tgv_solver(observed_nda, reconstruction_type, alpha, beta, iterations, L2=None,
                     verbose=0, dtype=None, tolerance=None, check_every=10,
                     isotropic=False):
    """The TGVPrimalDualSolver of a TGVL2 / TGVL1 run: start, data and scale as
    wiring() takes them (x0 = b = the observation, x_scale its maximum)."""
    from ..tgv_solver import TGVPrimalDualSolver
    b = observed_nda.flatten()
    return TGVPrimalDualSolver(
        b, b.copy(), observed_nda.ndim, alpha=alpha, beta=beta, iterations=iterations,
        data_loss="ell1" if reconstruction_type == "TGVL1" else "ell2",
        isotropic=isotropic, L2=L2, x_scale=np.max(observed_nda), verbose=verbose,
        dtype=dtype, tolerance=tolerance, check_every=check_every,
        shape=observed_nda.shape)


def build_parser():
    ap = argparse.ArgumentParser(
        description="Run TVL1/TVL2/HuberL1/HuberL2/TGVL1/TGVL2 denoising on an MI355X")
    ap.add_argument("--observation", required=True)
    ap.add_argument("--result", required=False)
    ap.add_argument("--reference", required=False)
    ap.add_argument("--reconstruction-type", default="TVL2",
                    choices=["TVL1", "TVL2", "HuberL1", "HuberL2", "TGVL2", "TGVL1"])
    ap.add_argument("--beta", type=float, default=None, metavar="B",
                    help="TGVL2 / TGVL1: the weight of the second-order term "
                         "|E w|_1 against |grad x - w|_1 (default 2)")
    ap.add_argument("--measures", nargs="+",
                    default=["PSNR", "RMSE", "NCC"])
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--solver", default="PD", choices=["PD"])
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.03])
    ap.add_argument("--L2", type=float, default=None,
                    help="default 8, which the reference hard-codes "
                         "(run_denoising.py:147); 3-D data needs >= 12 for a "
                         "convergent step size.  TGVL2 / TGVL1: default the bound "
                         "of |K|^2 for the data's dimension")
    ap.add_argument("--alg-type", default=DEFAULT_ALG_TYPE)
    ap.add_argument("--dtype", default="float32",
                    choices=["float32", "float64"])
    ap.add_argument("--verbose", type=int, default=0)
    ap.add_argument("--observe-every", type=int, default=None, metavar="K",
                    help="evaluate the measures on the device every K "
                         "iterations (and at the last) instead of on a host "
                         "copy of every iterate")
    ap.add_argument("--isotropic", action="store_true",
                    help="isotropic TV / Huber: project every voxel's gradient "
                         "vector onto the unit ball (what PriorMeasures reports "
                         "and ADMM minimises) instead of clamping its components")
    ap.add_argument("--result-dir", default=None, metavar="DIR",
                    help="with several --alpha: every member's result as "
                         "<stem>_alpha<value><ext> and the sweep's parameters "
                         "and measures as sweep.npz in DIR")
    ap.add_argument("--slice-wise", action="store_true",
                    help="treat a 3-D observation as shape[0] independent 2-D "
                         "images, each scaled by its own maximum, and run them "
                         "stacked (one launch per iteration for all slices)")
    wgroup = ap.add_mutually_exclusive_group()
    wgroup.add_argument("--mask", default=None, metavar="FILE",
                        help="image of the observation's shape: voxels > 0 count "
                             "in the data term (weight 1), the rest do not (weight "
                             "0) and are inpainted by the regulariser")
    wgroup.add_argument("--weights", default=None, metavar="FILE",
                        help="image of the observation's shape: per-voxel weights "
                             "of the data term, finite and >= 0, taken as they are")
    ap.add_argument("--tolerance", type=float, default=None, metavar="T",
                    help="stop once the relative change of the primal and of the "
                         "dual iterate in one iteration is <= T (default: run all "
                         "--iterations); not met below about 1e-6 in float32")
    ap.add_argument("--check-every", type=int, default=10, metavar="K",
                    help="with --tolerance: evaluate the change every K iterations "
                         "and at the last")
    return ap


def parse_args(argv=None, ap=None):
    """The checked arguments; a combination that is not taken is a parser error."""
    ap = ap or build_parser()
    args = ap.parse_args(argv)
    if args.reconstruction_type in TGV_TYPES:
        if len(args.alpha) > 1:
            ap.error("--reconstruction-type %s takes a single --alpha" %
                     args.reconstruction_type)
        if args.slice_wise:
            ap.error("--reconstruction-type %s does not take --slice-wise" %
                     args.reconstruction_type)
        if args.mask is not None or args.weights is not None:
            ap.error("--reconstruction-type %s does not take %s" % (
                args.reconstruction_type,
                "--mask" if args.mask is not None else "--weights"))
        if args.alg_type != DEFAULT_ALG_TYPE:
            ap.error("--reconstruction-type %s does not take --alg-type: its "
                     "iteration has constant steps" % args.reconstruction_type)
        if args.beta is None:
            args.beta = 2.0
        if not (np.isfinite(args.beta) and args.beta > 0):
            ap.error("--beta must be positive")
    else:
        if args.beta is not None:
            ap.error("--beta goes with --reconstruction-type TGVL2 / TGVL1")
        if args.L2 is None:
            args.L2 = 8
    if args.tolerance is not None and not args.tolerance >= 0:
        ap.error("--tolerance must be >= 0")
    if args.check_every < 1:
        ap.error("--check-every must be >= 1")
    if args.slice_wise and len(args.alpha) > 1:
        ap.error("--slice-wise takes a single --alpha")
    if args.slice_wise and args.observe_every is not None:
        ap.error("--slice-wise does not take --observe-every: the measures are "
                 "taken once, on the reassembled volume")
    return args


def main(argv=None):
    ap = build_parser()
    args = parse_args(argv, ap)

    if len(args.alpha) == 1 and args.result is None:
        raise IOError("'--result' must be specified")

    reader = dr.DataReader(args.observation)
    reader.read_data()
    observed_nda = reader.get_data()
    x_ref = None
    if args.reference is not None:
        ref_reader = dr.DataReader(args.reference)
        ref_reader.read_data()
        x_ref = ref_reader.get_data().flatten()

    try:
        weights = read_weights(args, observed_nda.shape)
    except ValueError as e:
        ap.error(str(e))

    if args.slice_wise:
        if observed_nda.ndim != 3:
            ap.error("--slice-wise needs a 3-D observation, not %d-D" %
                     observed_nda.ndim)
        return run_slice_wise(args, observed_nda, x_ref, reader, weights)

    if len(args.alpha) > 1 and not args.verbose:
        return run_sweep(args, observed_nda, x_ref, reader, weights)

    for alpha in args.alpha:
        if args.reconstruction_type in TGV_TYPES:
            try:
                solver = build_tgv_solver(
                    observed_nda, args.reconstruction_type, alpha, args.beta,
                    args.iterations, L2=args.L2, verbose=args.verbose,
                    dtype=np.dtype(args.dtype).type, tolerance=args.tolerance,
                    check_every=args.check_every, isotropic=args.isotropic)
            except ValueError as e:
                ap.error(str(e))
        else:
            solver = build_solver(observed_nda, args.reconstruction_type, alpha,
                                  args.iterations, L2=args.L2,
                                  verbose=args.verbose,
                                  dtype=np.dtype(args.dtype).type,
                                  alg_type=args.alg_type,
                                  isotropic=args.isotropic, weights=weights,
                                  tolerance=args.tolerance,
                                  check_every=args.check_every)
        obs = None
        if x_ref is not None:
            obs = Observer.Observer() if args.observe_every is None else \
                Observer.Observer(keep_iterates=False, every=args.observe_every)
            obs.set_measures({
                m: (lambda x, m=m:
                    SimilarityMeasures.similarity_measures[m](x, x_ref))
                for m in args.measures})
        solver.set_observer(obs)
        solver.run()
        recon = np.array(solver.get_x().reshape(*observed_nda.shape))
        print("%s alpha=%g: %d iterations in %s (%s)" % (
            args.reconstruction_type, alpha, args.iterations,
            solver.get_computational_time(), solver.get_execution()))
        if args.tolerance is not None:
            print_stop(solver, args.iterations)
        if obs is not None:
            obs.compute_measures()
            for m, vals in obs.get_measures().items():
                print("  %s: %.6g -> %.6g" % (m, vals[0], last_observed(vals)))
        if args.result is not None:
            dw.DataWriter(recon, args.result,
                          reader.get_image_sitk()).write_data()
    return 0


if __name__ == "__main__":
    sys.exit(main())
