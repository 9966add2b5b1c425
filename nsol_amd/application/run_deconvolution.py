"""TK0L2 / TK1L2 / TVL2 / HuberL2 / TGVL2 deconvolution from the command line
(nsol_run_deconvolution of the reference, nsol/application/
run_deconvolution.py:28-245 and the wiring of
deconvolution_solver_parameter_study_interface.py:217-325, without plotting).

    python -m nsol_amd.application.run_deconvolution --observation blurred.png \\
        --result out.png --blur 2 --reconstruction-type TVL2 --solver ADMM \\
        [--reference gt.png] [--measures PSNR RMSE SSIM NCC NMI]
        [--tolerance 1e-3 [--check-every 10]]

--solver PD takes --tolerance T / --check-every K, the stopping rule of
PrimalDualSolver (see run_denoising); the iterations actually done are printed.

--solver PDL (TVL2 / HuberL2) is PrimalDualLinearSolver: the blur is part of the
saddle-point problem's linear map instead of the primal prox, so no iteration solves a
linear system (one blur, one adjoint blur and two element-wise / stencil passes per
iteration).  It takes --isotropic, --tolerance / --check-every, --observe-every,
--mask FILE (voxels > 0 count) or --weights FILE (per-voxel weights of the data term,
as in run_denoising), --data-loss kl [--background B] for Poisson counts, the
Kullback-Leibler term sum w_i ((A x + B)_i - b_i log (A x + B)_i) with the options ell1
takes, --data-loss ell1 for sum w_i |(A x - b)_i| ("linear" is the l2
data term) and --nonnegative for the exact projection onto x >= 0.  --L2 is not used:
the step sizes come from the operator norms.  PDL needs more iterations than PD, each
of them far cheaper.

--solver PDL --result-dir DIR: the --alpha values are one sweep
(nsol_amd/linear_stack.py, PrimalDualLinearSweep): the members share the observation,
the weights and the start and advance in stacked launches; every member is written to
DIR/<stem>_alpha<value><ext> next to a sweep.npz, as run_denoising does.  Without
--result-dir several --alpha are a loop of solvers, each written to --result.

--solver PDL --slice-wise: a 3-D observation is shape[0] independent 2-D images under
the 2-D Gaussian of --blur, each with its own x_scale (weights are sliced with the
data), run together through PrimalDualLinearBatch and reassembled; a single --alpha,
no --observe-every.  With --tolerance the members of either run one after the other
(the tool says so).

--solver PDL --upsample F [F ...] [--sample-offset O [O ...]]: super-resolution.  The
observation is the COARSE data of the model "blur, then keep every F-th sample from O
on" (SampledConvolutionOperator), one factor per ARRAY axis.  The result has shape
obs.shape * F and the spacing obs spacing / F (a NIfTI result carries it); --blur is
read on that fine grid; the start is sampled_start (A^T b / A^T 1).  --mask / --weights
keep the observation's shape, --reference has the result's.  Not with --slice-wise or
--result-dir, whose stacked forms need b and x on one grid.

--solver PDL --reconstruction-type TGVL2 [--beta B]: second-order total generalised
variation as the regulariser (TGVPrimalDualLinearSolver, nsol_amd/tgv_solver.py), which
keeps the smooth ramps TV turns into terraces; B (default 2) weighs |E w|_1 against
|grad x - w|_1.  It takes what the other PDL types take -- --data-loss ell1, --mask /
--weights, --nonnegative, --isotropic, --tolerance / --check-every, --upsample /
--sample-offset, --observe-every, --dtype; several --alpha loop -- except --result-dir
and --slice-wise: the stacked TGV forms (nsol_amd/tgv_linear_stack.py) are reachable
through the API only.  --L2 is not used, as for the other PDL types: the steps come from
tgv_numpy.norm_bound_linear.

--solver PDL --psf FILE: the blur is the point spread function in FILE (.npy, .nii,
.png, .mat through DataReader) instead of the Gaussian of --blur, which is then ignored.
The taps are taken as they are (no normalisation, no flip: A x is
scipy.ndimage.convolve(x, psf, mode="wrap")), the PSF has as many axes as the
observation, and the adjoint is the exact transpose (ConvolutionOperator.transpose), so
a motion blur or a measured, asymmetric PSF is deconvolved with the right A^T.  A PSF
that is no outer product runs through the tiled dense-tap kernel.  Not with --upsample
or --slice-wise; --solver PD / ADMM do not take it (their inner solves use A for A^T).

With --reference, the measures are evaluated through an Observer on the flat
iterates against the flat reference (as run_denoising does and as the
reference's tool does) and printed as first -> last value.
"""
import argparse
import os
import sys

import numpy as np

from .. import linear_operators as LinearOperators
from .. import primal_dual_solver as pd
from .. import primal_dual_linear_solver as pdl
from .. import admm_linear_solver as admm
from .. import tikhonov_linear_solver as tk
from .. import data_reader as dr
from .. import data_writer as dw
from .. import observer as Observer
from ..proximal_operators import ProximalOperators as prox
from ..similarity_measures import SimilarityMeasures
from .run_denoising import (classify_slices, last_observed, member_result_path,
                            print_stop, read_weights)


def _regulariser(reconstruction_type):
    """The solver's keyword arguments that name the regulariser: reg_type for TVL2 /
    HuberL2 (PrimalDualLinearSolver); none for TGVL2, whose solver takes beta."""
    if reconstruction_type == "TGVL2":
        return {}
    return dict(reg_type="TV" if reconstruction_type == "TVL2" else "huber")


def pdl_wiring(observed_nda, spacing, blur, reconstruction_type="TVL2", alpha=0.01,
               iterations=10, verbose=0, dtype=None, tolerance=None, check_every=10,
               weights=None, pdl_data_loss="ell2", nonnegative=False, isotropic=False,
               background=0., psf=None):
    """The keyword arguments PrimalDualLinearSolver (tv_solver="PDL") and
    PrimalDualLinearSweep are built from.  background (in the observation's units) goes
    with pdl_data_loss="kl".  psf: an array of taps with the observation's number of
    axes in the place of the Gaussian of `blur`, with its exact transpose as A_adj."""
    dimension = observed_nda.ndim
    sigma = np.atleast_1d(blur).astype(float)
    cov = np.diag(np.ones(dimension)) * sigma ** 2
    if dimension == 1:
        cov = float(cov.reshape(-1)[0])
    b = observed_nda.flatten()
    x0 = observed_nda.flatten()
    x_scale = np.max(observed_nda)
    lo = getattr(LinearOperators, "LinearOperators%dD" % dimension)(
        spacing=spacing)
    if psf is None:
        A, A_adj = lo.get_gaussian_blurring_operators(cov)
    else:
        A, A_adj = lo.get_convolution_and_adjoint_convolution_operators(
            checked_psf(psf, dimension), exact_adjoint=True)
    X = observed_nda.shape
    A_1D = lambda x: A(x.reshape(*X)).flatten()
    A_adj_1D = lambda x: A_adj(x.reshape(*X)).flatten()
    if weights is not None:
        # as run_denoising.wiring: the scale is the maximum over the voxels that
        # count, the start is zero where a voxel that does not count is not finite
        weights = np.asarray(weights)
        if weights.shape != observed_nda.shape:
            raise ValueError("the weights have shape %s, the observation %s" %
                             (weights.shape, observed_nda.shape))
        counted = weights.flatten() > 0
        x_scale = np.max(b[counted]) if counted.any() else 1.
        x0[~counted & ~np.isfinite(x0)] = 0
        weights = weights.flatten()
    return dict(
        A=A_1D, A_adj=A_adj_1D, b=b, x0=x0, dimension=dimension, spacing=spacing,
        alpha=alpha, iterations=iterations,
        **_regulariser(reconstruction_type),
        isotropic=isotropic, data_loss=pdl_data_loss, weights=weights,
        bounds=(0., np.inf) if nonnegative else None, x_scale=x_scale,
        verbose=verbose, dtype=dtype, tolerance=tolerance, check_every=check_every,
        **_background(background))


def checked_psf(psf, dimension):
    """The PSF as a float64 array of `dimension` axes with finite taps, or ValueError."""
    psf = np.asarray(psf, dtype=np.float64)
    if psf.ndim != dimension:
        raise ValueError("the PSF has %d axes, the observation %d" % (psf.ndim, dimension))
    if psf.size < 1 or not np.all(np.isfinite(psf)):
        raise ValueError("the PSF must hold finite taps")
    return psf


def _background(background):
    """The solvers' background= where there is one (their default otherwise)."""
    return dict(background=background) if background else {}


def fine_grid(shape, spacing, factors):
    """(fine shape, fine spacing) of an observation upsampled by `factors` (one per
    ARRAY axis); spacing[0] belongs to the LAST array axis."""
    factors = [int(f) for f in factors]
    if len(factors) != len(shape) or min(factors) < 1:
        raise ValueError("--upsample takes one factor >= 1 per axis of the "
                         "observation (%d), not %r" % (len(shape), factors))
    fine_shape = tuple(int(s) * f for s, f in zip(shape, factors))
    fine_spacing = np.atleast_1d(spacing).astype(float) / np.array(factors[::-1], float)
    return fine_shape, fine_spacing


def sampled_pdl_wiring(observed_nda, spacing, blur, factors, offsets=None,
                       reconstruction_type="TVL2", alpha=0.01, iterations=10, verbose=0,
                       dtype=None, tolerance=None, check_every=10, weights=None,
                       pdl_data_loss="ell2", nonnegative=False, isotropic=False,
                       background=0.):
    """PrimalDualLinearSolver's keyword arguments for --upsample: the observation is
    the coarse data of a SampledConvolutionOperator on the fine grid."""
    dimension = observed_nda.ndim
    coarse = observed_nda.shape
    fine_shape, fine_spacing = fine_grid(coarse, spacing, factors)
    sigma = np.atleast_1d(blur).astype(float)
    cov = np.diag(np.ones(dimension)) * sigma ** 2
    if dimension == 1:
        cov = float(cov.reshape(-1)[0])
    lo = getattr(LinearOperators, "LinearOperators%dD" % dimension)(
        spacing=fine_spacing)
    A, A_adj = lo.get_sampled_gaussian_blurring_operators(
        cov, factors, offsets, fine_shape=fine_shape)
    if A._out_shape(fine_shape) != tuple(coarse):
        raise ValueError("the observation's shape %r is not what the factors and "
                         "offsets keep of the fine grid %r" % (tuple(coarse), fine_shape))
    b = observed_nda.flatten()
    x_scale = np.max(observed_nda)
    seen = np.array(observed_nda, dtype=np.float64)
    if weights is not None:
        weights = np.asarray(weights)
        if weights.shape != observed_nda.shape:
            raise ValueError("the weights have shape %s, the observation %s" %
                             (weights.shape, observed_nda.shape))
        counted = weights > 0
        x_scale = np.max(observed_nda[counted]) if counted.any() else 1.
        seen[~counted & ~np.isfinite(seen)] = 0
        weights = weights.flatten()
    x0 = LinearOperators.sampled_start(A_adj, seen, fine_shape).flatten()
    A_1D = lambda x: A(x.reshape(*fine_shape)).flatten()
    A_adj_1D = lambda q: A_adj(q.reshape(*coarse)).flatten()
    return dict(
        A=A_1D, A_adj=A_adj_1D, b=b, x0=x0, dimension=dimension, spacing=fine_spacing,
        alpha=alpha, iterations=iterations,
        **_regulariser(reconstruction_type),
        isotropic=isotropic, data_loss=pdl_data_loss, weights=weights,
        bounds=(0., np.inf) if nonnegative else None, x_scale=x_scale,
        verbose=verbose, dtype=dtype, tolerance=tolerance, check_every=check_every,
        shape=fine_shape, **_background(background))


def build_solver(observed_nda, spacing, blur, reconstruction_type="TVL2",
                 tv_solver="PD", alpha=0.01, iterations=10, iter_max=10,
                 rho=0.1, minimizer="lsmr", data_loss="linear",
                 data_loss_scale=1., L2=8, verbose=0, dtype=None,
                 tolerance=None, check_every=10, weights=None, pdl_data_loss="ell2",
                 nonnegative=False, upsample=None, sample_offset=None, beta=2.0,
                 background=0., psf=None, isotropic=False):
    """psf (tv_solver="PDL" without upsample): taps in the place of the Gaussian of blur,
    with the exact transpose as the adjoint (pdl_wiring).

    weights, pdl_data_loss ("ell2" | "ell1" | "kl", the last with background, a
    constant in the observation's units) and nonnegative belong to
    tv_solver="PDL" (PrimalDualLinearSolver), and so do upsample / sample_offset (one
    integer per array axis: the observation is the coarse data, sampled_pdl_wiring).
    reconstruction_type "TGVL2" with tv_solver "PDL" is TGVPrimalDualLinearSolver on the
    same wiring, with beta in the place of the regulariser's type."""
    if psf is not None and (tv_solver != "PDL" or upsample is not None):
        raise ValueError("psf belongs to tv_solver='PDL' without upsample")
    if reconstruction_type == "TGVL2":
        if tv_solver != "PDL":
            raise ValueError("reconstruction_type 'TGVL2' belongs to tv_solver='PDL'")
        from ..tgv_solver import TGVPrimalDualLinearSolver
        if upsample is not None:
            kw = sampled_pdl_wiring(
                observed_nda, spacing, blur, upsample, sample_offset, "TGVL2", alpha,
                iterations, verbose, dtype, tolerance, check_every, weights,
                pdl_data_loss, nonnegative, isotropic, background)
        else:
            kw = pdl_wiring(
                observed_nda, spacing, blur, "TGVL2", alpha, iterations, verbose, dtype,
                tolerance, check_every, weights, pdl_data_loss, nonnegative, isotropic,
                background, psf)
        return TGVPrimalDualLinearSolver(beta=beta, **kw)
    if upsample is not None:
        if not (reconstruction_type in ("TVL2", "HuberL2") and tv_solver == "PDL"):
            raise ValueError("upsample belongs to tv_solver='PDL'")
        return pdl.PrimalDualLinearSolver(**sampled_pdl_wiring(
            observed_nda, spacing, blur, upsample, sample_offset, reconstruction_type,
            alpha, iterations, verbose, dtype, tolerance, check_every, weights,
            pdl_data_loss, nonnegative, isotropic, background))
    if reconstruction_type in ("TVL2", "HuberL2") and tv_solver == "PDL":
        return pdl.PrimalDualLinearSolver(**pdl_wiring(
            observed_nda, spacing, blur, reconstruction_type, alpha, iterations,
            verbose, dtype, tolerance, check_every, weights, pdl_data_loss,
            nonnegative, isotropic, background, psf))
    dimension = observed_nda.ndim
    sigma = np.atleast_1d(blur).astype(float)
    cov = np.diag(np.ones(dimension)) * sigma ** 2
    if dimension == 1:
        cov = float(cov.reshape(-1)[0])
    b = observed_nda.flatten()
    x0 = observed_nda.flatten()
    x_scale = np.max(observed_nda)
    lo = getattr(LinearOperators, "LinearOperators%dD" % dimension)(
        spacing=spacing)
    A, A_adj = lo.get_gaussian_blurring_operators(cov)
    grad, grad_adj = lo.get_gradient_operators()
    X = observed_nda.shape
    Z = (dimension * X[0],) + tuple(X[1:]) if dimension > 1 else X
    A_1D = lambda x: A(x.reshape(*X)).flatten()
    A_adj_1D = lambda x: A_adj(x.reshape(*X)).flatten()
    D_1D = lambda x: grad(x.reshape(*X)).flatten()
    D_adj_1D = lambda x: grad_adj(x.reshape(*Z)).flatten()
    I_1D = lambda x: x.flatten()
    common = dict(A=A_1D, A_adj=A_adj_1D, b=b, x0=x0, alpha=alpha,
                  x_scale=x_scale, data_loss=data_loss,
                  data_loss_scale=data_loss_scale, iter_max=iter_max,
                  verbose=verbose, dtype=dtype)
    if weights is not None or nonnegative or background:
        raise ValueError("weights, nonnegative and background belong to tv_solver='PDL'")
    if reconstruction_type == "TK0L2":
        return tk.TikhonovLinearSolver(B=I_1D, B_adj=I_1D,
                                       minimizer=minimizer, **common)
    if reconstruction_type == "TK1L2":
        return tk.TikhonovLinearSolver(B=D_1D, B_adj=D_adj_1D,
                                       minimizer=minimizer, **common)
    if reconstruction_type == "TVL2" and tv_solver == "ADMM":
        return admm.ADMMLinearSolver(B=D_1D, B_adj=D_adj_1D, rho=rho,
                                     iterations=iterations,
                                     dimension=dimension,
                                     minimizer=minimizer, **common)
    if reconstruction_type in ("TVL2", "HuberL2"):
        prox_f = lambda x, tau: prox.prox_linear_least_squares(
            x=x, tau=tau, A=A_1D, A_adj=A_adj_1D, b=b, x0=x0,
            iter_max=iter_max, data_loss=data_loss,
            data_loss_scale=data_loss_scale, x_scale=x_scale)
        pg = prox.prox_tv_conj if reconstruction_type == "TVL2" \
            else prox.prox_huber_conj
        if isotropic:
            # the per-voxel vector norm ADMM shrinks by (prox_*_conj_isotropic)
            iso = prox.prox_tv_conj_isotropic if reconstruction_type == "TVL2" \
                else prox.prox_huber_conj_isotropic
            pg = lambda x, sigma: iso(x, sigma, dimension)
        return pd.PrimalDualSolver(prox_f=prox_f, prox_g_conj=pg, B=D_1D,
                                   B_conj=D_adj_1D, L2=L2, alpha=alpha,
                                   x0=x0, iterations=iterations,
                                   x_scale=x_scale, verbose=verbose,
                                   dtype=dtype, tolerance=tolerance,
                                   check_every=check_every)
    raise ValueError("Reconstruction type '%s' not known" %
                     reconstruction_type)


def _pdl_arguments(args):
    """build_solver's / pdl_wiring's keyword arguments that --solver PDL takes from
    the command line."""
    return dict(dtype=np.dtype(args.dtype).type, isotropic=args.isotropic,
                tolerance=args.tolerance, check_every=args.check_every,
                pdl_data_loss=_pdl_data_loss(args),
                nonnegative=args.nonnegative, **_background(args.background))


def _pdl_data_loss(args):
    """--data-loss as the PDL solvers name it ("linear" is their l2 data term)."""
    return args.data_loss if args.data_loss in ("ell1", "kl") else "ell2"


def run_sweep(args, observed_nda, spacing, x_ref, info, weights=None, psf=None):
    """--solver PDL --result-dir: the --alpha values as one PrimalDualLinearSweep."""
    from ..linear_stack import PrimalDualLinearSweep
    kw = pdl_wiring(observed_nda, spacing, args.blur, args.reconstruction_type,
                    iterations=args.iterations, verbose=args.verbose, weights=weights,
                    psf=psf, **_pdl_arguments(args))
    del kw["alpha"]
    sweep = PrimalDualLinearSweep(parameters={"alpha": list(args.alpha)}, **kw)
    if x_ref is not None:
        sweep.set_measures({
            m: (lambda x, m=m:
                SimilarityMeasures.similarity_measures[m](x, x_ref))
            for m in args.measures},
            every=args.observe_every or max(args.iterations, 1))
    sweep.run()
    measures = sweep.get_measures()
    if sweep.get_execution() == "sequential":
        print("the members ran sequentially, one solver after the other")
    os.makedirs(args.result_dir, exist_ok=True)
    for k, alpha in enumerate(args.alpha):
        print("%s alpha=%g: %d iterations in %s (%s)" % (
            args.reconstruction_type, alpha, args.iterations,
            sweep.get_computational_time(), sweep.get_execution()))
        if args.tolerance is not None:
            print("  stopped after %d of %d iterations" % (
                sweep.get_iterations_done()[k], args.iterations))
        for m, vals in measures.items():
            print("  %s: %.6g -> %.6g" % (m, vals[k, 0], last_observed(vals[k])))
        recon = np.array(sweep.get_x(k).reshape(*observed_nda.shape))
        dw.DataWriter(recon, args.result, info).write_data()
        dw.DataWriter(recon, member_result_path(args.result_dir, args.result, alpha),
                      info).write_data()
    if measures:
        lower = ("RMSE", "MSE", "MAE", "SSD", "SAD")
        print("best alpha: " + ", ".join(
            "%s %g" % (m, sweep.best(m, "min" if m in lower else "max")[1]["alpha"])
            for m in measures))
    np.savez(os.path.join(args.result_dir, "sweep.npz"),
             parameter_names=np.array(["alpha"]),
             parameters=np.array(args.alpha, dtype=np.float64).reshape(-1, 1),
             observed_iterations=np.array(sweep.get_observed_iterations(),
                                          dtype=np.int64),
             **{"measure_" + m: v for m, v in measures.items()})
    return 0


def run_slice_wise(args, observed_nda, spacing, x_ref, info, weights=None):
    """--solver PDL --slice-wise: one 2-D solver per slice, all through
    PrimalDualLinearBatch; a slice without a positive maximum is copied through."""
    import datetime
    from ..linear_stack import PrimalDualLinearBatch
    solve, copy = classify_slices(observed_nda, weights)
    # spacing[0] belongs to the LAST array axis: a slice keeps the first two
    solvers = [build_solver(observed_nda[k], np.asarray(spacing)[:2], args.blur,
                            args.reconstruction_type, "PDL", args.alpha[0],
                            args.iterations, verbose=args.verbose,
                            weights=None if weights is None else weights[k],
                            **_pdl_arguments(args))
               for k in solve]
    recon = np.array(observed_nda, dtype=np.float64)
    execution, took = [], datetime.timedelta(seconds=0)
    if solvers:
        batch = PrimalDualLinearBatch(solvers)
        batch.run()
        execution = batch.get_execution()
        for k, solver in zip(solve, solvers):
            recon[k] = solver.get_x().reshape(*observed_nda.shape[1:])
        took = batch.get_computational_time()
    print("%s alpha=%g slice-wise: %d iterations in %s (%d slices stacked, "
          "%d copied through, %d sequential)" % (
              args.reconstruction_type, args.alpha[0], args.iterations, took,
              execution.count("stacked"), len(copy), execution.count("sequential")))
    if args.tolerance is not None and solvers:
        done = [s.get_iterations_done() for s in solvers]
        print("  stopped after %d to %d of %d iterations" % (
            min(done), max(done), args.iterations))
    if x_ref is not None:
        flat = recon.flatten()
        for m in args.measures:
            print("  %s: %.6g" % (
                m, SimilarityMeasures.similarity_measures[m](flat, x_ref)))
    dw.DataWriter(recon, args.result, info).write_data()
    return 0


def build_parser():
    ap = argparse.ArgumentParser(
        description="Run TK0L2/TK1L2/TVL2/HuberL2/TGVL2 deconvolution on an MI355X")
    ap.add_argument("--observation", required=True)
    ap.add_argument("--result", required=True)
    ap.add_argument("--reference", required=False)
    ap.add_argument("--measures", nargs="+",
                    default=["PSNR", "RMSE", "SSIM", "NCC", "NMI"],
                    choices=sorted(SimilarityMeasures.similarity_measures))
    ap.add_argument("--blur", type=float, default=1.2,
                    help="standard deviation of the Gaussian blur; ignored when --psf "
                         "is given")
    ap.add_argument("--psf", default=None, metavar="FILE",
                    help="--solver PDL: the point spread function (.npy, .nii, .png, "
                         ".mat) in the place of the Gaussian of --blur, which is then "
                         "ignored; taps as they are, as many axes as the observation, "
                         "the adjoint is the exact transpose; not with --upsample or "
                         "--slice-wise")
    ap.add_argument("--reconstruction-type", default="TVL2",
                    choices=["TK0L2", "TK1L2", "TVL2", "HuberL2", "TGVL2"])
    ap.add_argument("--beta", type=float, default=None, metavar="B",
                    help="--solver PDL --reconstruction-type TGVL2: the weight of the "
                         "second-order term |E w|_1 against |grad x - w|_1 (default 2)")
    ap.add_argument("--solver", default="PD", choices=["PD", "ADMM", "PDL"])
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.01])
    ap.add_argument("--rho", type=float, default=0.1)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--iter-max", type=int, default=10)
    ap.add_argument("--minimizer", default="lsmr")
    ap.add_argument("--data-loss", default="linear")
    ap.add_argument("--data-loss-scale", type=float, default=1.)
    ap.add_argument("--background", type=float, default=None, metavar="B",
                    help="--solver PDL --data-loss kl: a known constant background "
                         ">= 0 in the observation's units (dark current, scatter): "
                         "the counts are Poisson with mean A x + B")
    ap.add_argument("--L2", type=float, default=8,
                    help="--solver PD: the bound of the operator norm its steps come "
                         "from.  Not used by --solver PDL, TGVL2 included: there the steps "
                         "come from the bound of the operator norms")
    ap.add_argument("--dtype", default="float32",
                    choices=["float32", "float64"])
    ap.add_argument("--verbose", type=int, default=0)
    ap.add_argument("--isotropic", action="store_true",
                    help="primal-dual TVL2 / HuberL2: the isotropic TV / Huber "
                         "norm (the one ADMM minimises) instead of the sum over "
                         "the gradient's components")
    ap.add_argument("--observe-every", type=int, default=None, metavar="K",
                    help="evaluate the measures on the device every K "
                         "iterations (and at the last) instead of on a host "
                         "copy of every iterate")
    wgroup = ap.add_mutually_exclusive_group()
    wgroup.add_argument("--mask", default=None, metavar="FILE",
                        help="--solver PDL: image of the observation's shape, voxels "
                             "> 0 count in the data term (weight 1), the rest do not "
                             "and are inpainted by the regulariser")
    wgroup.add_argument("--weights", default=None, metavar="FILE",
                        help="--solver PDL: image of the observation's shape, "
                             "per-voxel weights of the data term, finite and >= 0")
    ap.add_argument("--nonnegative", action="store_true",
                    help="--solver PDL: x >= 0 as an exact projection in every "
                         "iteration")
    ap.add_argument("--result-dir", default=None, metavar="DIR",
                    help="--solver PDL: the --alpha values run as one sweep "
                         "(PrimalDualLinearSweep, stacked launches); every member's "
                         "result as <stem>_alpha<value><ext> and the sweep's "
                         "parameters and measures as sweep.npz in DIR")
    ap.add_argument("--slice-wise", action="store_true",
                    help="--solver PDL: treat a 3-D observation as shape[0] "
                         "independent 2-D images under the 2-D Gaussian of --blur, each "
                         "scaled by its own maximum, and run them stacked "
                         "(PrimalDualLinearBatch)")
    ap.add_argument("--upsample", type=int, nargs="+", default=None, metavar="F",
                    help="--solver PDL: super-resolution -- the observation is the "
                         "blurred fine image with every F-th sample kept, one factor "
                         "per ARRAY axis; the result has shape obs.shape * F")
    ap.add_argument("--sample-offset", type=int, nargs="+", default=None, metavar="O",
                    help="with --upsample: the first kept sample along every array "
                         "axis, 0 <= O < F (default: zeros)")
    ap.add_argument("--tolerance", type=float, default=None, metavar="T",
                    help="--solver PD or PDL, TVL2 / HuberL2: stop once the relative change "
                         "of the primal and of the dual iterate in one iteration is "
                         "<= T (default: run all --iterations)")
    ap.add_argument("--check-every", type=int, default=10, metavar="K",
                    help="with --tolerance: evaluate the change every K iterations "
                         "and at the last")
    return ap


def parse_args(argv=None, ap=None):
    """The checked arguments; a combination that is not taken is a parser error."""
    ap = ap or build_parser()
    args = ap.parse_args(argv)
    tgv = args.reconstruction_type == "TGVL2"
    if tgv:
        if args.solver != "PDL":
            ap.error("--reconstruction-type TGVL2 is a form of --solver PDL "
                     "(TGVPrimalDualLinearSolver), not of --solver %s" % args.solver)
        if args.result_dir is not None or args.slice_wise:
            ap.error("--reconstruction-type TGVL2 does not take %s yet: the stacked "
                     "TGV forms (nsol_amd/tgv_linear_stack.py) are reachable through "
                     "the API only; several --alpha loop" %
                     ("--result-dir" if args.result_dir is not None else "--slice-wise"))
        if args.beta is None:
            args.beta = 2.0
        if not (np.isfinite(args.beta) and args.beta > 0):
            ap.error("--beta must be positive")
    elif args.beta is not None:
        ap.error("--beta goes with --reconstruction-type TGVL2")
    primal_dual = args.solver in ("PD", "PDL") and \
        args.reconstruction_type in ("TVL2", "HuberL2", "TGVL2")
    linear = args.solver == "PDL"
    if linear and not primal_dual:
        ap.error("--solver PDL applies to --reconstruction-type TVL2, HuberL2 or TGVL2")
    if linear and args.data_loss not in ("linear", "ell2", "ell1", "kl"):
        ap.error("--solver PDL takes --data-loss linear (the l2 data term), ell1 or kl "
                 "(Poisson counts), not '%s'" % args.data_loss)
    if args.background is not None:
        if not (linear and args.data_loss == "kl"):
            ap.error("--background goes with --solver PDL --data-loss kl")
        if not (np.isfinite(args.background) and args.background >= 0):
            ap.error("--background must be a finite number >= 0")
    else:
        args.background = 0.
    if args.nonnegative and not linear:
        ap.error("--nonnegative is an option of --solver PDL")
    if args.tolerance is not None and not primal_dual:
        ap.error("--tolerance is the stopping rule of the primal-dual solvers "
                 "(--solver PD or PDL with TVL2 or HuberL2)")
    if args.tolerance is not None and not args.tolerance >= 0:
        ap.error("--tolerance must be >= 0")
    if args.check_every < 1:
        ap.error("--check-every must be >= 1")
    if (args.mask is not None or args.weights is not None) and not linear:
        ap.error("--mask / --weights are options of run_denoising: the weighted "
                 "data term is a prox of the denoising problem, while "
                 "deconvolution with --solver %s solves a linear least-squares "
                 "problem per step (prox_linear_least_squares), where a mask belongs "
                 "in the operator A -- or use --solver PDL" % args.solver)

    if (args.result_dir is not None or args.slice_wise) and not linear:
        ap.error("--result-dir and --slice-wise are options of --solver PDL, whose "
                 "members run stacked (--solver %s loops over --alpha)" % args.solver)
    if args.slice_wise and args.result_dir is not None:
        ap.error("--result-dir keeps the members of an --alpha sweep; --slice-wise "
                 "writes one reassembled volume to --result")
    if args.slice_wise and len(args.alpha) > 1:
        ap.error("--slice-wise takes a single --alpha")
    if args.slice_wise and args.observe_every is not None:
        ap.error("--slice-wise does not take --observe-every: the measures are "
                 "taken once, on the reassembled volume")

    if args.psf is not None:
        if not linear:
            ap.error("--psf is an option of --solver PDL, which applies the exact "
                     "transpose of the PSF; --solver %s uses A itself for A^T in its "
                     "inner solves, which is right for point-symmetric blurs only -- "
                     "use --solver PDL" % args.solver)
        if args.upsample is not None:
            ap.error("--psf cannot be combined with --upsample: the sampled operator "
                     "takes separable taps only (a dense form is not provided)")
        if args.slice_wise:
            ap.error("--psf does not go with --slice-wise: the PSF has the "
                     "observation's number of axes, the slices one fewer")
    if args.sample_offset is not None and args.upsample is None:
        ap.error("--sample-offset belongs to --upsample")
    if args.upsample is not None:
        if not linear:
            ap.error("--upsample is an option of --solver PDL: the other solvers' "
                     "native paths assume an observation on the result's own grid "
                     "(b.size == x.size)")
        if args.slice_wise:
            ap.error("--upsample does not go with --slice-wise: the stacked batch "
                     "holds b and x on one grid, and the sampled operator acts on "
                     "the whole volume")
        if args.result_dir is not None:
            ap.error("--upsample does not go with --result-dir: the stacked sweep "
                     "holds b and x on one grid; loop over --alpha without it")
        if min(args.upsample) < 1:
            ap.error("--upsample takes factors >= 1")
        offs = args.sample_offset or [0] * len(args.upsample)
        if len(offs) != len(args.upsample) or \
                any(not 0 <= o < f for o, f in zip(offs, args.upsample)):
            ap.error("--sample-offset takes one offset per --upsample factor with "
                     "0 <= O < F")
    return args


def main(argv=None):
    ap = build_parser()
    args = parse_args(argv, ap)
    linear = args.solver == "PDL"

    reader = dr.DataReader(args.observation)
    reader.read_data()
    observed_nda = reader.get_data()
    info = reader.get_image_sitk()
    spacing = np.ones(observed_nda.ndim) if info is None \
        else np.array(info.GetSpacing())
    result_shape = observed_nda.shape
    if args.upsample is not None:
        if len(args.upsample) != observed_nda.ndim:
            ap.error("--upsample takes one factor per axis of the observation (%d), "
                     "not %d" % (observed_nda.ndim, len(args.upsample)))
        result_shape, fine_spacing = fine_grid(observed_nda.shape, spacing,
                                               args.upsample)
        if info is not None:       # the result is written on the fine grid
            info = dr.ImageInfo(fine_spacing, info.header)
    x_ref = None
    if args.reference is not None:
        ref_reader = dr.DataReader(args.reference)
        ref_reader.read_data()
        x_ref = ref_reader.get_data()
        if args.upsample is not None and x_ref.shape != tuple(result_shape):
            ap.error("--reference has shape %s; with --upsample it has the result's, "
                     "%s" % (x_ref.shape, tuple(result_shape)))
        x_ref = x_ref.flatten()
    weights = None
    if linear:
        try:
            weights = read_weights(args, observed_nda.shape)
        except ValueError as e:
            ap.error(str(e))
    psf = None
    if args.psf is not None:
        psf_reader = dr.DataReader(args.psf)
        psf_reader.read_data()
        try:
            psf = checked_psf(psf_reader.get_data(), observed_nda.ndim)
        except ValueError as e:
            ap.error("--psf: %s" % e)
    if args.slice_wise:
        if observed_nda.ndim != 3:
            ap.error("--slice-wise needs a 3-D observation, not %d-D" %
                     observed_nda.ndim)
        return run_slice_wise(args, observed_nda, spacing, x_ref, info, weights)
    if args.result_dir is not None:
        return run_sweep(args, observed_nda, spacing, x_ref, info, weights, psf)
    # (without --upsample the call is what it was)
    extra = {} if args.upsample is None else dict(upsample=args.upsample,
                                                  sample_offset=args.sample_offset)
    if args.reconstruction_type == "TGVL2":
        extra["beta"] = args.beta
    extra.update(_background(args.background))
    if psf is not None:
        extra["psf"] = psf
    for alpha in args.alpha:
        solver = build_solver(
            observed_nda, spacing, args.blur, args.reconstruction_type,
            args.solver, alpha, args.iterations, args.iter_max, args.rho,
            args.minimizer, args.data_loss, args.data_loss_scale, args.L2,
            args.verbose, np.dtype(args.dtype).type, isotropic=args.isotropic,
            tolerance=args.tolerance, check_every=args.check_every, weights=weights,
            pdl_data_loss=_pdl_data_loss(args),
            nonnegative=args.nonnegative, **extra)
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
        recon = np.array(solver.get_x().reshape(*result_shape))
        print("%s alpha=%g: %s" % (args.reconstruction_type, alpha,
                                   solver.get_computational_time()))
        if args.tolerance is not None:
            print_stop(solver, args.iterations)
        if obs is not None:
            obs.compute_measures()
            for m, vals in obs.get_measures().items():
                print("  %s: %.6g -> %.6g" % (m, vals[0], last_observed(vals)))
        dw.DataWriter(recon, args.result, info).write_data()
    return 0


if __name__ == "__main__":
    sys.exit(main())
