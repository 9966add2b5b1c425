/* nsol_hip_tgv_lin_stack.h -- the member-stacked primal step of TGV behind a linear
 * operator (nsol_tgv.hip, k_tgv_primal_lin_stack; nsol_amd/tgv_linear_stack.py).  Part of
 * libnsol_hip.so's C ABI: nsol_hip.h includes this file, and nsol_amd/_lib.py binds what it
 * declares beside nsol_hip.h's entries, by the same parser.  Conventions (returns,
 * NSOL_EINVAL, -2, streams): nsol_hip.h. */
#ifndef NSOL_HIP_TGV_LIN_STACK_H
#define NSOL_HIP_TGV_LIN_STACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* nsol_tgv_primal_lin_* on `members` (1 ... 65535) stacked problems in ONE launch, member
 * m at blockIdx.z = m, the arrays member-major as above: x, xbar and g at m * n, w, wbar
 * and p at m * ndim * n, q at m * M * n.  g always has a member stride of n: every member
 * has its own A^T r.  tau, theta, lo and hi are shared by value; a member's lambda sits in
 * nsol_pdl_stack_dual_data_*'s update of r and its beta in nsol_tgv_stack_dual_*, so this
 * entry takes no table.
 * nsol_tgv_stack_primal_lin_*: every member's result has the bits of
 *   nsol_tgv_primal_lin_* on that member's arrays (float32 rounds [lo, hi] towards its
 *   inside, as there).  Vector width and access form follow the alignment of every base
 *   and of the member strides in bytes.  Returns as nsol_tgv_primal_lin_*'s, the spans
 *   `members` times as long: 0 at once for an extent of 0; NSOL_EINVAL for a missing
 *   pointer, two spans that overlap, a tau that is not positive and finite, a theta that
 *   is not finite, !(lo <= hi); -2, nothing launched, for members outside 1 ... 65535,
 *   more than 2^31 voxels per member or a shape the stencil grid declines.  Counted by
 *   nsol_tgv_stack_launches, not by nsol_tgv_launches. */
int nsol_tgv_stack_primal_lin_f32(const float *p, const float *q, float *x, float *xbar,
    float *w, float *wbar, const float *g, int members, int ndim, int64_t nz, int64_t ny,
    int64_t nx, double wx, double wy, double wz, double tau, double theta, double lo,
    double hi, void *stream);
int nsol_tgv_stack_primal_lin_f64(const double *p, const double *q, double *x,
    double *xbar, double *w, double *wbar, const double *g, int members, int ndim,
    int64_t nz, int64_t ny, int64_t nx, double wx, double wy, double wz, double tau,
    double theta, double lo, double hi, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSOL_HIP_TGV_LIN_STACK_H */
