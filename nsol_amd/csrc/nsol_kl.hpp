// The Poisson (Kullback-Leibler) data term,  D(u; bt) = sum_i w_i ((u_i + g) - bt_i log(u_i + g)),
// the negative Poisson log-likelihood up to a constant: the two closed-form proxes that
// every kernel with this term goes through -- k_pdl_dual_data_kl and its stacked twin
// (nsol_pdl.hip, nsol_pdls.hip), k_prox_kl (nsol_pdw.hip) and the kKl form of
// tgv_primal_body (nsol_tgv.hip) -- so that all forms give the same bits, as prox_data_w
// and dual_project do for their families.  Restated operation for operation in
// nsol_amd/vector_numpy.py (kl_dual_prox, prox_kl).
//
// Each prox is the root of a quadratic, written in two branches that are the same number:
// each avoids the cancellation the other has (sqrt(d^2 + ...) - |d| for large |d|), which
// costs the one-line forms every digit in float32.  The divisions and square roots are
// IEEE ones in both types.
#pragma once

#include "nsol_common.hpp"

namespace nsol {

// The prox of sigma F* for F = lambda D at v (the caller has added sigma g to v where
// there is a background g): with c = lambda w, d = v - c and s = sqrt(d^2 + 4 sigma c bt),
//   d >  0: c - (2 sigma c bt) / (d + s)
//   d <= 0: c + (d - s) / 2
// always <= c; bt == 0 gives min(v, c).  w == 0: 0 exactly, whatever bt holds there (NaN
// included) -- a select on w, as in k_pdl_dual_data.
template <typename T>
__device__ __forceinline__ T kl_dual_prox(T v, T bt, T w, T sigma, T lmbda) {
  const T c = lmbda * w;
  const T d = v - c;
  const T scb = (sigma * c) * bt;
  const T s = t_sqrt(d * d + T(4) * scb);
  const T r = d > T(0) ? c - (T(2) * scb) / (d + s) : c + T(0.5) * (d - s);
  return w == T(0) ? T(0) : r;
}

// The prox of tl w D (no background) at u: with t = tl w, e = u - t and
// s = sqrt(e^2 + 4 t bt),
//   e >= 0: (e + s) / 2
//   e <  0: (2 t bt) / (s - e)
// always >= 0; bt == 0 gives max(u - t, 0).  w == 0 returns u itself, whatever bt holds.
template <typename T>
__device__ __forceinline__ T prox_kl(T u, T bt, T w, T tl) {
  const T t = tl * w;
  const T e = u - t;
  const T tb = t * bt;
  const T s = t_sqrt(e * e + T(4) * tb);
  const T r = e >= T(0) ? T(0.5) * (e + s) : (T(2) * tb) / (s - e);
  return w == T(0) ? u : r;
}

}  // namespace nsol
