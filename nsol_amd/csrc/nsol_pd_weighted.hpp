// The prox of the WEIGHTED data term, lambda/2 sum w_i (x_i - b_i)^2 or
// lambda sum w_i |x_i - b_i| with per-voxel weights w_i >= 0: the one device helper
// that the stand-alone kernels (nsol_prox_ell*_weighted_*) and the fused kernels
// k_pd_w / k_pd_w_iso (nsol_pdw.hip) go through, so that every form gives the same
// bits, as dual_project does for the isotropic dual step.
#pragma once

#include "nsol_common.hpp"

namespace nsol {

// t = tl * w, then
//   l2: (u + t * bt) / (1 + t)       an IEEE division in float32 AND float64: the
//                                    denominator differs per voxel, so the host-side
//                                    reciprocal of prox_ell2<float> does not apply
//   l1: prox_ell1(u, bt, t)
// w == 0 returns u itself, whatever bt holds (NaN and +-inf included: masked-out
// voxels of real files often hold garbage) -- a select on w, not a product with 0.
// float64 with w == 1: tl * 1 = tl and 1 + tl is prox_den<double>(tl), the bits of
// prox_data.
template <typename T>
__device__ __forceinline__ T prox_data_w(T u, T bt, T w, T tl, bool l1) {
  const T t = tl * w;
  T r;
  if (l1) {
    pin(u);            // a real (uniform) branch, as in prox_data
    r = prox_ell1(u, bt, t);
  } else {
    pin(u);
    r = (u + t * bt) / (T(1) + t);
  }
  return w == T(0) ? u : r;
}

}  // namespace nsol
