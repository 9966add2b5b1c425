// The explicit primal step of the iterations whose data term sits behind a linear
// operator A: the one device helper that the fused tiles (k_pd_lin, nsol_pdl.hip;
// k_pdl_stack, nsol_pdls.hip) and the LIN form of k_tgv_primal (nsol_tgv.hip) go
// through, so that every form gives the same bits.
#pragma once

#include "nsol_common.hpp"

namespace nsol {

// LIN: the explicit primal step of the iteration whose data term sits behind a linear
// operator A (k_pd_lin, nsol_pdl.hip): kt = grad^T p as the tile formed it, g = A^T q,
// their sum before the one multiplication by tau, then the projection onto [lo, hi].
template <typename T>
__device__ __forceinline__ T lin_step(T x, T kt, T g, T tau, T lo, T hi) {
  const T u = x - tau * (kt + g);
  const T c = u < lo ? lo : u;
  return c > hi ? hi : c;
}

}  // namespace nsol
