// scipy.ndimage's boundary rule as an index map, shared by the correlation kernels of
// nsol_conv.hip and nsol_convd.hip.
#pragma once

#include "nsol_common.hpp"

namespace nsol {

// index of the sample that position i (possibly outside [0,n)) refers to under
// `mode`; -1 means "zero" (constant mode).
__device__ __forceinline__ int64_t map_index(int64_t i, int64_t n, int mode) {
  if (i >= 0 && i < n) return i;
  switch (mode) {
    case NSOL_MODE_WRAP: {
      int64_t j = i % n;
      return j < 0 ? j + n : j;
    }
    case NSOL_MODE_NEAREST:
      return i < 0 ? 0 : n - 1;
    case NSOL_MODE_REFLECT: {
      const int64_t per = 2 * n;
      int64_t j = i % per;
      if (j < 0) j += per;
      return j < n ? j : per - 1 - j;
    }
    case NSOL_MODE_MIRROR: {
      if (n == 1) return 0;
      const int64_t per = 2 * n - 2;
      int64_t j = i % per;
      if (j < 0) j += per;
      return j < n ? j : per - j;
    }
    default:
      return -1;
  }
}

}  // namespace nsol
