// The float64 reduction of the stopping rule's four sums {sum dx^2, sum x^2,
// sum dp^2, sum p^2} (nsol_pdc.hip, nsol_pdm.hip; the scheme of nsol_observe.hip):
// wave shuffle, one partial per workgroup and sum in a workspace, then a closing
// workgroup that adds the partials in a fixed order.  No floating-point atomics: the
// same input gives the same bits on every run.
#pragma once

#include "nsol_common.hpp"

namespace nsol {

constexpr int kPdSums = 4;
constexpr int kPdSumWaves = kBlock / kWave;

__device__ __forceinline__ double pd_wave_sum(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;
}

// the workgroup's partial of every sum into ws[(row * 4 + k) * nparts + blockIdx.x],
// row the grid row of a stacked launch (0 where the grid has one); called by all
// threads of the workgroup
__device__ __forceinline__ void pd_block_store(const double (&a)[kPdSums],
                                               double *__restrict__ ws, int nparts,
                                               int64_t row) {
  __shared__ double s[kPdSums][kPdSumWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kPdSums; ++k) {
    const double v = pd_wave_sum(a[k]);
    if (lane == 0) s[k][wv] = v;
  }
  __syncthreads();
  if (threadIdx.x < kPdSums) {
    const int k = threadIdx.x;
    double t = s[k][0];
    for (int w = 1; w < kPdSumWaves; ++w) t += s[k][w];
    ws[(row * kPdSums + k) * nparts + blockIdx.x] = t;
  }
}

// part[0 .. nparts) added in a fixed order by one workgroup of kBlock threads, all of
// which call; thread 0 returns the sum (the others return 0)
__device__ __forceinline__ double pd_parts_sum(const double *__restrict__ part,
                                               int nparts) {
  __shared__ double s[kPdSumWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  double v = 0.0;
  for (int j = threadIdx.x; j < nparts; j += kBlock) v += part[j];
  v = pd_wave_sum(v);
  if (lane == 0) s[wv] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kPdSumWaves; ++w) t += s[w];
  __syncthreads();     // (s is free for the caller's next sum)
  return t;
}

}  // namespace nsol
