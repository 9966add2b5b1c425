// Evaluation measures beyond the pair sums of nsol_ops.hip (reference
// similarity_measures.py:122-277): SSIM, the range pass that fixes histogram
// edges, and the 1-D / joint histograms behind the entropies, MI and NMI.
//
// SSIM (skimage compare_ssim with a box window) is one pass: x and y are read
// once (plus halo), the five local moments x, y, x^2, y^2, xy live in LDS and
// registers only, and only the per-workgroup sums of the SSIM map leave the
// chip.  2-D / 3-D: an xy tile of both inputs in LDS, box sums along x, then y,
// then a z-march that keeps the last WZ planes' sums in registers.  1-D: chunks
// of the line in LDS.  Everything after the load is float64 in the order of the
// published algorithm, so the float32 and float64 instantiations see identical
// values.
//
// Histograms: a privatised uint32 histogram in LDS per workgroup, merged with
// integer atomics (order-free, deterministic); grids above kLdsBins bins count
// straight into global memory.  A wave whose active lanes all fall into one bin
// adds the lane count once.
#include "nsol_common.hpp"

using namespace nsol;

namespace {

// ------------------------------------------------------------------ SSIM ----
constexpr int kSsimTx = 16;             // output columns of a tile
constexpr int kSsimTy = 16;             // output rows of a tile (kSsimTx*kSsimTy = kBlock)
constexpr int kSsimZc = 64;             // output planes of one z-march
constexpr int kSsim1dChunk = 1024;      // outputs of one 1-D chunk (4 per thread)
constexpr int kSsimMaxParts = 8192;     // workgroups (and partial sums) at most

static_assert(kSsimTx * kSsimTy == kBlock, "one output per thread");

struct SsimConst {
  double C1, C2, cov_norm, inv_np;      // inv_np = 1 / (window volume)
};

// skimage _structural_similarity.py: moments -> S, in the reference's order
__device__ __forceinline__ double ssim_value(double sx, double sy, double sxx,
                                             double syy, double sxy,
                                             const SsimConst &k) {
  const double ux = sx * k.inv_np, uy = sy * k.inv_np;
  const double uxx = sxx * k.inv_np, uyy = syy * k.inv_np, uxy = sxy * k.inv_np;
  const double vx = k.cov_norm * (uxx - ux * ux);
  const double vy = k.cov_norm * (uyy - uy * uy);
  const double vxy = k.cov_norm * (uxy - ux * uy);
  const double A1 = 2.0 * ux * uy + k.C1, A2 = 2.0 * vxy + k.C2;
  const double B1 = ux * ux + uy * uy + k.C1, B2 = vx + vy + k.C2;
  const double D = B1 * B2;
  return (A1 * A2) / D;
}

// fixed-order block sum of one double per thread -> part[blockIdx.x]
__device__ __forceinline__ void block_sum_store(double v, double *part) {
  __shared__ double s[kBlock / kWave];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (lane == 0) s[wv] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = s[0];
    for (int k = 1; k < kBlock / kWave; ++k) t += s[k];
    part[blockIdx.x] = t;
  }
}

// fixed-order sum of nparts partials: thread t sums t, t+kBlock, ..., then the
// block sum of those
__global__ __launch_bounds__(kBlock) void k_sum_parts(const double *part, int nparts,
                                                      double *result) {
  double v = 0.0;
  for (int k = threadIdx.x; k < nparts; k += kBlock) v += part[k];
  __shared__ double s[kBlock / kWave];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (lane == 0) s[wv] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = s[0];
    for (int k = 1; k < kBlock / kWave; ++k) t += s[k];
    result[0] = t;
  }
}

// 2-D (WZ = 1) and 3-D (WZ = W) volumes [nz][ny][nx]; outputs are the valid
// windows, (oz, oy, ox) = (nz - WZ + 1, ny - W + 1, nx - W + 1).  Work item =
// (xy tile, z chunk); workgroup b takes items b, b + gridDim.x, ... in order.
template <typename T, int W, int WZ>
__global__ __launch_bounds__(kBlock) void k_ssim_tile(
    const T *__restrict__ x, const T *__restrict__ y, int64_t nz, int64_t ny,
    int64_t nx, int64_t tiles_x, int64_t tiles_y, int64_t zchunks, SsimConst k,
    double *part) {
  constexpr int LX = kSsimTx + W - 1, LY = kSsimTy + W - 1;
  __shared__ double in[5][LY][LX];          // x, y, x^2, y^2, xy of one plane
  __shared__ double rs[5][LY][kSsimTx];     // their box sums along x
  const int tx = threadIdx.x % kSsimTx, ty = threadIdx.x / kSsimTx;
  const int64_t ox = nx - W + 1, oy = ny - W + 1, oz = nz - WZ + 1;
  const int64_t items = tiles_x * tiles_y * zchunks;
  double acc = 0.0;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t zc = it % zchunks, tile = it / zchunks;
    const int64_t x0 = (tile % tiles_x) * kSsimTx, y0 = (tile / tiles_x) * kSsimTy;
    const int64_t z0 = zc * kSsimZc;
    int64_t z1 = z0 + kSsimZc;                        // output planes [z0, z1)
    if (z1 > oz) z1 = oz;
    const bool mine = (x0 + tx < ox) && (y0 + ty < oy);
    double ring[5][WZ] = {};                          // plane sums, oldest first
    for (int64_t zi = z0; zi < z1 + WZ - 1; ++zi) {
      const T *xp = x + zi * ny * nx, *yp = y + zi * ny * nx;
      __syncthreads();                                // previous plane consumed
      for (int e = threadIdx.x; e < LY * LX; e += kBlock) {
        const int r = e / LX, c = e % LX;
        const int64_t gy = y0 + r, gx = x0 + c;
        double a = 0.0, b = 0.0;
        if (gy < ny && gx < nx) {
          a = (double)xp[gy * nx + gx];
          b = (double)yp[gy * nx + gx];
        }
        in[0][r][c] = a; in[1][r][c] = b;
        in[2][r][c] = a * a; in[3][r][c] = b * b; in[4][r][c] = a * b;
      }
      __syncthreads();
      for (int e = threadIdx.x; e < LY * kSsimTx; e += kBlock) {
        const int r = e / kSsimTx, c = e % kSsimTx;
#pragma unroll
        for (int m = 0; m < 5; ++m) {
          double s = in[m][r][c];
#pragma unroll
          for (int j = 1; j < W; ++j) s += in[m][r][c + j];
          rs[m][r][c] = s;
        }
      }
      __syncthreads();
      double p[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        double s = rs[m][ty][tx];
#pragma unroll
        for (int j = 1; j < W; ++j) s += rs[m][ty + j][tx];
        p[m] = s;
      }
#pragma unroll
      for (int m = 0; m < 5; ++m) {
#pragma unroll
        for (int j = 0; j + 1 < WZ; ++j) ring[m][j] = ring[m][j + 1];
        ring[m][WZ - 1] = p[m];
      }
      if (mine && zi >= z0 + WZ - 1) {                // output plane zi - WZ + 1
        double q[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
          double s = ring[m][0];
#pragma unroll
          for (int j = 1; j < WZ; ++j) s += ring[m][j];
          q[m] = s;
        }
        acc += ssim_value(q[0], q[1], q[2], q[3], q[4], k);
      }
    }
  }
  __syncthreads();
  block_sum_store(acc, part);
}

// 1-D line of n elements: outputs 0 .. n - W, chunk c covers outputs
// [c*kSsim1dChunk, (c+1)*kSsim1dChunk); workgroup b takes chunks b, b + gridDim.x, ...
template <typename T, int W>
__global__ __launch_bounds__(kBlock) void k_ssim_line(const T *__restrict__ x,
                                                      const T *__restrict__ y,
                                                      int64_t n, int64_t chunks,
                                                      SsimConst k, double *part) {
  constexpr int L = kSsim1dChunk + W - 1;
  __shared__ double lx[L], ly[L];
  const int64_t on = n - W + 1;
  double acc = 0.0;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t base = c * kSsim1dChunk;
    __syncthreads();
    for (int e = threadIdx.x; e < L; e += kBlock) {
      const int64_t g = base + e;
      lx[e] = g < n ? (double)x[g] : 0.0;
      ly[e] = g < n ? (double)y[g] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSsim1dChunk / kBlock; ++r) {
      const int o = threadIdx.x + r * kBlock;
      if (base + o < on) {
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const double a = lx[o + j], b = ly[o + j];
          if (j == 0) {
            sx = a; sy = b; sxx = a * a; syy = b * b; sxy = a * b;
          } else {
            sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
          }
        }
        acc += ssim_value(sx, sy, sxx, syy, sxy, k);
      }
    }
  }
  __syncthreads();
  block_sum_store(acc, part);
}

template <typename T, int W>
int ssim_launch(const T *x, const T *y, int ndim, int64_t nz, int64_t ny, int64_t nx,
                const SsimConst &k, double *result, double *ws, hipStream_t st) {
  int64_t items;
  if (ndim == 1) {
    const int64_t chunks = (nx - W + 1 + kSsim1dChunk - 1) / kSsim1dChunk;
    items = chunks;
    const int g = (int)(items < kSsimMaxParts ? items : kSsimMaxParts);
    hipLaunchKernelGGL((k_ssim_line<T, W>), dim3(g), dim3(kBlock), 0, st, x, y, nx,
                       chunks, k, ws);
    hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(kBlock), 0, st, ws, g, result);
    return launch_status();
  }
  const int64_t tiles_x = (nx - W + 1 + kSsimTx - 1) / kSsimTx;
  const int64_t tiles_y = (ny - W + 1 + kSsimTy - 1) / kSsimTy;
  const int64_t oz = ndim == 3 ? nz - W + 1 : 1;
  const int64_t zchunks = (oz + kSsimZc - 1) / kSsimZc;
  items = tiles_x * tiles_y * zchunks;
  const int g = (int)(items < kSsimMaxParts ? items : kSsimMaxParts);
  if (ndim == 3)
    hipLaunchKernelGGL((k_ssim_tile<T, W, W>), dim3(g), dim3(kBlock), 0, st, x, y, nz,
                       ny, nx, tiles_x, tiles_y, zchunks, k, ws);
  else
    hipLaunchKernelGGL((k_ssim_tile<T, W, 1>), dim3(g), dim3(kBlock), 0, st, x, y, nz,
                       ny, nx, tiles_x, tiles_y, zchunks, k, ws);
  hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(kBlock), 0, st, ws, g, result);
  return launch_status();
}

template <typename T>
int ssim_impl(const T *x, const T *y, int ndim, int64_t nz, int64_t ny, int64_t nx,
              int win, double C1, double C2, double cov_norm, double *result,
              double *ws, void *stream) {
  static_assert(kSsimMaxParts <= kReducePartials, "workspace");
  if (!x || !y || !result || !ws || !geom_ok(ndim, nz, ny, nx)) return NSOL_EINVAL;
  if (nx < win || (ndim >= 2 && ny < win) || (ndim == 3 && nz < win))
    return NSOL_EINVAL;
  double np_ = 1.0;
  for (int a = 0; a < ndim; ++a) np_ *= (double)win;
  const SsimConst k{C1, C2, cov_norm, 1.0 / np_};
  const hipStream_t st = as_stream(stream);
  switch (win) {
    case 3: return ssim_launch<T, 3>(x, y, ndim, nz, ny, nx, k, result, ws, st);
    case 5: return ssim_launch<T, 5>(x, y, ndim, nz, ny, nx, k, result, ws, st);
    case 7: return ssim_launch<T, 7>(x, y, ndim, nz, ny, nx, k, result, ws, st);
    case 9: return ssim_launch<T, 9>(x, y, ndim, nz, ny, nx, k, result, ws, st);
    case 11: return ssim_launch<T, 11>(x, y, ndim, nz, ny, nx, k, result, ws, st);
    default: return NSOL_EINVAL;
  }
}

// ----------------------------------------------------------------- range ----
// result: { min x, max x, min y, max y, number of non-finite values in x and y }
constexpr int kRangeBlocks = 2048;

template <typename T>
__global__ __launch_bounds__(kBlock) void k_pair_range(const T *__restrict__ x,
                                                       const T *__restrict__ y,
                                                       int64_t n, double *ws) {
  double v[5] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double a = (double)x[i], b = (double)y[i];
    if (isfinite(a)) { v[0] = fmin(v[0], a); v[1] = fmax(v[1], a); } else v[4] += 1.0;
    if (isfinite(b)) { v[2] = fmin(v[2], b); v[3] = fmax(v[3], b); } else v[4] += 1.0;
  }
  __shared__ double s[5][kBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    double t = v[m];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const double o = __shfl_down(t, off, kWave);
      t = (m == 4) ? t + o : ((m & 1) ? fmax(t, o) : fmin(t, o));
    }
    if (lane == 0) s[m][wv] = t;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const int m = threadIdx.x;
    double t = s[m][0];
    for (int j = 1; j < kBlock / kWave; ++j)
      t = (m == 4) ? t + s[m][j] : ((m & 1) ? fmax(t, s[m][j]) : fmin(t, s[m][j]));
    ws[(int64_t)m * kRangeBlocks + blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(kBlock) void k_pair_range_final(const double *ws,
                                                             int nparts,
                                                             double *result) {
  if (threadIdx.x < 5) {
    const int m = threadIdx.x;
    double t = ws[(int64_t)m * kRangeBlocks];
    for (int j = 1; j < nparts; ++j) {
      const double o = ws[(int64_t)m * kRangeBlocks + j];
      t = (m == 4) ? t + o : ((m & 1) ? fmax(t, o) : fmin(t, o));
    }
    result[m] = t;
  }
}

template <typename T>
int pair_range_impl(const T *x, const T *y, int64_t n, double *result, double *ws,
                    void *stream) {
  static_assert(5 * kRangeBlocks <= kReducePartials, "workspace");
  if (n < 1 || !x || !y || !result || !ws) return NSOL_EINVAL;
  int64_t g = (n + kBlock - 1) / kBlock;
  if (g > kRangeBlocks) g = kRangeBlocks;
  hipLaunchKernelGGL(k_pair_range<T>, dim3((int)g), dim3(kBlock), 0, as_stream(stream),
                     x, y, n, ws);
  hipLaunchKernelGGL(k_pair_range_final, dim3(1), dim3(kBlock), 0, as_stream(stream), ws,
                     (int)g, result);
  return launch_status();
}

// ------------------------------------------------------------ histograms ----
constexpr int kLdsBins = 16384;         // 64 KiB of uint32 counts
constexpr int kHistBlocks = 2048;
constexpr int64_t kHistPerBlock = (int64_t)1 << 30;  // keeps a uint32 count from wrapping

// NumPy's bin of v for edges e[0..nb] (increasing): the last i with e[i] <= v,
// v == e[nb] in the last bin (np.histogram's corrected guess; histogramdd's
// searchsorted(..., 'right') - 1).  v lies in [e[0], e[nb]].
template <typename T>
__device__ __forceinline__ int bin_of(T v, const T *__restrict__ e, int nb, T scale) {
  T f = (v - e[0]) * scale;
  f = f > T(0) ? f : T(0);
  f = f < T(nb - 1) ? f : T(nb - 1);
  int i = (int)f;
  while (i > 0 && v < e[i]) --i;
  while (i < nb - 1 && v >= e[i + 1]) ++i;
  return i;
}

// adds one per active lane to cnt[b]; a wave whose active lanes share one bin
// adds their number once
template <typename C>
__device__ __forceinline__ void count_bin(C *cnt, int b) {
  const uint64_t active = __ballot(1);
  const int b0 = __builtin_amdgcn_readfirstlane(b);
  const uint64_t same = __ballot(b == b0);
  if (same == active) {
    const int lane = threadIdx.x & (kWave - 1);
    if ((active & ((1ull << lane) - 1)) == 0)         // first active lane
      atomicAdd(&cnt[b0], (C)__popcll(active));
  } else {
    atomicAdd(&cnt[b], (C)1);
  }
}

// joint (by > 0: bin = ix * by + iy) or 1-D (y == nullptr, by = 1) histogram.
// LDS: privatised uint32 bins merged into counts; !LDS: straight into counts.
template <typename T, bool LDS>
__global__ __launch_bounds__(kBlock) void k_hist(const T *__restrict__ x,
                                                 const T *__restrict__ y, int64_t n,
                                                 const T *__restrict__ ex, int bx, T sx,
                                                 const T *__restrict__ ey, int by, T sy,
                                                 unsigned long long *counts) {
  extern __shared__ unsigned int h[];
  const int nbins = bx * by;
  if (LDS) {
    for (int b = threadIdx.x; b < nbins; b += kBlock) h[b] = 0u;
    __syncthreads();
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int b = bin_of(x[i], ex, bx, sx);
    if (y) b = b * by + bin_of(y[i], ey, by, sy);
    if (LDS)
      count_bin(h, b);
    else
      count_bin(counts, b);
  }
  if (LDS) {
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += kBlock) {
      const unsigned int c = h[b];
      if (c) atomicAdd(&counts[b], (unsigned long long)c);
    }
  }
}

template <typename T>
int hist_impl(const T *x, const T *y, int64_t n, const T *ex, int bx, double gx,
              const T *ey, int by, double gy, uint64_t *counts, void *stream) {
  if (n < 1 || !x || !ex || bx < 1 || by < 1 || !counts) return NSOL_EINVAL;
  if (y && !ey) return NSOL_EINVAL;
  if ((int64_t)bx * by > (int64_t)1 << 30) return NSOL_EINVAL;
  const hipStream_t st = as_stream(stream);
  const int64_t nbins = (int64_t)bx * by;
  hipError_t e = hipMemsetAsync(counts, 0, nbins * sizeof(uint64_t), st);
  if (e != hipSuccess) return (int)e;
  int64_t g = (n + kBlock - 1) / kBlock;
  if (g > kHistBlocks) g = kHistBlocks;
  if (g < (n + kHistPerBlock - 1) / kHistPerBlock) g = (n + kHistPerBlock - 1) / kHistPerBlock;
  unsigned long long *c = reinterpret_cast<unsigned long long *>(counts);
  if (nbins <= kLdsBins)
    hipLaunchKernelGGL((k_hist<T, true>), dim3((unsigned)g), dim3(kBlock),
                       nbins * sizeof(unsigned int), st, x, y, n, ex, bx, (T)gx, ey,
                       y ? by : 1, (T)gy, c);
  else
    hipLaunchKernelGGL((k_hist<T, false>), dim3((unsigned)g), dim3(kBlock), 0, st, x, y,
                       n, ex, bx, (T)gx, ey, y ? by : 1, (T)gy, c);
  return launch_status();
}

}  // namespace

// ================================ C ABI ====================================
extern "C" {

#define NSOL_DEF_MEASURES(T, SUF)                                                \
  int nsol_ssim_##SUF(const T *x, const T *y, int ndim, int64_t nz, int64_t ny,  \
                      int64_t nx, int win, double C1, double C2,                 \
                      double cov_norm, double *result, double *ws, void *s) {    \
    return ssim_impl<T>(x, y, ndim, nz, ny, nx, win, C1, C2, cov_norm, result,   \
                        ws, s);                                                  \
  }                                                                              \
  int nsol_pair_range_##SUF(const T *x, const T *y, int64_t n, double *result,   \
                            double *ws, void *s) {                               \
    return pair_range_impl<T>(x, y, n, result, ws, s);                           \
  }                                                                              \
  int nsol_hist2d_##SUF(const T *x, const T *y, int64_t n, const T *xedges,      \
                        int bx, double xscale, const T *yedges, int by,          \
                        double yscale, uint64_t *counts, void *s) {              \
    if (!y) return NSOL_EINVAL;                                                  \
    return hist_impl<T>(x, y, n, xedges, bx, xscale, yedges, by, yscale, counts, \
                        s);                                                      \
  }                                                                              \
  int nsol_hist1d_##SUF(const T *x, int64_t n, const T *edges, int bins,         \
                        double scale, uint64_t *counts, void *s) {               \
    return hist_impl<T>(x, nullptr, n, edges, bins, scale, nullptr, 1, 0.0,      \
                        counts, s);                                              \
  }

NSOL_DEF_MEASURES(float, f32)
NSOL_DEF_MEASURES(double, f64)

}  // extern "C"
