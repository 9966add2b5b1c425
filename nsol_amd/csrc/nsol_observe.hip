// Observation of a solver's iterate on the device (nsol_amd/observer.py): the
// sums behind the reduction-type measures of similarity_measures.py and
// prior_measures.py, for the scaled iterate, in one pass and without a copy of
// the iterate to the host.
//
// The host path evaluates the measures on Solver.get_x(): x * x_scale formed in
// the element type (nsol_scale_*), widened to float64.  Here every voxel is
// formed the same way, xs = (double)(x[i] * (T)x_scale); the forward differences
// (k_grad with constant boundaries, D_a = x[i+e_a] * w_a + x[i] * (-w_a)), the
// norms and the Huber term (k_vector_norm_sum with f_scale = 1) are float64 in
// the order the float64 host path uses, so only the order of the sums differs.
//
// One grid-stride pass (four voxels per thread and step, their loads ahead of
// the arithmetic, coordinates advanced with the index instead of divided out) reads each x element once plus its halo (L1 / L2 hits) and y
// once if the pair group is on; every workgroup leaves its 9 partial sums
// in ws, one workgroup sums them in a fixed order into the board row: the same
// bits for the same input.
#include <type_traits>

#include "nsol_common.hpp"

using namespace nsol;

namespace {

constexpr int kObsSums = 9;
constexpr int kObsBlocks = 4096;
constexpr int kObsUnroll = 4;
static_assert(kObsSums * kObsBlocks <= kReducePartials, "workspace");

__device__ __forceinline__ double obs_wave_sum(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;
}

template <typename T>
__device__ __forceinline__ double widen_scaled(T v, T ts) {
  const T p = v * ts;                    // rounded in T, as nsol_scale_* does
  return (double)p;
}

// one voxel: the sums of the groups asked for (c: the voxel, h*: its forward
// neighbours or 0 behind the last one, yv: the reference)
template <typename T>
__device__ __forceinline__ void observe_voxel(double (&a)[kObsSums], bool pair, bool grad,
                                              bool huber, bool sq, int ndim, double c,
                                              double yv,
                                              double ybar, double hx, double hy, double hz,
                                              double wx, double wy, double wz, double gm,
                                              double g2, double two_gm) {
  if (pair) {
    const double d = c - yv, dc = c - ybar;
    a[0] += d * d;
    a[1] += fabs(d);
    a[2] += c;
    a[3] += dc * (yv - ybar);
    a[4] += dc * dc;
  }
  if (grad) {
    const double gx = hx * wx + c * (-wx);
    double n2 = gx * gx;
    if (ndim >= 2) {
      const double gy = hy * wy + c * (-wy);
      n2 = n2 + gy * gy;
    }
    if (ndim >= 3) {
      const double gz = hz * wz + c * (-wz);
      n2 = n2 + gz * gz;
    }
    const double q = sqrt(n2);
    a[5] += q;
    if (huber) {
      // loss_eval(NSOL_LOSS_HUBER, n2, s2 = 1, gamma) / (2 gamma): z = n2 / 1
      // and z * 1 are n2 itself, sqrt(z) is q
      const double rho = (n2 < g2) ? n2 : 2.0 * gm * q - g2;
      a[6] += rho / two_gm;
    }
    a[7] += n2;
  }
  if (sq) a[8] += c * c;
}

// kObsUnroll elements per thread and step, their loads issued before any of
// them is used.  I: the index type of the coordinate arithmetic (32-bit when
// the volume allows); COORD: coordinates are needed (gradient or row pitch),
// else x and y are read at the flat index.
template <typename T, typename Y, typename I, bool COORD>
__global__ __launch_bounds__(kBlock) void k_observe(
    const T *__restrict__ x, T ts, const Y *__restrict__ y, double ybar, int ndim,
    int64_t nz64, int64_t ny64, int64_t nx64, int64_t pitch, double wx, double wy,
    double wz, double gm, int flags, double *__restrict__ ws) {
  const bool pair = flags & NSOL_OBS_PAIR, grad = flags & NSOL_OBS_GRAD,
             sq = flags & NSOL_OBS_SQ, huber = grad && (flags & NSOL_OBS_HUBER);
  const I nz = (I)nz64, ny = (I)ny64, nx = (I)nx64;
  const int64_t n = nz64 * ny64 * nx64;
  const int64_t plane = ny64 * pitch;
  const double g2 = gm * gm, two_gm = 2.0 * gm;
  double a[kObsSums];
#pragma unroll
  for (int k = 0; k < kObsSums; ++k) a[k] = 0.0;
  const int64_t S = (int64_t)gridDim.x * kBlock;
  // coordinates of the flat index j, advanced with j by the grid stride
  // S = (sz * ny + sy) * nx + sx without a division per element
  const int64_t j_first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  I ix = 0, iy = 0, iz = 0, sx = 0, sy = 0, sz = 0;
  if constexpr (COORD) {
    const int64_t srow = S / nx64, row = j_first / nx64;
    sx = (I)(S - srow * nx64);
    sy = (I)(srow % ny64);
    sz = (I)(srow / ny64);
    ix = (I)(j_first - row * nx64);
    iy = (I)(row % ny64);
    iz = (I)(row / ny64);
  }
  for (int64_t j0 = j_first; j0 < n; j0 += S * kObsUnroll) {
    double c[kObsUnroll], yv[kObsUnroll], hx[kObsUnroll], hy[kObsUnroll],
        hz[kObsUnroll];
#pragma unroll
    for (int u = 0; u < kObsUnroll; ++u) {
      const int64_t j = j0 + u * S;
      c[u] = yv[u] = hx[u] = hy[u] = hz[u] = 0.0;
      if (j < n) {
        const int64_t o =
            COORD ? (int64_t)iz * plane + (int64_t)iy * pitch + ix : j;
        c[u] = widen_scaled(x[o], ts);
        if (pair) yv[u] = (double)y[j];
        if (COORD && grad) {
          if (ix + 1 < nx) hx[u] = widen_scaled(x[o + 1], ts);
          if (ndim >= 2 && iy + 1 < ny) hy[u] = widen_scaled(x[o + pitch], ts);
          if (ndim >= 3 && iz + 1 < nz) hz[u] = widen_scaled(x[o + plane], ts);
        }
      }
      if constexpr (COORD) {           // to j + S (sx < nx, sy < ny)
        ix += sx;
        const I carry = ix >= nx ? 1 : 0;
        ix -= carry * nx;
        iy += sy + carry;
        const I wrap = iy >= ny ? 1 : 0;
        iy -= wrap * ny;
        iz += sz + wrap;
      }
    }
#pragma unroll
    for (int u = 0; u < kObsUnroll; ++u) {
      if (j0 + u * S >= n) break;
      observe_voxel<T>(a, pair, COORD && grad, huber, sq, ndim, c[u], yv[u], ybar, hx[u],
                       hy[u], hz[u], wx, wy, wz, gm, g2, two_gm);
    }
  }
  __shared__ double s[kObsSums][kBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kObsSums; ++k) {
    const double v = obs_wave_sum(a[k]);
    if (lane == 0) s[k][wv] = v;
  }
  __syncthreads();
  if (threadIdx.x < kObsSums) {
    const int k = threadIdx.x;
    double t = s[k][0];
    for (int w = 1; w < kBlock / kWave; ++w) t += s[k][w];
    ws[(int64_t)k * kObsBlocks + blockIdx.x] = t;
  }
}

// the partial sums of every group in a fixed order into row[0..8]
__global__ __launch_bounds__(kBlock) void k_observe_final(const double *__restrict__ ws,
                                                          int nparts,
                                                          double *__restrict__ row) {
  __shared__ double s[kBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  for (int k = 0; k < kObsSums; ++k) {
    double v = 0.0;
    for (int j = threadIdx.x; j < nparts; j += kBlock) v += ws[(int64_t)k * kObsBlocks + j];
    v = obs_wave_sum(v);
    if (lane == 0) s[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int w = 0; w < kBlock / kWave; ++w) t += s[w];
      row[k] = t;
    }
    __syncthreads();
  }
}

// out[j] = (double)(x[j] * (T)x_scale) in contiguous order from a (pitched) x
template <typename T>
__global__ __launch_bounds__(kBlock) void k_observe_widen(double *__restrict__ out,
                                                          const T *__restrict__ x, T ts,
                                                          int64_t nrows, int64_t nx,
                                                          int64_t pitch) {
  const int64_t n = nrows * nx;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) {
    const int64_t r = j / nx;
    out[j] = widen_scaled(x[r * pitch + (j - r * nx)], ts);
  }
}

template <typename T>
int observe_impl(const T *x, double x_scale, const void *y, int y_f64, double ybar,
                 int ndim, int64_t nz, int64_t ny, int64_t nx, int64_t pitch,
                 double wx, double wy, double wz, double gm, int flags, double *row,
                 double *ws, void *stream) {
  NSOL_CHECK_GEOM(ndim, nz, ny, nx);
  if (!x || !row || !ws || (flags & ~(NSOL_OBS_PAIR | NSOL_OBS_GRAD | NSOL_OBS_SQ |
                                     NSOL_OBS_HUBER)))
    return NSOL_EINVAL;
  if ((flags & NSOL_OBS_PAIR) && !y) return NSOL_EINVAL;
  if ((flags & NSOL_OBS_GRAD) && !(gm > 0.0)) return NSOL_EINVAL;
  if (pitch <= 0) pitch = nx;
  if (pitch < nx) return NSOL_EINVAL;
  const int64_t n = nz * ny * nx;
  int g = grid_for(n);
  if (g > kObsBlocks) g = kObsBlocks;
  const T ts = (T)x_scale;
  const bool coord = (flags & NSOL_OBS_GRAD) || pitch != nx;
  // (coordinates in 32 bits while z + sz cannot overflow them)
  const bool small = nz + g * (int64_t)kBlock / (nx * ny) + 2 < ((int64_t)1 << 31) &&
                     nx < ((int64_t)1 << 30) && ny < ((int64_t)1 << 30);
  auto launch = [&](auto yp, auto idx, auto crd) {
    using Y = typename std::remove_const<
        typename std::remove_pointer<decltype(yp)>::type>::type;
    using I = decltype(idx);
    constexpr bool C = decltype(crd)::value;
    hipLaunchKernelGGL((k_observe<T, Y, I, C>), dim3(g), dim3(kBlock), 0,
                       as_stream(stream), x, ts, yp, ybar, ndim, nz, ny, nx, pitch, wx,
                       wy, wz, gm, flags, ws);
  };
  auto with_y = [&](auto yp) {
    if (!coord)
      launch(yp, int64_t(0), std::false_type());
    else if (small)
      launch(yp, int32_t(0), std::true_type());
    else
      launch(yp, int64_t(0), std::true_type());
  };
  if (y_f64)
    with_y(static_cast<const double *>(y));
  else
    with_y(static_cast<const T *>(y));
  hipLaunchKernelGGL(k_observe_final, dim3(1), dim3(kBlock), 0, as_stream(stream), ws, g,
                     row);
  return launch_status();
}

template <typename T>
int observe_widen_impl(double *out, const T *x, double x_scale, int64_t nz, int64_t ny,
                       int64_t nx, int64_t pitch, void *stream) {
  if (!out || !x || nz < 1 || ny < 1 || nx < 1) return NSOL_EINVAL;
  if (pitch <= 0) pitch = nx;
  if (pitch < nx) return NSOL_EINVAL;
  hipLaunchKernelGGL(k_observe_widen<T>, dim3(grid_for(nz * ny * nx)), dim3(kBlock), 0,
                     as_stream(stream), out, x, (T)x_scale, nz * ny, nx, pitch);
  return launch_status();
}

}  // namespace

extern "C" {

#define NSOL_DEF_OBS(T, SUF)                                                        \
  int nsol_observe_##SUF(const T *x, double x_scale, const void *y, int y_f64,      \
                         double ybar, int ndim, int64_t nz, int64_t ny, int64_t nx, \
                         int64_t pitch, double wx, double wy, double wz,            \
                         double gamma, int flags, double *row, double *ws,          \
                         void *stream) {                                            \
    return observe_impl<T>(x, x_scale, y, y_f64, ybar, ndim, nz, ny, nx, pitch, wx, \
                           wy, wz, gamma, flags, row, ws, stream);                  \
  }                                                                                 \
  int nsol_observe_widen_##SUF(double *out, const T *x, double x_scale, int64_t nz, \
                               int64_t ny, int64_t nx, int64_t pitch,               \
                               void *stream) {                                      \
    return observe_widen_impl<T>(out, x, x_scale, nz, ny, nx, pitch, stream);       \
  }

NSOL_DEF_OBS(float, f32)
NSOL_DEF_OBS(double, f64)

}  // extern "C"
