// Blur-and-sample along one axis and its exact transpose: the two halves of the
// acquisition model A = S G (a point-spread function, then "keep every f-th sample")
// behind SampledConvolutionOperator (nsol_amd/linear_operators.py).
//
//   down:  out[j] = sum_t w[t] x[map(o + j f - c + t)]                    j in [0, m)
//   up:    out[i] = sum_t w[t] q[(P - o) / f]   over the t with P >= o, f | P - o,
//          P = (i + c - t) mod len (wrap), or P = i + c - t where 0 <= P < len (constant)
//
// with m = ceil((len - o) / f).  Both are gathers: one thread owns its outputs, no
// atomics, the same bits on every run.  `down` computes only the samples it keeps; in
// the interior `up` visits only the taps t = (i + c - o) mod f, + f, ...: ceil(ntaps/f)
// loads per output.  Sums run over t upwards and accumulate in T, as k_corr_axis does.
//
// Thread mapping (all four kernels): the 256 threads of a workgroup are `lx` lanes
// along x times 256 / lx units; a unit is one row of the axis-2 kernels, and a run of
// kRun consecutive positions along the axis in one row of x of the axis-0 / axis-1
// kernels.  The index arithmetic of a unit -- its divisions, the interior test, the
// tap indices -- is therefore uniform per wave and kept in scalar registers
// (wave_uniform).  A run along axis 0 / 1 loads every input row it needs ONCE and adds
// it to the outputs of the run it reaches (down_run, up_run): (kRun - 1) f + ntaps row
// loads for kRun outputs of `down` instead of kRun ntaps.  The tap loops keep kAhead
// loads in flight.  Along axes 0 and 1 a lane owns a 16-byte vector of consecutive x
// where the rows are whole vectors and the pointers aligned, else one element.
// Indexing is 64-bit.
#include "nsol_common.hpp"

using namespace nsol;

namespace {

constexpr int kMaxTaps = 129;   // as nsol_corr_axis_* (ConvolutionOperator's limit)
constexpr int kRun = 8;         // consecutive positions along the axis per wave

template <typename T>
struct Taps {
  T w[kMaxTaps];
};

template <typename T, int VEC>
struct alignas(VEC * sizeof(T)) Pack {
  T v[VEC];
};

template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> load_pack(const T *p) {
  return *reinterpret_cast<const Pack<T, VEC> *>(p);
}

template <typename T, int VEC>
__device__ __forceinline__ void fma_pack(Pack<T, VEC> &acc, T w, const Pack<T, VEC> &v) {
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc.v[k] += w * v.v[k];
}

template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> zero_pack() {
  Pack<T, VEC> acc;
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc.v[k] = T(0);
  return acc;
}

// the sample that position p refers to: itself inside [0, len), its periodic image
// (wrap) or -1 = "no term" (constant) outside
__device__ __forceinline__ int64_t sample_at(int64_t p, int64_t len, int wrap) {
  if (p >= 0 && p < len) return p;
  if (!wrap) return -1;
  const int64_t j = p % len;
  return j < 0 ? j + len : j;
}

// v / f for v >= 0, f >= 1 (the 32-bit division is a fifth of the 64-bit one)
__device__ __forceinline__ int64_t div_pos(int64_t v, int f) {
  return (uint64_t)v >> 32 ? v / f : (int64_t)((uint32_t)v / (uint32_t)f);
}

// a value every lane of the wave holds, as a scalar: the wave's unit and everything
// derived from it (rows, interior tests, tap indices) then live in scalar registers
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// what the four kernels share: one axis of extent len sampled to m = ceil((len-o)/f)
struct Axis {
  int64_t len, m;
  int ntaps, centre, wrap, f, o;
};

constexpr int kAhead = 4;       // loads in flight per lane in the tap loops

// sum_t w[t] x[map(o + j f - c + t)] at stride `step`, VEC consecutive x at once
template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> down_at(const T *src, int64_t step, int64_t j,
                                                const Taps<T> &taps, const Axis &ax) {
  Pack<T, VEC> acc = zero_pack<T, VEC>();
  const int64_t lo = ax.o + j * ax.f - ax.centre;
  if (lo >= 0 && lo + ax.ntaps <= ax.len) {      // interior: no index mapping
    const T *p = src + lo * step;
    int t = 0;
    for (; t + kAhead <= ax.ntaps; t += kAhead) {
      Pack<T, VEC> v[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) v[k] = load_pack<T, VEC>(p + (t + k) * step);
#pragma unroll
      for (int k = 0; k < kAhead; ++k) fma_pack<T, VEC>(acc, taps.w[t + k], v[k]);
    }
    for (; t < ax.ntaps; ++t)
      fma_pack<T, VEC>(acc, taps.w[t], load_pack<T, VEC>(p + t * step));
  } else {
    for (int t = 0; t < ax.ntaps; ++t) {
      const int64_t P = sample_at(lo + t, ax.len, ax.wrap);
      if (P >= 0) fma_pack<T, VEC>(acc, taps.w[t], load_pack<T, VEC>(src + P * step));
    }
  }
  return acc;
}

// the transpose: sum over the taps that reach a kept sample from position i
template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> up_at(const T *src, int64_t step, int64_t i,
                                              const Taps<T> &taps, const Axis &ax) {
  Pack<T, VEC> acc = zero_pack<T, VEC>();
  const int64_t top = i + ax.centre;             // P of tap 0; P falls as t grows
  if (top - (ax.ntaps - 1) >= 0 && top < ax.len) {
    // interior: every P is a position of its own; the kept ones are f apart
    const int64_t v = top - ax.o;
    if (v < 0) return acc;                       // (every P is below the first sample)
    const int64_t k0 = div_pos(v, ax.f);         // (< m: P <= len - 1)
    const int t0 = (int)(v - k0 * ax.f);
    // terms: t = t0 + s f < ntaps with k = k0 - s >= 0
    int64_t terms = t0 < ax.ntaps ? (ax.ntaps - 1 - t0) / ax.f + 1 : 0;
    if (terms > k0 + 1) terms = k0 + 1;
    const T *p = src + k0 * step;
    int64_t s = 0;
    for (; s + kAhead <= terms; s += kAhead) {
      Pack<T, VEC> q[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) q[k] = load_pack<T, VEC>(p - (s + k) * step);
#pragma unroll
      for (int k = 0; k < kAhead; ++k)
        fma_pack<T, VEC>(acc, taps.w[t0 + (s + k) * ax.f], q[k]);
    }
    for (; s < terms; ++s)
      fma_pack<T, VEC>(acc, taps.w[t0 + s * ax.f], load_pack<T, VEC>(p - s * step));
  } else {
    for (int t = 0; t < ax.ntaps; ++t) {
      const int64_t P = sample_at(top - t, ax.len, ax.wrap);
      if (P < ax.o) continue;
      const int64_t d = P - ax.o;
      const int64_t k = div_pos(d, ax.f);
      if (d - k * ax.f == 0 && k < ax.m)
        fma_pack<T, VEC>(acc, taps.w[t], load_pack<T, VEC>(src + k * step));
    }
  }
  return acc;
}

// kRun consecutive outputs j = first .. first + nrun - 1 of `down` in one sweep over
// the input rows they share: every row is loaded once and added to the outputs it
// reaches.  For one output the rows arrive with t rising, the order of down_at.
template <typename T, int VEC>
__device__ __forceinline__ void down_run(const T *src, T *dst, int64_t step,
                                         int64_t first, int nrun, const Taps<T> &taps,
                                         const Axis &ax) {
  Pack<T, VEC> acc[kRun];
#pragma unroll
  for (int r = 0; r < kRun; ++r) acc[r] = zero_pack<T, VEC>();
  const int64_t lo0 = ax.o + first * ax.f - ax.centre;      // tap 0 of output `first`
  const int64_t span = (int64_t)(nrun - 1) * ax.f + ax.ntaps;
  for (int64_t d0 = 0; d0 < span; d0 += kAhead) {
    Pack<T, VEC> v[kAhead];
    bool has[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      const int64_t P = d0 + k < span ? sample_at(lo0 + d0 + k, ax.len, ax.wrap) : -1;
      has[k] = P >= 0;
      if (has[k]) v[k] = load_pack<T, VEC>(src + P * step);
    }
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      if (!has[k]) continue;
#pragma unroll
      for (int r = 0; r < kRun; ++r) {
        const int64_t t = d0 + k - (int64_t)r * ax.f;
        if (r < nrun && t >= 0 && t < ax.ntaps) fma_pack<T, VEC>(acc[r], taps.w[t], v[k]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kRun; ++r)
    if (r < nrun) *reinterpret_cast<Pack<T, VEC> *>(dst + (first + r) * step) = acc[r];
}

// The same for `up` where every output of the run is interior (no position wraps or
// leaves the axis): the kept samples k that reach the run, from the last down, each
// loaded once; output i = first + r takes tap t = i + c - o - k f, rising as k falls.
// Runs that touch the boundary go output by output through up_at.
template <typename T, int VEC>
__device__ __forceinline__ void up_run(const T *src, T *dst, int64_t step, int64_t first,
                                       int nrun, const Taps<T> &taps, const Axis &ax) {
  const int64_t top0 = first + ax.centre;
  if (!(top0 - (ax.ntaps - 1) >= 0 && top0 + nrun - 1 < ax.len)) {
    for (int r = 0; r < nrun; ++r)
      *reinterpret_cast<Pack<T, VEC> *>(dst + (first + r) * step) =
          up_at<T, VEC>(src, step, first + r, taps, ax);
    return;
  }
  Pack<T, VEC> acc[kRun];
#pragma unroll
  for (int r = 0; r < kRun; ++r) acc[r] = zero_pack<T, VEC>();
  const int64_t v0 = top0 - ax.o, v1 = v0 + nrun - 1;      // i + c - o of the run's ends
  if (v1 >= 0) {
    const int64_t k_hi = div_pos(v1, ax.f);                // (< m: P <= len - 1)
    const int64_t need = v0 - (ax.ntaps - 1);              // smallest k f that counts
    const int64_t k_lo = need <= 0 ? 0 : div_pos(need + ax.f - 1, ax.f);
    for (int64_t k0 = k_hi; k0 >= k_lo; k0 -= kAhead) {
      Pack<T, VEC> q[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k)
        if (k0 - k >= k_lo) q[k] = load_pack<T, VEC>(src + (k0 - k) * step);
#pragma unroll
      for (int k = 0; k < kAhead; ++k) {
        if (k0 - k < k_lo) continue;
#pragma unroll
        for (int r = 0; r < kRun; ++r) {
          const int64_t t = v0 + r - (k0 - k) * ax.f;
          if (r < nrun && t >= 0 && t < ax.ntaps)
            fma_pack<T, VEC>(acc[r], taps.w[t], q[k]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kRun; ++r)
    if (r < nrun) *reinterpret_cast<Pack<T, VEC> *>(dst + (first + r) * step) = acc[r];
}

// Array axis 0 or 1.  The side with the full extent `len` along the axis is
// (nz, ny, nx), the other has m there; UP: the full side is the output.  A unit is
// (run of kRun positions along the axis) x (index along the other slow axis).
template <typename T, int VEC, bool UP>
__global__ __launch_bounds__(kBlock) void k_sample_rows(
    const T *__restrict__ in, T *__restrict__ out, int axis, int64_t nz, int64_t ny,
    int64_t nx, Axis ax, Taps<T> taps, int lx_shift) {
  const int lx = 1 << lx_shift;
  const int64_t nxv = nx / VEC;
  const int64_t n_out = UP ? ax.len : ax.m;      // outputs along the axis
  const int64_t n_in = UP ? ax.m : ax.len;
  const int64_t runs = (n_out + kRun - 1) / kRun;
  const int64_t units = axis == 0 ? runs * ny : nz * runs;
  const int64_t inner = axis == 0 ? ny : runs;
  // strides along the axis, and of the other slow axis, on either side
  const int64_t step = axis == 0 ? ny * nx : nx;
  const int64_t in_other = axis == 0 ? nx : n_in * nx;
  const int64_t out_other = axis == 0 ? nx : n_out * nx;
  const int64_t per_block = kBlock >> lx_shift;
  for (int64_t u = wave_uniform((int64_t)blockIdx.x * per_block +
                                (threadIdx.x >> lx_shift));
       u < units; u += (int64_t)gridDim.x * per_block) {
    const int64_t a = u / inner, b = u - a * inner;
    const int64_t run = axis == 0 ? a : b, other = axis == 0 ? b : a;
    const int64_t first = run * kRun;
    const int nrun = (int)(first + kRun < n_out ? kRun : n_out - first);
    for (int64_t xv = (int64_t)blockIdx.y * lx + (threadIdx.x & (lx - 1)); xv < nxv;
         xv += (int64_t)gridDim.y * lx) {
      const T *src = in + other * in_other + xv * VEC;
      T *dst = out + other * out_other + xv * VEC;
      if (UP) up_run<T, VEC>(src, dst, step, first, nrun, taps, ax);
      else down_run<T, VEC>(src, dst, step, first, nrun, taps, ax);
    }
  }
}

// Array axis 2: a unit is a row; lanes run along the outputs of the row.  `down` reads
// its taps at stride f across the lanes (64 f + ntaps consecutive elements per wave and
// tap loop, the same cache lines for every t), `up` gathers ceil(ntaps / f) samples.
template <typename T, bool UP>
__global__ __launch_bounds__(kBlock) void k_sample_x(
    const T *__restrict__ in, T *__restrict__ out, int64_t rows, Axis ax, Taps<T> taps,
    int lx_shift) {
  const int lx = 1 << lx_shift;
  const int64_t n_out = UP ? ax.len : ax.m;
  const int64_t n_in = UP ? ax.m : ax.len;
  const int64_t per_block = kBlock >> lx_shift;
  for (int64_t r = wave_uniform((int64_t)blockIdx.x * per_block +
                                (threadIdx.x >> lx_shift));
       r < rows; r += (int64_t)gridDim.x * per_block) {
    const T *src = in + r * n_in;
    T *dst = out + r * n_out;
    for (int64_t j = (int64_t)blockIdx.y * lx + (threadIdx.x & (lx - 1)); j < n_out;
         j += (int64_t)gridDim.y * lx) {
      const Pack<T, 1> acc = UP ? up_at<T, 1>(src, 1, j, taps, ax)
                                : down_at<T, 1>(src, 1, j, taps, ax);
      dst[j] = acc.v[0];
    }
  }
}

// units along grid x (4 per workgroup of 64 lanes, or 1 of 256 where there are fewer
// than 4), lanes along grid y; both loops of the kernels stride by the grid
inline void launch_shape(int64_t units, int64_t items, dim3 *grid, int *lx_shift) {
  *lx_shift = units < 4 ? 8 : 6;
  const int64_t per_block = kBlock >> *lx_shift, lx = (int64_t)1 << *lx_shift;
  int64_t gx = (units + per_block - 1) / per_block, gy = (items + lx - 1) / lx;
  if (gx > 0x7fffffff) gx = 0x7fffffff;
  if (gy > 65535) gy = 65535;
  *grid = dim3((unsigned)gx, (unsigned)gy, 1);
}

template <typename T, bool UP>
int sample_impl(const T *in, T *out, int axis, int64_t nz, int64_t ny, int64_t nx,
                const double *taps_host, int ntaps, int centre, int mode, int factor,
                int offset, void *stream) {
  if (!in || !out || in == out || !taps_host || axis < 0 || axis > 2 || nz < 1 ||
      ny < 1 || nx < 1 || ntaps < 1 || ntaps > kMaxTaps || centre < 0 ||
      centre >= ntaps || (mode != NSOL_MODE_WRAP && mode != NSOL_MODE_CONSTANT) ||
      factor < 1)
    return NSOL_EINVAL;
  const int64_t len = axis == 2 ? nx : (axis == 1 ? ny : nz);
  if (offset < 0 || offset >= factor || offset >= len) return NSOL_EINVAL;
  Axis ax;
  ax.len = len;
  ax.m = (len - offset + factor - 1) / factor;
  ax.ntaps = ntaps; ax.centre = centre; ax.wrap = mode == NSOL_MODE_WRAP;
  ax.f = factor; ax.o = offset;
  Taps<T> taps;
  for (int t = 0; t < kMaxTaps; ++t) taps.w[t] = t < ntaps ? (T)taps_host[t] : T(0);
  hipStream_t st = as_stream(stream);
  dim3 grid;
  int lx_shift;
  if (axis == 2) {
    launch_shape(nz * ny, UP ? len : ax.m, &grid, &lx_shift);
    hipLaunchKernelGGL((k_sample_x<T, UP>), grid, dim3(kBlock), 0, st, in, out, nz * ny,
                       ax, taps, lx_shift);
    return launch_status();
  }
  constexpr int VEC = 16 / sizeof(T);
  const int64_t runs = ((UP ? len : ax.m) + kRun - 1) / kRun;
  const int64_t units = axis == 0 ? runs * ny : nz * runs;
  // rows of whole vectors from aligned bases: every row of either side starts on the
  // 16-byte grid (the row pitch is nx on both)
  if (nx % VEC == 0 && aligned16(in) && aligned16(out)) {
    launch_shape(units, nx / VEC, &grid, &lx_shift);
    hipLaunchKernelGGL((k_sample_rows<T, VEC, UP>), grid, dim3(kBlock), 0, st, in, out,
                       axis, nz, ny, nx, ax, taps, lx_shift);
  } else {
    launch_shape(units, nx, &grid, &lx_shift);
    hipLaunchKernelGGL((k_sample_rows<T, 1, UP>), grid, dim3(kBlock), 0, st, in, out,
                       axis, nz, ny, nx, ax, taps, lx_shift);
  }
  return launch_status();
}

}  // namespace

extern "C" {
int nsol_corr_axis_down_f32(const float *x, float *out, int axis, int64_t nz,
                            int64_t ny, int64_t nx, const double *taps_host, int ntaps,
                            int centre, int mode, int factor, int offset, void *stream) {
  return sample_impl<float, false>(x, out, axis, nz, ny, nx, taps_host, ntaps, centre,
                                   mode, factor, offset, stream);
}
int nsol_corr_axis_down_f64(const double *x, double *out, int axis, int64_t nz,
                            int64_t ny, int64_t nx, const double *taps_host, int ntaps,
                            int centre, int mode, int factor, int offset, void *stream) {
  return sample_impl<double, false>(x, out, axis, nz, ny, nx, taps_host, ntaps, centre,
                                    mode, factor, offset, stream);
}
int nsol_corr_axis_up_f32(const float *q, float *out, int axis, int64_t nz, int64_t ny,
                          int64_t nx, const double *taps_host, int ntaps, int centre,
                          int mode, int factor, int offset, void *stream) {
  return sample_impl<float, true>(q, out, axis, nz, ny, nx, taps_host, ntaps, centre,
                                  mode, factor, offset, stream);
}
int nsol_corr_axis_up_f64(const double *q, double *out, int axis, int64_t nz, int64_t ny,
                          int64_t nx, const double *taps_host, int ntaps, int centre,
                          int mode, int factor, int offset, void *stream) {
  return sample_impl<double, true>(q, out, axis, nz, ny, nx, taps_host, ntaps, centre,
                                   mode, factor, offset, stream);
}
}
