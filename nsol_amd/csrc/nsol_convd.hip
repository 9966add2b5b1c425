// Tiled correlation with arbitrary (dense) taps: what ConvolutionOperator runs for a
// kernel that is no outer product -- an oriented Gaussian, a measured or motion-blur
// PSF -- in the place of k_corr_dense (nsol_conv.hip), with the same bits.
//
// A 256-thread workgroup owns ty x tx outputs of a plane and marches along z over a slab
// of output planes.  The LDS holds a ring of kz input planes of (ty + ky - 1) rows; the
// boundary rule is applied when a plane is filled (through two tables of mapped row and
// column indices made once per workgroup; zero for `constant`), so the tap loops have no
// index mapping, no division and no global loads.  A lane item is kRX = 4 consecutive x
// outputs of one row: per tap row (a, b) it reads its window from the LDS in whole
// 16-byte vectors, kRX taps at a time, and slides the taps over it in registers (one
// ds_read_b128 -- two in double -- per 16 multiply-add pairs).  The taps are read through
// a uniform index from a const __restrict__ pointer; the compiler issues the four taps of
// a chunk as one 16-byte global load per lane (an L1 hit, off the LDS port the windows
// use) and scalar loads only for the last kx mod 4 taps of a row.
//
// The bits are k_corr_dense's for finite inputs and taps: every output accumulates in
// the same order (a, then b, then c, ascending) with a separate multiply and add (the
// library is built with -ffp-contract=off; there is no explicit fma here).  Under
// `constant` k_corr_dense skips a tap that falls outside, while this kernel adds
// tap * 0 for it.  That cannot change a finite sum: acc starts at +0, a finite tap
// times 0 is +0 or -0, and +0 + -0 = +0, v + (+-0) = v for every other v.
//
// Plan (tile, slab, LDS bytes, grid): nsol_convd_plan.hpp, host only.
#include <type_traits>

#include "nsol_common.hpp"
#include "nsol_conv_index.hpp"
#include "nsol_convd_plan.hpp"

using namespace nsol;
using nsol_convd::kRX;

namespace {

template <typename T>
struct Vec16 {
  static constexpr int N = 16 / sizeof(T);
  typedef T type __attribute__((ext_vector_type(16 / sizeof(T))));
};

// kRX consecutive elements from a 16-byte aligned LDS address
template <typename T>
__device__ __forceinline__ void load_window(const T *p, T (&w)[kRX]) {
  typedef typename Vec16<T>::type V;
  constexpr int N = Vec16<T>::N;
#pragma unroll
  for (int q = 0; q < kRX / N; ++q) {
    const V v = *reinterpret_cast<const V *>(p + q * N);
#pragma unroll
    for (int k = 0; k < N; ++k) w[q * N + k] = v[k];
  }
}

// VST: rows are whole 16-byte vectors and `out` lies on the 16-byte grid, so an item
// inside the row stores vectors; otherwise, and at a row's ragged end, element by element.
template <typename T, bool VST>
__global__ __launch_bounds__(nsol_convd::kThreads) void k_corr_dense_tile(
    const T *__restrict__ x, T *__restrict__ out, int64_t nz, int64_t ny, int64_t nx,
    const T *__restrict__ taps, int kz, int ky, int kx, int cz, int cy, int cx, int mode,
    int ty, int tx, int slab, int ntx, int nty) {
  constexpr int NT = nsol_convd::kThreads;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T *ring = reinterpret_cast<T *>(smem_raw);
  const int fh = ty + ky - 1, fw = tx + kx - 1;
  const int pw = tx + ((kx + kRX - 1) / kRX) * kRX;
  const int plane_elems = fh * pw;
  // (the ring's bytes are a multiple of 16: pw is a multiple of kRX)
  int64_t *ymap = reinterpret_cast<int64_t *>(ring + (size_t)kz * plane_elems);
  int64_t *xmap = ymap + fh;
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int bx = bid % ntx;
  bid /= ntx;
  const int by = bid % nty;
  const int bs = bid / nty;
  const int64_t x0 = (int64_t)bx * tx, y0 = (int64_t)by * ty, z0 = (int64_t)bs * slab;
  const int64_t z1 = z0 + slab < nz ? z0 + slab : nz;

  // rows of the tile's last, ragged part map like any position outside the volume: every
  // table entry is a valid index or -1
  for (int i = tid; i < fh; i += NT) ymap[i] = map_index(y0 + i - cy, ny, mode);
  for (int i = tid; i < fw; i += NT) xmap[i] = map_index(x0 + i - cx, nx, mode);
  __syncthreads();

  // element e = tid + k NT of a plane's fh x fw footprint, advanced without a division
  const unsigned fy0 = (unsigned)tid / (unsigned)fw, fx0 = (unsigned)tid - fy0 * (unsigned)fw;
  const unsigned dq = (unsigned)NT / (unsigned)fw, dr = (unsigned)NT - dq * (unsigned)fw;
  auto fill = [&](int64_t zin, int slot) {
    const int64_t jz = map_index(zin, nz, mode);
    T *dst = ring + (size_t)slot * plane_elems;
    const T *src = x + (jz < 0 ? 0 : jz) * ny * nx;
    unsigned fy = fy0, fx = fx0;
    while (fy < (unsigned)fh) {
      const int64_t jy = ymap[fy], jx = xmap[fx];
      T v = T(0);
      if (jz >= 0 && jy >= 0 && jx >= 0) v = src[jy * nx + jx];
      dst[fy * pw + fx] = v;
      fy += dq;
      fx += dr;
      if (fx >= (unsigned)fw) { fx -= (unsigned)fw; ++fy; }
    }
  };

  // ring slot of the input plane z0 - cz + q is q mod kz
  for (int q = 0; q + 1 < kz; ++q) fill(z0 - cz + q, q);

  const int lanes_x = tx / kRX;
  const int items = ty * lanes_x;
  int base = 0;                                   // (z - z0) mod kz
  for (int64_t z = z0; z < z1; ++z) {
    fill(z - cz + kz - 1, base == 0 ? kz - 1 : base - 1);
    __syncthreads();
    for (int it = tid; it < items; it += NT) {
      const int ly = (unsigned)it / (unsigned)lanes_x;
      const int lx = it - ly * lanes_x;
      const int64_t oy = y0 + ly, ox = x0 + (int64_t)lx * kRX;
      if (oy >= ny || ox >= nx) continue;
      T acc[kRX];
#pragma unroll
      for (int r = 0; r < kRX; ++r) acc[r] = T(0);
      const T *tw = taps;
      for (int a = 0; a < kz; ++a) {
        int slot = base + a;
        if (slot >= kz) slot -= kz;
        const T *row = ring + (size_t)slot * plane_elems + (size_t)ly * pw + lx * kRX;
        for (int b = 0; b < ky; ++b, row += pw, tw += kx) {
          T cur[kRX], nxt[kRX];
          load_window(row, cur);
          int c0 = 0;
          for (; c0 + kRX <= kx; c0 += kRX) {
            load_window(row + c0 + kRX, nxt);
#pragma unroll
            for (int j = 0; j < kRX; ++j) {
              const T w = tw[c0 + j];
#pragma unroll
              for (int r = 0; r < kRX; ++r) {
                const T v = r + j < kRX ? cur[r + j < kRX ? r + j : 0]
                                        : nxt[r + j >= kRX ? r + j - kRX : 0];
                acc[r] += w * v;
              }
            }
#pragma unroll
            for (int r = 0; r < kRX; ++r) cur[r] = nxt[r];
          }
          if (c0 < kx) {                         // the last kx mod kRX taps of the row
            load_window(row + c0 + kRX, nxt);
#pragma unroll
            for (int j = 0; j < kRX - 1; ++j) {
              if (c0 + j < kx) {
                const T w = tw[c0 + j];
#pragma unroll
                for (int r = 0; r < kRX; ++r) {
                  const T v = r + j < kRX ? cur[r + j < kRX ? r + j : 0]
                                          : nxt[r + j >= kRX ? r + j - kRX : 0];
                  acc[r] += w * v;
                }
              }
            }
          }
        }
      }
      T *o = out + (z * ny + oy) * nx + ox;
      if (VST && ox + kRX <= nx) {
        typedef typename Vec16<T>::type V;
        constexpr int N = Vec16<T>::N;
#pragma unroll
        for (int q = 0; q < kRX / N; ++q) {
          V v;
#pragma unroll
          for (int k = 0; k < N; ++k) v[k] = acc[q * N + k];
          *reinterpret_cast<V *>(o + q * N) = v;
        }
      } else {
#pragma unroll
        for (int r = 0; r < kRX; ++r)
          if (ox + r < nx) o[r] = acc[r];
      }
    }
    __syncthreads();
    if (++base == kz) base = 0;
  }
}

template <typename T>
int corr_dense_tiled_impl(const T *x, T *out, int64_t nz, int64_t ny, int64_t nx,
                          const T *taps, int kz, int ky, int kx, int cz, int cy, int cx,
                          int mode, int ty, int tx, int slab, void *stream) {
  if (!x || !out || !taps || nz < 1 || ny < 1 || nx < 1 || kz < 1 || ky < 1 || kx < 1 ||
      cz < 0 || cz >= kz || cy < 0 || cy >= ky || cx < 0 || cx >= kx || mode < 0 ||
      mode > 4 || ty < 0 || tx < 0 || slab < 0)
    return NSOL_EINVAL;
  if (ny > INT64_MAX / nx || nz > INT64_MAX / (ny * nx) / (int64_t)sizeof(T))
    return NSOL_EINVAL;
  const int64_t n = nz * ny * nx;
  {
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
    const uintptr_t bytes = (uintptr_t)n * sizeof(T);
    if (xa < oa + bytes && oa < xa + bytes) return NSOL_EINVAL;   // x and out overlap
  }
  const nsol_convd::Plan p =
      nsol_convd::plan(nz, ny, nx, kz, ky, kx, (int)sizeof(T), ty, tx, slab);
  if (p.status != nsol_convd::kOk) return p.status;
  const bool vst = (nx * sizeof(T)) % 16 == 0 && aligned16(out);
  void (*kern)(const T *, T *, int64_t, int64_t, int64_t, const T *, int, int, int, int, int,
               int, int, int, int, int, int, int) =
      vst ? k_corr_dense_tile<T, true> : k_corr_dense_tile<T, false>;
  if (p.lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)p.lds_bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return nsol_convd::kDecline; }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)p.blocks), dim3(nsol_convd::kThreads),
                     (size_t)p.lds_bytes, as_stream(stream), x, out, nz, ny, nx, taps, kz, ky,
                     kx, cz, cy, cx, mode, p.ty, p.tx, p.slab, (int)p.ntx, (int)p.nty);
  return launch_status();
}

}  // namespace

extern "C" {
int nsol_corr_dense_tiled_f32(const float *x, float *out, int64_t nz, int64_t ny, int64_t nx,
                              const float *taps, int kz, int ky, int kx, int cz, int cy,
                              int cx, int mode, int ty, int tx, int slab, void *stream) {
  return corr_dense_tiled_impl<float>(x, out, nz, ny, nx, taps, kz, ky, kx, cz, cy, cx, mode,
                                      ty, tx, slab, stream);
}
int nsol_corr_dense_tiled_f64(const double *x, double *out, int64_t nz, int64_t ny,
                              int64_t nx, const double *taps, int kz, int ky, int kx, int cz,
                              int cy, int cx, int mode, int ty, int tx, int slab,
                              void *stream) {
  return corr_dense_tiled_impl<double>(x, out, nz, ny, nx, taps, kz, ky, kx, cz, cy, cx,
                                       mode, ty, tx, slab, stream);
}
int nsol_corr_dense_tiled_plan(int64_t nz, int64_t ny, int64_t nx, int kz, int ky, int kx,
                               int elem_size, int ty, int tx, int slab, int64_t *plan) {
  if (!plan) return NSOL_EINVAL;
  const nsol_convd::Plan p = nsol_convd::plan(nz, ny, nx, kz, ky, kx, elem_size, ty, tx, slab);
  if (p.status != nsol_convd::kOk) return p.status;
  plan[0] = p.ty; plan[1] = p.tx; plan[2] = p.slab; plan[3] = p.lds_bytes;
  plan[4] = p.ntx; plan[5] = p.nty; plan[6] = p.nslab; plan[7] = p.blocks;
  return 0;
}
}
