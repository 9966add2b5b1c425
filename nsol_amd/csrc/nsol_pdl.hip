// Chambolle-Pock iteration for a LINEAR data term, lambda D_w(A x, b) + R(grad x) +
// the indicator of the box [lo, hi], for gfx950 (MI355X): the operator A is part of
// the saddle-point problem's linear map K = (grad, A) instead of the primal prox, so
// the data term has a dual variable q of its own and no iteration solves a linear
// system.
//
//   p <- prox_{sigma R*}(p + sigma grad xbar)             dual_update / dual_project
//   v  = q + sigma (A xbar - b);  q <- prox of the data term's conjugate at v
//   x+ = clip(x - tau (grad^T p + A^T q), lo, hi);  xbar <- x+ + theta (x+ - x)
//
// A and A^T are the caller's (the one-pass blur of nsol_blur3_*.hip where it applies);
// this unit holds the two kernels around them:
//   * k_pdl_dual_data: the element-wise update of q, weights, masks and the l1 data
//     term included; k_pdl_dual_data_kl: the same for the Poisson (KL) data term;
//   * k_pd_lin / k_pd_lin_iso: the regulariser's dual update and the explicit primal
//     step in ONE pass -- the tile bodies pd_fused_tile / pd_fused_iso_tile with LIN
//     on: the array in bt's place holds g = A^T q, the data prox is the step and the
//     clip.  11 words per voxel in 3-D as k_pd_fused (read xbar, x, g, p[3]; write
//     xbar, x, p[3]).
// Single volumes, one iteration per launch, contiguous arrays: there is no
// multi-iteration, persistent or pitched form.  The member-stacked form of both
// kernels (an alpha sweep, a stack of images) is nsol_pdls.hip.
#include <math.h>
#include <stddef.h>

#include <atomic>

#include "nsol_common.hpp"
#include "nsol_kl.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_fused_body.hpp"
#include "nsol_pd_iso_body.hpp"
#include "nsol_pd_launch.hpp"

using namespace nsol;

namespace {

std::atomic<int> g_lin_launches{0};

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_pd_lin(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ g, const T *__restrict__ p_in, T *__restrict__ p_out,
    Geom<T> G, PdScalars<T> S, T lo, T hi, int ntx, int nty, int zchunk, int slab) {
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  pd_fused_tile<T, VEC, LX, RY, NDIM, RAG, false, false, true>(
      xbar_in, xbar_out, x, g, p_in, p_out, G, S, tx, ty, zc, zchunk, nullptr, nullptr,
      lo, hi);
}

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_pd_lin_iso(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ g, const T *__restrict__ p_in, T *__restrict__ p_out,
    Geom<T> G, PdScalars<T> S, T lo, T hi, int ntx, int nty, int zchunk, int slab) {
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  pd_fused_iso_tile<T, VEC, LX, RY, NDIM, RAG, false, false, true>(
      xbar_in, xbar_out, x, g, p_in, p_out, G, S, tx, ty, zc, zchunk, nullptr, nullptr,
      lo, hi);
}

// The launcher struct of nsol_pd_launch.hpp, one volume.
template <bool ISO>
struct LinLauncher {
  template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
  static int launch_t(const PdLaunchArgs<T> &a) {
    const PdGridPlan g = pd_plan_grid<VEC, LX, RY>(a.G, 1, a.tune);
    if (g.blocks > kPdMaxBlocks) return -2;
    const dim3 grid((unsigned)g.blocks);
    if constexpr (ISO)
      hipLaunchKernelGGL((k_pd_lin_iso<T, VEC, LX, RY, NDIM, RAG>), grid, dim3(kBlock), 0,
                         a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.p_in, a.p_out, a.G,
                         a.S, a.lo, a.hi, g.ntx, g.nty, g.zchunk, g.slab);
    else
      hipLaunchKernelGGL((k_pd_lin<T, VEC, LX, RY, NDIM, RAG>), grid, dim3(kBlock), 0,
                         a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.p_in, a.p_out, a.G,
                         a.S, a.lo, a.hi, g.ntx, g.nty, g.zchunk, g.slab);
    const int rc = launch_status();
    if (rc == 0) g_lin_launches.fetch_add(1, std::memory_order_relaxed);
    return rc;
  }

  template <typename T, int VEC, int LX, bool RAG>
  static int launch(const PdLaunchArgs<T> &a) {
    return pd_launch_forms<LinLauncher<ISO>, T, VEC, LX, RAG>(
        a, pd_auto_rows_per_lane<VEC, LX>(a.G, 1));
  }
};

template <typename T>
int lin_iter_impl(const T *xbar_in, T *xbar_out, T *x, const T *g, const T *p_in,
                  T *p_out, int ndim, int64_t nz, int64_t ny, int64_t nx, double wx,
                  double wy, double wz, double sigma, double hden, double tau,
                  double theta, double lo, double hi, int flags, int has_p,
                  void *stream) {
  if (!pd_stack_takes(1, ndim, nz, ny, nx)) return -2;
  if (!xbar_in || !xbar_out || !x || !g || !p_in || !p_out || xbar_in == xbar_out ||
      p_in == p_out || !(lo <= hi) ||
      (flags & ~(NSOL_PD_REG_HUBER | NSOL_PD_REG_ISOTROPIC)))
    return NSOL_EINVAL;
  PdLaunchArgs<T> a{xbar_in, xbar_out, x, g, p_in, p_out,
                    make_geom<T>(ndim, nz, ny, nx, wx, wy, wz),
                    pd_make_scalars<T>(sigma, hden, tau, 0.0, theta, flags, has_p != 0)};
  // (the pd_* knobs do not reach this kernel: kPdStackTune)
  a.st = as_stream(stream);
  box_in<T>(lo, hi, a.lo, a.hi);
  if (flags & NSOL_PD_REG_ISOTROPIC) return pd_launch<LinLauncher<true>>(a);
  return pd_launch<LinLauncher<false>>(a);
}

// ---------------------------------------------------------------------------
// the data term's dual variable
// ---------------------------------------------------------------------------
// v = q + sigma (t - bt) with t = A xbar, or, t null, v = q - sigma bt with q already
// holding q + sigma A xbar (the blur's epilogue wrote it); c = lmbda * w (w = 1 without
// weights), then
//   l2: q = (v * c) / (c + sigma)        the prox of sigma (1/(2c)) |.|^2
//   l1: q = min(max(v, -c), c)           the projection onto [-c, c]
// w == 0: q = 0 exactly, whatever bt holds there -- a select on w, as in prox_data_w.
template <typename T, bool L1>
__global__ __launch_bounds__(kBlock) void k_pdl_dual_data(
    T *q, const T *__restrict__ t, const T *__restrict__ bt, const T *__restrict__ wt,
    T sigma, T lmbda, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T w = wt ? wt[i] : T(1);
    const T v = t ? q[i] + sigma * (t[i] - bt[i]) : q[i] - sigma * bt[i];
    const T c = lmbda * w;
    T r;
    if constexpr (L1) {
      r = v < -c ? -c : v;
      r = r > c ? c : r;
    } else {
      r = (v * c) / (c + sigma);
    }
    q[i] = w == T(0) ? T(0) : r;
  }
}

template <typename T>
int dual_data_impl(T *q, const T *t, const T *bt, const T *wt, double sigma, double lmbda,
                   int l1, int64_t n, void *stream) {
  if (n < 0) return NSOL_EINVAL;
  if (n == 0) return 0;
  if (!q || !bt || q == t || !(sigma > 0.0) || !(lmbda >= 0.0)) return NSOL_EINVAL;
  const dim3 grid(grid_for(n)), block(kBlock);
  if (l1)
    hipLaunchKernelGGL((k_pdl_dual_data<T, true>), grid, block, 0, as_stream(stream), q,
                       t, bt, wt, (T)sigma, (T)lmbda, n);
  else
    hipLaunchKernelGGL((k_pdl_dual_data<T, false>), grid, block, 0, as_stream(stream), q,
                       t, bt, wt, (T)sigma, (T)lmbda, n);
  return launch_status();
}

// The same pass for the Poisson (Kullback-Leibler) data term with a constant background
// bg >= 0, lambda sum w ((A x + bg) - bt log(A x + bg)): v = q + sigma * (t + bg), or, t
// null, v = q + sigma * bg; then kl_dual_prox of nsol_kl.hpp (0 where w == 0).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pdl_dual_data_kl(
    T *q, const T *__restrict__ t, const T *__restrict__ bt, const T *__restrict__ wt,
    T sigma, T lmbda, T bg, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T w = wt ? wt[i] : T(1);
    const T v = t ? q[i] + sigma * (t[i] + bg) : q[i] + sigma * bg;
    q[i] = kl_dual_prox<T>(v, bt[i], w, sigma, lmbda);
  }
}

template <typename T>
int dual_data_kl_impl(T *q, const T *t, const T *bt, const T *wt, double sigma,
                      double lmbda, double bg, int64_t n, void *stream) {
  if (n < 0) return NSOL_EINVAL;
  if (n == 0) return 0;
  if (!q || !bt || q == t || !(sigma > 0.0) || !(lmbda >= 0.0) ||
      !(isfinite(bg) && bg >= 0.0))
    return NSOL_EINVAL;
  hipLaunchKernelGGL((k_pdl_dual_data_kl<T>), dim3(grid_for(n)), dim3(kBlock), 0,
                     as_stream(stream), q, t, bt, wt, (T)sigma, (T)lmbda, (T)bg, n);
  return launch_status();
}

}  // namespace

extern "C" {

int nsol_pdl_launches(void) { return g_lin_launches.load(std::memory_order_relaxed); }

#define NSOL_PDL_DEF(T, SUF)                                                           \
  int nsol_pdl_dual_data_##SUF(T *q, const T *t, const T *bt, const T *wt,             \
                               double sigma, double lmbda, int l1, int64_t n,          \
                               void *s) {                                              \
    return dual_data_impl<T>(q, t, bt, wt, sigma, lmbda, l1, n, s);                    \
  }                                                                                    \
  int nsol_pdl_dual_data_kl_##SUF(T *q, const T *t, const T *bt, const T *wt,          \
                                  double sigma, double lmbda, double bg, int64_t n,    \
                                  void *s) {                                           \
    return dual_data_kl_impl<T>(q, t, bt, wt, sigma, lmbda, bg, n, s);                 \
  }                                                                                    \
  int nsol_pdl_iter_##SUF(const T *xi, T *xo, T *x, const T *g, const T *pi, T *po,    \
                          int ndim, int64_t nz, int64_t ny, int64_t nx, double wx,     \
                          double wy, double wz, double sigma, double hden, double tau, \
                          double theta, double lo, double hi, int flags, int has_p,    \
                          void *s) {                                                   \
    return lin_iter_impl<T>(xi, xo, x, g, pi, po, ndim, nz, ny, nx, wx, wy, wz, sigma, \
                            hden, tau, theta, lo, hi, flags, has_p, s);                \
  }

NSOL_PDL_DEF(float, f32)
NSOL_PDL_DEF(double, f64)
#undef NSOL_PDL_DEF

}  // extern "C"
