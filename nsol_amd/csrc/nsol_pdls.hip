// Member-stacked Chambolle-Pock iteration for a LINEAR data term for gfx950 (MI355X):
// P independent runs of nsol_pdl.hip's iteration on volumes of one shape -- the members
// of an alpha sweep on one observation, the slices of a stack deconvolved slice by
// slice, a set of small volumes -- advance by one iteration in one launch of each of
// the two kernels around the caller's A and A^T:
//   * k_pdl_dual_data_stack: the element-wise update of every member's q, member m =
//     blockIdx.y with its own lambda_m (a device array); bt and wt at a member stride of
//     0 (a sweep shares them) or n (a stack brings its own), as nsol_pd_weighted_*;
//   * k_pdl_stack / k_pdl_stack_iso: the regulariser's dual update and the explicit
//     primal step -- pd_fused_tile / pd_fused_iso_tile with LIN on, as k_pd_lin, on the
//     member's own slices with the member-local geometry G (the blockIdx.y pattern of
//     nsol_pdb.hip), so member m is bit-identical to nsol_pdl_iter_* on that member.
// The scalars and the box are common to the stack and passed by value: tau, sigma,
// theta, hden, the flags and the box do not depend on alpha in this solver; alpha
// enters the update of q alone.
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

std::atomic<int> g_lin_stack_launches{0};

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_pdl_stack(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ g, const T *__restrict__ p_in, T *__restrict__ p_out,
    Geom<T> G, PdScalars<T> S, T lo, T hi, int ntx, int nty, int zchunk, int slab) {
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  // gridDim.y = members
  const int64_t m = blockIdx.y;
  const int64_t xo = m * G.n;
  const int64_t po = m * G.n * NDIM;
  pd_fused_tile<T, VEC, LX, RY, NDIM, RAG, false, false, true>(
      xbar_in + xo, xbar_out + xo, x + xo, g + xo, p_in + po, p_out + po, G, S, tx, ty,
      zc, zchunk, nullptr, nullptr, lo, hi);
}

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_pdl_stack_iso(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ g, const T *__restrict__ p_in, T *__restrict__ p_out,
    Geom<T> G, PdScalars<T> S, T lo, T hi, int ntx, int nty, int zchunk, int slab) {
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  const int64_t m = blockIdx.y;
  const int64_t xo = m * G.n;
  const int64_t po = m * G.n * NDIM;
  pd_fused_iso_tile<T, VEC, LX, RY, NDIM, RAG, false, false, true>(
      xbar_in + xo, xbar_out + xo, x + xo, g + xo, p_in + po, p_out + po, G, S, tx, ty,
      zc, zchunk, nullptr, nullptr, lo, hi);
}

// The launcher struct of nsol_pd_launch.hpp: the members count as tiles in the grid
// and in the rows per lane, as in BatchLauncher.
template <bool ISO>
struct LinStackLauncher {
  template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
  static int launch_t(const PdLaunchArgs<T> &a) {
    const PdGridPlan g = pd_plan_grid<VEC, LX, RY>(a.G, a.members, a.tune);
    if (g.blocks > kPdMaxBlocks) return -2;   // (the caller runs the members one by one)
    const dim3 grid((unsigned)g.blocks, (unsigned)a.members);
    if constexpr (ISO)
      hipLaunchKernelGGL((k_pdl_stack_iso<T, VEC, LX, RY, NDIM, RAG>), grid, dim3(kBlock),
                         0, a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.p_in, a.p_out, a.G,
                         a.S, a.lo, a.hi, g.ntx, g.nty, g.zchunk, g.slab);
    else
      hipLaunchKernelGGL((k_pdl_stack<T, VEC, LX, RY, NDIM, RAG>), grid, dim3(kBlock), 0,
                         a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.p_in, a.p_out, a.G,
                         a.S, a.lo, a.hi, g.ntx, g.nty, g.zchunk, g.slab);
    const int rc = launch_status();
    if (rc == 0) g_lin_stack_launches.fetch_add(1, std::memory_order_relaxed);
    return rc;
  }

  template <typename T, int VEC, int LX, bool RAG>
  static int launch(const PdLaunchArgs<T> &a) {
    return pd_launch_forms<LinStackLauncher<ISO>, T, VEC, LX, RAG>(
        a, pd_auto_rows_per_lane<VEC, LX>(a.G, a.members));
  }
};

template <typename T>
int lin_stack_iter_impl(const T *xbar_in, T *xbar_out, T *x, const T *g, const T *p_in,
                        T *p_out, int members, int ndim, int64_t nz, int64_t ny,
                        int64_t nx, double wx, double wy, double wz, double sigma,
                        double hden, double tau, double theta, double lo, double hi,
                        int flags, int has_p, void *stream) {
  if (!pd_stack_takes(members, ndim, nz, ny, nx)) return -2;
  if (!xbar_in || !xbar_out || !x || !g || !p_in || !p_out || xbar_in == xbar_out ||
      p_in == p_out || !(lo <= hi) || !(sigma > 0.0) ||
      (flags & ~(NSOL_PD_REG_HUBER | NSOL_PD_REG_ISOTROPIC)))
    return NSOL_EINVAL;
  PdLaunchArgs<T> a{xbar_in, xbar_out, x, g, p_in, p_out,
                    make_geom<T>(ndim, nz, ny, nx, wx, wy, wz),
                    pd_make_scalars<T>(sigma, hden, tau, 0.0, theta, flags, has_p != 0)};
  a.members = members;    // (the pd_* knobs do not reach the stack: kPdStackTune)
  a.st = as_stream(stream);
  box_in<T>(lo, hi, a.lo, a.hi);
  if (flags & NSOL_PD_REG_ISOTROPIC) return pd_launch<LinStackLauncher<true>>(a);
  return pd_launch<LinStackLauncher<false>>(a);
}

// ---------------------------------------------------------------------------
// the data term's dual variables
// ---------------------------------------------------------------------------
// k_pdl_dual_data (nsol_pdl.hip) on member m = blockIdx.y, expression for expression:
// q and t at m n, bt and wt at m times their member strides, lmbda[m] rounded to T by
// the host as (T)lmbda is there.
template <typename T, bool L1>
__global__ __launch_bounds__(kBlock) void k_pdl_dual_data_stack(
    T *q_all, const T *__restrict__ t_all, const T *__restrict__ bt_all,
    int64_t bt_stride, const T *__restrict__ wt_all, int64_t wt_stride, T sigma,
    const T *__restrict__ lmbda_all, int64_t n) {
  const int64_t m = blockIdx.y;
  T *q = q_all + m * n;
  const T *t = t_all ? t_all + m * n : nullptr;
  const T *bt = bt_all + m * bt_stride;
  const T *wt = wt_all ? wt_all + m * wt_stride : nullptr;
  const T lmbda = lmbda_all[m];
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
int dual_data_stack_impl(T *q, const T *t, const T *bt, int64_t bt_stride, const T *wt,
                         int64_t wt_stride, double sigma, const T *lmbda, int l1,
                         int members, int64_t n, void *stream) {
  if (n < 0) return NSOL_EINVAL;
  // members * n within 2^31 elements, as the tile kernel's stack
  if (!pd_members_ok(members) || n > (int64_t(1) << 31) / members) return -2;
  if (n == 0) return 0;
  if (!q || !bt || !lmbda || q == t || !(sigma > 0.0) || !pd_stride_ok(bt_stride, n) ||
      (wt && !pd_stride_ok(wt_stride, n)))
    return NSOL_EINVAL;
  const dim3 grid((unsigned)grid_for(n), (unsigned)members), block(kBlock);
  if (l1)
    hipLaunchKernelGGL((k_pdl_dual_data_stack<T, true>), grid, block, 0,
                       as_stream(stream), q, t, bt, bt_stride, wt, wt_stride, (T)sigma,
                       lmbda, n);
  else
    hipLaunchKernelGGL((k_pdl_dual_data_stack<T, false>), grid, block, 0,
                       as_stream(stream), q, t, bt, bt_stride, wt, wt_stride, (T)sigma,
                       lmbda, n);
  return launch_status();
}

// k_pdl_dual_data_kl (nsol_pdl.hip) on member m = blockIdx.y, expression for expression.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pdl_dual_data_kl_stack(
    T *q_all, const T *__restrict__ t_all, const T *__restrict__ bt_all,
    int64_t bt_stride, const T *__restrict__ wt_all, int64_t wt_stride, T sigma,
    const T *__restrict__ lmbda_all, T bg, int64_t n) {
  const int64_t m = blockIdx.y;
  T *q = q_all + m * n;
  const T *t = t_all ? t_all + m * n : nullptr;
  const T *bt = bt_all + m * bt_stride;
  const T *wt = wt_all ? wt_all + m * wt_stride : nullptr;
  const T lmbda = lmbda_all[m];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T w = wt ? wt[i] : T(1);
    const T v = t ? q[i] + sigma * (t[i] + bg) : q[i] + sigma * bg;
    q[i] = kl_dual_prox<T>(v, bt[i], w, sigma, lmbda);
  }
}

template <typename T>
int dual_data_kl_stack_impl(T *q, const T *t, const T *bt, int64_t bt_stride, const T *wt,
                            int64_t wt_stride, double sigma, const T *lmbda, double bg,
                            int members, int64_t n, void *stream) {
  if (n < 0) return NSOL_EINVAL;
  if (!pd_members_ok(members) || n > (int64_t(1) << 31) / members) return -2;
  if (n == 0) return 0;
  if (!q || !bt || !lmbda || q == t || !(sigma > 0.0) || !pd_stride_ok(bt_stride, n) ||
      (wt && !pd_stride_ok(wt_stride, n)) || !(isfinite(bg) && bg >= 0.0))
    return NSOL_EINVAL;
  const dim3 grid((unsigned)grid_for(n), (unsigned)members), block(kBlock);
  hipLaunchKernelGGL((k_pdl_dual_data_kl_stack<T>), grid, block, 0, as_stream(stream), q,
                     t, bt, bt_stride, wt, wt_stride, (T)sigma, lmbda, (T)bg, n);
  return launch_status();
}

}  // namespace

extern "C" {

int nsol_pdl_stack_launches(void) {
  return g_lin_stack_launches.load(std::memory_order_relaxed);
}

#define NSOL_PDLS_DEF(T, SUF)                                                          \
  int nsol_pdl_stack_dual_data_##SUF(T *q, const T *t, const T *bt, int64_t bt_stride, \
                                     const T *wt, int64_t wt_stride, double sigma,     \
                                     const T *lmbda, int l1, int members, int64_t n,   \
                                     void *s) {                                        \
    return dual_data_stack_impl<T>(q, t, bt, bt_stride, wt, wt_stride, sigma, lmbda,   \
                                   l1, members, n, s);                                 \
  }                                                                                    \
  int nsol_pdl_stack_dual_data_kl_##SUF(T *q, const T *t, const T *bt,                 \
                                        int64_t bt_stride, const T *wt,                \
                                        int64_t wt_stride, double sigma,               \
                                        const T *lmbda, double bg, int members,        \
                                        int64_t n, void *s) {                          \
    return dual_data_kl_stack_impl<T>(q, t, bt, bt_stride, wt, wt_stride, sigma,       \
                                      lmbda, bg, members, n, s);                       \
  }                                                                                    \
  int nsol_pdl_stack_iter_##SUF(const T *xi, T *xo, T *x, const T *g, const T *pi,     \
                                T *po, int members, int ndim, int64_t nz, int64_t ny,  \
                                int64_t nx, double wx, double wy, double wz,           \
                                double sigma, double hden, double tau, double theta,   \
                                double lo, double hi, int flags, int has_p, void *s) { \
    return lin_stack_iter_impl<T>(xi, xo, x, g, pi, po, members, ndim, nz, ny, nx, wx, \
                                  wy, wz, sigma, hden, tau, theta, lo, hi, flags,      \
                                  has_p, s);                                           \
  }

NSOL_PDLS_DEF(float, f32)
NSOL_PDLS_DEF(double, f64)
#undef NSOL_PDLS_DEF

}  // extern "C"
