// Chambolle-Pock iteration with a WEIGHTED data term for gfx950 (MI355X):
// lambda/2 sum w_i (x_i - b_i)^2 or lambda sum w_i |x_i - b_i| with per-voxel weights
// w_i >= 0 -- a mask (w in {0, 1}: inpainting, a region of interest, dead detector
// rows) or a confidence map.
//
// reference: primal_dual_solver.py:232-261 with prox_f the weighted form of
// proximal_operators.py:95-98 / 117-120 (the reference has the unweighted two only).
//
// One member-stacked one-iteration kernel family, k_pd_w / k_pd_w_iso: everything is
// k_pd_batch's (nsol_pdb.hip) -- the member is blockIdx.y, the scalars are the row
// PdScalars[iteration][member] of a device table, the tile bodies are pd_fused_tile /
// pd_fused_iso_tile -- except that the bodies run with WGT on (one more 16-byte row
// load per plane, prox_data_w of nsol_pd_weighted.hpp in place of prox_data) and that
// bt and wt each take a MEMBER STRIDE of 0 or n: a single run is members = 1, a
// parameter sweep shares both arrays (stride 0), a stack of images brings its own of
// each (stride n).  48 bytes per voxel and iteration in 3-D float32 where k_pd_fused
// moves 44.
//
// The stand-alone kernels k_prox_w (nsol_prox_ell2_weighted_* / _ell1_) are what the
// generic device loop and NumPy callers run; they call the same prox_data_w, so the
// fused run and the loop of separate kernels give the same bits.
#include <atomic>

#include "nsol_common.hpp"
#include "nsol_kl.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_fused_body.hpp"
#include "nsol_pd_iso_body.hpp"
#include "nsol_pd_launch.hpp"
#include "nsol_pd_weighted.hpp"

using namespace nsol;

namespace {

std::atomic<int> g_weighted_launches{0};

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_pd_w(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ wt, const T *__restrict__ p_in,
    T *__restrict__ p_out, Geom<T> G, const PdScalars<T> *__restrict__ tab,
    int64_t bt_stride, int64_t wt_stride, int ntx, int nty, int zchunk, int slab) {
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  // gridDim.y = members: the row of this iteration starts at `tab`
  const int64_t m = blockIdx.y;
  const PdScalars<T> S = tab[m];           // uniform per workgroup, read-only
  const int64_t xo = m * G.n;
  const int64_t po = m * G.n * NDIM;
  pd_fused_tile<T, VEC, LX, RY, NDIM, RAG, true>(
      xbar_in + xo, xbar_out + xo, x + xo, bt + m * bt_stride, p_in + po, p_out + po, G,
      S, tx, ty, zc, zchunk, wt + m * wt_stride);
}

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_pd_w_iso(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ wt, const T *__restrict__ p_in,
    T *__restrict__ p_out, Geom<T> G, const PdScalars<T> *__restrict__ tab,
    int64_t bt_stride, int64_t wt_stride, int ntx, int nty, int zchunk, int slab) {
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  const int64_t m = blockIdx.y;
  const PdScalars<T> S = tab[m];
  const int64_t xo = m * G.n;
  const int64_t po = m * G.n * NDIM;
  pd_fused_iso_tile<T, VEC, LX, RY, NDIM, RAG, true>(
      xbar_in + xo, xbar_out + xo, x + xo, bt + m * bt_stride, p_in + po, p_out + po, G,
      S, tx, ty, zc, zchunk, wt + m * wt_stride);
}

// The launcher struct of nsol_pd_launch.hpp: the members count as tiles in the grid
// and in the rows per lane.
template <bool ISO>
struct WeightedLauncher {
  template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
  static int launch_t(const PdLaunchArgs<T> &a) {
    const PdGridPlan g = pd_plan_grid<VEC, LX, RY>(a.G, a.members, a.tune);
    if (g.blocks > kPdMaxBlocks) return -2;   // (the caller runs the members one by one)
    const dim3 grid((unsigned)g.blocks, (unsigned)a.members);
    if constexpr (ISO)
      hipLaunchKernelGGL((k_pd_w_iso<T, VEC, LX, RY, NDIM, RAG>), grid, dim3(kBlock), 0,
                         a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.wt, a.p_in, a.p_out,
                         a.G, a.row, a.bt_stride, a.wt_stride, g.ntx, g.nty, g.zchunk,
                         g.slab);
    else
      hipLaunchKernelGGL((k_pd_w<T, VEC, LX, RY, NDIM, RAG>), grid, dim3(kBlock), 0, a.st,
                         a.xbar_in, a.xbar_out, a.x, a.bt, a.wt, a.p_in, a.p_out, a.G,
                         a.row, a.bt_stride, a.wt_stride, g.ntx, g.nty, g.zchunk, g.slab);
    const int rc = launch_status();
    if (rc == 0) g_weighted_launches.fetch_add(1, std::memory_order_relaxed);
    return rc;
  }

  template <typename T, int VEC, int LX, bool RAG>
  static int launch(const PdLaunchArgs<T> &a) {
    return pd_launch_forms<WeightedLauncher<ISO>, T, VEC, LX, RAG>(
        a, pd_auto_rows_per_lane<VEC, LX>(a.G, a.members));
  }
};

template <typename T>
int weighted_iter_impl(const T *xbar_in, T *xbar_out, T *x, const T *bt, int64_t bt_stride,
                       const T *wt, int64_t wt_stride, const T *p_in, T *p_out,
                       int members, int ndim, int64_t nz, int64_t ny, int64_t nx,
                       double wx, double wy, double wz, const void *tab, int iteration,
                       int flags, void *stream) {
  if (!pd_stack_takes(members, ndim, nz, ny, nx)) return -2;
  const int64_t n = nz * ny * nx;
  if (!xbar_in || !xbar_out || !x || !bt || !wt || !p_in || !p_out || !tab ||
      iteration < 0 || xbar_in == xbar_out || p_in == p_out ||
      !(flags & NSOL_PD_DATA_WEIGHTED) || !pd_stride_ok(bt_stride, n) ||
      !pd_stride_ok(wt_stride, n))
    return NSOL_EINVAL;
  // (with whole vectors n is a multiple of the vector, so every member's slice of
  // bt and wt starts a whole number of vectors behind its base, as x's does)
  PdLaunchArgs<T> a{xbar_in, xbar_out, x, bt, p_in, p_out,
                    make_geom<T>(ndim, nz, ny, nx, wx, wy, wz)};
  a.row = static_cast<const PdScalars<T> *>(tab) + (int64_t)iteration * members;
  a.members = members;    // (the pd_* knobs do not reach the stack: kPdStackTune)
  a.st = as_stream(stream);
  a.wt = wt;
  a.bt_stride = bt_stride;
  a.wt_stride = wt_stride;
  if (flags & NSOL_PD_REG_ISOTROPIC) return pd_launch<WeightedLauncher<true>>(a);
  return pd_launch<WeightedLauncher<false>>(a);
}

// The table [iteration][member], rounded as a single run's scalars are
// (pd_make_scalars), uploaded once on the stream.
template <typename T>
int weighted_table_impl(int members, const double *lmbda, const double *sig,
                        const double *tau, const double *theta, int iterations,
                        int p_is_zero, double gamma_huber, int flags, void *tab_host,
                        void *tab, int64_t tab_bytes, void *stream) {
  if (!pd_members_ok(members)) return -2;
  return pd_table_fill_upload<T>(members, lmbda, sig, tau, theta, iterations, p_is_zero,
                                 gamma_huber, flags, tab_host, tab, tab_bytes,
                                 as_stream(stream));
}

template <typename T>
int weighted_run_impl(T *xbar0, T *xbar1, T *x, const T *bt, int64_t bt_stride,
                      const T *wt, int64_t wt_stride, T *p0, T *p1, int members, int ndim,
                      int64_t nz, int64_t ny, int64_t nx, double wx, double wy, double wz,
                      const double *lmbda, const double *sig, const double *tau,
                      const double *theta, int iterations, int p_is_zero,
                      double gamma_huber, int flags, void *tab_host, void *tab,
                      int64_t tab_bytes, int *final_slot, void *stream) {
  if (!pd_stack_takes(members, ndim, nz, ny, nx)) return -2;
  const int64_t n = nz * ny * nx;
  // everything the launches check, before the table is written or uploaded
  if (!xbar0 || !xbar1 || !x || !bt || !wt || !p0 || !p1 || xbar0 == xbar1 || p0 == p1 ||
      !(flags & NSOL_PD_DATA_WEIGHTED) || !pd_stride_ok(bt_stride, n) ||
      !pd_stride_ok(wt_stride, n))
    return NSOL_EINVAL;
  const int rc = weighted_table_impl<T>(members, lmbda, sig, tau, theta, iterations,
                                        p_is_zero, gamma_huber, flags, tab_host, tab,
                                        tab_bytes, stream);
  if (rc) return rc;
  T *xb[2] = {xbar0, xbar1};
  T *pp[2] = {p0, p1};
  return pd_ping_pong(iterations, final_slot, [&](int it, int slot) {
    return weighted_iter_impl<T>(xb[slot], xb[slot ^ 1], x, bt, bt_stride, wt, wt_stride,
                                 pp[slot], pp[slot ^ 1], members, ndim, nz, ny, nx, wx, wy,
                                 wz, tab, it, flags, stream);
  });
}

// ---------------------------------------------------------------------------
// the stand-alone weighted prox
// ---------------------------------------------------------------------------
// out may be x (every element is read before it is written by the same thread)
template <typename T, bool L1>
__global__ __launch_bounds__(kBlock) void k_prox_w(T *out, const T *x,
                                                   const T *__restrict__ bt,
                                                   const T *__restrict__ wt, T tl,
                                                   int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = prox_data_w<T>(x[i], bt[i], wt[i], tl, L1);
}

template <typename T, bool L1>
int prox_w_impl(T *out, const T *x, const T *bt, const T *wt, double tau, int64_t n,
                void *stream) {
  if (n < 0) return NSOL_EINVAL;
  if (n == 0) return 0;
  if (!out || !x || !bt || !wt) return NSOL_EINVAL;
  hipLaunchKernelGGL((k_prox_w<T, L1>), dim3(grid_for(n)), dim3(kBlock), 0,
                     as_stream(stream), out, x, bt, wt, (T)tau, n);
  return launch_status();
}

// The prox of the Poisson (Kullback-Leibler) data term, prox_kl of nsol_kl.hpp; wt may
// be null (all 1), a uniform branch on the pointer.  out may be x, as above.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_prox_kl(T *out, const T *x,
                                                    const T *__restrict__ bt,
                                                    const T *__restrict__ wt, T tl,
                                                    int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = prox_kl<T>(x[i], bt[i], wt ? wt[i] : T(1), tl);
}

template <typename T>
int prox_kl_impl(T *out, const T *x, const T *bt, const T *wt, double tl, int64_t n,
                 void *stream) {
  if (n < 0) return NSOL_EINVAL;
  if (n == 0) return 0;
  if (!out || !x || !bt || !(isfinite(tl) && tl >= 0.0)) return NSOL_EINVAL;
  hipLaunchKernelGGL((k_prox_kl<T>), dim3(grid_for(n)), dim3(kBlock), 0,
                     as_stream(stream), out, x, bt, wt, (T)tl, n);
  return launch_status();
}

}  // namespace

extern "C" {

int nsol_pd_weighted_launches(void) {
  return g_weighted_launches.load(std::memory_order_relaxed);
}

#define NSOL_PDW_DEF(T, SUF)                                                           \
  int nsol_prox_ell2_weighted_##SUF(T *out, const T *x, const T *bt, const T *wt,      \
                                    double tau, int64_t n, void *s) {                  \
    return prox_w_impl<T, false>(out, x, bt, wt, tau, n, s);                           \
  }                                                                                    \
  int nsol_prox_kl_##SUF(T *out, const T *x, const T *bt, const T *wt, double tl,      \
                         int64_t n, void *s) {                                         \
    return prox_kl_impl<T>(out, x, bt, wt, tl, n, s);                                  \
  }                                                                                    \
  int nsol_prox_ell1_weighted_##SUF(T *out, const T *x, const T *bt, const T *wt,      \
                                    double tau, int64_t n, void *s) {                  \
    return prox_w_impl<T, true>(out, x, bt, wt, tau, n, s);                            \
  }                                                                                    \
  int nsol_pd_weighted_table_##SUF(int members, const double *lm, const double *sg,    \
                                   const double *ta, const double *th, int iters,      \
                                   int p_is_zero, double gh, int flags, void *tab_host, \
                                   void *tab, int64_t tab_bytes, void *s) {            \
    return weighted_table_impl<T>(members, lm, sg, ta, th, iters, p_is_zero, gh, flags, \
                                  tab_host, tab, tab_bytes, s);                        \
  }                                                                                    \
  int nsol_pd_weighted_iter_##SUF(const T *xi, T *xo, T *x, const T *bt,               \
                                  int64_t bt_stride, const T *wt, int64_t wt_stride,   \
                                  const T *pi, T *po, int members, int ndim,           \
                                  int64_t nz, int64_t ny, int64_t nx, double wx,       \
                                  double wy, double wz, const void *tab, int iteration, \
                                  int flags, void *s) {                                \
    return weighted_iter_impl<T>(xi, xo, x, bt, bt_stride, wt, wt_stride, pi, po,      \
                                 members, ndim, nz, ny, nx, wx, wy, wz, tab, iteration, \
                                 flags, s);                                            \
  }                                                                                    \
  int nsol_pd_weighted_run_##SUF(T *xb0, T *xb1, T *x, const T *bt, int64_t bt_stride, \
                                 const T *wt, int64_t wt_stride, T *p0, T *p1,         \
                                 int members, int ndim, int64_t nz, int64_t ny,        \
                                 int64_t nx, double wx, double wy, double wz,          \
                                 const double *lm, const double *sg, const double *ta, \
                                 const double *th, int iters, int p_is_zero, double gh, \
                                 int flags, void *tab_host, void *tab,                 \
                                 int64_t tab_bytes, int *final_slot, void *s) {        \
    return weighted_run_impl<T>(xb0, xb1, x, bt, bt_stride, wt, wt_stride, p0, p1,     \
                                members, ndim, nz, ny, nx, wx, wy, wz, lm, sg, ta, th, \
                                iters, p_is_zero, gh, flags, tab_host, tab, tab_bytes, \
                                final_slot, s);                                        \
  }

NSOL_PDW_DEF(float, f32)
NSOL_PDW_DEF(double, f64)
#undef NSOL_PDW_DEF

}  // extern "C"
