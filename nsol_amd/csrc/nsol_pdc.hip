// The stopping rule of the primal-dual solver for gfx950 (MI355X): how much the
// iterates changed in one iteration,
//
//   r_x = sqrt(sum (x_k - x_{k-1})^2 / sum x_k^2),  r_p likewise for the dual p,
//
// as four float64 sums {sum dx^2, sum x^2, sum dp^2, sum p^2} in a row of a device
// board.  Every term is chk_add's (nsol_pd_common.hpp): ((double)new - (double)old)^2
// and (double)new^2 of the STORED values, so every form below adds the same summands
// and only the order of the sums differs.
//
// k_pd_check / k_pd_check_iso: ONE Chambolle-Pock iteration in one pass -- the tile
// bodies of k_pd_fused / k_pd_fused_iso / k_pd_w (pd_fused_tile, pd_fused_iso_tile)
// with CHK on.  At the point where a lane stores its results it holds the old and new
// x and the old and new p of its own voxels in registers, so the sums cost no byte of
// memory traffic.  The arrays it writes are the bits of the non-checking kernels: the
// sums are formed beside the iteration's arithmetic, which is untouched.
//
// k_pd_change: the same four sums from (x_old, x_new) and (p_old, p_new) in memory,
// for the loops of separate kernels.
//
// Reduction (nsol_pd_sums.hpp): wave shuffle, one partial per workgroup and sum in
// ws[sum * nparts + workgroup], then ONE closing workgroup that adds the partials in
// a fixed order into row[0..3].  No floating-point atomics: the same input gives the
// same bits on every run.
#include <stddef.h>

#include "nsol_common.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_fused_body.hpp"
#include "nsol_pd_iso_body.hpp"
#include "nsol_pd_launch.hpp"
#include "nsol_pd_sums.hpp"
#include "nsol_pd_weighted.hpp"

using namespace nsol;

namespace {

// the partials of every sum in a fixed order into row[0..3]; one workgroup
__global__ __launch_bounds__(kBlock) void k_pd_check_final(const double *__restrict__ ws,
                                                           int nparts,
                                                           double *__restrict__ row) {
  for (int k = 0; k < kPdSums; ++k) {
    const double t = pd_parts_sum(ws + (int64_t)k * nparts, nparts);
    if (threadIdx.x == 0) row[k] = t;
  }
}

// A workgroup without a tile (the XCD map rounds the grid up) leaves zeros: the
// closing workgroup adds every partial of the grid.
template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG, bool WGT>
__global__ __launch_bounds__(kBlock) void k_pd_check(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ wt, const T *__restrict__ p_in,
    T *__restrict__ p_out, Geom<T> G, PdScalars<T> S, int ntx, int nty, int zchunk,
    int slab, double *__restrict__ ws) {
  double a[kPdSums] = {0.0, 0.0, 0.0, 0.0};
  int tx, ty, zc;
  if (pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc))
    pd_fused_tile<T, VEC, LX, RY, NDIM, RAG, WGT, true>(xbar_in, xbar_out, x, bt, p_in,
                                                        p_out, G, S, tx, ty, zc, zchunk,
                                                        wt, a);
  pd_block_store(a, ws, (int)gridDim.x, 0);
}

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG, bool WGT>
__global__ __launch_bounds__(kBlock) void k_pd_check_iso(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ wt, const T *__restrict__ p_in,
    T *__restrict__ p_out, Geom<T> G, PdScalars<T> S, int ntx, int nty, int zchunk,
    int slab, double *__restrict__ ws) {
  double a[kPdSums] = {0.0, 0.0, 0.0, 0.0};
  int tx, ty, zc;
  if (pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc))
    pd_fused_iso_tile<T, VEC, LX, RY, NDIM, RAG, WGT, true>(xbar_in, xbar_out, x, bt,
                                                            p_in, p_out, G, S, tx, ty, zc,
                                                            zchunk, wt, a);
  pd_block_store(a, ws, (int)gridDim.x, 0);
}

// rows per lane: the knob "pd_ry" as k_pd_fused reads it (4 has no form here and
// falls to 2), else the automatic choice
template <int VEC, int LX, typename T>
int check_rows_per_lane(const Geom<T> &G, const PdLaunchTune &tune) {
  if (tune.ry == 0) return pd_auto_rows_per_lane<VEC, LX>(G, 1);
  return tune.ry == 1 ? 1 : 2;
}

// The launcher struct of nsol_pd_launch.hpp.
template <bool ISO, bool WGT>
struct CheckLauncher {
  template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
  static int launch_t(const PdLaunchArgs<T> &a) {
    const PdGridPlan g = pd_plan_grid<VEC, LX, RY>(a.G, 1, a.tune);
    if (g.blocks > kPdMaxBlocks) return -2;
    // one partial per workgroup and sum: the caller's workspace must hold them
    if (g.blocks > a.chk_ws_doubles / kPdSums) return NSOL_EINVAL;
    if constexpr (ISO)
      hipLaunchKernelGGL((k_pd_check_iso<T, VEC, LX, RY, NDIM, RAG, WGT>),
                         dim3((unsigned)g.blocks), dim3(kBlock), 0, a.st, a.xbar_in,
                         a.xbar_out, a.x, a.bt, a.wt, a.p_in, a.p_out, a.G, a.S, g.ntx,
                         g.nty, g.zchunk, g.slab, a.chk_ws);
    else
      hipLaunchKernelGGL((k_pd_check<T, VEC, LX, RY, NDIM, RAG, WGT>),
                         dim3((unsigned)g.blocks), dim3(kBlock), 0, a.st, a.xbar_in,
                         a.xbar_out, a.x, a.bt, a.wt, a.p_in, a.p_out, a.G, a.S, g.ntx,
                         g.nty, g.zchunk, g.slab, a.chk_ws);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_pd_check_final, dim3(1), dim3(kBlock), 0, a.st, a.chk_ws,
                       (int)g.blocks, a.chk_row);
    return launch_status();
  }

  template <typename T, int VEC, int LX, bool RAG>
  static int launch(const PdLaunchArgs<T> &a) {
    return pd_launch_forms<CheckLauncher<ISO, WGT>, T, VEC, LX, RAG>(
        a, check_rows_per_lane<VEC, LX>(a.G, a.tune));
  }
};

template <typename T>
int check_iter_impl(const T *xbar_in, T *xbar_out, T *x, const T *bt, const T *wt,
                    const T *p_in, T *p_out, int ndim, int64_t nz, int64_t ny, int64_t nx,
                    double wx, double wy, double wz, double sigma, double hden, double tau,
                    double tl, double theta, int flags, double *ws, int64_t ws_doubles,
                    double *row, void *stream) {
  if (!pd_stack_takes(1, ndim, nz, ny, nx)) return -2;
  const bool weighted = (flags & NSOL_PD_DATA_WEIGHTED) != 0;
  if (!xbar_in || !xbar_out || !x || !bt || !p_out || xbar_in == xbar_out ||
      p_in == p_out || !ws || !row || ws_doubles < kPdSums || weighted != (wt != nullptr))
    return NSOL_EINVAL;
  PdLaunchArgs<T> a{xbar_in, xbar_out, x, bt, p_in, p_out,
                    make_geom<T>(ndim, nz, ny, nx, wx, wy, wz),
                    pd_make_scalars<T>(sigma, hden, tau, tl, theta, flags,
                                       p_in != nullptr)};
  a.tune = pd_current_tune();
  a.st = as_stream(stream);
  a.wt = wt;
  a.chk_ws = ws;
  a.chk_ws_doubles = ws_doubles;
  a.chk_row = row;
  const bool iso = (flags & NSOL_PD_REG_ISOTROPIC) != 0;
  if (weighted)
    return iso ? pd_launch<CheckLauncher<true, true>>(a)
               : pd_launch<CheckLauncher<false, true>>(a);
  return iso ? pd_launch<CheckLauncher<true, false>>(a)
             : pd_launch<CheckLauncher<false, false>>(a);
}

// ---------------------------------------------------------------------------
// the stand-alone pass
// ---------------------------------------------------------------------------
// p_old == nullptr: p counts as zero (before the first iteration)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pd_change(
    const T *__restrict__ x_old, const T *__restrict__ x_new, int64_t n,
    const T *__restrict__ p_old, const T *__restrict__ p_new, int64_t np,
    double *__restrict__ ws) {
  double a[kPdSums] = {0.0, 0.0, 0.0, 0.0};
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  for (int64_t i = first; i < n; i += stride) chk_add(a[0], a[1], x_old[i], x_new[i]);
  for (int64_t i = first; i < np; i += stride)
    chk_add(a[2], a[3], p_old ? p_old[i] : T(0), p_new[i]);
  pd_block_store(a, ws, (int)gridDim.x, 0);
}

template <typename T>
int change_impl(const T *x_old, const T *x_new, int64_t n, const T *p_old, const T *p_new,
                int64_t np, double *ws, int64_t ws_doubles, double *row, void *stream) {
  if (!x_old || !x_new || !p_new || n < 1 || np < 1 || !ws || !row ||
      ws_doubles < kPdSums)
    return NSOL_EINVAL;
  int64_t g = grid_for(n > np ? n : np);
  if (g > ws_doubles / kPdSums) g = ws_doubles / kPdSums;
  hipLaunchKernelGGL(k_pd_change<T>, dim3((unsigned)g), dim3(kBlock), 0,
                     as_stream(stream), x_old, x_new, n, p_old, p_new, np, ws);
  int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(k_pd_check_final, dim3(1), dim3(kBlock), 0, as_stream(stream), ws,
                     (int)g, row);
  return launch_status();
}

}  // namespace

extern "C" {

int64_t nsol_pd_check_ws_doubles(int elem_size, int ndim, int64_t nz, int64_t ny,
                                 int64_t nx) {
  if ((elem_size != 4 && elem_size != 8) || !pd_stack_takes(1, ndim, nz, ny, nx))
    return -1;
  // the most workgroups a launch can ask for with the knobs as they stand
  const Geom<float> G = make_geom<float>(ndim, nz, ny, nx, 1.0, 1.0, 1.0);
  const PdLaunchTune tune = pd_current_tune();
  int64_t b = elem_size == 4 ? pd_max_blocks<4>(G, tune) : pd_max_blocks<2>(G, tune);
  // (nsol_pd_change_* never needs more than the grid-stride cap)
  if (b < kMaxGridBlocksLimit) b = kMaxGridBlocksLimit;
  return kPdSums * b;
}

#define NSOL_PDC_DEF(T, SUF)                                                           \
  int nsol_pd_check_iter_##SUF(const T *xi, T *xo, T *x, const T *bt, const T *wt,     \
                               const T *pi, T *po, int ndim, int64_t nz, int64_t ny,   \
                               int64_t nx, double wx, double wy, double wz,            \
                               double sigma, double hden, double tau, double tl,       \
                               double theta, int flags, double *ws, int64_t ws_doubles, \
                               double *row, void *s) {                                 \
    return check_iter_impl<T>(xi, xo, x, bt, wt, pi, po, ndim, nz, ny, nx, wx, wy, wz, \
                              sigma, hden, tau, tl, theta, flags, ws, ws_doubles, row, \
                              s);                                                      \
  }                                                                                    \
  int nsol_pd_change_##SUF(const T *x_old, const T *x_new, int64_t n, const T *p_old,  \
                           const T *p_new, int64_t np, double *ws, int64_t ws_doubles, \
                           double *row, void *s) {                                     \
    return change_impl<T>(x_old, x_new, n, p_old, p_new, np, ws, ws_doubles, row, s);  \
  }

NSOL_PDC_DEF(float, f32)
NSOL_PDC_DEF(double, f64)
#undef NSOL_PDC_DEF

}  // extern "C"
