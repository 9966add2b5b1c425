// Chambolle-Pock iteration with the ISOTROPIC total variation / Huber dual
// projection for gfx950 (MI355X): p = q / max(1, |q|_2) per voxel, |q|_2 the
// Euclidean norm of the stacked gradient vector.
//
// reference: the loop is primal_dual_solver.py:232-261; the vector norm is the one
// admm_linear_solver.py:239-253 shrinks by and prior_measures.py:27-52 reports
// (the reference's own prox_tv_conj, proximal_operators.py:138-140, clamps every
// component on its own -- the anisotropic form of nsol_pd.hip).
//
// Three kernels with the same per-voxel arithmetic (operation order of
// dual_project, nsol_pd_iso_body.hpp; IEEE sqrt and division, no contraction):
//   * k_prox_dual_project: the stand-alone prox, one pass, 8 dim bytes per voxel;
//   * k_dual_step_iso: the dual half of the two-pass form;
//   * k_pd_fused_iso: ONE pass per iteration, 11 words per voxel, the layout of
//     k_pd_fused (nsol_pd.hip) with the lower halo's whole dual vectors
//     recomputed (nsol_pd_iso_body.hpp).
#include "nsol_common.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_iso_body.hpp"
#include "nsol_pd_launch.hpp"

using namespace nsol;

namespace {

// ---------------------------------------------------------------------------
// stand-alone prox
// ---------------------------------------------------------------------------
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_prox_dual_project(
    T *out, const T *x, int64_t n, T hden, bool huber) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    T q0 = x[i], q1 = T(0), q2 = T(0);
    if constexpr (DIM >= 2) q1 = x[n + i];
    if constexpr (DIM >= 3) q2 = x[2 * n + i];
    dual_project<DIM>(q0, q1, q2, huber, hden);
    out[i] = q0;
    if constexpr (DIM >= 2) out[n + i] = q1;
    if constexpr (DIM >= 3) out[2 * n + i] = q2;
  }
}

template <typename T>
int prox_dual_project_impl(T *out, const T *x, double den, int64_t n, int dim,
                           void *stream) {
  if (!out || !x || n < 1 || dim < 1 || dim > 3) return NSOL_EINVAL;
  const T hd = huber_den<T>(den);
  const bool huber = den != 1.0;
  hipStream_t st = as_stream(stream);
  const dim3 grid(grid_for(n)), block(kBlock);
  switch (dim) {
    case 1: hipLaunchKernelGGL((k_prox_dual_project<T, 1>), grid, block, 0, st, out, x, n, hd, huber); break;
    case 2: hipLaunchKernelGGL((k_prox_dual_project<T, 2>), grid, block, 0, st, out, x, n, hd, huber); break;
    default: hipLaunchKernelGGL((k_prox_dual_project<T, 3>), grid, block, 0, st, out, x, n, hd, huber); break;
  }
  return launch_status();
}

// ---------------------------------------------------------------------------
// two-pass form: the dual half (the primal half is nsol_pd.hip's k_primal_step)
// ---------------------------------------------------------------------------
template <typename T, int NDIM>
__global__ __launch_bounds__(kBlock) void k_dual_step_iso(
    const T *__restrict__ xbar, const T *p_in, T *p_out, Geom<T> G, T sigma,
    T hden, bool huber) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G.n;
       i += stride) {
    const int64_t ix = i % G.nx;
    const int64_t r = i / G.nx;
    const T c = xbar[i];
    const T hx = (ix + 1 < G.nx) ? xbar[i + 1] : T(0);
    T q0 = dual_q(p_in ? p_in[i] : T(0), hx, c, G.wx, sigma), q1 = T(0), q2 = T(0);
    if constexpr (NDIM >= 2) {
      const T hy = (r % G.ny + 1 < G.ny) ? xbar[i + G.sy] : T(0);
      q1 = dual_q(p_in ? p_in[G.n + i] : T(0), hy, c, G.wy, sigma);
    }
    if constexpr (NDIM >= 3) {
      const T hz = (r / G.ny + 1 < G.nz) ? xbar[i + G.sz] : T(0);
      q2 = dual_q(p_in ? p_in[2 * G.n + i] : T(0), hz, c, G.wz, sigma);
    }
    dual_project<NDIM>(q0, q1, q2, huber, hden);
    p_out[i] = q0;
    if constexpr (NDIM >= 2) p_out[G.n + i] = q1;
    if constexpr (NDIM >= 3) p_out[2 * G.n + i] = q2;
  }
}

// ---------------------------------------------------------------------------
// single-pass fused form
// ---------------------------------------------------------------------------
template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG = false>
__global__ __launch_bounds__(kBlock) void k_pd_fused_iso(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ p_in,
    T *__restrict__ p_out, Geom<T> G, PdScalars<T> S, int ntx, int nty,
    int zchunk, int slab) {
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  pd_fused_iso_tile<T, VEC, LX, RY, NDIM, RAG>(xbar_in, xbar_out, x, bt, p_in, p_out, G,
                                               S, tx, ty, zc, zchunk);
}

struct IsoKernel {
  template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
  static int launch_t(const PdLaunchArgs<T> &a) {
    const PdGridPlan g = pd_plan_grid<VEC, LX, RY>(a.G, 1, a.tune);
    if (g.blocks > kPdMaxBlocks) return NSOL_EINVAL;
    hipLaunchKernelGGL((k_pd_fused_iso<T, VEC, LX, RY, NDIM, RAG>), dim3((unsigned)g.blocks),
                       dim3(kBlock), 0, a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.p_in,
                       a.p_out, a.G, a.S, g.ntx, g.nty, g.zchunk, g.slab);
    return launch_status();
  }

  // knob "pd_ry": 1 or 2 rows per lane, any other value = choose
  template <typename T, int VEC, int LX, bool RAG>
  static int launch(const PdLaunchArgs<T> &a) {
    int ry = a.tune.ry;
    if (ry != 1 && ry != 2) ry = pd_auto_rows_per_lane<VEC, LX>(a.G, 1);
    switch (a.G.ndim) {
      case 1: return launch_t<T, VEC, LX, 1, 1, RAG>(a);
      case 2:
        if (ry == 1) return launch_t<T, VEC, LX, 1, 2, RAG>(a);
        return launch_t<T, VEC, LX, 2, 2, RAG>(a);
      default:
        if (ry == 1) return launch_t<T, VEC, LX, 1, 3, RAG>(a);
        return launch_t<T, VEC, LX, 2, 3, RAG>(a);
    }
  }
};

}  // namespace

namespace nsol {

template <typename T>
int pd_iso_fused_iter(const T *xbar_in, T *xbar_out, T *x, const T *bt, const T *p_in,
                      T *p_out, int ndim, int64_t nz, int64_t ny, int64_t nx, double wx,
                      double wy, double wz, double sigma, double hden, double tau,
                      double tl, double theta, int flags, void *stream, int64_t pitch,
                      PdLaunchTune tune) {
  NSOL_CHECK_GEOM(ndim, nz, ny, nx);
  if (!xbar_in || !xbar_out || !x || !bt || !p_out || xbar_in == xbar_out ||
      p_in == p_out)
    return NSOL_EINVAL;
  PdLaunchArgs<T> a{xbar_in, xbar_out, x, bt, p_in, p_out,
                    make_geom_pitched<T>(ndim, nz, ny, nx, pitch, wx, wy, wz),
                    pd_make_scalars<T>(sigma, hden, tau, tl, theta, flags, p_in != nullptr)};
  a.tune = tune;
  a.st = as_stream(stream);
  return pd_launch<IsoKernel>(a);
}

template <typename T>
int pd_iso_dual_step(const T *xbar, const T *p_in, T *p_out, int ndim, int64_t nz,
                     int64_t ny, int64_t nx, double wx, double wy, double wz,
                     double sigma, double hden, void *stream) {
  NSOL_CHECK_GEOM(ndim, nz, ny, nx);
  if (!xbar || !p_out) return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  const dim3 grid(grid_for(G.n)), block(kBlock);
  hipStream_t st = as_stream(stream);
  const T sg = (T)sigma, hd = huber_den<T>(hden);
  const bool huber = hden != 1.0;
  switch (ndim) {
    case 1: hipLaunchKernelGGL((k_dual_step_iso<T, 1>), grid, block, 0, st, xbar, p_in, p_out, G, sg, hd, huber); break;
    case 2: hipLaunchKernelGGL((k_dual_step_iso<T, 2>), grid, block, 0, st, xbar, p_in, p_out, G, sg, hd, huber); break;
    default: hipLaunchKernelGGL((k_dual_step_iso<T, 3>), grid, block, 0, st, xbar, p_in, p_out, G, sg, hd, huber); break;
  }
  return launch_status();
}

#define NSOL_PDI_INST(T)                                                              \
  template int pd_iso_fused_iter<T>(const T *, T *, T *, const T *, const T *, T *,   \
                                    int, int64_t, int64_t, int64_t, double, double,   \
                                    double, double, double, double, double, double,   \
                                    int, void *, int64_t, PdLaunchTune);              \
  template int pd_iso_dual_step<T>(const T *, const T *, T *, int, int64_t, int64_t,  \
                                   int64_t, double, double, double, double, double,   \
                                   void *);
NSOL_PDI_INST(float)
NSOL_PDI_INST(double)
#undef NSOL_PDI_INST

}  // namespace nsol

extern "C" {

#define NSOL_PDI_DEF(T, SUF)                                                          \
  int nsol_prox_dual_project_##SUF(T *out, const T *x, double den,                    \
                                   int64_t n_per_block, int dim, void *s) {           \
    return prox_dual_project_impl<T>(out, x, den, n_per_block, dim, s);               \
  }                                                                                   \
  int nsol_pd_dual_step_iso_##SUF(const T *xbar, const T *p_in, T *p_out, int ndim,   \
                                  int64_t nz, int64_t ny, int64_t nx, double wx,      \
                                  double wy, double wz, double sigma, double hden,    \
                                  void *s) {                                          \
    return pd_iso_dual_step<T>(xbar, p_in, p_out, ndim, nz, ny, nx, wx, wy, wz,       \
                               sigma, hden, s);                                       \
  }
NSOL_PDI_DEF(float, f32)
NSOL_PDI_DEF(double, f64)
#undef NSOL_PDI_DEF

}  // extern "C"
