// Image-stacked Chambolle-Pock iteration for gfx950 (MI355X): P independent
// primal-dual runs on P DIFFERENT observations of one shape (the slices of a stack
// denoised slice by slice, a batch of images, a set of small volumes) advance by
// one iteration in one launch.
//
// reference: primal_dual_solver.py:232-261, looped over the images by its caller
// (run_denoising.py builds one solver per observation).
//
// What differs from the parameter sweep's k_pd_sweep (nsol_pds.hip) is the
// observation: every member has its own, so the member index blockIdx.y offsets bt
// as well (bt[m n + i]).  The arithmetic is the single-volume kernels': k_pd_batch
// runs pd_fused_tile (nsol_pd_fused_body.hpp), k_pd_batch_iso pd_fused_iso_tile
// (nsol_pd_iso_body.hpp), each on the member's own slice with the member-local
// geometry G, so member m is bit-identical to a single run with that member's data
// and scalars.  The tile bodies decide every boundary from G (x0 > 0, y0 > 0,
// zbeg > 0, z + 1 < nz ...), never from an address: a member's first row and plane
// have no neighbour in the member before it, and the isotropic lower halo is
// recomputed inside the member's slice exactly as k_pd_fused_iso recomputes it.
//
// k_scale_rows is the set-up's companion: row m of a (P, n) array divided or
// multiplied by the member's own scale s[m], one launch for the stack.
#include <atomic>

#include "nsol_common.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_fused_body.hpp"
#include "nsol_pd_iso_body.hpp"
#include "nsol_pd_launch.hpp"

using namespace nsol;

namespace {

std::atomic<int> g_batch_launches{0};

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_pd_batch(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ p_in, T *__restrict__ p_out,
    Geom<T> G, const PdScalars<T> *__restrict__ tab, int ntx, int nty, int zchunk,
    int slab) {
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  // gridDim.y = members: the row of this iteration starts at `tab`
  const int64_t m = blockIdx.y;
  const PdScalars<T> S = tab[m];           // uniform per workgroup, read-only
  const int64_t xo = m * G.n;
  const int64_t po = m * G.n * NDIM;
  pd_fused_tile<T, VEC, LX, RY, NDIM, RAG>(xbar_in + xo, xbar_out + xo, x + xo, bt + xo,
                                           p_in + po, p_out + po, G, S, tx, ty, zc,
                                           zchunk);
}

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_pd_batch_iso(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ p_in, T *__restrict__ p_out,
    Geom<T> G, const PdScalars<T> *__restrict__ tab, int ntx, int nty, int zchunk,
    int slab) {
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  const int64_t m = blockIdx.y;
  const PdScalars<T> S = tab[m];
  const int64_t xo = m * G.n;
  const int64_t po = m * G.n * NDIM;
  pd_fused_iso_tile<T, VEC, LX, RY, NDIM, RAG>(xbar_in + xo, xbar_out + xo, x + xo,
                                               bt + xo, p_in + po, p_out + po, G, S, tx,
                                               ty, zc, zchunk);
}

// The launcher structs of nsol_pd_launch.hpp: the members count as tiles in the grid
// and in the rows per lane.
template <bool ISO>
struct BatchLauncher {
  template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
  static int launch_t(const PdLaunchArgs<T> &a) {
    const PdGridPlan g = pd_plan_grid<VEC, LX, RY>(a.G, a.members, a.tune);
    if (g.blocks > kPdMaxBlocks) return -2;   // (the caller runs the members one by one)
    const dim3 grid((unsigned)g.blocks, (unsigned)a.members);
    if constexpr (ISO)
      hipLaunchKernelGGL((k_pd_batch_iso<T, VEC, LX, RY, NDIM, RAG>), grid, dim3(kBlock),
                         0, a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.p_in, a.p_out, a.G,
                         a.row, g.ntx, g.nty, g.zchunk, g.slab);
    else
      hipLaunchKernelGGL((k_pd_batch<T, VEC, LX, RY, NDIM, RAG>), grid, dim3(kBlock), 0,
                         a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.p_in, a.p_out, a.G,
                         a.row, g.ntx, g.nty, g.zchunk, g.slab);
    const int rc = launch_status();
    if (rc == 0) g_batch_launches.fetch_add(1, std::memory_order_relaxed);
    return rc;
  }

  template <typename T, int VEC, int LX, bool RAG>
  static int launch(const PdLaunchArgs<T> &a) {
    return pd_launch_forms<BatchLauncher<ISO>, T, VEC, LX, RAG>(
        a, pd_auto_rows_per_lane<VEC, LX>(a.G, a.members));
  }
};
using BatchKernel = BatchLauncher<false>;
using BatchIsoKernel = BatchLauncher<true>;

template <typename T>
int batch_iter_impl(const T *xbar_in, T *xbar_out, T *x, const T *bt, const T *p_in,
                    T *p_out, int members, int ndim, int64_t nz, int64_t ny, int64_t nx,
                    double wx, double wy, double wz, const void *tab, int iteration,
                    int flags, void *stream) {
  if (flags & NSOL_PD_DATA_WEIGHTED) return -2;   // no weights pointer here: nsol_pdw.hip
  if (!pd_stack_takes(members, ndim, nz, ny, nx)) return -2;
  if (!xbar_in || !xbar_out || !x || !bt || !p_in || !p_out || !tab || iteration < 0 ||
      xbar_in == xbar_out || p_in == p_out)
    return NSOL_EINVAL;
  PdLaunchArgs<T> a{xbar_in, xbar_out, x, bt, p_in, p_out,
                    make_geom<T>(ndim, nz, ny, nx, wx, wy, wz)};
  a.row = static_cast<const PdScalars<T> *>(tab) + (int64_t)iteration * members;
  a.members = members;    // (the pd_* knobs do not reach the stack: kPdStackTune)
  a.st = as_stream(stream);
  if (flags & NSOL_PD_REG_ISOTROPIC) return pd_launch<BatchIsoKernel>(a);
  return pd_launch<BatchKernel>(a);
}

template <typename T>
int batch_run_impl(T *xbar0, T *xbar1, T *x, const T *bt, T *p0, T *p1, int members,
                   int ndim, int64_t nz, int64_t ny, int64_t nx, double wx, double wy,
                   double wz, const double *lmbda, const double *sig, const double *tau,
                   const double *theta, int iterations, int p_is_zero, double gamma_huber,
                   int flags, void *tab_host, void *tab, int64_t tab_bytes,
                   int *final_slot, void *stream) {
  if (flags & NSOL_PD_DATA_WEIGHTED) return -2;   // no weights pointer here: nsol_pdw.hip
  if (!pd_stack_takes(members, ndim, nz, ny, nx)) return -2;
  // the table, [iteration][member], rounded as a single run's scalars are
  const int rc = pd_table_fill_upload<T>(members, lmbda, sig, tau, theta, iterations,
                                         p_is_zero, gamma_huber, flags, tab_host, tab,
                                         tab_bytes, as_stream(stream));
  if (rc) return rc;
  T *xb[2] = {xbar0, xbar1};
  T *pp[2] = {p0, p1};
  return pd_ping_pong(iterations, final_slot, [&](int n, int slot) {
    return batch_iter_impl<T>(xb[slot], xb[slot ^ 1], x, bt, pp[slot], pp[slot ^ 1],
                              members, ndim, nz, ny, nx, wx, wy, wz, tab, n, flags,
                              stream);
  });
}

// ---------------------------------------------------------------------------
// rows of a (members, n) array by their own scales
// ---------------------------------------------------------------------------
// out[m n + i] = in[m n + i] / or * s[m], formed in TIN with the scale rounded to
// TIN first -- nsol_scale_*'s arithmetic when TIN == TOUT -- and rounded once to
// TOUT: float64 -> float32 is how the scaled observation is made from float64 data.
template <typename TIN, typename TOUT, bool DIVIDE>
__global__ __launch_bounds__(kBlock) void k_scale_rows(TOUT *__restrict__ out,
                                                       const TIN *__restrict__ in,
                                                       const double *__restrict__ s,
                                                       int64_t n) {
  const int64_t m = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const TIN *src = in + m * n;
  TOUT *dst = out + m * n;
  const TIN a = (TIN)s[m];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    dst[i] = (TOUT)(DIVIDE ? src[i] / a : src[i] * a);
}

template <typename TIN, typename TOUT>
int scale_rows_impl(TOUT *out, const TIN *in, const double *s, int divide, int members,
                    int64_t n, void *stream) {
  if (members < 0 || n < 0 || members > 65535) return NSOL_EINVAL;
  if (members == 0 || n == 0) return 0;
  if (!out || !in || !s) return NSOL_EINVAL;
  const dim3 grid((unsigned)grid_for(n), (unsigned)members), block(kBlock);
  hipStream_t st = as_stream(stream);
  if (divide)
    hipLaunchKernelGGL((k_scale_rows<TIN, TOUT, true>), grid, block, 0, st, out, in, s, n);
  else
    hipLaunchKernelGGL((k_scale_rows<TIN, TOUT, false>), grid, block, 0, st, out, in, s, n);
  return launch_status();
}

}  // namespace

extern "C" {

int nsol_pd_batch_launches(void) {
  return g_batch_launches.load(std::memory_order_relaxed);
}

int nsol_scale_rows_f32(float *out, const float *in, const double *s, int divide,
                        int members, int64_t n, void *stream) {
  return scale_rows_impl<float, float>(out, in, s, divide, members, n, stream);
}

int nsol_scale_rows_f64(double *out, const double *in, const double *s, int divide,
                        int members, int64_t n, void *stream) {
  return scale_rows_impl<double, double>(out, in, s, divide, members, n, stream);
}

int nsol_scale_rows_f64_to_f32(float *out, const double *in, const double *s, int divide,
                               int members, int64_t n, void *stream) {
  return scale_rows_impl<double, float>(out, in, s, divide, members, n, stream);
}

#define NSOL_PDB_DEF(T, SUF)                                                          \
  int nsol_pd_batch_iter_##SUF(const T *xi, T *xo, T *x, const T *bt, const T *pi,    \
                               T *po, int members, int ndim, int64_t nz, int64_t ny,  \
                               int64_t nx, double wx, double wy, double wz,           \
                               const void *tab, int iteration, int flags, void *s) {  \
    return batch_iter_impl<T>(xi, xo, x, bt, pi, po, members, ndim, nz, ny, nx, wx,   \
                              wy, wz, tab, iteration, flags, s);                      \
  }                                                                                   \
  int nsol_pd_batch_run_##SUF(T *xb0, T *xb1, T *x, const T *bt, T *p0, T *p1,        \
                              int members, int ndim, int64_t nz, int64_t ny,          \
                              int64_t nx, double wx, double wy, double wz,            \
                              const double *lm, const double *sg, const double *ta,   \
                              const double *th, int iters, int p_is_zero, double gh,  \
                              int flags, void *tab_host, void *tab, int64_t tab_bytes, \
                              int *final_slot, void *s) {                             \
    return batch_run_impl<T>(xb0, xb1, x, bt, p0, p1, members, ndim, nz, ny, nx, wx,  \
                             wy, wz, lm, sg, ta, th, iters, p_is_zero, gh, flags,     \
                             tab_host, tab, tab_bytes, final_slot, s);                \
  }

NSOL_PDB_DEF(float, f32)
NSOL_PDB_DEF(double, f64)
#undef NSOL_PDB_DEF

}  // extern "C"
