// Member-stacked Chambolle-Pock iteration for gfx950 (MI355X): P independent
// primal-dual runs on ONE observation (a parameter sweep: the members differ in
// lambda = 1/alpha and in their step schedules only) advance by one iteration in
// one launch.
//
// reference: solver_parameter_study.py (_run: one solver per element of
// itertools.product of the parameter lists) driving primal_dual_solver.py:232-261.
//
// The arithmetic is k_pd_fused's (nsol_pd.hip): both kernels run pd_fused_tile of
// nsol_pd_fused_body.hpp, so member m of a stacked run is bit-identical to a
// single run with that member's scalars.  The member index is blockIdx.y; it
// offsets the base pointers (x[m n + i], p[m dim n + c n + i]; bt is shared) and
// selects the row PdScalars[iteration][member] of a device table that
// nsol_pd_sweep_run_* fills once per run.
#include <atomic>

#include "nsol_common.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_fused_body.hpp"
#include "nsol_pd_launch.hpp"

using namespace nsol;

namespace {

std::atomic<int> g_sweep_launches{0};

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_pd_sweep(
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
  pd_fused_tile<T, VEC, LX, RY, NDIM, RAG>(xbar_in + xo, xbar_out + xo, x + xo, bt,
                                           p_in + po, p_out + po, G, S, tx, ty, zc,
                                           zchunk);
}

// The members count as tiles in the launch geometry -- 64 members of a 256 x 256
// image fill the chip where one does not, so the stack takes two rows per lane and
// whole z runs sooner than a single volume would.  Placement never changes a result.
struct SweepKernel {
  template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
  static int launch_t(const PdLaunchArgs<T> &a) {
    const PdGridPlan g = pd_plan_grid<VEC, LX, RY>(a.G, a.members, a.tune);
    if (g.blocks > kPdMaxBlocks) return -2;   // (the caller runs the members one by one)
    hipLaunchKernelGGL((k_pd_sweep<T, VEC, LX, RY, NDIM, RAG>),
                       dim3((unsigned)g.blocks, (unsigned)a.members), dim3(kBlock), 0, a.st,
                       a.xbar_in, a.xbar_out, a.x, a.bt, a.p_in, a.p_out, a.G, a.row,
                       g.ntx, g.nty, g.zchunk, g.slab);
    const int rc = launch_status();
    if (rc == 0) g_sweep_launches.fetch_add(1, std::memory_order_relaxed);
    return rc;
  }

  template <typename T, int VEC, int LX, bool RAG>
  static int launch(const PdLaunchArgs<T> &a) {
    return pd_launch_forms<SweepKernel, T, VEC, LX, RAG>(
        a, pd_auto_rows_per_lane<VEC, LX>(a.G, a.members));
  }
};

template <typename T>
int sweep_iter_impl(const T *xbar_in, T *xbar_out, T *x, const T *bt, const T *p_in,
                    T *p_out, int members, int ndim, int64_t nz, int64_t ny, int64_t nx,
                    double wx, double wy, double wz, const void *tab, int iteration,
                    void *stream) {
  if (!pd_stack_takes(members, ndim, nz, ny, nx)) return -2;
  if (!xbar_in || !xbar_out || !x || !bt || !p_in || !p_out || !tab || iteration < 0 ||
      xbar_in == xbar_out || p_in == p_out)
    return NSOL_EINVAL;
  // (every member's slice starts a whole number of vectors behind the base when
  // the volume is whole vectors)
  PdLaunchArgs<T> a{xbar_in, xbar_out, x, bt, p_in, p_out,
                    make_geom<T>(ndim, nz, ny, nx, wx, wy, wz)};
  a.row = static_cast<const PdScalars<T> *>(tab) + (int64_t)iteration * members;
  a.members = members;    // (the pd_* knobs do not reach the stack: kPdStackTune)
  a.st = as_stream(stream);
  return pd_launch<SweepKernel>(a);
}

template <typename T>
int sweep_run_impl(T *xbar0, T *xbar1, T *x, const T *bt, T *p0, T *p1, int members,
                   int ndim, int64_t nz, int64_t ny, int64_t nx, double wx, double wy,
                   double wz, const double *lmbda, const double *sig, const double *tau,
                   const double *theta, int iterations, int p_is_zero, double gamma_huber,
                   int flags, void *tab_host, void *tab, int64_t tab_bytes,
                   int *final_slot, void *stream) {
  // the stacked kernel shares pd_fused_tile, the component-wise clamp: isotropic
  // sweeps run their members one after the other (nsol_pdi.hip)
  if (flags & (NSOL_PD_REG_ISOTROPIC | NSOL_PD_DATA_WEIGHTED)) return -2;
  if (!pd_stack_takes(members, ndim, nz, ny, nx)) return -2;
  // the table, [iteration][member], rounded as a single run's scalars are
  const int rc = pd_table_fill_upload<T>(members, lmbda, sig, tau, theta, iterations,
                                         p_is_zero, gamma_huber, flags, tab_host, tab,
                                         tab_bytes, as_stream(stream));
  if (rc) return rc;
  T *xb[2] = {xbar0, xbar1};
  T *pp[2] = {p0, p1};
  return pd_ping_pong(iterations, final_slot, [&](int n, int slot) {
    return sweep_iter_impl<T>(xb[slot], xb[slot ^ 1], x, bt, pp[slot], pp[slot ^ 1],
                              members, ndim, nz, ny, nx, wx, wy, wz, tab, n, stream);
  });
}

}  // namespace

extern "C" {

int nsol_pd_sweep_entry_bytes(int elem_size) {
  if (elem_size == 4) return (int)sizeof(PdScalars<float>);
  if (elem_size == 8) return (int)sizeof(PdScalars<double>);
  return NSOL_EINVAL;
}

int nsol_pd_sweep_launches(void) {
  return g_sweep_launches.load(std::memory_order_relaxed);
}

#define NSOL_PDS_DEF(T, SUF)                                                          \
  int nsol_pd_sweep_iter_##SUF(const T *xi, T *xo, T *x, const T *bt, const T *pi,    \
                               T *po, int members, int ndim, int64_t nz, int64_t ny,  \
                               int64_t nx, double wx, double wy, double wz,           \
                               const void *tab, int iteration, void *s) {             \
    return sweep_iter_impl<T>(xi, xo, x, bt, pi, po, members, ndim, nz, ny, nx, wx,   \
                              wy, wz, tab, iteration, s);                             \
  }                                                                                   \
  int nsol_pd_sweep_run_##SUF(T *xb0, T *xb1, T *x, const T *bt, T *p0, T *p1,        \
                              int members, int ndim, int64_t nz, int64_t ny,          \
                              int64_t nx, double wx, double wy, double wz,            \
                              const double *lm, const double *sg, const double *ta,   \
                              const double *th, int iters, int p_is_zero, double gh,  \
                              int flags, void *tab_host, void *tab, int64_t tab_bytes, \
                              int *final_slot, void *s) {                             \
    return sweep_run_impl<T>(xb0, xb1, x, bt, p0, p1, members, ndim, nz, ny, nx, wx,  \
                             wy, wz, lm, sg, ta, th, iters, p_is_zero, gh, flags,     \
                             tab_host, tab, tab_bytes, final_slot, s);                \
  }

NSOL_PDS_DEF(float, f32)
NSOL_PDS_DEF(double, f64)
#undef NSOL_PDS_DEF

}  // extern "C"
