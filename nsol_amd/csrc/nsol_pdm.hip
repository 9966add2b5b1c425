// Member-mapped stacked Chambolle-Pock iteration for gfx950 (MI355X): the members of
// a stack (nsol_pdb.hip, nsol_pdw.hip) or of a parameter sweep (nsol_pds.hip) that
// each stop at an iteration of their own (the stopping rule of nsol_pdc.hip) advance
// by one iteration in one launch, and a member that has stopped leaves the grid
// without any array being re-laid.
//
// One kernel family, k_pd_stack / k_pd_stack_iso: the layout is k_pd_w's (nsol_pdw.hip)
// -- the tile bodies pd_fused_tile / pd_fused_iso_tile on the member's own slice with
// the member-local geometry, the scalars from the row PdScalars[iteration][member] of a
// device table, bt and wt at a member stride of 0 or n -- except that the member is not
// the grid row itself but
//
//   m = map[blockIdx.y],
//
// `map` a device array of the strictly increasing indices of the members still
// running, gridDim.y their number.  A member that is not in the map is not touched: x
// is updated in place, so a retired member's result stays where it is.  The table's row
// stride stays the whole group's member count.
//
// WGT: the weighted data term (one more row load per plane, prox_data_w).
// CHK: the four sums of the stopping rule beside the iteration, as k_pd_check forms
// them (chk_add of nsol_pd_common.hpp on the values a lane holds when it stores them),
// PER MEMBER: the workgroup's partial of sum k goes to
//
//   ws[(blockIdx.y * 4 + k) * nparts + blockIdx.x],      nparts = gridDim.x,
//
// and the closing kernel k_pd_stack_final, one workgroup per active member, adds that
// member's partials in a fixed order into rows[m * 4 .. m * 4 + 3] -- rows are indexed
// by MEMBER, not by grid row.  No floating-point atomics: the same input gives the same
// bits on every run.  With CHK off the kernel neither receives nor touches ws, and a
// WGT-off launch with the identity map writes the bits k_pd_batch writes.
#include <stddef.h>

#include <atomic>

#include "nsol_common.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_fused_body.hpp"
#include "nsol_pd_iso_body.hpp"
#include "nsol_pd_launch.hpp"
#include "nsol_pd_sums.hpp"
#include "nsol_pd_weighted.hpp"

using namespace nsol;

namespace {

std::atomic<int> g_stack_launches{0};

// the checking kernel's last argument; nothing at all with CHK off
template <bool CHK>
struct StackWs {
  double *p;
};
template <>
struct StackWs<false> {};

// gridDim.x = active members: grid row r adds its nparts partials of every sum in a
// fixed order into rows[map[r] * 4 + k]
__global__ __launch_bounds__(kBlock) void k_pd_stack_final(
    const double *__restrict__ ws, int nparts, const int *__restrict__ map, int members,
    double *__restrict__ rows) {
  const int64_t r = blockIdx.x;
  const int m = map[r];
  const bool mine = (unsigned)m < (unsigned)members;   // (uniform; see k_pd_stack)
  for (int k = 0; k < kPdSums; ++k) {
    const double t = pd_parts_sum(ws + (r * kPdSums + k) * nparts, nparts);
    if (threadIdx.x == 0 && mine) rows[(int64_t)m * kPdSums + k] = t;
  }
}

// A workgroup without a tile (the XCD map rounds the grid up) leaves zeros with CHK on:
// the closing workgroup adds every partial of its grid row.  So does a workgroup whose
// map entry is no member: the kernels stay inside the arrays whatever the map holds.
template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG, bool WGT, bool CHK>
__global__ __launch_bounds__(kBlock) void k_pd_stack(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ wt, const T *__restrict__ p_in,
    T *__restrict__ p_out, Geom<T> G, const PdScalars<T> *__restrict__ tab,
    const int *__restrict__ map, int members, int64_t bt_stride, int64_t wt_stride,
    int ntx, int nty, int zchunk, int slab, StackWs<CHK> ws) {
  double a[kPdSums] = {0.0, 0.0, 0.0, 0.0};
  int tx, ty, zc;
  // the member of this grid row: uniform per workgroup, read once
  const int64_t m = map[blockIdx.y];
  if (pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc) &&
      (uint64_t)m < (uint64_t)members) {
    const PdScalars<T> S = tab[m];         // the row of this iteration starts at `tab`
    const int64_t xo = m * G.n;
    const int64_t po = m * G.n * NDIM;
    pd_fused_tile<T, VEC, LX, RY, NDIM, RAG, WGT, CHK>(
        xbar_in + xo, xbar_out + xo, x + xo, bt + m * bt_stride, p_in + po, p_out + po,
        G, S, tx, ty, zc, zchunk, WGT ? wt + m * wt_stride : nullptr, a);
  }
  if constexpr (CHK) pd_block_store(a, ws.p, (int)gridDim.x, blockIdx.y);
}

template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG, bool WGT, bool CHK>
__global__ __launch_bounds__(kBlock) void k_pd_stack_iso(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ wt, const T *__restrict__ p_in,
    T *__restrict__ p_out, Geom<T> G, const PdScalars<T> *__restrict__ tab,
    const int *__restrict__ map, int members, int64_t bt_stride, int64_t wt_stride,
    int ntx, int nty, int zchunk, int slab, StackWs<CHK> ws) {
  double a[kPdSums] = {0.0, 0.0, 0.0, 0.0};
  int tx, ty, zc;
  const int64_t m = map[blockIdx.y];
  if (pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc) &&
      (uint64_t)m < (uint64_t)members) {
    const PdScalars<T> S = tab[m];
    const int64_t xo = m * G.n;
    const int64_t po = m * G.n * NDIM;
    pd_fused_iso_tile<T, VEC, LX, RY, NDIM, RAG, WGT, CHK>(
        xbar_in + xo, xbar_out + xo, x + xo, bt + m * bt_stride, p_in + po, p_out + po,
        G, S, tx, ty, zc, zchunk, WGT ? wt + m * wt_stride : nullptr, a);
  }
  if constexpr (CHK) pd_block_store(a, ws.p, (int)gridDim.x, blockIdx.y);
}

// what a launch needs beyond PdLaunchArgs (whose `members` is the ACTIVE count here:
// the tiles the chip has to fill)
template <typename T>
struct StackArgs : PdLaunchArgs<T> {
  const int *map = nullptr;
  int group = 0;              // members of the whole group: the table's row stride
  double *rows = nullptr;     // the board, 4 doubles per member of the group
};

// The launcher struct of nsol_pd_launch.hpp: the active members count as tiles in the
// grid and in the rows per lane.
template <bool ISO, bool WGT, bool CHK>
struct StackLauncher {
  template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
  static int launch_t(const StackArgs<T> &a) {
    const PdGridPlan g = pd_plan_grid<VEC, LX, RY>(a.G, a.members, a.tune);
    if (g.blocks > kPdMaxBlocks) return -2;   // (the caller runs the members one by one)
    StackWs<CHK> ws;
    if constexpr (CHK) {
      // one partial per workgroup, sum and active member
      if (g.blocks > a.chk_ws_doubles / ((int64_t)kPdSums * a.members))
        return NSOL_EINVAL;
      ws.p = a.chk_ws;
    }
    const dim3 grid((unsigned)g.blocks, (unsigned)a.members);
    if constexpr (ISO)
      hipLaunchKernelGGL((k_pd_stack_iso<T, VEC, LX, RY, NDIM, RAG, WGT, CHK>), grid,
                         dim3(kBlock), 0, a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.wt,
                         a.p_in, a.p_out, a.G, a.row, a.map, a.group, a.bt_stride,
                         a.wt_stride, g.ntx, g.nty, g.zchunk, g.slab, ws);
    else
      hipLaunchKernelGGL((k_pd_stack<T, VEC, LX, RY, NDIM, RAG, WGT, CHK>), grid,
                         dim3(kBlock), 0, a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.wt,
                         a.p_in, a.p_out, a.G, a.row, a.map, a.group, a.bt_stride,
                         a.wt_stride, g.ntx, g.nty, g.zchunk, g.slab, ws);
    int rc = launch_status();
    if (rc) return rc;
    g_stack_launches.fetch_add(1, std::memory_order_relaxed);
    if constexpr (CHK) {
      hipLaunchKernelGGL(k_pd_stack_final, dim3((unsigned)a.members), dim3(kBlock), 0,
                         a.st, a.chk_ws, (int)g.blocks, a.map, a.group, a.rows);
      rc = launch_status();
    }
    return rc;
  }

  template <typename T, int VEC, int LX, bool RAG>
  static int launch(const PdLaunchArgs<T> &base) {
    const StackArgs<T> &a = static_cast<const StackArgs<T> &>(base);
    return pd_launch_forms<StackLauncher<ISO, WGT, CHK>, T, VEC, LX, RAG>(
        a, pd_auto_rows_per_lane<VEC, LX>(a.G, a.members));
  }
};

template <bool WGT, bool CHK, typename T>
int stack_launch(const StackArgs<T> &a, bool iso) {
  return iso ? pd_launch<StackLauncher<true, WGT, CHK>>(
                   static_cast<const PdLaunchArgs<T> &>(a))
             : pd_launch<StackLauncher<false, WGT, CHK>>(
                   static_cast<const PdLaunchArgs<T> &>(a));
}

template <typename T>
int stack_iter_impl(const T *xbar_in, T *xbar_out, T *x, const T *bt, int64_t bt_stride,
                    const T *wt, int64_t wt_stride, const T *p_in, T *p_out, int members,
                    const int *map, int active, int ndim, int64_t nz, int64_t ny,
                    int64_t nx, double wx, double wy, double wz, const void *tab,
                    int iteration, int flags, double *ws, int64_t ws_doubles,
                    double *rows, void *stream) {
  if (!pd_stack_takes(members, ndim, nz, ny, nx)) return -2;
  const int64_t n = nz * ny * nx;
  const bool weighted = (flags & NSOL_PD_DATA_WEIGHTED) != 0;
  if (!xbar_in || !xbar_out || !x || !bt || !p_in || !p_out || !tab || iteration < 0 ||
      xbar_in == xbar_out || p_in == p_out || weighted != (wt != nullptr) ||
      !pd_stride_ok(bt_stride, n) || (weighted && !pd_stride_ok(wt_stride, n)) ||
      active < 0 || active > members || (active > 0 && !map) ||
      (rows && (!ws || ws_doubles < (int64_t)kPdSums * active)))
    return NSOL_EINVAL;
  if (active == 0) return 0;
  // (with whole vectors n is a multiple of the vector, so every member's slice of
  // bt and wt starts a whole number of vectors behind its base, as x's does)
  StackArgs<T> a;
  static_cast<PdLaunchArgs<T> &>(a) =
      PdLaunchArgs<T>{xbar_in, xbar_out, x, bt, p_in, p_out,
                      make_geom<T>(ndim, nz, ny, nx, wx, wy, wz)};
  a.row = static_cast<const PdScalars<T> *>(tab) + (int64_t)iteration * members;
  a.members = active;     // (the pd_* knobs do not reach the stack: kPdStackTune)
  a.st = as_stream(stream);
  a.wt = wt;
  a.bt_stride = bt_stride;
  a.wt_stride = weighted ? wt_stride : 0;
  a.chk_ws = ws;
  a.chk_ws_doubles = ws_doubles;
  a.map = map;
  a.group = members;
  a.rows = rows;
  const bool iso = (flags & NSOL_PD_REG_ISOTROPIC) != 0;
  if (rows)
    return weighted ? stack_launch<true, true>(a, iso) : stack_launch<false, true>(a, iso);
  return weighted ? stack_launch<true, false>(a, iso) : stack_launch<false, false>(a, iso);
}

}  // namespace

extern "C" {

int nsol_pd_stack_launches(void) {
  return g_stack_launches.load(std::memory_order_relaxed);
}

int64_t nsol_pd_stack_ws_doubles(int elem_size, int ndim, int64_t nz, int64_t ny,
                                 int64_t nx, int members) {
  if ((elem_size != 4 && elem_size != 8) || !pd_stack_takes(members, ndim, nz, ny, nx))
    return -1;
  const Geom<float> G = make_geom<float>(ndim, nz, ny, nx, 1.0, 1.0, 1.0);
  const int64_t b = elem_size == 4 ? pd_max_blocks<4>(G, kPdStackTune)
                                   : pd_max_blocks<2>(G, kPdStackTune);
  return kPdSums * b * members;
}

#define NSOL_PDM_DEF(T, SUF)                                                           \
  int nsol_pd_stack_iter_##SUF(const T *xi, T *xo, T *x, const T *bt,                  \
                               int64_t bt_stride, const T *wt, int64_t wt_stride,      \
                               const T *pi, T *po, int members, const int *map,        \
                               int active, int ndim, int64_t nz, int64_t ny,           \
                               int64_t nx, double wx, double wy, double wz,            \
                               const void *tab, int iteration, int flags, double *ws,  \
                               int64_t ws_doubles, double *rows, void *s) {            \
    return stack_iter_impl<T>(xi, xo, x, bt, bt_stride, wt, wt_stride, pi, po, members, \
                              map, active, ndim, nz, ny, nx, wx, wy, wz, tab,          \
                              iteration, flags, ws, ws_doubles, rows, s);              \
  }

NSOL_PDM_DEF(float, f32)
NSOL_PDM_DEF(double, f64)
#undef NSOL_PDM_DEF

}  // extern "C"
