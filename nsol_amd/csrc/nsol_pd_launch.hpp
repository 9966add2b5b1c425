// Host-side launch path of the kernels that do ONE Chambolle-Pock iteration in one
// pass: k_pd_fused (nsol_pd.hip), k_pd_fused_iso (nsol_pdi.hip), the member-stacked
// k_pd_sweep (nsol_pds.hip), k_pd_batch (nsol_pdb.hip), k_pd_w (nsol_pdw.hip),
// k_pd_stack (nsol_pdm.hip), k_pd_check (nsol_pdc.hip), k_pd_lin (nsol_pdl.hip) and
// its member-stacked k_pdl_stack (nsol_pdls.hip).
// They share the wave layout of nsol_pd_fused_body.hpp -- a wave owns
// (LX*VEC) x (LY*RY) of an x-y tile and marches along z -- so everything that does
// not depend on the kernel's arguments lives here, once: the rounding of the
// scalars, what geometry a launch takes (pd_stack_takes), the access form
// (pd_launch), the (RY, NDIM) forms (pd_launch_forms), the grid (pd_plan_grid,
// pd_max_blocks), the table PdScalars[iteration][member] of the stacked runs
// (pd_table_fill_upload) and their ping-pong loop (pd_ping_pong).  A new kernel of
// the family supplies its __global__ function and a launcher struct K with
//
//   template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
//   static int launch_t(const PdLaunchArgs<T> &);   // plan the grid, launch
//   template <typename T, int VEC, int LX, bool RAG>
//   static int launch(const PdLaunchArgs<T> &);     // pick the rows per lane
//
// `launch` is the kernel's policy for the rows per lane (pd_auto_rows_per_lane, a
// knob) and a call of pd_launch_forms; the kernel's entry calls pd_launch<K>(args)
// after its own checks.  (FusedKernel and IsoKernel spell their forms out: k_pd_fused
// has four rows per lane as well, and the order in which either unit instantiates its
// forms is the order of the kernels in its code object, which stays as it is.)
#pragma once

#include <math.h>
#include <stddef.h>
#include <string.h>

#include "nsol_pd_common.hpp"

namespace nsol {

// The scalars of one iteration in the kernels' type.  (T)tl and prox_den<T>(tl)
// both round the double tl: a sweep member's table row and a single run's scalars
// must be the same bits.
template <typename T>
PdScalars<T> pd_make_scalars(double sigma, double hden, double tau, double tl,
                             double theta, int flags, bool has_p) {
  PdScalars<T> S;
  S.sigma = (T)sigma; S.hden = huber_den<T>(hden); S.tau = (T)tau; S.tl = (T)tl;
  S.one_plus_tl = prox_den<T>(tl); S.theta = (T)theta;
  S.huber = (flags & NSOL_PD_REG_HUBER) ? 1 : 0;
  S.l1 = (flags & NSOL_PD_DATA_L1) ? 1 : 0;
  S.has_p = has_p ? 1 : 0;
  return S;
}

// The box of the linear kernels (nsol_pdl.hip, nsol_pdls.hip) in the kernels' type,
// rounded towards its inside: a float32 iterate inside [(float)lo, (float)hi] rounded
// to nearest could lie outside the caller's [lo, hi].
template <typename T> inline void box_in(double lo, double hi, T &l, T &h);
template <> inline void box_in<double>(double lo, double hi, double &l, double &h) {
  l = lo; h = hi;
}
template <> inline void box_in<float>(double lo, double hi, float &l, float &h) {
  l = (float)lo; h = (float)hi;
  if (lo == hi) return;
  float li = l, hj = h;
  if ((double)li < lo) li = nextafterf(li, INFINITY);
  if ((double)hj > hi) hj = nextafterf(hj, -INFINITY);
  if (li <= hj) { l = li; h = hj; }
}

// The tune of every kernel the pd_* knobs do not reach (the stacked and the linear
// ones): automatic z chunks and rows per lane, the XCD map and the ragged form on.
constexpr PdLaunchTune kPdStackTune{0, 0, 1, 1};

template <typename T>
struct PdLaunchArgs {
  const T *xbar_in; T *xbar_out; T *x; const T *bt; const T *p_in; T *p_out;
  Geom<T> G;
  PdScalars<T> S;                     // the single-volume kernels' scalars, or
  const PdScalars<T> *row = nullptr;  // the stacked kernel's table row (device)
  int members = 1;                    // volumes stacked along gridDim.y
  PdLaunchTune tune = kPdStackTune;   // the single-volume entries put the knobs here
  hipStream_t st = nullptr;
  const T *wt = nullptr;              // the weighted kernel's per-voxel weights and
  int64_t bt_stride = 0, wt_stride = 0;  // its member strides of bt / wt (0 or G.n)
  double *chk_ws = nullptr;           // the checking kernel's partial sums (one per
  int64_t chk_ws_doubles = 0;         // workgroup and sum) and the board row its
  double *chk_row = nullptr;          // closing workgroup writes (nsol_pdc.hip)
  T lo = T(0), hi = T(0);             // the box of the linear kernels (nsol_pdl.hip)
};

struct PdGridPlan {
  int ntx, nty, zchunk, slab;
  int64_t blocks;   // along gridDim.x; more than kPdMaxBlocks cannot be launched
};
constexpr int64_t kPdMaxBlocks = 0x7fffffff;

// Tiles of TX x TY voxels, z cut into chunks, the y tiles dealt to the 8 XCDs in
// slabs.  `members` multiplies the tiles the chip has to fill, not the blocks.
template <int VEC, int LX, int RY, typename T>
PdGridPlan pd_plan_grid(const Geom<T> &G, int members, const PdLaunchTune &tune) {
  constexpr int LY = kWave / LX;
  constexpr int TY = (kBlock / kWave) * LY * RY;
  constexpr int TX = LX * VEC;
  const int64_t ntx = (G.nx + TX - 1) / TX;
  const int64_t nty = (G.ny + TY - 1) / TY;
  int64_t zchunk = tune.zchunk;
  if (zchunk <= 0) {
    // enough workgroups to fill 256 CUs several times; cache-resident volumes
    // get chunks as short as 2 planes (the extra plane per chunk is an L2 hit
    // there and 8 workgroups would leave the chip idle)
    const int64_t tiles = ntx * nty * members;
    const int64_t want = (4096 + tiles - 1) / tiles;
    zchunk = (G.nz + want - 1) / want;
    if (zchunk < 2) zchunk = 2;
  }
  if (zchunk > G.nz) zchunk = G.nz;
  const int64_t nzc = (G.nz + zchunk - 1) / zchunk;
  int64_t slab = 0;
  int64_t blocks = ntx * nty * nzc;
  if (tune.xcd_map && nty >= 16) {
    slab = (nty + 7) / 8;
    blocks = 8 * slab * ntx * nzc;
  }
  return PdGridPlan{(int)ntx, (int)nty, (int)zchunk, (int)slab, blocks};
}

// two rows per lane unless that leaves fewer than ~2 workgroups per CU
template <int VEC, int LX, typename T>
int pd_auto_rows_per_lane(const Geom<T> &G, int members) {
  constexpr int TY2 = (kBlock / kWave) * (kWave / LX) * 2;
  const int64_t tiles =
      ((G.nx + LX * VEC - 1) / (LX * VEC)) * ((G.ny + TY2 - 1) / TY2) * members;
  return (tiles * ((G.nz + 1) / 2) < 512) ? 1 : 2;
}

// The most workgroups along gridDim.x any access form and rows-per-lane choice of
// pd_launch can ask for on this geometry: with ONE member, as the z chunks only grow
// with the tiles the members add.  VW: elements per 16-byte access.
template <int VW>
int64_t pd_max_blocks(const Geom<float> &G, const PdLaunchTune &tune) {
  int64_t b = 0;
  auto take = [&](const PdGridPlan &g) { if (g.blocks > b) b = g.blocks; };
  take(pd_plan_grid<VW, 64, 1>(G, 1, tune)); take(pd_plan_grid<VW, 64, 2>(G, 1, tune));
  take(pd_plan_grid<VW, 16, 1>(G, 1, tune)); take(pd_plan_grid<VW, 16, 2>(G, 1, tune));
  take(pd_plan_grid<1, 64, 1>(G, 1, tune));  take(pd_plan_grid<1, 64, 2>(G, 1, tune));
  take(pd_plan_grid<1, 16, 1>(G, 1, tune));  take(pd_plan_grid<1, 16, 2>(G, 1, tune));
  return b;
}

// What the kernels take: a geometry of the single-volume kernels, at least one
// member and no more than the grid's y extent, all members together within 2^31
// voxels.  A single volume is members = 1.
inline bool pd_members_ok(int members) { return members >= 1 && members <= 65535; }
inline bool pd_stack_takes(int members, int ndim, int64_t nz, int64_t ny, int64_t nx) {
  if (!pd_members_ok(members)) return false;
  if (!geom_ok(ndim, nz, ny, nx)) return false;
  // (step by step: the product of three extents near 2^31 does not fit an int64)
  const int64_t cap = (int64_t(1) << 31) / members;
  return nx <= cap && ny <= cap / nx && nz <= cap / (nx * ny);
}

// a member stride is 0 (one array for all members) or n (member-major rows)
inline bool pd_stride_ok(int64_t stride, int64_t n) { return stride == 0 || stride == n; }

// The (RY, NDIM) forms every kernel of the family has: one or two rows per lane in
// 2-D and 3-D, one in 1-D.  ry (1 or 2) is the launcher's choice; A is PdLaunchArgs
// or what the launcher derives from it.
template <typename K, typename T, int VEC, int LX, bool RAG, typename A>
int pd_launch_forms(const A &a, int ry) {
  const bool two_rows = ry == 2;
  switch (a.G.ndim) {
    case 1: return K::template launch_t<T, VEC, LX, 1, 1, RAG>(a);
    case 2:
      return two_rows ? K::template launch_t<T, VEC, LX, 2, 2, RAG>(a)
                      : K::template launch_t<T, VEC, LX, 1, 2, RAG>(a);
    default:
      return two_rows ? K::template launch_t<T, VEC, LX, 2, 3, RAG>(a)
                      : K::template launch_t<T, VEC, LX, 1, 3, RAG>(a);
  }
}

// Access form: whole 16-byte vectors when every row and array allows them, else
// element-aligned 16-byte accesses with the row's last vector ragged (knob
// "pd_rag" = 0 restores the 4-byte form, for the tests), else single elements;
// 64 lanes along x when a row fills them, else 16.
template <typename K, typename T>
int pd_launch(const PdLaunchArgs<T> &a) {
  constexpr int VW = 16 / sizeof(T);  // elements per 16-byte access
  const Geom<T> &G = a.G;
  const bool vec_ok = (G.nx % VW == 0) && aligned16(a.xbar_in) && aligned16(a.xbar_out) &&
                      aligned16(a.x) && aligned16(a.bt) && aligned16(a.p_out) &&
                      (!a.p_in || aligned16(a.p_in)) && (!a.wt || aligned16(a.wt)) &&
                      ((G.nz * G.ny * G.nx) % VW == 0);
  const bool rag_ok = a.tune.rag && G.nx >= 2 * VW;
  // rows at a pitch need a vector form (the stacked kernel takes contiguous
  // volumes only: its G.padded is never set)
  if (G.padded && !rag_ok && !vec_ok) return NSOL_EINVAL;
  if (vec_ok) {
    if (G.nx / VW >= kWave) return K::template launch<T, VW, 64, false>(a);
    return K::template launch<T, VW, 16, false>(a);
  }
  if (rag_ok) {
    if ((G.nx + VW - 1) / VW >= kWave) return K::template launch<T, VW, 64, true>(a);
    return K::template launch<T, VW, 16, true>(a);
  }
  if (G.nx >= kWave) return K::template launch<T, 1, 64, false>(a);
  return K::template launch<T, 1, 16, false>(a);
}

// The table of a stacked run, [iteration][member], from the host schedules
// (lmbda[member], sig/tau/theta[member][iteration]): rounded as a single run's
// scalars are, written to the pinned tab_host and uploaded once on the stream.
// members is the caller's to check (pd_stack_takes, pd_members_ok).
template <typename T>
int pd_table_fill_upload(int members, const double *lmbda, const double *sig,
                         const double *tau, const double *theta, int iterations,
                         int p_is_zero, double gamma_huber, int flags, void *tab_host,
                         void *tab, int64_t tab_bytes, hipStream_t st) {
  if (iterations < 0 || !lmbda || !sig || !tau || !theta || !tab_host || !tab ||
      tab_bytes < (int64_t)sizeof(PdScalars<T>) * members * iterations)
    return NSOL_EINVAL;
  const bool huber = (flags & NSOL_PD_REG_HUBER) != 0;
  PdScalars<T> *h = static_cast<PdScalars<T> *>(tab_host);
  for (int n = 0; n < iterations; ++n)
    for (int m = 0; m < members; ++m) {
      const int64_t k = (int64_t)m * iterations + n;
      const double tl = tau[k] * lmbda[m];
      const PdScalars<T> S = pd_make_scalars<T>(
          sig[k], huber ? 1.0 + sig[k] * gamma_huber : 1.0, tau[k], tl, theta[k], flags,
          !(n == 0 && p_is_zero));
      // the table is uploaded as bytes: no stale padding behind the last member
      PdScalars<T> &row = h[(int64_t)n * members + m];
      memset(&row, 0, sizeof(row));
      memcpy(&row, &S, offsetof(PdScalars<T>, has_p) + sizeof(S.has_p));
    }
  if (iterations > 0) {
    hipError_t e = hipMemcpyAsync(tab, tab_host,
                                  sizeof(PdScalars<T>) * (size_t)members * iterations,
                                  hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// The iterations of a run over its ping-pong buffers: iter(n, slot) reads slot and
// writes slot ^ 1; *final_slot is the slot that holds the final state.
template <typename F>
int pd_ping_pong(int iterations, int *final_slot, F iter) {
  int slot = 0;
  for (int n = 0; n < iterations; ++n, slot ^= 1) {
    const int rc = iter(n, slot);
    if (rc) return rc;     // (-2 can only come from the first launch: nothing ran)
  }
  if (final_slot) *final_slot = slot;
  return 0;
}

}  // namespace nsol
