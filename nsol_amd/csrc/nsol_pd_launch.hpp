// Host-side launch path of the kernels that do ONE Chambolle-Pock iteration in one
// pass: k_pd_fused (nsol_pd.hip), k_pd_fused_iso (nsol_pdi.hip), the member-stacked
// k_pd_sweep (nsol_pds.hip), k_pd_batch (nsol_pdb.hip), k_pd_w (nsol_pdw.hip), k_pd_check (nsol_pdc.hip) and
// k_pd_lin (nsol_pdl.hip).  They share the wave layout of
// nsol_pd_fused_body.hpp -- a wave owns (LX*VEC) x (LY*RY) of an x-y tile and
// marches along z -- so the rounding of the scalars, the grid, the automatic rows
// per lane and the access form are chosen here, once.  A new kernel of the family
// supplies its __global__ function and a launcher struct K with
//
//   template <typename T, int VEC, int LX, bool RAG>
//   static int launch(const PdLaunchArgs<T> &);
//
// which picks the (RY, NDIM) forms the kernel has (pd_auto_rows_per_lane), plans the
// grid (pd_plan_grid) and launches; its entry calls pd_launch<K>(args) after its own
// checks.
#pragma once

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

template <typename T>
struct PdLaunchArgs {
  const T *xbar_in; T *xbar_out; T *x; const T *bt; const T *p_in; T *p_out;
  Geom<T> G;
  PdScalars<T> S;                     // the single-volume kernels' scalars, or
  const PdScalars<T> *row = nullptr;  // the stacked kernel's table row (device)
  int members = 1;                    // volumes stacked along gridDim.y
  PdLaunchTune tune{0, 0, 1, 1};
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

}  // namespace nsol
