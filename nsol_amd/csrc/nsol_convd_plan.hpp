// The planner of the tiled dense-tap correlation k_corr_dense_tile (nsol_convd.hip): which
// output tile a 256-thread workgroup owns, how many output planes it marches over (its
// slab), what that costs in LDS and how many workgroups a launch has -- or that the tiled
// form declines and k_corr_dense answers.
//
// Plain C++17: no HIP header, no global.  Everything is a function of its arguments, so the
// header compiles with the host compiler alone (tests/host/convd_plan_check.cpp).
//
// The kernel's layout, which the plan describes:
//   * a workgroup owns ty x tx outputs of a plane (tx a multiple of kRX) and the output
//     planes [s * slab, (s + 1) * slab) of slab s;
//   * a lane item is kRX consecutive x outputs of one row: ty * tx / kRX items per plane,
//     dealt to the kThreads lanes in turn;
//   * the LDS holds a ring of kz input planes of fh = ty + ky - 1 rows at a pitch of
//     pw = tx + ceil(kx / kRX) * kRX elements (fw = tx + kx - 1 of them filled: an item reads
//     whole kRX-element vectors, the last of which may reach past fw, never past pw), and
//     behind the ring the mapped source indices of the fh rows and the fw columns as int64
//     (the boundary rule is applied once per workgroup, not once per element and plane):
//         lds_bytes = kz * fh * pw * elem + 8 * (fh + fw).
#pragma once

#include <stdint.h>

namespace nsol_convd {

constexpr int kThreads = 256;           // lanes of a workgroup
constexpr int kRX = 4;                  // consecutive x outputs of a lane item
constexpr int kMaxTapsAxis = 129;       // taps along one axis (as the separable passes)
constexpr int64_t kLdsMax = 160 * 1024;     // LDS of a CU (gfx950)
constexpr int64_t kLdsShared = 64 * 1024;   // at or below: two workgroups share a CU
constexpr int kMaxTile = 4096;          // forced ty, tx
constexpr int64_t kMaxItems = 64 * kThreads;   // lane items of a forced tile
constexpr int kCus = 256;               // compute units the slab length is sized for
// Fewest taps (kz * ky * kx) for which the planner picks the tiled form on its own; below,
// it declines and k_corr_dense runs.  Measured on an MI355X (tools/bench_conv_dense.py,
// DESIGN.md section 4n): the numbers are beside the table there.
constexpr int64_t kMinTapsTiled = 27;
// Smallest nominal tile the planner shrinks to for the sake of more workgroups: 16 x 16
// outputs = 64 lane items, one full wave.
constexpr int kMinShrunkTile = 256;
// Fewest workgroups for which the planner picks the tiled form on its own: a launch that
// cannot reach this many even with the smallest tile and the shortest slabs leaves most of
// the chip idle while the plain kernel's grid is one thread per voxel.
// Fewest workgroups a plan was measured with (tools/bench_conv_dense.py on an MI355X,
// DESIGN.md section 4n): 30, a 7^3 and the 7 x 13 x 17 kernel on (20, 24, 40), where the
// tiled form takes 0.075 against 0.129 ms and 0.243 against 0.564 ms in float32, 0.086
// against 0.130 and 0.303 against 0.573 ms in float64; 32 workgroups (32^3) win by 1.6 to
// 2.6, 60 to 64 (3^3 on these volumes, launch-bound at 9 to 12 us) by 1.3 to 1.4.  Nothing
// smaller was measured, so the planner declines below.
constexpr int64_t kMinBlocksTiled = 30;

enum Status { kOk = 0, kInvalid = -1, kDecline = -2 };

struct Plan {
  int status;          // kOk, kDecline (the plain kernel answers), kInvalid (a forced tile
                       // the kernel cannot run, bad extents)
  int ty, tx, slab;
  int fh, fw, pw;      // ring rows, filled columns, pitch
  int64_t lds_bytes;
  int64_t ntx, nty, nslab, blocks;
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int64_t ring_bytes(int ty, int tx, int kz, int ky, int kx, int elem) {
  const int64_t fh = (int64_t)ty + ky - 1, fw = (int64_t)tx + kx - 1;
  const int64_t pw = (int64_t)tx + ceil_div(kx, kRX) * kRX;
  return (int64_t)kz * fh * pw * elem + 8 * (fh + fw);
}

// the nominal tiles, largest first; a tile is cut to the volume before it is weighed
struct Tile { int ty, tx; };
constexpr Tile kTiles[] = {{32, 64}, {32, 32}, {16, 32}, {16, 16}, {8, 16},
                           {8, 8},   {4, 8},   {4, 4},   {2, 4},   {1, 4}};
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);
// nominal outputs of a tile that keeps every lane busy
constexpr int kFullTile = kThreads * kRX;

// A nominal tile on a volume with few rows keeps its area: the rows it cannot have go to x
// (a 1-D signal runs as 1 x 2048).  Never wider than the row, rounded up to kRX.
inline Tile cut_to_volume(Tile t, int64_t ny, int64_t nx) {
  int64_t ty = t.ty, tx = t.tx;
  if (ty > ny) {
    tx = ceil_div(ty * tx, ny);
    ty = ny;
  }
  tx = ceil_div(tx, kRX) * kRX;
  const int64_t row = ceil_div(nx, kRX) * kRX;
  if (tx > row) tx = row;
  if (tx > kMaxTile) tx = kMaxTile;
  return Tile{(int)ty, (int)tx};
}

// Output planes per workgroup.  Every slab fills kz - 1 planes of the ring before its first
// output, so slabs are long where the volume allows: at least max(2 kz, 8) planes, and as
// many slabs as give four workgroups per CU.  Where that leaves fewer workgroups than CUs,
// part of the chip would idle: then slabs may be as short as max(ceil(kz / 2), 2) planes,
// as many as give one workgroup per CU.
inline int64_t slab_with(int64_t nz, int64_t min_slab, int64_t want) {
  const int64_t most = nz / min_slab > 1 ? nz / min_slab : 1;
  if (want > most) want = most;
  return ceil_div(nz, want);
}
inline int64_t slab_for(int64_t nz, int kz, int64_t tiles) {
  const int64_t long_slab = 2 * (int64_t)kz > 8 ? 2 * (int64_t)kz : 8;
  int64_t slab = slab_with(nz, long_slab, ceil_div(4 * (int64_t)kCus, tiles));
  if (tiles * ceil_div(nz, slab) < kCus) {
    const int64_t short_slab = (kz + 1) / 2 > 2 ? (kz + 1) / 2 : 2;
    slab = slab_with(nz, short_slab, ceil_div((int64_t)kCus, tiles));
  }
  return slab;
}
// workgroups of a launch with tile t and the planner's slab
inline int64_t blocks_with(Tile t, int64_t nz, int64_t ny, int64_t nx, int kz) {
  const int64_t tiles = ceil_div(nx, t.tx) * ceil_div(ny, t.ty);
  return tiles * ceil_div(nz, slab_for(nz, kz, tiles));
}

// (fty, ftx, fslab): forced values, 0 = the planner's choice for that one.
inline Plan plan(int64_t nz, int64_t ny, int64_t nx, int kz, int ky, int kx, int elem,
                 int fty = 0, int ftx = 0, int fslab = 0) {
  Plan p{};
  p.status = kInvalid;
  if (nz < 1 || ny < 1 || nx < 1 || kz < 1 || ky < 1 || kx < 1 ||
      (elem != 4 && elem != 8) || fty < 0 || ftx < 0 || fslab < 0)
    return p;
  p.status = kDecline;
  if (kz > kMaxTapsAxis || ky > kMaxTapsAxis || kx > kMaxTapsAxis) return p;
  const bool forced = fty > 0 || ftx > 0 || fslab > 0;
  if (!forced && (int64_t)kz * ky * kx < kMinTapsTiled) return p;
  // first the largest tile at or below kLdsShared that keeps every lane busy, then the
  // largest that fits the CU at all
  Tile best{0, 0};
  for (int pass = 0; pass < 2 && best.tx == 0; ++pass)
    for (int i = 0; i < kNumTiles && best.tx == 0; ++i) {
      if (pass == 0 && kTiles[i].ty * kTiles[i].tx < kFullTile) break;
      const Tile t = cut_to_volume(kTiles[i], ny, nx);
      if (ring_bytes(t.ty, t.tx, kz, ky, kx, elem) <= (pass == 0 ? kLdsShared : kLdsMax))
        best = t;
    }
  // Fewer workgroups than CUs: the LDS per workgroup no longer bounds what a CU runs, so
  // smaller tiles (down to one full wave of lane items) are taken while they give more
  // workgroups.
  if (!forced && best.tx != 0) {
    int64_t blocks = blocks_with(best, nz, ny, nx, kz);
    for (int i = 0; i < kNumTiles && blocks < kCus; ++i) {
      if (kTiles[i].ty * kTiles[i].tx < kMinShrunkTile) break;
      const Tile t = cut_to_volume(kTiles[i], ny, nx);
      if ((int64_t)t.ty * t.tx >= (int64_t)best.ty * best.tx ||
          ring_bytes(t.ty, t.tx, kz, ky, kx, elem) > kLdsMax)
        continue;
      const int64_t b = blocks_with(t, nz, ny, nx, kz);
      if (b > blocks) { best = t; blocks = b; }
    }
    if (blocks < kMinBlocksTiled) return p;
  }
  if (fty > 0) best.ty = fty;
  if (ftx > 0) best.tx = ftx;
  if (best.tx == 0) {
    // no tile of the planner's fits: a forced row count alone cannot help
    if (fty > 0) p.status = kInvalid;
    return p;
  }
  if (best.ty < 1) best.ty = 1;
  if (forced) {
    p.status = kInvalid;
    if (best.ty > kMaxTile || best.tx > kMaxTile || best.tx % kRX != 0 ||
        (int64_t)best.ty * (best.tx / kRX) > kMaxItems ||
        ring_bytes(best.ty, best.tx, kz, ky, kx, elem) > kLdsMax)
      return p;
  }
  p.ty = best.ty;
  p.tx = best.tx;
  p.fh = p.ty + ky - 1;
  p.fw = p.tx + kx - 1;
  p.pw = p.tx + (int)ceil_div(kx, kRX) * kRX;
  p.lds_bytes = ring_bytes(p.ty, p.tx, kz, ky, kx, elem);
  p.ntx = ceil_div(nx, p.tx);
  p.nty = ceil_div(ny, p.ty);
  int64_t slab = fslab > 0 ? fslab : slab_for(nz, kz, p.ntx * p.nty);
  if (slab > nz) slab = nz;
  if (slab > 0x7fffffff) slab = 0x7fffffff;
  p.slab = (int)slab;
  p.nslab = ceil_div(nz, slab);
  // one grid axis: fewer than 2^31 workgroups (the quotient guards the product)
  if (p.ntx > 0x7fffffff || p.nty > 0x7fffffff / p.ntx ||
      p.nslab > 0x7fffffff / (p.ntx * p.nty)) {
    p.status = forced ? kInvalid : kDecline;
    return p;
  }
  p.blocks = p.ntx * p.nty * p.nslab;
  p.status = kOk;
  return p;
}

}  // namespace nsol_convd
