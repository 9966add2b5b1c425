// The planner of the tiled dense correlation (nsol_amd/csrc/nsol_convd_plan.hpp) on the
// CPU: walks a grid of volumes, tap shapes, element sizes and forced tiles and checks every
// answer against the rules restated here.  Prints "ok <plans> <declines> <invalid>" and
// returns 0, or the first violation and 1.  tests/test_conv_dense_tiled_host.py builds it
// plain and with the address / undefined-behaviour sanitizers.
#include <stdint.h>
#include <stdio.h>

#include "../../nsol_amd/csrc/nsol_convd_plan.hpp"

using namespace nsol_convd;

static int fail(const char *what, int64_t nz, int64_t ny, int64_t nx, int kz, int ky, int kx,
                int elem, int fty, int ftx, int fslab) {
  printf("FAIL %s: volume %lld %lld %lld taps %d %d %d elem %d forced %d %d %d\n", what,
         (long long)nz, (long long)ny, (long long)nx, kz, ky, kx, elem, fty, ftx, fslab);
  return 1;
}

// the ring formula, written out again
static int64_t lds_formula(int ty, int tx, int kz, int ky, int kx, int elem) {
  const int64_t fh = ty + ky - 1, fw = tx + kx - 1;
  const int64_t pw = tx + ((kx + 3) / 4) * 4;
  return (int64_t)kz * fh * pw * elem + 8 * (fh + fw);
}

// whether any tile the planner may pick on its own fits the LDS of a CU
static bool some_tile_fits(int64_t ny, int64_t nx, int kz, int ky, int kx, int elem) {
  for (int i = 0; i < kNumTiles; ++i) {
    const Tile t = cut_to_volume(kTiles[i], ny, nx);
    if (lds_formula(t.ty, t.tx, kz, ky, kx, elem) <= 160 * 1024) return true;
  }
  return false;
}

// fewest and most workgroups over the tiles the planner may shrink to
static void block_range(int64_t nz, int64_t ny, int64_t nx, int kz, int ky, int kx, int elem,
                        int64_t *lo, int64_t *hi) {
  *lo = INT64_MAX;
  *hi = 0;
  for (int i = 0; i < kNumTiles; ++i) {
    const Tile t = cut_to_volume(kTiles[i], ny, nx);
    if (lds_formula(t.ty, t.tx, kz, ky, kx, elem) > 160 * 1024) continue;
    const int64_t b = blocks_with(t, nz, ny, nx, kz);
    if (b < *lo) *lo = b;
    if (b > *hi) *hi = b;
  }
}

int main() {
  const int64_t extents[] = {1, 2, 3, 19, 63, 70, 256, 2048, 100000};
  const int taps[] = {1, 2, 3, 5, 13, 17, 129, 131};
  const int forced[][3] = {{0, 0, 0}, {4, 8, 2}, {1, 4, 1}, {3, 12, 5}, {0, 16, 0},
                           {8, 0, 0}, {0, 0, 3}, {4, 6, 2}, {5000, 4, 1}, {64, 4096, 1},
                           {2, 4096, 1}};
  long plans = 0, declines = 0, invalid = 0;
  for (int64_t nz : extents)
    for (int64_t ny : extents)
      for (int64_t nx : extents) {
        if (nz > 256 || (double)nz * ny * nx > 1e11) continue;
        for (int kz : taps)
          for (int ky : taps)
            for (int kx : taps)
              for (int elem = 4; elem <= 8; elem += 4)
                for (const auto &f : forced) {
                  const int fty = f[0], ftx = f[1], fslab = f[2];
                  const Plan p = plan(nz, ny, nx, kz, ky, kx, elem, fty, ftx, fslab);
#define CHECK(c) \
  if (!(c)) return fail(#c, nz, ny, nx, kz, ky, kx, elem, fty, ftx, fslab)
                  const bool any_forced = fty || ftx || fslab;
                  const bool long_axis = kz > 129 || ky > 129 || kx > 129;
                  const bool few = !any_forced && (int64_t)kz * ky * kx < kMinTapsTiled;
                  int64_t lo_blocks, hi_blocks;
                  block_range(nz, ny, nx, kz, ky, kx, elem, &lo_blocks, &hi_blocks);
                  if (p.status == kDecline) {
                    ++declines;
                    // the documented declines, and nothing else
                    CHECK(long_axis || few || (!fty && !ftx &&
                                               !some_tile_fits(ny, nx, kz, ky, kx, elem)) ||
                          (!any_forced && p.ntx > 0) ||   // (a grid over 2^31 workgroups)
                          (!any_forced && lo_blocks < kMinBlocksTiled));
                    continue;
                  }
                  CHECK(!long_axis && !few);
                  if (p.status == kInvalid) {
                    ++invalid;
                    CHECK(any_forced);
                    continue;
                  }
                  CHECK(p.status == kOk);
                  ++plans;
                  // layout
                  CHECK(p.ty >= 1 && p.tx >= kRX && p.tx % kRX == 0 && p.slab >= 1);
                  CHECK(!fty || p.ty == fty);
                  CHECK(!ftx || p.tx == ftx);
                  CHECK(!fslab || p.slab == (fslab < nz ? fslab : nz));
                  CHECK(p.fh == p.ty + ky - 1 && p.fw == p.tx + kx - 1);
                  CHECK(p.pw % kRX == 0 && p.pw >= p.fw);
                  // the furthest element an item's vector reads lies inside the pitch
                  CHECK(p.tx - kRX + ((kx + kRX - 1) / kRX + 1) * kRX <= p.pw);
                  CHECK((int64_t)p.ty * (p.tx / kRX) <= (any_forced ? kMaxItems : 8 * kThreads));
                  // LDS
                  CHECK(p.lds_bytes == lds_formula(p.ty, p.tx, kz, ky, kx, elem));
                  CHECK(p.lds_bytes <= 160 * 1024);
                  CHECK(((int64_t)kz * p.fh * p.pw * elem) % 16 == 0);
                  // the tiles and slabs cover the volume exactly once
                  CHECK(p.ntx * p.tx >= nx && (p.ntx - 1) * p.tx < nx);
                  CHECK(p.nty * p.ty >= ny && (p.nty - 1) * p.ty < ny);
                  CHECK(p.nslab * p.slab >= nz && (p.nslab - 1) * p.slab < nz);
                  CHECK(p.blocks == p.ntx * p.nty * p.nslab && p.blocks >= 1 &&
                        p.blocks <= 0x7fffffff);
                  if (!any_forced) {
                    // at or below 64 KiB whenever a tile that keeps every lane busy fits there
                    bool shared = false;
                    for (int i = 0; i < kNumTiles; ++i) {
                      if (kTiles[i].ty * kTiles[i].tx < kFullTile) break;
                      const Tile t = cut_to_volume(kTiles[i], ny, nx);
                      shared = shared ||
                               lds_formula(t.ty, t.tx, kz, ky, kx, elem) <= 64 * 1024;
                    }
                    CHECK(!shared || p.lds_bytes <= 64 * 1024);
                    CHECK(p.ty <= ny && p.tx < nx + kRX);
                    // small volumes: enough workgroups, or no admissible smaller tile has more
                    CHECK(p.blocks >= kMinBlocksTiled);
                    CHECK(p.blocks == blocks_with(Tile{p.ty, p.tx}, nz, ny, nx, kz));
                    if (p.blocks < kCus)
                      for (int i = 0; i < kNumTiles; ++i) {
                        if (kTiles[i].ty * kTiles[i].tx < kMinShrunkTile) break;
                        const Tile t = cut_to_volume(kTiles[i], ny, nx);
                        if ((int64_t)t.ty * t.tx >= (int64_t)p.ty * p.tx ||
                            lds_formula(t.ty, t.tx, kz, ky, kx, elem) > 160 * 1024)
                          continue;
                        CHECK(blocks_with(t, nz, ny, nx, kz) <= p.blocks);
                      }
                    // slabs: long where that fills the chip, never shorter than the short rule
                    CHECK(p.slab >= (nz < ((kz + 1) / 2 > 2 ? (kz + 1) / 2 : 2)
                                         ? nz : ((kz + 1) / 2 > 2 ? (kz + 1) / 2 : 2)));
                  }
#undef CHECK
                }
      }
  // bad arguments
  if (plan(0, 1, 1, 1, 1, 1, 4).status != kInvalid || plan(1, 1, 1, 0, 1, 1, 4).status != kInvalid ||
      plan(1, 1, 1, 1, 1, 1, 2).status != kInvalid || plan(1, 1, 8, 1, 1, 3, 4, -1, 0, 0).status != kInvalid) {
    printf("FAIL bad arguments\n");
    return 1;
  }
  printf("ok %ld %ld %ld\n", plans, declines, invalid);
  return plans > 1000 && declines > 1000 && invalid > 1000 ? 0 : 1;
}
