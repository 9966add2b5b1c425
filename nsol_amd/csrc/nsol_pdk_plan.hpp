// The planner of the depth-2 / depth-3 kernels of nsol_pdk.hip: which footprints a launch
// may run on, what the cost model thinks of them, which of them a shape's plan lists, and
// what the online tuner does with the times it is given.
//
// Plain C++17: no HIP header, no global, no clock.  Everything is a function of its
// arguments (the knobs as a `const Tuning &`, the shape as a PlanKey, the CU count), so the
// header compiles with the host compiler alone and tests/host/pdk_plan_check.cpp prints the
// lists and replays sample sequences on a CPU.  nsol_pdk.hip keeps the kernels, the
// launchers, the knobs' one instance, the plans' map and the events around a sampled launch.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <tuple>
#include <vector>

#ifndef __HIP__
#define __host__
#define __device__
#endif

namespace nsol {

// Block -> (tile, z-chunk) of the depth-2 / depth-3 kernels of nsol_pdk.hip; one function
// for both kernels, their launchers and the host-side test entry.  blockIdx % 8 names the
// XCD under the round-robin dispatch, and the eight L2s are not coherent with each other.
//   mode 0  plain order: tile = b % tiles, z-chunk = b / tiles.
//   mode 1  XCD x owns a contiguous run of WHOLE tile rows, so the x-tiles of a tile row,
//           which share halo lines, always meet in one L2.  nty = 8 q + r tile rows: the
//           first 8 - r XCDs take q of them, the last r take q + 1.  The volume's last tile
//           row -- the only one that may be clipped by ny -- lies in XCD 7, which is among
//           the larger shares whenever there are any: the volume rows the XCDs cover
//           differ by at most one tile row's valid rows, and no split of whole tile rows
//           has a lighter heaviest XCD.  An XCD walks its tiles x-fastest, then y, then
//           z-chunk; the blocks it has left over return at once.
//   mode 2  the earlier map, for A/B runs: XCD x owns tiles [x slab, (x + 1) slab) with
//           slab = ceil(tiles / 8), whether or not that cuts a tile row in two.
struct PdkBlockMap {
  int mode;
  int ntx, nty;
  int nzc;      // z-chunks
  int q;        // mode 1: tile rows of the smaller share; mode 2: slab (tiles per XCD)
  int big;      // mode 1: first XCD of the larger share (8: none)
};
// want: 0 / 1 / 2 as above; 1 falls back to 0 with fewer than 8 tile rows, 2 with fewer
// than 16 tiles (as the earlier map did)
__host__ __device__ inline PdkBlockMap pdk_block_map(int want, int ntx, int nty, int nzc) {
  PdkBlockMap M{0, ntx, nty, nzc, 0, 8};
  if (want == 1 && nty >= 8) {
    M.mode = 1;
    M.q = nty / 8;
    M.big = 8 - nty % 8;
  } else if (want == 2 && ntx * nty >= 16) {
    M.mode = 2;
    M.q = (ntx * nty + 7) / 8;
  }
  return M;
}
__host__ __device__ inline long long pdk_map_blocks(const PdkBlockMap &M) {
  if (M.mode == 1) return 8LL * (M.q + (M.big < 8 ? 1 : 0)) * M.ntx * M.nzc;
  if (M.mode == 2) return 8LL * M.q * M.nzc;
  return (long long)M.ntx * M.nty * M.nzc;
}
// tile rows [first, first + count) of XCD x under mode 1
__host__ __device__ inline void pdk_map_xcd_rows(const PdkBlockMap &M, int x, int &first,
                                                 int &count) {
  const int over = x > M.big ? x - M.big : 0;
  first = x * M.q + over;
  count = M.q + (x >= M.big ? 1 : 0);
}
// false: block b is surplus
__host__ __device__ inline bool pdk_block_tile(const PdkBlockMap &M, int b, int &tile,
                                               int &zc) {
  const int ntiles = M.ntx * M.nty;
  if (M.mode == 1) {
    int first, count;
    pdk_map_xcd_rows(M, b & 7, first, count);
    const int j = b >> 3;
    const int per = count * M.ntx;
    zc = j / per;
    tile = first * M.ntx + (j - zc * per);
    return zc < M.nzc;
  }
  if (M.mode == 2) {
    const int j = b >> 3;
    tile = (b & 7) * M.q + j % M.q;
    zc = j / M.q;
    return tile < ntiles;
  }
  tile = b % ntiles;
  zc = b / ntiles;
  return true;
}

}  // namespace nsol

namespace nsol_pdk {

using nsol::PdkBlockMap;

struct Tiling {
  int lxb;    // lanes per footprint row
  int rows;   // footprint rows
  int xv;     // valid voxels per tile along x; 0 = one tile spans the row
  int ntx, nty;
  int split;  // 1: whole waves hold the interior lanes of a row, halo lanes at the end
};

struct Tuning {
  int enable = 1;
  int kmax = 3;
  int nw = 0;         // 0 = choose (12 or 8 waves for K = 3; 16 / 12 for K = 2)
  int zchunk = 0;     // 0 = choose
  int ntx = 0;        // 0 = choose
  int xcd_map = 1;    // 0 plain block order, 1 whole tile rows per XCD, 2 tile-count slabs
  int rows = 0;       // 0 = the tiling's own footprint rows; n forces n (a trimmed footprint)
  int verbose = 0;
  int autotune = 1;   // time the best few model candidates once per problem shape
  int tune_min_mvox = 16;   // ... for volumes of at least this many Mi voxels
  int pf2 = -1;       // -1 = where the registers allow; 0 / 1 force
  int split = -1;     // -1 / 1: split lane mapping where it applies; 0: never (experiment)
  int tail2 = 1;        // a run's trailing pair through depth 2 of this kernel once the
                        // shape's depth-3 plan has settled (else k_pd_fused2)
  int min_kvox = 1024;  // smaller volumes (Ki voxels) stay with the one-iteration kernel:
                        // cache resident, they want many short workgroups (crossover
                        // measured between 96^3 and 128^3, tools/crossover_pd.py)
  int shift = -1;       // the shifted form.  -1: long runs of large volumes; 0: never;
                        // 1: wherever it applies
  // Shortest run that takes the shifted block when shift is -1: the block pays for a
  // stand-alone dual and a stand-alone primal pass (28 bytes per voxel each) with 8 bytes
  // per voxel saved per launch.  Measured at 512^3 and 256^3 (DESIGN.md section 5 has the
  // curves): even at 24 iterations, 4 - 5 % ahead at 30.
  int shift_min_iters = 30;
};
// a knob pins the geometry: experiments and tests, no plan and no tuning
inline bool geometry_forced(const Tuning &t) {
  return t.nw > 0 || t.ntx > 0 || t.zchunk > 0 || t.rows > 0;
}
inline int shift_threshold(const Tuning &t) {
  if (t.shift > 0) return 4;            // one launch between the two stand-alone steps
  return t.shift_min_iters > 4 ? t.shift_min_iters : 4;
}

struct Config {
  int nw = 0;
  int pf2 = 0;       // 1 = two prefetch register sets
  int trimmed = 0;   // 1 = fewer footprint rows than fit (a plan lists these by rank only)
  Tiling q{};
  int64_t zchunk = 0;
  double cost = 0.0;      // modelled bytes through L2 -> fabric per launch
};

// A plan belongs to one device (its events live there and boxes differ), one
// element size, one depth and one volume shape.  The kernel variants of a shape
// (TV / Huber, l1 / l2, unit / non-unit spacing) share it on purpose: they differ
// in arithmetic per voxel, not in the footprint geometry the plan chooses.
struct PlanKey {
  int device, esize, k;
  int64_t nz, ny, nx;
  int64_t pitch = 0;     // row pitch of a padded layout (0: contiguous rows)
  int form = 0;          // 1: the shifted form (other tile counts and z-chunks)
  bool operator<(const PlanKey &o) const {
    return std::tie(device, esize, k, nz, ny, nx, pitch, form) <
           std::tie(o.device, o.esize, o.k, o.nz, o.ny, o.nx, o.pitch, o.form);
  }
  int64_t plane() const { return ny * (pitch > 0 ? pitch : nx); }   // plane stride
  int64_t voxels() const { return nz * plane(); }                   // padding included
};
// the volumes the online tuner measures on
inline bool tuned_size(const Tuning &t, int64_t voxels) {
  return t.autotune && voxels >= ((int64_t)t.tune_min_mvox << 20);
}

// Footprint of `nt` lanes cut into ntx columns of tiles.
// xv_fixed > 0: that many valid voxels per tile (the last tile may be shorter)
// instead of nx spread evenly over ntx tiles
// lost: footprint rows that are overlap (2 h; the shifted form: 2 above + 3 below)
// rows > 0: a trimmed footprint of that many rows (at most the nt / lxb that fit); the
// lanes of the rows left out idle (`active` in the kernels)
inline bool make_tiling(const Tuning &t, int64_t nx, int64_t ny, int nt, int vec, int h,
                        int hx, int lxm, int ntx, Tiling *out, int64_t xv_fixed = 0,
                        int lost = -1, int rows = 0) {
  if (lost < 0) lost = 2 * h;
  Tiling q;
  if (ntx == 1) {
    q.xv = 0;
    q.lxb = (int)((nx + vec - 1) / vec);
  } else {
    int64_t xv = xv_fixed > 0 ? xv_fixed : (nx + ntx - 1) / ntx;
    xv = (xv + vec - 1) / vec * vec;
    if (xv * (ntx - 1) >= nx) return false;   // fewer tiles would do
    q.xv = (int)xv;
    q.lxb = (int)(xv / vec) + 2 * (hx / vec);
  }
  if (q.lxb < 1 || q.lxb > lxm) return false;
  q.rows = nt / q.lxb;
  if (rows > q.rows) return false;
  if (rows > 0) q.rows = rows;
  if (q.rows - lost < 1) return false;
  q.ntx = ntx;
  q.nty = (int)((ny + (q.rows - lost) - 1) / (q.rows - lost));
  // interior of a row = whole half-waves: give them to whole half-waves
  q.split = (ntx > 1 && (q.xv / vec) % 32 == 0 && t.split != 0) ? 1 : 0;
  *out = q;
  return true;
}

// The block -> tile map of a launch under the knob pdk_xcd_map (the three modes are
// above); one place, should a form ever have to stay with another mode.
inline PdkBlockMap launch_map(const Tuning &t, const Tiling &q, int64_t nzc) {
  return nsol::pdk_block_map(t.xcd_map, q.ntx, q.nty, (int)nzc);
}

// z-chunk length: trade the 2(K-1) extra planes per chunk against filling the
// last round of workgroups (one workgroup per CU).  Returns the efficiency.
inline double pick_zchunk(int64_t nz, int64_t tiles, int extra, int64_t max_chunk, int cus,
                          int64_t *chunk_out) {
  const double slots = (double)cus;
  double best = -1.0;
  int64_t best_chunk = nz < max_chunk ? nz : max_chunk;
  for (int64_t nzc = 1; nzc <= nz; ++nzc) {
    const int64_t chunk = (nz + nzc - 1) / nzc;
    if (chunk < 8 && nzc > 1) break;
    if (chunk > max_chunk) continue;
    if ((nz + chunk - 1) / chunk != nzc) continue;
    const double blocks = (double)tiles * nzc;
    const double rounds = (double)(int64_t)((blocks + slots - 1) / slots);
    const double fill = blocks / (rounds * slots);
    const double eff = fill * (double)chunk / (double)(chunk + extra);
    if (eff > best) { best = eff; best_chunk = chunk; }
  }
  *chunk_out = best_chunk;
  return best > 0.0 ? best : 1.0;
}

// Bytes one launch pulls through L2 if no overlap is shared between footprints:
// whole 128-byte lines per footprint row (the x halo costs a line on each side,
// which is what makes narrow tiles expensive), six input arrays, plus the five
// output arrays once.  (The shifted form: five input arrays, four output arrays, and
// rows - 5 valid rows that start h = 2 rows inside the footprint.)
inline double model_cost(const Tuning &t, const Tiling &q, int64_t nx, int64_t ny,
                         int64_t nz, int vec, int esize, int h, int hx, double zeff,
                         bool shift = false) {
  double lines = 0.0;
  for (int tx = 0; tx < q.ntx; ++tx) {
    int64_t lo = q.xv ? (int64_t)tx * q.xv - hx : 0;
    int64_t hi = lo + (int64_t)q.lxb * vec;
    if (lo < 0) lo = 0;
    if (hi > nx) hi = nx;
    if (hi <= lo) continue;
    lines += (double)((hi * esize - 1) / 128 - (lo * esize) / 128 + 1);
  }
  // footprint rows inside the volume.  Under the whole-tile-row map eight times the rows of
  // the heaviest XCD stand for the sum, so a tiling whose tile rows deal evenly to the XCDs
  // ranks ahead of one with a nearly empty last tile row.  (Measured at 512^3 the lighter
  // XCDs do not idle -- a launch is as long as one workgroup's march, DESIGN.md section 5 --
  // but the tilings this charge puts first are the ones the tuner then keeps.)
  const int64_t tyv = q.rows - (shift ? 2 * h + 1 : 2 * h);
  auto rows_of = [&](int ty0, int ty1) {
    double r = 0.0;
    for (int ty = ty0; ty < ty1; ++ty) {
      int64_t lo = (int64_t)ty * tyv - h, hi = lo + q.rows;
      if (lo < 0) lo = 0;
      if (hi > ny) hi = ny;
      if (hi > lo) r += (double)(hi - lo);
    }
    return r;
  };
  double rows = rows_of(0, q.nty);
  const PdkBlockMap M = launch_map(t, q, 1);
  if (M.mode == 1) {
    double heavy = 0.0;
    for (int x = 0; x < 8; ++x) {
      int first, count;
      nsol::pdk_map_xcd_rows(M, x, first, count);
      heavy = std::max(heavy, rows_of(first, first + count));
    }
    rows = 8.0 * heavy;
  }
  const double reads = lines * 128.0 * rows * (double)nz * (shift ? 5.0 : 6.0);
  const double writes = (shift ? 4.0 : 5.0) * (double)nx * ny * nz * esize;
  return (reads + writes) / zeff;
}

// candidate configurations for a shape (key.esize, key.k, key.form and the extents; the
// device does not matter), cheapest (by model) first
// the shifted form: footprints of k_pd_shift3 (rows - 5 valid rows, an x halo of >= K
// voxels, one more plane of overlap per z-chunk)
inline std::vector<Config> candidates(const Tuning &t, const PlanKey &key, int cus,
                                      bool twins = false) {
  const int K = key.k;
  const bool SHIFT = key.form != 0;
  const int VW = 16 / key.esize;
  const int H = K - 1;
  const int HX = (((SHIFT ? K : H) + VW - 1) / VW) * VW;
  const int LOST = SHIFT ? 2 * H + 1 : 2 * H;   // rows, and planes per z-chunk
  std::vector<Config> out;
  const int64_t plane_bytes = key.plane() * (int64_t)key.esize;
  // 32-bit buffer offsets: the planes one workgroup touches span < 2^30 bytes
  const int64_t max_planes = ((int64_t)1 << 30) / plane_bytes - 1;
  const int64_t max_chunk = max_planes - 2 * K - 1;
  if (max_chunk < 8) return out;
  // workgroup sizes compiled per depth (16 waves: neither the registers nor the
  // LDS of K = 3 fit)
  for (int nw : {16, 12, 8}) {
    if (nw == 16 && K != 2) continue;
    if (t.nw > 0 && t.nw != nw) continue;
    if (key.nx % VW != 0 && nw != 12) continue;     // see launch_cfg
    if (SHIFT && t.pf2 == 0 && nw == 8) continue;   // 8 waves: the two-set form only
    const int nt = nw * 64;
    const int lxm = nt / (2 * K);
    // tile counts 1..64 with nx spread evenly, plus tiles whose interior is exactly
    // one or two waves wide (256 / 512 B-aligned rows for the split lane mapping)
    // where nx is not a multiple of that
    struct Spec { int ntx; int64_t xv; };
    std::vector<Spec> specs;
    for (int ntx = 1; ntx <= 64; ++ntx) specs.push_back({ntx, 0});
    for (int lanes : {64, 128}) {
      const int64_t xv = (int64_t)lanes * VW;
      const int ntx = (int)((key.nx + xv - 1) / xv);
      // (unless nx spread evenly over as many tiles gives that very width: listed already)
      if (key.nx > xv && key.nx % xv != 0 &&
          (ntx > 64 || ((key.nx + ntx - 1) / ntx + VW - 1) / VW * VW != xv))
        specs.push_back({ntx, xv});
    }
    for (const Spec &sp : specs) {
      const int ntx = sp.ntx;
      if (t.ntx > 0 && ntx != t.ntx) continue;
      Config c;
      c.nw = nw;
      c.pf2 = (nw == 8) ? 1 : 0;
      if (t.pf2 == 0) c.pf2 = 0;
      if (!make_tiling(t, key.nx, key.ny, nt, VW, H, HX, lxm, ntx, &c.q, sp.xv, LOST, t.rows))
        continue;
      // z-chunk and modelled cost of a tiling
      auto price = [&](Config &c) {
        const int64_t tiles = (int64_t)c.q.ntx * c.q.nty;
        double zeff;
        if (t.zchunk > 0) {
          c.zchunk = t.zchunk < max_chunk ? t.zchunk : max_chunk;
          if (c.zchunk > key.nz) c.zchunk = key.nz;
          zeff = (double)c.zchunk / (double)(c.zchunk + LOST);
        } else {
          zeff = pick_zchunk(key.nz, tiles, LOST, max_chunk, cus, &c.zchunk);
        }
        c.cost = model_cost(t, c.q, key.nx, key.ny, key.nz, VW, key.esize, H, HX, zeff, SHIFT);
        // fewer waves hide less latency: mild penalty so that ties go to more waves
        c.cost *= 1.0 + 0.02 * (16 - nw) / 4.0;
      };
      auto push = [&](Config c) {
        if (c.q.split) {
          // rows of whole waves stream ~15 % better (measured); rows of half waves
          // gain less and not always: the plain mapping stays a candidate there
          const bool whole = ((c.q.lxb - 2 * (HX / VW)) % 64) == 0;
          if (!whole) {
            Config d = c;
            d.q.split = 0;
            out.push_back(d);
          }
          c.cost *= whole ? 0.88 : 0.97;
        }
        out.push_back(c);
      };
      price(c);
      push(c);
      // Trimmed twins (the tuner's lists only): the same tiling with fewer footprint rows
      // than fit -- the largest count within 3 rows that makes nty a multiple of 8 (whole
      // tile rows deal evenly to the XCDs), and the largest that wastes fewer rows behind
      // the volume's end than the untrimmed tiling.  A twin stays if the model charges it
      // less than the untrimmed tiling, and gets on a plan's list by the model's rank alone
      // (never by the "few tiles along x" rule): exploration is paid in real launches.
      if (twins && t.rows == 0) {
        auto nty_of = [&](int r) { return (int64_t)((key.ny + (r - LOST) - 1) / (r - LOST)); };
        const int rmax = c.q.rows;
        int twin[2] = {0, 0};
        for (int r = rmax - 1; r >= rmax - 3 && r > LOST && !twin[0]; --r)
          if (nty_of(r) % 8 == 0) twin[0] = r;
        const int64_t waste = (int64_t)c.q.nty * (rmax - LOST) - key.ny;
        for (int r = rmax - 1; r > LOST && !twin[1]; --r)
          if (nty_of(r) * (r - LOST) - key.ny < waste) twin[1] = r;
        if (twin[1] == twin[0]) twin[1] = 0;
        for (int r : twin) {
          Config d = c;
          if (!r || !make_tiling(t, key.nx, key.ny, nt, VW, H, HX, lxm, ntx, &d.q, sp.xv, LOST, r))
            continue;
          d.trimmed = 1;
          price(d);
          if (d.cost < c.cost) push(d);
        }
      }
    }
  }
  std::sort(out.begin(), out.end(),
            [](const Config &a, const Config &b) { return a.cost < b.cost; });
  return out;
}
// ... with the trimmed twins where the tuner will measure: depth 3 of its volumes
inline std::vector<Config> plan_candidates(const Tuning &t, const PlanKey &key, int cus) {
  return candidates(t, key, cus, key.k == 3 && tuned_size(t, key.voxels()));
}

// ---- which candidates a plan lists
enum ListKind {
  kSingle,    // the model's best, settled: small volumes, the tuner off, one candidate
  kSeeded,    // depth 2 behind a settled depth-3 plan: one tiling, settled (seed_index)
  kShort,     // the unshifted depth-3 plan of a shape that has a shifted plan
  kShifted,   // the shifted plan
  kFull       // every other plan the tuner measures
};

// Depth 2 only ever runs the trailing pair of a run: ONE launch per run, far too
// few to explore on.  Where the depth-3 plan of the shape has settled, depth 2
// does not explore either: it takes 12-wave workgroups on whole rows where a row
// fits one (what 81 exploring launches settle on at 512^3 -- 12 : 1 : 256, 1.02 ms
// a pair against 1.19 for k_pd_fused2 and for the depth-3 plan's own tiling,
// tools/_probe/tail2_tuned.py), else the model's best tiling with the depth-3
// plan's workgroup size and tile count along x.  -1: neither is a candidate.
inline int seed_index(const std::vector<Config> &cand, const Config &c3) {
  for (int i = 0; i < (int)cand.size(); ++i)
    if (cand[i].nw == 12 && cand[i].q.ntx == 1) return i;
  for (int i = 0; i < (int)cand.size(); ++i)
    if (cand[i].nw == c3.nw && cand[i].q.ntx == c3.q.ntx) return i;
  return -1;
}

// The kind of list of a new plan.  settled3: what the shape's depth-3 plan has settled on
// (the unshifted plan's pick, else the shifted plan's; null: neither has settled);
// has_shifted: the shape has a shifted depth-3 plan, settled or not.
inline ListKind list_kind(const Tuning &t, const PlanKey &key, const std::vector<Config> &cand,
                          const Config *settled3, bool has_shifted) {
  if (!tuned_size(t, key.voxels())) return kSingle;
  if (key.k == 2 && settled3 && seed_index(cand, *settled3) >= 0) return kSeeded;
  if (cand.size() < 2) return kSingle;
  if (key.k == 3 && !key.form && has_shifted) return kShort;
  return key.form ? kShifted : kFull;
}

// The list of a plan of `kind` from the candidates in the model's order.  One rule: per
// workgroup size the model's best `best`, plus the untrimmed tilings with at most `tiles`
// tiles along x whatever their rank; the first `ztwins` per workgroup size also with a
// shorter z-chunk (more workgroups in flight).  The model ranks; the measurement decides.
//   short    explores on launches that long runs give up for it (plan_donation), and runs
//            only what the shifted block leaves over -- the short runs: no shorter
//            z-chunks (the full list settles on one of these at 512^3 and at 256^3)
//   shifted  explores on the launches of the first long runs of a shape (bench.py's plan
//            pass: 8 runs of 19 launches) -- at 512^3 about 14 candidates, two launches
//            each and four more for every finalist
struct ListRule { int best, tiles, ztwins; };
constexpr int kEveryone = 1 << 30;
constexpr ListRule kListRules[] = {
    /* kSingle  */ {0, 0, 0},     // (one entry, no rule: the model's best ...
    /* kSeeded  */ {0, 0, 0},     //  ... or the seed)
    /* kShort   */ {1, 4, 0},
    /* kShifted */ {3, 4, 2},
    /* kFull    */ {5, 8, kEveryone},
};
inline std::vector<Config> plan_list(const std::vector<Config> &cand, ListKind kind,
                                     int64_t nz, const Config *settled3 = nullptr) {
  if (kind == kSingle) return {cand[0]};
  if (kind == kSeeded) return {cand[seed_index(cand, *settled3)]};
  const ListRule R = kListRules[kind];
  std::vector<Config> out;
  int per_nw[17] = {0};
  for (const Config &c : cand) {
    const int rank = per_nw[c.nw]++;
    if (rank >= R.best && (c.q.ntx > R.tiles || c.trimmed)) continue;
    out.push_back(c);
    const int64_t zc = c.zchunk > 96 ? 64 : 24;
    if (rank < R.ztwins && zc < c.zchunk && zc <= nz) {
      Config d = c;
      d.zchunk = zc;
      out.push_back(d);
    }
  }
  return out;
}

// ---- the online tuner's sampling state, without its events
// A plan holds the model's best few configurations; while a plan is exploring, every REAL
// launch of the run uses the next candidate and is timed (nsol_pdk.hip brackets it with two
// events that are read back later -- no trial launches, no host synchronisation).  After
// `kRounds` samples per candidate and `kFinalRounds` for those within 6 % of the best, the
// finalist with the best score (plan_settle) is kept for the life of the process.
struct Plan {
  std::vector<Config> cand;
  std::vector<std::vector<float>> samples;
  std::vector<float> best_ms;
  std::vector<int> issued, done;
  std::vector<char> dropped;
  int chosen = -1;
};
constexpr int kRounds = 2;
// ... and the finalists -- whoever is within 6 % of the best after those -- are sampled
// up to kFinalRounds times, taking turns: two samples each, minutes apart on a part whose
// clock drifts, settled 511^3 on plans 14 % apart from run to run
constexpr int kFinalRounds = 6;     // (the first sample of a configuration is cold: 5 that count)
constexpr float kFinalBand = 1.06f;

// a plan on `list`; settled: on its first entry, nothing to measure
inline Plan plan_make(std::vector<Config> list, bool settled) {
  Plan P;
  const size_t n = list.size();
  P.cand = std::move(list);
  P.best_ms.assign(n, -1.f);
  P.samples.assign(n, std::vector<float>());
  P.issued.assign(n, 0);
  P.done.assign(n, 0);
  P.dropped.assign(n, 0);
  if (settled) P.chosen = 0;
  return P;
}
// the new plan of `key` on its (non-empty) candidates; settled3, has_shifted: list_kind
inline Plan plan_make(const Tuning &t, const PlanKey &key, const std::vector<Config> &cand,
                      const Config *settled3, bool has_shifted) {
  const ListKind kind = list_kind(t, key, cand, settled3, has_shifted);
  return plan_make(plan_list(cand, kind, key.nz, settled3),
                   kind == kSingle || kind == kSeeded);
}

// samples candidate i is owed (0: dropped)
inline int plan_target(const Plan &P, int i, float best) {
  if (P.dropped[i]) return 0;
  if (P.done[i] >= kRounds && best > 0.f && P.best_ms[i] > kFinalBand * best) return kRounds;
  return kFinalRounds;
}
inline float plan_best(const Plan &P) {
  float best = -1.f;
  for (int i = 0; i < (int)P.cand.size(); ++i)
    if (!P.dropped[i] && P.done[i] >= 1 && (best < 0.f || P.best_ms[i] < best))
      best = P.best_ms[i];
  return best;
}
// samples the plan has yet to issue
inline int plan_owed(const Plan &P) {
  const float best = plan_best(P);
  int want = 0;
  for (int i = 0; i < (int)P.cand.size(); ++i) {
    const int owed = plan_target(P, i, best) - P.issued[i];
    if (owed > 0) want += owed;
  }
  return want;
}

// every owed sample has gone out (or the plan has settled)
inline bool plan_issued(const Plan &P) { return P.chosen >= 0 || plan_owed(P) == 0; }

// a timed launch of candidate i took ms
inline void plan_record(Plan &P, int i, float ms) {
  if (P.best_ms[i] < 0.f || ms < P.best_ms[i]) P.best_ms[i] = ms;
  P.samples[i].push_back(ms);
  P.done[i]++;
}
// ... or its time could not be read: take the sample again
inline void plan_lost(Plan &P, int i) { P.issued[i]--; }

// Once every owed sample is in: score the candidates and keep the best for good.
// true: this call settled the plan.
inline bool plan_settle(Plan &P) {
  if (P.chosen >= 0) return false;
  const int n = (int)P.cand.size();
  // (nobody is dropped on ONE sample: a single slow launch -- the part's clock, another
  // process -- would bar the best tiling for the life of the process; candidates
  // outside the band simply stop at kRounds samples)
  const float best_now = plan_best(P);
  for (int i = 0; i < n; ++i)
    if (P.done[i] < plan_target(P, i, best_now)) return false;
  // the finalists by the SECOND SMALLEST of their warm samples -- the first launch of a
  // configuration is always slow (1.2 - 1.5 ms where the others take 1.13), and what
  // disturbs a launch afterwards only ever slows it down: the median of five let two or
  // three disturbed launches decide (a battery settled on 12 : 3 : 256, 1.20 ms, once in
  // three runs); one lucky launch must not decide either.  Everybody else by the minimum
  // of two.
  auto score = [&](int i) {
    if ((int)P.samples[i].size() < kFinalRounds) return P.best_ms[i] * kFinalBand;
    std::vector<float> v(P.samples[i].begin() + 1, P.samples[i].end());
    std::sort(v.begin(), v.end());
    return v[1];
  };
  int arg = 0;
  for (int i = 0; i < n; ++i)
    if (!P.dropped[i] && (P.dropped[arg] || score(i) < score(arg))) arg = i;
  P.chosen = arg;
  return true;
}

// What the next launch of an exploring plan runs.  timed: it is a sample of that candidate
// (the caller counts it in `issued` once the launch has gone out); `sample` false: the
// launch may not be timed (the first launch of a run reads no dual variable, so it is
// cheaper than all others).
struct PlanNext { int cand; bool timed; };
inline PlanNext plan_next(const Plan &P, bool sample) {
  // the next candidate that still needs a sample, round by round
  const float best_now = plan_best(P);
  for (int r = 1; r <= kFinalRounds && sample; ++r)
    for (int i = 0; i < (int)P.cand.size(); ++i) {
      const int owed = plan_target(P, i, best_now);
      if (P.issued[i] < (r < owed ? r : owed)) return {i, true};
    }
  // every sample is in flight: run the best one known so far meanwhile
  int pick = 0;
  for (int i = 0; i < (int)P.cand.size(); ++i)
    if (!P.dropped[i] && P.best_ms[i] >= 0.f &&
        (P.best_ms[pick] < 0.f || P.best_ms[i] < P.best_ms[pick]))
      pick = i;
  return {pick, false};
}

// Launches a long run gives up for the unshifted depth-3 plan of its shape (they run
// ahead of the block or behind it, three iterations each, bit-identical either way): 0
// until the shifted plan has issued its samples, then exactly the samples the unshifted
// plan is still owed, -1 once there is nothing left to ask for -- the run loop then stops
// asking.  Without them the unshifted form -- the short runs -- would explore on the very
// runs that are too short to gain from the block, or never.
// unshifted: the plan, or where it is not made yet what plan_make would make.
inline int plan_donation(const Plan &shifted, const Plan &unshifted) {
  // (the host runs ahead of the device: a long run has issued every sample of the
  // shifted plan long before the first one is read back -- that is when it hands over)
  if (!plan_issued(shifted)) return 0;
  if (unshifted.chosen >= 0) return -1;
  return plan_owed(unshifted) + 1;   // (+ 1: a run's first launch may read no dual variable: no sample)
}

}  // namespace nsol_pdk
