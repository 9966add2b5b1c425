// K Chambolle-Pock iterations in ONE pass over memory (temporal blocking of
// depth K = 2 or 3) on 2-D tiled footprints.
//
// reference: K consecutive trips of the loop body primal_dual_solver.py:242-256.
//
// Per launch the kernel reads xbar, x, bt, p[3] once and writes p[3], x, xbar
// once: 11 words per voxel for K iterations.
//
// Footprints.  The NW*64 lanes of a workgroup form a `rows` x `lxb` grid (lxb lanes
// of VEC voxels per row), so the footprint can be made close to square:
// iteration k needs iteration-(k-1) values one voxel further out, hence a
// footprint loses K-1 voxels on every side and only the interior
// (rows - 2(K-1)) x (lxb*VEC - 2*HX) is stored; the overlap is recomputed, never
// exchanged between workgroups.  k_pd_fused2 uses full rows (512 x 8 at
// nx = 512: 25 % of the lanes recompute overlap already at K = 2); here nx = 512
// is cut into 2 x 256 valid columns: 64 interior + 2 halo lanes per row, 11 rows
// per 12-wave workgroup, the interior lanes of a row in one wave ("split" lane
// mapping) and the halo lanes of all rows together in the last wave.
//
// Pipeline along z (one barrier per plane).  At step s
//   stage 1     runs iteration n+1 on plane s exactly like k_pd_fused (old-data
//               halos from L1/L2), results stay in registers; the loads of plane
//               s+1 are issued right behind it (software prefetch);
//   F_k, k>=2   finishes iteration n+k on plane s-(k-1): z-component of the
//               dual, K^T, prox, over-relaxation (it was waiting for
//               xbar^(k-1) of the plane above);
//   IP_k, k>=2  in-plane part of iteration n+k on plane s-(k-2): every lane
//               publishes xbar^(k-1), p_y^(k-1) and the last p_x^(k-1) of its
//               vector in LDS (double buffered, addressed by logical position),
//               reads the four neighbours' entries and forms p_x^(k), p_y^(k)
//               and the in-plane K^T.
// Waves whose rows lie so far out that nobody uses their stage-k results skip
// that arithmetic.  All global accesses are raw buffer loads / stores with a
// loop-invariant per-lane offset (out of range for lanes outside the volume), so
// the loop body has no exec-mask branches.  The arithmetic per voxel is that of K
// launches of k_pd_fused in the same order, so results are bit-identical.
//
// Host side: a cost model ranks footprint shapes; for large volumes an online tuner
// measures the best few on the run's own launches.  Both are plain C++ in
// nsol_pdk_plan.hpp; the bottom of this file launches, keeps the plans and times samples.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <deque>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <vector>

#include "nsol_common.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pdk_plan.hpp"

using namespace nsol;

// Timing experiments only (wrong results): -DPDK_ABLATE=32 no stage-1 halo loads, =1 no global loads,
// 2 no global stores, 4 no barrier, 8 no arithmetic (memory pattern + LDS exchange
// + barrier only), 16 with 8: no LDS exchange and no barrier either; bits combine
// (DESIGN.md section 5).
// Stage 1's halo (the old xbar of the rows above / below, the old p_y of the row above,
// the x neighbours of a wave's first / last lane) exchanged through the LDS inside the
// 12-wave depth-3 workgroup instead of re-loaded from global memory; only the footprint's
// outermost rows and lanes still load theirs (0: every lane loads its halo, for A/B runs)
#ifndef PDK_LH
#define PDK_LH 1
#endif
#ifndef PDK_ABLATE
#define PDK_ABLATE 0
#endif
// wave priority while a step's loads (bit 0) / stores (bit 1) are issued (experiment)
#ifndef PDK_PRIO
#define PDK_PRIO 0
#endif
// cache policy of the 16-byte plane loads (experiments: 1 = sc0, 2 = nt, 16 = sc1)
#ifndef PDK_LOAD_AUX
#define PDK_LOAD_AUX 0
#endif

// Measurement only (-DNSOL_PDK_FINISH_PROBE, off by default): when does each workgroup of
// the last depth-3 launch start and finish?  Wave 0 of block b writes the 100 MHz wall
// clock into words 2 b (after the block -> tile map) and 2 b + 1 (behind its last plane
// step) of a device table that nsol_pdk_finish_probe() copies out; surplus blocks leave
// zeros.  tools/pdk_finish_probe.py turns the table into finish times per XCD and tile
// row.
#ifdef NSOL_PDK_FINISH_PROBE
constexpr int kProbeBlocks = 8192;
__device__ unsigned long long g_finish_probe[2 * kProbeBlocks];
#define PDK_PROBE_MARK(w)                                                      \
  do {                                                                         \
    if (threadIdx.x == 0 && blockIdx.x < (unsigned)kProbeBlocks)               \
      g_finish_probe[2 * blockIdx.x + (w)] = wall_clock64();                   \
  } while (0)
#else
#define PDK_PROBE_MARK(w) do { } while (0)
#endif

namespace nsol_pdk {

template <typename T, int K>
struct StageScalars {
  T sigma[K], hden[K], tau[K], tl[K], optl[K], theta[K];
  int has_p;
};

// launches of k_pd_fusedk so far, [0]: K = 2, [1]: K = 3 (tests ask which kernel ran)
std::atomic<int> g_launches[2];
// ... and those of them that were launches of the shifted form (k_pd_shift3)
std::atomic<int> g_shift_launches;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

// Raw buffer addressing: a 32-bit byte offset per lane plus a scalar offset,
// and the hardware range check drops accesses whose offset is >= num_records
// (loads return 0).  Lanes outside the volume carry kInvalid as their offset,
// so the loop body needs neither exec-mask branches nor zero-initialised
// destination registers -- which is what lets the prefetch stay in flight.
constexpr uint32_t kInvalid = 0xC0000000u;

__device__ __forceinline__ rsrc_t make_rsrc(const void *p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, bytes, 0x00020000);
}
template <typename T, int V>
__device__ __forceinline__ void bld(rsrc_t r, uint32_t vo, uint32_t so, T (&v)[V]) {
  static_assert(sizeof(T) * V == 16, "one 16-byte vector per lane");
  typedef typename Pack<T, V>::type P;
#if PDK_ABLATE & 1
  for (int k = 0; k < V; ++k) v[k] = T(1e-3) * (T)((vo + so + k) & 255u);
  return;
#endif
  const P t = __builtin_bit_cast(P, __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, PDK_LOAD_AUX));
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = t[k];
}
template <typename T> __device__ __forceinline__ T bld1(rsrc_t r, uint32_t vo, uint32_t so);
template <> __device__ __forceinline__ float bld1<float>(rsrc_t r, uint32_t vo, uint32_t so) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0));
}
template <> __device__ __forceinline__ double bld1<double>(rsrc_t r, uint32_t vo, uint32_t so) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, 0));
}
// The whole offset goes into the VGPR and the scalar offset is the constant 0.
// A 16-byte buffer store reads its data registers over two passes; when the
// scalar offset is a REGISTER the compiler (ROCm 7.2) assumes there is no hazard
// and lets the next VALU instruction overwrite them -- on gfx950 that corrupted
// the stored vector in the lanes of the later passes.  With a constant scalar
// offset its hazard recogniser keeps a wait state between the store and such a
// write (checked in the ISA: at least one instruction separates them); the
// s_nop below is belt and braces only -- the scheduler is free to move it away
// from the store.
// The five output streams are written once and not read again by this launch:
// non-temporal stores (aux bit 1) leave the L2 to the footprints' overlap rows, which
// neighbouring workgroups do re-read (+1.1 % on one box, A/B with tools/_probe/ab_lib.sh).
constexpr int kStoreAux = 2;
template <typename T, int V>
__device__ __forceinline__ void bst(rsrc_t r, uint32_t vo, const T (&v)[V]) {
  typedef typename Pack<T, V>::type P;
  P t;
#pragma unroll
  for (int k = 0; k < V; ++k) t[k] = v[k];
#if PDK_ABLATE & 2
  if (t[0] != T(123.456)) return;
#endif
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, t), r, vo, 0, kStoreAux);
  asm volatile("s_nop 1");
}

// the first n elements only (the last vector of a row that is not a multiple of
// the vector width); same rules for the offsets as bst()
template <typename T, int V>
__device__ __forceinline__ void bst_part(rsrc_t r, uint32_t vo, const T (&v)[V], int n) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (j < n) {
      if constexpr (sizeof(T) == 4)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v[j]), r,
                                              vo + (uint32_t)(j * sizeof(T)), 0, 0);
      else
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v[j]), r,
                                              vo + (uint32_t)(j * sizeof(T)), 0, 0);
    }
  }
  asm volatile("s_nop 1");
}

// Element-wise dual update of a whole vector, out[j] = clamp((p_old[j] + sigma *
// (hi[j] - lo[j]) * w) / hden), with the float arithmetic issued as packed pairs
// (v_pk_add_f32 / v_pk_mul_f32).  There is no packed subtract and the compiler
// turns a + (-b) back into a scalar v_sub, hence the one-line asm with the
// negation in the operand modifiers; all values are exactly those of
// dual_update_u.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
template <bool HUBER, bool UNIT, typename T, int V>
__device__ __forceinline__ void dual_vec(T (&out)[V], const T (&p_old)[V],
                                         const T (&hi)[V], const T (&lo)[V], T w,
                                         T sigma, T hden) {
  if constexpr (sizeof(T) == 4 && V % 2 == 0) {
#pragma unroll
    for (int h = 0; h < V / 2; ++h) {
      const f32x2 a = {hi[2 * h], hi[2 * h + 1]};
      const f32x2 b = {lo[2 * h], lo[2 * h + 1]};
      const f32x2 p = {p_old[2 * h], p_old[2 * h + 1]};
      const f32x2 g = UNIT ? pk_sub(a, b) : a * w + b * (-w);
      f32x2 q = p + sigma * g;
      if constexpr (HUBER) q = q * hden;      // float: hden holds the reciprocal
      out[2 * h] = dual_clamp(q[0]);
      out[2 * h + 1] = dual_clamp(q[1]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      out[j] = dual_update_u<HUBER, UNIT>(p_old[j], hi[j], lo[j], w, sigma, hden);
  }
}

// LDS rows are padded by one (zero) row above and below the footprint
// lane in `mask` ? s : 0, formed where it is used: volatile, so that the compiler neither
// hoists it out of the plane loop nor keeps it in a register across a step (the
// LDS-halo form of the kernel has no register to spare for nine such per-lane constants)
__device__ __forceinline__ float masked_scalar(float s, uint64_t mask) {
  float r;
  // (one scalar operand per VOP3 instruction on gfx9: the value moves first)
  asm volatile("v_mov_b32 %0, %1\n\tv_cndmask_b32_e64 %0, 0, %0, %2"
               : "=&v"(r) : "s"(s), "s"(mask));
  return r;
}
__device__ __forceinline__ double masked_scalar(double s, uint64_t mask) {
  const uint64_t b = __builtin_bit_cast(uint64_t, s);
  uint32_t lo, hi;
  asm volatile("v_mov_b32 %0, %1\n\tv_cndmask_b32_e64 %0, 0, %0, %2"
               : "=&v"(lo) : "s"((uint32_t)b), "s"(mask));
  asm volatile("v_mov_b32 %0, %1\n\tv_cndmask_b32_e64 %0, 0, %0, %2"
               : "=&v"(hi) : "s"((uint32_t)(b >> 32)), "s"(mask));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

template <int NT, int K>
struct LdsShape {
  static constexpr int LXM = NT / (2 * K);          // widest row (lanes)
  static constexpr int N = NT + 2 * LXM;            // vectors per array
};

template <typename T, int V>
struct PlaneLoads {          // registers one prefetched plane lands in
  T xn[V], xv[V], btn[V], pxo[V], pyo[V], pzo[V], xdown[V], xup[V], pyup[V];
  T xright, xleft, pxleft;
};

template <typename T, int VEC, int NW, int K, int WPE, bool HUBER, bool L1, bool PF2,
          bool UNIT, bool RAG>
__global__ __launch_bounds__(NW * 64, WPE) void k_pd_fusedk(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out,
    const T *__restrict__ x_in, T *__restrict__ x_out,
    const T *__restrict__ bt, const T *__restrict__ p_in,
    T *__restrict__ p_out, Geom<T> G, StageScalars<T, K> S, Tiling Q, int zchunk,
    PdkBlockMap M) {
  constexpr int NT = NW * 64;
  constexpr int H = K - 1;
  constexpr int HX = ((H + VEC - 1) / VEC) * VEC;
  constexpr int LN = LdsShape<NT, K>::N;
  // LH (see PDK_LH): a second barrier per step separates the exchange of stage 1's inputs
  // from that of the later stages' -- the arrays then need no second copy by step parity,
  // which is what makes room for the stage-0 arrays (108 KB instead of 144)
  // (float, whole-vector rows: the double and the ragged-row instantiations would spill)
  constexpr bool LH = PDK_LH && K == 3 && NW == 12 && !PF2 && sizeof(T) == 4 && !RAG;
  constexpr int NB = LH ? 1 : 2;
  __shared__ __attribute__((aligned(16))) T s_xb[NB][K - 1][LN * VEC];
  __shared__ __attribute__((aligned(16))) T s_py[NB][K - 1][LN * VEC];
  __shared__ T s_px[NB][K - 1][LN];   // last p_x^(k-1) of every lane's vector
  __shared__ __attribute__((aligned(16))) T s_xb0[LH ? LN * VEC : VEC];   // old xbar[s]
  __shared__ __attribute__((aligned(16))) T s_py0[LH ? LN * VEC : VEC];   // old p_y[s]
  __shared__ T s_px0[LH ? LN : 1];                                        // old p_x[s], last

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // Block -> (tile, z-chunk): pdk_block_tile (nsol_pdk_plan.hpp).  A whole workgroup
  // leaves together.
  int tile, zc;
  if (!pdk_block_tile(M, (int)blockIdx.x, tile, zc)) return;
  PDK_PROBE_MARK(0);
  const int tx = tile % Q.ntx;
  const int ty = tile / Q.ntx;

  // ---- geometry of this lane
  // lane -> (row, lx) of the footprint.  Plain: row-major.  Split (the interior of
  // a row is a multiple of 32 lanes): whole (half) waves hold the interior lanes of
  // one row -- aligned, contiguous 512 B / 1 KiB per array -- and the halo lanes of
  // all rows sit together behind them; rows that straddle waves cost ~15 % of the
  // achievable bandwidth (tools/micro/copy_pattern.hip).
  const int lxb = Q.lxb;
  constexpr int HL = HX / VEC;                 // halo lanes on each side of a row
  int row, lx;
  bool lone = false;                           // neighbours along x are not adjacent lanes
  if (Q.split) {
    const int inner = lxb - 2 * HL;
    const int main = Q.rows * inner;
    if (tid < main) {
      row = tid / inner;
      lx = HL + (tid - row * inner);
      // the interior's first / last lane: the neighbour is a halo lane elsewhere
      lone = (lx == HL) || (lx == HL + inner - 1);
    } else {
      const int h = tid - main;
      row = h / (2 * HL);
      const int side = h - row * (2 * HL);
      lx = side < HL ? side : inner + side;
      lone = true;
    }
  } else {
    row = tid / lxb;
    lx = tid - row * lxb;
  }
  const bool active = row < Q.rows;
  const bool single_x = (Q.xv == 0);
  const int64_t xv_lo = single_x ? 0 : (int64_t)tx * Q.xv;
  const int64_t xv_hi = single_x ? G.nx : xv_lo + Q.xv;
  const int64_t x0 = (single_x ? 0 : xv_lo - HX) + (int64_t)lx * VEC;
  const int64_t tyv = Q.rows - 2 * H;
  const int64_t yv_lo = (int64_t)ty * tyv;
  const int64_t yv_hi = yv_lo + tyv;
  const int64_t y = yv_lo - H + row;
  const bool rin = active && x0 >= 0 && x0 < G.nx && y >= 0 && y < G.ny;
  const bool rvalid = rin && x0 >= xv_lo && x0 < xv_hi && y >= yv_lo && y < yv_hi;

  // Step sizes masked to zero outside the volume: a voxel there gets p = 0 and
  // x = xbar = 0 in every stage (K and K^T pad with zeros) without selects.
  T sig_m[K], tau_m[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    sig_m[k] = rin ? S.sigma[k] : T(0);
    tau_m[k] = rin ? S.tau[k] : T(0);
  }
  // (LH: the same values from lane masks in scalar registers at every use, see
  // masked_scalar)
  const uint64_t m_rin = __builtin_amdgcn_ballot_w64(rin);
  auto sigm = [&](int k) -> T {
    if constexpr (LH) return masked_scalar(S.sigma[k], m_rin); else return sig_m[k];
  };
  auto taum = [&](int k) -> T {
    if constexpr (LH) return masked_scalar(S.tau[k], m_rin); else return tau_m[k];
  };

  // plane indices fit in 32 bits (the host checks nz < 2^30): scalar registers
  // are the scarce resource here (11 buffer descriptors)
  const int nzi = (int)G.nz;
  const int zbeg = zc * zchunk;
  int zend = zbeg + zchunk;
  if (zend > nzi) zend = nzi;
  const int s_first = zbeg > H ? zbeg - H : 0;
  const int s_last = zend + K - 2;
  const int s_hi = s_last < nzi - 1 ? s_last : nzi - 1;   // last step with a stage 1

  // ---- buffer resources over the planes [pz0, pe) this workgroup touches
  const int pz0 = s_first > 0 ? s_first - 1 : 0;
  int pe = s_last + 2;
  if (pe > nzi) pe = nzi;
  const uint32_t szb = (uint32_t)(G.sz * (int64_t)sizeof(T));
  const uint32_t syb = (uint32_t)(G.sy * (int64_t)sizeof(T));
  const uint32_t span = (uint32_t)(pe - pz0) * szb;       // < 2^30 (host-checked)
  const int64_t boff = (int64_t)pz0 * G.sz;
  const uint32_t pspan = S.has_p ? span : 0u;             // p = 0: every load returns 0
  const rsrc_t r_xb = make_rsrc(xbar_in + boff, span);
  const rsrc_t r_x = make_rsrc(x_in + boff, span);
  const rsrc_t r_bt = make_rsrc(bt + boff, span);
  const rsrc_t r_px = make_rsrc(p_in + boff, pspan);
  const rsrc_t r_py = make_rsrc(p_in + G.n + boff, pspan);
  const rsrc_t r_pz = make_rsrc(p_in + 2 * G.n + boff, pspan);
  const rsrc_t w_xb = make_rsrc(xbar_out + boff, span);
  const rsrc_t w_x = make_rsrc(x_out + boff, span);
  const rsrc_t w_px = make_rsrc(p_out + boff, span);
  const rsrc_t w_py = make_rsrc(p_out + G.n + boff, span);
  const rsrc_t w_pz = make_rsrc(p_out + 2 * G.n + boff, span);

  // per-lane byte offsets inside a plane (loop invariant); the plane is selected
  // by the scalar offset.  Stage-1 halos: old data from global memory (L1/L2).
  const bool row_end = (lx == lxb - 1) || lane == 63 || lone;
  const bool row_beg = (lx == 0) || lane == 0 || lone;
  const uint32_t o0 = (uint32_t)((y * G.sy + x0) * (int64_t)sizeof(T));
  const uint32_t v_own = rin ? o0 : kInvalid;
  // (LH: only the footprint's first / last row and first / last lane load their halo;
  // everybody else's comes out of the LDS)
  const bool e_up = !LH || row == 0, e_down = !LH || row == Q.rows - 1;
  const bool e_right = LH ? lx == lxb - 1 : row_end, e_left = LH ? lx == 0 : row_beg;
  uint32_t v_up = (rin && y > 0 && e_up) ? o0 - syb : kInvalid;
  const uint32_t v_down = (rin && y + 1 < G.ny && e_down) ? o0 + syb : kInvalid;
  uint32_t v_right = (rin && e_right && x0 + VEC < G.nx) ? o0 + 16u : kInvalid;
  const uint32_t v_left = (rin && e_left && x0 > 0) ? o0 - (uint32_t)sizeof(T) : kInvalid;
  // (LH: a lane sits in at most one outermost row and is at most one outermost lane, so
  // the row beyond the footprint -- above OR below -- lands in one register vector and
  // the x neighbour beyond it -- right OR left -- in one register: four vector registers
  // and a load less per lane and step)
  const bool last_row = row == Q.rows - 1;
  if (LH && last_row && row != 0) v_up = v_down;
  if (LH && lx == 0 && lxb > 1) v_right = v_left;
  const uint32_t v_pyup = (LH && row != 0) ? kInvalid : v_up;
  const uint32_t v_st = rvalid ? o0 : kInvalid;
  // RAG: rows are not a multiple of the vector width, so the row's last vector
  // sticks out by VEC - nval elements (they belong to the next row).  Their xbar
  // must read as zero -- the zero padding of K -- wherever a valid neighbour looks
  // at it, and they are left out of the stores; whatever else is computed for
  // them is read by nobody.  (Accesses are 4-byte aligned then: legal, 90 % of the
  // aligned rate, tools/micro/unaligned_b128.hip.)
  int nval = VEC;
  if constexpr (RAG) {
    const int64_t left = G.nx - x0;
    nval = left >= VEC ? VEC : (left > 0 ? (int)left : 0);
  }
  auto cut_tail = [&](T (&v)[VEC]) {
    if constexpr (RAG) {
#pragma unroll
      for (int j = 1; j < VEC; ++j) v[j] = j < nval ? v[j] : T(0);
    }
  };
  auto store_vec = [&](rsrc_t r, uint32_t vo, const T (&v)[VEC]) {
    if constexpr (RAG) {
      // (rows held at a pitch: what sticks out of the row is padding -- whole store)
      if (nval < VEC && !G.padded) {
        bst_part<T, VEC>(r, vo, v, nval);
        return;
      }
    }
    bst<T, VEC>(r, vo, v);
  };
  // stages >= 2: neighbours inside the footprint come from LDS; beyond it the
  // value is zero (the zero padding of K / K^T at the volume edge) or belongs
  // to a voxel whose result is recomputed by the next footprint and not stored
  const bool n_r = active && lx < lxb - 1;
  const bool v_l = rin && lx > 0 && x0 > 0;      // the left / upper voxel is in the volume
  const bool v_u = rin && row > 0 && y > 0;
  const bool g_l = rin && row_beg && x0 > 0;
  const bool g_u = rin && y > 0;
  // LDS slot of this lane: logical position, one padding row above.  Idle lanes
  // (row >= rows) keep the plain mapping: their zeros land in the bottom padding.
  const int slot = active ? (row + 1) * lxb + lx : tid + lxb;
  const int li = slot * VEC;
  // step size of the recomputed dual of the voxel above: zero where there is none
  // (its inputs are zero there -- out-of-range load, zero LDS row, or a lane outside
  // the volume -- so the result is exactly zero without a select per value)
  T sig_u[K];
  sig_u[0] = g_u ? S.sigma[0] : T(0);
#pragma unroll
  for (int k = 1; k < K; ++k) sig_u[k] = v_u ? S.sigma[k] : T(0);
  const uint64_t m_gu = __builtin_amdgcn_ballot_w64(g_u), m_vu = __builtin_amdgcn_ballot_w64(v_u);
  auto sigu = [&](int k) -> T {
    if constexpr (LH) return masked_scalar(S.sigma[k], k == 0 ? m_gu : m_vu);
    else return sig_u[k];
  };
  // Stage k is exact -- and its result used -- only k-1 rows inside the footprint
  // (and, for the last stage, off the x halo lanes): the outer rows run stage 1
  // only, the next ones stages 1-2, ...  A wave none of whose lanes needs a stage
  // skips its arithmetic (it still publishes its previous stage and joins the
  // barrier); with the split lane mapping a wave is one row, so 6 of 33
  // row-stages disappear at 11 rows.
  bool wneed[K];
  wneed[0] = true;
#pragma unroll
  for (int k = 2; k <= K; ++k) {
    const bool in_x = single_x || k < K || (lx >= HL && lx < lxb - HL);
    const bool mine = active && row >= k - 1 && row <= Q.rows - k && in_x;
    wneed[k - 1] = __ballot(mine) != 0ull;
  }

  // zero rows above and below the footprint, once
  for (int i = tid; i < NB * (K - 1) * 2 * lxb * VEC; i += NT) {
    const int e = i % (lxb * VEC);
    int r = i / (lxb * VEC);
    const int side = r & 1; r >>= 1;
    const int kk = r % (K - 1);
    const int b = r / (K - 1);
    const int at = side ? (Q.rows + 1) * lxb * VEC + e : e;
    s_xb[b][kk][at] = T(0);
    s_py[b][kk][at] = T(0);
    if (LH && b == 0 && kk == 0) { s_xb0[at] = T(0); s_py0[at] = T(0); }
  }

  // State carried from one plane step to the next.  The 8-wave variants keep two
  // copies: a step reads one and writes the other (main loop unrolled by two), so
  // "carrying" is a renaming of registers instead of ~40 v_mov per step; with 12
  // or 16 waves that spills, and one copy is updated in place.
  struct Carry {
    T xc[VEC];              // xbar[s]
    T pz[K][VEC];           // pz[k-1]: p^(k)_z on the plane stage k finished last
    T c_xb[K][VEC];         // [k-1], k>=2: xbar^(k-1) on plane s-(k-1)
    T c_x[K][VEC];          //               x^(k-1) there
    T c_bt[K][VEC];         //               bt there
    T c_kt[K][VEC];         //               in-plane part of K^T p^(k) there
    T c_px[K][VEC];         // [k-1], k>=3: p_x^(k-1) on plane s-(k-1)+1 (from IP_{k-1})
    T c_py[K][VEC];
  };
  Carry CA, CB;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    zero(CA.pz[k]); zero(CA.c_xb[k]); zero(CA.c_x[k]); zero(CA.c_bt[k]);
    zero(CA.c_kt[k]); zero(CA.c_px[k]); zero(CA.c_py[k]);
  }
  uint32_t adv = (uint32_t)(s_first - pz0) * szb;   // scalar offset of plane s
  bld<T, VEC>(r_xb, v_own, adv, CA.xc);
  cut_tail(CA.xc);
  {
    // p'_z of the plane below the first one (zero at the bottom of the volume)
    T xm[VEC], pm[VEC];
    const uint32_t vb = s_first > 0 ? v_own : kInvalid;
    const uint32_t ab = s_first > 0 ? adv - szb : 0u;
    bld<T, VEC>(r_xb, vb, ab, xm);
    bld<T, VEC>(r_pz, vb, ab, pm);
    const T sg = s_first > 0 ? S.sigma[0] : T(0);
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      CA.pz[0][j] = dual_update_u<HUBER, UNIT>(pm[j], CA.xc[j], xm[j], G.wz, sg, S.hden[0]);
  }

  // Software pipeline: the loads of plane s+1 are issued right after the stage-1
  // arithmetic of plane s and stay in flight while the later stages (and the
  // barrier) run -- the waves of a workgroup move in lockstep, so nothing else
  // would hide the latency.
  // PF2: two register sets, so the loads of plane s+1 are issued BEFORE the
  // stage-1 arithmetic of plane s (a full step of latency hiding; +36 VGPRs).
  typedef PlaneLoads<T, VEC> Loads;
  Loads LA, LB;
  // stage 1's halo of plane `a`
  auto issue_halo = [&](Loads &L, uint32_t a) {
#if PDK_ABLATE & 32
    // (timing experiment, wrong results: stage 1 without its halo loads -- what an
    // exchange of the old xbar / p_y rows inside the workgroup could save at most)
    L.xright = L.xleft = L.pxleft = T(0);
    zero(L.xdown); zero(L.xup); zero(L.pyup);
#else
    if constexpr (LH) {
      // The rows beyond the footprint (every wave issues the two loads, nine of the
      // twelve with every lane out of range: a wave-uniform branch around them cost more
      // than it saved -- 1.250 against 1.168 ms per launch, without the exchange 1.193).
      // The VOXELS beyond the footprint's first / last lane are not loaded at all: they
      // only reach stage 1 of the footprint's outermost voxel, and with HX >= K what a
      // stored value depends on ends one voxel short of it (static_assert below).
      static_assert(!LH || HX >= K, "LH: the x halo must be wider than the dependency cone");
      L.xright = L.pxleft = T(0);
      bld<T, VEC>(r_xb, v_up, a, L.xup);
      bld<T, VEC>(r_py, v_pyup, a, L.pyup);
    } else {
      L.xright = bld1<T>(r_xb, v_right, a);
      L.xleft = bld1<T>(r_xb, v_left, a);
      L.pxleft = bld1<T>(r_px, v_left, a);
      bld<T, VEC>(r_xb, v_down, a, L.xdown);
      bld<T, VEC>(r_xb, v_up, a, L.xup);
      bld<T, VEC>(r_py, v_up, a, L.pyup);
    }
#endif
  };
  auto issue_loads = [&](Loads &L, int sp, uint32_t a) {
    // sp: plane; a: its scalar offset.  The plane above the volume is zero.
#if PDK_PRIO & 1
    __builtin_amdgcn_s_setprio(3);
#endif
    // (LH: the halo loads first.  They are what the next step publishes first, under
    // lane masks, and the compiler waits for the LAST load of a step with vmcnt(0) --
    // the stores issued behind it drained at the top of every step; the own planes'
    // loads it counts)
    if constexpr (LH) issue_halo(L, a);
    bld<T, VEC>(r_xb, (sp + 1 < nzi) ? v_own : kInvalid, a + szb, L.xn);
    bld<T, VEC>(r_x, v_own, a, L.xv);
    bld<T, VEC>(r_bt, v_own, a, L.btn);
    bld<T, VEC>(r_px, v_own, a, L.pxo);
    bld<T, VEC>(r_py, v_own, a, L.pyo);
    bld<T, VEC>(r_pz, v_own, a, L.pzo);
    if constexpr (!LH) issue_halo(L, a);
#if PDK_PRIO & 1
    __builtin_amdgcn_s_setprio(0);
#endif
  };
  issue_loads(LA, s_first, adv);

  // one plane step; HAVE1 = false in the drain steps above the volume's last plane
  auto step = [&](auto have1_tag, int s, Loads &L, Loads &LN, const Carry &P,
                  Carry &N) {
    constexpr bool HAVE1 = decltype(have1_tag)::value;
#if PDK_ABLATE & 8
    {
      // Timing experiment (wrong results): the step's memory traffic without its
      // arithmetic -- the prefetched plane is summed up (every load stays alive),
      // the sum goes through the LDS exchange and the barrier of a step (bit 16:
      // neither) and out through the five stores.
      const bool more = s + 1 <= s_hi;
      T acc[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        acc[j] = L.xn[j] + L.xv[j] + L.btn[j] + L.pxo[j] + L.pyo[j] + L.pzo[j] + L.xdown[j] +
                 L.xup[j] + L.pyup[j] + L.xright + L.xleft + L.pxleft + P.xc[j];
      if constexpr (HAVE1) issue_loads(L, more ? s + 1 : s, more ? adv + szb : adv);
      const int buf = LH ? 0 : (int)(s & 1);
#if !(PDK_ABLATE & 16)
#pragma unroll
      for (int k = 2; k <= K; ++k) {
        stv<T, VEC>(&s_xb[buf][k - 2][li], acc);
        stv<T, VEC>(&s_py[buf][k - 2][li], acc);
        s_px[buf][k - 2][slot] = acc[0];
      }
      __syncthreads();
#pragma unroll
      for (int k = 2; k <= K; ++k) {
        T below[VEC], above[VEC], above_py[VEC];
        ldv<T, VEC>(&s_xb[buf][k - 2][li + lxb * VEC], below);
        ldv<T, VEC>(&s_xb[buf][k - 2][li - lxb * VEC], above);
        ldv<T, VEC>(&s_py[buf][k - 2][li - lxb * VEC], above_py);
        const T e = s_xb[buf][k - 2][li + VEC] + s_xb[buf][k - 2][li - 1] +
                    s_px[buf][k - 2][slot - 1];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] += below[j] + above[j] + above_py[j] + e;
      }
#endif
      const int f = s - (K - 1);
      if (f >= zbeg && f < zend) {
        const uint32_t vo = v_st + (adv - (uint32_t)(K - 1) * szb);
        store_vec(w_pz, vo, acc);
        store_vec(w_x, vo, acc);
        store_vec(w_xb, vo, acc);
      }
      const int a = s - (K - 2);
      if (a >= zbeg && a < zend) {
        const uint32_t vo = v_st + (adv - (uint32_t)(K - 2) * szb);
        store_vec(w_px, vo, acc);
        store_vec(w_py, vo, acc);
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) N.xc[j] = acc[j];
      adv += szb;
      return;
    }
#endif
    // fr_*[k-1]: results of stage k produced in this step
    T fr_xb[K][VEC], fr_x[K][VEC], fr_bt[K][VEC], pzn[K][VEC];
    T f_px[VEC], f_py[VEC];
    if constexpr (HAVE1) {
      // prefetch plane s+1 (after the last plane: re-reads it, unused)
      const bool more = s + 1 <= s_hi;
      if constexpr (PF2) issue_loads(LN, more ? s + 1 : s, more ? adv + szb : adv);
#if PDK_ABLATE & 64
      {
        // (timing experiment, with bit 32: what an exchange of stage 1's halo through
        // the LDS would cost -- two vectors and a scalar published, a SECOND barrier in
        // the step, three vectors and three scalars read back)
        const int b0 = LH ? 0 : (int)(s & 1);
        stv<T, VEC>(&s_xb[b0][0][li], P.xc);
        stv<T, VEC>(&s_py[b0][0][li], L.pyo);
        s_px[b0][0][slot] = L.pxo[VEC - 1];
        __syncthreads();
        ldv<T, VEC>(&s_xb[b0][0][li + lxb * VEC], L.xdown);
        ldv<T, VEC>(&s_xb[b0][0][li - lxb * VEC], L.xup);
        ldv<T, VEC>(&s_py[b0][0][li - lxb * VEC], L.pyup);
        L.xright = s_xb[b0][0][li + VEC];
        L.xleft = s_xb[b0][0][li - 1];
        L.pxleft = s_px[b0][0][slot - 1];
      }
#endif
      // ================= stage 1: iteration n+1 on plane s ===================
      // its halo: loaded (every lane its own), or -- LH -- the old values every lane
      // holds anyway exchanged through the LDS: own xbar[s], p_y[s] and the last p_x[s]
      // published, the footprint's outermost rows also put the row they loaded from
      // beyond it into the padding row, a barrier, the neighbours read
      T h_down[VEC], h_up[VEC], h_pyup[VEC];
      T h_right = L.xright, h_left = LH ? L.xright : L.xleft, h_pxleft = L.pxleft;
      if constexpr (LH) {
        __builtin_amdgcn_sched_barrier(0);
        if (active) {
          stv<T, VEC>(&s_xb0[li], P.xc);
          stv<T, VEC>(&s_py0[li], L.pyo);
          s_px0[slot] = L.pxo[VEC - 1];
          if (row == 0) {
            stv<T, VEC>(&s_xb0[li - lxb * VEC], L.xup);
            stv<T, VEC>(&s_py0[li - lxb * VEC], L.pyup);
          }
          // (the last row's L.xup holds the row BELOW the footprint; a one-row footprint
          // would need both and does not exist: rows >= 2 K - 1)
          if (last_row && row != 0) stv<T, VEC>(&s_xb0[li + lxb * VEC], L.xup);
        }
        __syncthreads();
        ldv<T, VEC>(&s_xb0[li + lxb * VEC], h_down);
        ldv<T, VEC>(&s_xb0[li - lxb * VEC], h_up);
        ldv<T, VEC>(&s_py0[li - lxb * VEC], h_pyup);
        if (lx != lxb - 1) h_right = s_xb0[li + VEC];
        if (lx != 0) {
          h_left = s_xb0[li - 1];
          h_pxleft = s_px0[slot - 1];
        }
        // (the halo-free parts of stage 1 stay below the exchange: hoisted above the
        // barrier they hold their results across it and the kernel spills)
        __builtin_amdgcn_sched_barrier(0);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          h_down[j] = L.xdown[j];
          h_up[j] = L.xup[j];
          h_pyup[j] = L.pyup[j];
        }
      }
      T nb = __shfl_down(P.xc[0], 1, kWave);
      if (row_end) nb = h_right;
      const T sm0 = sigm(0), tm0 = taum(0), su0 = sigu(0);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const T hx = (j + 1 < VEC) ? P.xc[(j + 1) % VEC] : nb;
        f_px[j] = dual_update_u<HUBER, UNIT>(L.pxo[j], hx, P.xc[j], G.wx, sm0, S.hden[0]);
      }
      dual_vec<HUBER, UNIT>(f_py, L.pyo, h_down, P.xc, G.wy, sm0, S.hden[0]);
      dual_vec<HUBER, UNIT>(pzn[0], L.pzo, L.xn, P.xc, G.wz, sm0, S.hden[0]);
      T pxl = __shfl_up(f_px[VEC - 1], 1, kWave);
      if (row_beg)
        pxl = g_l ? dual_update_u<HUBER, UNIT>(h_pxleft, P.xc[0], h_left, G.wx, S.sigma[0],
                                         S.hden[0])
                  : T(0);
      // the upper neighbour's new dual; without one, pyup = xup = 0 (offset out
      // of range) and sig_u = 0 make it exactly zero
      T puv[VEC];
      dual_vec<HUBER, UNIT>(puv, h_pyup, P.xc, h_up, G.wy, su0, S.hden[0]);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const T pu = puv[j];
        const T pl = (j > 0) ? f_px[(j + VEC - 1) % VEC] : pxl;
        T kt = adj_term<UNIT>(f_px[j], pl, G.wx);
        kt += adj_term<UNIT>(f_py[j], pu, G.wy);
        kt += adj_term<UNIT>(pzn[0][j], P.pz[0][j], G.wz);
        const T u = L.xv[j] - tm0 * kt;
        const T xnew = prox_data_s<L1>(u, L.btn[j], S.tl[0], S.optl[0]);
        fr_x[0][j] = xnew;
        fr_xb[0][j] = xnew + S.theta[0] * (xnew - L.xv[j]);
        fr_bt[0][j] = L.btn[j];
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) N.xc[j] = L.xn[j];
      cut_tail(N.xc);
      if constexpr (K > 1) cut_tail(fr_xb[0]);
      if constexpr (!PF2) issue_loads(L, more ? s + 1 : s, more ? adv + szb : adv);
    } else {
      // (LH: the arrays of the later stages have one copy -- the barrier that stage 1's
      // exchange brings in a full step separates this step's writes from the reads of
      // the step before here too)
      if constexpr (LH) __syncthreads();
      zero(fr_xb[0]); zero(fr_x[0]); zero(fr_bt[0]); zero(pzn[0]);
      zero(f_px); zero(f_py);
#pragma unroll
      for (int j = 0; j < VEC; ++j) N.xc[j] = P.xc[j];
    }

    // ================= F_k: finish iteration n+k on plane s-(k-1) ===========
#pragma unroll
    for (int k = 2; k <= K; ++k) {
      const int f = s - (k - 1);
      // below the volume and above it everything is zero padding
      const bool inr = f >= 0 && f < nzi;
      // the last stage needs no per-lane masks: what it computes for a voxel
      // outside the volume is neither stored nor read by anyone
      // (wneed first: sigm / taum are formed by volatile instructions)
      if (!wneed[k - 1]) {                         // wave-uniform
        zero(fr_x[k - 1]); zero(fr_xb[k - 1]); zero(fr_bt[k - 1]); zero(pzn[k - 1]);
        continue;
      }
      const T sk = inr ? (k == K ? S.sigma[K - 1] : sigm(k - 1)) : T(0);
      const T tk = inr ? (k == K ? S.tau[K - 1] : taum(k - 1)) : T(0);
      T pkz[VEC];
      dual_vec<HUBER, UNIT>(pkz, P.pz[k - 2], fr_xb[k - 2], P.c_xb[k - 1], G.wz, sk,
                            S.hden[k - 1]);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        T kt = P.c_kt[k - 1][j];
        kt += adj_term<UNIT>(pkz[j], P.pz[k - 1][j], G.wz);
        const T u = P.c_x[k - 1][j] - tk * kt;
        const T xk = prox_data_s<L1>(u, P.c_bt[k - 1][j], S.tl[k - 1], S.optl[k - 1]);
        fr_x[k - 1][j] = xk;
        fr_xb[k - 1][j] = xk + S.theta[k - 1] * (xk - P.c_x[k - 1][j]);
        fr_bt[k - 1][j] = P.c_bt[k - 1][j];
        pzn[k - 1][j] = pkz[j];
      }
      if (k < K) cut_tail(fr_xb[k - 1]);
      if (k == K && f >= zbeg && f < zend) {      // uniform
        const uint32_t vo = v_st + (adv - (uint32_t)(K - 1) * szb);
        store_vec(w_pz, vo, pkz);
        store_vec(w_x, vo, fr_x[K - 1]);
        store_vec(w_xb, vo, fr_xb[K - 1]);
      }
    }

    // ================= IP_k: in-plane part of iteration n+k on plane s-(k-2) =
    const int buf = LH ? 0 : (int)(s & 1);
#pragma unroll
    for (int k = 2; k <= K; ++k) {
      stv<T, VEC>(&s_xb[buf][k - 2][li], fr_xb[k - 2]);
      if (k == 2) {
        stv<T, VEC>(&s_py[buf][0][li], f_py);
        s_px[buf][0][slot] = f_px[VEC - 1];
      } else {
        stv<T, VEC>(&s_py[buf][k - 2][li], P.c_py[k - 1]);
        s_px[buf][k - 2][slot] = P.c_px[k - 1][VEC - 1];
      }
    }
#if !(PDK_ABLATE & 4)
    __syncthreads();
#endif
    T n_kt[K][VEC], n_px[K][VEC], n_py[K][VEC];
#pragma unroll
    for (int k = 2; k <= K; ++k) {
      if (!wneed[k - 1]) {                         // wave-uniform
        zero(n_kt[k - 1]); zero(n_px[k - 1]); zero(n_py[k - 1]);
        continue;
      }
      T below[VEC], above[VEC], above_py[VEC];
      ldv<T, VEC>(&s_xb[buf][k - 2][li + lxb * VEC], below);
      ldv<T, VEC>(&s_xb[buf][k - 2][li - lxb * VEC], above);
      ldv<T, VEC>(&s_py[buf][k - 2][li - lxb * VEC], above_py);
      T right = s_xb[buf][k - 2][li + VEC];
      if (!n_r) right = T(0);
      const T left_xb = s_xb[buf][k - 2][li - 1];
      const T left_px = s_px[buf][k - 2][slot - 1];
      const T pl0 = v_l ? dual_update_u<HUBER, UNIT>(left_px, fr_xb[k - 2][0], left_xb, G.wx,
                                               S.sigma[k - 1], S.hden[k - 1])
                        : T(0);
      T pkx[VEC], pky[VEC], puv[VEC];
      const T sgk = (k == K) ? S.sigma[K - 1] : sigm(k - 1);    // see F_k
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const T px_old = (k == 2) ? f_px[j] : P.c_px[k - 1][j];
        const T hx = (j + 1 < VEC) ? fr_xb[k - 2][(j + 1) % VEC] : right;
        pkx[j] = dual_update_u<HUBER, UNIT>(px_old, hx, fr_xb[k - 2][j], G.wx, sgk,
                                      S.hden[k - 1]);
      }
      if (k == 2)
        dual_vec<HUBER, UNIT>(pky, f_py, below, fr_xb[k - 2], G.wy, sgk, S.hden[k - 1]);
      else
        dual_vec<HUBER, UNIT>(pky, P.c_py[k - 1], below, fr_xb[k - 2], G.wy, sgk,
                              S.hden[k - 1]);
      dual_vec<HUBER, UNIT>(puv, above_py, fr_xb[k - 2], above, G.wy, sigu(k - 1),
                            S.hden[k - 1]);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const T pu = puv[j];
        const T pl = (j > 0) ? pkx[(j + VEC - 1) % VEC] : pl0;
        T kt = adj_term<UNIT>(pkx[j], pl, G.wx);
        kt += adj_term<UNIT>(pky[j], pu, G.wy);
        n_kt[k - 1][j] = kt;
        n_px[k - 1][j] = pkx[j];
        n_py[k - 1][j] = pky[j];
      }
      if (k == K) {
        const int a = s - (K - 2);
        if (a >= zbeg && a < zend) {              // uniform
          const uint32_t vo = v_st + (adv - (uint32_t)(K - 2) * szb);
          store_vec(w_px, vo, pkx);
          store_vec(w_py, vo, pky);
        }
      }
    }

    // ================= next state ==========================================
#pragma unroll
    for (int k = K; k >= 2; --k) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        N.c_xb[k - 1][j] = fr_xb[k - 2][j];
        N.c_x[k - 1][j] = fr_x[k - 2][j];
        N.c_bt[k - 1][j] = fr_bt[k - 2][j];
        N.c_kt[k - 1][j] = n_kt[k - 1][j];
        if (k < K) {
          N.c_px[k][j] = n_px[k - 1][j];
          N.c_py[k][j] = n_py[k - 1][j];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < VEC; ++j) N.pz[k][j] = pzn[k][j];
    adv += szb;
  };

  __syncthreads();   // LDS padding rows are zero before anyone reads them
  int s = s_first;
  if constexpr (PF2) {
    // 8 waves: registers to spare -> two load sets and two state sets
    for (; s + 1 <= s_hi; s += 2) {
      step(std::true_type{}, s, LA, LB, CA, CB);
      step(std::true_type{}, s + 1, LB, LA, CB, CA);
    }
    if (s <= s_hi) {
      step(std::true_type{}, s, LA, LB, CA, CB);
      CA = CB;
      ++s;
    }
  } else {
    // one set of each, updated in place (a step writes its state last)
    for (; s <= s_hi; ++s) step(std::true_type{}, s, LA, LA, CA, CA);
  }
  for (; s <= s_last; ++s)       // at most K-1 drain steps
    step(std::false_type{}, s, LA, LA, CA, CA);
  PDK_PROBE_MARK(1);
}

// ---------------------------------------------------------------------------
// The SHIFTED depth-3 form: a run cut after the dual step instead of after the
// primal step.  Once p^{n+1} exists nothing reads xbar^n any more (the primal update
// reads x^n, bt and p^{n+1}; xbar^{n+1} is formed from x^{n+1} and x^n), so the state
// that crosses such a cut is (x^n, p^{n+1}): four words instead of five.  A launch runs
//   P_1 D_2 P_2 D_3 P_3 D_4
// -- the same six half-steps as k_pd_fusedk's D P D P D P, the same arithmetic per
// voxel in the same order -- reads x, bt, p[3] and writes x, p[3]: 9 words per voxel
// instead of 11.  nsol_pd.hip's run loop puts a stand-alone dual step in front of a
// block of such launches and a stand-alone primal step behind it.
//
// Pipeline at step s (one barrier per step, LDS arrays double buffered by step parity):
//   stage 1   primal only, plane s: K^T of the LOADED p^(1) (own vectors, p_y of the row
//             above and the one p_x left of a wave / row start from L1/L2, p_z of the
//             plane before carried from the previous step's load);
//   F_2, F_3  as in k_pd_fusedk, planes s-1, s-2 (stage 3 keeps its per-lane masks: its
//             xbar IS read here, by stage 4); x^(3) is stored at plane s-2;
//   IP_2      plane s: the recomputed p^(2) of the left / upper voxel starts from the
//             same loaded p^(1) halo stage 1 used, so only p^(2) travels through the LDS;
//   IP_3      plane s-1: p_x^(3), p_y^(3) are carried a step instead of being stored;
//   IP_4      plane s-2: p_x^(4), p_y^(4) from xbar^(3) of the right neighbour and the
//             row below (a third s_xb set), stored there;
//   F_4       plane s-3: p_z^(4) from xbar^(3) of that plane (carried) and of plane s-2.
// Dependency cone: the last dual step needs xbar^(3) one row further down, one voxel
// further right and one plane further up than a launch of k_pd_fusedk does, so a
// footprint keeps rows [2, rows-4] (2 above, 3 below: rows - 5 valid), the x halo is
// HX >= K voxels wide (3 needed on the right) and a z-chunk runs one step longer.
template <typename T>
struct ShiftScalars {
  T sigma[4], hden[4];                     // [k-1]: the dual step of stage k (k = 2..4)
  T tau[3], tl[3], optl[3], theta[3];      // [k-1]: the primal step of stage k (k = 1..3)
};

template <typename T, int V>
struct ShiftLoads {          // registers one prefetched plane lands in
  T xv[V], btn[V], pxo[V], pyo[V], pzo[V], pyup[V];
  T pxleft;
};

template <typename T, int VEC, int NW, int WPE, bool HUBER, bool L1, bool PF2, bool UNIT>
__global__ __launch_bounds__(NW * 64, WPE) void k_pd_shift3(
    const T *__restrict__ x_in, T *__restrict__ x_out, const T *__restrict__ bt,
    const T *__restrict__ p_in, T *__restrict__ p_out, Geom<T> G, ShiftScalars<T> S,
    Tiling Q, int zchunk, PdkBlockMap M) {
  constexpr int K = 3;
  constexpr int NT = NW * 64;
  constexpr int HA = 2, HB = 3;                      // rows lost above / below
  constexpr int HX = ((K + VEC - 1) / VEC) * VEC;
  static_assert(HX >= K, "the x halo must hold the three voxels the right-hand cone needs");
  constexpr int LN = LdsShape<NT, K>::N;
  __shared__ __attribute__((aligned(16))) T s_xb[2][K][LN * VEC];   // xbar^(1..3)
  __shared__ __attribute__((aligned(16))) T s_py[2][LN * VEC];      // p_y^(2)
  __shared__ T s_px[2][LN];                                         // last p_x^(2) of a vector

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  int tile, zc;
  if (!pdk_block_tile(M, (int)blockIdx.x, tile, zc)) return;
  PDK_PROBE_MARK(0);
  const int tx = tile % Q.ntx;
  const int ty = tile / Q.ntx;

  // ---- geometry of this lane (lane mappings as in k_pd_fusedk)
  const int lxb = Q.lxb;
  constexpr int HL = HX / VEC;
  int row, lx;
  bool lone = false;
  if (Q.split) {
    const int inner = lxb - 2 * HL;
    const int main = Q.rows * inner;
    if (tid < main) {
      row = tid / inner;
      lx = HL + (tid - row * inner);
      lone = (lx == HL) || (lx == HL + inner - 1);
    } else {
      const int h = tid - main;
      row = h / (2 * HL);
      const int side = h - row * (2 * HL);
      lx = side < HL ? side : inner + side;
      lone = true;
    }
  } else {
    row = tid / lxb;
    lx = tid - row * lxb;
  }
  const bool active = row < Q.rows;
  const bool single_x = (Q.xv == 0);
  const int64_t xv_lo = single_x ? 0 : (int64_t)tx * Q.xv;
  const int64_t xv_hi = single_x ? G.nx : xv_lo + Q.xv;
  const int64_t x0 = (single_x ? 0 : xv_lo - HX) + (int64_t)lx * VEC;
  const int64_t tyv = Q.rows - (HA + HB);
  const int64_t yv_lo = (int64_t)ty * tyv;
  const int64_t yv_hi = yv_lo + tyv;
  const int64_t y = yv_lo - HA + row;
  const bool rin = active && x0 >= 0 && x0 < G.nx && y >= 0 && y < G.ny;
  const bool rvalid = rin && x0 >= xv_lo && x0 < xv_hi && y >= yv_lo && y < yv_hi;

  // step sizes masked to zero outside the volume, for every stage whose xbar is read
  // by a later one -- all three here
  T sig_m[K], tau_m[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    sig_m[k] = rin ? S.sigma[k] : T(0);
    tau_m[k] = rin ? S.tau[k] : T(0);
  }

  const int nzi = (int)G.nz;
  const int zbeg = zc * zchunk;
  int zend = zbeg + zchunk;
  if (zend > nzi) zend = nzi;
  const int s_first = zbeg > HA ? zbeg - HA : 0;
  const int s_last = zend + K - 1;
  const int s_hi = s_last < nzi - 1 ? s_last : nzi - 1;   // last step with a stage 1

  // ---- buffer resources over the planes [pz0, pe) this workgroup touches
  const int pz0 = s_first > 0 ? s_first - 1 : 0;
  int pe = s_last + 1;
  if (pe > nzi) pe = nzi;
  const uint32_t szb = (uint32_t)(G.sz * (int64_t)sizeof(T));
  const uint32_t syb = (uint32_t)(G.sy * (int64_t)sizeof(T));
  const uint32_t span = (uint32_t)(pe - pz0) * szb;       // < 2^30 (host-checked)
  const int64_t boff = (int64_t)pz0 * G.sz;
  const rsrc_t r_x = make_rsrc(x_in + boff, span);
  const rsrc_t r_bt = make_rsrc(bt + boff, span);
  const rsrc_t r_px = make_rsrc(p_in + boff, span);
  const rsrc_t r_py = make_rsrc(p_in + G.n + boff, span);
  const rsrc_t r_pz = make_rsrc(p_in + 2 * G.n + boff, span);
  const rsrc_t w_x = make_rsrc(x_out + boff, span);
  const rsrc_t w_px = make_rsrc(p_out + boff, span);
  const rsrc_t w_py = make_rsrc(p_out + G.n + boff, span);
  const rsrc_t w_pz = make_rsrc(p_out + 2 * G.n + boff, span);

  const bool row_beg = (lx == 0) || lane == 0 || lone;
  const uint32_t o0 = (uint32_t)((y * G.sy + x0) * (int64_t)sizeof(T));
  const uint32_t v_own = rin ? o0 : kInvalid;
  const uint32_t v_up = (rin && y > 0) ? o0 - syb : kInvalid;
  const uint32_t v_left = (rin && row_beg && x0 > 0) ? o0 - (uint32_t)sizeof(T) : kInvalid;
  const uint32_t v_st = rvalid ? o0 : kInvalid;
  const bool n_r = active && lx < lxb - 1;
  const bool v_l = rin && lx > 0 && x0 > 0;      // the left / upper voxel is in the volume
  const bool v_u = rin && row > 0 && y > 0;
  const int slot = active ? (row + 1) * lxb + lx : tid + lxb;
  const int li = slot * VEC;
  T sig_u[K];
#pragma unroll
  for (int k = 1; k < K; ++k) sig_u[k] = v_u ? S.sigma[k] : T(0);
  // Stage k (2, 3) is exact k-1 rows inside the footprint; stage 3 is used up to the first
  // voxel of the right x halo (stage 4's right neighbour), stage 4 on the stored voxels.
  bool wneed[K + 1];
  wneed[0] = true;
#pragma unroll
  for (int k = 2; k <= K + 1; ++k) {
    const bool in_x = single_x || k < K ||
                      (lx >= HL && (k == K ? lx <= lxb - HL : lx < lxb - HL));
    const int last = k <= K ? Q.rows - k : Q.rows - 1 - HB;
    const bool mine = active && row >= (k <= K ? k - 1 : HA) && row <= last && in_x;
    wneed[k - 1] = __ballot(mine) != 0ull;
  }

  // zero rows above and below the footprint, once
  for (int i = tid; i < 2 * lxb * VEC; i += NT) {
    const int e = i % (lxb * VEC);
    const int at = i >= lxb * VEC ? (Q.rows + 1) * lxb * VEC + e : e;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int kk = 0; kk < K; ++kk) s_xb[b][kk][at] = T(0);
      s_py[b][at] = T(0);
    }
  }

  struct Carry {
    T pz[K][VEC];           // pz[k-1]: p^(k)_z on the plane stage k finished last
    T c_xb[K + 1][VEC];     // [k-1], k = 2..4: xbar^(k-1) on plane s-(k-1)
    T c_x[K][VEC];          //        k = 2..3:    x^(k-1) there
    T c_bt[K][VEC];         //                     bt there
    T c_kt[K][VEC];         //                     in-plane part of K^T p^(k) there
    T c_px[K + 1][VEC];     // [k-1], k = 3..4: p_x^(k-1) on plane s-(k-2) (from IP_{k-1})
    T c_py[K + 1][VEC];
  };
  Carry CA, CB;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    zero(CA.pz[k]); zero(CA.c_x[k]); zero(CA.c_bt[k]); zero(CA.c_kt[k]);
  }
#pragma unroll
  for (int k = 0; k <= K; ++k) { zero(CA.c_xb[k]); zero(CA.c_px[k]); zero(CA.c_py[k]); }
  uint32_t adv = (uint32_t)(s_first - pz0) * szb;   // scalar offset of plane s
  // p_z^(1) of the plane below the first one (zero at the bottom of the volume)
  bld<T, VEC>(r_pz, s_first > 0 ? v_own : kInvalid, s_first > 0 ? adv - szb : 0u, CA.pz[0]);

  typedef ShiftLoads<T, VEC> Loads;
  Loads LA, LB;
  auto issue_loads = [&](Loads &L, uint32_t a) {
    bld<T, VEC>(r_x, v_own, a, L.xv);
    bld<T, VEC>(r_bt, v_own, a, L.btn);
    bld<T, VEC>(r_px, v_own, a, L.pxo);
    bld<T, VEC>(r_py, v_own, a, L.pyo);
    bld<T, VEC>(r_pz, v_own, a, L.pzo);
    bld<T, VEC>(r_py, v_up, a, L.pyup);
    L.pxleft = bld1<T>(r_px, v_left, a);
  };
  issue_loads(LA, adv);

  auto step = [&](auto have1_tag, int s, Loads &L, Loads &LN, const Carry &P,
                  Carry &N) {
    constexpr bool HAVE1 = decltype(have1_tag)::value;
    // fr_*[k-1]: results of stage k produced in this step
    T fr_xb[K][VEC], fr_x[K][VEC], fr_bt[K][VEC], pzn[K][VEC];
    T f_px[VEC], f_py[VEC], h_pyup[VEC];
    T pxl;                       // p_x^(1) of the voxel left of this lane's vector
    if constexpr (HAVE1) {
      const bool more = s + 1 <= s_hi;
      if constexpr (PF2) issue_loads(LN, more ? adv + szb : adv);
      // ================= stage 1: the primal half of iteration n+1 on plane s ==
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        f_px[j] = L.pxo[j];
        f_py[j] = L.pyo[j];
        pzn[0][j] = L.pzo[j];
        h_pyup[j] = L.pyup[j];
      }
      pxl = __shfl_up(f_px[VEC - 1], 1, kWave);
      if (row_beg) pxl = L.pxleft;
      const T tm0 = tau_m[0];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const T pl = (j > 0) ? f_px[(j + VEC - 1) % VEC] : pxl;
        T kt = adj_term<UNIT>(f_px[j], pl, G.wx);
        kt += adj_term<UNIT>(f_py[j], h_pyup[j], G.wy);
        kt += adj_term<UNIT>(pzn[0][j], P.pz[0][j], G.wz);
        const T u = L.xv[j] - tm0 * kt;
        const T xnew = prox_data_s<L1>(u, L.btn[j], S.tl[0], S.optl[0]);
        fr_x[0][j] = xnew;
        fr_xb[0][j] = xnew + S.theta[0] * (xnew - L.xv[j]);
        fr_bt[0][j] = L.btn[j];
      }
      if constexpr (!PF2) issue_loads(L, more ? adv + szb : adv);
    } else {
      zero(fr_xb[0]); zero(fr_x[0]); zero(fr_bt[0]); zero(pzn[0]);
      zero(f_px); zero(f_py); zero(h_pyup);
      pxl = T(0);
    }

    // ================= F_k: finish iteration n+k on plane s-(k-1) ===========
    const int a = s - (K - 1);                     // the plane x, p_x, p_y are stored at
    const bool st_a = a >= zbeg && a < zend;       // uniform
#pragma unroll
    for (int k = 2; k <= K; ++k) {
      const int f = s - (k - 1);
      const bool inr = f >= 0 && f < nzi;
      if (!wneed[k - 1]) {                         // wave-uniform
        zero(fr_x[k - 1]); zero(fr_xb[k - 1]); zero(fr_bt[k - 1]); zero(pzn[k - 1]);
        continue;
      }
      const T sk = inr ? sig_m[k - 1] : T(0);
      const T tk = inr ? tau_m[k - 1] : T(0);
      T pkz[VEC];
      dual_vec<HUBER, UNIT>(pkz, P.pz[k - 2], fr_xb[k - 2], P.c_xb[k - 1], G.wz, sk,
                            S.hden[k - 1]);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        T kt = P.c_kt[k - 1][j];
        kt += adj_term<UNIT>(pkz[j], P.pz[k - 1][j], G.wz);
        const T u = P.c_x[k - 1][j] - tk * kt;
        const T xk = prox_data_s<L1>(u, P.c_bt[k - 1][j], S.tl[k - 1], S.optl[k - 1]);
        fr_x[k - 1][j] = xk;
        fr_xb[k - 1][j] = xk + S.theta[k - 1] * (xk - P.c_x[k - 1][j]);
        fr_bt[k - 1][j] = P.c_bt[k - 1][j];
        pzn[k - 1][j] = pkz[j];
      }
      if (k == K && st_a)
        bst<T, VEC>(w_x, v_st + (adv - (uint32_t)(K - 1) * szb), fr_x[K - 1]);
    }
    // ================= F_4: the z component of the last dual step, plane s-K ===
    if (wneed[K]) {
      const int f = s - K;
      if (f >= zbeg && f < zend) {                 // uniform
        T pkz[VEC];
        dual_vec<HUBER, UNIT>(pkz, P.pz[K - 1], fr_xb[K - 1], P.c_xb[K], G.wz, S.sigma[K],
                              S.hden[K]);
        bst<T, VEC>(w_pz, v_st + (adv - (uint32_t)K * szb), pkz);
      }
    }

    // ================= IP_k: in-plane part of iteration n+k on plane s-(k-2) =
    const int buf = (int)(s & 1);
#pragma unroll
    for (int k = 2; k <= K + 1; ++k) stv<T, VEC>(&s_xb[buf][k - 2][li], fr_xb[k - 2]);
    stv<T, VEC>(&s_py[buf][li], P.c_py[K - 1]);
    s_px[buf][slot] = P.c_px[K - 1][VEC - 1];
    __syncthreads();
    T n_kt[K][VEC], n_px[K][VEC], n_py[K][VEC];
#pragma unroll
    for (int k = 2; k <= K; ++k) {
      if (!wneed[k - 1]) {                         // wave-uniform
        zero(n_kt[k - 1]); zero(n_px[k - 1]); zero(n_py[k - 1]);
        continue;
      }
      T below[VEC], above[VEC], above_py[VEC];
      ldv<T, VEC>(&s_xb[buf][k - 2][li + lxb * VEC], below);
      ldv<T, VEC>(&s_xb[buf][k - 2][li - lxb * VEC], above);
      if (k == 2) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) above_py[j] = h_pyup[j];
      } else {
        ldv<T, VEC>(&s_py[buf][li - lxb * VEC], above_py);
      }
      T right = s_xb[buf][k - 2][li + VEC];
      if (!n_r) right = T(0);
      const T left_xb = s_xb[buf][k - 2][li - 1];
      const T left_px = (k == 2) ? pxl : s_px[buf][slot - 1];
      const T pl0 = v_l ? dual_update_u<HUBER, UNIT>(left_px, fr_xb[k - 2][0], left_xb, G.wx,
                                               S.sigma[k - 1], S.hden[k - 1])
                        : T(0);
      T pkx[VEC], pky[VEC], puv[VEC];
      const T sgk = sig_m[k - 1];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const T px_old = (k == 2) ? f_px[j] : P.c_px[k - 1][j];
        const T hx = (j + 1 < VEC) ? fr_xb[k - 2][(j + 1) % VEC] : right;
        pkx[j] = dual_update_u<HUBER, UNIT>(px_old, hx, fr_xb[k - 2][j], G.wx, sgk,
                                      S.hden[k - 1]);
      }
      if (k == 2)
        dual_vec<HUBER, UNIT>(pky, f_py, below, fr_xb[k - 2], G.wy, sgk, S.hden[k - 1]);
      else
        dual_vec<HUBER, UNIT>(pky, P.c_py[k - 1], below, fr_xb[k - 2], G.wy, sgk,
                              S.hden[k - 1]);
      dual_vec<HUBER, UNIT>(puv, above_py, fr_xb[k - 2], above, G.wy, sig_u[k - 1],
                            S.hden[k - 1]);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const T pl = (j > 0) ? pkx[(j + VEC - 1) % VEC] : pl0;
        T kt = adj_term<UNIT>(pkx[j], pl, G.wx);
        kt += adj_term<UNIT>(pky[j], puv[j], G.wy);
        n_kt[k - 1][j] = kt;
        n_px[k - 1][j] = pkx[j];
        n_py[k - 1][j] = pky[j];
      }
    }
    // ================= IP_4: p_x, p_y of the last dual step on plane s-(K-1) ===
    // (no K^T follows it: neither the left nor the upper voxel's dual is recomputed)
    if (wneed[K] && st_a) {
      T below[VEC], pkx[VEC], pky[VEC];
      ldv<T, VEC>(&s_xb[buf][K - 1][li + lxb * VEC], below);
      T right = s_xb[buf][K - 1][li + VEC];
      if (!n_r) right = T(0);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const T hx = (j + 1 < VEC) ? fr_xb[K - 1][(j + 1) % VEC] : right;
        pkx[j] = dual_update_u<HUBER, UNIT>(P.c_px[K][j], hx, fr_xb[K - 1][j], G.wx,
                                      S.sigma[K], S.hden[K]);
      }
      dual_vec<HUBER, UNIT>(pky, P.c_py[K], below, fr_xb[K - 1], G.wy, S.sigma[K], S.hden[K]);
      const uint32_t vo = v_st + (adv - (uint32_t)(K - 1) * szb);
      bst<T, VEC>(w_px, vo, pkx);
      bst<T, VEC>(w_py, vo, pky);
    }

    // ================= next state ==========================================
#pragma unroll
    for (int k = K + 1; k >= 2; --k) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        N.c_xb[k - 1][j] = fr_xb[k - 2][j];
        if (k <= K) {
          N.c_x[k - 1][j] = fr_x[k - 2][j];
          N.c_bt[k - 1][j] = fr_bt[k - 2][j];
          N.c_kt[k - 1][j] = n_kt[k - 1][j];
          N.c_px[k][j] = n_px[k - 1][j];
          N.c_py[k][j] = n_py[k - 1][j];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < VEC; ++j) N.pz[k][j] = pzn[k][j];
    adv += szb;
  };

  __syncthreads();   // LDS padding rows are zero before anyone reads them
  int s = s_first;
  if constexpr (PF2) {
    for (; s + 1 <= s_hi; s += 2) {
      step(std::true_type{}, s, LA, LB, CA, CB);
      step(std::true_type{}, s + 1, LB, LA, CB, CA);
    }
    if (s <= s_hi) {
      step(std::true_type{}, s, LA, LB, CA, CB);
      CA = CB;
      ++s;
    }
  } else {
    for (; s <= s_hi; ++s) step(std::true_type{}, s, LA, LA, CA, CA);
  }
  for (; s <= s_last; ++s)       // at most K drain steps
    step(std::false_type{}, s, LA, LA, CA, CA);
  PDK_PROBE_MARK(1);
}

// ---- host side: the knobs, the launchers, the plans and their events.  Which footprints
// there are, what they cost, which of them a plan lists and what the tuner makes of the
// times it gets: nsol_pdk_plan.hpp.
Tuning g_tunek;     // the knobs as they stand (nsol_hip_set_param_pdk)

// The grid of one launch of `c`: its blocks from the tiling and the block map, refused
// beyond what the kernels' 32-bit indices hold; the pdk_verbose line (`head`: the kernel).
inline int launch_grid(const Config &c, int64_t nz, const char *head, int nw, int pf2,
                       PdkBlockMap *M, unsigned *blocks) {
  const Tiling &Q = c.q;
  const int64_t tiles = (int64_t)Q.ntx * Q.nty;
  const int64_t nzc = (nz + c.zchunk - 1) / c.zchunk;
  if (tiles * nzc > 0x3fffffff) return NSOL_EINVAL;
  *M = launch_map(g_tunek, Q, nzc);
  const int64_t n = pdk_map_blocks(*M);
  if (n > 0x7fffffff) return NSOL_EINVAL;
  if (g_tunek.verbose == 1)
    fprintf(stderr, "%s waves=%d pf2=%d split=%d: lxb=%d rows=%d xv=%d tiles=%dx%d "
            "zchunk=%lld blocks=%lld map=%d:%d model=%.3f GB\n", head, nw, pf2, Q.split, Q.lxb,
            Q.rows, Q.xv, Q.ntx, Q.nty, (long long)c.zchunk, (long long)n, M->mode, M->q,
            c.cost * 1e-9);
  *blocks = (unsigned)n;
  return 0;
}

template <typename T, int VEC, int NW, int K, int WPE, bool HUBER, bool L1, bool PF2,
          bool UNIT, bool RAG>
int launch_f(const Config &c, const T *xbar_in, T *xbar_out, const T *x_in, T *x_out,
             const T *bt, const T *p_in, T *p_out, const Geom<T> &G,
             const StageScalars<T, K> &S, hipStream_t st) {
  PdkBlockMap M;
  unsigned blocks;
  if (int rc = launch_grid(c, G.nz, K == 3 ? "k_pd_fusedk K=3" : "k_pd_fusedk K=2", NW,
                           (int)PF2, &M, &blocks))
    return rc;
  hipLaunchKernelGGL((k_pd_fusedk<T, VEC, NW, K, WPE, HUBER, L1, PF2, UNIT, RAG>),
                     dim3(blocks), dim3(NW * 64), 0, st, xbar_in, xbar_out,
                     x_in, x_out, bt, p_in, p_out, G, S, c.q, (int)c.zchunk, M);
  g_launches[K == 3 ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
  return launch_status();
}

template <typename T, int VEC, int NW, int K, int WPE, bool PF2, bool RAG>
int launch_k(const Config &c, const T *xbar_in, T *xbar_out, const T *x_in, T *x_out,
             const T *bt, const T *p_in, T *p_out, const Geom<T> &G,
             const StageScalars<T, K> &S, int flags, hipStream_t st) {
#define NSOL_F(HB, L)                                                           \
  (unit ? launch_f<T, VEC, NW, K, WPE, HB, L, PF2, true, RAG>(                  \
              c, xbar_in, xbar_out, x_in, x_out, bt, p_in, p_out, G, S, st)     \
        : launch_f<T, VEC, NW, K, WPE, HB, L, PF2, false, RAG>(                 \
              c, xbar_in, xbar_out, x_in, x_out, bt, p_in, p_out, G, S, st))
  const bool unit = G.wx == T(1) && G.wy == T(1) && G.wz == T(1);
  const bool huber = (flags & NSOL_PD_REG_HUBER) != 0;
  const bool l1 = (flags & NSOL_PD_DATA_L1) != 0;
  if (huber) return l1 ? NSOL_F(true, true) : NSOL_F(true, false);
  return l1 ? NSOL_F(false, true) : NSOL_F(false, false);
#undef NSOL_F
}

// the workgroup sizes candidates() offers per depth, each with its compiled form
template <typename T, int K>
int launch_cfg(const Config &c, const T *xbar_in, T *xbar_out, const T *x_in,
               T *x_out, const T *bt, const T *p_in, T *p_out, const Geom<T> &G,
               const StageScalars<T, K> &S, int flags, hipStream_t st) {
  constexpr int VW = 16 / sizeof(T);
#define NSOL_W(NWV, WPE, PF)                                                      \
  launch_k<T, VW, NWV, K, WPE, PF, false>(c, xbar_in, xbar_out, x_in, x_out, bt,    \
                                          p_in, p_out, G, S, flags, st)
  // rows that are not a multiple of the vector width: 12-wave workgroups only
  // (candidates() offers nothing else for such shapes)
  if (G.nx % VW != 0) {
    if (c.nw != 12) return NSOL_EINVAL;
    return launch_k<T, VW, 12, K, 3, false, true>(c, xbar_in, xbar_out, x_in, x_out, bt,
                                                  p_in, p_out, G, S, flags, st);
  }
  // two prefetch register sets where the register file has room for them
  if (c.nw == 8) return c.pf2 ? NSOL_W(8, 2, true) : NSOL_W(8, 2, false);
  if constexpr (K == 2) {
    if (c.nw == 12) return NSOL_W(12, 3, false);
    if (c.nw == 16) return NSOL_W(16, 4, false);
  } else {
    if (c.nw == 12) return NSOL_W(12, 3, false);
  }
#undef NSOL_W
  return NSOL_EINVAL;
}

template <typename T, int VEC, int NW, int WPE, bool PF2>
int launch_shift(const Config &c, const T *x_in, T *x_out, const T *bt, const T *p_in,
                 T *p_out, const Geom<T> &G, const ShiftScalars<T> &S, int flags,
                 hipStream_t st) {
  PdkBlockMap M;
  unsigned blocks;
  if (int rc = launch_grid(c, G.nz, "k_pd_shift3", NW, (int)PF2, &M, &blocks)) return rc;
#define NSOL_S(HB, L, U)                                                             \
  hipLaunchKernelGGL((k_pd_shift3<T, VEC, NW, WPE, HB, L, PF2, U>), dim3(blocks),    \
                     dim3(NW * 64), 0, st, x_in, x_out, bt, p_in, p_out, G, S, c.q,  \
                     (int)c.zchunk, M)
#define NSOL_SU(HB, L) do { if (unit) NSOL_S(HB, L, true); else NSOL_S(HB, L, false); } while (0)
  const bool unit = G.wx == T(1) && G.wy == T(1) && G.wz == T(1);
  const bool huber = (flags & NSOL_PD_REG_HUBER) != 0;
  const bool l1 = (flags & NSOL_PD_DATA_L1) != 0;
  if (huber) { if (l1) NSOL_SU(true, true); else NSOL_SU(true, false); }
  else { if (l1) NSOL_SU(false, true); else NSOL_SU(false, false); }
#undef NSOL_SU
#undef NSOL_S
  g_launches[1].fetch_add(1, std::memory_order_relaxed);
  g_shift_launches.fetch_add(1, std::memory_order_relaxed);
  return launch_status();
}

// ---- the plans of this process and the events of their samples in flight: a sampled
// launch is bracketed by two events that are read back later with hipEventQuery
struct Sample { hipEvent_t e0, e1; int cand; };
struct Tuned {
  Plan P;
  std::deque<Sample> pending;
};
std::map<PlanKey, Tuned> g_plans;
std::mutex g_plans_mutex;

inline int current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  return dev;
}
// the plan of a shape on the current device, null if there is none (g_plans_mutex held)
inline Tuned *find_plan(int esize, int k, int64_t nz, int64_t ny, int64_t nx, int64_t pitch,
                        int form) {
  auto it = g_plans.find(PlanKey{current_device(), esize, k, nz, ny, nx, pitch, form});
  return it == g_plans.end() ? nullptr : &it->second;
}

// hand the samples that have come back to the plan; settle it once all are in
inline void plan_poll(Tuned &E, int K) {
  Plan &P = E.P;
  while (!E.pending.empty()) {
    Sample sm = E.pending.front();
    hipError_t q = hipEventQuery(sm.e1);
    if (q == hipErrorNotReady) break;
    float ms = 0.f;
    if (q == hipSuccess && hipEventElapsedTime(&ms, sm.e0, sm.e1) == hipSuccess) {
      plan_record(P, sm.cand, ms);
    } else {
      (void)hipGetLastError();
      plan_lost(P, sm.cand);
    }
    (void)hipEventDestroy(sm.e0);
    (void)hipEventDestroy(sm.e1);
    E.pending.pop_front();
  }
  if (plan_settle(P) && g_tunek.verbose) {
    for (int i = 0; i < (int)P.cand.size(); ++i) {
      fprintf(stderr, "k_pd_fusedk tune K=%d waves=%d ntx=%d zchunk=%lld rows=%d: %.3f ms%s  [",
              K, P.cand[i].nw, P.cand[i].q.ntx, (long long)P.cand[i].zchunk, P.cand[i].q.rows,
              P.best_ms[i], i == P.chosen ? "  <- kept" : (P.dropped[i] ? "  (dropped)" : ""));
      for (float v : P.samples[i]) fprintf(stderr, " %.3f", v);
      fprintf(stderr, " ]\n");
    }
  }
}

// One launch under the plan of `key`: `go(config)` launches; `sample`: this launch may be
// timed as a sample of an exploring plan.
template <typename Go>
int planned_launch(const PlanKey &key, bool sample, hipStream_t st, Go go) {
  if (geometry_forced(g_tunek)) {      // experiments and tests: no plan, no tuning
    const std::vector<Config> cand = candidates(g_tunek, key, cu_count());
    if (cand.empty()) return -2;
    return go(cand[0]);
  }
  std::lock_guard<std::mutex> lock(g_plans_mutex);
  auto it = g_plans.find(key);
  if (it == g_plans.end()) {
    const std::vector<Config> cand = plan_candidates(g_tunek, key, cu_count());
    if (cand.empty()) return -2;
    // what the shape's depth-3 plans have to say about the new plan's list (list_kind;
    // of a shape whose long runs take the shifted block the unshifted plan may lag)
    const Tuned *u3 = find_plan(key.esize, 3, key.nz, key.ny, key.nx, key.pitch, 0);
    const Tuned *s3 = find_plan(key.esize, 3, key.nz, key.ny, key.nx, key.pitch, 1);
    const Tuned *set3 = (u3 && u3->P.chosen >= 0) ? u3 : s3;
    const Config *settled3 =
        (set3 && set3->P.chosen >= 0) ? &set3->P.cand[set3->P.chosen] : nullptr;
    it = g_plans.emplace(key, Tuned{plan_make(g_tunek, key, cand, settled3, s3 != nullptr), {}})
             .first;
  }
  Tuned &E = it->second;
  Plan &P = E.P;
  // no event queries / records on a stream that is being captured into a graph:
  // such launches use the settled plan, or the model's best while exploring
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
  if (cap != hipStreamCaptureStatusNone) return go(P.cand[P.chosen >= 0 ? P.chosen : 0]);
  plan_poll(E, key.k);
  if (P.chosen >= 0) return go(P.cand[P.chosen]);
  const PlanNext next = plan_next(P, sample);     // exploring
  const Config &c = P.cand[next.cand];
  if (!next.timed) return go(c);
  Sample sm;
  sm.cand = next.cand;
  if (hipEventCreate(&sm.e0) != hipSuccess) { (void)hipGetLastError(); return go(c); }
  if (hipEventCreate(&sm.e1) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipEventDestroy(sm.e0);
    return go(c);
  }
  (void)hipEventRecord(sm.e0, st);
  const int rc = go(c);
  (void)hipEventRecord(sm.e1, st);
  if (rc == 0) {
    P.issued[sm.cand]++;
    E.pending.push_back(sm);
  } else {
    (void)hipEventDestroy(sm.e0);
    (void)hipEventDestroy(sm.e1);
  }
  return rc;
}

template <typename T>
PlanKey plan_key(const Geom<T> &G, int k, int form) {
  return PlanKey{current_device(), (int)sizeof(T), k, G.nz, G.ny, G.nx, G.padded ? G.sy : 0,
                 form};
}

template <typename T, int K>
int fusedk_k(const T *xbar_in, T *xbar_out, const T *x_in, T *x_out, const T *bt,
             const T *p_in, T *p_out, const Geom<T> &G, const double *sigma,
             const double *hden, const double *tau, const double *tl,
             const double *theta, int flags, hipStream_t st) {
  StageScalars<T, K> S;
  for (int i = 0; i < K; ++i) {
    S.sigma[i] = (T)sigma[i]; S.hden[i] = huber_den<T>(hden[i]); S.tau[i] = (T)tau[i];
    S.tl[i] = (T)tl[i]; S.optl[i] = prox_den<T>(tl[i]); S.theta[i] = (T)theta[i];
  }
  S.has_p = p_in != nullptr ? 1 : 0;
  return planned_launch(plan_key(G, K, 0), S.has_p != 0, st, [&](const Config &cfg) {
    return launch_cfg<T, K>(cfg, xbar_in, xbar_out, x_in, x_out, bt, p_in, p_out, G, S,
                            flags, st);
  });
}

// ---- the shifted form: where it applies, and what its long runs give the short ones
// nsol_pdk_plan.hpp's plan_donation for a shape, its plans polled first
inline int shift_donation(int esize, int64_t nz, int64_t ny, int64_t nx) {
  if (!tuned_size(g_tunek, nz * ny * nx) || geometry_forced(g_tunek)) return -1;
  std::lock_guard<std::mutex> lock(g_plans_mutex);
  Tuned *S = find_plan(esize, 3, nz, ny, nx, 0, 1);
  if (!S) return 0;
  plan_poll(*S, 3);
  if (!plan_issued(S->P)) return 0;
  if (Tuned *U = find_plan(esize, 3, nz, ny, nx, 0, 0)) {
    plan_poll(*U, 3);
    return plan_donation(S->P, U->P);
  }
  // not made yet: what its first launch will make of it
  const PlanKey key{current_device(), esize, 3, nz, ny, nx, 0, 0};
  const std::vector<Config> cand = plan_candidates(g_tunek, key, cu_count());
  if (cand.empty()) return -1;
  return plan_donation(S->P, plan_make(g_tunek, key, cand, nullptr, true));
}

// does the shifted form apply to this shape under the knobs as they stand
inline bool shift_shape_ok(int esize, int ndim, int64_t nz, int64_t ny, int64_t nx,
                           int64_t pitch) {
  const int VW = esize == 4 ? 4 : 2;
  if (!g_tunek.shift || !g_tunek.enable || g_tunek.kmax < 3 || ndim != 3 || pitch > nx)
    return false;
  const int64_t n = nz * ny * nx;
  if (n < ((int64_t)g_tunek.min_kvox << 10) || nx % VW != 0 || nx / VW < 8 || ny < 8 ||
      nz < 8 || nz >= ((int64_t)1 << 30))
    return false;
  // by itself only on the volumes the online tuner handles (measured there)
  return g_tunek.shift > 0 || n >= ((int64_t)g_tunek.tune_min_mvox << 20);
}

// the shortest run of this shape that takes the shifted block (0: none): the form
// applies under the knobs as they stand and a footprint fits
inline int shift_min_iters(int esize, int ndim, int64_t nz, int64_t ny, int64_t nx,
                           int64_t pitch) {
  if (!shift_shape_ok(esize, ndim, nz, ny, nx, pitch)) return 0;
  std::lock_guard<std::mutex> lock(g_plans_mutex);
  if (geometry_forced(g_tunek) || !find_plan(esize, 3, nz, ny, nx, 0, 1))
    if (candidates(g_tunek, PlanKey{0, esize, 3, nz, ny, nx, 0, 1}, cu_count()).empty())
      return 0;
  return shift_threshold(g_tunek);
}

// The depth-k plan the reporting entries speak of (g_plans_mutex held).  Depth 3 of a shape
// whose long runs take the shifted block: that form's plan (*shifted = true) -- unless the
// process has made short runs only so far: then the unshifted plan is all there is.
inline Tuned *reported_plan(int esize, int k, int64_t nz, int64_t ny, int64_t nx,
                            bool *shifted) {
  Tuned *E = nullptr;
  if (k == 3 && shift_shape_ok(esize, 3, nz, ny, nx, 0)) E = find_plan(esize, k, nz, ny, nx, 0, 1);
  *shifted = E != nullptr;
  return E ? E : find_plan(esize, k, nz, ny, nx, 0, 0);
}
// what a settled plan has chosen; NSOL_EINVAL: no plan, or not settled
inline int report_choice(const Tuned *E, int *waves, int *ntx, int64_t *zchunk) {
  if (!E || E->P.chosen < 0) return NSOL_EINVAL;
  const Config &c = E->P.cand[E->P.chosen];
  if (waves) *waves = c.nw;
  if (ntx) *ntx = c.q.ntx;
  if (zchunk) *zchunk = c.zchunk;
  return 0;
}

}  // namespace nsol_pdk

namespace nsol {

// The shortest run of this problem that nsol_pd_run_* sends through the shifted block,
// 0 if none does: the form applies to the flags and the shape, and a footprint fits.
template <typename T>
int pd_shift3_min_iters(const T *x, const T *x_alt, const T *bt, const T *p0, const T *p1,
                        int ndim, int64_t nz, int64_t ny, int64_t nx, int flags,
                        int64_t pitch, int iterations) {
  // (a run too short for the block under any shape asks nothing else: the short runs'
  // path gains no host work -- the plan lookup and, without a plan, the candidate list
  // cost tens of microseconds in front of a run's first launch)
  if (!nsol_pdk::g_tunek.shift || iterations < nsol_pdk::shift_threshold(nsol_pdk::g_tunek))
    return 0;
  if (!x || !x_alt || !bt || !p0 || !p1 || !aligned16(x) || !aligned16(x_alt) ||
      !aligned16(bt) || !aligned16(p0) || !aligned16(p1))
    return 0;
  return nsol_pd_shift_min_iters((int)sizeof(T), ndim, nz, ny, nx, flags, pitch);
}

template <typename T>
int pd_shift3_donation(int64_t nz, int64_t ny, int64_t nx) {
  return nsol_pdk::shift_donation((int)sizeof(T), nz, ny, nx);
}

// One launch of k_pd_shift3: iterations n .. n+2's primal steps and n+1 .. n+3's dual
// steps.  sigma, hden: 4 values (iterations n .. n+3, the first unused); tau, tl, theta: 3.
// -2: the form does not apply, nothing was launched.
template <typename T>
int pd_shift3_iter(const T *x_in, T *x_out, const T *bt, const T *p_in, T *p_out, int ndim,
                   int64_t nz, int64_t ny, int64_t nx, double wx, double wy, double wz,
                   const double *sigma, const double *hden, const double *tau,
                   const double *tl, const double *theta, int flags, void *stream) {
  using namespace nsol_pdk;
  if (!x_in || !x_out || !bt || !p_in || !p_out || !sigma || !hden || !tau || !tl ||
      !theta || x_in == x_out || p_in == p_out)
    return NSOL_EINVAL;
  if (!pd_shift3_min_iters<T>(x_in, x_out, bt, p_in, p_out, ndim, nz, ny, nx, flags, 0,
                              1 << 30))
    return -2;
  constexpr int VW = 16 / sizeof(T);
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  ShiftScalars<T> S;
  for (int i = 0; i < 4; ++i) { S.sigma[i] = (T)sigma[i]; S.hden[i] = huber_den<T>(hden[i]); }
  for (int i = 0; i < 3; ++i) {
    S.tau[i] = (T)tau[i]; S.tl[i] = (T)tl[i]; S.optl[i] = prox_den<T>(tl[i]);
    S.theta[i] = (T)theta[i];
  }
  hipStream_t st = as_stream(stream);
  return planned_launch(plan_key(G, 3, 1), true, st, [&](const Config &c) {
    if (c.nw == 12)
      return launch_shift<T, VW, 12, 3, false>(c, x_in, x_out, bt, p_in, p_out, G, S, flags, st);
    if (c.nw == 8)
      return launch_shift<T, VW, 8, 2, true>(c, x_in, x_out, bt, p_in, p_out, G, S, flags, st);
    return (int)NSOL_EINVAL;
  });
}

#define NSOL_PDS_INST(T)                                                               \
  template int pd_shift3_donation<T>(int64_t, int64_t, int64_t);                         \
  template int pd_shift3_min_iters<T>(const T *, const T *, const T *, const T *,        \
                                      const T *, int, int64_t, int64_t, int64_t, int,    \
                                      int64_t, int);                                          \
  template int pd_shift3_iter<T>(const T *, T *, const T *, const T *, T *, int, int64_t, \
                                 int64_t, int64_t, double, double, double, const double *, \
                                 const double *, const double *, const double *,         \
                                 const double *, int, void *);
NSOL_PDS_INST(float)
NSOL_PDS_INST(double)
#undef NSOL_PDS_INST

// returns -2 if the kernel does not apply to this problem
template <typename T>
int pd_fusedk_iter(const T *xbar_in, T *xbar_out, const T *x_in, T *x_out, const T *bt,
                   const T *p_in, T *p_out, int ndim, int64_t nz, int64_t ny, int64_t nx,
                   double wx, double wy, double wz, int k, const double *sigma,
                   const double *hden, const double *tau, const double *tl,
                   const double *theta, int flags, void *stream, int64_t pitch) {
  using nsol_pdk::g_tunek;
  // the footprint overlap is sized for the component-wise clamp: the isotropic
  // projection (nsol_pdi.hip) has no multi-iteration form
  if (flags & (NSOL_PD_REG_ISOTROPIC | NSOL_PD_DATA_WEIGHTED)) return -2;
  NSOL_CHECK_GEOM(ndim, nz, ny, nx);
  if (!xbar_in || !xbar_out || !x_in || !x_out || !bt || !p_out || !sigma ||
      !hden || !tau || !tl || !theta || xbar_in == xbar_out || p_in == p_out ||
      x_in == x_out || k < 2 || k > 3)
    return NSOL_EINVAL;
  constexpr int VW = 16 / sizeof(T);
  if (pitch > 0 && (pitch < nx || pitch % VW != 0)) return NSOL_EINVAL;
  // (rows that are not a multiple of 16 bytes take the RAG instantiation: their
  // accesses are 4-byte aligned anyway, so only the element size matters then)
  const bool rag = nx % VW != 0;
  if (!g_tunek.enable || k > g_tunek.kmax || ndim != 3 ||
      nz * ny * nx < ((int64_t)g_tunek.min_kvox << 10) ||
      nx / VW < 8 || ny < 8 || nz < 8 || nz >= ((int64_t)1 << 30) ||
      (!rag && (!aligned16(xbar_in) || !aligned16(xbar_out) || !aligned16(x_in) ||
                !aligned16(x_out) || !aligned16(bt) || !aligned16(p_out) ||
                (p_in && !aligned16(p_in)) ||
                (nz * ny * nx) % VW != 0)))
    return -2;
  const Geom<T> G = make_geom_pitched<T>(ndim, nz, ny, nx, pitch, wx, wy, wz);
  hipStream_t st = as_stream(stream);
  if (k == 2)
    return nsol_pdk::fusedk_k<T, 2>(xbar_in, xbar_out, x_in, x_out, bt, p_in, p_out, G, sigma,
                          hden, tau, tl, theta, flags, st);
  return nsol_pdk::fusedk_k<T, 3>(xbar_in, xbar_out, x_in, x_out, bt, p_in, p_out, G, sigma,
                        hden, tau, tl, theta, flags, st);
}

#define NSOL_PDK_INST(T)                                                             \
  template int pd_fusedk_iter<T>(const T *, T *, const T *, T *, const T *, const T *, \
                                 T *, int, int64_t, int64_t, int64_t, double, double,  \
                                 double, int, const double *, const double *,          \
                                 const double *, const double *, const double *, int,  \
                                 void *, int64_t);
NSOL_PDK_INST(float)
NSOL_PDK_INST(double)
#undef NSOL_PDK_INST

}  // namespace nsol

extern "C" {

int nsol_hip_set_param_pdk(const char *name, int value) {
  using namespace nsol_pdk;
  static const struct { const char *name; int Tuning::*field; } knobs[] = {
      {"pdk_enable", &Tuning::enable},       {"pdk_kmax", &Tuning::kmax},
      {"pdk_nw", &Tuning::nw},               {"pdk_zchunk", &Tuning::zchunk},
      {"pdk_ntx", &Tuning::ntx},             {"pdk_xcd_map", &Tuning::xcd_map},
      {"pdk_rows", &Tuning::rows},           {"pdk_verbose", &Tuning::verbose},
      {"pdk_autotune", &Tuning::autotune},   {"pdk_pf2", &Tuning::pf2},
      {"pdk_split", &Tuning::split},         {"pdk_min_kvox", &Tuning::min_kvox},
      {"pdk_tail2", &Tuning::tail2},         {"pdk_tune_min_mvox", &Tuning::tune_min_mvox},
      {"pdk_shift", &Tuning::shift},         {"pdk_shift_min_iters", &Tuning::shift_min_iters},
  };
  if (!name) return NSOL_EINVAL;
  if (!strcmp(name, "pdk_forget")) {
    std::lock_guard<std::mutex> lock(g_plans_mutex);
    for (auto &kv : g_plans)
      for (auto &sm : kv.second.pending) {
        (void)hipEventDestroy(sm.e0);
        (void)hipEventDestroy(sm.e1);
      }
    g_plans.clear();
    return 0;
  }
  for (const auto &kn : knobs)
    if (!strcmp(name, kn.name)) {
      if (kn.field == &Tuning::shift) value = value < 0 ? -1 : (value ? 1 : 0);
      g_tunek.*kn.field = value;
      return 0;
    }
  return NSOL_EINVAL;
}

int nsol_pd_fusedk_tuned(int elem_size, int k, int64_t nz, int64_t ny, int64_t nx) {
  using namespace nsol_pdk;
  std::lock_guard<std::mutex> lock(g_plans_mutex);
  bool shifted;
  Tuned *E = reported_plan(elem_size, k, nz, ny, nx, &shifted);
  if (!E) return -1;
  plan_poll(*E, k);
  if (shifted && E->P.chosen >= 0 && tuned_size(g_tunek, nz * ny * nx)) {
    /* ... and the unshifted plan, which explores on launches the long runs give up for
     * it once the shifted plan has settled: the shape's short runs take that one */
    E = find_plan(elem_size, k, nz, ny, nx, 0, 0);
    if (!E) return 0;
    plan_poll(*E, k);
  }
  return E->P.chosen >= 0 ? 1 : 0;
}

/* 1 when a run's trailing pair of iterations should go through depth 2 of k_pd_fusedk
 * (the shape's depth-3 plan has settled and the knob is on), else 0 */
extern "C" int nsol_pd_fusedk_tail2_pitched(int elem_size, int64_t nz, int64_t ny, int64_t nx,
                                            int64_t pitch);
extern "C" int nsol_pd_fusedk_tail2(int elem_size, int64_t nz, int64_t ny, int64_t nx) {
  return nsol_pd_fusedk_tail2_pitched(elem_size, nz, ny, nx, 0);
}
extern "C" int nsol_pd_fusedk_tail2_pitched(int elem_size, int64_t nz, int64_t ny, int64_t nx,
                                            int64_t pitch) {
  using namespace nsol_pdk;
  if (!g_tunek.tail2 || !g_tunek.enable || g_tunek.kmax < 3 ||
      nz * ny * nx < ((int64_t)g_tunek.tune_min_mvox << 20))
    return 0;                       /* (measured on volumes the online tuner handles) */
  std::lock_guard<std::mutex> lock(g_plans_mutex);
  for (int form = 0; form < 2; ++form) {      /* either form's depth-3 plan */
    const Tuned *E = find_plan(elem_size, 3, nz, ny, nx, pitch > nx ? pitch : 0, form);
    if (E && E->P.chosen >= 0) return 1;
  }
  return 0;
}

int nsol_pd_fusedk_launches(int k) {
  if (k != 2 && k != 3) return -1;
  return nsol_pdk::g_launches[k - 2].load(std::memory_order_relaxed);
}

int nsol_pd_shift_launches(void) {
  return nsol_pdk::g_shift_launches.load(std::memory_order_relaxed);
}

int nsol_pd_run_parts(int iterations, int min_iters, int *lead, int *launches) {
  int l = iterations > 0 ? iterations : 0, m = 0;
  if (min_iters > 0 && iterations >= min_iters && iterations >= 4) {
    l = (iterations - 1) % 3;
    m = (iterations - 1) / 3;
  }
  if (lead) *lead = l;
  if (launches) *launches = m;
  return m > 0 ? 1 : 0;
}

int nsol_pd_shift_min_iters(int elem_size, int ndim, int64_t nz, int64_t ny, int64_t nx,
                            int flags, int64_t pitch) {
  if (flags & (NSOL_PD_REG_ISOTROPIC | NSOL_PD_DATA_WEIGHTED)) return 0;
  if (ndim != 3 || nz < 1 || ny < 1 || nx < 1) return 0;
  if (elem_size != 4 && elem_size != 8) return 0;
  return nsol_pdk::shift_min_iters(elem_size, ndim, nz, ny, nx, pitch);
}

int nsol_pd_fusedk_plan_form(int elem_size, int k, int64_t nz, int64_t ny, int64_t nx,
                             int form, int *waves, int *ntx, int64_t *zchunk) {
  using namespace nsol_pdk;
  std::lock_guard<std::mutex> lock(g_plans_mutex);
  Tuned *E = find_plan(elem_size, k, nz, ny, nx, 0, form ? 1 : 0);
  if (E) plan_poll(*E, k);
  return report_choice(E, waves, ntx, zchunk);
}

int nsol_pd_fusedk_plan(int elem_size, int k, int64_t nz, int64_t ny, int64_t nx,
                        int *waves, int *ntx, int64_t *zchunk) {
  using namespace nsol_pdk;
  std::lock_guard<std::mutex> lock(g_plans_mutex);
  bool shifted;
  return report_choice(reported_plan(elem_size, k, nz, ny, nx, &shifted), waves, ntx, zchunk);
}

int nsol_pdk_block_map(int mode, int ntx, int nty, int nzc, int *out, int max_blocks) {
  if (mode < 0 || mode > 2 || ntx < 1 || nty < 1 || nzc < 1 || !out ||
      (int64_t)ntx * nty * nzc > 0x3fffffff)
    return NSOL_EINVAL;
  const nsol::PdkBlockMap M = nsol::pdk_block_map(mode, ntx, nty, nzc);
  const long long blocks = nsol::pdk_map_blocks(M);
  if (blocks > max_blocks) return NSOL_EINVAL;
  for (int b = 0; b < (int)blocks; ++b) {
    int tile, zc;
    const bool live = nsol::pdk_block_tile(M, b, tile, zc);
    out[2 * b] = live ? tile : -1;
    out[2 * b + 1] = live ? zc : -1;
  }
  return (int)blocks;
}

int nsol_pdk_finish_probe(int64_t *out, int words) {
#ifdef NSOL_PDK_FINISH_PROBE
  if (!out || words < 0 || words > 2 * kProbeBlocks) return NSOL_EINVAL;
  if (hipDeviceSynchronize() != hipSuccess) return launch_status();
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_finish_probe), (size_t)words * 8) != hipSuccess)
    return launch_status();
  void *table = nullptr;
  if (hipGetSymbolAddress(&table, HIP_SYMBOL(g_finish_probe)) != hipSuccess ||
      hipMemset(table, 0, sizeof(unsigned long long) * 2 * kProbeBlocks) != hipSuccess)
    return launch_status();
  return 0;
#else
  (void)out; (void)words;
  return -2;      /* the library was built without the probe */
#endif
}

#define NSOL_PDK_DEF(T, SUF)                                                           \
  int nsol_pd_fusedk_iter_pitched_##SUF(                                               \
      const T *xbar_in, T *xbar_out, const T *x_in, T *x_out, const T *bt, const T *p_in, \
      T *p_out, int ndim, int64_t nz, int64_t ny, int64_t nx, int64_t pitch, double wx, \
      double wy, double wz, int k, const double *sigma, const double *hden,            \
      const double *tau, const double *tl, const double *theta, int flags,             \
      void *stream) {                                                                  \
    return pd_fusedk_iter<T>(xbar_in, xbar_out, x_in, x_out, bt, p_in, p_out, ndim,    \
                             nz, ny, nx, wx, wy, wz, k, sigma, hden, tau, tl, theta,   \
                             flags, stream, pitch);                                    \
  }                                                                                    \
  int nsol_pd_fusedk_iter_##SUF(                                                       \
      const T *xbar_in, T *xbar_out, const T *x_in, T *x_out, const T *bt, const T *p_in, \
      T *p_out, int ndim, int64_t nz, int64_t ny, int64_t nx, double wx, double wy,    \
      double wz, int k, const double *sigma, const double *hden, const double *tau,    \
      const double *tl, const double *theta, int flags, void *stream) {                \
    return pd_fusedk_iter<T>(xbar_in, xbar_out, x_in, x_out, bt, p_in, p_out, ndim,    \
                             nz, ny, nx, wx, wy, wz, k, sigma, hden, tau, tl, theta,   \
                             flags, stream, 0);                                        \
  }
NSOL_PDK_DEF(float, f32)
NSOL_PDK_DEF(double, f64)
#undef NSOL_PDK_DEF

}  // extern "C"
