// The per-tile work of the single-pass primal-dual iteration, shared by
// k_pd_fused (nsol_pd.hip: one volume per launch) and k_pd_sweep (nsol_pds.hip:
// the members of a parameter sweep stacked in one launch), so that the two
// produce the same bits by construction.
#pragma once

#include "nsol_common.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_lin_step.hpp"
#include "nsol_pd_weighted.hpp"

namespace nsol {

// Block -> tile map.  Workgroups are dealt round-robin to the 8 XCDs
// (bid % 8 names the group that shares an L2), so with slab > 0 each
// XCD walks its own slab of `slab` consecutive y-tiles: the halo rows and
// columns that neighbouring tiles re-read are then served by that XCD's L2.
// Placement only affects speed, never results.  False: no tile for this block.
__device__ __forceinline__ bool pd_fused_block_tile(int bid, int ntx, int nty, int slab,
                                                    int &tx, int &ty, int &zc) {
  if (slab > 0) {
    const int xcd = bid & 7;
    int j = bid >> 3;
    tx = j % ntx;
    j /= ntx;
    ty = xcd * slab + j % slab;
    zc = j / slab;
    if (ty >= nty) return false;
  } else {
    tx = bid % ntx;
    bid /= ntx;
    ty = bid % nty;
    zc = bid / nty;
  }
  return true;
}

// One iteration on tile (tx, ty), z-chunk zc of one volume: each wave owns a
// (LX*VEC) x (LY*RY) patch of the x-y tile and marches along z (see nsol_pd.hip).
// RAG: rows that are not a multiple of VEC elements / arrays that are not 16-byte
// aligned.  WGT: the data term carries per-voxel weights wt (nsol_pd_weighted.hpp),
// one more row load per plane and prox_data_w in place of prox_data (k_pd_w,
// nsol_pdw.hip); the unweighted kernels leave it off and are compiled as before.
// CHK: the lane adds the four float64 sums of the stopping rule (chk_add,
// nsol_pd_common.hpp) over the voxels it STORES -- not the elements behind a ragged
// row's end, not the rows outside the volume, not the dual values it recomputes on
// the lower halo -- to chk[0..3] (k_pd_check, nsol_pdc.hip); off by default, and the
// other kernels are compiled as before.
// LIN: the array in bt's place holds g = A^T q and the data prox is lin_step with the
// box [lo, hi] (k_pd_lin, nsol_pdl.hip); off by default, the other kernels are
// compiled as before.
template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG, bool WGT = false,
          bool CHK = false, bool LIN = false>
__device__ __forceinline__ void pd_fused_tile(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ p_in, T *__restrict__ p_out,
    const Geom<T> &G, const PdScalars<T> &S, int tx, int ty, int zc, int zchunk,
    const T *__restrict__ wt = nullptr, double *chk = nullptr, T lo = T(0),
    T hi = T(0)) {
  constexpr int LY = kWave / LX;
  constexpr int WAVES = kBlock / kWave;
  constexpr int TY = WAVES * LY * RY;

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int lx = lane % LX;
  const int ly = lane / LX;

  const int64_t x0 = ((int64_t)tx * LX + lx) * VEC;
  const int64_t y0 = (int64_t)ty * TY + (int64_t)(wave * LY + ly) * RY;
  const bool xin = x0 < G.nx;
  // valid elements of this lane's vector (RAG: the row may end inside it)
  const int nval = !RAG ? VEC : (G.nx - x0 >= VEC ? VEC : (int)(xin ? G.nx - x0 : 0));
  auto ld = [&](const T *q, T (&v)[VEC]) {
    if constexpr (RAG) ldv_rag<T, VEC>(q, v, nval);
    else ldv<T, VEC>(q, v);
  };
  auto st = [&](T *q, const T (&v)[VEC]) {
    if constexpr (RAG) stv_rag<T, VEC>(q, v, nval);
    else stv<T, VEC>(q, v);
  };
  bool rin[RY];
#pragma unroll
  for (int r = 0; r < RY; ++r) rin[r] = xin && (y0 + r < G.ny);

  const int64_t zbeg = (int64_t)zc * zchunk;
  int64_t zend = zbeg + zchunk;
  if (zend > G.nz) zend = G.nz;

  const T *pin_x = p_in;
  const T *pin_y = p_in + G.n;
  const T *pin_z = p_in + 2 * G.n;
  T *pout_x = p_out;
  T *pout_y = p_out + G.n;
  T *pout_z = p_out + 2 * G.n;

  // edge roles of this lane inside its wave patch
  const bool left_edge = (lx == 0);
  const bool right_edge = (lx == LX - 1);
  const bool top_edge = (ly == 0);
  const bool bottom_edge = (ly == LY - 1);
  const bool has_left = xin && left_edge && x0 > 0;
  const bool has_right = right_edge && (x0 + VEC < G.nx);
  const bool has_up = xin && top_edge && y0 > 0 && y0 - 1 < G.ny;
  const bool has_down = xin && bottom_edge && (y0 + RY < G.ny);

  T xc[RY][VEC];      // xbar[z]
  T pzprev[RY][VEC];  // new p_z at z-1

  int64_t off = zbeg * G.sz + y0 * G.sy + x0;  // (zbeg, y0, x0)
#pragma unroll
  for (int r = 0; r < RY; ++r) {
    zero(xc[r]);
    zero(pzprev[r]);
    if (rin[r]) ld(xbar_in + off + r * G.sy, xc[r]);
  }
  if constexpr (NDIM >= 3) {
    if (zbeg > 0) {
#pragma unroll
      for (int r = 0; r < RY; ++r) {
        if (rin[r]) {
          T xm[VEC], pm[VEC];
          zero(pm);
          ld(xbar_in + off - G.sz + r * G.sy, xm);
          if (S.has_p) ld(pin_z + off - G.sz + r * G.sy, pm);
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            pzprev[r][k] = dual_update(pm[k], xc[r][k], xm[k], G.wz, S);
        }
      }
    }
  }

  for (int64_t z = zbeg; z < zend; ++z, off += G.sz) {
    // ---------------- loads of plane z (and xbar of plane z+1) ------------
    T xn[RY][VEC], xv[RY][VEC], bv[RY][VEC];
    T wv[RY][VEC];      // WGT: the weights of the data term (zero outside the row)
    T pxo[RY][VEC], pyo[RY][VEC], pzo[RY][VEC];
    const bool znext = (NDIM >= 3) && (z + 1 < G.nz);
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      zero(xn[r]); zero(xv[r]); zero(bv[r]);
      if constexpr (WGT) zero(wv[r]);
      zero(pxo[r]); zero(pyo[r]); zero(pzo[r]);
      if (rin[r]) {
        const int64_t o = off + r * G.sy;
        if (znext) ld(xbar_in + o + G.sz, xn[r]);
        ld(x + o, xv[r]);
        ld(bt + o, bv[r]);
        if constexpr (WGT) ld(wt + o, wv[r]);
        if (S.has_p) {
          ld(pin_x + o, pxo[r]);
          if constexpr (NDIM >= 2) ld(pin_y + o, pyo[r]);
          if constexpr (NDIM >= 3) ld(pin_z + o, pzo[r]);
        }
      }
    }
    // halo: column to the right / left of the wave patch
    T xright[RY], xleft[RY], pxleft[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      xright[r] = T(0); xleft[r] = T(0); pxleft[r] = T(0);
      const int64_t o = off + r * G.sy;
      if (has_right && (y0 + r < G.ny)) xright[r] = xbar_in[o + VEC];
      if (has_left && rin[r]) {
        xleft[r] = xbar_in[o - 1];
        if (S.has_p) pxleft[r] = pin_x[o - 1];
      }
    }
    // halo: row above / below the wave patch
    T xdown[VEC], xup[VEC], pyup[VEC];
    zero(xdown); zero(xup); zero(pyup);
    if constexpr (NDIM >= 2) {
      if (has_down) ld(xbar_in + off + RY * G.sy, xdown);
      if (has_up) {
        ld(xbar_in + off - G.sy, xup);
        if (S.has_p) ld(pin_y + off - G.sy, pyup);
      }
    }

    // ---------------- dual update at the lane's own voxels ----------------
    T pxn[RY][VEC], pyn[RY][VEC], pzn[RY][VEC];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      // x-neighbour to the right: next lane's first element
      T nb = __shfl_down(xc[r][0], 1, kWave);
      if (right_edge) nb = xright[r];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const T hi = (k + 1 < VEC) ? xc[r][k + 1] : nb;
        pxn[r][k] = dual_update(pxo[r][k], hi, xc[r][k], G.wx, S);
      }
    }
    if constexpr (NDIM >= 2) {
      T below[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if constexpr (LY > 1) below[k] = __shfl_down(xc[0][k], LX, kWave);
        else below[k] = T(0);
        if (bottom_edge) below[k] = xdown[k];
      }
#pragma unroll
      for (int r = 0; r < RY; ++r)
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const T hi = (r + 1 < RY) ? xc[(r + 1) % RY][k] : below[k];
          pyn[r][k] = dual_update(pyo[r][k], hi, xc[r][k], G.wy, S);
        }
    }
    if constexpr (NDIM >= 3) {
#pragma unroll
      for (int r = 0; r < RY; ++r)
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          pzn[r][k] = dual_update(pzo[r][k], xn[r][k], xc[r][k], G.wz, S);
    }

    // ---------------- new dual values on the lower halo -------------------
    T pxl[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      pxl[r] = __shfl_up(pxn[r][VEC - 1], 1, kWave);
      if (left_edge)
        pxl[r] = has_left ? dual_update(pxleft[r], xc[r][0], xleft[r], G.wx, S)
                          : T(0);
    }
    T pyu[VEC];
    if constexpr (NDIM >= 2) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if constexpr (LY > 1) pyu[k] = __shfl_up(pyn[RY - 1][k], LX, kWave);
        else pyu[k] = T(0);
        if (top_edge)
          pyu[k] = has_up ? dual_update(pyup[k], xc[0][k], xup[k], G.wy, S)
                          : T(0);
      }
    }

    // ---------------- primal update + stores ------------------------------
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      T xo_new[VEC], xb_new[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const T pl = (k > 0) ? pxn[r][(k + VEC - 1) % VEC] : pxl[r];
        T kt = pxn[r][k] * (-G.wx) + pl * G.wx;
        if constexpr (NDIM >= 2) {
          const T pu = (r > 0) ? pyn[(r + RY - 1) % RY][k] : pyu[k];
          kt += pyn[r][k] * (-G.wy) + pu * G.wy;
        }
        if constexpr (NDIM >= 3)
          kt += pzn[r][k] * (-G.wz) + pzprev[r][k] * G.wz;
        const T u = xv[r][k] - S.tau * kt;
        T xnew;
        if constexpr (LIN) xnew = lin_step(xv[r][k], kt, bv[r][k], S.tau, lo, hi);
        else if constexpr (WGT)
          xnew = prox_data_w(u, bv[r][k], wv[r][k], S.tl, S.l1 != 0);
        else xnew = prox_data(u, bv[r][k], S.tl, S.one_plus_tl, S.l1 != 0);
        xo_new[k] = xnew;
        xb_new[k] = xnew + S.theta * (xnew - xv[r][k]);
      }
      if (rin[r]) {
        const int64_t o = off + r * G.sy;
        st(pout_x + o, pxn[r]);
        if constexpr (NDIM >= 2) st(pout_y + o, pyn[r]);
        if constexpr (NDIM >= 3) st(pout_z + o, pzn[r]);
        st(x + o, xo_new);
        st(xbar_out + o, xb_new);
        if constexpr (CHK) {
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            if (k < nval) {
              chk_add(chk[0], chk[1], xv[r][k], xo_new[k]);
              chk_add(chk[2], chk[3], pxo[r][k], pxn[r][k]);
              if constexpr (NDIM >= 2) chk_add(chk[2], chk[3], pyo[r][k], pyn[r][k]);
              if constexpr (NDIM >= 3) chk_add(chk[2], chk[3], pzo[r][k], pzn[r][k]);
            }
        }
      }
      if constexpr (NDIM >= 3) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          pzprev[r][k] = pzn[r][k];
          xc[r][k] = xn[r][k];
        }
      }
    }
  }
}

}  // namespace nsol
