// The per-tile work of the single-pass primal-dual iteration with the ISOTROPIC
// dual projection p = q / max(1, |q|_2), |q|_2 the Euclidean norm of the voxel's
// stacked gradient vector (admm_linear_solver.py:239-253 shrinks the same vector;
// prior_measures.py:27-52 measures it), used by k_pd_fused_iso (nsol_pdi.hip).
//
// The patch / march layout is pd_fused_tile's (nsol_pd_fused_body.hpp).  What
// differs is the lower halo: the new dual value at a neighbour voxel i - e_a is a
// component of that voxel's PROJECTED vector, so the lane that needs it forms the
// neighbour's whole q -- all its forward differences and all its old dual
// components -- and projects it.  These are loads of lines that the neighbouring
// wave streams anyway (L1 / L2 hits); nothing is exchanged between waves, so the
// march along z has no barrier and no inter-workgroup dependency.
#pragma once

#include "nsol_common.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_weighted.hpp"
#include "nsol_pd_fused_body.hpp"

namespace nsol {

// q = p_old + sigma * (hi*w + lo*(-w)): dual_update's argument, same order
template <typename T>
__device__ __forceinline__ T dual_q(T p_old, T hi, T lo, T w, T sigma) {
  return p_old + sigma * (hi * w + lo * (-w));
}

// (q0, q1, q2) -> q / max(1, sqrt(((q0*q0) + q1*q1) + q2*q2)), after the Huber
// division of every component; IEEE square root and division.  In 1-D
// sqrt(q*q) = |q| exactly, which makes this dual_clamp bit for bit.
template <int NDIM, typename T>
__device__ __forceinline__ void dual_project(T &q0, T &q1, T &q2, bool huber, T hden) {
  if (huber) {
    pin(q0);           // a real (uniform) branch, as in dual_update
    q0 = huber_div(q0, hden);
    if constexpr (NDIM >= 2) q1 = huber_div(q1, hden);
    if constexpr (NDIM >= 3) q2 = huber_div(q2, hden);
  }
  T s = q0 * q0;
  if constexpr (NDIM >= 2) s = s + q1 * q1;
  if constexpr (NDIM >= 3) s = s + q2 * q2;
  const T m = t_max(T(1), t_sqrt(s));
  q0 = q0 / m;
  if constexpr (NDIM >= 2) q1 = q1 / m;
  if constexpr (NDIM >= 3) q2 = q2 / m;
}

// One iteration on tile (tx, ty), z-chunk zc of one volume; arguments as
// pd_fused_tile (WGT / wt, CHK / chk and LIN / lo, hi included).
template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG, bool WGT = false,
          bool CHK = false, bool LIN = false>
__device__ __forceinline__ void pd_fused_iso_tile(
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
  const bool huber = S.huber != 0;

  const bool left_edge = (lx == 0);
  const bool right_edge = (lx == LX - 1);
  const bool top_edge = (ly == 0);
  const bool bottom_edge = (ly == LY - 1);
  const bool has_left = xin && left_edge && x0 > 0;
  const bool has_right = right_edge && (x0 + VEC < G.nx);
  const bool has_up = xin && top_edge && y0 > 0 && y0 - 1 < G.ny;
  const bool has_down = xin && bottom_edge && (y0 + RY < G.ny);

  // The projected dual vector of the lane's own voxels on the plane at offset o0
  // (its xbar in xa, the next plane's -- zeros behind the volume -- in xb).
  // CHK and `count`: the old and new dual values of the voxels this plane stores go
  // into the sums of the stopping rule (not the plane before a z chunk).
  auto dual_own = [&](int64_t o0, const T (&xa)[RY][VEC], const T (&xb)[RY][VEC],
                      T (&px)[RY][VEC], T (&py)[RY][VEC], T (&pz)[RY][VEC],
                      bool count) __attribute__((always_inline)) {
    T xdown[VEC];
    zero(xdown);
    if constexpr (NDIM >= 2) {
      if (has_down) ld(xbar_in + o0 + RY * G.sy, xdown);
    }
    T below[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if constexpr (NDIM >= 2 && LY > 1) below[k] = __shfl_down(xa[0][k], LX, kWave);
      else below[k] = T(0);
      if (bottom_edge) below[k] = xdown[k];
    }
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      zero(px[r]); zero(py[r]); zero(pz[r]);
      const int64_t o = o0 + r * G.sy;
      if (rin[r] && S.has_p) {
        ld(pin_x + o, px[r]);
        if constexpr (NDIM >= 2) ld(pin_y + o, py[r]);
        if constexpr (NDIM >= 3) ld(pin_z + o, pz[r]);
      }
      T xright = T(0);
      if (has_right && (y0 + r < G.ny)) xright = xbar_in[o + VEC];
      // x-neighbour to the right: next lane's first element
      T nb = __shfl_down(xa[r][0], 1, kWave);
      if (right_edge) nb = xright;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const T c = xa[r][k];
        const T hx = (k + 1 < VEC) ? xa[r][(k + 1) % VEC] : nb;
        T q0 = dual_q(px[r][k], hx, c, G.wx, S.sigma), q1 = T(0), q2 = T(0);
        if constexpr (NDIM >= 2) {
          const T hy = (r + 1 < RY) ? xa[(r + 1) % RY][k] : below[k];
          q1 = dual_q(py[r][k], hy, c, G.wy, S.sigma);
        }
        if constexpr (NDIM >= 3) q2 = dual_q(pz[r][k], xb[r][k], c, G.wz, S.sigma);
        dual_project<NDIM>(q0, q1, q2, huber, S.hden);
        if constexpr (CHK) {
          if (count && rin[r] && k < nval) {
            chk_add(chk[2], chk[3], px[r][k], q0);
            if constexpr (NDIM >= 2) chk_add(chk[2], chk[3], py[r][k], q1);
            if constexpr (NDIM >= 3) chk_add(chk[2], chk[3], pz[r][k], q2);
          }
        }
        px[r][k] = q0; py[r][k] = q1; pz[r][k] = q2;
      }
    }
  };

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
      // the plane before the chunk: its whole projection, of which p_z is kept
      T xm[RY][VEC], tx_[RY][VEC], ty_[RY][VEC];
#pragma unroll
      for (int r = 0; r < RY; ++r) {
        zero(xm[r]);
        if (rin[r]) ld(xbar_in + off - G.sz + r * G.sy, xm[r]);
      }
      dual_own(off - G.sz, xm, xc, tx_, ty_, pzprev, false);
    }
  }

  for (int64_t z = zbeg; z < zend; ++z, off += G.sz) {
    T xn[RY][VEC], xv[RY][VEC], bv[RY][VEC];
    T wv[RY][VEC];      // WGT: the weights of the data term (zero outside the row)
    const bool znext = (NDIM >= 3) && (z + 1 < G.nz);
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      zero(xn[r]); zero(xv[r]); zero(bv[r]);
      if constexpr (WGT) zero(wv[r]);
      if (rin[r]) {
        const int64_t o = off + r * G.sy;
        if (znext) ld(xbar_in + o + G.sz, xn[r]);
        ld(x + o, xv[r]);
        ld(bt + o, bv[r]);
        if constexpr (WGT) ld(wt + o, wv[r]);
      }
    }

    // ---------------- dual update at the lane's own voxels ----------------
    T pxn[RY][VEC], pyn[RY][VEC], pzn[RY][VEC];
    dual_own(off, xc, xn, pxn, pyn, pzn, true);

    // ---------------- new dual values on the lower halo -------------------
    // left of the wave patch: voxel (x0-1, y0+r, z), its x-difference against the
    // lane's own first element, its y / z differences and old dual from memory
    T pxl[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      pxl[r] = __shfl_up(pxn[r][VEC - 1], 1, kWave);
      if (left_edge) {
        T q0 = T(0);
        if (has_left && rin[r]) {
          const int64_t o = off + r * G.sy - 1;
          const T c = xbar_in[o];
          T q1 = T(0), q2 = T(0), o0 = T(0), o1 = T(0), o2 = T(0);
          if (S.has_p) {
            o0 = pin_x[o];
            if constexpr (NDIM >= 2) o1 = pin_y[o];
            if constexpr (NDIM >= 3) o2 = pin_z[o];
          }
          q0 = dual_q(o0, xc[r][0], c, G.wx, S.sigma);
          if constexpr (NDIM >= 2) {
            const T hy = (y0 + r + 1 < G.ny) ? xbar_in[o + G.sy] : T(0);
            q1 = dual_q(o1, hy, c, G.wy, S.sigma);
          }
          if constexpr (NDIM >= 3) {
            const T hz = znext ? xbar_in[o + G.sz] : T(0);
            q2 = dual_q(o2, hz, c, G.wz, S.sigma);
          }
          dual_project<NDIM>(q0, q1, q2, huber, S.hden);
        }
        pxl[r] = q0;
      }
    }
    // above the wave patch: row y0-1, its y-difference against the lane's own
    // first row, the rest from memory
    T pyu[VEC];
    if constexpr (NDIM >= 2) {
      T cu[VEC], zu[VEC], ox[VEC], oy[VEC], oz[VEC];
      zero(cu); zero(zu); zero(ox); zero(oy); zero(oz);
      T ru = T(0);
      if (has_up) {
        const int64_t o = off - G.sy;
        ld(xbar_in + o, cu);
        if (x0 + VEC < G.nx) ru = xbar_in[o + VEC];
        if (znext) ld(xbar_in + o + G.sz, zu);
        if (S.has_p) {
          ld(pin_x + o, ox);
          ld(pin_y + o, oy);
          if constexpr (NDIM >= 3) ld(pin_z + o, oz);
        }
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if constexpr (LY > 1) pyu[k] = __shfl_up(pyn[RY - 1][k], LX, kWave);
        else pyu[k] = T(0);
        if (top_edge) {
          T q1 = T(0);
          if (has_up) {
            const T hx = (k + 1 < VEC) ? cu[(k + 1) % VEC] : ru;
            T q0 = dual_q(ox[k], hx, cu[k], G.wx, S.sigma), q2 = T(0);
            q1 = dual_q(oy[k], xc[0][k], cu[k], G.wy, S.sigma);
            if constexpr (NDIM >= 3) q2 = dual_q(oz[k], zu[k], cu[k], G.wz, S.sigma);
            dual_project<NDIM>(q0, q1, q2, huber, S.hden);
          }
          pyu[k] = q1;
        }
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
            if (k < nval) chk_add(chk[0], chk[1], xv[r][k], xo_new[k]);
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
