// Second-order total generalised variation (TGV^2, Bredies / Kunisch / Pock) for gfx950
// (MI355X): the two kernels of one Chambolle-Pock iteration on
//
//   min over x (n values), w (d n values)   lambda D(x, b~) + |grad x - w|_1 + beta |E w|_1
//
// with grad the zero-padded forward difference of k_grad (component a = 0 is the x axis),
// D_a^T its exact transpose (grad_adj_vec) and E w the symmetrised gradient of w,
// (E w)_aa = D_a w_a, (E w)_ab = 1/2 (D_a w_b + D_b w_a), stored diagonals first (3-D: xx,
// yy, zz, xy, xz, yz; 2-D: xx, yy, xy; 1-D: xx).  Off-diagonals count twice in every norm.
//
//   k_tgv_dual    p_a  <- P_1   (p_a  + sigma (D_a xbar - wbar_a))
//                 q_ab <- P_beta(q_ab + sigma (E wbar)_ab)
//                 reads xbar, wbar and their forward neighbours, p and q at their own
//                 index; writes p and q in place.
//   k_tgv_primal  x+   = prox_{tau lambda D}(x - tau sum_a D_a^T p_a)
//                 w_a+ = w_a - tau (-p_a + D_a^T q_aa + sum_{b != a} D_b^T q_ab)
//                 xbar = x+ + theta (x+ - x), wbar likewise
//                 reads p, q and their backward neighbours, x, w, b~ at their own index;
//                 writes x, w, xbar, wbar in place.
//   k_tgv_primal_w, k_tgv_primal_lin: the same body with the weighted prox (one more
//                 read-only stream wt) or, for a data term behind a linear operator A, the
//                 explicit clipped step on g = A^T r in b~'s place (TgvForm below).
//   k_tgv_primal_kl: the same body with the prox of the Poisson (Kullback-Leibler) data
//                 term, prox_kl of nsol_kl.hpp; wt may be null.
//   k_tgv_dual_stack, k_tgv_primal_stack, k_tgv_primal_w_stack, k_tgv_primal_lin_stack:
//                 the same device functions
//                 on member blockIdx.z of a stack of independent problems of one shape (a
//                 stack of images, an (alpha, beta) sweep): the member's arrays at
//                 member-major 64-bit offsets, its beta, tl and prox denominator from a
//                 device table (TgvMember; the kLin form reads none: its step takes tau,
//                 theta and the box only).  The thread mapping uses blockIdx.x and
//                 blockIdx.y only, so blockIdx.z adds a constant to a member's linear
//                 workgroup ids and the slab grouping of voxel_at is kept within a member.
//
// No array is read at a neighbour and written in the same launch: no ping-pong buffers,
// no dependency between workgroups.  The thread mapping is nsol_stencil.hpp's (k_grad /
// k_grad_adj); 3-D traffic is 22 + 22 words per voxel and iteration, 2-D 13 + 15.
//
// w, p and q are d or M components stacked at stride n.  Voxel::wide is computed against
// ONE n-element array (c.i + forward offset + VEC <= n), so a whole-vector read that it
// allows at component k ends at k n + n at the latest: inside the stack for every
// component, the last one included.
#include <math.h>

#include <atomic>
#include <type_traits>

#include "nsol_common.hpp"
#include "nsol_kl.hpp"
#include "nsol_pd_iso_body.hpp"
#include "nsol_pd_launch.hpp"
#include "nsol_pd_lin_step.hpp"
#include "nsol_pd_weighted.hpp"
#include "nsol_stencil.hpp"

using namespace nsol;

namespace {

std::atomic<int> g_tgv_launches{0};
std::atomic<int> g_tgv_stack_launches{0};   // the member-stacked kernels'

// stored component of the off-diagonal (a, b), a < b
template <int NDIM>
__device__ __forceinline__ constexpr int sym_off(int a, int b) {
  return NDIM == 2 ? 2 : (a == 0 ? 2 + b : 5);
}

// D_a u at the lane's voxels; `own` holds u there (u: one component's base)
template <bool RAG, typename T, int VEC>
__device__ __forceinline__ void fwd_dir(int a, const T *__restrict__ u, const T (&own)[VEC],
                                        const Geom<T> &G, const Voxel &c, T (&g)[VEC]) {
  if (a == 0) {
    const T right = (c.ix + VEC < G.nx) ? u[c.i + VEC] : T(0);
    fwd_diff_x<T, VEC>(own, right, G.wx, g);
  } else {
    T hi[VEC];
    vzero(hi);
    if (a == 1) {
      if (c.iy + 1 < G.ny) vlc<RAG, T, VEC>(c, u + c.i + G.sy, hi);
    } else {
      if (c.iz + 1 < G.nz) vlc<RAG, T, VEC>(c, u + c.i + G.sz, hi);
    }
    fwd_diff<T, VEC>(own, hi, a == 1 ? G.wy : G.wz, g);
  }
}

// D_a^T u at the lane's voxels, u[i] * (-w_a) + u[i - e_a] * w_a as grad_adj_vec forms
// it; `own` receives u there
template <bool RAG, typename T, int VEC>
__device__ __forceinline__ void adj_dir(int a, const T *__restrict__ u, const Geom<T> &G,
                                        const Voxel &c, T (&own)[VEC], T (&out)[VEC]) {
  vlc<RAG, T, VEC>(c, u + c.i, own);
  if (a == 0) {
    const T left = (c.ix > 0) ? u[c.i - 1] : T(0);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const T l = (k > 0) ? own[(k + VEC - 1) % VEC] : left;
      out[k] = own[k] * (-G.wx) + l * G.wx;
    }
  } else {
    T lo[VEC];
    vzero(lo);
    if (a == 1) {
      if (c.iy > 0) vlc<RAG, T, VEC>(c, u + c.i - G.sy, lo);
    } else {
      if (c.iz > 0) vlc<RAG, T, VEC>(c, u + c.i - G.sz, lo);
    }
    const T w = a == 1 ? G.wy : G.wz;
#pragma unroll
    for (int k = 0; k < VEC; ++k) out[k] = own[k] * (-w) + lo[k] * w;
  }
}

template <typename T>
__device__ __forceinline__ T clamp_beta(T v, T beta) {
  v = v < -beta ? -beta : v;
  return v > beta ? beta : v;
}

// One member's dual step.  The single kernel passes its arguments on as they are; the
// stacked one passes member blockIdx.z's arrays and its beta (k_tgv_dual_stack below).
template <typename T, int VEC, int ROWS, int NDIM, bool RAG, bool ISO>
__device__ __forceinline__ void tgv_dual_body(const T *__restrict__ xbar,
                                              const T *__restrict__ wbar, T *p, T *q,
                                              const Geom<T> &G, T sigma, T beta) {
  constexpr int M = NDIM * (NDIM + 1) / 2;
  const int64_t nrg = row_groups<T, VEC, ROWS>(G);
  for (int64_t rg = blockIdx.y; rg < nrg; rg += gridDim.y) {
    const Voxel c = voxel_at<T, VEC, ROWS>(G, rg);
    if (!c.ok) continue;
    T xb[VEC], wb[NDIM][VEC], pn[NDIM][VEC], e[M][VEC], g[VEC];
    vlc<RAG, T, VEC>(c, xbar + c.i, xb);
#pragma unroll
    for (int b = 0; b < NDIM; ++b) vlc<RAG, T, VEC>(c, wbar + b * G.n + c.i, wb[b]);
    // one direction a at a time: D_a xbar into p_a, the d shifted vectors of wbar into
    // q_aa and the q_ab they feed
#pragma unroll
    for (int a = 0; a < NDIM; ++a) {
      fwd_dir<RAG, T, VEC>(a, xbar, xb, G, c, g);
      vlc<RAG, T, VEC>(c, p + a * G.n + c.i, pn[a]);
#pragma unroll
      for (int k = 0; k < VEC; ++k) pn[a][k] = pn[a][k] + sigma * (g[k] - wb[a][k]);
#pragma unroll
      for (int b = 0; b < NDIM; ++b) {
        fwd_dir<RAG, T, VEC>(a, wbar + b * G.n, wb[b], G, c, g);
        if (b == a) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) e[a][k] = g[k];
        } else if (a < b) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) e[sym_off<NDIM>(a, b)][k] = g[k];   // D_a w_b
        } else {
          const int m = sym_off<NDIM>(b, a);
#pragma unroll
          for (int k = 0; k < VEC; ++k) e[m][k] = T(0.5) * (e[m][k] + g[k]);  // + D_a w_b
        }
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if constexpr (ISO) {
        T q0 = pn[0][k], q1 = T(0), q2 = T(0);
        if constexpr (NDIM >= 2) q1 = pn[1][k];
        if constexpr (NDIM >= 3) q2 = pn[2][k];
        dual_project<NDIM>(q0, q1, q2, false, T(1));
        pn[0][k] = q0;
        if constexpr (NDIM >= 2) pn[1][k] = q1;
        if constexpr (NDIM >= 3) pn[2][k] = q2;
      } else {
#pragma unroll
        for (int a = 0; a < NDIM; ++a) pn[a][k] = dual_clamp<T>(pn[a][k]);
      }
    }
#pragma unroll
    for (int a = 0; a < NDIM; ++a) vs<RAG, T, VEC>(c.nval, p + a * G.n + c.i, pn[a]);

    // q <- P_beta(q + sigma E wbar), into e
#pragma unroll
    for (int m = 0; m < M; ++m) {
      vlc<RAG, T, VEC>(c, q + m * G.n + c.i, g);
#pragma unroll
      for (int k = 0; k < VEC; ++k) e[m][k] = g[k] + sigma * e[m][k];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if constexpr (ISO) {
        // Frobenius norm with the off-diagonals doubled; q / max(1, |q|_F / beta)
        T s = e[0][k] * e[0][k];
#pragma unroll
        for (int m = 1; m < NDIM; ++m) s = s + e[m][k] * e[m][k];
#pragma unroll
        for (int m = NDIM; m < M; ++m) s = s + T(2) * (e[m][k] * e[m][k]);
        const T den = t_max(T(1), t_sqrt(s) / beta);
#pragma unroll
        for (int m = 0; m < M; ++m) e[m][k] = e[m][k] / den;
      } else {
#pragma unroll
        for (int m = 0; m < M; ++m) e[m][k] = clamp_beta<T>(e[m][k], beta);
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) vs<RAG, T, VEC>(c.nval, q + m * G.n + c.i, e[m]);
  }
}

template <typename T, int VEC, int ROWS, int NDIM, bool RAG, bool ISO>
__global__ __launch_bounds__(kBlock) void k_tgv_dual(const T *__restrict__ xbar,
                                                      const T *__restrict__ wbar, T *p,
                                                      T *q, Geom<T> G, T sigma, T beta) {
  tgv_dual_body<T, VEC, ROWS, NDIM, RAG, ISO>(xbar, wbar, p, q, G, sigma, beta);
}

// What differs from member to member of a stack, in the kernels' type: beta (dual
// kernel), tl = tau / alpha and prox_den<T>(tl) (primal kernels).  4 values of T per
// member; nsol_tgv_stack_table_* fills the table.
template <typename T>
struct TgvMember {
  T beta, tl, den, pad;
};

// k_tgv_dual on member m = blockIdx.z of a stack: xbar at m n, wbar and p at m d n, q
// at m M n (64-bit offsets), beta from the table.  Components stay at stride n inside a
// member, so Voxel::wide -- computed against one n-element array -- holds for every
// member as it does for one.
template <typename T, int VEC, int ROWS, int NDIM, bool RAG, bool ISO>
__global__ __launch_bounds__(kBlock) void k_tgv_dual_stack(
    const T *__restrict__ xbar, const T *__restrict__ wbar, T *p, T *q, Geom<T> G, T sigma,
    const TgvMember<T> *__restrict__ tab) {
  constexpr int M = NDIM * (NDIM + 1) / 2;
  const int64_t m = blockIdx.z;
  tgv_dual_body<T, VEC, ROWS, NDIM, RAG, ISO>(xbar + m * G.n, wbar + m * NDIM * G.n,
                                              p + m * NDIM * G.n, q + m * M * G.n, G, sigma,
                                              tab[m].beta);
}

// The x step of k_tgv_primal comes in three forms that share everything else:
//   kPlain  prox_data(u, b~): the denoising prox, all weights 1
//   kWgt    prox_data_w(u, b~, wt) of nsol_pd_weighted.hpp: per-voxel weights, one more
//           read-only stream (23 words per voxel in 3-D); wt == 0 keeps u
//   kLin    lin_step(x, sum_a D_a^T p_a, g) of nsol_pd_lin_step.hpp: the array in b~'s
//           place holds g = A^T r and the step is explicit, clipped to [lo, hi] (22 words)
//   kKl     prox_kl(u, b~, wt) of nsol_kl.hpp: the Poisson (Kullback-Leibler) data term;
//           wt may be null (all weights 1), a uniform branch on the pointer
enum TgvForm { kPlain = 0, kWgt = 1, kLin = 2, kKl = 3 };

template <typename T, int VEC, int ROWS, int NDIM, bool RAG, bool L1, int FORM>
__device__ __forceinline__ void tgv_primal_body(
    const T *__restrict__ p, const T *__restrict__ q, T *x, T *xbar, T *w, T *wbar,
    const T *__restrict__ bt, const T *__restrict__ wt, const Geom<T> &G, T tau, T tl,
    T den, T theta, T lo, T hi) {
  const int64_t nrg = row_groups<T, VEC, ROWS>(G);
  for (int64_t rg = blockIdx.y; rg < nrg; rg += gridDim.y) {
    const Voxel c = voxel_at<T, VEC, ROWS>(G, rg);
    if (!c.ok) continue;
    T pw[NDIM][VEC], acc[VEC], t[VEC], own[VEC], v[VEC], o[VEC];
    // x+ = prox(x - tau sum_a D_a^T p_a); the own p_a are kept for w
    adj_dir<RAG, T, VEC>(0, p, G, c, pw[0], acc);
#pragma unroll
    for (int a = 1; a < NDIM; ++a) {
      adj_dir<RAG, T, VEC>(a, p + a * G.n, G, c, pw[a], t);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] += t[k];
    }
    vlc<RAG, T, VEC>(c, x + c.i, v);
    vlc<RAG, T, VEC>(c, bt + c.i, t);
    if constexpr (FORM == kWgt) vlc<RAG, T, VEC>(c, wt + c.i, own);
    if constexpr (FORM == kKl) {
      if (wt) {
        vlc<RAG, T, VEC>(c, wt + c.i, own);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) own[k] = T(1);
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      T xn;
      if constexpr (FORM == kLin)
        xn = lin_step<T>(v[k], acc[k], t[k], tau, lo, hi);
      else if constexpr (FORM == kWgt)
        xn = prox_data_w<T>(v[k] - tau * acc[k], t[k], own[k], tl, L1);
      else if constexpr (FORM == kKl)
        xn = prox_kl<T>(v[k] - tau * acc[k], t[k], own[k], tl);
      else
        xn = prox_data<T>(v[k] - tau * acc[k], t[k], tl, den, L1);
      o[k] = xn + theta * (xn - v[k]);
      v[k] = xn;
    }
    vs<RAG, T, VEC>(c.nval, x + c.i, v);
    vs<RAG, T, VEC>(c.nval, xbar + c.i, o);
    // w_a+ = w_a - tau (-p_a + D_a^T q_aa + sum_{b != a} D_b^T q_ab)
#pragma unroll
    for (int a = 0; a < NDIM; ++a) {
      adj_dir<RAG, T, VEC>(a, q + a * G.n, G, c, own, t);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = -pw[a][k] + t[k];
#pragma unroll
      for (int b = 0; b < NDIM; ++b) {
        if (b == a) continue;
        const int m = a < b ? sym_off<NDIM>(a, b) : sym_off<NDIM>(b, a);
        adj_dir<RAG, T, VEC>(b, q + m * G.n, G, c, own, t);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += t[k];
      }
      vlc<RAG, T, VEC>(c, w + a * G.n + c.i, v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const T wn = v[k] - tau * acc[k];
        o[k] = wn + theta * (wn - v[k]);
        v[k] = wn;
      }
      vs<RAG, T, VEC>(c.nval, w + a * G.n + c.i, v);
      vs<RAG, T, VEC>(c.nval, wbar + a * G.n + c.i, o);
    }
  }
}

template <typename T, int VEC, int ROWS, int NDIM, bool RAG, bool ISO, bool L1>
__global__ __launch_bounds__(kBlock) void k_tgv_primal(
    const T *__restrict__ p, const T *__restrict__ q, T *x, T *xbar, T *w, T *wbar,
    const T *__restrict__ bt, Geom<T> G, T tau, T tl, T den, T theta) {
  // (ISO does not change the primal step; it is a template parameter so that both
  // kernels of one iteration are named by the same list)
  tgv_primal_body<T, VEC, ROWS, NDIM, RAG, L1, kPlain>(p, q, x, xbar, w, wbar, bt, nullptr,
                                                       G, tau, tl, den, theta, T(0), T(0));
}

template <typename T, int VEC, int ROWS, int NDIM, bool RAG, bool L1>
__global__ __launch_bounds__(kBlock) void k_tgv_primal_w(
    const T *__restrict__ p, const T *__restrict__ q, T *x, T *xbar, T *w, T *wbar,
    const T *__restrict__ bt, const T *__restrict__ wt, Geom<T> G, T tau, T tl, T theta) {
  tgv_primal_body<T, VEC, ROWS, NDIM, RAG, L1, kWgt>(p, q, x, xbar, w, wbar, bt, wt, G, tau,
                                                     tl, T(0), theta, T(0), T(0));
}

template <typename T, int VEC, int ROWS, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_tgv_primal_lin(
    const T *__restrict__ p, const T *__restrict__ q, T *x, T *xbar, T *w, T *wbar,
    const T *__restrict__ g, Geom<T> G, T tau, T theta, T lo, T hi) {
  tgv_primal_body<T, VEC, ROWS, NDIM, RAG, false, kLin>(p, q, x, xbar, w, wbar, g, nullptr,
                                                        G, tau, T(0), T(0), theta, lo, hi);
}

template <typename T, int VEC, int ROWS, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_tgv_primal_kl(
    const T *__restrict__ p, const T *__restrict__ q, T *x, T *xbar, T *w, T *wbar,
    const T *__restrict__ bt, const T *__restrict__ wt, Geom<T> G, T tau, T tl, T theta) {
  tgv_primal_body<T, VEC, ROWS, NDIM, RAG, false, kKl>(p, q, x, xbar, w, wbar, bt, wt, G,
                                                       tau, tl, T(0), theta, T(0), T(0));
}

// tgv_primal_body (kPlain, kWgt) on member m = blockIdx.z: the state at member-major
// offsets as in k_tgv_dual_stack, bt and wt at a member stride of 0 (a sweep shares them)
// or n (a batch brings one per member), tl and den from the table.
template <typename T, int VEC, int ROWS, int NDIM, bool RAG, bool L1>
__global__ __launch_bounds__(kBlock) void k_tgv_primal_stack(
    const T *__restrict__ p, const T *__restrict__ q, T *x, T *xbar, T *w, T *wbar,
    const T *__restrict__ bt, int64_t bt_stride, Geom<T> G, T tau, T theta,
    const TgvMember<T> *__restrict__ tab) {
  constexpr int M = NDIM * (NDIM + 1) / 2;
  const int64_t m = blockIdx.z;
  const TgvMember<T> s = tab[m];
  tgv_primal_body<T, VEC, ROWS, NDIM, RAG, L1, kPlain>(
      p + m * NDIM * G.n, q + m * M * G.n, x + m * G.n, xbar + m * G.n, w + m * NDIM * G.n,
      wbar + m * NDIM * G.n, bt + m * bt_stride, nullptr, G, tau, s.tl, s.den, theta, T(0),
      T(0));
}

template <typename T, int VEC, int ROWS, int NDIM, bool RAG, bool L1>
__global__ __launch_bounds__(kBlock) void k_tgv_primal_w_stack(
    const T *__restrict__ p, const T *__restrict__ q, T *x, T *xbar, T *w, T *wbar,
    const T *__restrict__ bt, int64_t bt_stride, const T *__restrict__ wt,
    int64_t wt_stride, Geom<T> G, T tau, T theta, const TgvMember<T> *__restrict__ tab) {
  constexpr int M = NDIM * (NDIM + 1) / 2;
  const int64_t m = blockIdx.z;
  tgv_primal_body<T, VEC, ROWS, NDIM, RAG, L1, kWgt>(
      p + m * NDIM * G.n, q + m * M * G.n, x + m * G.n, xbar + m * G.n, w + m * NDIM * G.n,
      wbar + m * NDIM * G.n, bt + m * bt_stride, wt + m * wt_stride, G, tau, tab[m].tl,
      T(0), theta, T(0), T(0));
}

// tgv_primal_body (kLin) on member m = blockIdx.z: the state at member-major offsets as
// in k_tgv_dual_stack, g = A^T r at m n (every member has its own).  tau, theta and the
// box are shared by value; a member's lambda sits in the data side's r update and its
// beta in the dual kernel, so this kernel reads no table.
template <typename T, int VEC, int ROWS, int NDIM, bool RAG>
__global__ __launch_bounds__(kBlock) void k_tgv_primal_lin_stack(
    const T *__restrict__ p, const T *__restrict__ q, T *x, T *xbar, T *w, T *wbar,
    const T *__restrict__ g, Geom<T> G, T tau, T theta, T lo, T hi) {
  constexpr int M = NDIM * (NDIM + 1) / 2;
  const int64_t m = blockIdx.z;
  tgv_primal_body<T, VEC, ROWS, NDIM, RAG, false, kLin>(
      p + m * NDIM * G.n, q + m * M * G.n, x + m * G.n, xbar + m * G.n, w + m * NDIM * G.n,
      wbar + m * NDIM * G.n, g + m * G.n, nullptr, G, tau, T(0), T(0), theta, lo, hi);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr int kTgvFlags = NSOL_PD_REG_ISOTROPIC | NSOL_PD_DATA_L1;

struct Span {
  const void *ptr;
  int64_t bytes;
};

// a missing pointer, or two of the arrays overlap
template <size_t N>
bool spans_bad(const Span (&s)[N]) {
  for (size_t i = 0; i < N; ++i) {
    if (!s[i].ptr) return true;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(s[i].ptr), a1 = a0 + s[i].bytes;
    for (size_t j = 0; j < i; ++j) {
      const uintptr_t b0 = reinterpret_cast<uintptr_t>(s[j].ptr), b1 = b0 + s[j].bytes;
      if (a0 < b1 && b0 < a1) return true;
    }
  }
  return false;
}

inline bool positive(double v) { return isfinite(v) && v > 0.0; }

// 0: go on; else the value to return (1 stands for "n = 0: return 0")
inline int tgv_geometry(int ndim, int64_t nz, int64_t ny, int64_t nx, int flags) {
  if (ndim < 1 || ndim > 3 || nz < 0 || ny < 0 || nx < 0 || (flags & ~kTgvFlags))
    return NSOL_EINVAL;
  if (nz == 0 || ny == 0 || nx == 0) return 1;
  if (!geom_ok(ndim, nz, ny, nx)) return NSOL_EINVAL;
  // more than 2^31 voxels (by division: the product itself may not fit 64 bits)
  constexpr int64_t most = (int64_t)1 << 31;
  if (nx > most || ny > most / nx || nz > most / (ny * nx)) return -2;
  if (!stencil_grid_ok(nz, ny, nx)) return -2;
  return 0;
}

template <typename T, typename F>
int tgv_dispatch(int ndim, int64_t nz, int64_t ny, int64_t nx, bool aligned, F f,
                 std::atomic<int> &launches = g_tgv_launches) {
  return dispatch_stencil<T>(nz, ny, nx, aligned, [&](auto vec, auto rows, auto rag) {
    int rc;
    switch (ndim) {
      case 1: rc = f(vec, rows, rag, std::integral_constant<int, 1>()); break;
      case 2: rc = f(vec, rows, rag, std::integral_constant<int, 2>()); break;
      default: rc = f(vec, rows, rag, std::integral_constant<int, 3>()); break;
    }
    if (rc == 0) launches.fetch_add(1, std::memory_order_relaxed);
    return rc;
  });
}

template <typename T>
int tgv_dual_impl(const T *xbar, const T *wbar, T *p, T *q, int ndim, int64_t nz,
                  int64_t ny, int64_t nx, double wx, double wy, double wz, double sigma,
                  double beta, int flags, void *stream) {
  const int gr = tgv_geometry(ndim, nz, ny, nx, flags);
  if (gr) return gr == 1 ? 0 : gr;
  const int64_t nb = nz * ny * nx * (int64_t)sizeof(T), M = ndim * (ndim + 1) / 2;
  const Span spans[] = {{xbar, nb}, {wbar, ndim * nb}, {p, ndim * nb}, {q, M * nb}};
  if (spans_bad(spans) || !positive(sigma) || !positive(beta)) return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  const bool al = aligned16(xbar) && aligned16(wbar) && aligned16(p) && aligned16(q);
  const hipStream_t st = as_stream(stream);
  return tgv_dispatch<T>(ndim, nz, ny, nx, al, [&](auto vec, auto rows, auto rag, auto nd) {
    constexpr int V = decltype(vec)::value, R = decltype(rows)::value;
    constexpr int D = decltype(nd)::value;
    constexpr bool RG = decltype(rag)::value;
    const dim3 grid = stencil_grid<V, R>(nz, ny, nx);
    if (flags & NSOL_PD_REG_ISOTROPIC)
      hipLaunchKernelGGL((k_tgv_dual<T, V, R, D, RG, true>), grid, dim3(kBlock), 0, st,
                         xbar, wbar, p, q, G, (T)sigma, (T)beta);
    else
      hipLaunchKernelGGL((k_tgv_dual<T, V, R, D, RG, false>), grid, dim3(kBlock), 0, st,
                         xbar, wbar, p, q, G, (T)sigma, (T)beta);
    return launch_status();
  });
}

template <typename T>
int tgv_primal_impl(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar, const T *bt,
                    int ndim, int64_t nz, int64_t ny, int64_t nx, double wx, double wy,
                    double wz, double tau, double tl, double theta, int flags,
                    void *stream) {
  const int gr = tgv_geometry(ndim, nz, ny, nx, flags);
  if (gr) return gr == 1 ? 0 : gr;
  const int64_t nb = nz * ny * nx * (int64_t)sizeof(T), M = ndim * (ndim + 1) / 2;
  const Span spans[] = {{p, ndim * nb}, {q, M * nb},       {x, nb}, {xbar, nb},
                        {w, ndim * nb}, {wbar, ndim * nb}, {bt, nb}};
  if (spans_bad(spans) || !positive(tau) || !(isfinite(tl) && tl >= 0.0) ||
      !isfinite(theta))
    return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  const bool al = aligned16(p) && aligned16(q) && aligned16(x) && aligned16(xbar) &&
                  aligned16(w) && aligned16(wbar) && aligned16(bt);
  const hipStream_t st = as_stream(stream);
  const T den = prox_den<T>(tl);
  const bool l1 = (flags & NSOL_PD_DATA_L1) != 0;
  return tgv_dispatch<T>(ndim, nz, ny, nx, al, [&](auto vec, auto rows, auto rag, auto nd) {
    constexpr int V = decltype(vec)::value, R = decltype(rows)::value;
    constexpr int D = decltype(nd)::value;
    constexpr bool RG = decltype(rag)::value;
    const dim3 grid = stencil_grid<V, R>(nz, ny, nx);
    // (the projection does not enter the primal step: one instantiation serves both)
    if (l1)
      hipLaunchKernelGGL((k_tgv_primal<T, V, R, D, RG, false, true>), grid, dim3(kBlock),
                         0, st, p, q, x, xbar, w, wbar, bt, G, (T)tau, (T)tl, den,
                         (T)theta);
    else
      hipLaunchKernelGGL((k_tgv_primal<T, V, R, D, RG, false, false>), grid, dim3(kBlock),
                         0, st, p, q, x, xbar, w, wbar, bt, G, (T)tau, (T)tl, den,
                         (T)theta);
    return launch_status();
  });
}

template <typename T>
int tgv_primal_w_impl(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar, const T *bt,
                      const T *wt, int ndim, int64_t nz, int64_t ny, int64_t nx, double wx,
                      double wy, double wz, double tau, double tl, double theta, int flags,
                      void *stream) {
  if (flags & ~NSOL_PD_DATA_L1) return NSOL_EINVAL;
  const int gr = tgv_geometry(ndim, nz, ny, nx, flags);
  if (gr) return gr == 1 ? 0 : gr;
  const int64_t nb = nz * ny * nx * (int64_t)sizeof(T), M = ndim * (ndim + 1) / 2;
  const Span spans[] = {{p, ndim * nb}, {q, M * nb},       {x, nb},  {xbar, nb},
                        {w, ndim * nb}, {wbar, ndim * nb}, {bt, nb}, {wt, nb}};
  if (spans_bad(spans) || !positive(tau) || !(isfinite(tl) && tl >= 0.0) ||
      !isfinite(theta))
    return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  const bool al = aligned16(p) && aligned16(q) && aligned16(x) && aligned16(xbar) &&
                  aligned16(w) && aligned16(wbar) && aligned16(bt) && aligned16(wt);
  const hipStream_t st = as_stream(stream);
  const bool l1 = (flags & NSOL_PD_DATA_L1) != 0;
  return tgv_dispatch<T>(ndim, nz, ny, nx, al, [&](auto vec, auto rows, auto rag, auto nd) {
    constexpr int V = decltype(vec)::value, R = decltype(rows)::value;
    constexpr int D = decltype(nd)::value;
    constexpr bool RG = decltype(rag)::value;
    const dim3 grid = stencil_grid<V, R>(nz, ny, nx);
    if (l1)
      hipLaunchKernelGGL((k_tgv_primal_w<T, V, R, D, RG, true>), grid, dim3(kBlock), 0, st,
                         p, q, x, xbar, w, wbar, bt, wt, G, (T)tau, (T)tl, (T)theta);
    else
      hipLaunchKernelGGL((k_tgv_primal_w<T, V, R, D, RG, false>), grid, dim3(kBlock), 0, st,
                         p, q, x, xbar, w, wbar, bt, wt, G, (T)tau, (T)tl, (T)theta);
    return launch_status();
  });
}

// wt may be null: all weights 1
template <typename T>
int tgv_primal_kl_impl(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar, const T *bt,
                       const T *wt, int ndim, int64_t nz, int64_t ny, int64_t nx, double wx,
                       double wy, double wz, double tau, double tl, double theta,
                       void *stream) {
  const int gr = tgv_geometry(ndim, nz, ny, nx, 0);
  if (gr) return gr == 1 ? 0 : gr;
  const int64_t nb = nz * ny * nx * (int64_t)sizeof(T), M = ndim * (ndim + 1) / 2;
  const Span spans[] = {{p, ndim * nb}, {q, M * nb},       {x, nb},  {xbar, nb},
                        {w, ndim * nb}, {wbar, ndim * nb}, {bt, nb},
                        // (no weights: an empty span, which overlaps nothing)
                        {wt ? wt : bt, wt ? nb : 0}};
  if (spans_bad(spans) || !positive(tau) || !(isfinite(tl) && tl >= 0.0) ||
      !isfinite(theta))
    return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  const bool al = aligned16(p) && aligned16(q) && aligned16(x) && aligned16(xbar) &&
                  aligned16(w) && aligned16(wbar) && aligned16(bt) &&
                  (!wt || aligned16(wt));
  const hipStream_t st = as_stream(stream);
  return tgv_dispatch<T>(ndim, nz, ny, nx, al, [&](auto vec, auto rows, auto rag, auto nd) {
    constexpr int V = decltype(vec)::value, R = decltype(rows)::value;
    constexpr int D = decltype(nd)::value;
    constexpr bool RG = decltype(rag)::value;
    const dim3 grid = stencil_grid<V, R>(nz, ny, nx);
    hipLaunchKernelGGL((k_tgv_primal_kl<T, V, R, D, RG>), grid, dim3(kBlock), 0, st, p, q,
                       x, xbar, w, wbar, bt, wt, G, (T)tau, (T)tl, (T)theta);
    return launch_status();
  });
}

template <typename T>
int tgv_primal_lin_impl(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar, const T *g,
                        int ndim, int64_t nz, int64_t ny, int64_t nx, double wx, double wy,
                        double wz, double tau, double theta, double lo, double hi,
                        void *stream) {
  const int gr = tgv_geometry(ndim, nz, ny, nx, 0);
  if (gr) return gr == 1 ? 0 : gr;
  const int64_t nb = nz * ny * nx * (int64_t)sizeof(T), M = ndim * (ndim + 1) / 2;
  const Span spans[] = {{p, ndim * nb}, {q, M * nb},       {x, nb}, {xbar, nb},
                        {w, ndim * nb}, {wbar, ndim * nb}, {g, nb}};
  if (spans_bad(spans) || !positive(tau) || !isfinite(theta) || !(lo <= hi))
    return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  const bool al = aligned16(p) && aligned16(q) && aligned16(x) && aligned16(xbar) &&
                  aligned16(w) && aligned16(wbar) && aligned16(g);
  const hipStream_t st = as_stream(stream);
  T l, h;
  box_in<T>(lo, hi, l, h);
  return tgv_dispatch<T>(ndim, nz, ny, nx, al, [&](auto vec, auto rows, auto rag, auto nd) {
    constexpr int V = decltype(vec)::value, R = decltype(rows)::value;
    constexpr int D = decltype(nd)::value;
    constexpr bool RG = decltype(rag)::value;
    const dim3 grid = stencil_grid<V, R>(nz, ny, nx);
    hipLaunchKernelGGL((k_tgv_primal_lin<T, V, R, D, RG>), grid, dim3(kBlock), 0, st, p, q,
                       x, xbar, w, wbar, g, G, (T)tau, (T)theta, l, h);
    return launch_status();
  });
}

// ---------------------------------------------------------------------------
// the member-stacked entries
// ---------------------------------------------------------------------------
// The table of a stack, TgvMember<T>[members], from the host's beta[m] and tl[m]: checked
// as tgv_dual_impl and tgv_primal_impl check their scalars and rounded as they round
// them, written to the pinned tab_host and uploaded in one copy on the stream.  The
// steps are constant, so one table serves every iteration of a run.
template <typename T>
int tgv_stack_table_impl(int members, const double *beta, const double *tl, void *tab_host,
                         void *tab, int64_t tab_bytes, void *stream) {
  if (!pd_members_ok(members)) return -2;
  if (!beta || !tl || !tab_host || !tab ||
      tab_bytes < (int64_t)sizeof(TgvMember<T>) * members)
    return NSOL_EINVAL;
  for (int m = 0; m < members; ++m)
    if (!positive(beta[m]) || !(isfinite(tl[m]) && tl[m] >= 0.0)) return NSOL_EINVAL;
  TgvMember<T> *h = static_cast<TgvMember<T> *>(tab_host);
  for (int m = 0; m < members; ++m) {
    h[m].beta = (T)beta[m];
    h[m].tl = (T)tl[m];
    h[m].den = prox_den<T>(tl[m]);
    h[m].pad = T(0);
  }
  const hipError_t e = hipMemcpyAsync(tab, tab_host, sizeof(TgvMember<T>) * (size_t)members,
                                      hipMemcpyHostToDevice, as_stream(stream));
  return e == hipSuccess ? 0 : (int)e;
}

// What every stacked launch checks first.  0: go on; 1: an empty volume, return 0; else
// the value to return.
inline int tgv_stack_geometry(int members, int ndim, int64_t nz, int64_t ny, int64_t nx,
                              int flags) {
  if (!pd_members_ok(members)) return -2;
  return tgv_geometry(ndim, nz, ny, nx, flags);
}

// whole 16-byte vectors need every member to start on a 16-byte boundary: the bases (the
// caller's check) and the member strides in bytes.  Every stride is a multiple of n
// elements; a stride of 0 elements is aligned.
template <typename T>
inline bool stack_strides_aligned(int members, int64_t n) {
  return members == 1 || (n * (int64_t)sizeof(T)) % 16 == 0;
}

template <typename T>
int tgv_stack_dual_impl(const T *xbar, const T *wbar, T *p, T *q, int members, int ndim,
                        int64_t nz, int64_t ny, int64_t nx, double wx, double wy, double wz,
                        double sigma, const void *tab, int flags, void *stream) {
  const int gr = tgv_stack_geometry(members, ndim, nz, ny, nx, flags);
  if (gr) return gr == 1 ? 0 : gr;
  const int64_t n = nz * ny * nx, nb = members * n * (int64_t)sizeof(T);
  const int64_t M = ndim * (ndim + 1) / 2;
  const Span spans[] = {{xbar, nb}, {wbar, ndim * nb}, {p, ndim * nb}, {q, M * nb}};
  if (spans_bad(spans) || !tab || !positive(sigma)) return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  const bool al = aligned16(xbar) && aligned16(wbar) && aligned16(p) && aligned16(q) &&
                  stack_strides_aligned<T>(members, n);
  const hipStream_t st = as_stream(stream);
  const TgvMember<T> *tb = static_cast<const TgvMember<T> *>(tab);
  return tgv_dispatch<T>(
      ndim, nz, ny, nx, al,
      [&](auto vec, auto rows, auto rag, auto nd) {
        constexpr int V = decltype(vec)::value, R = decltype(rows)::value;
        constexpr int D = decltype(nd)::value;
        constexpr bool RG = decltype(rag)::value;
        dim3 grid = stencil_grid<V, R>(nz, ny, nx);
        grid.z = (unsigned)members;
        if (flags & NSOL_PD_REG_ISOTROPIC)
          hipLaunchKernelGGL((k_tgv_dual_stack<T, V, R, D, RG, true>), grid, dim3(kBlock), 0,
                             st, xbar, wbar, p, q, G, (T)sigma, tb);
        else
          hipLaunchKernelGGL((k_tgv_dual_stack<T, V, R, D, RG, false>), grid, dim3(kBlock), 0,
                             st, xbar, wbar, p, q, G, (T)sigma, tb);
        return launch_status();
      },
      g_tgv_stack_launches);
}

// wt == nullptr with weighted == false: the plain prox
template <typename T>
int tgv_stack_primal_impl(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar, const T *bt,
                          int64_t bt_stride, const T *wt, int64_t wt_stride, bool weighted,
                          int members, int ndim, int64_t nz, int64_t ny, int64_t nx,
                          double wx, double wy, double wz, double tau, double theta,
                          const void *tab, int flags, void *stream) {
  if (weighted && (flags & ~NSOL_PD_DATA_L1)) return NSOL_EINVAL;
  const int gr = tgv_stack_geometry(members, ndim, nz, ny, nx, flags);
  if (gr) return gr == 1 ? 0 : gr;
  const int64_t n = nz * ny * nx, n1 = n * (int64_t)sizeof(T), nb = members * n1;
  const int64_t M = ndim * (ndim + 1) / 2;
  if (!pd_stride_ok(bt_stride, n) || (weighted && !pd_stride_ok(wt_stride, n)))
    return NSOL_EINVAL;
  const Span spans[] = {{p, ndim * nb}, {q, M * nb}, {x, nb}, {xbar, nb}, {w, ndim * nb},
                        {wbar, ndim * nb}, {bt, bt_stride ? nb : n1},
                        // (unweighted: an empty span, which overlaps nothing)
                        {weighted ? wt : bt, weighted ? (wt_stride ? nb : n1) : 0}};
  if (spans_bad(spans) || !tab || !positive(tau) || !isfinite(theta)) return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  const bool al = aligned16(p) && aligned16(q) && aligned16(x) && aligned16(xbar) &&
                  aligned16(w) && aligned16(wbar) && aligned16(bt) &&
                  (!weighted || aligned16(wt)) && stack_strides_aligned<T>(members, n);
  const hipStream_t st = as_stream(stream);
  const TgvMember<T> *tb = static_cast<const TgvMember<T> *>(tab);
  const bool l1 = (flags & NSOL_PD_DATA_L1) != 0;
  return tgv_dispatch<T>(
      ndim, nz, ny, nx, al,
      [&](auto vec, auto rows, auto rag, auto nd) {
        constexpr int V = decltype(vec)::value, R = decltype(rows)::value;
        constexpr int D = decltype(nd)::value;
        constexpr bool RG = decltype(rag)::value;
        dim3 grid = stencil_grid<V, R>(nz, ny, nx);
        grid.z = (unsigned)members;
        if (weighted) {
          if (l1)
            hipLaunchKernelGGL((k_tgv_primal_w_stack<T, V, R, D, RG, true>), grid,
                               dim3(kBlock), 0, st, p, q, x, xbar, w, wbar, bt, bt_stride, wt,
                               wt_stride, G, (T)tau, (T)theta, tb);
          else
            hipLaunchKernelGGL((k_tgv_primal_w_stack<T, V, R, D, RG, false>), grid,
                               dim3(kBlock), 0, st, p, q, x, xbar, w, wbar, bt, bt_stride, wt,
                               wt_stride, G, (T)tau, (T)theta, tb);
        } else {
          if (l1)
            hipLaunchKernelGGL((k_tgv_primal_stack<T, V, R, D, RG, true>), grid,
                               dim3(kBlock), 0, st, p, q, x, xbar, w, wbar, bt, bt_stride, G,
                               (T)tau, (T)theta, tb);
          else
            hipLaunchKernelGGL((k_tgv_primal_stack<T, V, R, D, RG, false>), grid,
                               dim3(kBlock), 0, st, p, q, x, xbar, w, wbar, bt, bt_stride, G,
                               (T)tau, (T)theta, tb);
        }
        return launch_status();
      },
      g_tgv_stack_launches);
}

// tgv_primal_lin_impl's checks and rounding of the box on spans `members` times as long
template <typename T>
int tgv_stack_primal_lin_impl(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar,
                              const T *g, int members, int ndim, int64_t nz, int64_t ny,
                              int64_t nx, double wx, double wy, double wz, double tau,
                              double theta, double lo, double hi, void *stream) {
  const int gr = tgv_stack_geometry(members, ndim, nz, ny, nx, 0);
  if (gr) return gr == 1 ? 0 : gr;
  const int64_t n = nz * ny * nx, nb = members * n * (int64_t)sizeof(T);
  const int64_t M = ndim * (ndim + 1) / 2;
  const Span spans[] = {{p, ndim * nb}, {q, M * nb},       {x, nb}, {xbar, nb},
                        {w, ndim * nb}, {wbar, ndim * nb}, {g, nb}};
  if (spans_bad(spans) || !positive(tau) || !isfinite(theta) || !(lo <= hi))
    return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  const bool al = aligned16(p) && aligned16(q) && aligned16(x) && aligned16(xbar) &&
                  aligned16(w) && aligned16(wbar) && aligned16(g) &&
                  stack_strides_aligned<T>(members, n);
  const hipStream_t st = as_stream(stream);
  T l, h;
  box_in<T>(lo, hi, l, h);
  return tgv_dispatch<T>(
      ndim, nz, ny, nx, al,
      [&](auto vec, auto rows, auto rag, auto nd) {
        constexpr int V = decltype(vec)::value, R = decltype(rows)::value;
        constexpr int D = decltype(nd)::value;
        constexpr bool RG = decltype(rag)::value;
        dim3 grid = stencil_grid<V, R>(nz, ny, nx);
        grid.z = (unsigned)members;
        hipLaunchKernelGGL((k_tgv_primal_lin_stack<T, V, R, D, RG>), grid, dim3(kBlock), 0,
                           st, p, q, x, xbar, w, wbar, g, G, (T)tau, (T)theta, l, h);
        return launch_status();
      },
      g_tgv_stack_launches);
}

}  // namespace

extern "C" {

int nsol_tgv_launches(void) { return g_tgv_launches.load(std::memory_order_relaxed); }
int nsol_tgv_stack_launches(void) {
  return g_tgv_stack_launches.load(std::memory_order_relaxed);
}

#define NSOL_TGV_DEF(T, SUF)                                                              \
  int nsol_tgv_dual_##SUF(const T *xbar, const T *wbar, T *p, T *q, int ndim, int64_t nz, \
                          int64_t ny, int64_t nx, double wx, double wy, double wz,        \
                          double sigma, double beta, int flags, void *s) {                \
    return tgv_dual_impl<T>(xbar, wbar, p, q, ndim, nz, ny, nx, wx, wy, wz, sigma, beta,  \
                            flags, s);                                                    \
  }                                                                                       \
  int nsol_tgv_primal_##SUF(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar,         \
                            const T *bt, int ndim, int64_t nz, int64_t ny, int64_t nx,    \
                            double wx, double wy, double wz, double tau, double tl,       \
                            double theta, int flags, void *s) {                           \
    return tgv_primal_impl<T>(p, q, x, xbar, w, wbar, bt, ndim, nz, ny, nx, wx, wy, wz,   \
                              tau, tl, theta, flags, s);                                  \
  }                                                                                       \
  int nsol_tgv_primal_w_##SUF(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar,       \
                              const T *bt, const T *wt, int ndim, int64_t nz, int64_t ny, \
                              int64_t nx, double wx, double wy, double wz, double tau,    \
                              double tl, double theta, int flags, void *s) {              \
    return tgv_primal_w_impl<T>(p, q, x, xbar, w, wbar, bt, wt, ndim, nz, ny, nx, wx, wy, \
                                wz, tau, tl, theta, flags, s);                            \
  }                                                                                       \
  int nsol_tgv_primal_kl_##SUF(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar,      \
                               const T *bt, const T *wt, int ndim, int64_t nz,            \
                               int64_t ny, int64_t nx, double wx, double wy, double wz,   \
                               double tau, double tl, double theta, void *s) {            \
    return tgv_primal_kl_impl<T>(p, q, x, xbar, w, wbar, bt, wt, ndim, nz, ny, nx, wx,    \
                                 wy, wz, tau, tl, theta, s);                              \
  }                                                                                       \
  int nsol_tgv_primal_lin_##SUF(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar,     \
                                const T *g, int ndim, int64_t nz, int64_t ny, int64_t nx, \
                                double wx, double wy, double wz, double tau,              \
                                double theta, double lo, double hi, void *s) {            \
    return tgv_primal_lin_impl<T>(p, q, x, xbar, w, wbar, g, ndim, nz, ny, nx, wx, wy,    \
                                  wz, tau, theta, lo, hi, s);                             \
  }

#define NSOL_TGV_STACK_DEF(T, SUF)                                                        \
  int nsol_tgv_stack_table_##SUF(int members, const double *beta, const double *tl,       \
                                 void *tab_host, void *tab, int64_t tab_bytes, void *s) { \
    return tgv_stack_table_impl<T>(members, beta, tl, tab_host, tab, tab_bytes, s);       \
  }                                                                                       \
  int nsol_tgv_stack_dual_##SUF(const T *xbar, const T *wbar, T *p, T *q, int members,    \
                                int ndim, int64_t nz, int64_t ny, int64_t nx, double wx,  \
                                double wy, double wz, double sigma, const void *tab,      \
                                int flags, void *s) {                                     \
    return tgv_stack_dual_impl<T>(xbar, wbar, p, q, members, ndim, nz, ny, nx, wx, wy, wz, \
                                  sigma, tab, flags, s);                                  \
  }                                                                                       \
  int nsol_tgv_stack_primal_##SUF(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar,   \
                                  const T *bt, int64_t bt_stride, int members, int ndim,  \
                                  int64_t nz, int64_t ny, int64_t nx, double wx,          \
                                  double wy, double wz, double tau, double theta,         \
                                  const void *tab, int flags, void *s) {                  \
    return tgv_stack_primal_impl<T>(p, q, x, xbar, w, wbar, bt, bt_stride, nullptr, 0,    \
                                    false, members, ndim, nz, ny, nx, wx, wy, wz, tau,    \
                                    theta, tab, flags, s);                                \
  }                                                                                       \
  int nsol_tgv_stack_primal_w_##SUF(const T *p, const T *q, T *x, T *xbar, T *w, T *wbar, \
                                    const T *bt, int64_t bt_stride, const T *wt,          \
                                    int64_t wt_stride, int members, int ndim, int64_t nz, \
                                    int64_t ny, int64_t nx, double wx, double wy,         \
                                    double wz, double tau, double theta, const void *tab, \
                                    int flags, void *s) {                                 \
    return tgv_stack_primal_impl<T>(p, q, x, xbar, w, wbar, bt, bt_stride, wt, wt_stride, \
                                    true, members, ndim, nz, ny, nx, wx, wy, wz, tau,     \
                                    theta, tab, flags, s);                                \
  }                                                                                       \
  int nsol_tgv_stack_primal_lin_##SUF(const T *p, const T *q, T *x, T *xbar, T *w,        \
                                      T *wbar, const T *g, int members, int ndim,         \
                                      int64_t nz, int64_t ny, int64_t nx, double wx,      \
                                      double wy, double wz, double tau, double theta,     \
                                      double lo, double hi, void *s) {                    \
    return tgv_stack_primal_lin_impl<T>(p, q, x, xbar, w, wbar, g, members, ndim, nz, ny, \
                                        nx, wx, wy, wz, tau, theta, lo, hi, s);           \
  }

NSOL_TGV_DEF(float, f32)
NSOL_TGV_DEF(double, f64)
#undef NSOL_TGV_DEF
NSOL_TGV_STACK_DEF(float, f32)
NSOL_TGV_STACK_DEF(double, f64)
#undef NSOL_TGV_STACK_DEF

}  // extern "C"
