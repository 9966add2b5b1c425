// Chambolle-Pock primal-dual iteration for gfx950 (MI355X).
//
// reference: primal_dual_solver.py:232-261 driving linear_operators.py:121-169
// and proximal_operators.py:95-159.
//
// Three forms, all producing the same per-voxel arithmetic (same operation
// order as the NumPy reference; the library is built with -ffp-contract=off):
//   * k_dual_step / k_primal_step: two passes (14 words per voxel in 3-D);
//   * k_pd_fused: ONE pass, 11 words per voxel (read xbar, x, bt, p[3]; write
//     p[3], x, xbar).  Each wave owns a (LX*VEC) x (LY*RY) patch of an x-y tile
//     and marches along z, keeping xbar[z], xbar[z+1] and the new p_z[z-1] in
//     registers; x-neighbours travel by wave shuffles, y-neighbours live in
//     registers (RY rows per lane) or come from the neighbouring lane row; only
//     the patch's outer halo (one row above/below, one column left/right) is
//     re-read from L1/L2.  The dual update of the lower halo (p_new at i - e_a)
//     is recomputed instead of being exchanged, so there is no inter-workgroup
//     dependency inside a launch; xbar and p are ping-pong buffers.
#include <stdlib.h>
#include <string.h>

#include "nsol_common.hpp"
#include "nsol_pd_common.hpp"
#include "nsol_pd_fused_body.hpp"
#include "nsol_pd_launch.hpp"

using namespace nsol;

namespace {

struct PdTuning {
  int zchunk = 0;   // 0 = auto
  int ry = 0;       // rows per lane (1, 2 or 4); 0 = auto
  int force_two_pass = 0;
  int xcd_map = 1;  // 0 = plain block order, 1 = XCD-aware slabs
  int rag = 1;      // unaligned rows: 1 = element-aligned 16-byte accesses, 0 = 4-byte
};
PdTuning g_tune;

// ---------------------------------------------------------------------------
// two-pass form
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dual_step(
    const T *__restrict__ xbar, const T *p_in, T *p_out, Geom<T> G, T sigma,
    T hden, bool huber) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G.n;
       i += stride) {
    const int64_t ix = i % G.nx;
    const int64_t r = i / G.nx;
    const int64_t iy = r % G.ny;
    const int64_t iz = r / G.ny;
    const T c = xbar[i];
    {
      const T nb = (ix + 1 < G.nx) ? xbar[i + 1] : T(0);
      T q = (p_in ? p_in[i] : T(0)) + sigma * (nb * G.wx + c * (-G.wx));
      if (huber) q = huber_div(q, hden);
      p_out[i] = dual_clamp(q);
    }
    if (G.ndim >= 2) {
      const T nb = (iy + 1 < G.ny) ? xbar[i + G.sy] : T(0);
      T q = (p_in ? p_in[G.n + i] : T(0)) + sigma * (nb * G.wy + c * (-G.wy));
      if (huber) q = huber_div(q, hden);
      p_out[G.n + i] = dual_clamp(q);
    }
    if (G.ndim >= 3) {
      const T nb = (iz + 1 < G.nz) ? xbar[i + G.sz] : T(0);
      T q = (p_in ? p_in[2 * G.n + i] : T(0)) +
            sigma * (nb * G.wz + c * (-G.wz));
      if (huber) q = huber_div(q, hden);
      p_out[2 * G.n + i] = dual_clamp(q);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_primal_step(
    const T *__restrict__ p, T *__restrict__ x, T *__restrict__ xbar,
    const T *__restrict__ bt, Geom<T> G, T tau, T tl, T one_plus_tl, T theta,
    bool l1) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G.n;
       i += stride) {
    const int64_t ix = i % G.nx;
    const int64_t r = i / G.nx;
    T kt = p[i] * (-G.wx) + ((ix > 0) ? p[i - 1] : T(0)) * G.wx;
    if (G.ndim >= 2) {
      const T *py = p + G.n;
      kt += py[i] * (-G.wy) + ((r % G.ny > 0) ? py[i - G.sy] : T(0)) * G.wy;
    }
    if (G.ndim >= 3) {
      const T *pz = p + 2 * G.n;
      kt += pz[i] * (-G.wz) + ((r / G.ny > 0) ? pz[i - G.sz] : T(0)) * G.wz;
    }
    const T xo = x[i];
    const T u = xo - tau * kt;
    const T xn = prox_data(u, bt[i], tl, one_plus_tl, l1);
    x[i] = xn;
    xbar[i] = xn + theta * (xn - xo);
  }
}

// ---------------------------------------------------------------------------
// single-pass fused form
// ---------------------------------------------------------------------------
// RAG: rows that are not a multiple of VEC elements / arrays that are not 16-byte
// aligned (ldv_rag / stv_rag; the elements of a row's last vector that lie behind
// the row read as zero -- exactly the "u := 0 past the last index" of the forward
// difference -- and are never stored).
template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG = false>
__global__ __launch_bounds__(kBlock) void k_pd_fused(
    const T *__restrict__ xbar_in, T *__restrict__ xbar_out, T *x,
    const T *__restrict__ bt, const T *__restrict__ p_in,
    T *__restrict__ p_out, Geom<T> G, PdScalars<T> S, int ntx, int nty,
    int zchunk, int slab) {
  // (the per-tile work lives in nsol_pd_fused_body.hpp, shared with the
  // member-stacked kernel of nsol_pds.hip)
  int tx, ty, zc;
  if (!pd_fused_block_tile(blockIdx.x, ntx, nty, slab, tx, ty, zc)) return;
  pd_fused_tile<T, VEC, LX, RY, NDIM, RAG>(xbar_in, xbar_out, x, bt, p_in, p_out, G, S,
                                           tx, ty, zc, zchunk);
}

struct FusedKernel {
  template <typename T, int VEC, int LX, int RY, int NDIM, bool RAG>
  static int launch_t(const PdLaunchArgs<T> &a) {
    const PdGridPlan g = pd_plan_grid<VEC, LX, RY>(a.G, 1, a.tune);
    if (g.blocks > kPdMaxBlocks) return NSOL_EINVAL;
    hipLaunchKernelGGL((k_pd_fused<T, VEC, LX, RY, NDIM, RAG>), dim3((unsigned)g.blocks),
                       dim3(kBlock), 0, a.st, a.xbar_in, a.xbar_out, a.x, a.bt, a.p_in,
                       a.p_out, a.G, a.S, g.ntx, g.nty, g.zchunk, g.slab);
    return launch_status();
  }

  template <typename T, int VEC, int LX, int RY, bool RAG>
  static int launch_nd(const PdLaunchArgs<T> &a) {
    switch (a.G.ndim) {
      case 1: return launch_t<T, VEC, LX, 1, 1, RAG>(a);
      case 2: return launch_t<T, VEC, LX, RY, 2, RAG>(a);
      default: return launch_t<T, VEC, LX, RY, 3, RAG>(a);
    }
  }

  // knob "pd_ry": 0 = choose; 4 has no ragged form and falls to 2, as any other value
  template <typename T, int VEC, int LX, bool RAG>
  static int launch(const PdLaunchArgs<T> &a) {
    int ry = a.tune.ry;
    if (ry == 0) ry = pd_auto_rows_per_lane<VEC, LX>(a.G, 1);
    switch (ry) {
      case 1: return launch_nd<T, VEC, LX, 1, RAG>(a);
      case 4:
        if constexpr (!RAG) return launch_nd<T, VEC, LX, 4, false>(a);
      default: return launch_nd<T, VEC, LX, 2, RAG>(a);
    }
  }
};

template <typename T>
int fused_iter_impl(const T *xbar_in, T *xbar_out, T *x, const T *bt,
                    const T *p_in, T *p_out, int ndim, int64_t nz, int64_t ny,
                    int64_t nx, double wx, double wy, double wz, double sigma,
                    double hden, double tau, double tl, double theta, int flags,
                    void *stream, int64_t pitch = 0) {
  if (flags & NSOL_PD_DATA_WEIGHTED) return -2;   // no weights pointer here: nsol_pdw.hip
  const PdLaunchTune tune{g_tune.zchunk, g_tune.ry, g_tune.xcd_map, g_tune.rag};
  if (flags & NSOL_PD_REG_ISOTROPIC)   // k_pd_fused_iso, nsol_pdi.hip
    return pd_iso_fused_iter<T>(xbar_in, xbar_out, x, bt, p_in, p_out, ndim, nz, ny, nx,
                                wx, wy, wz, sigma, hden, tau, tl, theta, flags, stream,
                                pitch, tune);
  NSOL_CHECK_GEOM(ndim, nz, ny, nx);
  if (!xbar_in || !xbar_out || !x || !bt || !p_out || xbar_in == xbar_out ||
      p_in == p_out)
    return NSOL_EINVAL;
  // (rows at a pitch: only the strides change -- the kernel indexes rows and planes
  // by G.sy / G.sz and a gradient field's components by G.n)
  PdLaunchArgs<T> a{xbar_in, xbar_out, x, bt, p_in, p_out,
                    make_geom_pitched<T>(ndim, nz, ny, nx, pitch, wx, wy, wz),
                    pd_make_scalars<T>(sigma, hden, tau, tl, theta, flags, p_in != nullptr)};
  a.tune = tune;
  a.st = as_stream(stream);
  return pd_launch<FusedKernel>(a);
}

template <typename T>
int dual_step_impl(const T *xbar, const T *p_in, T *p_out, int ndim, int64_t nz,
                   int64_t ny, int64_t nx, double wx, double wy, double wz,
                   double sigma, double hden, void *stream) {
  NSOL_CHECK_GEOM(ndim, nz, ny, nx);
  if (!xbar || !p_out) return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  hipLaunchKernelGGL(k_dual_step<T>, dim3(grid_for(G.n)), dim3(kBlock), 0,
                     as_stream(stream), xbar, p_in, p_out, G, (T)sigma, huber_den<T>(hden),
                     hden != 1.0);
  return launch_status();
}

template <typename T>
int primal_step_impl(const T *p, T *x, T *xbar, const T *bt, int ndim,
                     int64_t nz, int64_t ny, int64_t nx, double wx, double wy,
                     double wz, double tau, double tl, double theta, int flags,
                     void *stream) {
  NSOL_CHECK_GEOM(ndim, nz, ny, nx);
  if (!p || !x || !xbar || !bt) return NSOL_EINVAL;
  const Geom<T> G = make_geom<T>(ndim, nz, ny, nx, wx, wy, wz);
  hipLaunchKernelGGL(k_primal_step<T>, dim3(grid_for(G.n)), dim3(kBlock), 0,
                     as_stream(stream), p, x, xbar, bt, G, (T)tau, (T)tl,
                     prox_den<T>(tl), (T)theta, (flags & NSOL_PD_DATA_L1) != 0);
  return launch_status();
}

// pitch > nx: every array holds its rows at that pitch (elements; whole 16-byte vectors),
// planes ny * pitch apart, the components of p nz * ny * pitch apart -- the layout
// nsol_amd's solver keeps volumes in whose rows are not whole vectors: aligned accesses,
// the row's partial vector masked in registers, the padding free to hold anything.
template <typename T>
int run_impl(T *xbar0, T *xbar1, T *x, T *x_alt, const T *bt, T *p0, T *p1,
             int ndim, int64_t nz, int64_t ny, int64_t nx, double wx, double wy,
             double wz, double lambda, const double *sig, const double *tau,
             const double *theta, int iterations, int p_is_zero,
             double gamma_huber, int flags, int *final_slot, void *stream,
             int64_t pitch = 0) {
  if (flags & NSOL_PD_DATA_WEIGHTED) return -2;   // no weights pointer here: nsol_pdw.hip
  NSOL_CHECK_GEOM(ndim, nz, ny, nx);
  if (iterations < 0 || !sig || !tau || !theta || !x) return NSOL_EINVAL;
  const bool pitched = pitch > nx;
  if (pitch > 0 && (pitch < nx || ndim != 3 || pitch % (16 / (int64_t)sizeof(T)) != 0))
    return NSOL_EINVAL;
  const bool may_swap = (flags & NSOL_PD_RUN_X_MAY_SWAP) != 0 && final_slot != nullptr;
  flags &= ~NSOL_PD_RUN_X_MAY_SWAP;
  T *xb[2] = {xbar0, xbar1};
  T *pp[2] = {p0, p1};
  T *xcur = x, *xoth = x_alt;
  int slot = 0;
  const bool huber = (flags & NSOL_PD_REG_HUBER) != 0;
  // the isotropic projection has the one-iteration forms only (the multi-iteration
  // entries decline it): one launch of k_pd_fused_iso per iteration
  const bool iso = (flags & NSOL_PD_REG_ISOTROPIC) != 0;
  // A long run ends in a block of shifted launches (k_pd_shift3, nsol_pdk.hip): a
  // stand-alone dual step, m launches of P D P D P D on (x, p) alone, a stand-alone
  // primal step -- 3 m + 1 iterations; the (N - 1) mod 3 iterations before it take the
  // usual rungs (at most two: no depth-3 launch, unless whole triples are handed to the
  // unshifted plan's exploration below)
  int lead = iterations, m_shift = 0;
  if (!iso && xoth && !g_tune.force_two_pass)
    nsol_pd_run_parts(iterations,
                      pd_shift3_min_iters<T>(xcur, xoth, bt, p0, p1, ndim, nz, ny, nx, flags,
                                             pitched ? pitch : 0, iterations),
                      &lead, &m_shift);
  bool ask = false;      // may the unshifted plan still want launches during this run
  if (m_shift > 1) {
    // while the shape's unshifted depth-3 plan is still owed samples (the plan its short
    // runs take), that many leading launches of the block go to it: three iterations
    // each, same bits
    int d = pd_shift3_donation<T>(nz, ny, nx);
    ask = d >= 0;
    if (d < 0) d = 0;
    if (d > m_shift - 1) d = m_shift - 1;
    lead += 3 * d;
    m_shift -= d;
  }
  int n = 0;
  while (n < iterations) {
    if (n == lead && m_shift > 0) {
      const T *pin = (n == 0 && p_is_zero) ? nullptr : pp[slot];
      int rc = dual_step_impl<T>(xb[slot], pin, pp[slot ^ 1], ndim, nz, ny, nx, wx, wy, wz,
                                 sig[n], huber ? 1.0 + sig[n] * gamma_huber : 1.0, stream);
      if (rc) return rc;
      slot ^= 1;                       // p^{n+1} is in pp[slot]; xb[slot] is free
      for (int i = 0; i < m_shift; ++i, n += 3) {
        double h4[4], tl3[3];
        for (int j = 0; j < 4; ++j) h4[j] = huber ? 1.0 + sig[n + j] * gamma_huber : 1.0;
        for (int j = 0; j < 3; ++j) tl3[j] = tau[n + j] * lambda;
        rc = pd_shift3_iter<T>(xcur, xoth, bt, pp[slot], pp[slot ^ 1], ndim, nz, ny, nx, wx,
                               wy, wz, sig + n, h4, tau + n, tl3, theta + n, flags, stream);
        if (rc) return rc == -2 ? NSOL_EINVAL : rc;   // (pd_shift3_min_iters said it applies)
        slot ^= 1;
        T *t = xcur; xcur = xoth; xoth = t;
        // the shifted plan settled on this launch and the unshifted plan still explores:
        // the block ends here, the rest of the run (whole triples) goes to that plan
        if (ask && i + 2 < m_shift && pd_shift3_donation<T>(nz, ny, nx) > 0) m_shift = i + 1;
      }
      rc = primal_step_impl<T>(pp[slot], xcur, xb[slot], bt, ndim, nz, ny, nx, wx, wy, wz,
                               tau[n], tau[n] * lambda, theta[n], flags, stream);
      if (rc) return rc;
      n += 1;
      m_shift = 0;                     // one block per run: what is left takes the rungs
      continue;
    }
    const T *pin = (n == 0 && p_is_zero) ? nullptr : pp[slot];
    const int until = m_shift > 0 ? lead : iterations;   // end of this stretch of rungs
    if (!iso && xoth && n + 1 < until && !g_tune.force_two_pass) {
      // deepest temporal blocking first: 3 iterations per pass (tiled
      // footprints), then 2 (tiled or full-row footprints), then 1
      double h3[3], tl3[3];
      const int left = until - n < 3 ? until - n : 3;
      for (int i = 0; i < left; ++i) {
        h3[i] = huber ? 1.0 + sig[n + i] * gamma_huber : 1.0;
        tl3[i] = tau[n + i] * lambda;
      }
      auto fusedk = [&](int depth) {
        return pd_fusedk_iter<T>(xb[slot], xb[slot ^ 1], xcur, xoth, bt, pin, pp[slot ^ 1],
                                 ndim, nz, ny, nx, wx, wy, wz, depth, sig + n, h3, tau + n,
                                 tl3, theta + n, flags, stream, pitched ? pitch : 0);
      };
      auto fused2 = [&](int) {
        return pd_fused2_iter<T>(xb[slot], xb[slot ^ 1], xcur, xoth, bt, pin, pp[slot ^ 1],
                                 ndim, nz, ny, nx, wx, wy, wz, sig + n, h3, tau + n, tl3,
                                 theta + n, flags, stream);
      };
      // one rung: nothing once an earlier one has run; 0 -> `depth` iterations are
      // done; -2 -> the kernel declined, the next rung is tried; else the error
      int done = 0;
      auto attempt = [&](int depth, auto call) {
        if (done) return 0;
        const int rc = call(depth);
        if (rc == 0) done = depth;
        return rc == -2 ? 0 : rc;
      };
      int err = 0;
      if (pitched) {
        // rows at a pitch: depth 3, then depth 2 of k_pd_fusedk (k_pd_fused2 wants
        // contiguous whole rows), then one iteration at a time
        if (left >= 3) err = attempt(3, fusedk);
        if (!err) err = attempt(2, fusedk);
      } else {
        // trailing pair of a run on a shape whose depth-3 plan has settled
        if (left == 2 && nsol_pd_fusedk_tail2((int)sizeof(T), nz, ny, nx))
          err = attempt(2, fusedk);
        if (!err && left >= 3) err = attempt(3, fusedk);
        if (!err) err = attempt(2, fused2);
        if (!err) err = attempt(2, fusedk);   // e.g. rows too short for the full-row footprints
      }
      if (err) return err;
      if (done) {
        n += done;
        slot ^= 1;
        T *t = xcur; xcur = xoth; xoth = t;
        continue;
      }
    }
    const double hden = huber ? 1.0 + sig[n] * gamma_huber : 1.0;
    int rc;
    if (g_tune.force_two_pass && !pitched) {
      rc = iso ? pd_iso_dual_step<T>(xb[slot], pin, pp[slot ^ 1], ndim, nz, ny, nx, wx,
                                     wy, wz, sig[n], hden, stream)
               : dual_step_impl<T>(xb[slot], pin, pp[slot ^ 1], ndim, nz, ny, nx, wx, wy,
                                   wz, sig[n], hden, stream);
      if (rc) return rc;
      rc = primal_step_impl<T>(pp[slot ^ 1], xcur, xb[slot ^ 1], bt, ndim, nz, ny,
                               nx, wx, wy, wz, tau[n], tau[n] * lambda, theta[n],
                               flags, stream);
    } else {
      rc = fused_iter_impl<T>(xb[slot], xb[slot ^ 1], xcur, bt, pin, pp[slot ^ 1],
                              ndim, nz, ny, nx, wx, wy, wz, sig[n], hden, tau[n],
                              tau[n] * lambda, theta[n], flags, stream, pitch);
    }
    if (rc) return rc;
    n += 1;
    slot ^= 1;
  }
  if (xcur != x && !may_swap) {
    hipError_t e = hipMemcpyAsync(x, xcur,
                                  sizeof(T) * (size_t)(nz * ny * (pitched ? pitch : nx)),
                                  hipMemcpyDeviceToDevice, as_stream(stream));
    if (e != hipSuccess) return (int)e;
  }
  if (final_slot) *final_slot = slot | ((xcur != x && may_swap) ? 2 : 0);
  return 0;
}

}  // namespace

namespace nsol {
PdLaunchTune pd_current_tune() {
  return PdLaunchTune{g_tune.zchunk, g_tune.ry, g_tune.xcd_map, g_tune.rag};
}
}  // namespace nsol

extern "C" {

/* tuning knobs for experiments: "pd_zchunk", "pd_ry", "pd_two_pass" */
int nsol_hip_set_param(const char *name, int value) {
  if (!name) return NSOL_EINVAL;
  if (!strcmp(name, "pd_zchunk")) g_tune.zchunk = value;
  else if (!strcmp(name, "pd_ry")) g_tune.ry = value;
  else if (!strcmp(name, "pd_two_pass")) g_tune.force_two_pass = value;
  else if (!strcmp(name, "pd_xcd_map")) g_tune.xcd_map = value;
  else if (!strcmp(name, "pd_rag")) g_tune.rag = value;
  else if (!strcmp(name, "stencil_slabs")) g_stencil_slabs = value ? 1 : 0;
  else if (!strcmp(name, "stencil_blocks"))
    g_stencil_blocks = value < 256 ? 256 : (value > kReducePartials ? kReducePartials : value);
  else if (!strcmp(name, "max_grid_blocks"))
    g_max_grid_blocks = value < 1 ? 1 : (value > kMaxGridBlocksLimit ? kMaxGridBlocksLimit : value);
  else return NSOL_EINVAL;
  return 0;
}

#define NSOL_PD_DEF(T, SUF)                                                      \
  int nsol_pd_dual_step_##SUF(const T *xbar, const T *p_in, T *p_out, int ndim,  \
                              int64_t nz, int64_t ny, int64_t nx, double wx,     \
                              double wy, double wz, double sigma, double hden,   \
                              void *s) {                                         \
    return dual_step_impl<T>(xbar, p_in, p_out, ndim, nz, ny, nx, wx, wy, wz,    \
                             sigma, hden, s);                                    \
  }                                                                              \
  int nsol_pd_primal_step_##SUF(const T *p, T *x, T *xbar, const T *bt,          \
                                int ndim, int64_t nz, int64_t ny, int64_t nx,    \
                                double wx, double wy, double wz, double tau,     \
                                double tl, double theta, int flags, void *s) {   \
    return primal_step_impl<T>(p, x, xbar, bt, ndim, nz, ny, nx, wx, wy, wz,     \
                               tau, tl, theta, flags, s);                        \
  }                                                                              \
  int nsol_pd_fused_iter_##SUF(const T *xi, T *xo, T *x, const T *bt,            \
                               const T *pi, T *po, int ndim, int64_t nz,         \
                               int64_t ny, int64_t nx, double wx, double wy,     \
                               double wz, double sigma, double hden, double tau, \
                               double tl, double theta, int flags, void *s) {    \
    return fused_iter_impl<T>(xi, xo, x, bt, pi, po, ndim, nz, ny, nx, wx, wy,   \
                              wz, sigma, hden, tau, tl, theta, flags, s);        \
  }                                                                              \
  int nsol_pd_run_##SUF(T *xb0, T *xb1, T *x, T *x_alt, const T *bt, T *p0,      \
                        T *p1, int ndim, int64_t nz, int64_t ny, int64_t nx,     \
                        double wx, double wy, double wz, double lambda,          \
                        const double *sg, const double *ta, const double *th,    \
                        int iters, int p_is_zero, double gh, int flags,          \
                        int *final_slot, void *s) {                              \
    return run_impl<T>(xb0, xb1, x, x_alt, bt, p0, p1, ndim, nz, ny, nx, wx, wy,  \
                       wz, lambda, sg, ta, th, iters, p_is_zero, gh, flags,      \
                       final_slot, s);                                           \
  }

NSOL_PD_DEF(float, f32)
NSOL_PD_DEF(double, f64)

#define NSOL_PD_PITCHED(T, SUF)                                                   \
  int nsol_pd_run_pitched_##SUF(T *xb0, T *xb1, T *x, T *x_alt, const T *bt, T *p0, \
                                T *p1, int ndim, int64_t nz, int64_t ny, int64_t nx, \
                                int64_t pitch, double wx, double wy, double wz,    \
                                double lambda, const double *sg, const double *ta, \
                                const double *th, int iters, int p_is_zero,        \
                                double gh, int flags, int *final_slot, void *s) {  \
    return run_impl<T>(xb0, xb1, x, x_alt, bt, p0, p1, ndim, nz, ny, nx, wx, wy,   \
                       wz, lambda, sg, ta, th, iters, p_is_zero, gh, flags,        \
                       final_slot, s, pitch);                                      \
  }
NSOL_PD_PITCHED(float, f32)
NSOL_PD_PITCHED(double, f64)
#undef NSOL_PD_PITCHED

}  // extern "C"
