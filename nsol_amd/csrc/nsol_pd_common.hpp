// Device helpers, the scalars' struct and the entries that the primal-dual units
// (nsol_pd*.hip) call in each other.  The host-side launch path of the
// one-iteration kernels is nsol_pd_launch.hpp.
#pragma once

#include "nsol_common.hpp"

namespace nsol {

template <typename T, int V>
struct Pack {
  typedef T type __attribute__((ext_vector_type(V)));
};

template <typename T, int V>
__device__ __forceinline__ void ldv(const T *p, T (&v)[V]) {
  if constexpr (V == 1) {
    v[0] = *p;
  } else {
    typedef typename Pack<T, V>::type P;
    const P t = *reinterpret_cast<const P *>(p);
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = t[k];
  }
}

template <typename T, int V>
__device__ __forceinline__ void stv(T *p, const T (&v)[V]) {
  if constexpr (V == 1) {
    *p = v[0];
  } else {
    typedef typename Pack<T, V>::type P;
    P t;
#pragma unroll
    for (int k = 0; k < V; ++k) t[k] = v[k];
    *reinterpret_cast<P *>(p) = t;
  }
}

// The same accesses for rows whose length is not a multiple of V elements (or
// whose base is not 16-byte aligned): the vector starts at an element-aligned
// address (legal for global memory, ~90 % of the aligned rate) and the row's last
// vector holds nval < V valid elements, moved one by one; what lies behind the row
// reads as zero and is never written.
template <typename T, int V>
__device__ __forceinline__ void ldv_rag(const T *p, T (&v)[V], int nval) {
  typedef T P __attribute__((ext_vector_type(V), aligned(sizeof(T))));
  if (nval >= V) {
    const P t = *reinterpret_cast<const P *>(p);
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = t[k];
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = k < nval ? p[k] : T(0);
  }
}

template <typename T, int V>
__device__ __forceinline__ void stv_rag(T *p, const T (&v)[V], int nval) {
  typedef T P __attribute__((ext_vector_type(V), aligned(sizeof(T))));
  if (nval >= V) {
    P t;
#pragma unroll
    for (int k = 0; k < V; ++k) t[k] = v[k];
    *reinterpret_cast<P *>(p) = t;
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (k < nval) p[k] = v[k];
  }
}

template <typename T, int V>
__device__ __forceinline__ void zero(T (&v)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = T(0);
}

// One term of the stopping rule's sums (nsol_pdc.hip): num += (new - old)^2 and
// den += new^2, formed in float64 from the stored values -- exact for float32
// inputs, so the float32 and float64 kernels add the same kind of summand and only
// the order of the sums differs between the forms.
template <typename T>
__device__ __forceinline__ void chk_add(double &num, double &den, T old_v, T new_v) {
  const double nv = (double)new_v;
  const double d = nv - (double)old_v;
  num += d * d;
  den += nv * nv;
}

template <typename T>
struct PdScalars {
  T sigma, hden, tau, tl, one_plus_tl, theta;
  int huber, l1, has_p;
};

// p_new = clamp((p_old + sigma * (hi*w + lo*(-w))) / hden)
template <typename T>
__device__ __forceinline__ T dual_update(T p_old, T hi, T lo, T w,
                                         const PdScalars<T> &S) {
  T q = p_old + S.sigma * (hi * w + lo * (-w));
  if (S.huber) {
    pin(q);            // a real (uniform) branch, not a speculated division
    q = huber_div(q, S.hden);
  }
  return dual_clamp(q);
}

// compile-time flags and an explicit step size (sigma may be masked to zero
// for voxels outside the volume, which makes the new dual exactly zero)
template <bool HUBER, typename T>
__device__ __forceinline__ T dual_update_s(T p_old, T hi, T lo, T w, T sigma,
                                           T hden) {
  T q = p_old + sigma * (hi * w + lo * (-w));
  if constexpr (HUBER) q = huber_div(q, hden);
  return dual_clamp(q);
}

// UNIT: all inverse spacings are exactly 1.  x*1 and x*(-1) are exact, so
// hi*1 + lo*(-1) == hi - lo and p*(-1) + pl*1 == pl - p bit for bit: the
// multiplications can be dropped without changing a single result.
template <bool HUBER, bool UNIT, typename T>
__device__ __forceinline__ T dual_update_u(T p_old, T hi, T lo, T w, T sigma, T hden) {
  const T g = UNIT ? hi - lo : hi * w + lo * (-w);
  T q = p_old + sigma * g;
  if constexpr (HUBER) q = huber_div(q, hden);
  return dual_clamp(q);
}
// one axis of K^T p: p*(-w) + p_prev*w
template <bool UNIT, typename T>
__device__ __forceinline__ T adj_term(T p, T p_prev, T w) {
  return UNIT ? p_prev - p : p * (-w) + p_prev * w;
}

// The knobs of nsol_pd.hip that shape a one-iteration launch (nsol_pd_launch.hpp),
// handed on to the isotropic launcher of nsol_pdi.hip.
struct PdLaunchTune {
  int zchunk, ry, xcd_map, rag;
};
// the knobs as they stand (nsol_pd.hip), for the checking kernel of nsol_pdc.hip
PdLaunchTune pd_current_tune();
// What nsol_pd.hip's entries call in the other units; each is instantiated for
// float and double where it is defined.
// One iteration through k_pd_fused_iso / the isotropic dual step of the two-pass
// form (nsol_pdi.hip); arguments as nsol_pd_fused_iter_* / nsol_pd_dual_step_*.
template <typename T>
int pd_iso_fused_iter(const T *xbar_in, T *xbar_out, T *x, const T *bt, const T *p_in,
                      T *p_out, int ndim, int64_t nz, int64_t ny, int64_t nx, double wx,
                      double wy, double wz, double sigma, double hden, double tau,
                      double tl, double theta, int flags, void *stream, int64_t pitch,
                      PdLaunchTune tune);
template <typename T>
int pd_iso_dual_step(const T *xbar, const T *p_in, T *p_out, int ndim, int64_t nz,
                     int64_t ny, int64_t nx, double wx, double wy, double wz,
                     double sigma, double hden, void *stream);
// Two iterations through k_pd_fused2 (nsol_pd2.hip), k = 2 or 3 through k_pd_fusedk
// (nsol_pdk.hip; pitch > nx: rows at that pitch); arguments as nsol_pd_fused2_iter_* /
// nsol_pd_fusedk_iter_pitched_*.  -2: the kernel does not apply, nothing was launched.
template <typename T>
int pd_fused2_iter(const T *xbar_in, T *xbar_out, const T *x_in, T *x_out, const T *bt,
                   const T *p_in, T *p_out, int ndim, int64_t nz, int64_t ny, int64_t nx,
                   double wx, double wy, double wz, const double *sigma,
                   const double *hden, const double *tau, const double *tl,
                   const double *theta, int flags, void *stream);
template <typename T>
int pd_fusedk_iter(const T *xbar_in, T *xbar_out, const T *x_in, T *x_out, const T *bt,
                   const T *p_in, T *p_out, int ndim, int64_t nz, int64_t ny, int64_t nx,
                   double wx, double wy, double wz, int k, const double *sigma,
                   const double *hden, const double *tau, const double *tl,
                   const double *theta, int flags, void *stream, int64_t pitch);

// The shifted depth-3 form (k_pd_shift3, nsol_pdk.hip): a launch runs P D P D P D on
// (x, p) alone -- no xbar crosses it.  pd_shift3_min_iters: the shortest run of this
// problem that takes a block of such launches (0: none does, or `iterations` is below the
// threshold of any shape); pd_shift3_iter: one launch
// (sigma, hden: iterations n .. n+3, the first unused; tau, tl, theta: n .. n+2).
template <typename T>
int pd_shift3_min_iters(const T *x, const T *x_alt, const T *bt, const T *p0, const T *p1,
                        int ndim, int64_t nz, int64_t ny, int64_t nx, int flags,
                        int64_t pitch, int iterations);
// launches a long run of this shape gives up for the unshifted depth-3 plan's exploration
template <typename T>
int pd_shift3_donation(int64_t nz, int64_t ny, int64_t nx);
template <typename T>
int pd_shift3_iter(const T *x_in, T *x_out, const T *bt, const T *p_in, T *p_out, int ndim,
                   int64_t nz, int64_t ny, int64_t nx, double wx, double wy, double wz,
                   const double *sigma, const double *hden, const double *tau,
                   const double *tl, const double *theta, int flags, void *stream);

template <bool L1, typename T>
__device__ __forceinline__ T prox_data_s(T u, T bt, T tl, T one_plus_tl) {
  if constexpr (L1) return prox_ell1(u, bt, tl);
  else return prox_ell2(u, bt, tl, one_plus_tl);
}

}  // namespace nsol
