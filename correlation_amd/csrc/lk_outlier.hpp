// lk_outlier.hpp - the selection and the ratio arithmetic of the outlier flags (include/lk_engine.h: lk_flag_outliers,
// lk_outlier_from_window).  One piece of code for the kernel (lk_outlier.hip) and the host entry point, like lk_strain.hpp
// and lk_uncertainty.hpp: what differs is only who counts - a lane group over its window, or one loop over an array.
//
// Selection: the k-th smallest of n floats is found on their order-preserving uint32 keys by bisection from the top bit
// down: the answer is the largest key T with |{key < T}| <= k, and that predicate is monotone in T, so each of the 32
// rounds fixes one bit with one count.  Nothing is sorted or stored; u and v share the rounds.  The second order statistic
// of an even n costs one more round: |{key <= x_k}| says whether x_(k+1) equals x_k, else it is the smallest key above x_k.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lk_engine.h"

// float -> key with a < b (as IEEE numbers) <=> key(a) < key(b); both zeros share +0's key
__host__ __device__ inline uint32_t lk_outlier_key(float f) {
  union {
    float f;
    uint32_t u;
  } c;
  c.f = f;
  uint32_t b = c.u;
  if (b == 0x80000000u)
    b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float lk_outlier_unkey(uint32_t k) {
  union {
    float f;
    uint32_t u;
  } c;
  c.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return c.f;
}
// the value a window member enters a selection with: e itself, or its distance from the median
__host__ __device__ inline float lk_outlier_value(float e, bool deviation, float med) {
  return deviation ? (float)fabs((double)e - (double)med) : e;
}

// The medians of both components.  Src is the window:
//   src.below(tu, tv, cu, cv)                 cu = |{key(u value) < tu}|, cv alike
//   src.above(xu, xv, cu, cv, mu, mv)         cu = |{key <= xu}|, mu = the smallest key > xu (0xffffffff if none), v alike
// median = (float)(((double)x[(n - 1) / 2] + (double)x[n / 2]) / 2) of the sorted values.
template <class Src> __host__ __device__ inline void lk_outlier_medians(Src &src, int n, float *med_u, float *med_v) {
  const int k = (n - 1) / 2;
  uint32_t pu = 0, pv = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t tu = pu | (1u << bit), tv = pv | (1u << bit);
    int cu, cv;
    src.below(tu, tv, cu, cv);
    if (cu <= k)
      pu = tu;
    if (cv <= k)
      pv = tv;
  }
  uint32_t qu = pu, qv = pv;
  if (n / 2 != k) {
    int cu, cv;
    uint32_t mu, mv;
    src.above(pu, pv, cu, cv, mu, mv);
    if (cu < k + 2)
      qu = mu;
    if (cv < k + 2)
      qv = mv;
  }
  *med_u = (float)(((double)lk_outlier_unkey(pu) + (double)lk_outlier_unkey(qu)) / 2.0);
  *med_v = (float)(((double)lk_outlier_unkey(pv) + (double)lk_outlier_unkey(qv)) / 2.0);
}

// ratio = (float)(|e_s - med| / (mad + eps)) per component, in double; flagged on the double values.  Fills the six float
// fields and the status (OK or FLAGGED) of *o.
__host__ __device__ inline void lk_outlier_ratios(float es_u, float es_v, float med_u, float med_v, float mad_u, float mad_v,
                                                  float eps, float threshold, lk_outlier *o) {
  const double ru = fabs((double)es_u - (double)med_u) / ((double)mad_u + (double)eps);
  const double rv = fabs((double)es_v - (double)med_v) / ((double)mad_v + (double)eps);
  o->med_u = med_u, o->med_v = med_v;
  o->mad_u = mad_u, o->mad_v = mad_v;
  o->ratio_u = (float)ru, o->ratio_v = (float)rv;
  o->status = (ru > rv ? ru : rv) > (double)threshold ? LK_OUTLIER_FLAGGED : LK_OUTLIER_OK;
}

// the window as two arrays (the host entry point)
struct LkOutlierArraySrc {
  const float *u, *v;
  int n;
  bool deviation;
  float med_u, med_v;
  __host__ __device__ void below(uint32_t tu, uint32_t tv, int &cu, int &cv) const {
    cu = cv = 0;
    for (int i = 0; i < n; ++i) {
      cu += lk_outlier_key(lk_outlier_value(u[i], deviation, med_u)) < tu ? 1 : 0;
      cv += lk_outlier_key(lk_outlier_value(v[i], deviation, med_v)) < tv ? 1 : 0;
    }
  }
  __host__ __device__ void above(uint32_t xu, uint32_t xv, int &cu, int &cv, uint32_t &mu, uint32_t &mv) const {
    cu = cv = 0;
    mu = mv = 0xffffffffu;
    for (int i = 0; i < n; ++i) {
      const uint32_t ku = lk_outlier_key(lk_outlier_value(u[i], deviation, med_u));
      const uint32_t kv = lk_outlier_key(lk_outlier_value(v[i], deviation, med_v));
      cu += ku <= xu ? 1 : 0;
      cv += kv <= xv ? 1 : 0;
      mu = ku > xu && ku < mu ? ku : mu;
      mv = kv > xv && kv < mv ? kv : mv;
    }
  }
};

// Returns 1 for n < 1 (out untouched), else 0.
__host__ __device__ inline int lk_outlier_from_window_impl(int n, const float *e_u, const float *e_v, float es_u, float es_v,
                                                           float eps, float threshold, lk_outlier *out) {
  if (n < 1)
    return 1;
  LkOutlierArraySrc src{e_u, e_v, n, false, 0.f, 0.f};
  float med_u, med_v, mad_u, mad_v;
  lk_outlier_medians(src, n, &med_u, &med_v);
  src.deviation = true;
  src.med_u = med_u, src.med_v = med_v;
  lk_outlier_medians(src, n, &mad_u, &mad_v);
  lk_outlier_ratios(es_u, es_v, med_u, med_v, mad_u, mad_v, eps, threshold, out);
  out->neighbours = n;
  return 0;
}
