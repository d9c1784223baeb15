// lk_znssd.hpp - from the sums of one evaluation to the criterion and the damped step of the ZNSSD refinement
// (include/lk_engine.h: lk_refine_znssd, lk_znssd_step_from_sums).  One function for the kernel
// (lk_znssd.hip) and the host entry point, like lk_uncertainty.hpp: criterion and step are this function of a sector's sums,
// whoever computes them.  All in double without fused multiply-add.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"
#include "lk_residual.hpp"    // kLkPhotoFlat: the FLAT rule is photometry's
#include "lk_uncertainty.hpp" // kLkUncMinPivot: the pivot rule is the uncertainty pass's

constexpr int kLkZnSums = 45; // the sums of the six-parameter model; a smaller model's come first, zeros behind them

// the layout of a model's sums: Sf, Sg, Sff, Sgg, Sfg | SH[P] | SHH[P (P + 1) / 2] upper triangle row-major | SHf[P] | SHg[P] |
// the samples the sampler flagged
template <int P> struct LkZnLayout {
  static constexpr int NA = P * (P + 1) / 2;
  static constexpr int H = 5, HH = H + P, HF = HH + NA, HG = HF + P, FLAGGED = HG + P, N = FLAGGED + 1;
};
static_assert(LkZnLayout<6>::N == kLkZnSums, "the six-parameter model fills the sums");

struct LkZnCriterion {
  double crit, gain, offset, zncc;
};

// The criterion of n samples of total weight N with these sums: 0, or the status that refuses them (LK_ZN_TOO_FEW, LK_ZN_FLAT
// - all four numbers 0 - or LK_ZN_NEGATIVE, all four numbers filled).  n counts the samples that take part (the too-few
// test); N stands where the unweighted formulas have (double)n: the sum of the weights (lk_refine_weighted, DESIGN.md
// section 26).
template <int P> __host__ __device__ inline int lk_znssd_criterion(int n, double N, const double *sums, LkZnCriterion *out) {
  out->crit = out->gain = out->offset = out->zncc = 0.0;
  if (n < P + 2)
    return LK_ZN_TOO_FEW;
  const double Sf = sums[0], Sg = sums[1], Sff = sums[2], Sgg = sums[3], Sfg = sums[4];
  const double qf = N * Sff, qg = N * Sgg;
  const double vf = qf - Sf * Sf, vg = qg - Sg * Sg, c = N * Sfg - Sf * Sg;
  if (!(vf > kLkPhotoFlat * qf) || !(vg > kLkPhotoFlat * qg)) // (also: not a number)
    return LK_ZN_FLAT;
  const double vv = vf * vg;
  const double gain = c / vg;
  const double rest = 1.0 - c * c / vv;
  out->gain = gain;
  out->offset = (Sf - gain * Sg) / N;
  out->zncc = c / sqrt(vv);
  out->crit = rest > 0.0 ? rest : 0.0;
  return c > 0.0 ? 0 : LK_ZN_NEGATIVE;
}
// unit weights: N = n
template <int P> __host__ __device__ inline int lk_znssd_criterion(int n, const double *sums, LkZnCriterion *out) {
  return lk_znssd_criterion<P>(n, (double)n, sums, out);
}

// The criterion, and the Gauss-Newton step of ZNSSD with gain and offset eliminated, damped by lambda:
//   A_kl = gain^2 (SHH_kl - SH_k SH_l / N) / N,  b_k = gain ((SHf_k - SH_k Sf / N) - gain (SHg_k - SH_k Sg / N)) / N,
//   diag(A) (1 + lambda), A delta = b.
// A is scaled to C = A_kl / sqrt(A_kk A_ll) - a diagonal of 1 + lambda - and factored as L D L^T without pivoting; a diagonal
// entry of A that is not positive, or a pivot of C that is not above kLkUncMinPivot, gives LK_ZN_SINGULAR (delta zeros, the
// criterion filled).  Returns 0 or the refusing status.  Fully unrolled: every index is a compile-time constant on the device.
// n and N as for the criterion.
template <int P>
__host__ __device__ inline int lk_znssd_step(int n, double N, const double *sums, double lambda, double *delta, LkZnCriterion *cr) {
  using Y = LkZnLayout<P>;
#pragma unroll
  for (int k = 0; k < P; ++k)
    delta[k] = 0.0;
  const int refused = lk_znssd_criterion<P>(n, N, sums, cr);
  if (refused != 0)
    return refused;
  const double gain = cr->gain, Sf = sums[0], Sg = sums[1];
  const double gg = gain * gain;
  double A[P][P], b[P], root[P];
  {
    int idx = 0;
#pragma unroll
    for (int k = 0; k < P; ++k)
#pragma unroll
      for (int l = k; l < P; ++l) {
        A[k][l] = A[l][k] = gg * (sums[Y::HH + idx] - sums[Y::H + k] * sums[Y::H + l] / N) / N;
        ++idx;
      }
  }
  bool singular = false;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const double hf = sums[Y::HF + k] - sums[Y::H + k] * Sf / N, hg = sums[Y::HG + k] - sums[Y::H + k] * Sg / N;
    b[k] = gain * (hf - gain * hg) / N;
    singular = singular || !(A[k][k] > 0.0); // (no variation along this parameter, or not a number)
    root[k] = sqrt(A[k][k]);
  }
  if (singular)
    return LK_ZN_SINGULAR;
  const double damp = 1.0 + lambda;
  double L[P][P], D[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    double d = damp;
#pragma unroll
    for (int k = 0; k < j; ++k)
      d = d - L[j][k] * L[j][k] * D[k];
    D[j] = d;
    singular = singular || !(d > kLkUncMinPivot);
#pragma unroll
    for (int i = j + 1; i < P; ++i) {
      double t = A[i][j] / (root[i] * root[j]);
#pragma unroll
      for (int k = 0; k < j; ++k)
        t = t - L[i][k] * L[j][k] * D[k];
      L[i][j] = t / d;
    }
  }
  if (singular)
    return LK_ZN_SINGULAR;
  // L z = b / root, D w = z, L^T y = w, delta = y / root
  double y[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double t = b[i] / root[i];
#pragma unroll
    for (int k = 0; k < i; ++k)
      t = t - L[i][k] * y[k];
    y[i] = t;
  }
#pragma unroll
  for (int i = 0; i < P; ++i)
    y[i] = y[i] / D[i];
#pragma unroll
  for (int i = P - 1; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int k = i + 1; k < P; ++k)
      t = t - L[k][i] * y[k];
    y[i] = t;
  }
#pragma unroll
  for (int i = 0; i < P; ++i)
    delta[i] = y[i] / root[i];
  return 0;
}
// unit weights: N = n
template <int P>
__host__ __device__ inline int lk_znssd_step(int n, const double *sums, double lambda, double *delta, LkZnCriterion *cr) {
  return lk_znssd_step<P>(n, (double)n, sums, lambda, delta, cr);
}

// the weight of parameter k of a model with P parameters in the convergence test: 1 for the translations, the half-width of
// a square subset of n samples for the gradient terms and the rotation (never below 1)
__host__ __device__ inline double lk_znssd_weight(int k, int P, int n) {
  if (k < (P == 1 ? 1 : 2))
    return 1.0;
  const double half = sqrt((double)n) / 2.0;
  return half > 1.0 ? half : 1.0;
}

// Returns -1 for an unknown model (outputs untouched), else the status of lk_znssd_step; delta: 6 doubles, zeros behind P.
inline int lk_znssd_step_from_sums_impl(int model, int n, double N, const double *sums, double lambda, double *delta6,
                                        LkZnCriterion *cr) {
  if (model != LK_FM_U && model != LK_FM_UV && model != LK_FM_UVQ && model != LK_FM_UVUXUYVXVY)
    return -1;
  for (int k = 0; k < 6; ++k)
    delta6[k] = 0.0;
  switch (model) {
  case LK_FM_U: return lk_znssd_step<1>(n, N, sums, lambda, delta6, cr);
  case LK_FM_UV: return lk_znssd_step<2>(n, N, sums, lambda, delta6, cr);
  case LK_FM_UVQ: return lk_znssd_step<3>(n, N, sums, lambda, delta6, cr);
  case LK_FM_UVUXUYVXVY: return lk_znssd_step<6>(n, N, sums, lambda, delta6, cr);
  default: return -1;
  }
}
inline int lk_znssd_step_from_sums_impl(int model, int n, const double *sums, double lambda, double *delta6, LkZnCriterion *cr) {
  return lk_znssd_step_from_sums_impl(model, n, (double)n, sums, lambda, delta6, cr);
}
