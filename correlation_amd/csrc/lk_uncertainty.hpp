// lk_uncertainty.hpp - from the sums of one evaluation to the uncertainty record of a sector (include/lk_engine.h:
// lk_parameter_uncertainty, lk_uncertainty_from_sums).  One function for the kernel (lk_uncertainty.hip) and the host
// entry point, like lk_strain.hpp: a record is this function of its sector's 28 sums, whoever computes it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"

constexpr int kLkUncSums = 28;           // Sums<6>::N: the sums of every model, padded with zeros
constexpr double kLkUncMinPivot = 1e-10; // smallest pivot of the unit-diagonal C that is factored through

__host__ __device__ inline void lk_uncertainty_clear(lk_uncertainty *out, int n, int status) {
  for (int k = 0; k < 6; ++k)
    out->sigma[k] = 0.f;
  out->noise = out->rho_uv = out->sigma_major = out->sigma_minor = out->theta = out->sssig_x = out->sssig_y = 0.f;
  out->n_points = n;
  out->status = status;
  out->reserved = 0;
}

// sums = A (upper triangle, row-major), b, chi of P parameters (the layout of Sums<P>); n samples; level L of the evaluation.
// All in double without fused multiply-add, every output rounded to float once.  Writes the whole record: LK_UNC_OK,
// LK_UNC_TOO_FEW or LK_UNC_SINGULAR (zeros).  Fully unrolled: every index is a compile-time constant on the device.
template <int P> __host__ __device__ inline void lk_uncertainty_record(int n, const double *sums, int level, lk_uncertainty *out) {
  constexpr int NA = P * (P + 1) / 2;
  if (n <= P) {
    lk_uncertainty_clear(out, n, LK_UNC_TOO_FEW);
    return;
  }
  double A[P][P];
  {
    int idx = 0;
#pragma unroll
    for (int a = 0; a < P; ++a)
#pragma unroll
      for (int b = a; b < P; ++b)
        A[a][b] = A[b][a] = sums[idx++];
  }
  bool singular = false;
#pragma unroll
  for (int a = 0; a < P; ++a)
    singular = singular || !(A[a][a] > 0.0); // (a sum of squares: zero, or not a number)
  if (singular) {
    lk_uncertainty_clear(out, n, LK_UNC_SINGULAR);
    return;
  }
  // C = L D L^T, L unit lower triangular, no pivoting: C has a unit diagonal, so a pivot is scale-free
  double L[P][P], D[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    double d = 1.0;
#pragma unroll
    for (int k = 0; k < j; ++k)
      d = d - L[j][k] * L[j][k] * D[k];
    D[j] = d;
    singular = singular || !(d > kLkUncMinPivot);
#pragma unroll
    for (int i = j + 1; i < P; ++i) {
      double t = A[i][j] / sqrt(A[i][i] * A[j][j]);
#pragma unroll
      for (int k = 0; k < j; ++k)
        t = t - L[i][k] * L[j][k] * D[k];
      L[i][j] = t / d;
    }
  }
  if (singular) {
    lk_uncertainty_clear(out, n, LK_UNC_SINGULAR);
    return;
  }
  // M = L^-1 (unit lower), C^-1 = M^T D^-1 M
  double M[P][P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    M[j][j] = 1.0;
#pragma unroll
    for (int i = j + 1; i < P; ++i) {
      double t = L[i][j];
#pragma unroll
      for (int k = j + 1; k < i; ++k)
        t = t + L[i][k] * M[k][j];
      M[i][j] = -t;
    }
  }
  const double s2 = sums[NA + P] / (double)(n - P);
  auto cov = [&](int a, int b) { // a <= b
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k)
      if (k >= b)
        t = t + M[k][a] * M[k][b] / D[k];
    return s2 * t / sqrt(A[a][a] * A[b][b]);
  };
  const double up = (double)(1 << level); // u and v back to level-0 pixels
#pragma unroll
  for (int k = 0; k < 6; ++k)
    out->sigma[k] = k < P ? (float)(sqrt(cov(k, k)) * (k < 2 ? up : 1.0)) : 0.f;
  out->noise = (float)sqrt(s2);
  out->sssig_x = (float)(A[0][0] / (double)n);
  if constexpr (P >= 2) {
    const double c00 = cov(0, 0) * up * up, c01 = cov(0, 1) * up * up, c11 = cov(1, 1) * up * up;
    // principal values and angle by the formulas of lk_strain.hpp
    const double mean = (c00 + c11) * 0.5, half = (c00 - c11) * 0.5;
    const double rad = sqrt(half * half + c01 * c01);
    const double minor = mean - rad;
    out->rho_uv = (float)(c01 / sqrt(c00 * c11));
    out->sigma_major = (float)sqrt(mean + rad);
    out->sigma_minor = (float)sqrt(minor > 0.0 ? minor : 0.0);
    out->theta = (float)(0.5 * atan2(2.0 * c01, c00 - c11));
    out->sssig_y = (float)(A[1][1] / (double)n);
  } else {
    out->rho_uv = 0.f;
    out->sigma_major = out->sigma[0];
    out->sigma_minor = out->theta = out->sssig_y = 0.f;
  }
  out->n_points = n;
  out->status = LK_UNC_OK;
  out->reserved = 0;
}

// Returns 1 for an unknown model or level (out untouched), else 0.
__host__ __device__ inline int lk_uncertainty_from_sums_impl(int model, int n, const double *sums, int level, lk_uncertainty *out) {
  if (level < 0 || level >= LK_MAX_LEVELS)
    return 1;
  switch (model) {
  case LK_FM_U: lk_uncertainty_record<1>(n, sums, level, out); return 0;
  case LK_FM_UV: lk_uncertainty_record<2>(n, sums, level, out); return 0;
  case LK_FM_UVQ: lk_uncertainty_record<3>(n, sums, level, out); return 0;
  case LK_FM_UVUXUYVXVY: lk_uncertainty_record<6>(n, sums, level, out); return 0;
  default: return 1;
  }
}
