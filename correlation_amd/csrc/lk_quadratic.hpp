// lk_quadratic.hpp - from the sums of one evaluation to the criterion and the damped step of the second-order refinement
// (include/lk_engine.h: lk_refine_quadratic, lk_quadratic_step_from_sums).  One function for the kernel
// (lk_quadratic.hip) and the host entry point, like lk_znssd.hpp, whose criterion and formulas it applies to twelve
// parameters.  All in double without fused multiply-add.
//
// The sums use the moment structure of the model: every H is g_x or g_y times a monomial of (X, Y) = (dx, dy) of degree <= 2
// times 1 or 1/2, so SH, SHH, SHf and SHg of the twelve parameters are 87 moments times 1, 1/2 or 1/4 - not the 120 sums of a
// generic twelve-parameter layout.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"
#include "lk_znssd.hpp" // lk_znssd_criterion, LkZnCriterion; through it kLkPhotoFlat and kLkUncMinPivot

constexpr int kLkQdParams = 12; // u, v, ux, uy, vx, vy, uxx, uxy, uyy, vxx, vxy, vyy
constexpr int kLkQdSums = 88;
constexpr int kLkQdMono = 15;   // the monomials X^a Y^b, a + b <= 4, by degree, then by falling a
constexpr int kLkQdLow = 6;     // those of degree <= 2 come first

// the layout of the sums: Sf, Sg, Sff, Sgg, Sfg | sum w M[k] for w = gx gx, gx gy, gy gy (k = 0 .. 14 each) | sum t for
// t = gx M[k] (k = 0 .. 5), then t = gy M[k] | sum t f | sum t g | a spare, always 0 | the samples the sampler flagged
struct LkQdLayout {
  static constexpr int W = 5, T = W + 3 * kLkQdMono, TF = T + 2 * kLkQdLow, TG = TF + 2 * kLkQdLow, SPARE = TG + 2 * kLkQdLow,
                       FLAGGED = SPARE + 1, N = FLAGGED + 1;
};
static_assert(LkQdLayout::T == 50 && LkQdLayout::TF == 62 && LkQdLayout::TG == 74 && LkQdLayout::N == kLkQdSums, "the layout of the header");

// the index of X^a Y^b among the monomials
__host__ __device__ inline int lk_qd_mono(int a, int b) {
  const int d = a + b;
  return d * (d + 1) / 2 + b;
}

// parameter k: H_k = coef g_c X^a Y^b with c = 0 for g_x (the u terms) and 1 for g_y (the v terms)
__host__ __device__ inline void lk_qd_param(int k, int *c, int *a, int *b, double *coef) {
  *coef = 1.0;
  if (k < 2) {
    *c = k, *a = 0, *b = 0;
  } else if (k < 6) {
    *c = (k - 2) / 2, *b = (k - 2) & 1, *a = 1 - *b;
  } else {
    const int j = k - 6;
    *c = j / 3, *b = j % 3, *a = 2 - *b;
    *coef = *b == 1 ? 1.0 : 0.5;
  }
}

// what lk_quadratic_step works in besides its outputs: SH, b, root, D, y (12 each) and the lower triangle of A, then of the
// scaled matrix, then of L (78).  LDS next to the kept sums in the kernel, the stack on the host.
constexpr int kLkQdTri = kLkQdParams * (kLkQdParams + 1) / 2;
constexpr int kLkQdWork = 5 * kLkQdParams + kLkQdTri;

// The criterion (lk_znssd_criterion with P = 12: LK_ZN_TOO_FEW for n < 14) and the step of lk_znssd_step - the same A, b,
// scaling to a diagonal of 1 + lambda, unpivoted L D L^T and pivot rule - on the twelve parameters, whose SH, SHH, SHf, SHg
// are expanded from the 88 sums on the way.  Loops over `work` (kLkQdWork doubles) instead of lk_znssd_step's unrolled
// register arrays: twice 144 doubles do not fit into a lane's registers.  delta: 12 doubles, zeros unless 0 is returned.
// n and N as for lk_znssd_criterion: the samples that take part, and their total weight where the unweighted formulas have
// (double)n (lk_refine_composed).
__host__ __device__ inline int lk_quadratic_step(int n, double N, const double *sums, double lambda, double *delta, LkZnCriterion *cr,
                                                 double *work) {
  constexpr int P = kLkQdParams;
  using Y = LkQdLayout;
#pragma unroll 1
  for (int k = 0; k < P; ++k)
    delta[k] = 0.0;
  const int refused = lk_znssd_criterion<P>(n, N, sums, cr);
  if (refused != 0)
    return refused;
  const double gain = cr->gain, Sf = sums[0], Sg = sums[1];
  const double gg = gain * gain;
  double *SH = work, *b = SH + P, *root = b + P, *D = root + P, *y = D + P, *C = y + P; // C(i, j), j <= i, at i (i + 1) / 2 + j
  bool singular = false;
#pragma unroll 1
  for (int k = 0; k < P; ++k) {
    int c, ea, eb;
    double coef;
    lk_qd_param(k, &c, &ea, &eb, &coef);
    const int t = c * kLkQdLow + lk_qd_mono(ea, eb);
    const double sh = coef * sums[Y::T + t], shf = coef * sums[Y::TF + t], shg = coef * sums[Y::TG + t]; // (exact: 1 or 1/2)
    SH[k] = sh;
    const double hf = shf - sh * Sf / N, hg = shg - sh * Sg / N;
    b[k] = gain * (hf - gain * hg) / N;
  }
#pragma unroll 1
  for (int i = 0; i < P; ++i) {
    int ci, ai, bi;
    double fi;
    lk_qd_param(i, &ci, &ai, &bi, &fi);
#pragma unroll 1
    for (int j = 0; j <= i; ++j) {
      int cj, aj, bj;
      double fj;
      lk_qd_param(j, &cj, &aj, &bj, &fj);
      const double shh = (fi * fj) * sums[Y::W + (ci + cj) * kLkQdMono + lk_qd_mono(ai + aj, bi + bj)]; // (exact: 1, 1/2 or 1/4)
      C[i * (i + 1) / 2 + j] = gg * (shh - SH[j] * SH[i] / N) / N;
    }
    const double aii = C[i * (i + 1) / 2 + i];
    singular = singular || !(aii > 0.0); // (no variation along this parameter, or not a number)
    root[i] = sqrt(aii);
  }
  if (singular)
    return LK_ZN_SINGULAR;
  const double damp = 1.0 + lambda;
#pragma unroll 1
  for (int i = 0; i < P; ++i) {
#pragma unroll 1
    for (int j = 0; j < i; ++j)
      C[i * (i + 1) / 2 + j] = C[i * (i + 1) / 2 + j] / (root[i] * root[j]);
    C[i * (i + 1) / 2 + i] = damp;
  }
  // in place: column j of L replaces column j of the scaled matrix, which nothing reads afterwards
#pragma unroll 1
  for (int j = 0; j < P; ++j) {
    const double *Lj = C + j * (j + 1) / 2;
    double d = damp;
#pragma unroll 1
    for (int k = 0; k < j; ++k)
      d = d - Lj[k] * Lj[k] * D[k];
    D[j] = d;
    singular = singular || !(d > kLkUncMinPivot);
#pragma unroll 1
    for (int i = j + 1; i < P; ++i) {
      double *Li = C + i * (i + 1) / 2;
      double t = Li[j];
#pragma unroll 1
      for (int k = 0; k < j; ++k)
        t = t - Li[k] * Lj[k] * D[k];
      Li[j] = t / d;
    }
  }
  if (singular)
    return LK_ZN_SINGULAR;
  // L z = b / root, D w = z, L^T y = w, delta = y / root
#pragma unroll 1
  for (int i = 0; i < P; ++i) {
    const double *Li = C + i * (i + 1) / 2;
    double t = b[i] / root[i];
#pragma unroll 1
    for (int k = 0; k < i; ++k)
      t = t - Li[k] * y[k];
    y[i] = t;
  }
#pragma unroll 1
  for (int i = 0; i < P; ++i)
    y[i] = y[i] / D[i];
#pragma unroll 1
  for (int i = P - 1; i >= 0; --i) {
    double t = y[i];
#pragma unroll 1
    for (int k = i + 1; k < P; ++k)
      t = t - C[k * (k + 1) / 2 + i] * y[k];
    y[i] = t;
  }
#pragma unroll 1
  for (int i = 0; i < P; ++i)
    delta[i] = y[i] / root[i];
  return 0;
}
// unit weights: N = n
__host__ __device__ inline int lk_quadratic_step(int n, const double *sums, double lambda, double *delta, LkZnCriterion *cr, double *work) {
  return lk_quadratic_step(n, (double)n, sums, lambda, delta, cr, work);
}

// the weight of parameter k in the convergence test, with h = max(1, sqrt(n) / 2), the half-width of a square subset of n
// samples: 1 for the translations, h for the gradients, h^2 / 2 for uxx, uyy, vxx, vyy and h^2 for uxy, vxy - how far a
// unit of the parameter moves a sample at the rim
__host__ __device__ inline double lk_quadratic_weight(int k, int n) {
  if (k < 2)
    return 1.0;
  const double half = sqrt((double)n) / 2.0;
  const double h = half > 1.0 ? half : 1.0;
  if (k < 6)
    return h;
  const double hh = h * h;
  return k == 7 || k == 10 ? hh : hh / 2.0;
}

// the second-order displacement at the rim of a subset of n0 level-0 samples, in level-0 pixels (p: level-0 scale)
__host__ __device__ inline double lk_quadratic_bend(const float *p, int n0) {
  const double h0 = sqrt((double)n0) / 2.0;
  const double bu = (fabs((double)p[6]) / 2.0 + fabs((double)p[7])) + fabs((double)p[8]) / 2.0;
  const double bv = (fabs((double)p[9]) / 2.0 + fabs((double)p[10])) + fabs((double)p[11]) / 2.0;
  return (h0 * h0) * (bu > bv ? bu : bv);
}
