// lk_residual.hpp - the arithmetic that the photometry pass and the residual map share with the host (include/lk_engine.h:
// lk_photometry, lk_photometry_from_sums, lk_residual_map, lk_map_owner).  One function for the kernel (lk_residual.hip) and
// the host entry point, like lk_uncertainty.hpp: a record is this function of its sector's eight sums, and a pixel's owner is
// decided by these two comparisons, whoever evaluates them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"

constexpr int kLkPhotoSums = 8;        // sum f, sum g, sum f^2, sum g^2, sum f g, sum V^2, flagged samples, max |V|
constexpr double kLkPhotoFlat = 1e-12; // FLAT: N sum x^2 - (sum x)^2 <= this times N sum x^2
constexpr int kLkMapCapacity = 512;    // candidates a pixel tile keeps in LDS

__host__ __device__ inline void lk_photometry_clear(struct lk_photometry *out, int n, int status) {
  out->n_points = n;
  out->status = status;
  out->mean_f = out->mean_g = out->std_f = out->std_g = out->zncc = out->gain = out->offset = 0.f;
  out->rms = out->rms_zn = out->znssd = out->max_abs = 0.f;
  out->reserved[0] = out->reserved[1] = out->reserved[2] = 0;
}

// sums: kLkPhotoSums doubles of one evaluated sector of n samples.  All in double without fused multiply-add, every output
// rounded to float once.  Writes the whole record: LK_PHOTO_OK, _OUT_OF_IMAGE (a flagged sample), _TOO_FEW or _FLAT.
__host__ __device__ inline void lk_photometry_record(int n, const double *sums, struct lk_photometry *out) {
  if (sums[6] != 0.0) {
    lk_photometry_clear(out, n, LK_PHOTO_OUT_OF_IMAGE);
    return;
  }
  if (n < 2) {
    lk_photometry_clear(out, n, LK_PHOTO_TOO_FEW);
    return;
  }
  lk_photometry_clear(out, n, LK_PHOTO_OK);
  const double N = (double)n;
  const double Sf = sums[0], Sg = sums[1], Sff = sums[2], Sgg = sums[3], Sfg = sums[4], SVV = sums[5];
  const double mf = Sf / N, mg = Sg / N;
  const double qf = N * Sff, qg = N * Sgg;
  const double vf = qf - Sf * Sf, vg = qg - Sg * Sg, c = N * Sfg - Sf * Sg;
  out->mean_f = (float)mf;
  out->mean_g = (float)mg;
  out->std_f = (float)(sqrt(vf > 0.0 ? vf : 0.0) / N);
  out->std_g = (float)(sqrt(vg > 0.0 ? vg : 0.0) / N);
  out->rms = (float)sqrt(SVV / N);
  out->max_abs = (float)sums[7];
  if (!(vf > kLkPhotoFlat * qf) || !(vg > kLkPhotoFlat * qg)) { // (also: not a number)
    out->status = LK_PHOTO_FLAT;
    return;
  }
  const double z = c / sqrt(vf * vg);
  const double gain = c / vf;
  const double rest = 1.0 - z * z;
  out->zncc = (float)z;
  out->gain = (float)gain;
  out->offset = (float)(mg - gain * mf);
  out->rms_zn = (float)(sqrt(vg) / N * sqrt(rest > 0.0 ? rest : 0.0));
  out->znssd = (float)(2.0 * (1.0 - z));
}

// ---- the owner rule of the residual map ------------------------------------------------------------------------------------
// squared distance of the level-0 position (X, Y) from a float centre: rounded squares, one rounded sum
__host__ __device__ inline double lk_map_d2(float cx, float cy, double X, double Y) {
  const double dx = (double)cx - X, dy = (double)cy - Y;
  const double xx = dx * dx, yy = dy * dy;
  return xx + yy;
}
// does candidate (d2, index) replace the best so far (best < 0: none yet)?  The caller has checked d2 <= r2 (false for the
// NaN of a sector that is not good).  The pair is compared: candidates arrive in ascending order only inside one cell.
__host__ __device__ inline bool lk_map_better(double d2, int index, double best_d2, int best) {
  return best < 0 || d2 < best_d2 || (d2 == best_d2 && index < best);
}

inline int lk_map_owner_impl(int n, const float *centers_xy, const uint8_t *good, double X, double Y, double radius) {
  const double r2 = radius * radius;
  int best = -1;
  double best_d2 = 0.0;
  for (int s = 0; s < n; ++s) {
    if (good && !good[s])
      continue;
    const double d2 = lk_map_d2(centers_xy[2 * s], centers_xy[2 * s + 1], X, Y);
    if (d2 <= r2 && lk_map_better(d2, s, best_d2, best)) {
      best = s;
      best_d2 = d2;
    }
  }
  return best;
}
