// lk_pattern.hpp - the arithmetic that the speckle-quality pass shares with the host (include/lk_engine.h: lk_pattern_quality,
// lk_pattern_from_sums, lk_suggest_subset).  One function for the kernel (lk_pattern.hip) and the host entry point, like
// lk_residual.hpp: a sector's record is this function of its nine integer sums and its one double sum, and a point's record
// is lk_subset_fill of the box sums the table gave, whoever evaluates them.
//
// Shared definitions.  Pixels are I(x, y) of the level-L image, u8 taken as integers.  The doubled central differences use
// clamped neighbours: gx2 = I(min(x + 1, cols - 1), y) - I(max(x - 1, 0), y), gy2 alike in y; the gradient is gx2 / 2, so
// every sum is an integer: Gxx = sum gx2^2, Gyy = sum gy2^2, Gxy = sum gx2 gy2, and SSSIG_x = Gxx / 4, SSSIG_y = Gyy / 4.
//
// The summed-area tables of gx2^2 and gy2^2 are uint32 and wrap: a candidate box is at most 257 x 257 pixels
// (LK_PATTERN_MAX_HALF = 128) of at most 255^2 each, 4 294 836 225 < 2^32 in all, so the four-corner difference modulo 2^32
// is the exact box sum although the table itself wraps many times over a large image.  Half the footprint and traffic of
// 64-bit tables.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lk_engine.h"

constexpr int kLkPatternSums = 9;          // sum I, sum I^2, Gxx, Gyy, Gxy, n_low, n_high, min I, max I
constexpr double kLkPatternAperture = 1e-6; // APERTURE: Gxx Gyy - Gxy^2 <= this times Gxx Gyy (the strain pass's degenerate rule)
static_assert(257ull * 257ull * 255ull * 255ull < (1ull << 32), "a clipped box of half-width LK_PATTERN_MAX_HALF fits a wrapped uint32");
static_assert(LK_PATTERN_MAX_HALF == 128, "the box-sum bound above is that of 257 x 257 pixels");

__host__ __device__ inline void lk_pattern_clear(struct lk_pattern *out, int n, int status) {
  out->n_points = n;
  out->status = status;
  out->mean = out->std = 0.f;
  out->grey_min = out->grey_max = 0;
  out->frac_low = out->frac_high = out->sssig_x = out->sssig_y = out->mig = 0.f;
  out->sigma_u = out->sigma_v = out->sigma_major = out->theta = 0.f;
  out->reserved = 0;
}

// sums: kLkPatternSums integers of one sector of n samples; mig_sum: sum sqrt(gx2^2 + gy2^2).  The sums are converted to
// double first (Gxx Gyy overflows int64 for giant sectors); all in double without fused multiply-add, every output rounded
// to float once.  Writes the whole record: LK_PATTERN_OK, _TOO_FEW (everything but n_points 0), _FLAT, _APERTURE (the four
// sigma fields and theta 0) or _SATURATED.
__host__ __device__ inline void lk_pattern_record(int n, const int64_t *sums, double mig_sum, float noise_sigma, float max_saturated,
                                                  struct lk_pattern *out) {
  if (n < 2) {
    lk_pattern_clear(out, n, LK_PATTERN_TOO_FEW);
    return;
  }
  lk_pattern_clear(out, n, LK_PATTERN_OK);
  const double N = (double)n;
  const double S1 = (double)sums[0], S2 = (double)sums[1], Gxx = (double)sums[2], Gyy = (double)sums[3], Gxy = (double)sums[4];
  const double low = (double)sums[5], high = (double)sums[6];
  const double q = N * S2, ss = S1 * S1;
  const double var = q - ss;
  out->mean = (float)(S1 / N);
  out->std = (float)(sqrt(var > 0.0 ? var : 0.0) / N);
  out->grey_min = (int32_t)sums[7];
  out->grey_max = (int32_t)sums[8];
  out->frac_low = (float)(low / N);
  out->frac_high = (float)(high / N);
  out->sssig_x = (float)(Gxx / 4.0);
  out->sssig_y = (float)(Gyy / 4.0);
  out->mig = (float)(mig_sum / (2.0 * N));
  if (sums[2] + sums[3] == 0) {
    out->status = LK_PATTERN_FLAT;
    return;
  }
  const double prod = Gxx * Gyy, cross = Gxy * Gxy;
  const double det = prod - cross;
  if (!(det > kLkPatternAperture * prod)) { // (also: one of Gxx, Gyy is 0)
    out->status = LK_PATTERN_APERTURE;
    return;
  }
  // Cov = 2 sigma^2 G^-1, G = the structure tensor in gradient units (the sums / 4): noise in both images
  const double sg = noise_sigma > 0.f ? (double)noise_sigma : 1.0;
  const double s2 = sg * sg;
  const double c00 = s2 * (8.0 * Gyy / det), c11 = s2 * (8.0 * Gxx / det), c01 = s2 * (-8.0 * Gxy / det);
  out->sigma_u = (float)(sg * sqrt(8.0 * Gyy / det));
  out->sigma_v = (float)(sg * sqrt(8.0 * Gxx / det));
  // principal value and angle by the formulas of lk_uncertainty.hpp
  const double mean = (c00 + c11) * 0.5, half = (c00 - c11) * 0.5;
  const double rad = sqrt(half * half + c01 * c01);
  out->sigma_major = (float)sqrt(mean + rad);
  out->theta = (float)(0.5 * atan2(2.0 * c01, c00 - c11));
  if (low + high > (double)max_saturated * N)
    out->status = LK_PATTERN_SATURATED;
}

// ---- lk_suggest_subset ------------------------------------------------------------------------------------------------------
// the node of a float position along one axis of `size` pixels: (int)(q + 0.5f) where that lies in 0 .. size - 1, else -1 (a
// position that is not finite included); the comparison is made on the float, so that no conversion overflows
__host__ __device__ inline int lk_subset_node(float q, int size) {
  const float f = q + 0.5f;
  return f > -1.f && f < (float)size ? (int)f : -1;
}

// T = ceil(4 sssig_min) as an integer in 1 .. 2^32 - 1, or 0 for a threshold that is refused
inline uint32_t lk_subset_threshold(float sssig_min) {
  if (!isfinite(sssig_min) || !(sssig_min > 0.f))
    return 0;
  const double t = ceil(4.0 * (double)sssig_min);
  return t <= 4294967295.0 ? (uint32_t)t : 0;
}

// the record of a point whose reported box (half-width `half` about the node, n_pixels after clipping) has the sums gxx, gyy
__host__ __device__ inline void lk_subset_fill(struct lk_subset *out, int half, int status, int n_pixels, int clipped, uint32_t gxx,
                                               uint32_t gyy, float noise_sigma) {
  const double sg = noise_sigma > 0.f ? (double)noise_sigma : 1.0;
  const double sx = (double)gxx / 4.0, sy = (double)gyy / 4.0;
  out->half = half;
  out->status = status;
  out->n_pixels = n_pixels;
  out->clipped = clipped;
  out->sssig_x = (float)sx;
  out->sssig_y = (float)sy;
  out->sigma_u = gxx ? (float)(sg * sqrt(2.0 / sx)) : 0.f; // Pan's formula; no gradient: 0
  out->sigma_v = gyy ? (float)(sg * sqrt(2.0 / sy)) : 0.f;
}
