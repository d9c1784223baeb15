// lk_strain.hpp - the windowed plane fit and the strain tensor of a displacement gradient (include/lk_engine.h:
// lk_strain_field, lk_strain_from_gradient).  One function each for the kernels (lk_strain.hip, lk_outlier.hip, lk_track.hip
// through lk_track.hpp) and the host entry points, like lk_compose.hpp: the plane is this function of a window's count and
// sums, the record's six tensor fields are this function of its four gradient fields, whoever computes them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"

// The least-squares planes u(x, y) = u0 + ux x + uy y and v(x, y) = v0 + vx x + vy y of a window of n centres, from
// sums11 = {Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv} in the window's coordinates: the centred moments and the 2 x 2
// solve, all in double, each product, quotient and difference rounded to double in the order written.  Which windows have
// a plane (enough centres, CC != 0, D large enough against CC, ...) is the caller's rule: the coefficients of a window that
// fails it are whatever the divisions give and are not to be read.
struct LkPlaneFit {
  double Cxx, Cxy, Cyy, CC, D; // moments of the centres, Cxx Cyy, the determinant
  double ux, uy, vx, vy, u0, v0;
};
// lk_plane_fit_w is the same fit of a weighted window (lk_field.hpp): n = the sum of the weights, the sums weighted alike.
__host__ __device__ inline LkPlaneFit lk_plane_fit_w(double n, const double *sums11) {
  const double Sx = sums11[0], Sy = sums11[1], Sxx = sums11[2], Sxy = sums11[3], Syy = sums11[4], Su = sums11[5];
  const double Sxu = sums11[6], Syu = sums11[7], Sv = sums11[8], Sxv = sums11[9], Syv = sums11[10];
  const double Cxx = Sxx - Sx * Sx / n, Cxy = Sxy - Sx * Sy / n, Cyy = Syy - Sy * Sy / n;
  const double Cxu = Sxu - Sx * Su / n, Cyu = Syu - Sy * Su / n, Cxv = Sxv - Sx * Sv / n, Cyv = Syv - Sy * Sv / n;
  const double CC = Cxx * Cyy, D = CC - Cxy * Cxy;
  LkPlaneFit f;
  f.Cxx = Cxx, f.Cxy = Cxy, f.Cyy = Cyy, f.CC = CC, f.D = D;
  f.ux = (Cyy * Cxu - Cxy * Cyu) / D, f.uy = (Cxx * Cyu - Cxy * Cxu) / D;
  f.vx = (Cyy * Cxv - Cxy * Cyv) / D, f.vy = (Cxx * Cyv - Cxy * Cxv) / D;
  f.u0 = Su / n - f.ux * (Sx / n) - f.uy * (Sy / n), f.v0 = Sv / n - f.vx * (Sx / n) - f.vy * (Sy / n);
  return f;
}
__host__ __device__ inline LkPlaneFit lk_plane_fit(int count, const double *sums11) { return lk_plane_fit_w((double)count, sums11); }

// grad4 = {ux, uy, vx, vy} as stored (float); out6 = {exx, eyy, exy, e1, e2, theta}.  Computed in double, each result
// rounded to float once.  Returns 1 for an unknown tensor (out6 untouched), else 0.
__host__ __device__ inline int lk_strain_tensor_impl(int tensor, const float *grad4, float *out6) {
  if (tensor != LK_STRAIN_GREEN_LAGRANGE && tensor != LK_STRAIN_SMALL)
    return 1;
  const double ux = (double)grad4[0], uy = (double)grad4[1], vx = (double)grad4[2], vy = (double)grad4[3];
  double exx = ux, eyy = vy, exy = 0.5 * (uy + vx);
  if (tensor == LK_STRAIN_GREEN_LAGRANGE) {
    exx = ux + 0.5 * (ux * ux + vx * vx);
    eyy = vy + 0.5 * (uy * uy + vy * vy);
    exy = exy + 0.5 * (ux * uy + vx * vy);
  }
  const double mean = (exx + eyy) * 0.5, half = (exx - eyy) * 0.5;
  const double rad = sqrt(half * half + exy * exy);
  out6[0] = (float)exx;
  out6[1] = (float)eyy;
  out6[2] = (float)exy;
  out6[3] = (float)(mean + rad);
  out6[4] = (float)(mean - rad);
  out6[5] = (float)(0.5 * atan2(2.0 * exy, exx - eyy));
  return 0;
}
