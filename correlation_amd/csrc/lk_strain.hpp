// lk_strain.hpp - the strain tensor of a displacement gradient (include/lk_engine.h: lk_strain_field,
// lk_strain_from_gradient).  One function for the kernel (lk_strain.hip) and the host entry point, like lk_compose.hpp:
// the record's six tensor fields are this function of its four gradient fields, whoever computes them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"

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
