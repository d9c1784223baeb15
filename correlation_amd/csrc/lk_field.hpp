// lk_field.hpp - the fit of one node of the field map (include/lk_engine.h: lk_field_map, lk_field_from_sums).  One function
// for the kernel (lk_field.hip) and the host entry point, like lk_track.hpp: a node's status and its twelve floats are this
// function of the window's count, weight sum and weighted sums, whoever computes them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"
#include "lk_strain.hpp"
#include "lk_track.hpp"

constexpr int kLkFieldCapacity = 1024; // candidates a tile of nodes keeps in LDS, 16 bytes each
constexpr int kLkFieldChannels = 15;   // u, v, ux, uy, vx, vy, exx, eyy, exy, e1, e2, theta, X0, Y0, MISFIT
constexpr int kLkFieldMaxIterations = 16;

// The weight of a member at squared distance d2 <= r2 (both double).  BISQUARE: (1 - d2 / r2)^2, each operation rounded;
// a member on the rim has weight 0 and still counts.
__host__ __device__ inline double lk_field_weight(int weight, double d2, double r2) {
  if (weight != LK_FIELD_BISQUARE)
    return 1.0;
  const double t = 1.0 - d2 / r2;
  return t * t;
}

// Count, weight sum and the eleven weighted sums of a window in coordinates relative to its position, in lk_plane_fit's
// layout.  With w = 1 every term has PlaneSums::add's bits (lk_neighbours.hpp): w x is x.
struct LkFieldSums {
  double s[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv
  double W = 0;
  int n = 0;
  __host__ __device__ inline void add(double w, double x, double y, double u, double v) {
    const double wx = w * x, wy = w * y;
    W += w;
    s[0] += wx;
    s[1] += wy;
    s[2] += wx * x;
    s[3] += wx * y;
    s[4] += wy * y;
    s[5] += w * u;
    s[6] += wx * u;
    s[7] += wy * u;
    s[8] += w * v;
    s[9] += wx * v;
    s[10] += wy * v;
    ++n;
  }
};

// Status of a window and, where it is LK_FIELD_OK, its planes (lk_plane_fit's formulas with n replaced by W): the rules of
// lk_track_step_impl on the weighted moments, checked in this order.
__host__ __device__ inline int lk_field_fit(int min_neighbours, int n, double W, const double *sums11, LkPlaneFit *pf) {
  if (n < min_neighbours)
    return LK_FIELD_TOO_FEW;
  if (!(W > 0.0))
    return LK_FIELD_DEGENERATE;
  *pf = lk_plane_fit_w(W, sums11);
  const double Sxx = sums11[2], Syy = sums11[4];
  if (pf->CC == 0.0 || !(pf->Cxx > kLkTrackNoise * Sxx) || !(pf->Cyy > kLkTrackNoise * Syy) || !(pf->D > 1e-6 * pf->CC))
    return LK_FIELD_DEGENERATE;
  return LK_FIELD_OK;
}

// out12 = {u, v, ux, uy, vx, vy, exx, eyy, exy, e1, e2, theta} of a fitted plane: each coefficient rounded to float once,
// the tensor of the four float gradients.
__host__ __device__ inline void lk_field_values(const LkPlaneFit &pf, int tensor, float *out12) {
  out12[0] = (float)pf.u0, out12[1] = (float)pf.v0;
  out12[2] = (float)pf.ux, out12[3] = (float)pf.uy, out12[4] = (float)pf.vx, out12[5] = (float)pf.vy;
  (void)lk_strain_tensor_impl(tensor, out12 + 2, out12 + 6);
}

// the two together; a window without a fit has NaN in all twelve
__host__ __device__ inline int lk_field_from_sums_impl(int min_neighbours, int n, double W, const double *sums11, int tensor,
                                                       float *out12) {
  LkPlaneFit pf;
  const int status = lk_field_fit(min_neighbours, n, W, sums11, &pf);
  if (status == LK_FIELD_OK) {
    lk_field_values(pf, tensor, out12);
  } else {
    for (int i = 0; i < 12; ++i)
      out12[i] = NAN;
  }
  return status;
}
