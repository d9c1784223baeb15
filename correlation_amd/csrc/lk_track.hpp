// lk_track.hpp - one frame of a tracked material point (include/lk_engine.h: lk_track_points, lk_track_step).  One
// function for the kernel (lk_track.hip) and the host entry point, like lk_strain.hpp: the state and the record of a
// (frame, point) are this function of the window's count and sums and of the state before, whoever computes them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"
#include "lk_strain.hpp"

// A centred moment that is at most this share of its raw sum is the rounding of that sum (2^-53 per term), not a spread of
// the centres: a row of centres seen from a position off their lattice has Cyy = Syy - Sy Sy / n of the order of 1e-16 Syy,
// not exactly 0 as at a sector centre, and D <= 1e-6 Cxx Cyy cannot catch it (both sides scale with that noise).
constexpr double kLkTrackNoise = 9.094947017729282e-13; // 2^-40

__host__ __device__ inline bool lk_track_finite(double v) { return v - v == 0.0; } // (false for a NaN and for an infinity)

// n: good sectors of the window; sums11 = {Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv} in the window's coordinates
// (relative to the position the fit is centred at: X, Y in TOTAL mode, the state's x, y in INCREMENTAL mode);
// state8 = {X, Y, x, y, Fxx, Fxy, Fyx, Fyy}, read and written.  All in double, each product and sum rounded to double;
// each output rounded to float once.  For every status but OK the float fields are 0 and the state's x, y and F become
// NaN (X and Y stay): an INCREMENTAL chain that meets such a state is LOST, a TOTAL one does not read it.
__host__ __device__ inline void lk_track_step_impl(int mode, int min_neighbours, int n, const double *sums11, double *state8,
                                                   int tensor, lk_track *out) {
  const double X = state8[0], Y = state8[1];
  const bool incremental = mode == LK_TRACK_INCREMENTAL;
  const double Sxx = sums11[2], Syy = sums11[4];
  const LkPlaneFit pf = lk_plane_fit(n, sums11);
  int status = LK_TRACK_OK;
  if (!lk_track_finite(X) || !lk_track_finite(Y))
    status = LK_TRACK_BAD_POINT;
  else if (incremental && !(lk_track_finite(state8[2]) && lk_track_finite(state8[3]) && lk_track_finite(state8[4]) &&
                            lk_track_finite(state8[5]) && lk_track_finite(state8[6]) && lk_track_finite(state8[7])))
    status = LK_TRACK_LOST;
  else if (n < min_neighbours)
    status = LK_TRACK_TOO_FEW;
  else if (pf.CC == 0.0 || !(pf.Cxx > kLkTrackNoise * Sxx) || !(pf.Cyy > kLkTrackNoise * Syy) || !(pf.D > 1e-6 * pf.CC))
    status = LK_TRACK_DEGENERATE;

  float f[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // u, v, ux, uy, vx, vy, exx .. theta
  float px = 0.f, py = 0.f;
  if (status == LK_TRACK_OK) {
    const double gux = pf.ux, guy = pf.uy, gvx = pf.vx, gvy = pf.vy, du = pf.u0, dv = pf.v0;
    double x, y, Fxx, Fxy, Fyx, Fyy;
    if (incremental) { // x_f = x_{f-1} + du(x_{f-1}),  F_f = (I + g) F_{f-1}
      const double a = 1.0 + gux, d = 1.0 + gvy;
      const double Pxx = state8[4], Pxy = state8[5], Pyx = state8[6], Pyy = state8[7];
      x = state8[2] + du;
      y = state8[3] + dv;
      Fxx = a * Pxx + guy * Pyx;
      Fxy = a * Pxy + guy * Pyy;
      Fyx = gvx * Pxx + d * Pyx;
      Fyy = gvx * Pxy + d * Pyy;
    } else {
      x = X + du;
      y = Y + dv;
      Fxx = 1.0 + gux;
      Fxy = guy;
      Fyx = gvx;
      Fyy = 1.0 + gvy;
    }
    state8[2] = x, state8[3] = y, state8[4] = Fxx, state8[5] = Fxy, state8[6] = Fyx, state8[7] = Fyy;
    px = (float)x, py = (float)y;
    f[0] = (float)(x - X);
    f[1] = (float)(y - Y);
    f[2] = (float)(Fxx - 1.0);
    f[3] = (float)Fxy;
    f[4] = (float)Fyx;
    f[5] = (float)(Fyy - 1.0);
    (void)lk_strain_tensor_impl(tensor, f + 2, f + 6);
  } else {
    const double lost = (double)NAN;
    for (int i = 2; i < 8; ++i)
      state8[i] = lost;
  }
  out->x = px, out->y = py;
  out->u = f[0], out->v = f[1];
  out->ux = f[2], out->uy = f[3], out->vx = f[4], out->vy = f[5];
  out->exx = f[6], out->eyy = f[7], out->exy = f[8], out->e1 = f[9], out->e2 = f[10], out->theta = f[11];
  out->neighbours = status == LK_TRACK_BAD_POINT || status == LK_TRACK_LOST ? 0 : n;
  out->status = status;
}
