// lk_motion.hpp - the global motion of a frame and its removal from a record (include/lk_engine.h: lk_rigid_motion,
// lk_motion_from_sums, lk_motion_apply, lk_motion_remove).  One function each for the kernels (lk_motion.hip) and the host
// entry points (lk_motion.cpp), like lk_strain.hpp and lk_track.hpp: the motion is this function of the fit set's count and
// sums, a record without the motion is this function of the record and the 64-byte motion, whoever computes them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"
#include "lk_strain.hpp"

// What the residual pass and the next pass's trimming read of a fit, in double and before any rounding to float, in the
// coordinates of the sums (relative to the origin, the centre of the centres' bounding box).
struct LkMotionFit {
  double cx, cy;             // centroid of the fit set
  double tx, ty;             // its displacement
  double axx, axy, ayx, ayy; // A
  double threshold;          // reject * rms of this pass (+inf without trimming); set by the residual pass
  int status, n;
};

__host__ __device__ inline int lk_motion_min_sectors(int kind) {
  return kind == LK_MOTION_TRANSLATION ? 1 : kind == LK_MOTION_AFFINE ? 3 : 2;
}

// n: sectors of the fit set; sums11 = {Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv} relative to (ox, oy).  All in
// double, each product, quotient, sum and difference rounded to double in the order written; nothing but + - * / sqrt on
// the way to c, t, A and scale (theta's atan2 is the one exception), so that the host and the device give the same bytes.
// The record's float fields are each rounded once; rms, max_residual, n_rejected and passes_run are left 0 for the caller.
__host__ __device__ inline LkMotionFit lk_motion_fit_impl(int kind, int min_sectors, int n, const double *sums11, double ox,
                                                          double oy, lk_motion *out) {
  const double N = (double)n;
  const double Sx = sums11[0], Sy = sums11[1], Su = sums11[5], Sxu = sums11[6], Syu = sums11[7], Sv = sums11[8];
  const double Sxv = sums11[9], Syv = sums11[10];
  const LkPlaneFit pf = lk_plane_fit(n, sums11);
  // the cross moments, by lk_plane_fit's own expressions
  const double Cxu = Sxu - Sx * Su / N, Cyu = Syu - Sy * Su / N, Cxv = Sxv - Sx * Sv / N, Cyv = Syv - Sy * Sv / N;
  const double num = Cxv - Cyu, den = pf.Cxx + Cxu + pf.Cyy + Cyv;
  const double h = sqrt(num * num + den * den), spread = pf.Cxx + pf.Cyy;
  LkMotionFit f;
  f.cx = Sx / N, f.cy = Sy / N, f.tx = Su / N, f.ty = Sv / N;
  f.axx = 1.0, f.axy = 0.0, f.ayx = 0.0, f.ayy = 1.0;
  f.threshold = (double)INFINITY;
  f.n = n;
  int status = LK_MOTION_OK;
  if (n < min_sectors) {
    status = LK_MOTION_TOO_FEW;
  } else if (kind == LK_MOTION_RIGID || kind == LK_MOTION_SIMILARITY) {
    if (spread == 0.0 || h == 0.0 || !(h - h == 0.0) || !(spread - spread == 0.0)) {
      status = LK_MOTION_DEGENERATE;
    } else {
      const double q = kind == LK_MOTION_RIGID ? h : spread;
      f.axx = den / q, f.axy = (0.0 - num) / q, f.ayx = num / q, f.ayy = den / q;
    }
  } else if (kind == LK_MOTION_AFFINE) {
    f.axx = 1.0 + pf.ux, f.axy = pf.uy, f.ayx = pf.vx, f.ayy = 1.0 + pf.vy;
    // lk_strain_field's rule for the centres; and an A that folds the plane onto a line has no inverse to remove it with
    if (pf.CC == 0.0 || !(pf.D > 1e-6 * pf.CC) || !(f.axx * f.ayy - f.axy * f.ayx != 0.0))
      status = LK_MOTION_DEGENERATE;
  }
  f.status = status;
  out->cx = out->cy = out->tx = out->ty = 0.f;
  out->axx = out->axy = out->ayx = out->ayy = 0.f;
  out->theta = out->scale = out->rms = out->max_residual = 0.f;
  out->n_fit = n, out->n_rejected = 0, out->status = status, out->passes_run = 0;
  if (status == LK_MOTION_OK) {
    const double det = f.axx * f.ayy - f.axy * f.ayx;
    out->cx = (float)(ox + f.cx), out->cy = (float)(oy + f.cy);
    out->tx = (float)f.tx, out->ty = (float)f.ty;
    out->axx = (float)f.axx, out->axy = (float)f.axy, out->ayx = (float)f.ayx, out->ayy = (float)f.ayy;
    out->theta = (float)atan2(f.ayx - f.axy, f.axx + f.ayy);
    out->scale = (float)sqrt(det < 0.0 ? 0.0 - det : det);
  }
  return f;
}

// The residual of one sector to a fit, squared: |x' - (c + t + A (x - c))|^2 with x the centre relative to the origin and
// x' = x + (u, v), all in double.
__host__ __device__ inline double lk_motion_residual2(const LkMotionFit &f, double x, double y, double u, double v) {
  const double dx = x - f.cx, dy = y - f.cy;
  const double rx = (x + u) - (f.cx + f.tx + (f.axx * dx + f.axy * dy));
  const double ry = (y + v) - (f.cy + f.ty + (f.ayx * dx + f.ayy * dy));
  return rx * rx + ry * ry;
}

// One record with the motion m taken out: x'' = c + A^-1 (x' - c - t) with x' = centre + (u, v), (u'', v'') = x'' - centre,
// and the record's own deformation gradient F'' = A^-1 F, from the motion's float fields as stored, in double, each output
// rounded to float once.  chi, the counts, the error code and undCenter are copied.  The caller decides which records are
// rewritten (the good ones of a frame whose motion is LK_MOTION_OK) and refuses LK_FM_U with a kind that has an A.
// Returns 1 (and copies the record) when A has no inverse, else 0.
// The six parameters travel by name (the kernel keeps them in registers); returns 1, the parameters untouched, when A has
// no inverse, else 0.
__host__ __device__ inline int lk_motion_remove_params(int model, const lk_motion &m, float centre_x, float centre_y, float &p0,
                                                       float &p1, float &p2, float &p3, float &p4, float &p5) {
  const double axx = (double)m.axx, axy = (double)m.axy, ayx = (double)m.ayx, ayy = (double)m.ayy;
  const double det = axx * ayy - axy * ayx;
  if (!(det != 0.0) || !(det - det == 0.0))
    return 1;
  const double ixx = ayy / det, ixy = (0.0 - axy) / det, iyx = (0.0 - ayx) / det, iyy = axx / det;
  const double X = (double)centre_x, Y = (double)centre_y;
  const double u = (double)p0, v = model == LK_FM_U ? 0.0 : (double)p1;
  const double dx = (X + u) - (double)m.cx - (double)m.tx, dy = (Y + v) - (double)m.cy - (double)m.ty;
  const double x2 = (double)m.cx + (ixx * dx + ixy * dy), y2 = (double)m.cy + (iyx * dx + iyy * dy);
  // (every parameter is stored once, by a select: no store whose destination depends on the model)
  const bool uvq = model == LK_FM_UVQ, six = model == LK_FM_UVUXUYVXVY;
  const double q = (double)p2;
  const double Fxx = uvq ? 1.0 : 1.0 + (double)p2, Fxy = uvq ? 0.0 - q : (double)p3;
  const double Fyx = uvq ? q : (double)p4, Fyy = uvq ? 1.0 : 1.0 + (double)p5;
  const double Gxx = ixx * Fxx + ixy * Fyx, Gxy = ixx * Fxy + ixy * Fyy;
  const double Gyx = iyx * Fxx + iyy * Fyx, Gyy = iyx * Fxy + iyy * Fyy;
  const float n0 = (float)(x2 - X), n1 = model == LK_FM_U ? p1 : (float)(y2 - Y);
  const float n2 = uvq ? (float)((Gyx - Gxy) / 2.0) : six ? (float)(Gxx - 1.0) : p2;
  const float n3 = six ? (float)Gxy : p3, n4 = six ? (float)Gyx : p4, n5 = six ? (float)(Gyy - 1.0) : p5;
  p0 = n0, p1 = n1, p2 = n2, p3 = n3, p4 = n4, p5 = n5;
  return 0;
}
__host__ __device__ inline int lk_motion_remove_impl(int model, const lk_motion &m, float centre_x, float centre_y,
                                                     const lk_result &in, lk_result *out) {
  *out = in;
  float *p = out->resultingParameters;
  return lk_motion_remove_params(model, m, centre_x, centre_y, p[0], p[1], p[2], p[3], p[4], p[5]);
}
