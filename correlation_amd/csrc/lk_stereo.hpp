// lk_stereo.hpp - a calibrated two-camera rig: projection, triangulation, the fundamental matrix and the strain of a surface
// of 3-D points (include/lk_engine.h: lk_stereo_project, lk_stereo_triangulate, lk_stereo_fundamental, lk_stereo_points,
// lk_stereo_strain, lk_stereo_surface_from_sums).  One function each for the kernels (lk_stereo.hip) and the host entry points
// (lk_stereo.cpp), like lk_lens.hpp: a triangulated point and a surface record are these functions of their inputs, whoever
// computes them.  The triangulation is in double, nothing but + - * / sqrt in the order written (the build keeps products and
// sums apart; sqrt of a double is correctly rounded on both sides), so the host and the device give the same bytes.  The lens
// of a camera is lk_lens.hpp's, called, not restated.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/lk_engine.h"
#include "lk_device.hpp"
#include "lk_lens.hpp"
#include "lk_strain.hpp"

// Gauss-Newton steps of the triangulation.  The start, the midpoint of the common perpendicular, is off the minimiser of the
// reprojection error by the matching error itself, e0 <= (epsilon / f) Z / sin(angle) with epsilon the pixel error of a match:
// 0.5 px at f = 800, Z = 400 and 20 degrees is 0.7 of a world unit, 2e-3 of Z.  The problem has a small residual, so a
// Gauss-Newton step multiplies the error by about (epsilon / f) / sin(angle) + e / Z - the neglected second-order term over
// the first-order one - some 4e-3 here: 2e-3, 8e-6, 3e-8, 1e-10, 5e-13 ... relative.  Five steps reach the rounding of
// double on such a rig, seven leave two in hand (tests/test_stereo_host.py checks J^T r at the result).
constexpr int kLkStereoNewton = 7;

// rays whose sin^2 of the angle between them is at most this are PARALLEL (an angle of 1e-6 rad); scale-free
constexpr double kLkStereoParallel = 1e-12;
// the surface seen edge-on: G11 G22 - G12^2 <= this times G11 G22
constexpr double kLkStereoEdgeOn = 1e-12;

__host__ __device__ inline bool lk_camera_has_lens(const lk_camera &c) {
  return c.lens.k1 != 0.0 || c.lens.k2 != 0.0 || c.lens.p1 != 0.0 || c.lens.p2 != 0.0;
}

// a world point -> x_cam = R X + t
__host__ __device__ inline void lk_stereo_to_camera(const lk_camera &c, double X, double Y, double Z, double &x, double &y, double &z) {
  x = (c.R[0] * X + c.R[1] * Y) + (c.R[2] * Z + c.t[0]);
  y = (c.R[3] * X + c.R[4] * Y) + (c.R[5] * Z + c.t[1]);
  z = (c.R[6] * X + c.R[7] * Y) + (c.R[8] * Z + c.t[2]);
}

// the pinhole: x_cam -> the undistorted pixel (z > 0 is the caller's check)
__host__ __device__ inline void lk_stereo_pinhole(const lk_camera &c, double x, double y, double z, double &u, double &v) {
  const double xn = x / z, yn = y / z;
  u = (c.fx * xn + c.skew * yn) + c.cx;
  v = c.fy * yn + c.cy;
}

// A world point -> the pixel the camera shows it at: pinhole, then the lens.  Returns 1 (outputs 0) for a point that is not in
// front of the camera.
__host__ __device__ inline int lk_stereo_project_impl(const lk_camera &c, double X, double Y, double Z, double &px, double &py) {
  double x, y, z, u, v;
  lk_stereo_to_camera(c, X, Y, Z, x, y, z);
  px = 0.0, py = 0.0;
  if (!(z > 0.0))
    return 1;
  lk_stereo_pinhole(c, x, y, z, u, v);
  if (lk_camera_has_lens(c))
    lk_lens_distort_point(c.lens, u, v, px, py);
  else
    px = u, py = v;
  return 0;
}

// A pixel as the camera shows it -> the undistorted pixel (a camera without lens coefficients: the pixel itself, exactly).
// Returns 1 outside the lens's domain.
__host__ __device__ inline int lk_stereo_undistort(const lk_camera &c, double x, double y, double &xu, double &yu) {
  if (!lk_camera_has_lens(c)) {
    xu = x, yu = y;
    return 0;
  }
  LkLensJac J;
  return lk_lens_undistort_point(c.lens, x, y, xu, yu, J);
}

// the ray of an undistorted pixel in the world frame: origin o = -R^T t, direction d = R^T K^-1 (u, v, 1) (not normalised)
__host__ __device__ inline void lk_stereo_ray(const lk_camera &c, double u, double v, double *o, double *d) {
  const double yn = (v - c.cy) / c.fy;
  const double xn = ((u - c.cx) - c.skew * yn) / c.fx;
  for (int i = 0; i < 3; ++i) {
    d[i] = (c.R[i] * xn + c.R[3 + i] * yn) + c.R[6 + i];
    o[i] = 0.0 - ((c.R[i] * c.t[0] + c.R[3 + i] * c.t[1]) + c.R[6 + i] * c.t[2]);
  }
}

// atan2(s, c) for s >= 0, in [0, pi], from + - * / sqrt alone (the host's and the device's libraries differ in their last
// bit): two halvings atan(x) = 2 atan(x / (1 + sqrt(1 + x^2))) bring x in [0, 1] below tan(pi / 16) = 0.199, where the
// series to x^27 / 27 is below 1e-20.
__host__ __device__ inline double lk_stereo_atan_unit(double x) { // 0 <= x <= 1
  for (int i = 0; i < 2; ++i)
    x = x / (1.0 + sqrt(1.0 + x * x));
  const double x2 = x * x;
  double p = 1.0 / 27.0;
  for (int k = 25; k >= 1; k -= 2)
    p = 1.0 / (double)k - x2 * p;
  return 4.0 * (x * p);
}
__host__ __device__ inline double lk_stereo_angle(double s, double c) {
  const double pi = 3.14159265358979323846;
  if (s == 0.0 && c == 0.0)
    return 0.0;
  if (c >= s)
    return lk_stereo_atan_unit(s / c);
  if (0.0 - c >= s)
    return pi - lk_stereo_atan_unit(s / (0.0 - c));
  const double a = lk_stereo_atan_unit((c < 0.0 ? 0.0 - c : c) / s);
  return c < 0.0 ? pi / 2.0 + a : pi / 2.0 - a;
}

// One camera's share of a Gauss-Newton step at the point P: its two residuals (observed - projected) and their rows' products
// added to J^T J and J^T r.  Scalars throughout: nothing here is indexed by a running number.  Returns 1 for a point that is
// not in front of the camera.
struct LkStereoNormal {
  double a00, a01, a02, a11, a12, a22, g0, g1, g2;
};
__host__ __device__ inline int lk_stereo_residual(const lk_camera &cam, double PX, double PY, double PZ, double mu, double mv, double &ru,
                                                  double &rv, LkStereoNormal &N) {
  double x, y, z, u, v;
  lk_stereo_to_camera(cam, PX, PY, PZ, x, y, z);
  if (!(z > 0.0))
    return 1;
  lk_stereo_pinhole(cam, x, y, z, u, v);
  ru = mu - u, rv = mv - v;
  const double xn = x / z, yn = y / z;
  const double ex0 = cam.R[0] - xn * cam.R[6], ex1 = cam.R[1] - xn * cam.R[7], ex2 = cam.R[2] - xn * cam.R[8];
  const double ey0 = cam.R[3] - yn * cam.R[6], ey1 = cam.R[4] - yn * cam.R[7], ey2 = cam.R[5] - yn * cam.R[8];
  const double ju0 = (cam.fx * ex0 + cam.skew * ey0) / z, ju1 = (cam.fx * ex1 + cam.skew * ey1) / z, ju2 = (cam.fx * ex2 + cam.skew * ey2) / z;
  const double jv0 = (cam.fy * ey0) / z, jv1 = (cam.fy * ey1) / z, jv2 = (cam.fy * ey2) / z;
  N.a00 += ju0 * ju0 + jv0 * jv0;
  N.a01 += ju0 * ju1 + jv0 * jv1;
  N.a02 += ju0 * ju2 + jv0 * jv2;
  N.a11 += ju1 * ju1 + jv1 * jv1;
  N.a12 += ju1 * ju2 + jv1 * jv2;
  N.a22 += ju2 * ju2 + jv2 * jv2;
  N.g0 += ju0 * ru + jv0 * rv;
  N.g1 += ju1 * ru + jv1 * rv;
  N.g2 += ju2 * ru + jv2 * rv;
  return 0;
}

// One matched pair of pixels (x0 in camera 0, x1 in camera 1, as the cameras show them) -> the 3-D point.  The steps, the
// statuses and their order are include/lk_engine.h's (`triangulation`).  A record that is not OK is all zeros but its status.
__host__ __device__ inline lk_stereo_point lk_stereo_triangulate_impl(const LkStereoRig &rig, int good, double x0, double y0, double x1,
                                                                      double y1) {
  lk_stereo_point out;
  out.X = out.Y = out.Z = 0.0;
  out.residual[0] = out.residual[1] = out.residual[2] = out.residual[3] = 0.f;
  out.epipolar = out.angle = 0.f;
  out.reserved[0] = out.reserved[1] = out.reserved[2] = 0;
  out.status = LK_STEREO_BAD_RECORD;
  if (!good || !(x0 - x0 == 0.0) || !(y0 - y0 == 0.0) || !(x1 - x1 == 0.0) || !(y1 - y1 == 0.0))
    return out;
  // 1. the undistorted pixels
  double m0x, m0y, m1x, m1y;
  const int outside0 = lk_stereo_undistort(rig.cam[0], x0, y0, m0x, m0y);
  const int outside1 = lk_stereo_undistort(rig.cam[1], x1, y1, m1x, m1y);
  out.status = LK_STEREO_OUTSIDE_LENS;
  if (outside0 || outside1)
    return out;
  // 2. the rays
  double o0[3], d0[3], o1[3], d1[3];
  lk_stereo_ray(rig.cam[0], m0x, m0y, o0, d0);
  lk_stereo_ray(rig.cam[1], m1x, m1y, o1, d1);
  // 3. the midpoint of the common perpendicular: o0 + s d0 and o1 + t d1 closest to each other
  const double w[3] = {o0[0] - o1[0], o0[1] - o1[1], o0[2] - o1[2]};
  const double a = (d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2];
  const double b = (d0[0] * d1[0] + d0[1] * d1[1]) + d0[2] * d1[2];
  const double c = (d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2];
  const double d = (d0[0] * w[0] + d0[1] * w[1]) + d0[2] * w[2];
  const double e = (d1[0] * w[0] + d1[1] * w[1]) + d1[2] * w[2];
  const double ac = a * c, det = ac - b * b;
  out.status = LK_STEREO_PARALLEL;
  if (!(det > kLkStereoParallel * ac))
    return out;
  const double s = (b * e - c * d) / det, t = (a * e - b * d) / det;
  out.status = LK_STEREO_BEHIND;
  if (!(s > 0.0) || !(t > 0.0))
    return out;
  // 4. Gauss-Newton on the four reprojection residuals (undistorted pixels) over the point
  double PX = ((o0[0] + s * d0[0]) + (o1[0] + t * d1[0])) / 2.0;
  double PY = ((o0[1] + s * d0[1]) + (o1[1] + t * d1[1])) / 2.0;
  double PZ = ((o0[2] + s * d0[2]) + (o1[2] + t * d1[2])) / 2.0;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  for (int it = 0; it <= kLkStereoNewton; ++it) {
    LkStereoNormal N = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (lk_stereo_residual(rig.cam[0], PX, PY, PZ, m0x, m0y, r0, r1, N) || lk_stereo_residual(rig.cam[1], PX, PY, PZ, m1x, m1y, r2, r3, N))
      return out; // (BEHIND)
    if (it == kLkStereoNewton)
      break; // (the residuals of the result)
    // A = L D L^T, then the two triangular solves, in this order
    const double l10 = N.a01 / N.a00, l20 = N.a02 / N.a00;
    const double D1 = N.a11 - l10 * N.a01;
    const double m21 = N.a12 - l20 * N.a01;
    const double l21 = m21 / D1;
    const double D2 = (N.a22 - l20 * N.a02) - l21 * m21;
    const double z0 = N.g0, z1 = N.g1 - l10 * z0, z2 = (N.g2 - l20 * z0) - l21 * z1;
    const double q2 = z2 / D2;
    const double q1 = z1 / D1 - l21 * q2;
    const double q0 = (z0 / N.a00 - l10 * q1) - l20 * q2;
    PX = PX + q0, PY = PY + q1, PZ = PZ + q2;
  }
  out.status = LK_STEREO_PARALLEL; // a step that left the numbers: the normal equations were singular
  if (!((PX - PX) + (PY - PY) + (PZ - PZ) == 0.0) || !((r0 - r0) + (r1 - r1) + (r2 - r2) + (r3 - r3) == 0.0))
    return out;
  // the epipolar line of point 0 in camera 1, l = F (m0, 1), and the signed distance of point 1 from it
  const double *F = rig.F;
  const double l0 = (F[0] * m0x + F[1] * m0y) + F[2], l1 = (F[3] * m0x + F[4] * m0y) + F[5], l2 = (F[6] * m0x + F[7] * m0y) + F[8];
  const double ln = sqrt(l0 * l0 + l1 * l1);
  const double epi = ln > 0.0 ? ((l0 * m1x + l1 * m1y) + l2) / ln : 0.0;
  // the angle between the rays: atan2(|d0 x d1|, d0 . d1)
  const double cx = d0[1] * d1[2] - d0[2] * d1[1], cy = d0[2] * d1[0] - d0[0] * d1[2], cz = d0[0] * d1[1] - d0[1] * d1[0];
  const double angle = lk_stereo_angle(sqrt((cx * cx + cy * cy) + cz * cz), b);
  out.X = PX, out.Y = PY, out.Z = PZ;
  out.residual[0] = (float)r0, out.residual[1] = (float)r1, out.residual[2] = (float)r2, out.residual[3] = (float)r3;
  out.epipolar = (float)epi;
  out.angle = (float)angle;
  out.status = LK_STEREO_OK;
  return out;
}

// ---- the surface fit -------------------------------------------------------------------------------------------------------
// The sums of a window in lk_stereo_surface_from_sums' layout: {Sx, Sy, Sxx, Sxy, Syy} and {Sf, Sxf, Syf} of the six
// functions X, Y, Z (the reference points) and U, V, W (frame point minus reference point).
constexpr int kLkStereoSums = 23; // (the count travels beside them as an int)
struct LkStereoPlanes {           // f(x, y) = f0 + fx x + fy y of the six functions, and the status of the window
  double f0[6], fx[6], fy[6];
  int status;
};

// The six planes: lk_plane_fit's moments and solve, two functions at a time (the moments of the centres come out the same
// bits each time), and the first two statuses.  self_good = 0: a valid fit is FILLED.
__host__ __device__ inline LkStereoPlanes lk_stereo_planes(int n, const double *sums23, int min_neighbours, int self_good) {
  LkStereoPlanes p;
  double CC = 0.0, D = 0.0;
  for (int k = 0; k < 3; ++k) {
    double s11[11];
    for (int i = 0; i < 5; ++i)
      s11[i] = sums23[i];
    for (int i = 0; i < 3; ++i)
      s11[5 + i] = sums23[5 + 6 * k + i], s11[8 + i] = sums23[8 + 6 * k + i];
    const LkPlaneFit f = lk_plane_fit(n, s11);
    CC = f.CC, D = f.D;
    p.f0[2 * k] = f.u0, p.fx[2 * k] = f.ux, p.fy[2 * k] = f.uy;
    p.f0[2 * k + 1] = f.v0, p.fx[2 * k + 1] = f.vx, p.fy[2 * k + 1] = f.vy;
  }
  p.status = LK_STEREO_SURFACE_OK;
  if (n < min_neighbours)
    p.status = LK_STEREO_SURFACE_TOO_FEW;
  else if (CC == 0.0 || !(D > 1e-6 * CC))
    p.status = LK_STEREO_SURFACE_DEGENERATE;
  else {
    const double G11 = (p.fx[0] * p.fx[0] + p.fx[1] * p.fx[1]) + p.fx[2] * p.fx[2];
    const double G12 = (p.fx[0] * p.fy[0] + p.fx[1] * p.fy[1]) + p.fx[2] * p.fy[2];
    const double G22 = (p.fy[0] * p.fy[0] + p.fy[1] * p.fy[1]) + p.fy[2] * p.fy[2];
    const double GG = G11 * G22;
    if (!(GG - G12 * G12 > kLkStereoEdgeOn * GG))
      p.status = LK_STEREO_SURFACE_DEGENERATE;
    else if (!self_good)
      p.status = LK_STEREO_SURFACE_FILLED;
  }
  return p;
}

// The record of a window from its planes and the sum of the squared 3-D misfits of the displacement planes (rr, the second
// walk's).  The gradients of the reference planes are the tangent vectors a1, a2; the algebra is include/lk_engine.h's (`tensor`).
__host__ __device__ inline lk_stereo_surface lk_stereo_surface_impl(int n, const LkStereoPlanes &p, double rr) {
  lk_stereo_surface o;
  float *f = &o.X;
  for (int i = 0; i < 19; ++i)
    f[i] = 0.f;
  o.neighbours = n, o.status = p.status;
  for (int i = 0; i < 11; ++i)
    o.reserved[i] = 0;
  if (p.status != LK_STEREO_SURFACE_OK && p.status != LK_STEREO_SURFACE_FILLED)
    return o;
  const double *a1 = p.fx, *a2 = p.fy; // reference tangents (0..2); displacement gradients (3..5)
  double b1[3], b2[3];
  for (int i = 0; i < 3; ++i)
    b1[i] = a1[i] + a1[3 + i], b2[i] = a2[i] + a2[3 + i];
  const double G11 = (a1[0] * a1[0] + a1[1] * a1[1]) + a1[2] * a1[2];
  const double G12 = (a1[0] * a2[0] + a1[1] * a2[1]) + a1[2] * a2[2];
  const double G22 = (a2[0] * a2[0] + a2[1] * a2[1]) + a2[2] * a2[2];
  const double g11 = (b1[0] * b1[0] + b1[1] * b1[1]) + b1[2] * b1[2];
  const double g12 = (b1[0] * b2[0] + b1[1] * b2[1]) + b1[2] * b2[2];
  const double g22 = (b2[0] * b2[0] + b2[1] * b2[1]) + b2[2] * b2[2];
  // [a1 a2] = [e1 e2] Ra, Ra upper triangular; M = Ra^-1; C = M^T g M
  const double r11 = sqrt(G11), r12 = G12 / r11, r22 = sqrt(G22 - r12 * r12);
  const double m11 = 1.0 / r11, m22 = 1.0 / r22, m12 = (0.0 - r12) / (r11 * r22);
  const double h1 = g11 * m12 + g12 * m22; // (g M) entry (1, 2)
  const double h2 = g12 * m12 + g22 * m22; // (g M) entry (2, 2)
  const double C11 = (m11 * m11) * g11, C12 = m11 * h1, C22 = m12 * h1 + m22 * h2;
  const double exx = (C11 - 1.0) / 2.0, eyy = (C22 - 1.0) / 2.0, exy = C12 / 2.0;
  // principal values and angle: lk_strain_from_gradient's formulas
  const double mean = (exx + eyy) * 0.5, half = (exx - eyy) * 0.5;
  const double rad = sqrt(half * half + exy * exy);
  const double p1 = mean + rad, p2 = mean - rad;
  // n = e1 x e2 = (a1 x a2) / |a1 x a2|
  const double cx = a1[1] * a2[2] - a1[2] * a2[1], cy = a1[2] * a2[0] - a1[0] * a2[2], cz = a1[0] * a2[1] - a1[1] * a2[0];
  const double cn = sqrt((cx * cx + cy * cy) + cz * cz);
  const double nx = cx / cn, ny = cy / cn, nz = cz / cn;
  o.X = (float)p.f0[0], o.Y = (float)p.f0[1], o.Z = (float)p.f0[2];
  o.U = (float)p.f0[3], o.V = (float)p.f0[4], o.W = (float)p.f0[5];
  o.nx = (float)nx, o.ny = (float)ny, o.nz = (float)nz;
  o.exx = (float)exx, o.eyy = (float)eyy, o.exy = (float)exy;
  o.e1 = (float)p1, o.e2 = (float)p2;
  o.theta = (float)(0.5 * atan2(2.0 * exy, exx - eyy));
  // Biot: sqrt(1 + 2 e_k) - 1 (a principal stretch minus one; 1 + 2 e_k is an eigenvalue of C, positive for a fit that is valid)
  const double s1 = 1.0 + 2.0 * p1, s2 = 1.0 + 2.0 * p2;
  o.biot1 = (float)(sqrt(s1 > 0.0 ? s1 : 0.0) - 1.0), o.biot2 = (float)(sqrt(s2 > 0.0 ? s2 : 0.0) - 1.0);
  o.normal = (float)((p.f0[3] * nx + p.f0[4] * ny) + p.f0[5] * nz);
  o.residual = (float)sqrt(rr / (double)n);
  return o;
}
