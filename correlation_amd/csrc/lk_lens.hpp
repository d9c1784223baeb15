// lk_lens.hpp - the lens model, its inverse, the correction of a record and the rows of the lens fit (include/lk_engine.h:
// lk_lens_distort, lk_lens_undistort, lk_lens_correct, lk_lens_correct_record, lk_lens_fit).  One function each for the kernels
// (lk_lens.hip) and the host entry points (lk_lens.cpp), like lk_motion.hpp: an undistorted position, a corrected record
// and a row of the fit are these functions of their inputs, whoever computes them.  Everything in double, nothing but
// + - * / in the order written (the build keeps products and sums apart), so the host and the device give the same bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lk_engine.h"

// Newton steps of U = D^-1.  From rho_d the first error is the distortion itself, e0 = |d(rho) - rho| <= 0.05 |rho| at a rim
// distortion of 5 %, and a step squares it up to the ratio of the second to the first derivative of d, which is below 1 for
// such a lens: 5e-2, 3e-3, 1e-5, 1e-10, 1e-20 - four steps reach the rounding of double, six leave two in hand.
constexpr int kLkLensNewton = 6;

constexpr int kLkLensMaxQ = 6;
__host__ __device__ constexpr int lk_lens_q(int nuisance) { return nuisance == LK_LENS_TRANSLATION ? 2 : nuisance == LK_LENS_SIMILARITY ? 4 : 6; }
__host__ __device__ constexpr int lk_lens_width(int q) { return 7 + q; }
__host__ __device__ constexpr int lk_lens_triangle(int q) { return (7 + q) * (8 + q) / 2; }
// doubles of a frame's sums: {n, the triangle, n_outside}
__host__ __device__ constexpr int lk_lens_sums_len(int q) { return lk_lens_triangle(q) + 2; }

// d(rho) = D in units of rn about the centre, and the symmetric Jacobian J = dd / drho = dD / dx_u
struct LkLensJac {
  double xx, xy, yy, det;
};
__host__ __device__ inline void lk_lens_eval(const lk_lens &L, double rx, double ry, double &dx, double &dy, LkLensJac &J) {
  const double xx = rx * rx, yy = ry * ry, xy = rx * ry;
  const double r2 = xx + yy;
  const double radial = 1.0 + L.k1 * r2 + L.k2 * (r2 * r2);
  const double g = 2.0 * L.k1 + 4.0 * L.k2 * r2;
  dx = rx * radial + (2.0 * L.p1 * xy + L.p2 * (r2 + 2.0 * xx));
  dy = ry * radial + (L.p1 * (r2 + 2.0 * yy) + 2.0 * L.p2 * xy);
  J.xx = radial + g * xx + (2.0 * L.p1 * ry + 6.0 * L.p2 * rx);
  J.xy = g * xy + (2.0 * L.p1 * rx + 2.0 * L.p2 * ry);
  J.yy = radial + g * yy + (6.0 * L.p1 * ry + 2.0 * L.p2 * rx);
  J.det = J.xx * J.yy - J.xy * J.xy;
}

// rho_u = U(rho_d) and J there.  Returns 1 when an iterate, the result included, has det J <= 0 (or is not finite): the point
// is outside the model's domain and the outputs mean nothing.
__host__ __device__ inline int lk_lens_undistort_rho(const lk_lens &L, double qx, double qy, double &rx, double &ry, LkLensJac &J) {
  int outside = 0;
  rx = qx, ry = qy;
  double dx, dy;
  for (int it = 0; it < kLkLensNewton; ++it) {
    lk_lens_eval(L, rx, ry, dx, dy, J);
    if (!(J.det > 0.0))
      outside = 1;
    const double ex = dx - qx, ey = dy - qy;
    rx = rx - (J.yy * ex - J.xy * ey) / J.det;
    ry = ry - (J.xx * ey - J.xy * ex) / J.det;
  }
  lk_lens_eval(L, rx, ry, dx, dy, J);
  if (!(J.det > 0.0) || !(J.det - J.det == 0.0))
    outside = 1;
  return outside;
}

// positions in level-0 pixels
__host__ __device__ inline void lk_lens_distort_point(const lk_lens &L, double x, double y, double &xd, double &yd) {
  LkLensJac J;
  double dx, dy;
  lk_lens_eval(L, (x - L.cx) / L.rn, (y - L.cy) / L.rn, dx, dy, J);
  xd = L.cx + L.rn * dx, yd = L.cy + L.rn * dy;
}
__host__ __device__ inline int lk_lens_undistort_point(const lk_lens &L, double x, double y, double &xu, double &yu, LkLensJac &J) {
  double rx, ry;
  const int outside = lk_lens_undistort_rho(L, (x - L.cx) / L.rn, (y - L.cy) / L.rn, rx, ry, J);
  xu = L.cx + L.rn * rx, yu = L.cy + L.rn * ry;
  return outside;
}

// One record with the distortion taken out: X_u = U(X), x_u = U(X + (u, v)), (u', v') = x_u - X_u and the record's own
// gradient F' = J_D(x_u)^-1 F J_D(X_u), written back in the model's layout as lk_motion_remove_params does, each output rounded
// to float once.  Returns 0, or 2 with the parameters untouched when either point is outside the model's domain.
__host__ __device__ inline int lk_lens_correct_params(int model, const lk_lens &L, float centre_x, float centre_y, float &p0, float &p1,
                                                      float &p2, float &p3, float &p4, float &p5) {
  const double X = (double)centre_x, Y = (double)centre_y;
  const double u = (double)p0, v = model == LK_FM_U ? 0.0 : (double)p1;
  LkLensJac A, B; // at X_u and at x_u
  double Xu, Yu, xu2, yu2;
  const int out_X = lk_lens_undistort_point(L, X, Y, Xu, Yu, A);
  const int out_x = lk_lens_undistort_point(L, X + u, Y + v, xu2, yu2, B);
  if (out_X || out_x)
    return 2;
  const bool uvq = model == LK_FM_UVQ, six = model == LK_FM_UVUXUYVXVY;
  const double q = (double)p2;
  const double Fxx = uvq ? 1.0 : 1.0 + (double)p2, Fxy = uvq ? 0.0 - q : (double)p3;
  const double Fyx = uvq ? q : (double)p4, Fyy = uvq ? 1.0 : 1.0 + (double)p5;
  // F J_D(X_u), then J_D(x_u)^-1 of it
  const double Hxx = Fxx * A.xx + Fxy * A.xy, Hxy = Fxx * A.xy + Fxy * A.yy;
  const double Hyx = Fyx * A.xx + Fyy * A.xy, Hyy = Fyx * A.xy + Fyy * A.yy;
  const double ixx = B.yy / B.det, ixy = (0.0 - B.xy) / B.det, iyy = B.xx / B.det;
  const double Gxx = ixx * Hxx + ixy * Hyx, Gxy = ixx * Hxy + ixy * Hyy;
  const double Gyx = ixy * Hxx + iyy * Hyx, Gyy = ixy * Hxy + iyy * Hyy;
  // (every parameter is stored once, by a select: no store whose destination depends on the model)
  const float n0 = (float)(xu2 - Xu), n1 = model == LK_FM_U ? p1 : (float)(yu2 - Yu);
  const float n2 = uvq ? (float)((Gyx - Gxy) / 2.0) : six ? (float)(Gxx - 1.0) : p2;
  const float n3 = six ? (float)Gxy : p3, n4 = six ? (float)Gyx : p4, n5 = six ? (float)(Gyy - 1.0) : p5;
  p0 = n0, p1 = n1, p2 = n2, p3 = n3, p4 = n4, p5 = n5;
  return 0;
}

// dU / d(k1, k2, p1, p2, cx, cy) at the undistorted point rho with J = J_D there: -J^-1 dD/dtheta, and dD/dc = I - J.
// out[j] = {x, y} of parameter j, in pixels.
__host__ __device__ inline void lk_lens_du(const lk_lens &L, double rx, double ry, const LkLensJac &J, double (*out)[2]) {
  const double xx = rx * rx, yy = ry * ry, xy = rx * ry;
  const double r2 = xx + yy, r4 = r2 * r2;
  const double ixx = J.yy / J.det, ixy = (0.0 - J.xy) / J.det, iyy = J.xx / J.det;
  const double dDx[4] = {L.rn * (rx * r2), L.rn * (rx * r4), L.rn * (2.0 * xy), L.rn * (r2 + 2.0 * xx)};
  const double dDy[4] = {L.rn * (ry * r2), L.rn * (ry * r4), L.rn * (r2 + 2.0 * yy), L.rn * (2.0 * xy)};
  for (int j = 0; j < 4; ++j) {
    out[j][0] = 0.0 - (ixx * dDx[j] + ixy * dDy[j]);
    out[j][1] = 0.0 - (ixy * dDx[j] + iyy * dDy[j]);
  }
  out[4][0] = 1.0 - ixx, out[4][1] = 0.0 - ixy;
  out[5][0] = 0.0 - ixy, out[5][1] = 1.0 - iyy;
}

// The two rows of one record of the fit set, W = 7 + Q wide each: [dr/d(k1, k2, p1, p2, cx, cy) | dr/dn (Q) | r] with
//   r = U(X + u) - U(X) - N(U(X)),  N(X_u) = t + G (X_u - o),  n = {tx, ty} / {tx, ty, a, b}: G = [[a, -b], [b, a]] /
//   {tx, ty, gxx, gxy, gyx, gyy},
//   dr/dtheta = dx_u/dtheta - (I + G) dX_u/dtheta.
// nu: the frame's six nuisance doubles (those beyond Q are not read).  Returns 1 (rows untouched) when X or X + u is outside
// the model's domain.
template <int Q>
__host__ __device__ inline int lk_lens_rows(const lk_lens &L, const double *nu, double ox, double oy, double X, double Y, double u,
                                            double v, double *ax, double *ay) {
  LkLensJac A, B;
  double RX, RY, rx, ry;
  const int out_X = lk_lens_undistort_rho(L, (X - L.cx) / L.rn, (Y - L.cy) / L.rn, RX, RY, A);
  const int out_x = lk_lens_undistort_rho(L, ((X + u) - L.cx) / L.rn, ((Y + v) - L.cy) / L.rn, rx, ry, B);
  if (out_X || out_x)
    return 1;
  const double Xu = L.cx + L.rn * RX, Yu = L.cy + L.rn * RY, xu = L.cx + L.rn * rx, yu = L.cy + L.rn * ry;
  double dX[6][2], dx[6][2];
  lk_lens_du(L, RX, RY, A, dX);
  lk_lens_du(L, rx, ry, B, dx);
  double gxx = 0.0, gxy = 0.0, gyx = 0.0, gyy = 0.0;
  if (Q == 4)
    gxx = nu[2], gxy = 0.0 - nu[3], gyx = nu[3], gyy = nu[2];
  if (Q == 6)
    gxx = nu[2], gxy = nu[3], gyx = nu[4], gyy = nu[5];
  const double mxx = 1.0 + gxx, myy = 1.0 + gyy;
  const double ex = Xu - ox, ey = Yu - oy;
  for (int j = 0; j < 6; ++j) {
    ax[j] = dx[j][0] - (mxx * dX[j][0] + gxy * dX[j][1]);
    ay[j] = dx[j][1] - (gyx * dX[j][0] + myy * dX[j][1]);
  }
  ax[6] = -1.0, ay[6] = 0.0;
  ax[7] = 0.0, ay[7] = -1.0;
  if (Q == 4) {
    ax[8] = 0.0 - ex, ay[8] = 0.0 - ey;
    ax[9] = ey, ay[9] = 0.0 - ex;
  }
  if (Q == 6) {
    ax[8] = 0.0 - ex, ay[8] = 0.0;
    ax[9] = 0.0 - ey, ay[9] = 0.0;
    ax[10] = 0.0, ay[10] = 0.0 - ex;
    ax[11] = 0.0, ay[11] = 0.0 - ey;
  }
  ax[6 + Q] = (xu - Xu) - (nu[0] + (gxx * ex + gxy * ey));
  ay[6 + Q] = (yu - Yu) - (nu[1] + (gyx * ex + gyy * ey));
  return 0;
}
