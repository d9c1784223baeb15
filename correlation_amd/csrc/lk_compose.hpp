// lk_compose.hpp - the parameter update of the backward (inverse-compositional) mode: W(p) o W(q)^-1.  One function for
// the kernel (lk_backward.hip) and the host entry point lk_compose_inverse, so that both give the same bits (compiled
// without contraction on either side; only +, -, * and a correctly rounded division).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lk_engine.h"

// W(p): d -> t_p + A_p d, d = x - c.  Returns 1 (p_out untouched) when |det A_q| < 1e-6, else 0.
// A = A_p A_q^-1 and t = t_p - A t_q; A - I is formed from the small terms directly (A_q = I + Q, adj(A_q) = I + Q',
// det A_q = 1 + e), so that the gradient terms keep their precision: A - I = (P + Q' + P Q' - e I) / det.
// FM_UVQ (a linearised rotation, not a group): q_out = ((A - I)_10 - (A - I)_01) / 2, the translation is the composed map's.
__host__ __device__ inline int lk_compose_inverse_impl(int model, const float *p, const float *q, float *p_out) {
  if (model == LK_FM_U) {
    p_out[0] = p[0] - q[0];
    return 0;
  }
  if (model == LK_FM_UV) {
    p_out[0] = p[0] - q[0];
    p_out[1] = p[1] - q[1];
    return 0;
  }
  float P00, P01, P10, P11, Q00, Q01, Q10, Q11;
  if (model == LK_FM_UVQ) {
    P00 = 0.f, P01 = -p[2], P10 = p[2], P11 = 0.f;
    Q00 = 0.f, Q01 = -q[2], Q10 = q[2], Q11 = 0.f;
  } else {
    P00 = p[2], P01 = p[3], P10 = p[4], P11 = p[5];
    Q00 = q[2], Q01 = q[3], Q10 = q[4], Q11 = q[5];
  }
  const float e = (Q00 + Q11) + (Q00 * Q11 - Q01 * Q10);
  const float det = 1.f + e;
  if (fabsf(det) < 1e-6f) // (a NaN step is not singular: it composes to NaN parameters, whose evaluation fails, as forward)
    return 1;
  // adj(A_q) - I
  const float R00 = Q11, R01 = -Q01, R10 = -Q10, R11 = Q00;
  const float inv = 1.f / det;
  const float M00 = ((P00 + R00) + (P00 * R00 + P01 * R10) - e) * inv;
  const float M01 = ((P01 + R01) + (P00 * R01 + P01 * R11)) * inv;
  const float M10 = ((P10 + R10) + (P10 * R00 + P11 * R10)) * inv;
  const float M11 = ((P11 + R11) + (P10 * R01 + P11 * R11) - e) * inv;
  // t = t_p - t_q - (A - I) t_q
  const float tx = (p[0] - q[0]) - (M00 * q[0] + M01 * q[1]);
  const float ty = (p[1] - q[1]) - (M10 * q[0] + M11 * q[1]);
  p_out[0] = tx;
  p_out[1] = ty;
  if (model == LK_FM_UVQ) {
    p_out[2] = (M10 - M01) * 0.5f;
  } else {
    p_out[2] = M00;
    p_out[3] = M01;
    p_out[4] = M10;
    p_out[5] = M11;
  }
  return 0;
}
