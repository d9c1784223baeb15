// lk_weighted.hpp - what the weighted refinement's kernel and its host entry points share (include/lk_engine.h:
// lk_refine_weighted, lk_weight_window): the window function.  All in float; a product and a sum are
// rounded separately except where __builtin_fmaf says otherwise, and no library exponential takes part, so that the host
// and the device give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

constexpr float kLkWindowCut = 126.f; // t at and above which the window is 0 (2^-126 is the smallest normal float)

// The Gaussian window exp(-r^2 / (2 sigma^2)) as 2^-t, t = r2 inv, with inv = log2(e) / (2 sigma^2) formed by the caller and
// r2 = fma(dy, dy, dx dx).  t = k + x with k = (int)(t + 0.5f) and x = t - k in [-0.5, 0.5], exact in float; 2^-x is the
// Taylor polynomial of degree 7 of exp(-x ln 2) - each coefficient the float nearest (-ln 2)^j / j!; the first dropped term
// is at most (0.5 ln 2)^8 / 8! = 5.2e-9, 7e-9 of the smallest value - by Horner's rule, one fused multiply-add per power;
// 2^-k by ldexpf, which is exact: k <= 126 and the polynomial is >= 1 for x <= 0, so no result is subnormal.  0 for
// t >= 126 or a t that is not a number.
__host__ __device__ __forceinline__ float lk_window_weight(float inv, float dx, float dy) {
  const float r2 = __builtin_fmaf(dy, dy, dx * dx);
  const float t = r2 * inv;
  if (!(t < kLkWindowCut))
    return 0.f;
  const int k = (int)(t + 0.5f);
  const float x = t - (float)k;
  constexpr double c[8] = {1.0,
                           -0.6931471805599453,
                           0.2402265069591007,
                           -0.05550410866482158,
                           0.009618129107628477,
                           -0.0013333558146428443,
                           0.00015403530393381608,
                           -1.5252733804059841e-05};
  float v = (float)c[7];
#pragma unroll
  for (int j = 6; j >= 0; --j)
    v = __builtin_fmaf(v, x, (float)c[j]);
  return ldexpf(v, -k);
}
