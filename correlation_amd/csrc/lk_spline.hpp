// lk_spline.hpp - what the B-spline refinement's kernels and its host entry points share (include/lk_engine.h:
// lk_refine_spline, lk_spline_weights): the constants of the recursive prefilter and the weights of
// the sampler.  All in float; a product and a sum are rounded separately except where __builtin_fmaf says otherwise.
#pragma once
#include <hip/hip_runtime.h>

constexpr int kLkSplineStart = 28; // terms of the causal start-up sum (|z|^28 < 6e-11 for the largest pole)
constexpr int kLkSplineMinSide = 8; // the smallest level image the pass takes

// The poles of the order's prefilter in the order they are applied, each the float nearest the double value, and the gain
// prod (1 - z)(1 - 1 / z) = 6 or 120.
template <int ORDER> struct LkSplinePoles;
template <> struct LkSplinePoles<3> {
  static constexpr int N = 1;
  static constexpr float gain = 6.0f;
  __host__ __device__ static constexpr float z(int) { return (float)-0.2679491924311228; } // sqrt(3) - 2
};
template <> struct LkSplinePoles<5> {
  static constexpr int N = 2;
  static constexpr float gain = 120.0f;
  // sqrt(67.5 - sqrt(4436.25)) + sqrt(26.25) - 6.5, sqrt(67.5 + sqrt(4436.25)) - sqrt(26.25) - 6.5
  __host__ __device__ static constexpr float z(int i) { return i == 0 ? (float)-0.43057534709997825 : (float)-0.04309628820326328; }
};

// The uniform B-spline of the order at the nodes i - ORDER / 2, i = 0 .. ORDER, for the fraction t in [0, 1), and its
// derivative: the pieces as polynomials in t, lowest power first, each coefficient the float nearest the fraction;
// evaluated by Horner's rule, one fused multiply-add per power.  At t = 0 the weights are the first column.
template <int ORDER> __host__ __device__ __forceinline__ void lk_spline_weights(float t, float (&w)[ORDER + 1], float (&g)[ORDER + 1]) {
  static_assert(ORDER == 3 || ORDER == 5, "cubic or quintic");
  if constexpr (ORDER == 3) {
    constexpr double a[4][4] = {{1.0 / 6, -1.0 / 2, 1.0 / 2, -1.0 / 6},
                                {2.0 / 3, 0.0, -1.0, 1.0 / 2},
                                {1.0 / 6, 1.0 / 2, 1.0 / 2, -1.0 / 2},
                                {0.0, 0.0, 0.0, 1.0 / 6}};
    constexpr double d[4][3] = {{-1.0 / 2, 1.0, -1.0 / 2}, {0.0, -2.0, 3.0 / 2}, {1.0 / 2, 1.0, -3.0 / 2}, {0.0, 0.0, 1.0 / 2}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf((float)a[i][3], t, (float)a[i][2]), t, (float)a[i][1]), t, (float)a[i][0]);
      g[i] = __builtin_fmaf(__builtin_fmaf((float)d[i][2], t, (float)d[i][1]), t, (float)d[i][0]);
    }
  } else {
    constexpr double a[6][6] = {{1.0 / 120, -1.0 / 24, 1.0 / 12, -1.0 / 12, 1.0 / 24, -1.0 / 120},
                                {13.0 / 60, -5.0 / 12, 1.0 / 6, 1.0 / 6, -1.0 / 6, 1.0 / 24},
                                {11.0 / 20, 0.0, -1.0 / 2, 0.0, 1.0 / 4, -1.0 / 12},
                                {13.0 / 60, 5.0 / 12, 1.0 / 6, -1.0 / 6, -1.0 / 6, 1.0 / 12},
                                {1.0 / 120, 1.0 / 24, 1.0 / 12, 1.0 / 12, 1.0 / 24, -1.0 / 24},
                                {0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / 120}};
    constexpr double d[6][5] = {{-1.0 / 24, 1.0 / 6, -1.0 / 4, 1.0 / 6, -1.0 / 24},
                                {-5.0 / 12, 1.0 / 3, 1.0 / 2, -2.0 / 3, 5.0 / 24},
                                {0.0, -1.0, 0.0, 1.0, -5.0 / 12},
                                {5.0 / 12, 1.0 / 3, -1.0 / 2, -2.0 / 3, 5.0 / 12},
                                {1.0 / 24, 1.0 / 6, 1.0 / 4, 1.0 / 6, -5.0 / 24},
                                {0.0, 0.0, 0.0, 0.0, 1.0 / 24}};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      float v = (float)a[i][5], q = (float)d[i][4];
#pragma unroll
      for (int k = 4; k >= 0; --k)
        v = __builtin_fmaf(v, t, (float)a[i][k]);
#pragma unroll
      for (int k = 3; k >= 0; --k)
        q = __builtin_fmaf(q, t, (float)d[i][k]);
      w[i] = v;
      g[i] = q;
    }
  }
}
