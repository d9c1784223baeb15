// lk_composed.hpp - what the composed refinement's kernels and its host entry points share (include/lk_engine.h:
// lk_refine_composed, lk_composed_step_from_sums): how a sampler names a kernel instance, and the
// step of either order from a sector's sums - the functions of lk_znssd.hpp and lk_quadratic.hpp, nothing of its own.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lk_engine.h"
#include "lk_quadratic.hpp"
#include "lk_znssd.hpp"

// the SAMPLER of lk_composed_second_kernel: an LK_IM_* interpolator (0 .. 3), or this plus the spline order (3 or 5)
constexpr int kLkComposedSpline = 8;

// Returns -1 for an order that is not 1 or 2 or, with order 1, an unknown model (outputs untouched), else the status of
// lk_znssd_step (order 1; delta: zeros behind P) or lk_quadratic_step (order 2; the model plays no part).  delta12: 12 doubles.
inline int lk_composed_step_from_sums_impl(int order, int model, int n_valid, double N, const double *sums, double lambda, double *delta12,
                                           LkZnCriterion *cr) {
  if (order == 1) {
    double d6[6];
    const int st = lk_znssd_step_from_sums_impl(model, n_valid, N, sums, lambda, d6, cr);
    if (st < 0)
      return -1;
    for (int k = 0; k < kLkQdParams; ++k)
      delta12[k] = k < 6 ? d6[k] : 0.0;
    return st;
  }
  if (order != 2)
    return -1;
  double work[kLkQdWork];
  return lk_quadratic_step(n_valid, N, sums, lambda, delta12, cr, work);
}
