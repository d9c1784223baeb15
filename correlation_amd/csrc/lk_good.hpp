// lk_good.hpp - the "good" rule of a record (include/lk_engine.h, recovery pass): one device function for every kernel
// that asks whether a sector's record can be trusted (lk_reseed.hip, lk_strain.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lk_engine.h"

__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// include/lk_engine.h, "good": error_none, finite parameters and chi, chi <= chi_max when chi_max > 0
__device__ inline bool reseed_good(const lk_result &r, int n_params, float chi_max) {
  if (r.errorCode != LK_ERROR_NONE || !finite_bits(r.chi))
    return false;
  for (int i = 0; i < n_params; ++i)
    if (!finite_bits(r.resultingParameters[i]))
      return false;
  return !(chi_max > 0.f) || r.chi <= chi_max;
}

__device__ inline int n_params_of(int model) {
  return model == LK_FM_U ? 1 : model == LK_FM_UV ? 2 : model == LK_FM_UVQ ? 3 : 6;
}
