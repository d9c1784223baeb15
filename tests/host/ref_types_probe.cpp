// ref_types_probe.cpp - TEST INFRASTRUCTURE: prints the values and the layout of the reference declarations that
// include/lk_cuda_class_adapter.hpp uses, one "name value" line each.  Compiled once against the reference's own
// enums.hpp / domains.hpp (tests/golden/make_golden.py -> tests/golden/ref_pins.npz) and, in the test suite, against
// tests/host/ref_min: the two outputs must be equal.
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "domains.hpp"
#include "enums.hpp"

#define V(x) std::printf("%s %ld\n", #x, static_cast<long>(x));

int main() {
  V(im_nearest) V(im_bilinear) V(im_bicubic) V(im_NUMBER_OF_ITEMS)
  V(fm_U) V(fm_UV) V(fm_UVQ) V(fm_UVUxUyVxVy) V(fm_NUMBER_OF_ITEMS)
  V(error_none) V(error_model_out_of_image) V(error_interpolation_out_of_image) V(error_correlation_max_iters_reached)
  V(error_bad_domain) V(error_cuSolver) V(error_cuda) V(error_multiThread) V(error_NUMBER_OF_ITEMS)
  V(color_monochrome) V(color_color) V(color_NUMBER_OF_ITEMS)
  V(def_strict_Lagrangian) V(def_Lagrangian) V(def_Eulerian) V(def_NUMBER_OF_ITEMS)
  V(sizeof(errorEnum))
  V(sizeof(CorrelationResult))
  V(offsetof(CorrelationResult, resultingParameters)) V(offsetof(CorrelationResult, chi))
  V(offsetof(CorrelationResult, numberOfPoints)) V(offsetof(CorrelationResult, iterations))
  V(offsetof(CorrelationResult, errorCode)) V(offsetof(CorrelationResult, undCenterX))
  V(offsetof(CorrelationResult, undCenterY))
  V((std::is_same<v_points, std::vector<std::pair<float, float>>>::value))
  return 0;
}
