// lk_quadratic.hip - the second-order refinement pass (include/lk_engine.h: lk_refine_quadratic).
//
// The loop is lk_quadratic_loop.hpp - twelve parameters, 88 sums in three sweeps, the step in LDS; its header comment says
// why - with the engine's interpolator and unit weights: nothing of a weight is compiled into this kernel.
#include "lk_launch.hpp"
#include "lk_quadratic_loop.hpp"
#include "lk_sector_policies.hpp"

namespace {

template <int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_quadratic_kernel(LkQuadraticArgs a) {
  lk_quadratic_sector<GROUP>(a, WtImageSampler<INTERP>{}, LkZnUnitWeight{});
}

} // namespace

hipError_t lk_launch_quadratic(const LkQuadraticArgs &a, int interp, int group, hipStream_t st) {
  return dispatch_interp(interp, [&](auto i) {
    return dispatch_group(group, [&](auto g) {
      constexpr int I = decltype(i)::value, G = decltype(g)::value;
      return launch_sector_groups<G>(lk_quadratic_kernel<I, G>, a, a.n_sectors, st);
    });
  });
}
