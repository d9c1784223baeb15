// lk_weighted.hip - the weighted refinement pass (include/lk_engine.h: lk_refine_weighted).
//
// The loop is lk_znssd_loop.hpp with the engine's interpolator, as lk_znssd.hip, and a weight policy (WtMaskWindow,
// lk_sector_policies.hpp, where lk_composed.hip finds it too): the weight of a sample
// is the mask byte at its undeformed node (0 or 1) times the Gaussian window about the committed centre (lk_weighted.hpp).
// It is recomputed wherever it is needed - in the prologue and in every evaluation - from the sample alone: a byte load and
// a handful of fused multiply-adds beside a 16-tap sample, and nothing per sample is kept between evaluations.
#include "lk_launch.hpp"
#include "lk_sector_policies.hpp" // WtImageSampler, WtMaskWindow
#include "lk_weighted.hpp"
#include "lk_znssd_loop.hpp"

namespace {

template <int MODEL, int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_weighted_kernel(LkWeightedArgs a) {
  lk_znssd_sector<MODEL, GROUP>(a.zn, WtImageSampler<INTERP>{}, WtMaskWindow<struct lk_weighted>{(gptr<uint8_t>)a.mask, a.out, a.inv, a.min_fraction});
}

} // namespace

hipError_t lk_launch_weighted(const LkWeightedArgs &a, int model, int interp, int group, hipStream_t st) {
  return dispatch_sector_kernel(model, interp, group, [&](auto m, auto i, auto g) {
    constexpr int M = decltype(m)::value, I = decltype(i)::value, G = decltype(g)::value;
    return launch_sector_groups<G>(lk_weighted_kernel<M, I, G>, a, a.zn.n_sectors, st);
  });
}
