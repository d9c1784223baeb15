// lk_znssd.hip - the ZNSSD refinement pass (include/lk_engine.h: lk_refine_znssd).
//
// The loop - one lane group carries one sector from its seed to its record - is lk_znssd_loop.hpp, shared with
// lk_spline.hip; this file gives it the engine's interpolator, sample_def<> on the deformed level image.
#include "lk_launch.hpp"
#include "lk_znssd_loop.hpp"

namespace {

template <int INTERP> struct ZnImageSampler {
  __device__ __forceinline__ bool operator()(const SectorLevel &c, float xd, float yd, float &g, float &gx, float &gy) const {
    return sample_def<INTERP>(c.def, c.drows, c.dcols, xd, yd, g, gx, gy);
  }
};

template <int MODEL, int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_znssd_kernel(LkZnssdArgs a) {
  lk_znssd_sector<MODEL, GROUP>(a, ZnImageSampler<INTERP>{}, LkZnUnitWeight{});
}

} // namespace

hipError_t lk_launch_znssd(const LkZnssdArgs &a, int model, int interp, int group, hipStream_t st) {
  return dispatch_sector_kernel(model, interp, group, [&](auto m, auto i, auto g) {
    constexpr int M = decltype(m)::value, I = decltype(i)::value, G = decltype(g)::value;
    return launch_sector_groups<G>(lk_znssd_kernel<M, I, G>, a, a.n_sectors, st);
  });
}
