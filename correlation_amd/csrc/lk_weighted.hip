// lk_weighted.hip - the weighted refinement pass (include/lk_engine.h: lk_refine_weighted).
//
// The loop is lk_znssd_loop.hpp with the engine's interpolator, as lk_znssd.hip, and a weight policy: the weight of a sample
// is the mask byte at its undeformed node (0 or 1) times the Gaussian window about the committed centre (lk_weighted.hpp).
// It is recomputed wherever it is needed - in the prologue and in every evaluation - from the sample alone: a byte load and
// a handful of fused multiply-adds beside a 16-tap sample, and nothing per sample is kept between evaluations.
#include "lk_launch.hpp"
#include "lk_weighted.hpp"
#include "lk_znssd_loop.hpp"

namespace {

template <int INTERP> struct WtImageSampler {
  __device__ __forceinline__ bool operator()(const SectorLevel &c, float xd, float yd, float &g, float &gx, float &gy) const {
    return sample_def<INTERP>(c.def, c.drows, c.dcols, xd, yd, g, gx, gy);
  }
};

struct WtMaskWindow {
  static constexpr bool kWeighted = true;
  gptr<uint8_t> mask; // [urows][ucols] or null
  struct lk_weighted *out;
  float inv, min_fraction;

  __device__ __forceinline__ float of(const SectorLevel &c, f32x2 q) const {
    if (mask) { // the node of sector_und_node
      int uix = (int)(q.x + 0.5f), uiy = (int)(q.y + 0.5f);
      uix = min(max(uix, 0), c.ucols - 1);
      uiy = min(max(uiy, 0), c.urows - 1);
      if (mask[(size_t)uiy * (size_t)c.ucols + (size_t)uix] == 0)
        return 0.f;
    }
    return inv > 0.f ? lk_window_weight(inv, q.x - c.cx, q.y - c.cy) : 1.f;
  }
  __device__ __forceinline__ bool too_few(int n_valid, int n) const { return (double)n_valid < (double)min_fraction * (double)n; }
  __device__ __forceinline__ void store(int s, const struct lk_znssd &o, const LkZnWeightSums &w, int level) const {
    struct lk_weighted r;
    r.n_points = o.n_points;
    r.status = o.status;
    r.iterations = o.iterations;
    r.evaluations = o.evaluations;
    r.zncc = o.zncc;
    r.gain = o.gain;
    r.offset = o.offset;
    r.znssd = o.znssd;
    r.zncc_seed = o.zncc_seed;
    r.shift = o.shift;
    r.lambda = o.lambda;
    r.last_step = o.last_step;
    r.n_valid = w.n_valid;
    r.weight_sum = (float)w.sw;
    const double scale = (double)(1 << level); // level-L pixels to level-0 pixels
    r.n_eff = r.centroid_dx = r.centroid_dy = 0.f;
    if (w.sw > 0.0) { // (else the sector has no weight: zeros, and nothing is divided)
      const double sq = w.sw * w.sw, cx = w.swx / w.sw, cy = w.swy / w.sw;
      r.n_eff = (float)(sq / w.sww);
      r.centroid_dx = (float)(cx * scale);
      r.centroid_dy = (float)(cy * scale);
    }
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    out[s] = r;
  }
};

template <int MODEL, int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_weighted_kernel(LkWeightedArgs a) {
  lk_znssd_sector<MODEL, GROUP>(a.zn, WtImageSampler<INTERP>{}, WtMaskWindow{(gptr<uint8_t>)a.mask, a.out, a.inv, a.min_fraction});
}

} // namespace

hipError_t lk_launch_weighted(const LkWeightedArgs &a, int model, int interp, int group, hipStream_t st) {
  return dispatch_sector_kernel(model, interp, group, [&](auto m, auto i, auto g) {
    constexpr int M = decltype(m)::value, I = decltype(i)::value, G = decltype(g)::value;
    return launch_sector_groups<G>(lk_weighted_kernel<M, I, G>, a, a.zn.n_sectors, st);
  });
}
