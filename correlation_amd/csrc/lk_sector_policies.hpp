// lk_sector_policies.hpp - the samplers and the weight policy of the refinement loops (lk_znssd_loop.hpp,
// lk_quadratic_loop.hpp), in one header so that every pass can combine them: lk_spline.hip, lk_weighted.hip, lk_quadratic.hip
// and lk_composed.hip (DESIGN.md sections 25 to 27).  Device only.
//   WtImageSampler<INTERP>   the engine's interpolator on the deformed level image
//   ZnSplineSampler<ORDER>   the cubic or quintic B-spline of a coefficient image (lk_launch_spline_build)
//   WtMaskWindow<INFO>       w = mask(node) * window(q - centre); the info record goes out as INFO: struct lk_weighted from
//                            the first-order loop, struct lk_composed from the second-order loop
#pragma once
#include "lk_sector_eval.hpp"
#include "lk_spline.hpp"
#include "lk_weighted.hpp"
#include "lk_znssd_loop.hpp"

namespace {

template <int INTERP> struct WtImageSampler {
  __device__ __forceinline__ bool operator()(const SectorLevel &c, float xd, float yd, float &g, float &gx, float &gy) const {
    return sample_def<INTERP>(c.def, c.drows, c.dcols, xd, yd, g, gx, gy);
  }
};

// The spline of the coefficients and its gradient at (xd, yd); false where the window of ORDER + 1 nodes a side is not
// inside the image by the bicubic's rule (order 3) or one pixel further in (order 5).  Per image row a value and an
// x-derivative, each a chain of fused multiply-adds from the left; the rows are folded into W, Wx, Wy as they arrive.
// FENCE: the instruction scheduler may not move anything across the end of an image row, so the loads of at most one row
// are in flight - the same instructions on the same values, in fewer registers (lk_composed.hip says which instance asks).
template <int ORDER, bool FENCE = false>
__device__ __forceinline__ bool spline_sample(gptr<float> coef, int rows, int cols, float xd, float yd, float &W, float &Wx, float &Wy) {
  constexpr int NT = ORDER + 1, L = ORDER / 2;
  if (!(xd > (float)L && yd > (float)L && xd < (float)cols - (float)(L + 1) && yd < (float)rows - (float)(L + 1)))
    return false;
  const int ix = (int)xd, iy = (int)yd;
  const float tx = xd - (float)ix, ty = yd - (float)iy;
  float wx[NT], gx[NT], wy[NT], gy[NT];
  lk_spline_weights<ORDER>(tx, wx, gx);
  lk_spline_weights<ORDER>(ty, wy, gy);
  gptr<float> base = coef + (size_t)(iy - L) * (size_t)cols + (size_t)(ix - L);
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    gptr<float> r = base + (size_t)j * (size_t)cols;
    float v = wx[0] * r[0], d = gx[0] * r[0];
#pragma unroll
    for (int i = 1; i < NT; ++i) {
      v = __builtin_fmaf(wx[i], r[i], v);
      d = __builtin_fmaf(gx[i], r[i], d);
    }
    if (j == 0) {
      W = wy[0] * v;
      Wx = wy[0] * d;
      Wy = gy[0] * v;
    } else {
      W = __builtin_fmaf(wy[j], v, W);
      Wx = __builtin_fmaf(wy[j], d, Wx);
      Wy = __builtin_fmaf(gy[j], v, Wy);
    }
    if constexpr (FENCE)
      __builtin_amdgcn_sched_barrier(0);
  }
  return true;
}

template <int ORDER, bool FENCE = false> struct ZnSplineSampler {
  gptr<float> coef; // [drows][dcols] of the sector's deformed level image
  __device__ __forceinline__ bool operator()(const SectorLevel &c, float xd, float yd, float &g, float &gx, float &gy) const {
    return spline_sample<ORDER, FENCE>(coef, c.drows, c.dcols, xd, yd, g, gx, gy);
  }
};

template <class INFO> struct WtMaskWindow {
  static constexpr bool kWeighted = true;
  gptr<uint8_t> mask; // [urows][ucols] or null
  INFO *out;
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
  // the weights' words of either info record
  __device__ __forceinline__ void fill(INFO &r, const LkZnWeightSums &w, int level) const {
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
  }
  // from lk_znssd_sector: INFO = struct lk_weighted
  __device__ __forceinline__ void store(int s, const struct lk_znssd &o, const LkZnWeightSums &w, int level) const {
    INFO r;
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
    fill(r, w, level);
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    out[s] = r;
  }
  // from lk_quadratic_sector: INFO = struct lk_composed, struct lk_quadratic's words up to bend and the weights' behind them
  __device__ __forceinline__ void store(int s, const struct lk_quadratic &o, const LkZnWeightSums &w, int level) const {
    INFO r;
    r.n_points = o.n_points;
    r.status = o.status;
    r.iterations = o.iterations;
    r.evaluations = o.evaluations;
#pragma unroll
    for (int i = 0; i < 12; ++i)
      r.p[i] = o.p[i];
    r.zncc = o.zncc;
    r.gain = o.gain;
    r.offset = o.offset;
    r.znssd = o.znssd;
    r.zncc_seed = o.zncc_seed;
    r.shift = o.shift;
    r.lambda = o.lambda;
    r.last_step = o.last_step;
    r.bend = o.bend;
    fill(r, w, level);
    r.reserved[0] = r.reserved[1] = 0;
    out[s] = r;
  }
};

} // namespace
