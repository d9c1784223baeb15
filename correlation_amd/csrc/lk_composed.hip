// lk_composed.hip - the composed refinement pass (include/lk_engine.h: lk_refine_composed): model
// order, deformed-image sampler and sample weights chosen independently.  No loop of its own: the two shared bodies
// (lk_znssd_loop.hpp, lk_quadratic_loop.hpp) with the policies of lk_sector_policies.hpp, always under WtMaskWindow.
//   order 1, a spline sampler    lk_znssd_sector: 4 models x 2 spline orders x 3 lane groups
//   order 2                      lk_quadratic_sector: (4 interpolators + 2 spline orders) x 3 lane groups
//   order 1, the interpolator    is lk_weighted_kernel (lk_launch_weighted); it is not instantiated a second time
// The first-order bodies leave struct lk_weighted; lk_composed_info_kernel widens it to struct lk_composed with the record's
// parameters.
#include "lk_composed.hpp"
#include "lk_launch.hpp"
#include "lk_quadratic_loop.hpp"
#include "lk_sector_policies.hpp"

namespace {

template <int MODEL, int ORDER, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_composed_first_kernel(LkComposedFirstArgs a) {
  // six parameters, the quintic's 36 nodes and the window in a 512-thread workgroup: 256 registers a lane, and the sampler's
  // loads scheduled all at once do not fit into what the 45 accumulators leave (28 bytes of scratch without the fence)
  constexpr bool FENCE = MODEL == LK_FM_UVUXUYVXVY && ORDER == 5 && GROUP == 512;
  lk_znssd_sector<MODEL, GROUP>(a.wt.zn, ZnSplineSampler<ORDER, FENCE>{(gptr<float>)a.coef},
                                WtMaskWindow<struct lk_weighted>{(gptr<uint8_t>)a.wt.mask, a.wt.out, a.wt.inv, a.wt.min_fraction});
}

// SAMPLER: an LK_IM_* interpolator, or kLkComposedSpline + the spline order
template <int SAMPLER, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_composed_second_kernel(LkComposedSecondArgs a) {
  const WtMaskWindow<struct lk_composed> weight{(gptr<uint8_t>)a.mask, a.out, a.inv, a.min_fraction};
  if constexpr (SAMPLER >= kLkComposedSpline)
    lk_quadratic_sector<GROUP>(a.qd, ZnSplineSampler<SAMPLER - kLkComposedSpline>{(gptr<float>)a.coef}, weight);
  else
    lk_quadratic_sector<GROUP>(a.qd, WtImageSampler<SAMPLER>{}, weight);
}

// struct lk_weighted [n] and the records written with them -> struct lk_composed [n] of a first-order call: p = the
// record's parameters (the engine model's P of them, level-0 scale; zeros for BAD_SEED and OUT_OF_IMAGE), bend = 0
__global__ void __launch_bounds__(256) lk_composed_info_kernel(const struct lk_weighted *in, const lk_result *rec, int n_par, int n,
                                                               struct lk_composed *out) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= n)
    return;
  const struct lk_weighted w = in[s];
  const lk_result r = rec[s];
  const bool evaluated = w.status != LK_ZN_BAD_SEED && w.status != LK_ZN_OUT_OF_IMAGE;
  struct lk_composed o;
  o.n_points = w.n_points;
  o.status = w.status;
  o.iterations = w.iterations;
  o.evaluations = w.evaluations;
#pragma unroll
  for (int i = 0; i < 12; ++i)
    o.p[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    o.p[i] = evaluated && i < n_par ? r.resultingParameters[i] : 0.f;
  o.zncc = w.zncc;
  o.gain = w.gain;
  o.offset = w.offset;
  o.znssd = w.znssd;
  o.zncc_seed = w.zncc_seed;
  o.shift = w.shift;
  o.lambda = w.lambda;
  o.last_step = w.last_step;
  o.bend = 0.f;
  o.n_valid = w.n_valid;
  o.weight_sum = w.weight_sum;
  o.n_eff = w.n_eff;
  o.centroid_dx = w.centroid_dx;
  o.centroid_dy = w.centroid_dy;
  o.reserved[0] = o.reserved[1] = 0;
  out[s] = o;
}

template <class F> hipError_t dispatch_spline(int order, F &&f) {
  return order == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 5>{});
}

} // namespace

hipError_t lk_launch_composed_first(const LkComposedFirstArgs &a, int model, int spline, int group, hipStream_t st) {
  return dispatch_model(model, [&](auto m) {
    return dispatch_spline(spline, [&](auto o) {
      return dispatch_group(group, [&](auto g) {
        constexpr int M = decltype(m)::value, O = decltype(o)::value, G = decltype(g)::value;
        return launch_sector_groups<G>(lk_composed_first_kernel<M, O, G>, a, a.wt.zn.n_sectors, st);
      });
    });
  });
}

hipError_t lk_launch_composed_second(const LkComposedSecondArgs &a, int interp, int spline, int group, hipStream_t st) {
  if (spline != 0)
    return dispatch_spline(spline, [&](auto o) {
      return dispatch_group(group, [&](auto g) {
        constexpr int O = decltype(o)::value, G = decltype(g)::value;
        return launch_sector_groups<G>(lk_composed_second_kernel<kLkComposedSpline + O, G>, a, a.qd.n_sectors, st);
      });
    });
  return dispatch_interp(interp, [&](auto i) {
    return dispatch_group(group, [&](auto g) {
      constexpr int I = decltype(i)::value, G = decltype(g)::value;
      return launch_sector_groups<G>(lk_composed_second_kernel<I, G>, a, a.qd.n_sectors, st);
    });
  });
}

hipError_t lk_launch_composed_info(const struct lk_weighted *in, const lk_result *rec, int n_par, int n, struct lk_composed *out,
                                   hipStream_t st) {
  if (n <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(lk_composed_info_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, rec, n_par, n, out);
  return hipGetLastError();
}
