// lk_composed.cpp - host side of the composed refinement (include/lk_engine.h: lk_refine_composed,
// lk_composed_step_from_sums).  The kernels are lk_composed.hip and, for the first-order model under the engine's
// interpolator, lk_weighted.hip; the coefficient image is lk_spline.hip's.  lk_weighted.cpp and lk_quadratic.cpp in one call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_composed.hpp"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_spline.hpp"

namespace {

struct ComposedState : LkPassState {
  LkDevBytes rec, guess, second, order, count0, rec_out, out, sums;
  LkDevBytes first; // struct lk_weighted [S]: what the first-order kernels leave, widened into `out`
  LkDevBytes mask;  // uploaded by every call that has one: nothing is kept that could go stale
  LkDevBytes coef;  // the coefficient image, rebuilt by every call with a spline sampler
  std::vector<uint32_t> h_order;
  std::vector<int32_t> h_count0;
  int count[3] = {0, 0, 0};
  hipError_t init() { return LkPassState::init(false); } // (no cell grid: no bounding box to land)
};

static_assert(sizeof(struct lk_composed) == 128 && sizeof(lk_composed_config) == 64, "the records of the header");
static_assert(offsetof(struct lk_composed, bend) == offsetof(struct lk_quadratic, bend) &&
                  offsetof(struct lk_composed, n_valid) == offsetof(struct lk_quadratic, reserved),
              "struct lk_composed is struct lk_quadratic up to bend, the weights' words in its reserved ones");

constexpr int kCmDefaultIters = 50; // lk_refine_znssd's defaults
constexpr float kCmDefaultPrecision = 1e-3f;
constexpr float kCmDefaultLambda = 1e-3f;
constexpr double kLog2E = 1.4426950408889634; // log2(e)

} // namespace

extern "C" {

int lk_composed_step_from_sums(int order, int model, int n_valid, double N, const double *sums, float lambda, double *delta12, double *crit,
                               double *gain_offset2, int32_t *status) {
  if (!sums || !status || n_valid < 0 || !(N >= 0.0) || !std::isfinite(N) || !(lambda >= 0.f) || !std::isfinite(lambda))
    return LK_ERROR_BAD_DOMAIN;
  double delta[kLkQdParams];
  LkZnCriterion cr;
  const int st = lk_composed_step_from_sums_impl(order, model, n_valid, N, sums, (double)lambda, delta, &cr);
  if (st < 0)
    return LK_ERROR_BAD_DOMAIN;
  *status = st;
  if (delta12)
    for (int k = 0; k < kLkQdParams; ++k)
      delta12[k] = delta[k];
  if (crit)
    *crit = cr.crit;
  if (gain_offset2) {
    gain_offset2[0] = cr.gain;
    gain_offset2[1] = cr.offset;
  }
  return LK_ERROR_NONE;
}

int lk_refine_composed(lk_engine *e, const lk_composed_config *cfg, const uint8_t *mask, const lk_result *records, const float *guesses,
                       const float *second, lk_result *records_out, struct lk_composed *info_out, double *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: no configuration");
  if (!records_out && !info_out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: no output (records_out and info_out are both null)");
  for (int r : cfg->reserved)
    if (r != 0)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: reserved words must be 0");
  if (cfg->order != 1 && cfg->order != 2)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: order must be 1 (the engine's model) or 2 (twelve parameters)");
  if (cfg->sampler != 0 && cfg->sampler != 3 && cfg->sampler != 5)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_refine_composed: sampler must be 0 (the engine's interpolator), 3 or 5 (cubic or quintic B-spline)");
  if (second && cfg->order == 1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: second-order seeds are given with order 1");
  if (records && guesses)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: records and guesses are both given (seeds are one or the other)");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: chi_max must be finite (<= 0: the error code alone decides)");
  if (!std::isfinite(cfg->precision) || !std::isfinite(cfg->lambda0))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: precision and lambda0 must be finite (<= 0: the default)");
  if (!(cfg->sigma >= 0.f) || !std::isfinite(cfg->sigma))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: sigma must be finite and >= 0 (0: no window)");
  if (!(cfg->min_fraction >= 0.f && cfg->min_fraction <= 1.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: min_fraction must lie in [0, 1]");
  if (mask && (cfg->mask_rows <= 0 || cfg->mask_cols <= 0))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: a mask without dimensions (mask_rows, mask_cols)");
  if (!mask && (cfg->mask_rows != 0 || cfg->mask_cols != 0))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: mask dimensions without a mask (0, 0 with mask == NULL)");
  const bool held = !records && !guesses;
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_refine_composed", LK_VIEW_IMAGES | (held ? LK_VIEW_RECORDS : 0), cfg->def_slot, &v))
    return rc;
  if (mask && (cfg->mask_rows != v.urows || cfg->mask_cols != v.ucols))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_refine_composed: the mask dimensions are not those of the level-py_start undeformed image");
  if (cfg->sampler != 0 && (v.drows < kLkSplineMinSide || v.dcols < kLkSplineMinSide))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: the level image has a side below 8");
  float inv = 0.f;
  if (cfg->sigma > 0.f) {
    const double sigma_l = std::ldexp((double)cfg->sigma, -v.level);
    inv = (float)(kLog2E / (2.0 * sigma_l * sigma_l));
    if (!(inv > 0.f) || !std::isfinite(inv))
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_composed: sigma is outside the range a float window can have");
  }
  ComposedState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_COMPOSED, "hipEventCreate (lk_refine_composed)", &st))
    return rc;
  const bool second_order = cfg->order == 2;
  const size_t n = (size_t)v.S, n_sums = second_order ? (size_t)kLkQdSums : (size_t)kLkZnSums;
  lk_pass_order_by_group(v.h_rect0, v.h_off0, v.S, st->h_order, st->count);
  st->h_count0.resize(n);
  for (size_t s = 0; s < n; ++s) {
    const int4 r = v.h_rect0[s];
    st->h_count0[s] = r.z > 0 ? r.w : (int32_t)(v.h_off0[s + 1] - v.h_off0[s]);
  }
  LK_HIPCHK(st->order.ensure(n * sizeof(uint32_t)));
  LK_HIPCHK(st->count0.ensure(n * sizeof(int32_t)));
  LK_HIPCHK(st->rec_out.ensure(n * sizeof(lk_result)));
  LK_HIPCHK(st->out.ensure(n * sizeof(struct lk_composed)));
  if (!second_order)
    LK_HIPCHK(st->first.ensure(n * sizeof(struct lk_weighted)));
  if (sums_out)
    LK_HIPCHK(st->sums.ensure(n * n_sums * sizeof(double)));
  LK_HIPCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  LK_HIPCHK(hipMemcpyAsync(st->count0.p, st->h_count0.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
  if (mask) {
    const size_t bytes = (size_t)v.urows * (size_t)v.ucols;
    LK_HIPCHK(st->mask.ensure(bytes));
    LK_HIPCHK(hipMemcpyAsync(st->mask.p, mask, bytes, hipMemcpyHostToDevice, v.stream));
  }
  const lk_result *d_rec = guesses ? nullptr : v.result;
  if (int rc = lk_pass_records(e, st->rec, records, n, v.stream, &d_rec))
    return rc;
  if (guesses) {
    LK_HIPCHK(st->guess.ensure(n * 6 * sizeof(float)));
    LK_HIPCHK(hipMemcpyAsync(st->guess.p, guesses, n * 6 * sizeof(float), hipMemcpyHostToDevice, v.stream));
  }
  if (second) {
    LK_HIPCHK(st->second.ensure(n * 6 * sizeof(float)));
    LK_HIPCHK(hipMemcpyAsync(st->second.p, second, n * 6 * sizeof(float), hipMemcpyHostToDevice, v.stream));
  }
  if (cfg->sampler != 0)
    LK_HIPCHK(st->coef.ensure((size_t)v.drows * (size_t)v.dcols * sizeof(float)));
  const int max_iters = cfg->max_iters < 0 ? kCmDefaultIters : cfg->max_iters;
  const float precision = cfg->precision > 0.f ? cfg->precision : kCmDefaultPrecision;
  const float lambda0 = cfg->lambda0 > 0.f ? cfg->lambda0 : kCmDefaultLambda;
  LK_HIPCHK(st->begin(v.stream));
  if (cfg->sampler != 0)
    LK_HIPCHK(lk_launch_spline_build(cfg->sampler, v.def, v.drows, v.dcols, st->coef.as<float>(), v.stream));
  const uint32_t *order = st->order.as<uint32_t>();
  if (second_order) {
    LkComposedSecondArgs a{};
    a.qd.ev = lk_pass_sector_eval(v, d_rec);
    a.qd.guess = guesses ? st->guess.as<float>() : nullptr;
    a.qd.second = second ? st->second.as<float>() : nullptr;
    a.qd.count0 = st->count0.as<int32_t>();
    a.qd.rec_out = st->rec_out.as<lk_result>();
    a.qd.out = nullptr;
    a.qd.sums = sums_out ? st->sums.as<double>() : nullptr;
    a.qd.level = v.level;
    a.qd.model = v.model;
    a.qd.max_iters = max_iters;
    a.qd.chi_max = cfg->chi_max;
    a.qd.precision = precision;
    a.qd.lambda0 = lambda0;
    a.coef = cfg->sampler != 0 ? st->coef.as<float>() : nullptr;
    a.mask = mask ? st->mask.as<uint8_t>() : nullptr;
    a.out = st->out.as<struct lk_composed>();
    a.inv = inv;
    a.min_fraction = cfg->min_fraction;
    for (int g = 0; g < 3; ++g) {
      a.qd.ev.order = order;
      a.qd.n_sectors = st->count[g];
      if (a.qd.n_sectors > 0)
        LK_HIPCHK(lk_launch_composed_second(a, v.interp, cfg->sampler, kLkPassGroups[g], v.stream));
      order += st->count[g];
    }
  } else {
    LkComposedFirstArgs a{};
    a.wt.zn.ev = lk_pass_sector_eval(v, d_rec);
    a.wt.zn.guess = guesses ? st->guess.as<float>() : nullptr;
    a.wt.zn.count0 = st->count0.as<int32_t>();
    a.wt.zn.rec_out = st->rec_out.as<lk_result>();
    a.wt.zn.out = nullptr;
    a.wt.zn.sums = sums_out ? st->sums.as<double>() : nullptr;
    a.wt.zn.level = v.level;
    a.wt.zn.max_iters = max_iters;
    a.wt.zn.chi_max = cfg->chi_max;
    a.wt.zn.precision = precision;
    a.wt.zn.lambda0 = lambda0;
    a.wt.mask = mask ? st->mask.as<uint8_t>() : nullptr;
    a.wt.out = st->first.as<struct lk_weighted>();
    a.wt.inv = inv;
    a.wt.min_fraction = cfg->min_fraction;
    a.coef = cfg->sampler != 0 ? st->coef.as<float>() : nullptr;
    for (int g = 0; g < 3; ++g) {
      a.wt.zn.ev.order = order;
      a.wt.zn.n_sectors = st->count[g];
      if (a.wt.zn.n_sectors > 0) {
        if (cfg->sampler != 0)
          LK_HIPCHK(lk_launch_composed_first(a, v.model, cfg->sampler, kLkPassGroups[g], v.stream));
        else // exactly lk_refine_weighted's kernel
          LK_HIPCHK(lk_launch_weighted(a.wt, v.model, v.interp, kLkPassGroups[g], v.stream));
      }
      order += st->count[g];
    }
    const int n_par = v.model == LK_FM_U ? 1 : v.model == LK_FM_UV ? 2 : v.model == LK_FM_UVQ ? 3 : 6;
    LK_HIPCHK(lk_launch_composed_info(st->first.as<struct lk_weighted>(), st->rec_out.as<lk_result>(), n_par, v.S,
                                      st->out.as<struct lk_composed>(), v.stream));
  }
  LK_HIPCHK(st->end(v.stream));
  if (records_out)
    LK_HIPCHK(hipMemcpyAsync(records_out, st->rec_out.p, n * sizeof(lk_result), hipMemcpyDeviceToHost, v.stream));
  if (info_out)
    LK_HIPCHK(hipMemcpyAsync(info_out, st->out.p, n * sizeof(struct lk_composed), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    LK_HIPCHK(hipMemcpyAsync(sums_out, st->sums.p, n * n_sums * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_composed_last(lk_engine *e, float *device_ms, int *count3) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  ComposedState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_COMPOSED, "lk_internal_composed_last: no lk_refine_composed yet", device_ms, &st))
    return rc;
  if (count3)
    for (int g = 0; g < 3; ++g)
      count3[g] = st->count[g];
  return LK_ERROR_NONE;
}

} // extern "C"
