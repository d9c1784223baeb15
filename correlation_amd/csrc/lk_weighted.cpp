// lk_weighted.cpp - host side of the weighted refinement (include/lk_engine.h: lk_refine_weighted, lk_weight_window,
// lk_weighted_step_from_sums).  The kernel is lk_weighted.hip; the window is lk_weighted.hpp; the loop, criterion and step
// are lk_refine_znssd's (lk_znssd_loop.hpp, lk_znssd.hpp) with the sum of the weights in place of the sample count.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_weighted.hpp"
#include "lk_znssd.hpp"

namespace {

struct WeightedState : LkPassState {
  LkDevBytes rec, guess, order, count0, rec_out, out, sums;
  LkDevBytes mask; // uploaded by every call that has one: nothing is kept that could go stale
  std::vector<uint32_t> h_order;
  std::vector<int32_t> h_count0;
  int count[3] = {0, 0, 0};
  hipError_t init() { return LkPassState::init(false); } // (no cell grid: no bounding box to land)
};

constexpr int kWtDefaultIters = 50; // lk_refine_znssd's defaults
constexpr float kWtDefaultPrecision = 1e-3f;
constexpr float kWtDefaultLambda = 1e-3f;
constexpr double kLog2E = 1.4426950408889634; // log2(e)

} // namespace

extern "C" {

int lk_weight_window(float inv, float dx, float dy, float *w) {
  if (!w || !(inv >= 0.f) || !std::isfinite(inv) || !std::isfinite(dx) || !std::isfinite(dy))
    return LK_ERROR_BAD_DOMAIN;
  *w = lk_window_weight(inv, dx, dy);
  return LK_ERROR_NONE;
}

int lk_weighted_step_from_sums(int model, int n_valid, double N, const double *sums, float lambda, double *delta6, double *crit,
                               double *gain_offset2, int32_t *status) {
  if (!sums || !status || n_valid < 0 || !(N >= 0.0) || !std::isfinite(N) || !(lambda >= 0.f) || !std::isfinite(lambda))
    return LK_ERROR_BAD_DOMAIN;
  double delta[6];
  LkZnCriterion cr;
  const int st = lk_znssd_step_from_sums_impl(model, n_valid, N, sums, (double)lambda, delta, &cr);
  if (st < 0)
    return LK_ERROR_BAD_DOMAIN;
  *status = st;
  if (delta6)
    for (int k = 0; k < 6; ++k)
      delta6[k] = delta[k];
  if (crit)
    *crit = cr.crit;
  if (gain_offset2) {
    gain_offset2[0] = cr.gain;
    gain_offset2[1] = cr.offset;
  }
  return LK_ERROR_NONE;
}

int lk_refine_weighted(lk_engine *e, const lk_weighted_config *cfg, const uint8_t *mask, const lk_result *records, const float *guesses,
                       lk_result *records_out, struct lk_weighted *info_out, double *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: no configuration");
  if (!records_out && !info_out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: no output (records_out and info_out are both null)");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: reserved words must be 0");
  if (records && guesses)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: records and guesses are both given (seeds are one or the other)");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: chi_max must be finite (<= 0: the error code alone decides)");
  if (!std::isfinite(cfg->precision) || !std::isfinite(cfg->lambda0))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: precision and lambda0 must be finite (<= 0: the default)");
  if (!(cfg->sigma >= 0.f) || !std::isfinite(cfg->sigma))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: sigma must be finite and >= 0 (0: no window)");
  if (!(cfg->min_fraction >= 0.f && cfg->min_fraction <= 1.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: min_fraction must lie in [0, 1]");
  if (mask && (cfg->mask_rows <= 0 || cfg->mask_cols <= 0))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: a mask without dimensions (mask_rows, mask_cols)");
  if (!mask && (cfg->mask_rows != 0 || cfg->mask_cols != 0))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: mask dimensions without a mask (0, 0 with mask == NULL)");
  const bool held = !records && !guesses;
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_refine_weighted", LK_VIEW_IMAGES | (held ? LK_VIEW_RECORDS : 0), cfg->def_slot, &v))
    return rc;
  if (mask && (cfg->mask_rows != v.urows || cfg->mask_cols != v.ucols))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_refine_weighted: the mask dimensions are not those of the level-py_start undeformed image");
  float inv = 0.f;
  if (cfg->sigma > 0.f) {
    const double sigma_l = std::ldexp((double)cfg->sigma, -v.level);
    inv = (float)(kLog2E / (2.0 * sigma_l * sigma_l));
    if (!(inv > 0.f) || !std::isfinite(inv))
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_weighted: sigma is outside the range a float window can have");
  }
  WeightedState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_WEIGHTED, "hipEventCreate (lk_refine_weighted)", &st))
    return rc;
  const size_t n = (size_t)v.S;
  lk_pass_order_by_group(v.h_rect0, v.h_off0, v.S, st->h_order, st->count);
  st->h_count0.resize(n);
  for (size_t s = 0; s < n; ++s) {
    const int4 r = v.h_rect0[s];
    st->h_count0[s] = r.z > 0 ? r.w : (int32_t)(v.h_off0[s + 1] - v.h_off0[s]);
  }
  LK_HIPCHK(st->order.ensure(n * sizeof(uint32_t)));
  LK_HIPCHK(st->count0.ensure(n * sizeof(int32_t)));
  LK_HIPCHK(st->rec_out.ensure(n * sizeof(lk_result)));
  LK_HIPCHK(st->out.ensure(n * sizeof(struct lk_weighted)));
  if (sums_out)
    LK_HIPCHK(st->sums.ensure(n * kLkZnSums * sizeof(double)));
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
  LkWeightedArgs a{};
  a.zn.ev = lk_pass_sector_eval(v, d_rec);
  a.zn.guess = guesses ? st->guess.as<float>() : nullptr;
  a.zn.count0 = st->count0.as<int32_t>();
  a.zn.rec_out = st->rec_out.as<lk_result>();
  a.zn.out = nullptr;
  a.zn.sums = sums_out ? st->sums.as<double>() : nullptr;
  a.zn.level = v.level;
  a.zn.max_iters = cfg->max_iters < 0 ? kWtDefaultIters : cfg->max_iters;
  a.zn.chi_max = cfg->chi_max;
  a.zn.precision = cfg->precision > 0.f ? cfg->precision : kWtDefaultPrecision;
  a.zn.lambda0 = cfg->lambda0 > 0.f ? cfg->lambda0 : kWtDefaultLambda;
  a.mask = mask ? st->mask.as<uint8_t>() : nullptr;
  a.out = st->out.as<struct lk_weighted>();
  a.inv = inv;
  a.min_fraction = cfg->min_fraction;
  LK_HIPCHK(st->begin(v.stream));
  const uint32_t *order = st->order.as<uint32_t>();
  for (int g = 0; g < 3; ++g) {
    a.zn.ev.order = order;
    a.zn.n_sectors = st->count[g];
    if (a.zn.n_sectors > 0)
      LK_HIPCHK(lk_launch_weighted(a, v.model, v.interp, kLkPassGroups[g], v.stream));
    order += st->count[g];
  }
  LK_HIPCHK(st->end(v.stream));
  if (records_out)
    LK_HIPCHK(hipMemcpyAsync(records_out, st->rec_out.p, n * sizeof(lk_result), hipMemcpyDeviceToHost, v.stream));
  if (info_out)
    LK_HIPCHK(hipMemcpyAsync(info_out, st->out.p, n * sizeof(struct lk_weighted), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    LK_HIPCHK(hipMemcpyAsync(sums_out, st->sums.p, n * kLkZnSums * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_weighted_last(lk_engine *e, float *device_ms, int *count3) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  WeightedState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_WEIGHTED, "lk_internal_weighted_last: no lk_refine_weighted yet", device_ms, &st))
    return rc;
  if (count3)
    for (int g = 0; g < 3; ++g)
      count3[g] = st->count[g];
  return LK_ERROR_NONE;
}

} // extern "C"
