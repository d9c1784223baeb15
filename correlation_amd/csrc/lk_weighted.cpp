// lk_weighted.cpp - host side of the weighted refinement (include/lk_engine.h: lk_refine_weighted, lk_weight_window,
// lk_weighted_step_from_sums).  The kernel is lk_weighted.hip; the window is lk_weighted.hpp; the loop, criterion and step
// are lk_refine_znssd's (lk_znssd_loop.hpp, lk_znssd.hpp) with the sum of the weights in place of the sample count.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_refine.hpp"
#include "lk_weighted.hpp"
#include "lk_znssd.hpp"

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
  lk_refine_step_out(delta, 6, cr, delta6, crit, gain_offset2);
  return LK_ERROR_NONE;
}

int lk_refine_weighted(lk_engine *e, const lk_weighted_config *cfg, const uint8_t *mask, const lk_result *records, const float *guesses,
                       lk_result *records_out, struct lk_weighted *info_out, double *sums_out) {
  LkRefineCall c{"lk_refine_weighted", records, guesses, nullptr, mask, records_out, info_out, sums_out, sizeof(struct lk_weighted), kLkZnSums};
  if (int rc = lk_refine_check_head(e, c, cfg))
    return rc;
  c.sigma = cfg->sigma, c.min_fraction = cfg->min_fraction, c.mask_rows = cfg->mask_rows, c.mask_cols = cfg->mask_cols;
  if (int rc = lk_refine_check_view(e, c))
    return rc;
  LkWeightedArgs a{};
  if (int rc = lk_refine_window(e, c, &a.inv))
    return rc;
  LkRefineState *st = nullptr;
  if (int rc = lk_refine_prepare(e, c, LK_PASS_WEIGHTED, "hipEventCreate (lk_refine_weighted)", &st))
    return rc;
  lk_refine_fill(a.zn, c, st);
  a.mask = c.d_mask;
  a.out = st->out.as<struct lk_weighted>();
  a.min_fraction = c.min_fraction;
  LK_HIPCHK(st->begin(c.v.stream));
  LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), st->count, [&](int group, const uint32_t *order, int n) {
    a.zn.ev.order = order;
    a.zn.n_sectors = n;
    return lk_launch_weighted(a, c.v.model, c.v.interp, group, c.v.stream);
  }));
  return lk_refine_finish(e, c, st);
}

// bench hook (lk_internal.hpp)
int lk_internal_weighted_last(lk_engine *e, float *device_ms, int *count3) {
  return lk_pass_last_groups<LkRefineState>(e, LK_PASS_WEIGHTED, "lk_internal_weighted_last: no lk_refine_weighted yet", device_ms, count3);
}

} // extern "C"
