// lk_composed.cpp - host side of the composed refinement (include/lk_engine.h: lk_refine_composed, lk_composed_step_from_sums).
// The kernels are lk_composed.hip and, for the first-order model under the engine's interpolator, lk_weighted.hip; the
// coefficient image is lk_spline.hip's.  What lk_weighted.cpp and lk_quadratic.cpp take of lk_refine.hpp, in one call.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lk_engine.h"
#include "lk_composed.hpp"
#include "lk_launch.hpp"
#include "lk_refine.hpp"
#include "lk_spline.hpp"

namespace {

struct ComposedState : LkRefineState {
  LkDevBytes first; // struct lk_weighted [S]: what the first-order kernels leave, widened into `out`
  LkDevBytes coef;  // the coefficient image, rebuilt by every call with a spline sampler
};

static_assert(sizeof(struct lk_composed) == 128 && sizeof(lk_composed_config) == 64, "the records of the header");
static_assert(offsetof(struct lk_composed, bend) == offsetof(struct lk_quadratic, bend) &&
                  offsetof(struct lk_composed, n_valid) == offsetof(struct lk_quadratic, reserved),
              "struct lk_composed is struct lk_quadratic up to bend, the weights' words in its reserved ones");

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
  lk_refine_step_out(delta, kLkQdParams, cr, delta12, crit, gain_offset2);
  return LK_ERROR_NONE;
}

int lk_refine_composed(lk_engine *e, const lk_composed_config *cfg, const uint8_t *mask, const lk_result *records, const float *guesses,
                       const float *second, lk_result *records_out, struct lk_composed *info_out, double *sums_out) {
  LkRefineCall c{"lk_refine_composed", records, guesses, second, mask, records_out, info_out, sums_out, sizeof(struct lk_composed), 0};
  if (int rc = lk_refine_check_head(e, c, cfg))
    return rc;
  if (cfg->order != 1 && cfg->order != 2)
    return lk_refine_refuse(e, c, "order must be 1 (the engine's model) or 2 (twelve parameters)");
  if (cfg->sampler != 0 && cfg->sampler != 3 && cfg->sampler != 5)
    return lk_refine_refuse(e, c, "sampler must be 0 (the engine's interpolator), 3 or 5 (cubic or quintic B-spline)");
  if (second && cfg->order == 1)
    return lk_refine_refuse(e, c, "second-order seeds are given with order 1");
  c.sigma = cfg->sigma, c.min_fraction = cfg->min_fraction, c.mask_rows = cfg->mask_rows, c.mask_cols = cfg->mask_cols;
  if (int rc = lk_refine_check_view(e, c))
    return rc;
  const LkPassView &v = c.v;
  if (cfg->sampler != 0 && (v.drows < kLkSplineMinSide || v.dcols < kLkSplineMinSide))
    return lk_refine_refuse(e, c, "the level image has a side below 8");
  float inv;
  if (int rc = lk_refine_window(e, c, &inv))
    return rc;
  const bool second_order = cfg->order == 2;
  c.n_sums = second_order ? kLkQdSums : kLkZnSums;
  ComposedState *st = nullptr;
  if (int rc = lk_refine_prepare(e, c, LK_PASS_COMPOSED, "hipEventCreate (lk_refine_composed)", &st))
    return rc;
  if (!second_order)
    LK_HIPCHK(st->first.ensure((size_t)v.S * sizeof(struct lk_weighted)));
  if (cfg->sampler != 0)
    LK_HIPCHK(st->coef.ensure((size_t)v.drows * (size_t)v.dcols * sizeof(float)));
  const float *coef = cfg->sampler != 0 ? st->coef.as<float>() : nullptr;
  LK_HIPCHK(st->begin(v.stream));
  if (coef)
    LK_HIPCHK(lk_launch_spline_build(cfg->sampler, v.def, v.drows, v.dcols, st->coef.as<float>(), v.stream));
  if (second_order) {
    LkComposedSecondArgs a{};
    lk_refine_fill_second(a.qd, c, st);
    a.coef = coef;
    a.mask = c.d_mask;
    a.out = st->out.as<struct lk_composed>();
    a.inv = inv;
    a.min_fraction = c.min_fraction;
    LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), st->count, [&](int group, const uint32_t *order, int n_sectors) {
      a.qd.ev.order = order;
      a.qd.n_sectors = n_sectors;
      return lk_launch_composed_second(a, v.interp, cfg->sampler, group, v.stream);
    }));
  } else {
    LkComposedFirstArgs a{};
    lk_refine_fill(a.wt.zn, c, st);
    a.wt.mask = c.d_mask;
    a.wt.out = st->first.as<struct lk_weighted>();
    a.wt.inv = inv;
    a.wt.min_fraction = c.min_fraction;
    a.coef = coef;
    LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), st->count, [&](int group, const uint32_t *order, int n_sectors) {
      a.wt.zn.ev.order = order;
      a.wt.zn.n_sectors = n_sectors;
      return coef ? lk_launch_composed_first(a, v.model, cfg->sampler, group, v.stream)
                  : lk_launch_weighted(a.wt, v.model, v.interp, group, v.stream); // exactly lk_refine_weighted's kernel
    }));
    const int n_par = v.model == LK_FM_U ? 1 : v.model == LK_FM_UV ? 2 : v.model == LK_FM_UVQ ? 3 : 6;
    LK_HIPCHK(lk_launch_composed_info(st->first.as<struct lk_weighted>(), st->rec_out.as<lk_result>(), n_par, v.S,
                                      st->out.as<struct lk_composed>(), v.stream));
  }
  return lk_refine_finish(e, c, st);
}

// bench hook (lk_internal.hpp)
int lk_internal_composed_last(lk_engine *e, float *device_ms, int *count3) {
  return lk_pass_last_groups<LkRefineState>(e, LK_PASS_COMPOSED, "lk_internal_composed_last: no lk_refine_composed yet", device_ms, count3);
}

} // extern "C"
