// lk_quadratic.cpp - host side of the second-order refinement (include/lk_engine.h: lk_refine_quadratic,
// lk_quadratic_step_from_sums).  The kernel is lk_quadratic.hip; criterion and step are lk_quadratic.hpp.  lk_znssd.cpp
// with one more input, the second-order seeds.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_quadratic.hpp"
#include "lk_refine.hpp"

static_assert(sizeof(struct lk_quadratic) == 128 && sizeof(lk_quadratic_config) == 32, "the records of the header");

extern "C" {

int lk_quadratic_step_from_sums(int n, const double *sums88, float lambda, double *delta12, double *crit, double *gain_offset2,
                                int32_t *status) {
  if (!sums88 || !status || n < 0 || !(lambda >= 0.f) || !std::isfinite(lambda))
    return LK_ERROR_BAD_DOMAIN;
  double delta[kLkQdParams], work[kLkQdWork];
  LkZnCriterion cr;
  *status = lk_quadratic_step(n, sums88, (double)lambda, delta, &cr, work);
  lk_refine_step_out(delta, kLkQdParams, cr, delta12, crit, gain_offset2);
  return LK_ERROR_NONE;
}

int lk_refine_quadratic(lk_engine *e, const lk_quadratic_config *cfg, const lk_result *records, const float *guesses, const float *second,
                        lk_result *records_out, struct lk_quadratic *info_out, double *sums_out) {
  LkRefineCall c{"lk_refine_quadratic", records, guesses, second, nullptr, records_out, info_out, sums_out, sizeof(struct lk_quadratic),
                 kLkQdSums};
  if (int rc = lk_refine_check_head(e, c, cfg))
    return rc;
  if (int rc = lk_refine_check_view(e, c))
    return rc;
  LkRefineState *st = nullptr;
  if (int rc = lk_refine_prepare(e, c, LK_PASS_QUADRATIC, "hipEventCreate (lk_refine_quadratic)", &st))
    return rc;
  LkQuadraticArgs a{};
  lk_refine_fill_second(a, c, st);
  a.out = st->out.as<struct lk_quadratic>();
  LK_HIPCHK(st->begin(c.v.stream));
  LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), st->count, [&](int group, const uint32_t *order, int n) {
    a.ev.order = order;
    a.n_sectors = n;
    return lk_launch_quadratic(a, c.v.interp, group, c.v.stream);
  }));
  return lk_refine_finish(e, c, st);
}

// bench hook (lk_internal.hpp)
int lk_internal_quadratic_last(lk_engine *e, float *device_ms, int *count3) {
  return lk_pass_last_groups<LkRefineState>(e, LK_PASS_QUADRATIC, "lk_internal_quadratic_last: no lk_refine_quadratic yet", device_ms, count3);
}

} // extern "C"
