// lk_znssd.cpp - host side of the ZNSSD refinement (include/lk_engine.h: lk_refine_znssd, lk_znssd_step_from_sums).  The
// kernel is lk_znssd.hip; criterion and step are lk_znssd.hpp; what the call does around its launches is lk_refine.hpp.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_refine.hpp"
#include "lk_znssd.hpp"

// (the table of level-0 counts grows through it; the passes' units inline it, and the library goes on exporting it)
template void std::vector<int32_t>::resize(std::vector<int32_t>::size_type);

extern "C" {

int lk_znssd_step_from_sums(int model, int n, const double *sums, float lambda, double *delta6, double *crit, double *gain_offset2,
                            int32_t *status) {
  if (!sums || !status || n < 0 || !(lambda >= 0.f) || !std::isfinite(lambda))
    return LK_ERROR_BAD_DOMAIN;
  double delta[6];
  LkZnCriterion cr;
  const int st = lk_znssd_step_from_sums_impl(model, n, sums, (double)lambda, delta, &cr);
  if (st < 0)
    return LK_ERROR_BAD_DOMAIN;
  *status = st;
  lk_refine_step_out(delta, 6, cr, delta6, crit, gain_offset2);
  return LK_ERROR_NONE;
}

int lk_refine_znssd(lk_engine *e, const lk_znssd_config *cfg, const lk_result *records, const float *guesses, lk_result *records_out,
                    struct lk_znssd *info_out, double *sums_out) {
  LkRefineCall c{"lk_refine_znssd", records, guesses, nullptr, nullptr, records_out, info_out, sums_out, sizeof(struct lk_znssd), kLkZnSums};
  if (int rc = lk_refine_check_head(e, c, cfg))
    return rc;
  if (int rc = lk_refine_check_view(e, c))
    return rc;
  LkRefineState *st = nullptr;
  if (int rc = lk_refine_prepare(e, c, LK_PASS_ZNSSD, "hipEventCreate (lk_refine_znssd)", &st))
    return rc;
  LkZnssdArgs a{};
  lk_refine_fill(a, c, st);
  a.out = st->out.as<struct lk_znssd>();
  LK_HIPCHK(st->begin(c.v.stream));
  LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), st->count, [&](int group, const uint32_t *order, int n) {
    a.ev.order = order;
    a.n_sectors = n;
    return lk_launch_znssd(a, c.v.model, c.v.interp, group, c.v.stream);
  }));
  return lk_refine_finish(e, c, st);
}

// bench hook (lk_internal.hpp)
int lk_internal_znssd_last(lk_engine *e, float *device_ms, int *count3) {
  return lk_pass_last_groups<LkRefineState>(e, LK_PASS_ZNSSD, "lk_internal_znssd_last: no lk_refine_znssd yet", device_ms, count3);
}

} // extern "C"
