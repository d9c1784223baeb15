// lk_uncertainty.cpp - host side of the per-sector uncertainty (include/lk_engine.h: lk_parameter_uncertainty,
// lk_uncertainty_from_sums).  The kernel is lk_uncertainty.hip; the record's arithmetic is lk_uncertainty.hpp.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_uncertainty.hpp"

namespace {

struct UncertaintyState : LkPassState {
  LkDevBytes rec, order, out, sums;
  std::vector<uint32_t> h_order;
  int count[3] = {0, 0, 0};
  hipError_t init() { return LkPassState::init(false); } // (no cell grid: no bounding box to land)
};

} // namespace

extern "C" {

int lk_uncertainty_from_sums(int model, int n, const double *sums28, int level, lk_uncertainty *out) {
  if (!sums28 || !out || lk_uncertainty_from_sums_impl(model, n, sums28, level, out) != 0)
    return LK_ERROR_BAD_DOMAIN;
  return LK_ERROR_NONE;
}

int lk_parameter_uncertainty(lk_engine *e, const lk_uncertainty_config *cfg, const lk_result *records, lk_uncertainty *out,
                             double *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_parameter_uncertainty: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_parameter_uncertainty: no output");
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_parameter_uncertainty", LK_VIEW_IMAGES | (records ? 0 : LK_VIEW_RECORDS), cfg->def_slot, &v))
    return rc;
  UncertaintyState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_UNCERTAINTY, "hipEventCreate (lk_parameter_uncertainty)", &st))
    return rc;
  const size_t n = (size_t)v.S;
  lk_pass_order_by_group(v.h_rect0, v.h_off0, v.S, st->h_order, st->count);
  LK_HIPCHK(st->order.ensure(n * sizeof(uint32_t)));
  LK_HIPCHK(st->out.ensure(n * sizeof(lk_uncertainty)));
  if (sums_out)
    LK_HIPCHK(st->sums.ensure(n * kLkUncSums * sizeof(double)));
  LK_HIPCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  const lk_result *d_rec = v.result;
  if (int rc = lk_pass_records(e, st->rec, records, n, v.stream, &d_rec))
    return rc;
  LkUncertaintyArgs a{};
  a.ev = lk_pass_sector_eval(v, d_rec);
  a.level = v.level;
  a.out = st->out.as<lk_uncertainty>();
  a.sums = sums_out ? st->sums.as<double>() : nullptr;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), st->count, [&](int group, const uint32_t *order, int n_sectors) {
    a.ev.order = order;
    a.n_sectors = n_sectors;
    return lk_launch_uncertainty(a, v.model, v.interp, group, v.stream);
  }));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(lk_uncertainty), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    LK_HIPCHK(hipMemcpyAsync(sums_out, st->sums.p, n * kLkUncSums * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_uncertainty_last(lk_engine *e, float *device_ms, int *count3) {
  return lk_pass_last_groups<UncertaintyState>(e, LK_PASS_UNCERTAINTY, "lk_internal_uncertainty_last: no lk_parameter_uncertainty yet", device_ms,
                                               count3);
}

} // extern "C"
