// lk_uncertainty.cpp - host side of the per-sector uncertainty (include/lk_engine.h: lk_parameter_uncertainty,
// lk_uncertainty_from_sums).  The kernel is lk_uncertainty.hip; the record's arithmetic is lk_uncertainty.hpp.
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_cell_grid.hpp"
#include "lk_device.hpp"
#include "lk_internal.hpp"
#include "lk_launch.hpp"
#include "lk_uncertainty.hpp"

#define UNCHK(call)                                                                                   \
  do {                                                                                                \
    hipError_t _e = (call);                                                                           \
    if (_e != hipSuccess)                                                                             \
      return lk_internal_hipfail(e, _e, #call);                                                       \
  } while (0)

namespace {

constexpr int kGroups[3] = {16, 64, 512};

struct UncertaintyState {
  LkDevBytes rec, order, out, sums;
  std::vector<uint32_t> h_order;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false; // ev0 / ev1 bracket the kernels of a finished call (read by lk_internal_uncertainty_last)
  int count[3] = {0, 0, 0};
};

int get_state(lk_engine *e, UncertaintyState **out) {
  void **slot = lk_internal_uncertainty_slot(e);
  if (!*slot) {
    UncertaintyState *st = new UncertaintyState();
    hipError_t err = hipEventCreate(&st->ev0);
    if (err == hipSuccess)
      err = hipEventCreate(&st->ev1);
    if (err != hipSuccess) {
      lk_internal_uncertainty_release(st);
      return lk_internal_hipfail(e, err, "hipEventCreate (lk_parameter_uncertainty)");
    }
    *slot = st;
  }
  *out = (UncertaintyState *)*slot;
  return LK_ERROR_NONE;
}

} // namespace

void lk_internal_uncertainty_release(void *state) {
  UncertaintyState *st = (UncertaintyState *)state;
  if (!st)
    return;
  for (LkDevBytes *b : {&st->rec, &st->order, &st->out, &st->sums})
    b->release();
  if (st->ev0)
    (void)hipEventDestroy(st->ev0);
  if (st->ev1)
    (void)hipEventDestroy(st->ev1);
  delete st;
}

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
  LkUncertaintyView v{};
  if (int rc = lk_internal_uncertainty_view(e, records ? 0 : 1, cfg->def_slot, &v))
    return rc;
  UncertaintyState *st = nullptr;
  if (int rc = get_state(e, &st))
    return rc;
  const size_t n = (size_t)v.S;
  // the sectors by lane group: from the level-0 sample count alone, as the backward solve's tables
  st->h_order.resize(n);
  size_t at = 0;
  for (int g = 0; g < 3; ++g) {
    const size_t begin = at;
    for (int s = 0; s < v.S; ++s) {
      const int4 r = v.h_rect0[s];
      const int n0 = r.z > 0 ? r.w : (int)(v.h_off0[s + 1] - v.h_off0[s]);
      if (lk_bw_group(n0) == kGroups[g])
        st->h_order[at++] = (uint32_t)s;
    }
    st->count[g] = (int)(at - begin);
  }
  UNCHK(st->order.ensure(n * sizeof(uint32_t)));
  UNCHK(st->out.ensure(n * sizeof(lk_uncertainty)));
  if (sums_out)
    UNCHK(st->sums.ensure(n * kLkUncSums * sizeof(double)));
  UNCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  const lk_result *d_rec = v.result;
  if (records) {
    UNCHK(st->rec.ensure(n * sizeof(lk_result)));
    UNCHK(hipMemcpyAsync(st->rec.p, records, n * sizeof(lk_result), hipMemcpyHostToDevice, v.stream));
    d_rec = st->rec.as<lk_result>();
  }
  LkUncertaintyArgs a{};
  a.und = v.und;
  a.def = v.def;
  a.urows = v.urows;
  a.ucols = v.ucols;
  a.drows = v.drows;
  a.dcols = v.dcols;
  a.xy = v.xy;
  a.off = v.off;
  a.rect = v.rect;
  a.center = v.center;
  a.rec = d_rec;
  a.out = st->out.as<lk_uncertainty>();
  a.sums = sums_out ? st->sums.as<double>() : nullptr;
  a.level = v.level;
  st->timed = false;
  UNCHK(hipEventRecord(st->ev0, v.stream));
  const uint32_t *order = st->order.as<uint32_t>();
  for (int g = 0; g < 3; ++g) {
    a.order = order;
    a.n_sectors = st->count[g];
    if (a.n_sectors > 0)
      UNCHK(lk_launch_uncertainty(a, v.model, v.interp, kGroups[g], v.stream));
    order += st->count[g];
  }
  UNCHK(hipEventRecord(st->ev1, v.stream));
  UNCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(lk_uncertainty), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    UNCHK(hipMemcpyAsync(sums_out, st->sums.p, n * kLkUncSums * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  UNCHK(hipStreamSynchronize(v.stream));
  st->timed = true;
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_uncertainty_last(lk_engine *e, float *device_ms, int *count3) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  UncertaintyState *st = (UncertaintyState *)*lk_internal_uncertainty_slot(e);
  if (!st || !st->timed)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_internal_uncertainty_last: no lk_parameter_uncertainty yet");
  if (device_ms)
    UNCHK(hipEventElapsedTime(device_ms, st->ev0, st->ev1));
  if (count3)
    for (int g = 0; g < 3; ++g)
      count3[g] = st->count[g];
  return LK_ERROR_NONE;
}

} // extern "C"
