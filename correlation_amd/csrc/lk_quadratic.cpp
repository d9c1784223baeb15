// lk_quadratic.cpp - host side of the second-order refinement (include/lk_engine.h: lk_refine_quadratic,
// lk_quadratic_step_from_sums).  The kernel is lk_quadratic.hip; criterion and step are lk_quadratic.hpp.  lk_znssd.cpp
// with one more input, the second-order seeds.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_quadratic.hpp"

namespace {

struct QuadraticState : LkPassState {
  LkDevBytes rec, guess, second, order, count0, rec_out, out, sums;
  std::vector<uint32_t> h_order;
  std::vector<int32_t> h_count0;
  int count[3] = {0, 0, 0};
  hipError_t init() { return LkPassState::init(false); } // (no cell grid: no bounding box to land)
};

static_assert(sizeof(struct lk_quadratic) == 128 && sizeof(lk_quadratic_config) == 32, "the records of the header");

constexpr int kQdDefaultIters = 50; // lk_config's documented defaults, as lk_znssd.cpp
constexpr float kQdDefaultPrecision = 1e-3f;
constexpr float kQdDefaultLambda = 1e-3f;

} // namespace

extern "C" {

int lk_quadratic_step_from_sums(int n, const double *sums88, float lambda, double *delta12, double *crit, double *gain_offset2,
                                int32_t *status) {
  if (!sums88 || !status || n < 0 || !(lambda >= 0.f) || !std::isfinite(lambda))
    return LK_ERROR_BAD_DOMAIN;
  double delta[kLkQdParams], work[kLkQdWork];
  LkZnCriterion cr;
  *status = lk_quadratic_step(n, sums88, (double)lambda, delta, &cr, work);
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

int lk_refine_quadratic(lk_engine *e, const lk_quadratic_config *cfg, const lk_result *records, const float *guesses, const float *second,
                        lk_result *records_out, struct lk_quadratic *info_out, double *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_quadratic: no configuration");
  if (!records_out && !info_out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_quadratic: no output (records_out and info_out are both null)");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_quadratic: reserved words must be 0");
  if (records && guesses)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_quadratic: records and guesses are both given (seeds are one or the other)");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_quadratic: chi_max must be finite (<= 0: the error code alone decides)");
  if (!std::isfinite(cfg->precision) || !std::isfinite(cfg->lambda0))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_quadratic: precision and lambda0 must be finite (<= 0: the default)");
  const bool held = !records && !guesses;
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_refine_quadratic", LK_VIEW_IMAGES | (held ? LK_VIEW_RECORDS : 0), cfg->def_slot, &v))
    return rc;
  QuadraticState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_QUADRATIC, "hipEventCreate (lk_refine_quadratic)", &st))
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
  LK_HIPCHK(st->out.ensure(n * sizeof(struct lk_quadratic)));
  if (sums_out)
    LK_HIPCHK(st->sums.ensure(n * kLkQdSums * sizeof(double)));
  LK_HIPCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  LK_HIPCHK(hipMemcpyAsync(st->count0.p, st->h_count0.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
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
  LkQuadraticArgs a{};
  a.ev = lk_pass_sector_eval(v, d_rec);
  a.guess = guesses ? st->guess.as<float>() : nullptr;
  a.second = second ? st->second.as<float>() : nullptr;
  a.count0 = st->count0.as<int32_t>();
  a.rec_out = st->rec_out.as<lk_result>();
  a.out = st->out.as<struct lk_quadratic>();
  a.sums = sums_out ? st->sums.as<double>() : nullptr;
  a.level = v.level;
  a.model = v.model;
  a.max_iters = cfg->max_iters < 0 ? kQdDefaultIters : cfg->max_iters;
  a.chi_max = cfg->chi_max;
  a.precision = cfg->precision > 0.f ? cfg->precision : kQdDefaultPrecision;
  a.lambda0 = cfg->lambda0 > 0.f ? cfg->lambda0 : kQdDefaultLambda;
  LK_HIPCHK(st->begin(v.stream));
  const uint32_t *order = st->order.as<uint32_t>();
  for (int g = 0; g < 3; ++g) {
    a.ev.order = order;
    a.n_sectors = st->count[g];
    if (a.n_sectors > 0)
      LK_HIPCHK(lk_launch_quadratic(a, v.interp, kLkPassGroups[g], v.stream));
    order += st->count[g];
  }
  LK_HIPCHK(st->end(v.stream));
  if (records_out)
    LK_HIPCHK(hipMemcpyAsync(records_out, st->rec_out.p, n * sizeof(lk_result), hipMemcpyDeviceToHost, v.stream));
  if (info_out)
    LK_HIPCHK(hipMemcpyAsync(info_out, st->out.p, n * sizeof(struct lk_quadratic), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    LK_HIPCHK(hipMemcpyAsync(sums_out, st->sums.p, n * kLkQdSums * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_quadratic_last(lk_engine *e, float *device_ms, int *count3) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  QuadraticState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_QUADRATIC, "lk_internal_quadratic_last: no lk_refine_quadratic yet", device_ms, &st))
    return rc;
  if (count3)
    for (int g = 0; g < 3; ++g)
      count3[g] = st->count[g];
  return LK_ERROR_NONE;
}

} // extern "C"
