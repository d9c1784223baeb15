// lk_spline.cpp - host side of the B-spline refinement (include/lk_engine.h: lk_refine_spline, lk_spline_coefficients,
// lk_spline_sample, lk_spline_weights).  The kernels are lk_spline.hip; poles and weights are lk_spline.hpp; the loop,
// criterion and step are lk_refine_znssd's (lk_znssd_loop.hpp, lk_znssd.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_spline.hpp"
#include "lk_znssd.hpp"

namespace {

struct SplineState : LkPassState {
  LkDevBytes rec, guess, order, count0, rec_out, out, sums;
  LkDevBytes coef;        // the coefficient image, rebuilt by every call
  LkDevBytes points, w4;  // lk_spline_sample
  std::vector<uint32_t> h_order;
  std::vector<int32_t> h_count0;
  int count[3] = {0, 0, 0};
  hipEvent_t ev_mid = nullptr; // behind the build of the coefficient image
  hipError_t init() {
    const hipError_t err = LkPassState::init(false); // (no cell grid: no bounding box to land)
    return err != hipSuccess ? err : hipEventCreate(&ev_mid);
  }
  ~SplineState() override {
    if (ev_mid)
      (void)hipEventDestroy(ev_mid);
  }
};

const char *const kWhere = "hipEventCreate (lk_refine_spline, lk_spline_coefficients, lk_spline_sample)";

constexpr int kSpDefaultIters = 50; // lk_refine_znssd's defaults
constexpr float kSpDefaultPrecision = 1e-3f;
constexpr float kSpDefaultLambda = 1e-3f;

// 3 or 5, or 0 for an order the pass does not have
int spline_order(int order) { return order == 0 ? 5 : order == 3 || order == 5 ? order : 0; }

// the coefficient image of a level image into st->coef, on `stream`; refuses an image with a side below kLkSplineMinSide
int spline_build(lk_engine *e, const char *who, SplineState *st, int order, const uint8_t *img, int rows, int cols, hipStream_t stream) {
  if (rows < kLkSplineMinSide || cols < kLkSplineMinSide)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string(who) + ": the level image has a side below 8").c_str());
  LK_HIPCHK(st->coef.ensure((size_t)rows * (size_t)cols * sizeof(float)));
  LK_HIPCHK(lk_launch_spline_build(order, img, rows, cols, st->coef.as<float>(), stream));
  return LK_ERROR_NONE;
}

// what lk_spline_coefficients and lk_spline_sample begin with: the image of `slot`, the state, the coefficients
int spline_of_slot(lk_engine *e, const char *who, int slot, int order, LkPassView *v, SplineState **st) {
  if (spline_order(order) == 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string(who) + ": order must be 3 or 5 (0: 5)").c_str());
  if (int rc = lk_internal_image_view(e, who, slot, 0, v))
    return rc;
  if (int rc = lk_pass_state(e, LK_PASS_SPLINE, kWhere, st))
    return rc;
  return spline_build(e, who, *st, spline_order(order), v->und, v->urows, v->ucols, v->stream);
}

} // namespace

extern "C" {

int lk_spline_weights(int order, float t, float *w6, float *g6) {
  if (!w6 || !g6 || spline_order(order) == 0 || !std::isfinite(t))
    return LK_ERROR_BAD_DOMAIN;
  for (int i = 0; i < 6; ++i)
    w6[i] = g6[i] = 0.f;
  if (spline_order(order) == 3) {
    float w[4], g[4];
    lk_spline_weights<3>(t, w, g);
    for (int i = 0; i < 4; ++i)
      w6[i] = w[i], g6[i] = g[i];
  } else {
    float w[6], g[6];
    lk_spline_weights<5>(t, w, g);
    for (int i = 0; i < 6; ++i)
      w6[i] = w[i], g6[i] = g[i];
  }
  return LK_ERROR_NONE;
}

int lk_spline_coefficients(lk_engine *e, int slot, int order, float *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_spline_coefficients: no output");
  LkPassView v{};
  SplineState *st = nullptr;
  if (int rc = spline_of_slot(e, "lk_spline_coefficients", slot, order, &v, &st))
    return rc;
  LK_HIPCHK(hipMemcpyAsync(out, st->coef.p, (size_t)v.urows * (size_t)v.ucols * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  return LK_ERROR_NONE;
}

int lk_spline_sample(lk_engine *e, int slot, int order, const float *xy, int n, float *out4) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!xy || !out4 || n < 1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_spline_sample: no points (n >= 1 positions {x, y}) or no output");
  LkPassView v{};
  SplineState *st = nullptr;
  if (int rc = spline_of_slot(e, "lk_spline_sample", slot, order, &v, &st))
    return rc;
  const size_t np = (size_t)n;
  LK_HIPCHK(st->points.ensure(np * sizeof(float2)));
  LK_HIPCHK(st->w4.ensure(np * sizeof(float4)));
  LK_HIPCHK(hipMemcpyAsync(st->points.p, xy, np * sizeof(float2), hipMemcpyHostToDevice, v.stream));
  LK_HIPCHK(lk_launch_spline_sample(spline_order(order), st->coef.as<float>(), v.urows, v.ucols, st->points.as<float2>(), n,
                                    st->w4.as<float4>(), v.stream));
  LK_HIPCHK(hipMemcpyAsync(out4, st->w4.p, np * sizeof(float4), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  return LK_ERROR_NONE;
}

int lk_refine_spline(lk_engine *e, const lk_spline_config *cfg, const lk_result *records, const float *guesses, lk_result *records_out,
                     struct lk_znssd *info_out, double *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_spline: no configuration");
  if (!records_out && !info_out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_spline: no output (records_out and info_out are both null)");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_spline: reserved words must be 0");
  if (spline_order(cfg->order) == 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_spline: order must be 3 or 5 (0: 5)");
  if (records && guesses)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_spline: records and guesses are both given (seeds are one or the other)");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_spline: chi_max must be finite (<= 0: the error code alone decides)");
  if (!std::isfinite(cfg->precision) || !std::isfinite(cfg->lambda0))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_refine_spline: precision and lambda0 must be finite (<= 0: the default)");
  const int order_n = spline_order(cfg->order);
  const bool held = !records && !guesses;
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_refine_spline", LK_VIEW_IMAGES | (held ? LK_VIEW_RECORDS : 0), cfg->def_slot, &v))
    return rc;
  SplineState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_SPLINE, kWhere, &st))
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
  LK_HIPCHK(st->out.ensure(n * sizeof(struct lk_znssd)));
  if (sums_out)
    LK_HIPCHK(st->sums.ensure(n * kLkZnSums * sizeof(double)));
  LK_HIPCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  LK_HIPCHK(hipMemcpyAsync(st->count0.p, st->h_count0.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
  const lk_result *d_rec = guesses ? nullptr : v.result;
  if (int rc = lk_pass_records(e, st->rec, records, n, v.stream, &d_rec))
    return rc;
  if (guesses) {
    LK_HIPCHK(st->guess.ensure(n * 6 * sizeof(float)));
    LK_HIPCHK(hipMemcpyAsync(st->guess.p, guesses, n * 6 * sizeof(float), hipMemcpyHostToDevice, v.stream));
  }
  LK_HIPCHK(st->begin(v.stream));
  if (int rc = spline_build(e, "lk_refine_spline", st, order_n, v.def, v.drows, v.dcols, v.stream))
    return rc;
  LK_HIPCHK(hipEventRecord(st->ev_mid, v.stream));
  LkSplineArgs a{};
  a.coef = st->coef.as<float>();
  a.zn.ev = lk_pass_sector_eval(v, d_rec);
  a.zn.guess = guesses ? st->guess.as<float>() : nullptr;
  a.zn.count0 = st->count0.as<int32_t>();
  a.zn.rec_out = st->rec_out.as<lk_result>();
  a.zn.out = st->out.as<struct lk_znssd>();
  a.zn.sums = sums_out ? st->sums.as<double>() : nullptr;
  a.zn.level = v.level;
  a.zn.max_iters = cfg->max_iters < 0 ? kSpDefaultIters : cfg->max_iters;
  a.zn.chi_max = cfg->chi_max;
  a.zn.precision = cfg->precision > 0.f ? cfg->precision : kSpDefaultPrecision;
  a.zn.lambda0 = cfg->lambda0 > 0.f ? cfg->lambda0 : kSpDefaultLambda;
  const uint32_t *order = st->order.as<uint32_t>();
  for (int g = 0; g < 3; ++g) {
    a.zn.ev.order = order;
    a.zn.n_sectors = st->count[g];
    if (a.zn.n_sectors > 0)
      LK_HIPCHK(lk_launch_spline(a, v.model, order_n, kLkPassGroups[g], v.stream));
    order += st->count[g];
  }
  LK_HIPCHK(st->end(v.stream));
  if (records_out)
    LK_HIPCHK(hipMemcpyAsync(records_out, st->rec_out.p, n * sizeof(lk_result), hipMemcpyDeviceToHost, v.stream));
  if (info_out)
    LK_HIPCHK(hipMemcpyAsync(info_out, st->out.p, n * sizeof(struct lk_znssd), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    LK_HIPCHK(hipMemcpyAsync(sums_out, st->sums.p, n * kLkZnSums * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_spline_last(lk_engine *e, float *device_ms, int *count3, float *build_ms) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  SplineState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_SPLINE, "lk_internal_spline_last: no lk_refine_spline yet", device_ms, &st))
    return rc;
  if (count3)
    for (int g = 0; g < 3; ++g)
      count3[g] = st->count[g];
  if (build_ms)
    LK_HIPCHK(hipEventElapsedTime(build_ms, st->ev0, st->ev_mid));
  return LK_ERROR_NONE;
}

} // extern "C"
