// lk_spline.cpp - host side of the B-spline refinement (include/lk_engine.h: lk_refine_spline, lk_spline_coefficients,
// lk_spline_sample, lk_spline_weights).  The kernels are lk_spline.hip; poles and weights are lk_spline.hpp; the loop,
// criterion and step are lk_refine_znssd's (lk_znssd_loop.hpp, lk_znssd.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_refine.hpp"
#include "lk_spline.hpp"
#include "lk_znssd.hpp"

namespace {

struct SplineState : LkRefineState {
  LkDevBytes coef;        // the coefficient image, rebuilt by every call
  LkDevBytes points, w4;  // lk_spline_sample
  hipEvent_t ev_mid = nullptr; // behind the build of the coefficient image
  hipError_t init() {
    const hipError_t err = LkRefineState::init();
    return err != hipSuccess ? err : hipEventCreate(&ev_mid);
  }
  ~SplineState() override {
    if (ev_mid)
      (void)hipEventDestroy(ev_mid);
  }
};

const char *const kWhere = "hipEventCreate (lk_refine_spline, lk_spline_coefficients, lk_spline_sample)";

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
  LkRefineCall c{"lk_refine_spline", records, guesses, nullptr, nullptr, records_out, info_out, sums_out, sizeof(struct lk_znssd), kLkZnSums};
  if (int rc = lk_refine_check_head(e, c, cfg))
    return rc;
  const int order_n = spline_order(cfg->order);
  if (order_n == 0)
    return lk_refine_refuse(e, c, "order must be 3 or 5 (0: 5)");
  if (int rc = lk_refine_check_view(e, c))
    return rc;
  SplineState *st = nullptr;
  if (int rc = lk_refine_prepare(e, c, LK_PASS_SPLINE, kWhere, &st))
    return rc;
  const LkPassView &v = c.v;
  LK_HIPCHK(st->begin(v.stream));
  if (int rc = spline_build(e, c.who, st, order_n, v.def, v.drows, v.dcols, v.stream))
    return rc;
  LK_HIPCHK(hipEventRecord(st->ev_mid, v.stream));
  LkSplineArgs a{};
  a.coef = st->coef.as<float>();
  lk_refine_fill(a.zn, c, st);
  a.zn.out = st->out.as<struct lk_znssd>();
  LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), st->count, [&](int group, const uint32_t *order, int n) {
    a.zn.ev.order = order;
    a.zn.n_sectors = n;
    return lk_launch_spline(a, v.model, order_n, group, v.stream);
  }));
  return lk_refine_finish(e, c, st);
}

// bench hook (lk_internal.hpp)
int lk_internal_spline_last(lk_engine *e, float *device_ms, int *count3, float *build_ms) {
  SplineState *st = nullptr;
  if (int rc = lk_pass_last_groups(e, LK_PASS_SPLINE, "lk_internal_spline_last: no lk_refine_spline yet", device_ms, count3, &st))
    return rc;
  if (build_ms)
    LK_HIPCHK(hipEventElapsedTime(build_ms, st->ev0, st->ev_mid));
  return LK_ERROR_NONE;
}

} // extern "C"
