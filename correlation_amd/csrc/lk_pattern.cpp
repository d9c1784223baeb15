// lk_pattern.cpp - host side of the speckle-quality pass (include/lk_engine.h: lk_pattern_quality, lk_pattern_from_sums,
// lk_suggest_subset).  The kernels are lk_pattern.hip; the records' arithmetic, the node rule and the threshold are
// lk_pattern.hpp; the one image the calls read comes through lk_internal_image_view.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_pattern.hpp"

namespace {

struct PatternState : LkPassState {
  LkDevBytes order, out, sums, mig;        // sectors
  LkDevBytes table, band, points, sub, box; // tables and query
  std::vector<uint32_t> h_order;
  hipEvent_t ev_mid = nullptr;             // between the table build and the query
  bool split = false;                      // ev_mid was recorded by the last call
  hipError_t init() {
    const hipError_t err = LkPassState::init(false); // no bounding box
    return err != hipSuccess ? err : hipEventCreate(&ev_mid);
  }
  ~PatternState() override {
    if (ev_mid)
      (void)hipEventDestroy(ev_mid);
  }
};

const char *const kWhere = "hipEventCreate (lk_pattern_quality, lk_suggest_subset)";

} // namespace

extern "C" {

int lk_pattern_from_sums(int n, const int64_t *sums9, double mig_sum, float noise_sigma, float max_saturated, struct lk_pattern *out) {
  if (!sums9 || !out || n < 0 || !std::isfinite(noise_sigma) || !std::isfinite(max_saturated))
    return LK_ERROR_BAD_DOMAIN;
  lk_pattern_record(n, sums9, mig_sum, noise_sigma, max_saturated, out);
  return LK_ERROR_NONE;
}

int lk_pattern_quality(lk_engine *e, const lk_pattern_config *cfg, struct lk_pattern *out, int64_t *sums_out, double *mig_sum_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_pattern_quality: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_pattern_quality: no output");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_pattern_quality: reserved words must be 0");
  if (cfg->grey_low < 0 || cfg->grey_low > 255 || cfg->grey_high < 0 || cfg->grey_high > 255)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_pattern_quality: grey_low and grey_high must lie in 0 .. 255");
  if (!std::isfinite(cfg->noise_sigma) || !std::isfinite(cfg->max_saturated))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_pattern_quality: noise_sigma and max_saturated must be finite");
  LkPassView v{};
  if (int rc = lk_internal_image_view(e, "lk_pattern_quality", cfg->slot, 1, &v))
    return rc;
  PatternState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_PATTERN, kWhere, &st))
    return rc;
  const size_t n = (size_t)v.S;
  int count[3];
  lk_pass_order_by_group(v.h_rect0, v.h_off0, v.S, st->h_order, count);
  LK_HIPCHK(st->order.ensure(n * sizeof(uint32_t)));
  LK_HIPCHK(st->out.ensure(n * sizeof(struct lk_pattern)));
  if (sums_out)
    LK_HIPCHK(st->sums.ensure(n * kLkPatternSums * sizeof(int64_t)));
  if (mig_sum_out)
    LK_HIPCHK(st->mig.ensure(n * sizeof(double)));
  LK_HIPCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  LkPatternArgs a{};
  a.ev = lk_pass_sector_eval(v, nullptr);
  a.level = v.level;
  a.out = st->out.as<struct lk_pattern>();
  a.sums = sums_out ? st->sums.as<long long>() : nullptr;
  a.mig_sum = mig_sum_out ? st->mig.as<double>() : nullptr;
  a.grey_low = cfg->grey_low;
  a.grey_high = cfg->grey_high;
  a.noise_sigma = cfg->noise_sigma;
  a.max_saturated = cfg->max_saturated;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), count, [&](int group, const uint32_t *order, int n_sectors) {
    a.ev.order = order;
    a.n_sectors = n_sectors;
    return lk_launch_pattern(a, group, v.stream);
  }));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(struct lk_pattern), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    LK_HIPCHK(hipMemcpyAsync(sums_out, st->sums.p, n * kLkPatternSums * sizeof(int64_t), hipMemcpyDeviceToHost, v.stream));
  if (mig_sum_out)
    LK_HIPCHK(hipMemcpyAsync(mig_sum_out, st->mig.p, n * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->split = false;
  st->finished();
  return LK_ERROR_NONE;
}

int lk_suggest_subset(lk_engine *e, const lk_subset_config *cfg, int n_points, const float *points_xy, struct lk_subset *out,
                      uint32_t *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_suggest_subset: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_suggest_subset: no output");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_suggest_subset: reserved words must be 0");
  if (n_points < 1 || !points_xy)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_suggest_subset: no points (n_points >= 1 positions {x, y})");
  if (cfg->half_min < 1 || cfg->half_max < cfg->half_min || cfg->half_max > LK_PATTERN_MAX_HALF || cfg->half_step < 1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_suggest_subset: the candidates need 1 <= half_min <= half_max <= LK_PATTERN_MAX_HALF and half_step >= 1");
  const uint32_t threshold = lk_subset_threshold(cfg->sssig_min);
  if (threshold == 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_suggest_subset: sssig_min must be finite and positive, with ceil(4 sssig_min) below 2^32");
  if (!std::isfinite(cfg->noise_sigma))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_suggest_subset: noise_sigma must be finite");
  LkPassView v{};
  if (int rc = lk_internal_image_view(e, "lk_suggest_subset", cfg->slot, 0, &v))
    return rc;
  PatternState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_PATTERN, kWhere, &st))
    return rc;
  const int n_cand = (cfg->half_max - cfg->half_min) / cfg->half_step + 1;
  const size_t n = (size_t)n_points;
  LkSatArgs t{};
  t.img = v.und;
  t.rows = v.urows;
  t.cols = v.ucols;
  t.pitch = (v.ucols + 3) / 4 * 4;
  t.n_bands = (v.urows + kLkSatBandRows - 1) / kLkSatBandRows;
  const size_t plane = (size_t)t.rows * (size_t)t.pitch;
  LK_HIPCHK(st->table.ensure(2 * plane * sizeof(uint32_t)));
  LK_HIPCHK(st->band.ensure(2 * (size_t)t.n_bands * (size_t)t.pitch * sizeof(uint32_t)));
  LK_HIPCHK(st->points.ensure(n * sizeof(float2)));
  LK_HIPCHK(st->sub.ensure(n * sizeof(struct lk_subset)));
  if (sums_out)
    LK_HIPCHK(st->box.ensure(n * (size_t)n_cand * 2 * sizeof(uint32_t)));
  t.table = st->table.as<uint32_t>();
  t.band = st->band.as<uint32_t>();
  LK_HIPCHK(hipMemcpyAsync(st->points.p, points_xy, n * sizeof(float2), hipMemcpyHostToDevice, v.stream));
  LkSubsetArgs q{};
  q.table = t.table;
  q.rows = t.rows;
  q.cols = t.cols;
  q.pitch = t.pitch;
  q.points = st->points.as<float2>();
  q.out = st->sub.as<struct lk_subset>();
  q.sums = sums_out ? st->box.as<uint32_t>() : nullptr;
  q.n_points = n_points;
  q.n_cand = n_cand;
  q.half_min = cfg->half_min;
  q.half_step = cfg->half_step;
  q.threshold = threshold;
  q.noise_sigma = cfg->noise_sigma;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(lk_launch_sat_build(t, v.stream));
  LK_HIPCHK(hipEventRecord(st->ev_mid, v.stream));
  LK_HIPCHK(lk_launch_subset_query(q, v.stream));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(out, st->sub.p, n * sizeof(struct lk_subset), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    LK_HIPCHK(hipMemcpyAsync(sums_out, st->box.p, n * (size_t)n_cand * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->split = true;
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_pattern_last(lk_engine *e, float *device_ms, int *row_tile, int *band_rows, float *build_ms, float *query_ms) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  PatternState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_PATTERN, "lk_internal_pattern_last: no lk_pattern_quality or lk_suggest_subset yet", device_ms, &st))
    return rc;
  if (row_tile)
    *row_tile = kLkSatRowTile;
  if (band_rows)
    *band_rows = kLkSatBandRows;
  if (build_ms) {
    *build_ms = 0.f;
    if (st->split)
      LK_HIPCHK(hipEventElapsedTime(build_ms, st->ev0, st->ev_mid));
  }
  if (query_ms) {
    *query_ms = 0.f;
    if (st->split)
      LK_HIPCHK(hipEventElapsedTime(query_ms, st->ev_mid, st->ev1));
  }
  return LK_ERROR_NONE;
}

} // extern "C"
