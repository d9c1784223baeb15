// lk_outlier.cpp - host side of the outlier flags (include/lk_engine.h: lk_flag_outliers, lk_outlier_from_window).  The
// kernels are lk_outlier.hip; the selection and the ratio arithmetic are lk_outlier.hpp; the bounding box and the cell grid
// are the recovery pass's (lk_reseed.hip through lk_cell_grid.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <initializer_list>

#include "../../include/lk_engine.h"
#include "lk_cell_grid.hpp"
#include "lk_device.hpp"
#include "lk_internal.hpp"
#include "lk_launch.hpp"
#include "lk_outlier.hpp"

#define OLCHK(call)                                                                                   \
  do {                                                                                                \
    hipError_t _e = (call);                                                                           \
    if (_e != hipSuccess)                                                                             \
      return lk_internal_hipfail(e, _e, #call);                                                       \
  } while (0)

namespace {

// Lanes per sector, from the expected members of a sector's 3 x 3 cells (9 S / cells), as lk_strain.cpp chooses: the walk
// is the strain field's, and there the 16-lane row won every case measured, up to 502 members.  The selection adds a reason
// of its own to switch: a lane stashes kLkOutlierRows members, and about a third of the candidates of the 3 x 3 cells are
// inside the circle, so 16 lanes keep windows of up to 16 x 16 in LDS - some 700 candidates.  Not timed on an MI355X
// (DESIGN.md section 17).
constexpr double kWideGroupFrom = 640.0;

struct OutlierState {
  LkDevBytes rec, good, pack, out, bbox;
  LkCellGridBufs grid;
  float *h_bbox = nullptr; // pinned [4]
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;      // ev0 / ev1 bracket the device part of a finished call (read by lk_internal_outlier_last)
  int group = 0, lds_rows = 0;
  double members = 0;      // expected members of the 3 x 3 cells of the last call
};

int get_state(lk_engine *e, OutlierState **out) {
  void **slot = lk_internal_outlier_slot(e);
  if (!*slot) {
    OutlierState *st = new OutlierState();
    hipError_t err = hipHostMalloc((void **)&st->h_bbox, 4 * sizeof(float), hipHostMallocDefault);
    if (err == hipSuccess)
      err = hipEventCreate(&st->ev0);
    if (err == hipSuccess)
      err = hipEventCreate(&st->ev1);
    if (err != hipSuccess) {
      lk_internal_outlier_release(st);
      return lk_internal_hipfail(e, err, "hipHostMalloc / hipEventCreate (lk_flag_outliers)");
    }
    *slot = st;
  }
  *out = (OutlierState *)*slot;
  return LK_ERROR_NONE;
}

// test hooks: LK_OUTLIER_GROUP = 16 / 64 overrides the choice of the lane group; LK_OUTLIER_LDS_CAP =
// the members of a window a group may keep in LDS (rounded down to whole rows of `group` lanes, at most kLkOutlierRows rows;
// 0 re-walks every window)
int env_group(int otherwise) {
  const char *s = std::getenv("LK_OUTLIER_GROUP");
  if (!s || !*s)
    return otherwise;
  const int v = std::atoi(s);
  return v == 16 || v == 64 ? v : otherwise;
}
int env_rows(int group) {
  const char *s = std::getenv("LK_OUTLIER_LDS_CAP");
  if (!s || !*s)
    return kLkOutlierRows;
  const long v = std::atol(s);
  if (v < 0)
    return kLkOutlierRows;
  const long rows = v / group;
  return rows < kLkOutlierRows ? (int)rows : kLkOutlierRows;
}

bool positive(float v) { return std::isfinite(v) && v > 0.f; }

} // namespace

void lk_internal_outlier_release(void *state) {
  OutlierState *st = (OutlierState *)state;
  if (!st)
    return;
  for (LkDevBytes *b : {&st->rec, &st->good, &st->pack, &st->out, &st->bbox, &st->grid.cell_of, &st->grid.start, &st->grid.cursor,
                        &st->grid.unordered, &st->grid.members})
    b->release();
  if (st->h_bbox)
    (void)hipHostFree(st->h_bbox);
  if (st->ev0)
    (void)hipEventDestroy(st->ev0);
  if (st->ev1)
    (void)hipEventDestroy(st->ev1);
  delete st;
}

extern "C" {

int lk_flag_outliers(lk_engine *e, const lk_outlier_config *cfg, const lk_result *records, lk_outlier *out,
                     lk_result *records_out, int *n_flagged) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: no output");
  if (!positive(cfg->radius))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: radius must be finite and positive");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: chi_max must be finite (<= 0: the error code alone decides)");
  if (!positive(cfg->eps))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: eps must be finite and positive");
  if (!positive(cfg->threshold))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: threshold must be finite and positive");
  if (cfg->detrend != 0 && cfg->detrend != 1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: detrend must be 0 or 1");
  if (cfg->mark != 0 && cfg->mark != 1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: mark must be 0 or 1");
  if (cfg->min_neighbours < (cfg->detrend ? 4 : 3))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_flag_outliers: min_neighbours must be at least 4 with detrend (a plane has three unknowns and "
                            "the sector itself is not counted), at least 3 without");
  if (cfg->passes < 1 || cfg->passes > 4)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: passes must be 1..4");
  LkOutlierView v{};
  if (int rc = lk_internal_outlier_view(e, records ? 0 : 1, &v))
    return rc;
  if (cfg->mark && !records && lk_internal_reference_order(e))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_flag_outliers: mark = 1 on the engine-held records is refused in reference-order mode (its records "
                            "are the CPU engine's); pass records, or mark = 0");
  OutlierState *st = nullptr;
  if (int rc = get_state(e, &st))
    return rc;
  const size_t n = (size_t)v.S;
  OLCHK(st->good.ensure(n));
  OLCHK(st->pack.ensure(n * sizeof(float4)));
  OLCHK(st->out.ensure(n * sizeof(lk_outlier)));
  OLCHK(st->bbox.ensure(4 * sizeof(float)));
  lk_result *d_rec = v.result;
  if (records) {
    OLCHK(st->rec.ensure(n * sizeof(lk_result)));
    OLCHK(hipMemcpyAsync(st->rec.p, records, n * sizeof(lk_result), hipMemcpyHostToDevice, v.stream));
    d_rec = st->rec.as<lk_result>(); // (the call's own copy: marking it touches nothing of the engine's)
  }
  st->timed = false;
  OLCHK(hipEventRecord(st->ev0, v.stream));
  // the centres' bounding box sizes the grid: the call's one round trip before the kernels
  OLCHK(lk_launch_reseed_bbox(v.center, v.S, st->bbox.as<float>(), v.stream));
  OLCHK(hipMemcpyAsync(st->h_bbox, st->bbox.p, 4 * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  OLCHK(hipStreamSynchronize(v.stream));
  if (!lk_cell_grid_bbox_finite(st->h_bbox))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_flag_outliers: a sector centre is not finite");
  LkOutlierArgs a{};
  OLCHK(lk_cell_grid_build(st->grid, v.center, v.S, cfg->radius, st->h_bbox, v.stream, &a.grid));
  OLCHK(lk_launch_outlier_prep(d_rec, v.center, v.S, v.model, cfg->chi_max, st->good.as<uint8_t>(), st->pack.as<float4>(), v.stream));
  a.center = v.center;
  a.good = st->good.as<uint8_t>();
  a.pack = st->pack.as<float4>();
  a.out = st->out.as<lk_outlier>();
  a.n_sectors = v.S;
  a.min_neighbours = cfg->min_neighbours;
  a.detrend = cfg->detrend;
  a.eps = cfg->eps;
  a.threshold = cfg->threshold;
  a.radius = (double)cfg->radius;
  st->members = 9.0 * (double)v.S / ((double)a.grid.nx * (double)a.grid.ny);
  st->group = env_group(st->members > kWideGroupFrom ? 64 : 16);
  st->lds_rows = a.lds_rows = env_rows(st->group);
  for (int pass = 0; pass < cfg->passes; ++pass) {
    if (pass > 0) // (the pass before has written every record of a.out; this one writes them again after reading the marks)
      OLCHK(lk_launch_outlier_exclude(a.out, v.center, a.good, v.S, st->pack.as<float4>(), v.stream));
    OLCHK(lk_launch_outlier(a, st->group, v.stream));
  }
  const bool marks = cfg->mark && (records_out || !records);
  if (marks)
    OLCHK(lk_launch_outlier_mark(a.out, v.S, d_rec, v.stream));
  OLCHK(hipEventRecord(st->ev1, v.stream));
  OLCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(lk_outlier), hipMemcpyDeviceToHost, v.stream));
  if (records_out)
    OLCHK(hipMemcpyAsync(records_out, d_rec, n * sizeof(lk_result), hipMemcpyDeviceToHost, v.stream));
  OLCHK(hipStreamSynchronize(v.stream));
  st->timed = true;
  if (n_flagged) {
    int c = 0;
    for (size_t s = 0; s < n; ++s)
      c += out[s].status == LK_OUTLIER_FLAGGED ? 1 : 0;
    *n_flagged = c;
  }
  return LK_ERROR_NONE;
}

int lk_outlier_from_window(int n, const float *e_u, const float *e_v, float es_u, float es_v, float eps, float threshold,
                           lk_outlier *out) {
  if (!e_u || !e_v || !out || n < 1 || !std::isfinite(es_u) || !std::isfinite(es_v) || !positive(eps) || !positive(threshold))
    return LK_ERROR_BAD_DOMAIN;
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(e_u[i]) || !std::isfinite(e_v[i]))
      return LK_ERROR_BAD_DOMAIN;
  return lk_outlier_from_window_impl(n, e_u, e_v, es_u, es_v, eps, threshold, out) == 0 ? LK_ERROR_NONE : LK_ERROR_BAD_DOMAIN;
}

// bench hook (lk_internal.hpp)
int lk_internal_outlier_last(lk_engine *e, float *device_ms, int *group, int *lds_rows, double *members) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  OutlierState *st = (OutlierState *)*lk_internal_outlier_slot(e);
  if (!st || !st->timed)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_internal_outlier_last: no lk_flag_outliers yet");
  if (device_ms)
    OLCHK(hipEventElapsedTime(device_ms, st->ev0, st->ev1));
  if (group)
    *group = st->group;
  if (lds_rows)
    *lds_rows = st->lds_rows;
  if (members)
    *members = st->members;
  return LK_ERROR_NONE;
}

} // extern "C"
