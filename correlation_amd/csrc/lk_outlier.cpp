// lk_outlier.cpp - host side of the outlier flags (include/lk_engine.h: lk_flag_outliers, lk_outlier_from_window).  The
// kernels are lk_outlier.hip; the selection and the ratio arithmetic are lk_outlier.hpp; the bounding box and the cell grid
// are the recovery pass's (lk_reseed.hip through lk_cell_grid.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_outlier.hpp"
#include "lk_pass.hpp"

namespace {

// Lanes per sector, from the expected members of a sector's 3 x 3 cells (9 S / cells), as lk_strain.cpp chooses: the walk
// is the strain field's, and there the 16-lane row won every case measured, up to 502 members.  The selection adds a reason
// of its own to switch: a lane stashes kLkOutlierRows members, and about a third of the candidates of the 3 x 3 cells are
// inside the circle, so 16 lanes keep windows of up to 16 x 16 in LDS - some 700 candidates.  Not timed on an MI355X
// (DESIGN.md section 17).
constexpr double kWideGroupFrom = 640.0;

struct OutlierState : LkPassState {
  LkDevBytes rec, good, pack, out, bbox;
  LkCellGridBufs grid;
  int group = 0, lds_rows = 0;
  double members = 0; // expected members of the 3 x 3 cells of the last call
};

// test hooks: LK_OUTLIER_GROUP = 16 / 64 overrides the choice of the lane group; LK_OUTLIER_LDS_CAP =
// the members of a window a group may keep in LDS (rounded down to whole rows of `group` lanes, at most kLkOutlierRows rows;
// 0 re-walks every window)
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
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_flag_outliers", records ? 0 : LK_VIEW_RECORDS, -1, &v))
    return rc;
  if (cfg->mark && !records && lk_internal_reference_order(e))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_flag_outliers: mark = 1 on the engine-held records is refused in reference-order mode (its records "
                            "are the CPU engine's); pass records, or mark = 0");
  OutlierState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_OUTLIER, "hipHostMalloc / hipEventCreate (lk_flag_outliers)", &st))
    return rc;
  const size_t n = (size_t)v.S;
  LK_HIPCHK(st->good.ensure(n));
  LK_HIPCHK(st->pack.ensure(n * sizeof(float4)));
  LK_HIPCHK(st->out.ensure(n * sizeof(lk_outlier)));
  LK_HIPCHK(st->bbox.ensure(4 * sizeof(float)));
  lk_result *d_rec = v.result;
  if (int rc = lk_pass_records(e, st->rec, records, n, v.stream, &d_rec)) // (the call's own copy: marking it touches nothing of the engine's)
    return rc;
  LK_HIPCHK(st->begin(v.stream));
  LkOutlierArgs a{};
  if (int rc = lk_pass_grid(e, "lk_flag_outliers", st, st->bbox, st->grid, v.center, v.S, cfg->radius, v.stream, &a.grid))
    return rc;
  LK_HIPCHK(lk_launch_pack_prep(d_rec, v.center, v.S, 1, v.model, cfg->chi_max, 1, st->good.as<uint8_t>(), st->pack.as<float4>(), v.stream));
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
  st->group = lk_pass_env_choice("LK_OUTLIER_GROUP", 16, 64, st->members > kWideGroupFrom ? 64 : 16);
  st->lds_rows = a.lds_rows = env_rows(st->group);
  for (int pass = 0; pass < cfg->passes; ++pass) {
    if (pass > 0) // (the pass before has written every record of a.out; this one writes them again after reading the marks)
      LK_HIPCHK(lk_launch_outlier_exclude(a.out, v.center, a.good, v.S, st->pack.as<float4>(), v.stream));
    LK_HIPCHK(lk_launch_outlier(a, st->group, v.stream));
  }
  const bool marks = cfg->mark && (records_out || !records);
  if (marks)
    LK_HIPCHK(lk_launch_outlier_mark(a.out, v.S, d_rec, v.stream));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(lk_outlier), hipMemcpyDeviceToHost, v.stream));
  if (records_out)
    LK_HIPCHK(hipMemcpyAsync(records_out, d_rec, n * sizeof(lk_result), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
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
  OutlierState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_OUTLIER, "lk_internal_outlier_last: no lk_flag_outliers yet", device_ms, &st))
    return rc;
  if (group)
    *group = st->group;
  if (lds_rows)
    *lds_rows = st->lds_rows;
  if (members)
    *members = st->members;
  return LK_ERROR_NONE;
}

} // extern "C"
