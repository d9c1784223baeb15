// lk_residual.cpp - host side of the photometry pass and the residual map (include/lk_engine.h: lk_photometry,
// lk_photometry_from_sums, lk_residual_map, lk_map_owner).  The kernels are lk_residual.hip; the record's arithmetic and the
// owner rule are lk_residual.hpp; the bounding box and the cell grid are the recovery pass's (lk_reseed.hip through
// lk_cell_grid.hpp).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_residual.hpp"

namespace {

struct ResidualState : LkPassState {
  LkDevBytes rec, order, out, sums;                      // photometry
  LkDevBytes pack, bbox, warped, residual, owner, count; // map
  LkCellGridBufs grid;
  std::vector<uint32_t> h_order;
  uint32_t *h_count = nullptr; // pinned [1]
  int tiles = 0, fallback = 0;
  hipError_t init() {
    const hipError_t err = LkPassState::init();
    return err != hipSuccess ? err : hipHostMalloc((void **)&h_count, sizeof(uint32_t), hipHostMallocDefault);
  }
  ~ResidualState() override {
    if (h_count)
      (void)hipHostFree(h_count);
  }
};

} // namespace

extern "C" {

int lk_photometry_from_sums(int n, const double *sums8, struct lk_photometry *out) {
  if (!sums8 || !out || n < 0)
    return LK_ERROR_BAD_DOMAIN;
  lk_photometry_record(n, sums8, out);
  return LK_ERROR_NONE;
}

int lk_map_owner(int n, const float *centers_xy, const uint8_t *good, double X, double Y, double radius) {
  if (n < 0 || (n > 0 && !centers_xy) || !std::isfinite(radius) || !(radius > 0.0))
    return INT_MIN;
  return lk_map_owner_impl(n, centers_xy, good, X, Y, radius);
}

int lk_photometry(lk_engine *e, const lk_photometry_config *cfg, const lk_result *records, struct lk_photometry *out,
                  double *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_photometry: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_photometry: no output");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_photometry: reserved words must be 0");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_photometry: chi_max must be finite (<= 0: the error code alone decides)");
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_photometry", LK_VIEW_IMAGES | (records ? 0 : LK_VIEW_RECORDS), cfg->def_slot, &v))
    return rc;
  ResidualState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_RESIDUAL, "hipHostMalloc / hipEventCreate (lk_photometry, lk_residual_map)", &st))
    return rc;
  const size_t n = (size_t)v.S;
  int count[3];
  lk_pass_order_by_group(v.h_rect0, v.h_off0, v.S, st->h_order, count);
  LK_HIPCHK(st->order.ensure(n * sizeof(uint32_t)));
  LK_HIPCHK(st->out.ensure(n * sizeof(struct lk_photometry)));
  if (sums_out)
    LK_HIPCHK(st->sums.ensure(n * kLkPhotoSums * sizeof(double)));
  LK_HIPCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  const lk_result *d_rec = v.result;
  if (int rc = lk_pass_records(e, st->rec, records, n, v.stream, &d_rec))
    return rc;
  LkPhotometryArgs a{};
  a.ev = lk_pass_sector_eval(v, d_rec);
  a.level = v.level;
  a.out = st->out.as<struct lk_photometry>();
  a.sums = sums_out ? st->sums.as<double>() : nullptr;
  a.chi_max = cfg->chi_max;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), count, [&](int group, const uint32_t *order, int n_sectors) {
    a.ev.order = order;
    a.n_sectors = n_sectors;
    return lk_launch_photometry(a, v.model, v.interp, group, v.stream);
  }));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(struct lk_photometry), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    LK_HIPCHK(hipMemcpyAsync(sums_out, st->sums.p, n * kLkPhotoSums * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->tiles = st->fallback = 0;
  st->finished();
  return LK_ERROR_NONE;
}

int lk_residual_map(lk_engine *e, const lk_residual_map_config *cfg, const lk_result *records, float *warped, float *residual,
                    int32_t *owner) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_residual_map: no configuration");
  if (!warped && !residual && !owner)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_residual_map: no output");
  if (cfg->reserved != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_residual_map: the reserved word must be 0");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_residual_map: chi_max must be finite (<= 0: the error code alone decides)");
  if (!std::isfinite(cfg->radius) || !(cfg->radius > 0.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_residual_map: radius must be finite and positive");
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_residual_map", LK_VIEW_IMAGES | (records ? 0 : LK_VIEW_RECORDS), cfg->def_slot, &v))
    return rc;
  int x0 = cfg->x0, y0 = cfg->y0, w = cfg->w, h = cfg->h;
  if (x0 == 0 && y0 == 0 && w == 0 && h == 0) {
    w = v.ucols;
    h = v.urows;
  }
  if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || (long long)x0 + w > (long long)v.ucols || (long long)y0 + h > (long long)v.urows)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_residual_map: the window must lie inside the undeformed image of level py_start (all four 0: "
                            "the whole image)");
  ResidualState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_RESIDUAL, "hipHostMalloc / hipEventCreate (lk_photometry, lk_residual_map)", &st))
    return rc;
  const size_t n = (size_t)v.S, pixels = (size_t)w * (size_t)h;
  LK_HIPCHK(st->pack.ensure(n * sizeof(LkMapSector)));
  LK_HIPCHK(st->bbox.ensure(4 * sizeof(float)));
  LK_HIPCHK(st->count.ensure(sizeof(uint32_t)));
  if (warped)
    LK_HIPCHK(st->warped.ensure(pixels * sizeof(float)));
  if (residual)
    LK_HIPCHK(st->residual.ensure(pixels * sizeof(float)));
  if (owner)
    LK_HIPCHK(st->owner.ensure(pixels * sizeof(int32_t)));
  const lk_result *d_rec = v.result;
  if (int rc = lk_pass_records(e, st->rec, records, n, v.stream, &d_rec))
    return rc;
  LK_HIPCHK(st->begin(v.stream));
  LkResidualMapArgs a{};
  if (int rc = lk_pass_grid(e, "lk_residual_map", st, st->bbox, st->grid, v.center, v.S, cfg->radius, v.stream, &a.grid))
    return rc;
  LK_HIPCHK(lk_launch_map_prep(d_rec, v.center, v.S, v.model, v.level, cfg->chi_max, st->pack.as<LkMapSector>(), v.stream));
  LK_HIPCHK(hipMemsetAsync(st->count.p, 0, sizeof(uint32_t), v.stream));
  a.und = v.und;
  a.def = v.def;
  a.urows = v.urows;
  a.ucols = v.ucols;
  a.drows = v.drows;
  a.dcols = v.dcols;
  a.pack = st->pack.as<LkMapSector>();
  a.warped = warped ? st->warped.as<float>() : nullptr;
  a.residual = residual ? st->residual.as<float>() : nullptr;
  a.owner = owner ? st->owner.as<int32_t>() : nullptr;
  a.fallback = st->count.as<uint32_t>();
  a.n_sectors = v.S;
  a.level = v.level;
  a.x0 = x0;
  a.y0 = y0;
  a.w = w;
  a.h = h;
  a.tiles_x = (w + kLkMapTileW - 1) / kLkMapTileW;
  a.r2 = (double)cfg->radius * (double)cfg->radius;
  int tiles = 0;
  LK_HIPCHK(lk_launch_residual_map(a, v.model, v.interp, &tiles, v.stream));
  LK_HIPCHK(st->end(v.stream));
  if (warped)
    LK_HIPCHK(hipMemcpyAsync(warped, st->warped.p, pixels * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  if (residual)
    LK_HIPCHK(hipMemcpyAsync(residual, st->residual.p, pixels * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  if (owner)
    LK_HIPCHK(hipMemcpyAsync(owner, st->owner.p, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipMemcpyAsync(st->h_count, st->count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->tiles = tiles;
  st->fallback = (int)*st->h_count;
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_residual_last(lk_engine *e, float *device_ms, int *tiles, int *fallback_tiles) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  ResidualState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_RESIDUAL, "lk_internal_residual_last: no lk_photometry or lk_residual_map yet", device_ms, &st))
    return rc;
  if (tiles)
    *tiles = st->tiles;
  if (fallback_tiles)
    *fallback_tiles = st->fallback;
  return LK_ERROR_NONE;
}

} // extern "C"
