// lk_residual.cpp - host side of the photometry pass and the residual map (include/lk_engine.h: lk_photometry,
// lk_photometry_from_sums, lk_residual_map, lk_map_owner).  The kernels are lk_residual.hip; the record's arithmetic and the
// owner rule are lk_residual.hpp; the engine is read through the uncertainty pass's accessor; the bounding box and the cell
// grid are the recovery pass's (lk_reseed.hip through lk_cell_grid.hpp).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <initializer_list>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_cell_grid.hpp"
#include "lk_device.hpp"
#include "lk_internal.hpp"
#include "lk_launch.hpp"
#include "lk_residual.hpp"

#define RSCHK(call)                                                                                   \
  do {                                                                                                \
    hipError_t _e = (call);                                                                           \
    if (_e != hipSuccess)                                                                             \
      return lk_internal_hipfail(e, _e, #call);                                                       \
  } while (0)

namespace {

constexpr int kGroups[3] = {16, 64, 512};

struct ResidualState {
  LkDevBytes rec, order, out, sums;                      // photometry
  LkDevBytes pack, bbox, warped, residual, owner, count; // map
  LkCellGridBufs grid;
  std::vector<uint32_t> h_order;
  float *h_bbox = nullptr;       // pinned [4]
  uint32_t *h_count = nullptr;   // pinned [1]
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false; // ev0 / ev1 bracket the device part of a finished call (read by lk_internal_residual_last)
  int tiles = 0, fallback = 0;
};

int get_state(lk_engine *e, ResidualState **out) {
  void **slot = lk_internal_residual_slot(e);
  if (!*slot) {
    ResidualState *st = new ResidualState();
    hipError_t err = hipHostMalloc((void **)&st->h_bbox, 4 * sizeof(float), hipHostMallocDefault);
    if (err == hipSuccess)
      err = hipHostMalloc((void **)&st->h_count, sizeof(uint32_t), hipHostMallocDefault);
    if (err == hipSuccess)
      err = hipEventCreate(&st->ev0);
    if (err == hipSuccess)
      err = hipEventCreate(&st->ev1);
    if (err != hipSuccess) {
      lk_internal_residual_release(st);
      return lk_internal_hipfail(e, err, "hipHostMalloc / hipEventCreate (lk_photometry, lk_residual_map)");
    }
    *slot = st;
  }
  *out = (ResidualState *)*slot;
  return LK_ERROR_NONE;
}

} // namespace

void lk_internal_residual_release(void *state) {
  ResidualState *st = (ResidualState *)state;
  if (!st)
    return;
  for (LkDevBytes *b : {&st->rec, &st->order, &st->out, &st->sums, &st->pack, &st->bbox, &st->warped, &st->residual, &st->owner,
                        &st->count, &st->grid.cell_of, &st->grid.start, &st->grid.cursor, &st->grid.unordered, &st->grid.members})
    b->release();
  if (st->h_bbox)
    (void)hipHostFree(st->h_bbox);
  if (st->h_count)
    (void)hipHostFree(st->h_count);
  if (st->ev0)
    (void)hipEventDestroy(st->ev0);
  if (st->ev1)
    (void)hipEventDestroy(st->ev1);
  delete st;
}

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
  LkUncertaintyView v{};
  if (int rc = lk_internal_uncertainty_view(e, records ? 0 : 1, cfg->def_slot, &v))
    return rc;
  ResidualState *st = nullptr;
  if (int rc = get_state(e, &st))
    return rc;
  const size_t n = (size_t)v.S;
  // the sectors by lane group: from the level-0 sample count alone, as lk_parameter_uncertainty
  st->h_order.resize(n);
  int count[3] = {0, 0, 0};
  size_t at = 0;
  for (int g = 0; g < 3; ++g) {
    const size_t begin = at;
    for (int s = 0; s < v.S; ++s) {
      const int4 r = v.h_rect0[s];
      const int n0 = r.z > 0 ? r.w : (int)(v.h_off0[s + 1] - v.h_off0[s]);
      if (lk_bw_group(n0) == kGroups[g])
        st->h_order[at++] = (uint32_t)s;
    }
    count[g] = (int)(at - begin);
  }
  RSCHK(st->order.ensure(n * sizeof(uint32_t)));
  RSCHK(st->out.ensure(n * sizeof(struct lk_photometry)));
  if (sums_out)
    RSCHK(st->sums.ensure(n * kLkPhotoSums * sizeof(double)));
  RSCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  const lk_result *d_rec = v.result;
  if (records) {
    RSCHK(st->rec.ensure(n * sizeof(lk_result)));
    RSCHK(hipMemcpyAsync(st->rec.p, records, n * sizeof(lk_result), hipMemcpyHostToDevice, v.stream));
    d_rec = st->rec.as<lk_result>();
  }
  LkPhotometryArgs a{};
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
  a.out = st->out.as<struct lk_photometry>();
  a.sums = sums_out ? st->sums.as<double>() : nullptr;
  a.level = v.level;
  a.chi_max = cfg->chi_max;
  st->timed = false;
  RSCHK(hipEventRecord(st->ev0, v.stream));
  const uint32_t *order = st->order.as<uint32_t>();
  for (int g = 0; g < 3; ++g) {
    a.order = order;
    a.n_sectors = count[g];
    if (a.n_sectors > 0)
      RSCHK(lk_launch_photometry(a, v.model, v.interp, kGroups[g], v.stream));
    order += count[g];
  }
  RSCHK(hipEventRecord(st->ev1, v.stream));
  RSCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(struct lk_photometry), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    RSCHK(hipMemcpyAsync(sums_out, st->sums.p, n * kLkPhotoSums * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  RSCHK(hipStreamSynchronize(v.stream));
  st->tiles = st->fallback = 0;
  st->timed = true;
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
  LkUncertaintyView v{};
  if (int rc = lk_internal_uncertainty_view(e, records ? 0 : 1, cfg->def_slot, &v))
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
  if (int rc = get_state(e, &st))
    return rc;
  const size_t n = (size_t)v.S, pixels = (size_t)w * (size_t)h;
  RSCHK(st->pack.ensure(n * sizeof(LkMapSector)));
  RSCHK(st->bbox.ensure(4 * sizeof(float)));
  RSCHK(st->count.ensure(sizeof(uint32_t)));
  if (warped)
    RSCHK(st->warped.ensure(pixels * sizeof(float)));
  if (residual)
    RSCHK(st->residual.ensure(pixels * sizeof(float)));
  if (owner)
    RSCHK(st->owner.ensure(pixels * sizeof(int32_t)));
  const lk_result *d_rec = v.result;
  if (records) {
    RSCHK(st->rec.ensure(n * sizeof(lk_result)));
    RSCHK(hipMemcpyAsync(st->rec.p, records, n * sizeof(lk_result), hipMemcpyHostToDevice, v.stream));
    d_rec = st->rec.as<lk_result>();
  }
  st->timed = false;
  RSCHK(hipEventRecord(st->ev0, v.stream));
  // the centres' bounding box sizes the grid: the call's one round trip before the kernels
  RSCHK(lk_launch_reseed_bbox(v.center, v.S, st->bbox.as<float>(), v.stream));
  RSCHK(hipMemcpyAsync(st->h_bbox, st->bbox.p, 4 * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  RSCHK(hipStreamSynchronize(v.stream));
  if (!lk_cell_grid_bbox_finite(st->h_bbox))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_residual_map: a sector centre is not finite");
  LkResidualMapArgs a{};
  RSCHK(lk_cell_grid_build(st->grid, v.center, v.S, cfg->radius, st->h_bbox, v.stream, &a.grid));
  RSCHK(lk_launch_map_prep(d_rec, v.center, v.S, v.model, v.level, cfg->chi_max, st->pack.as<LkMapSector>(), v.stream));
  RSCHK(hipMemsetAsync(st->count.p, 0, sizeof(uint32_t), v.stream));
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
  RSCHK(lk_launch_residual_map(a, v.model, v.interp, &tiles, v.stream));
  RSCHK(hipEventRecord(st->ev1, v.stream));
  if (warped)
    RSCHK(hipMemcpyAsync(warped, st->warped.p, pixels * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  if (residual)
    RSCHK(hipMemcpyAsync(residual, st->residual.p, pixels * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  if (owner)
    RSCHK(hipMemcpyAsync(owner, st->owner.p, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
  RSCHK(hipMemcpyAsync(st->h_count, st->count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
  RSCHK(hipStreamSynchronize(v.stream));
  st->tiles = tiles;
  st->fallback = (int)*st->h_count;
  st->timed = true;
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_residual_last(lk_engine *e, float *device_ms, int *tiles, int *fallback_tiles) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  ResidualState *st = (ResidualState *)*lk_internal_residual_slot(e);
  if (!st || !st->timed)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_internal_residual_last: no lk_photometry or lk_residual_map yet");
  if (device_ms)
    RSCHK(hipEventElapsedTime(device_ms, st->ev0, st->ev1));
  if (tiles)
    *tiles = st->tiles;
  if (fallback_tiles)
    *fallback_tiles = st->fallback;
  return LK_ERROR_NONE;
}

} // extern "C"
