// lk_field.cpp - host side of the field map (include/lk_engine.h: lk_field_map, lk_field_from_sums).  The kernel is
// lk_field.hip; the node's arithmetic is lk_field.hpp; the pack is lk_strain.hip's; the bounding box and the cell grid are the
// recovery pass's (lk_reseed.hip through lk_cell_grid.hpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lk_engine.h"
#include "lk_field.hpp"
#include "lk_launch.hpp"
#include "lk_pass.hpp"

namespace {

struct FieldState : LkPassState {
  LkDevBytes rec, pack, bbox, maps, neighbours, status, count;
  LkCellGridBufs grid;
  uint32_t *h_count = nullptr; // pinned [1]
  int tiles = 0, fallback = 0;
  hipError_t init() {
    const hipError_t err = LkPassState::init();
    return err != hipSuccess ? err : hipHostMalloc((void **)&h_count, sizeof(uint32_t), hipHostMallocDefault);
  }
  ~FieldState() override {
    if (h_count)
      (void)hipHostFree(h_count);
  }
};

} // namespace

extern "C" {

int lk_field_from_sums(int min_neighbours, int n, double W, const double *sums11, int tensor, float *out12, int32_t *status) {
  if (!sums11 || !out12 || !status || n < 0 || min_neighbours < 3 || (tensor != LK_STRAIN_GREEN_LAGRANGE && tensor != LK_STRAIN_SMALL))
    return LK_ERROR_BAD_DOMAIN;
  *status = lk_field_from_sums_impl(min_neighbours, n, W, sums11, tensor, out12);
  return LK_ERROR_NONE;
}

int lk_field_map(lk_engine *e, const lk_field_map_config *cfg, const lk_result *records, float *maps, int32_t *neighbours,
                 uint8_t *status) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: no configuration");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: reserved words must be 0");
  if (!std::isfinite(cfg->radius) || !(cfg->radius > 0.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: radius must be finite and positive");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: chi_max must be finite (<= 0: the error code alone decides)");
  if (cfg->min_neighbours < 3)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: min_neighbours must be at least 3 (a plane has three unknowns)");
  if (cfg->tensor != LK_STRAIN_GREEN_LAGRANGE && cfg->tensor != LK_STRAIN_SMALL)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: unknown tensor");
  if (cfg->weight != LK_FIELD_UNIFORM && cfg->weight != LK_FIELD_BISQUARE)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: unknown weight");
  if (cfg->frame != LK_FIELD_REFERENCE && cfg->frame != LK_FIELD_DEFORMED)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: unknown frame");
  if (cfg->frame == LK_FIELD_DEFORMED && (cfg->iterations < 1 || cfg->iterations > kLkFieldMaxIterations))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: iterations must be 1 .. 16 in the deformed frame");
  if (cfg->nx < 1 || cfg->ny < 1 || cfg->stride < 1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: nx, ny and stride must be at least 1");
  if ((long long)cfg->nx * (long long)cfg->ny > 0x7fffffffLL)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: more than 2^31 - 1 nodes");
  if (cfg->channels >> kLkFieldChannels != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: unknown channel bits");
  if (cfg->channels == 0 && !neighbours && !status)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: no output");
  if (cfg->channels != 0 && !maps)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_field_map: channels selected but no maps");
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_field_map", records ? 0 : LK_VIEW_RECORDS, -1, &v))
    return rc;
  FieldState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_FIELD, "hipHostMalloc / hipEventCreate (lk_field_map)", &st))
    return rc;
  const size_t n = (size_t)v.S, nodes = (size_t)cfg->nx * (size_t)cfg->ny;
  const size_t planes = (size_t)__builtin_popcount(cfg->channels);
  LK_HIPCHK(st->pack.ensure(n * sizeof(float4)));
  LK_HIPCHK(st->bbox.ensure(4 * sizeof(float)));
  LK_HIPCHK(st->count.ensure(sizeof(uint32_t)));
  if (planes)
    LK_HIPCHK(st->maps.ensure(planes * nodes * sizeof(float)));
  if (neighbours)
    LK_HIPCHK(st->neighbours.ensure(nodes * sizeof(int32_t)));
  if (status)
    LK_HIPCHK(st->status.ensure(nodes));
  const lk_result *d_rec = v.result;
  if (int rc = lk_pass_records(e, st->rec, records, n, v.stream, &d_rec))
    return rc;
  LK_HIPCHK(st->begin(v.stream));
  LkFieldArgs a{};
  if (int rc = lk_pass_grid(e, "lk_field_map", st, st->bbox, st->grid, v.center, v.S, cfg->radius, v.stream, &a.grid))
    return rc;
  LK_HIPCHK(lk_launch_pack_prep(d_rec, v.center, v.S, 1, v.model, cfg->chi_max, 0, nullptr, st->pack.as<float4>(), v.stream));
  LK_HIPCHK(hipMemsetAsync(st->count.p, 0, sizeof(uint32_t), v.stream));
  a.pack = st->pack.as<float4>();
  a.maps = planes ? st->maps.as<float>() : nullptr;
  a.neighbours = neighbours ? st->neighbours.as<int32_t>() : nullptr;
  a.status = status ? st->status.as<uint8_t>() : nullptr;
  a.fallback = st->count.as<uint32_t>();
  a.n_sectors = v.S;
  a.min_neighbours = cfg->min_neighbours;
  a.tensor = cfg->tensor;
  a.iterations = cfg->frame == LK_FIELD_DEFORMED ? cfg->iterations : 0;
  a.x0 = cfg->x0;
  a.y0 = cfg->y0;
  a.nx = cfg->nx;
  a.ny = cfg->ny;
  a.stride = cfg->stride;
  a.tiles_x = (cfg->nx + kLkMapTileW - 1) / kLkMapTileW;
  // test hook and tuning experiments (scripts/field_map_bench.py): LK_FIELD_WALK = 1 stages nothing, every node walks
  a.walk = lk_pass_env_choice("LK_FIELD_WALK", 0, 1, 0);
  a.channels = cfg->channels;
  a.r2 = (double)cfg->radius * (double)cfg->radius;
  int tiles = 0;
  LK_HIPCHK(lk_launch_field_map(a, cfg->weight, cfg->frame, &tiles, v.stream));
  LK_HIPCHK(st->end(v.stream));
  if (planes)
    LK_HIPCHK(hipMemcpyAsync(maps, st->maps.p, planes * nodes * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  if (neighbours)
    LK_HIPCHK(hipMemcpyAsync(neighbours, st->neighbours.p, nodes * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
  if (status)
    LK_HIPCHK(hipMemcpyAsync(status, st->status.p, nodes, hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipMemcpyAsync(st->h_count, st->count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->tiles = tiles;
  st->fallback = (int)*st->h_count;
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_field_last(lk_engine *e, float *device_ms, int *tiles, int *fallback_tiles) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  FieldState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_FIELD, "lk_internal_field_last: no lk_field_map yet", device_ms, &st))
    return rc;
  if (tiles)
    *tiles = st->tiles;
  if (fallback_tiles)
    *fallback_tiles = st->fallback;
  return LK_ERROR_NONE;
}

} // extern "C"
