// lk_strain.cpp - host side of the strain field (include/lk_engine.h: lk_strain_field).  The kernels are lk_strain.hip;
// the bounding box and the cell grid are the recovery pass's (lk_reseed.hip through lk_cell_grid.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <initializer_list>

#include "../../include/lk_engine.h"
#include "lk_cell_grid.hpp"
#include "lk_device.hpp"
#include "lk_internal.hpp"
#include "lk_launch.hpp"

#define STCHK(call)                                                                                   \
  do {                                                                                                \
    hipError_t _e = (call);                                                                           \
    if (_e != hipSuccess)                                                                             \
      return lk_internal_hipfail(e, _e, #call);                                                       \
  } while (0)

namespace {

// Lanes per sector: a 16-lane row while the 3 x 3 cells around a sector hold at most this many members on average
// (9 S / cells, known on the host), a whole wavefront above.  Measured on an MI355X (profiles/strain_bench.txt): the
// 16-lane row is the faster one on every case, by 1.2 - 1.8 x at 56 members (2.5 pitches) and still by 1.24 x at 502
// (7.5 pitches, four sectors' walks in flight per wavefront hide more latency than one).  The switch lies at twice the
// largest window measured; nothing above it has been timed.
constexpr double kWideGroupFrom = 1024.0;

struct StrainState {
  LkDevBytes rec, good, pack, out, bbox;
  LkCellGridBufs grid;
  float *h_bbox = nullptr; // pinned [4]
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;      // ev0 / ev1 bracket the device part of a finished call (read by lk_internal_strain_last)
  int group = 0, packed = 0;
  double members = 0;      // expected members of the 3 x 3 cells of the last call
};

int get_state(lk_engine *e, StrainState **out) {
  void **slot = lk_internal_strain_slot(e);
  if (!*slot) {
    StrainState *st = new StrainState();
    hipError_t err = hipHostMalloc((void **)&st->h_bbox, 4 * sizeof(float), hipHostMallocDefault);
    if (err == hipSuccess)
      err = hipEventCreate(&st->ev0);
    if (err == hipSuccess)
      err = hipEventCreate(&st->ev1);
    if (err != hipSuccess) {
      lk_internal_strain_release(st);
      return lk_internal_hipfail(e, err, "hipHostMalloc / hipEventCreate (lk_strain_field)");
    }
    *slot = st;
  }
  *out = (StrainState *)*slot;
  return LK_ERROR_NONE;
}

// tuning experiments (scripts/strain_bench.py): LK_STRAIN_GROUP = 16 / 64 and LK_STRAIN_PACKED = 0 / 1 override the choice
int env_choice(const char *name, int a, int b, int otherwise) {
  const char *s = std::getenv(name);
  if (!s || !*s)
    return otherwise;
  const int v = std::atoi(s);
  return v == a || v == b ? v : otherwise;
}

} // namespace

void lk_internal_strain_release(void *state) {
  StrainState *st = (StrainState *)state;
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

int lk_strain_field(lk_engine *e, const lk_strain_config *cfg, const lk_result *records, lk_strain *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_strain_field: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_strain_field: no output");
  if (!std::isfinite(cfg->radius) || !(cfg->radius > 0.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_strain_field: radius must be finite and positive");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_strain_field: chi_max must be finite (<= 0: the error code alone decides)");
  if (cfg->min_neighbours < 3)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_strain_field: min_neighbours must be at least 3 (a plane has three unknowns)");
  if (cfg->tensor != LK_STRAIN_GREEN_LAGRANGE && cfg->tensor != LK_STRAIN_SMALL)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_strain_field: unknown tensor");
  LkStrainView v{};
  if (int rc = lk_internal_strain_view(e, records ? 0 : 1, &v))
    return rc;
  StrainState *st = nullptr;
  if (int rc = get_state(e, &st))
    return rc;
  const size_t n = (size_t)v.S;
  STCHK(st->good.ensure(n));
  STCHK(st->pack.ensure(n * sizeof(float4)));
  STCHK(st->out.ensure(n * sizeof(lk_strain)));
  STCHK(st->bbox.ensure(4 * sizeof(float)));
  const lk_result *d_rec = v.result;
  if (records) {
    STCHK(st->rec.ensure(n * sizeof(lk_result)));
    STCHK(hipMemcpyAsync(st->rec.p, records, n * sizeof(lk_result), hipMemcpyHostToDevice, v.stream));
    d_rec = st->rec.as<lk_result>();
  }
  st->timed = false;
  STCHK(hipEventRecord(st->ev0, v.stream));
  // the centres' bounding box sizes the grid: the call's one round trip before the kernels
  STCHK(lk_launch_reseed_bbox(v.center, v.S, st->bbox.as<float>(), v.stream));
  STCHK(hipMemcpyAsync(st->h_bbox, st->bbox.p, 4 * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  STCHK(hipStreamSynchronize(v.stream));
  if (!lk_cell_grid_bbox_finite(st->h_bbox))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_strain_field: a sector centre is not finite");
  LkStrainArgs a{};
  STCHK(lk_cell_grid_build(st->grid, v.center, v.S, cfg->radius, st->h_bbox, v.stream, &a.grid));
  STCHK(lk_launch_strain_prep(d_rec, v.center, v.S, v.model, cfg->chi_max, st->good.as<uint8_t>(), st->pack.as<float4>(), v.stream));
  a.center = v.center;
  a.rec = d_rec;
  a.good = st->good.as<uint8_t>();
  a.pack = st->pack.as<float4>();
  a.out = st->out.as<lk_strain>();
  a.n_sectors = v.S;
  a.has_v = v.model == LK_FM_U ? 0 : 1;
  a.min_neighbours = cfg->min_neighbours;
  a.tensor = cfg->tensor;
  a.radius = (double)cfg->radius;
  st->members = 9.0 * (double)v.S / ((double)a.grid.nx * (double)a.grid.ny);
  st->group = env_choice("LK_STRAIN_GROUP", 16, 64, st->members > kWideGroupFrom ? 64 : 16);
  st->packed = env_choice("LK_STRAIN_PACKED", 0, 1, 1);
  STCHK(lk_launch_strain(a, st->group, st->packed, v.stream));
  STCHK(hipEventRecord(st->ev1, v.stream));
  STCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(lk_strain), hipMemcpyDeviceToHost, v.stream));
  STCHK(hipStreamSynchronize(v.stream));
  st->timed = true;
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_strain_last(lk_engine *e, float *device_ms, int *group, int *packed, double *members) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  StrainState *st = (StrainState *)*lk_internal_strain_slot(e);
  if (!st || !st->timed)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_internal_strain_last: no lk_strain_field yet");
  if (device_ms)
    STCHK(hipEventElapsedTime(device_ms, st->ev0, st->ev1));
  if (group)
    *group = st->group;
  if (packed)
    *packed = st->packed;
  if (members)
    *members = st->members;
  return LK_ERROR_NONE;
}

} // extern "C"
