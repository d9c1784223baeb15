// lk_strain.cpp - host side of the strain field (include/lk_engine.h: lk_strain_field).  The kernels are lk_strain.hip;
// the bounding box and the cell grid are the recovery pass's (lk_reseed.hip through lk_cell_grid.hpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"

namespace {

// Lanes per sector: a 16-lane row while the 3 x 3 cells around a sector hold at most this many members on average
// (9 S / cells, known on the host), a whole wavefront above.  Measured on an MI355X (profiles/strain_bench.txt): the
// 16-lane row is the faster one on every case, by 1.2 - 1.8 x at 56 members (2.5 pitches) and still by 1.24 x at 502
// (7.5 pitches, four sectors' walks in flight per wavefront hide more latency than one).  The switch lies at twice the
// largest window measured; nothing above it has been timed.
constexpr double kWideGroupFrom = 1024.0;

struct StrainState : LkPassState {
  LkDevBytes rec, good, pack, out, bbox;
  LkCellGridBufs grid;
  int group = 0, packed = 0;
  double members = 0; // expected members of the 3 x 3 cells of the last call
};

} // namespace

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
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_strain_field", records ? 0 : LK_VIEW_RECORDS, -1, &v))
    return rc;
  StrainState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_STRAIN, "hipHostMalloc / hipEventCreate (lk_strain_field)", &st))
    return rc;
  const size_t n = (size_t)v.S;
  LK_HIPCHK(st->good.ensure(n));
  LK_HIPCHK(st->pack.ensure(n * sizeof(float4)));
  LK_HIPCHK(st->out.ensure(n * sizeof(lk_strain)));
  LK_HIPCHK(st->bbox.ensure(4 * sizeof(float)));
  const lk_result *d_rec = v.result;
  if (int rc = lk_pass_records(e, st->rec, records, n, v.stream, &d_rec))
    return rc;
  LK_HIPCHK(st->begin(v.stream));
  LkStrainArgs a{};
  if (int rc = lk_pass_grid(e, "lk_strain_field", st, st->bbox, st->grid, v.center, v.S, cfg->radius, v.stream, &a.grid))
    return rc;
  LK_HIPCHK(lk_launch_pack_prep(d_rec, v.center, v.S, 1, v.model, cfg->chi_max, 0, st->good.as<uint8_t>(), st->pack.as<float4>(), v.stream));
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
  // tuning experiments (scripts/strain_bench.py): LK_STRAIN_GROUP = 16 / 64 and LK_STRAIN_PACKED = 0 / 1 override the choice
  st->group = lk_pass_env_choice("LK_STRAIN_GROUP", 16, 64, st->members > kWideGroupFrom ? 64 : 16);
  st->packed = lk_pass_env_choice("LK_STRAIN_PACKED", 0, 1, 1);
  LK_HIPCHK(lk_launch_strain(a, st->group, st->packed, v.stream));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(lk_strain), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_strain_last(lk_engine *e, float *device_ms, int *group, int *packed, double *members) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  StrainState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_STRAIN, "lk_internal_strain_last: no lk_strain_field yet", device_ms, &st))
    return rc;
  if (group)
    *group = st->group;
  if (packed)
    *packed = st->packed;
  if (members)
    *members = st->members;
  return LK_ERROR_NONE;
}

} // extern "C"
