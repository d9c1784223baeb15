// lk_track.cpp - host side of the material-point tracks (include/lk_engine.h: lk_track_points, lk_track_step,
// lk_gauges_from_tracks).  The kernels are lk_track.hip; the bounding box and the cell grid are the recovery pass's
// (lk_reseed.hip through lk_cell_grid.hpp); the per-frame step is lk_track.hpp's, here compiled for the host as well.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_track.hpp"

namespace {

// Lanes per point: lk_strain.cpp's rule - a 16-lane row while the 3 x 3 cells around a position hold at most this many
// members on average (9 S / cells), a whole wavefront above.  Measured on an MI355X (profiles/track_bench.txt): the 16-lane
// row is the faster one on every case, by 1.1 - 1.7 x at one frame and 1.3 - 3.5 x at 64 frames, still by 1.1 - 1.5 x at 502
// members (7.5 pitches).  The switch lies at twice the largest window measured; nothing above it has been timed.
constexpr double kWideGroupFrom = 1024.0;

struct TrackState : LkPassState {
  LkDevBytes rec, pack, state, out, bbox;
  LkCellGridBufs grid;
  int group = 0;
  double members = 0; // expected members of the 3 x 3 cells of the last call
};

} // namespace

extern "C" {

int lk_track_points(lk_engine *e, const lk_track_config *cfg, int n_points, const float *points_xy, int n_frames,
                    const lk_result *records, double *state_inout, lk_track *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: no output");
  if (n_points < 1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: n_points must be at least 1");
  if (!points_xy && !state_inout)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: neither points nor a state to continue from");
  if (!std::isfinite(cfg->radius) || !(cfg->radius > 0.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: radius must be finite and positive");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: chi_max must be finite (<= 0: the error code alone decides)");
  if (cfg->min_neighbours < 3)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: min_neighbours must be at least 3 (a plane has three unknowns)");
  if (cfg->tensor != LK_STRAIN_GREEN_LAGRANGE && cfg->tensor != LK_STRAIN_SMALL)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: unknown tensor");
  if (cfg->mode != LK_TRACK_TOTAL && cfg->mode != LK_TRACK_INCREMENTAL)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: unknown mode");
  if (cfg->source != LK_TRACK_RECORDS_CALLER && cfg->source != LK_TRACK_RECORDS_ENGINE && cfg->source != LK_TRACK_RECORDS_WINDOW)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: unknown source");
  if (cfg->source == LK_TRACK_RECORDS_CALLER) {
    if (!records)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: source CALLER needs records");
    if (n_frames < 1)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: n_frames must be at least 1");
  } else if (records) {
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: records must be NULL unless the source is CALLER");
  } else if (cfg->source == LK_TRACK_RECORDS_ENGINE && n_frames != 1) {
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: n_frames must be 1 for the engine-held records of a batch solve");
  } else if (cfg->source == LK_TRACK_RECORDS_WINDOW && n_frames < 0) {
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: n_frames must be 0 or the window's frame count");
  }
  LkPassView v{};
  const unsigned need = cfg->source == LK_TRACK_RECORDS_ENGINE ? LK_VIEW_RECORDS : cfg->source == LK_TRACK_RECORDS_WINDOW ? LK_VIEW_WINDOW : 0u;
  if (int rc = lk_internal_pass_view(e, "lk_track_points", need, -1, &v))
    return rc;
  if (cfg->source == LK_TRACK_RECORDS_WINDOW) {
    if (n_frames != 0 && n_frames != v.window_frames)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_track_points: n_frames must be 0 or the window's frame count");
    n_frames = v.window_frames;
  }
  TrackState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_TRACK, "hipHostMalloc / hipEventCreate (lk_track_points)", &st))
    return rc;
  const size_t S = (size_t)v.S, F = (size_t)n_frames, Q = (size_t)n_points;
  std::vector<double> h_state(Q * 8);
  for (size_t q = 0; q < Q; ++q) {
    double *s = h_state.data() + q * 8;
    if (points_xy) {
      const double X = (double)points_xy[2 * q], Y = (double)points_xy[2 * q + 1];
      s[0] = X, s[1] = Y, s[2] = X, s[3] = Y, s[4] = 1.0, s[5] = 0.0, s[6] = 0.0, s[7] = 1.0;
    } else {
      for (int i = 0; i < 8; ++i)
        s[i] = state_inout[q * 8 + i];
    }
  }
  LK_HIPCHK(st->pack.ensure(F * S * sizeof(float4)));
  LK_HIPCHK(st->state.ensure(Q * 8 * sizeof(double)));
  LK_HIPCHK(st->out.ensure(F * Q * sizeof(lk_track)));
  LK_HIPCHK(st->bbox.ensure(4 * sizeof(float)));
  const lk_result *d_rec = cfg->source == LK_TRACK_RECORDS_WINDOW ? v.window : v.result;
  if (int rc = lk_pass_records(e, st->rec, records, F * S, v.stream, &d_rec))
    return rc;
  LK_HIPCHK(hipMemcpyAsync(st->state.p, h_state.data(), Q * 8 * sizeof(double), hipMemcpyHostToDevice, v.stream)); // (pageable: staged before it returns)
  LK_HIPCHK(st->begin(v.stream));
  LkTrackArgs a{};
  if (int rc = lk_pass_grid(e, "lk_track_points", st, st->bbox, st->grid, v.center, v.S, cfg->radius, v.stream, &a.grid))
    return rc;
  LK_HIPCHK(lk_launch_pack_prep(d_rec, v.center, v.S, n_frames, v.model, cfg->chi_max, 0, nullptr, st->pack.as<float4>(), v.stream));
  a.pack = st->pack.as<float4>();
  a.state = st->state.as<double>();
  a.out = st->out.as<lk_track>();
  a.n_points = n_points;
  a.n_frames = n_frames;
  a.n_sectors = v.S;
  a.min_neighbours = cfg->min_neighbours;
  a.tensor = cfg->tensor;
  a.mode = cfg->mode;
  a.radius = (double)cfg->radius;
  st->members = 9.0 * (double)v.S / ((double)a.grid.nx * (double)a.grid.ny);
  // tuning experiments (scripts/track_bench.py): LK_TRACK_GROUP = 16 / 64 overrides the choice
  st->group = lk_pass_env_choice("LK_TRACK_GROUP", 16, 64, st->members > kWideGroupFrom ? 64 : 16);
  LK_HIPCHK(lk_launch_track(a, st->group, v.stream));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(h_state.data(), st->state.p, Q * 8 * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipMemcpyAsync(out, st->out.p, F * Q * sizeof(lk_track), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  if (state_inout)
    for (size_t i = 0; i < Q * 8; ++i)
      state_inout[i] = h_state[i];
  st->finished();
  return LK_ERROR_NONE;
}

int lk_track_step(int mode, int min_neighbours, int n, const double *sums11, double *state8, int tensor, lk_track *out) {
  if (!sums11 || !state8 || !out || n < 0 || min_neighbours < 3 || (mode != LK_TRACK_TOTAL && mode != LK_TRACK_INCREMENTAL) ||
      (tensor != LK_STRAIN_GREEN_LAGRANGE && tensor != LK_STRAIN_SMALL))
    return LK_ERROR_BAD_DOMAIN;
  lk_track_step_impl(mode, min_neighbours, n, sums11, state8, tensor, out);
  return LK_ERROR_NONE;
}

int lk_gauges_from_tracks(int n_frames, int n_points, const lk_track *tracks, int n_gauges, const int32_t *pairs_ij, float *out4) {
  if (!tracks || !pairs_ij || !out4 || n_frames < 1 || n_points < 1 || n_gauges < 1)
    return LK_ERROR_BAD_DOMAIN;
  for (int g = 0; g < 2 * n_gauges; ++g)
    if (pairs_ij[g] < 0 || pairs_ij[g] >= n_points)
      return LK_ERROR_BAD_DOMAIN;
  for (int f = 0; f < n_frames; ++f)
    for (int g = 0; g < n_gauges; ++g) {
      const lk_track &a = tracks[(size_t)f * (size_t)n_points + (size_t)pairs_ij[2 * g]];
      const lk_track &b = tracks[(size_t)f * (size_t)n_points + (size_t)pairs_ij[2 * g + 1]];
      float *o = out4 + ((size_t)f * (size_t)n_gauges + (size_t)g) * 4;
      o[0] = o[1] = o[2] = o[3] = 0.f;
      if (a.status != LK_TRACK_OK || b.status != LK_TRACK_OK)
        continue;
      const double dx = (double)b.x - (double)a.x, dy = (double)b.y - (double)a.y;
      const double dx0 = ((double)b.x - (double)b.u) - ((double)a.x - (double)a.u);
      const double dy0 = ((double)b.y - (double)b.v) - ((double)a.y - (double)a.v);
      const double L = std::sqrt(dx * dx + dy * dy), L0 = std::sqrt(dx0 * dx0 + dy0 * dy0);
      if (L0 == 0.0)
        continue;
      o[0] = (float)L;
      o[1] = (float)((L - L0) / L0);
      o[2] = (float)std::log(L / L0);
      o[3] = (float)std::atan2(dx0 * dy - dy0 * dx, dx0 * dx + dy0 * dy);
    }
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_track_last(lk_engine *e, float *device_ms, int *group, double *members) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  TrackState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_TRACK, "lk_internal_track_last: no lk_track_points yet", device_ms, &st))
    return rc;
  if (group)
    *group = st->group;
  if (members)
    *members = st->members;
  return LK_ERROR_NONE;
}

} // extern "C"
