// lk_motion.cpp - host side of the global motion per frame (include/lk_engine.h: lk_rigid_motion, lk_motion_from_sums,
// lk_motion_apply, lk_motion_remove).  The kernels are lk_motion.hip; the bounding box is the recovery pass's
// (lk_reseed.hip); the fit and the removal are lk_motion.hpp's, here compiled for the host as well.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_motion.hpp"
#include "lk_pass.hpp"

namespace {

// Sectors per chunk, one workgroup each: eight per lane.  LK_MOTION_CHUNK = 64 (tests: a small domain then spans several
// chunks) / 2048 overrides it.
constexpr int kChunk = 2048, kChunkSmall = 64;

struct MotionState : LkPassState {
  LkDevBytes rec, pack, mask, keep, partial, sums, fit, out, rec_out, bbox;
  int chunk = 0, chunks = 0;
};

bool known_kind(int kind) { return kind >= LK_MOTION_TRANSLATION && kind <= LK_MOTION_AFFINE; }

} // namespace

extern "C" {

int lk_rigid_motion(lk_engine *e, const lk_motion_config *cfg, int n_frames, const lk_result *records, const uint8_t *fit_mask,
                    lk_motion *out, lk_result *records_out, double *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: no output");
  if (!known_kind(cfg->kind))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: unknown kind");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: chi_max must be finite (<= 0: the error code alone decides)");
  if (!std::isfinite(cfg->reject))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: reject must be finite (<= 0: no trimming)");
  if (cfg->passes < 1 || cfg->passes > 4)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: passes must be 1 .. 4");
  if (cfg->passes > 1 && !(cfg->reject > 0.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: passes > 1 needs reject > 0");
  if (cfg->min_sectors < lk_motion_min_sectors(cfg->kind))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: min_sectors is below the kind's minimum (1, 2, 2, 3 unknowns' worth of sectors)");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: reserved words must be 0");
  if (cfg->source != LK_TRACK_RECORDS_CALLER && cfg->source != LK_TRACK_RECORDS_ENGINE && cfg->source != LK_TRACK_RECORDS_WINDOW)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: unknown source");
  if (cfg->source == LK_TRACK_RECORDS_CALLER) {
    if (!records)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: source CALLER needs records");
    if (n_frames < 1)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: n_frames must be at least 1");
  } else if (records) {
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: records must be NULL unless the source is CALLER");
  } else if (cfg->source == LK_TRACK_RECORDS_ENGINE && n_frames != 1) {
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: n_frames must be 1 for the engine-held records of a batch solve");
  } else if (cfg->source == LK_TRACK_RECORDS_WINDOW && n_frames < 0) {
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: n_frames must be 0 or the window's frame count");
  }
  LkPassView v{};
  const unsigned need = cfg->source == LK_TRACK_RECORDS_ENGINE ? LK_VIEW_RECORDS : cfg->source == LK_TRACK_RECORDS_WINDOW ? LK_VIEW_WINDOW : 0u;
  if (int rc = lk_internal_pass_view(e, "lk_rigid_motion", need, -1, &v))
    return rc;
  if (cfg->source == LK_TRACK_RECORDS_WINDOW) {
    if (n_frames != 0 && n_frames != v.window_frames)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: n_frames must be 0 or the window's frame count");
    n_frames = v.window_frames;
  }
  if (n_frames > 65535)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: n_frames must be at most 65535 per call");
  if (v.model == LK_FM_U && cfg->kind != LK_MOTION_TRANSLATION)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: LK_FM_U has no v: the kind must be LK_MOTION_TRANSLATION");
  MotionState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_MOTION, "hipHostMalloc / hipEventCreate (lk_rigid_motion)", &st))
    return rc;
  const size_t S = (size_t)v.S, F = (size_t)n_frames;
  st->chunk = lk_pass_env_choice("LK_MOTION_CHUNK", kChunkSmall, kChunk, kChunk);
  st->chunks = (v.S + st->chunk - 1) / st->chunk;
  LK_HIPCHK(st->pack.ensure(F * S * sizeof(float4)));
  LK_HIPCHK(st->keep.ensure(F * S));
  LK_HIPCHK(st->partial.ensure(F * (size_t)st->chunks * kLkMotionPartial * sizeof(double)));
  LK_HIPCHK(st->sums.ensure(F * 12 * sizeof(double)));
  LK_HIPCHK(st->fit.ensure(F * sizeof(LkMotionFit)));
  LK_HIPCHK(st->out.ensure(F * sizeof(lk_motion)));
  LK_HIPCHK(st->bbox.ensure(4 * sizeof(float)));
  if (records_out)
    LK_HIPCHK(st->rec_out.ensure(F * S * sizeof(lk_result)));
  const lk_result *d_rec = cfg->source == LK_TRACK_RECORDS_WINDOW ? v.window : v.result;
  if (int rc = lk_pass_records(e, st->rec, records, F * S, v.stream, &d_rec))
    return rc;
  if (fit_mask) {
    LK_HIPCHK(st->mask.ensure(S));
    LK_HIPCHK(hipMemcpyAsync(st->mask.p, fit_mask, S, hipMemcpyHostToDevice, v.stream)); // (pageable: staged before it returns)
  }
  // the origin of the sums: the centre of the centres' bounding box (the call's one round trip before its kernels)
  LK_HIPCHK(lk_launch_reseed_bbox(v.center, v.S, st->bbox.as<float>(), v.stream));
  LK_HIPCHK(hipMemcpyAsync(st->h_bbox, st->bbox.p, 4 * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  if (!lk_cell_grid_bbox_finite(st->h_bbox))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_rigid_motion: a sector centre is not finite");
  LkMotionArgs a{};
  a.ox = ((double)st->h_bbox[0] + (double)st->h_bbox[2]) / 2.0;
  a.oy = ((double)st->h_bbox[1] + (double)st->h_bbox[3]) / 2.0;
  a.pack = st->pack.as<float4>();
  a.fit_mask = fit_mask ? st->mask.as<uint8_t>() : nullptr;
  a.keep = st->keep.as<uint8_t>();
  a.partial = st->partial.as<double>();
  a.sums = st->sums.as<double>();
  a.fit = st->fit.as<LkMotionFit>();
  a.out = st->out.as<lk_motion>();
  a.rec = d_rec;
  a.center = v.center;
  a.rec_out = st->rec_out.as<lk_result>();
  a.n_frames = n_frames;
  a.n_sectors = v.S;
  a.chunk = st->chunk;
  a.chunks = st->chunks;
  a.kind = cfg->kind;
  a.min_sectors = cfg->min_sectors;
  a.model = v.model;
  a.reject = (double)cfg->reject;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(lk_launch_pack_prep(d_rec, v.center, v.S, n_frames, v.model, cfg->chi_max, 0, nullptr, st->pack.as<float4>(), v.stream));
  for (a.pass = 0; a.pass < cfg->passes; ++a.pass)
    LK_HIPCHK(lk_launch_motion_pass(a, v.stream));
  if (records_out)
    LK_HIPCHK(lk_launch_motion_remove(a, v.stream));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(out, st->out.p, F * sizeof(lk_motion), hipMemcpyDeviceToHost, v.stream));
  if (records_out)
    LK_HIPCHK(hipMemcpyAsync(records_out, st->rec_out.p, F * S * sizeof(lk_result), hipMemcpyDeviceToHost, v.stream));
  if (sums_out)
    LK_HIPCHK(hipMemcpyAsync(sums_out, st->sums.p, F * 12 * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
  return LK_ERROR_NONE;
}

int lk_motion_from_sums(int kind, int min_sectors, int n, const double *sums11, const double *origin_xy, lk_motion *out) {
  if (!sums11 || !origin_xy || !out || n < 0 || !known_kind(kind) || min_sectors < lk_motion_min_sectors(kind))
    return LK_ERROR_BAD_DOMAIN;
  (void)lk_motion_fit_impl(kind, min_sectors, n, sums11, origin_xy[0], origin_xy[1], out);
  return LK_ERROR_NONE;
}

int lk_motion_apply(const lk_motion *m, int n, const float *xy, float *uv_out) {
  if (!m || !xy || !uv_out || n < 1)
    return LK_ERROR_BAD_DOMAIN;
  const bool ok = m->status == LK_MOTION_OK;
  const double gxx = (double)m->axx - 1.0, gxy = (double)m->axy, gyx = (double)m->ayx, gyy = (double)m->ayy - 1.0;
  for (int i = 0; i < n; ++i) {
    const double dx = (double)xy[2 * i] - (double)m->cx, dy = (double)xy[2 * i + 1] - (double)m->cy;
    uv_out[2 * i] = ok ? (float)((double)m->tx + (gxx * dx + gxy * dy)) : 0.f;
    uv_out[2 * i + 1] = ok ? (float)((double)m->ty + (gyx * dx + gyy * dy)) : 0.f;
  }
  return LK_ERROR_NONE;
}

int lk_motion_remove(int model, const lk_motion *m, float cx, float cy, const lk_result *in, lk_result *out) {
  if (!m || !in || !out || model < LK_FM_U || model > LK_FM_UVUXUYVXVY)
    return LK_ERROR_BAD_DOMAIN;
  if (m->status != LK_MOTION_OK) {
    *out = *in;
    return LK_ERROR_NONE;
  }
  if (model == LK_FM_U && !(m->axx == 1.f && m->axy == 0.f && m->ayx == 0.f && m->ayy == 1.f))
    return LK_ERROR_BAD_DOMAIN;
  lk_result r;
  if (lk_motion_remove_impl(model, *m, cx, cy, *in, &r))
    return LK_ERROR_BAD_DOMAIN;
  *out = r;
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_motion_last(lk_engine *e, float *device_ms, int *chunk, int *chunks) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  MotionState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_MOTION, "lk_internal_motion_last: no lk_rigid_motion yet", device_ms, &st))
    return rc;
  if (chunk)
    *chunk = st->chunk;
  if (chunks)
    *chunks = st->chunks;
  return LK_ERROR_NONE;
}

} // extern "C"
