// lk_rotated_search.cpp - host side of the rotation-aware automatic initial guess (include/lk_engine.h: lk_search_rotated,
// lk_get_rotated_search_info, lk_get_rotated_search_profile, lk_rotation_table).  The kernels are lk_rotated_search.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"

namespace {

// what the pass keeps on its slot of the engine: the table, the per-angle records, and the results of the last call
struct LkRotatedState : LkPassSlot {
  LkDevBytes table, angle, profile, match;
  std::vector<float> h_table;
  int S = 0, n_angles = 0; // what `match` and `profile` hold (0: no search yet)
  hipError_t init() { return hipSuccess; }
};

bool angles_ok(const lk_rotated_search *cfg) {
  if (!cfg || cfg->n_half < 0 || 2 * (long long)cfg->n_half + 1 > LK_RS_MAX_ANGLES || !std::isfinite(cfg->angle_center))
    return false;
  return cfg->n_half == 0 || (std::isfinite(cfg->angle_step) && cfg->angle_step > 0.f);
}

// the results of the last search, once it covers the committed sectors
int last_search(lk_engine *e, const char *who, LkRotatedState **st) {
  *st = static_cast<LkRotatedState *>(*lk_internal_pass_slot(e, LK_PASS_ROTATED));
  if (!*st || (*st)->S <= 0 || (*st)->S != lk_internal_sector_count(e))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string(who) + ": no rotated search of the committed sectors").c_str());
  return LK_ERROR_NONE;
}

} // namespace

extern "C" {

int lk_rotation_table(const lk_rotated_search *cfg, float *cos_sin_out) {
  if (!angles_ok(cfg) || !cos_sin_out)
    return LK_ERROR_BAD_DOMAIN;
  const int K = cfg->n_half;
  const double step = K > 0 ? (double)cfg->angle_step : 0.0;
  for (int k = -K; k <= K; ++k) {
    const double theta = (double)cfg->angle_center + (double)k * step;
    cos_sin_out[2 * (k + K)] = (float)std::cos(theta);
    cos_sin_out[2 * (k + K) + 1] = (float)std::sin(theta);
  }
  return LK_ERROR_NONE;
}

int lk_search_rotated(lk_engine *e, const lk_rotated_search *cfg, float *guesses_inout) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_rotated: no configuration");
  const lk_guess_search &gs = cfg->search;
  if (gs.radius < 0 || gs.radius > LK_GS_MAX_RADIUS)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_rotated: radius must be in 0 .. LK_GS_MAX_RADIUS");
  if (gs.level < -1 || gs.def_slot < -1 || !(gs.min_score == gs.min_score))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_rotated: bad level, ring slot or min_score");
  if (!angles_ok(cfg))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_search_rotated: n_half must be in 0 .. (LK_RS_MAX_ANGLES - 1) / 2, angle_step > 0, both angles finite");
  LkGuessSearchView v{};
  if (int rc = lk_internal_guess_search_view(e, gs.level, gs.def_slot, &v, "lk_search_rotated")) // (level -1: py_stop)
    return rc;
  if (v.model != LK_FM_UVQ && v.model != LK_FM_UVUXUYVXVY)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_rotated: LK_FM_U and LK_FM_UV have no parameter that carries an angle");
  LkRotatedState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_ROTATED, "lk_search_rotated: state", &st))
    return rc;
  const int K = cfg->n_half, nA = 2 * K + 1, R = gs.radius;
  st->S = 0;
  st->h_table.resize(2 * (size_t)nA);
  if (lk_rotation_table(cfg, st->h_table.data()) != LK_ERROR_NONE)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_rotated: bad angles");
  const size_t cells = (size_t)std::max(v.S, 1) * (size_t)nA;
  LK_HIPCHK(st->table.ensure(2 * sizeof(float) * (size_t)nA));
  LK_HIPCHK(st->angle.ensure(sizeof(LkRotAngleRecord) * cells));
  LK_HIPCHK(st->profile.ensure(sizeof(double) * cells));
  LK_HIPCHK(st->match.ensure(sizeof(lk_rotated_match) * (size_t)std::max(v.S, 1)));

  LkRotatedSearchArgs a{};
  a.gs.und = v.und;
  a.gs.def = v.def;
  a.gs.urows = v.urows;
  a.gs.ucols = v.ucols;
  a.gs.drows = v.drows;
  a.gs.dcols = v.dcols;
  a.gs.xy = v.xy;
  a.gs.off = v.off;
  a.gs.rect = v.rect;
  a.gs.guess = v.d_guess;
  a.gs.prev_p = v.d_prev_p;
  a.gs.match = nullptr;
  a.gs.n_sectors = v.S;
  a.gs.level = v.level;
  a.gs.radius = R;
  a.gs.has_v = 1;
  a.gs.min_samples = gs.min_samples > 0 ? gs.min_samples : 9;
  a.gs.min_score = gs.min_score;
  a.center = v.center;
  a.cos_sin = st->table.as<float2>();
  a.angle = st->angle.as<LkRotAngleRecord>();
  a.profile = st->profile.as<double>();
  a.match = st->match.as<lk_rotated_match>();
  a.n_angles = nA;
  a.model = v.model;
  a.angle_center = (double)cfg->angle_center;
  a.angle_step = K > 0 ? (double)cfg->angle_step : 0.0;
  // LDS for the deformed window: what the largest implicit rectangle needs at its widest angle (the rotated bounding box
  // plus the rounding's pixel on either side), or the whole budget when there are lists.  Only a bound for the launch:
  // the kernel decides per workgroup, from the window it meets, whether the window is staged.
  const int budget = lk_guess_search_window_budget(R, 1);
  long long max_w = 0, max_h = 0, need = 0;
  for (int s = 0; s < v.S && need < budget; ++s) {
    const int4 r = v.h_rect[s];
    if (r.z > 0) {
      max_w = std::max<long long>(max_w, r.z);
      max_h = std::max<long long>(max_h, r.w / r.z);
    } else if (v.h_off[s + 1] > v.h_off[s]) {
      need = budget;
    }
  }
  if (max_w > 0)
    for (int q = 0; q < nA && need < budget; ++q) {
      const double c = std::fabs((double)st->h_table[2 * (size_t)q]), s_ = std::fabs((double)st->h_table[2 * (size_t)q + 1]);
      const long long bw = (long long)(c * (double)(max_w - 1) + s_ * (double)(max_h - 1)) + 3;
      const long long bh = (long long)(s_ * (double)(max_w - 1) + c * (double)(max_h - 1)) + 3;
      need = std::max(need, (bw + 2 * R) * (bh + 2 * R));
    }
  a.gs.win_bytes = (int)std::min<long long>(budget, (need + 3) / 4 * 4);

  if (guesses_inout)
    LK_HIPCHK(hipMemcpyAsync(v.d_guess, guesses_inout, 6 * sizeof(float) * (size_t)v.S, hipMemcpyHostToDevice, v.stream));
  // (pageable source: the copy has left h_table when the call returns)
  LK_HIPCHK(hipMemcpyAsync(st->table.p, st->h_table.data(), 2 * sizeof(float) * (size_t)nA, hipMemcpyHostToDevice, v.stream));
  LK_HIPCHK(lk_launch_rotated_search(a, v.stream));
  LK_HIPCHK(lk_launch_rotated_reduce(a, v.stream));
  st->S = v.S;
  st->n_angles = nA;
  if (guesses_inout) {
    LK_HIPCHK(hipMemcpyAsync(guesses_inout, v.d_guess, 6 * sizeof(float) * (size_t)v.S, hipMemcpyDeviceToHost, v.stream));
    LK_HIPCHK(hipStreamSynchronize(v.stream));
  }
  return LK_ERROR_NONE;
}

int lk_get_rotated_search_info(lk_engine *e, lk_rotated_match *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  LkRotatedState *st = nullptr;
  if (int rc = last_search(e, "lk_get_rotated_search_info", &st))
    return rc;
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_get_rotated_search_info: no output");
  hipStream_t stream = nullptr;
  if (int rc = lk_internal_engine_stream(e, &stream))
    return rc;
  LK_HIPCHK(hipMemcpyAsync(out, st->match.p, sizeof(lk_rotated_match) * (size_t)st->S, hipMemcpyDeviceToHost, stream));
  LK_HIPCHK(hipStreamSynchronize(stream));
  return LK_ERROR_NONE;
}

int lk_get_rotated_search_profile(lk_engine *e, double *best_per_angle) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  LkRotatedState *st = nullptr;
  if (int rc = last_search(e, "lk_get_rotated_search_profile", &st))
    return rc;
  if (!best_per_angle)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_get_rotated_search_profile: no output");
  hipStream_t stream = nullptr;
  if (int rc = lk_internal_engine_stream(e, &stream))
    return rc;
  LK_HIPCHK(hipMemcpyAsync(best_per_angle, st->profile.p, sizeof(double) * (size_t)st->S * (size_t)st->n_angles,
                           hipMemcpyDeviceToHost, stream));
  LK_HIPCHK(hipStreamSynchronize(stream));
  return LK_ERROR_NONE;
}

} // extern "C"
