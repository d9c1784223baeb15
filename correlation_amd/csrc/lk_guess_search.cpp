// lk_guess_search.cpp - host side of the automatic initial guess (include/lk_engine.h: lk_search_guesses) and the
// tracker's switch for it (include/lk_tracker.h: lk_tracker_set_guess_search).  The kernel is lk_guess_search.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/lk_engine.h"
#include "../../include/lk_tracker.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"

// lk_tracker.cpp: the search the sequence functions run on frame 0 (nullptr: none)
extern "C" int lk_tracker_internal_set_search(lk_tracker *t, const lk_guess_search *cfg,
                                   int (*search)(lk_engine *, const lk_guess_search *, float *));

extern "C" {

int lk_search_guesses(lk_engine *e, const lk_guess_search *cfg, float *guesses_inout) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_guesses: no configuration");
  if (cfg->radius < 0 || cfg->radius > LK_GS_MAX_RADIUS)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_guesses: radius must be in 0 .. LK_GS_MAX_RADIUS");
  if (cfg->level < -1 || cfg->def_slot < -1 || !(cfg->min_score == cfg->min_score))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_guesses: bad level, ring slot or min_score");
  LkGuessSearchView v{};
  if (int rc = lk_internal_guess_search_view(e, cfg->level, cfg->def_slot, &v)) // (level -1: py_stop)
    return rc;
  const int level = v.level;
  const int has_v = v.model != LK_FM_U;
  LkGuessSearchArgs a{};
  a.und = v.und;
  a.def = v.def;
  a.urows = v.urows;
  a.ucols = v.ucols;
  a.drows = v.drows;
  a.dcols = v.dcols;
  a.xy = v.xy;
  a.off = v.off;
  a.rect = v.rect;
  a.guess = v.d_guess;
  a.prev_p = v.d_prev_p;
  a.match = v.d_match;
  a.n_sectors = v.S;
  a.level = level;
  a.radius = cfg->radius;
  a.has_v = has_v;
  a.min_samples = cfg->min_samples > 0 ? cfg->min_samples : 9;
  a.min_score = cfg->min_score;
  // LDS for the deformed window: what the largest implicit rectangle needs, or the whole budget when there are lists
  const int budget = lk_guess_search_window_budget(cfg->radius, has_v);
  long long need = 0;
  for (int s = 0; s < v.S && need < budget; ++s) {
    const int4 r = v.h_rect[s];
    if (r.z > 0) {
      const long long w = r.z, h = r.w / r.z;
      need = std::max(need, (w + 2 * cfg->radius) * (h + (has_v ? 2 * cfg->radius : 0)));
    } else if (v.h_off[s + 1] > v.h_off[s]) {
      need = budget;
    }
  }
  a.win_bytes = (int)std::min<long long>(budget, (need + 3) / 4 * 4);
  if (guesses_inout)
    LK_HIPCHK(hipMemcpyAsync(v.d_guess, guesses_inout, 6 * sizeof(float) * (size_t)v.S, hipMemcpyHostToDevice, v.stream));
  LK_HIPCHK(lk_launch_guess_search(a, v.stream));
  *lk_internal_guess_search_count(e) = v.S;
  if (guesses_inout) {
    LK_HIPCHK(hipMemcpyAsync(guesses_inout, v.d_guess, 6 * sizeof(float) * (size_t)v.S, hipMemcpyDeviceToHost, v.stream));
    LK_HIPCHK(hipStreamSynchronize(v.stream));
  }
  return LK_ERROR_NONE;
}

int lk_get_guess_search_info(lk_engine *e, lk_guess_match *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  const int n = *lk_internal_guess_search_count(e);
  if (!out || n <= 0 || n != lk_internal_sector_count(e))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_get_guess_search_info: no search of the committed sectors");
  lk_guess_match *d_match = nullptr;
  hipStream_t st = nullptr;
  if (int rc = lk_internal_guess_search_matches(e, &d_match, &st))
    return rc;
  LK_HIPCHK(hipMemcpyAsync(out, d_match, sizeof(lk_guess_match) * (size_t)n, hipMemcpyDeviceToHost, st));
  LK_HIPCHK(hipStreamSynchronize(st));
  return LK_ERROR_NONE;
}

int lk_tracker_set_guess_search(lk_tracker *t, const lk_guess_search *cfg) {
  if (!t)
    return LK_ERROR_BAD_DOMAIN;
  if (cfg && (cfg->radius < 0 || cfg->radius > LK_GS_MAX_RADIUS || cfg->level < -1))
    return LK_ERROR_BAD_DOMAIN;
  const bool on = cfg && cfg->radius > 0;
  return lk_tracker_internal_set_search(t, on ? cfg : nullptr, on ? &lk_search_guesses : nullptr);
}

} // extern "C"
