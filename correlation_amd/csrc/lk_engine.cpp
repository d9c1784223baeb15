// lk_engine.cpp - the engine behind include/lk_engine.h: create and destroy, the setters, synchronise, the counters, and the
// lk_internal_* views and hooks of lk_internal.hpp.  The state is lk_engine_state.hpp; images, sectors, moves, solves and
// sequence windows are the lk_engine_*.cpp units beside this one.  (The entry points get their C linkage from their
// declarations in the public header.)
#include "lk_engine_state.hpp"

namespace {

int n_params_of(int model) {
  switch (model) {
  case LK_FM_U: return 1;
  case LK_FM_UV: return 2;
  case LK_FM_UVQ: return 3;
  case LK_FM_UVUXUYVXVY: return 6;
  default: return -1;
  }
}

} // namespace

int lk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

int lk_create(const lk_config *cfg, lk_engine **out) {
  if (!cfg || !out)
    return LK_ERROR_BAD_DOMAIN;
  *out = nullptr;
  if (n_params_of(cfg->fitting_model) < 0 || cfg->interpolation < 0 || cfg->interpolation > LK_IM_BICUBIC_SEPARABLE)
    return LK_ERROR_BAD_DOMAIN;
  if (cfg->py_step < 1 || cfg->py_start < 0 || cfg->py_stop < cfg->py_start ||
      cfg->py_stop >= LK_MAX_LEVELS || (cfg->py_stop - cfg->py_start) % cfg->py_step != 0)
    return LK_ERROR_BAD_DOMAIN;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return LK_ERROR_DEVICE; // no silent CPU fallback: the HIP device is the product
  if (cfg->device < 0 || cfg->device >= ndev)
    return LK_ERROR_DEVICE;
  lk_engine *e = new lk_engine();
  e->cfg = *cfg;
  e->P = n_params_of(cfg->fitting_model);
  bool ok = hipSetDevice(cfg->device) == hipSuccess &&
            hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&e->nxt_stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&e->nxt_done, hipEventDisableTiming) == hipSuccess &&
            hipEventCreate(&e->ev_s0) == hipSuccess && hipEventCreate(&e->ev_s1) == hipSuccess &&
            hipEventCreate(&e->ev_p0) == hipSuccess && hipEventCreate(&e->ev_p1) == hipSuccess;
  if (!ok) {
    delete e;
    return LK_ERROR_DEVICE;
  }
  e->stream = e->own_stream;
  *out = e;
  return LK_ERROR_NONE;
}

void lk_destroy(lk_engine *e) {
  if (!e)
    return;
  (void)hipSetDevice(e->cfg.device);
  (void)hipDeviceSynchronize();
  for (LkPassSlot *&p : e->pass) {
    delete p;
    p = nullptr;
  }
  for (auto &im : e->img)
    for (auto &p : im.lvl)
      if (p)
        (void)hipFree(p);
  e->d_lv.release();
  for (int l = 0; l < LK_MAX_LEVELS; ++l) {
    e->d_xy[l].release();
    e->d_xy_eval[l].release();
    e->d_off[l].release();
    e->d_rect[l].release();
  }
  e->d_center.release();
  e->d_gs_match.release();
  e->d_xy0_alt.release();
  e->d_xy_eval0_alt.release();
  e->d_off_eval.release();
  e->d_off0_alt.release();
  e->d_pos.release();
  e->d_tiles.release();
  e->d_level_total.release();
  e->d_roi_sectors.release();
  e->d_roi_flats.release();
  e->d_roi_tile_begin.release();
  e->d_offsets.release();
  e->d_guess.release();
  e->d_last_p.release();
  e->d_last_eval_p.release();
  e->d_prev_p.release();
  e->d_result.release();
  e->d_stats.release();
  e->d_order.release();
  e->d_single.release();
  e->d_queue.release();
  e->d_handoff.release();
  e->d_mid.release();
  e->d_finish_list.release();
  e->d_finish_count.release();
  e->d_ill_list.release();
  e->d_ill_count.release();
  e->d_mean_scratch.release();
  e->d_scratch.release();
  e->d_stale.release();
  e->d_warp.release();
  e->d_team_partials.release();
  e->d_team_arrivals.release();
  for (auto &im : e->ring)
    for (auto &p : im.lvl)
      if (p)
        (void)hipFree(p);
  for (hipEvent_t ev : e->ring_ready)
    if (ev)
      (void)hipEventDestroy(ev);
  for (hipEvent_t ev : e->seq_done)
    if (ev)
      (void)hipEventDestroy(ev);
  if (e->ev_seq)
    (void)hipEventDestroy(e->ev_seq);
  e->d_seq_result.release();
  e->d_seq_stats.release();
  e->d_seq_guess.release();
  e->d_seq_chain.release();
  e->d_seq_chain_safe.release();
  e->d_seq_img.release();
  e->d_seq_flags.release();
  e->d_prev_p_alt.release();
  if (e->h_seq_flags)
    (void)hipHostFree(e->h_seq_flags);
  for (lk_result *hp : e->h_seq_results)
    if (hp)
      (void)hipHostFree(hp);
  for (hipStream_t cs : e->class_stream)
    if (cs)
      (void)hipStreamDestroy(cs);
  for (hipEvent_t ev : e->ev_join)
    if (ev)
      (void)hipEventDestroy(ev);
  if (e->ev_fork)
    (void)hipEventDestroy(e->ev_fork);
  if (e->ev_results)
    (void)hipEventDestroy(e->ev_results);
  if (e->h_results)
    (void)hipHostFree(e->h_results);
  if (e->own_stream)
    (void)hipStreamDestroy(e->own_stream);
  if (e->nxt_stream)
    (void)hipStreamDestroy(e->nxt_stream);
  for (hipEvent_t ev : {e->nxt_done, e->ev_s0, e->ev_s1, e->ev_p0, e->ev_p1})
    if (ev)
      (void)hipEventDestroy(ev);
  delete e;
}

const char *lk_last_error_string(const lk_engine *e) { return e ? e->err.c_str() : "null engine"; }

int lk_set_stream(lk_engine *e, void *hip_stream) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->stream = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
  return LK_ERROR_NONE;
}

int lk_set_timing(lk_engine *e, int enabled) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  e->timing = enabled != 0;
  return LK_ERROR_NONE;
}

int lk_set_batch_invariant(lk_engine *e, int enabled) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  e->batch_invariant = enabled != 0;
  e->lv_dirty = true; // (which copy of the lists the lane groups walk)
  return LK_ERROR_NONE;
}

int lk_set_reference_order(lk_engine *e, int threads) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (threads < 0 || threads > 4096)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_reference_order: threads must be in 0..4096");
  if (threads > 0 && e->update == LK_UPDATE_BACKWARD)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_reference_order: the backward update has no reference arithmetic to follow");
  if ((threads > 0) != (e->reference_order > 0) && e->committed)
    e->recommit_pending = true; // the lane groups depend on the mode (commit_impl)
  e->reference_order = threads;
  return LK_ERROR_NONE;
}

int lk_set_update(lk_engine *e, int mode) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (mode != LK_UPDATE_FORWARD && mode != LK_UPDATE_BACKWARD)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_update: mode must be LK_UPDATE_FORWARD or LK_UPDATE_BACKWARD");
  if (mode == LK_UPDATE_BACKWARD && e->reference_order > 0)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_update: the backward update has no reference arithmetic (reference-order mode is on)");
  e->update = mode;
  return LK_ERROR_NONE;
}

int lk_compose_inverse(int model, const float *p, const float *delta, float *p_out) {
  if (model < LK_FM_U || model > LK_FM_UVUXUYVXVY || !p || !delta || !p_out)
    return LK_ERROR_BAD_DOMAIN;
  return lk_compose_inverse_impl(model, p, delta, p_out);
}

int lk_strain_from_gradient(int tensor, const float *grad4, float *out6) {
  if (!grad4 || !out6 || lk_strain_tensor_impl(tensor, grad4, out6) != 0)
    return LK_ERROR_BAD_DOMAIN;
  return LK_ERROR_NONE;
}

int lk_set_pairs_in_flight(lk_engine *e, int n) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (n < 1 || n > 64)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_pairs_in_flight: n must be in 1..64");
  e->pairs_in_flight = n;
  return LK_ERROR_NONE;
}

int lk_synchronize(lk_engine *e) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->nxt_stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return LK_ERROR_NONE;
}

int lk_internal_set_defer_stale(lk_engine *e, int on) { // (lk_internal.hpp)
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  e->defer_stale = on != 0;
  return LK_ERROR_NONE;
}
int lk_internal_reference_order(const lk_engine *e) { return e ? e->reference_order : 0; }
// does a solve of this engine launch teams (workgroups that wait for each other and must all be resident)?  A collective
// kernel on another stream could hold the slots one of them needs: the group then keeps its collectives in stream order.
int lk_internal_team_launches(const lk_engine *e) {
  if (!e || !e->committed)
    return 0;
  const int n_team = e->class_begin[kTeamClass + 1] - e->class_begin[kTeamClass];
  const int n_big = e->class_begin[kTeamClass + 1] - e->class_begin[kTeamClass - 1];
  return (n_team > 0 && e->team_w > 1) || (e->reference_order > 1 && n_big > 0) ? 1 : 0;
}
int lk_internal_sector_count(const lk_engine *e) { return e ? e->S : 0; }

int lk_internal_fail(lk_engine *e, int code, const char *what) { return e->fail(code, what); }
int lk_internal_hipfail(lk_engine *e, hipError_t err, const char *where) { return e->hipfail(err, where); }
int *lk_internal_guess_search_count(lk_engine *e) { return &e->gs_count; }

int lk_internal_engine_stream(lk_engine *e, hipStream_t *stream) {
  HIPCHK(hipSetDevice(e->cfg.device));
  *stream = e->stream;
  return LK_ERROR_NONE;
}

int lk_internal_guess_search_matches(lk_engine *e, lk_guess_match **d_match, hipStream_t *stream) {
  if (!e->d_gs_match.p)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_guess_search_info: no search yet");
  HIPCHK(hipSetDevice(e->cfg.device));
  *d_match = e->d_gs_match.p;
  *stream = e->stream;
  return LK_ERROR_NONE;
}

// The images of a pass that reads level `level`: the undeformed one and LK_IMG_DEF (def_slot < 0) or a ring slot, whose
// pyramid the engine's stream then waits for.
static int level_images(lk_engine *e, const char *who, int level, int def_slot, const DevImage **und, const DevImage **def) {
  const std::string w(who);
  const DevImage &u = e->img[LK_IMG_UND];
  const DevImage *d = &e->img[LK_IMG_DEF];
  if (def_slot >= 0) {
    if (def_slot >= (int)e->ring.size())
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": unknown ring slot (lk_sequence_reserve)");
    d = &e->ring[(size_t)def_slot];
    if (d->valid)
      HIPCHK(hipStreamWaitEvent(e->stream, e->ring_ready[(size_t)def_slot], 0));
  }
  if (!u.valid || !d->valid || !u.lvl[level] || !d->lvl[level])
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": the undeformed and the deformed image must be set");
  *und = &u;
  *def = d;
  return LK_ERROR_NONE;
}

int lk_internal_guess_search_view(lk_engine *e, int level, int def_slot, LkGuessSearchView *v, const char *who) {
  const std::string w(who);
  if (level < 0)
    level = e->cfg.py_stop;
  if (!e->committed)
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": sectors are not committed (call lk_commit_sectors)");
  if (level < 0 || level > e->cfg.py_stop || level >= LK_MAX_LEVELS || e->h_off[level].size() != (size_t)e->S + 1 ||
      e->h_rect[level].size() != (size_t)e->S)
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": the engine builds no sample lists for that level");
  HIPCHK(hipSetDevice(e->cfg.device));
  if (int rc = recommit_if_pending(e)) // (as the next solve would)
    return rc;
  const DevImage *u = nullptr, *d = nullptr;
  if (int rc = level_images(e, who, level, def_slot, &u, &d)) // (any negative def_slot: LK_IMG_DEF)
    return rc;
  HIPCHK(e->d_gs_match.ensure((size_t)std::max(e->S, 1)));
  v->stream = e->stream;
  v->S = e->S;
  v->model = e->cfg.fitting_model;
  v->level = level;
  v->und = u->lvl[level];
  v->def = d->lvl[level];
  v->urows = u->rows >> level;
  v->ucols = u->cols >> level;
  v->drows = d->rows >> level;
  v->dcols = d->cols >> level;
  v->xy = e->d_xy[level].p;
  v->off = e->d_off[level].p;
  v->rect = e->d_rect[level].p;
  v->h_rect = e->h_rect[level].data();
  v->h_off = e->h_off[level].data();
  v->d_guess = e->d_guess.p;
  v->d_prev_p = e->d_prev_p.p;
  v->d_match = e->d_gs_match.p;
  v->center = e->d_center.p;
  return LK_ERROR_NONE;
}

int lk_internal_reseed_view(lk_engine *e, int need_solve, const char *who, LkReseedView *v) {
  const std::string w(who);
  if (!e->committed || e->S <= 0)
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": no committed sectors (call lk_commit_sectors)");
  if (e->reference_order > 0)
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": reference-order mode is on - its records are the CPU engine's, which has no such pass");
  if (e->results_pending)
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": the outstanding solve has not been waited for (lk_wait_results)");
  if (e->seq.outstanding)
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": a sequence window is outstanding (lk_wait_sequence)");
  HIPCHK(hipSetDevice(e->cfg.device));
  if (need_solve) {
    if (e->records_S != e->S)
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": no solve of the committed sectors yet (lk_correlate_all*)");
    if (int rc = refresh_level_views(e))
      return rc;
  } else if (int rc = recommit_if_pending(e)) { // (the lists and the centres, as the next solve would)
    return rc;
  }
  if (int rc = reclassify_if_dirty(e))
    return rc;
  v->stream = e->stream;
  v->S = e->S;
  v->model = e->cfg.fitting_model;
  v->backward = e->update == LK_UPDATE_BACKWARD ? 1 : 0;
  v->center = e->d_center.p;
  v->result = e->d_result.p;
  v->last_p = e->d_last_p.p;
  v->last_eval_p = e->d_last_eval_p.p;
  v->stats = e->d_stats.p;
  v->order = e->d_order.p;
  for (int c = 0; c <= kNumClasses; ++c)
    v->class_begin[c] = e->class_begin[c];
  v->bw_order = nullptr;
  for (int g = 0; g < 4; ++g)
    v->bw_begin[g] = 0;
  if (v->backward && need_solve) {
    if (int rc = bw_tables(e))
      return rc;
    v->bw_order = e->d_bw_order.p;
    for (int g = 0; g < 4; ++g)
      v->bw_begin[g] = e->bw_begin[g];
  }
  return LK_ERROR_NONE;
}

int lk_internal_solve_set(lk_engine *e, const LkSectorSet *set, const float *d_guess, lk_result *d_result) {
  if (int rc = refresh_level_views(e))
    return rc;
  return launch_all(e, d_guess, d_result, set);
}

int lk_internal_reseed_stats(lk_engine *e, const unsigned long long totals[5]) {
  lk_stats s{};
  s.sectors = totals[0];
  s.evaluations = totals[1];
  s.sample_evaluations = totals[2];
  s.point_iterations = totals[3];
  s.ill_conditioned_solves = totals[4];
  s.algorithmic_bytes = (e->update == LK_UPDATE_BACKWARD ? 40ull : 25ull) * s.sample_evaluations + 196ull * s.evaluations;
  s.solve_ms = e->stats.solve_ms;
  s.pyramid_ms = e->stats.pyramid_ms;
  e->stats = s;
  e->stats_valid = true;
  e->stats_frames = 1;
  return LK_ERROR_NONE;
}

LkPassSlot **lk_internal_pass_slot(lk_engine *e, int which) { return &e->pass[which]; }

int lk_internal_pass_view(lk_engine *e, const char *who, unsigned need, int def_slot, LkPassView *v) {
  const std::string w(who);
  if (!e->committed || e->S <= 0)
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": no committed sectors (call lk_commit_sectors)");
  if (need & LK_VIEW_RECORDS) {
    if (e->results_pending)
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": the outstanding solve has not been waited for (lk_wait_results)");
    if (e->seq.outstanding)
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": a sequence window is outstanding (lk_wait_sequence)");
    if (e->records_S != e->S)
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": no solve of the committed sectors yet (lk_correlate_all*); pass records");
  }
  if (need & LK_VIEW_WINDOW) {
    if (e->seq.outstanding)
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": the sequence window is outstanding (lk_wait_sequence)");
    if (!e->d_seq_result.p || e->seq.n_frames < 1 || e->window_S != e->S || e->d_seq_result.n < (size_t)e->seq.n_frames * (size_t)e->S)
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": no window of the committed sectors was solved (lk_correlate_sequence_async)");
  }
  HIPCHK(hipSetDevice(e->cfg.device));
  *v = LkPassView{};
  if (need & LK_VIEW_IMAGES) {
    if (int rc = recommit_if_pending(e)) // (as the next solve would: the pass walks the lists)
      return rc;
    if (def_slot < -1)
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": def_slot must be -1 (LK_IMG_DEF) or a ring slot");
    const int level = e->cfg.py_start; // a level the commit builds lists for (commit_impl: level 0 and py_start, ...)
    const DevImage *u = nullptr, *d = nullptr;
    if (int rc = level_images(e, who, level, def_slot, &u, &d))
      return rc;
    v->level = level;
    v->und = u->lvl[level];
    v->def = d->lvl[level];
    v->urows = u->rows >> level;
    v->ucols = u->cols >> level;
    v->drows = d->rows >> level;
    v->dcols = d->cols >> level;
    v->xy = e->d_xy[level].p;
    v->off = e->d_off[level].p;
    v->rect = e->d_rect[level].p;
  }
  v->stream = e->stream;
  v->S = e->S;
  v->model = e->cfg.fitting_model;
  v->interp = e->cfg.interpolation;
  v->h_rect0 = e->h_rect[0].data();
  v->h_off0 = e->h_off[0].data();
  v->center = e->d_center.p;
  v->result = e->d_result.p;
  if (need & LK_VIEW_WINDOW) {
    v->window = e->d_seq_result.p;
    v->window_frames = e->seq.n_frames;
  }
  return LK_ERROR_NONE;
}

int lk_internal_image_view(lk_engine *e, const char *who, int slot, int need_sectors, LkPassView *v) {
  const std::string w(who);
  if (slot != LK_IMG_UND && slot != LK_IMG_DEF && slot != LK_IMG_NXT)
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": unknown slot (LK_IMG_UND, LK_IMG_DEF or LK_IMG_NXT)");
  if (need_sectors && (!e->committed || e->S <= 0))
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": no committed sectors (call lk_commit_sectors)");
  HIPCHK(hipSetDevice(e->cfg.device));
  *v = LkPassView{};
  const int level = e->cfg.py_start;
  if (need_sectors)
    if (int rc = recommit_if_pending(e)) // (as the next solve would)
      return rc;
  {
    std::unique_lock<std::mutex> lock(e->nxt_mu, std::defer_lock);
    if (slot == LK_IMG_NXT)
      lock.lock();
    const DevImage &im = e->img[slot];
    if (!im.valid || !im.lvl[level])
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": the image of that slot is not set (lk_set_image)");
    if (slot == LK_IMG_NXT && e->nxt_pending) // filled on its own stream: the engine's stream must see the finished pyramid
      HIPCHK(hipStreamWaitEvent(e->stream, e->nxt_done, 0));
    v->und = v->def = im.lvl[level];
    v->urows = v->drows = im.rows >> level;
    v->ucols = v->dcols = im.cols >> level;
  }
  v->level = level;
  v->stream = e->stream;
  v->model = e->cfg.fitting_model;
  v->interp = e->cfg.interpolation;
  if (need_sectors) {
    v->S = e->S;
    v->xy = e->d_xy[level].p;
    v->off = e->d_off[level].p;
    v->rect = e->d_rect[level].p;
    v->h_rect0 = e->h_rect[0].data();
    v->h_off0 = e->h_off[0].data();
    v->center = e->d_center.p;
  }
  return LK_ERROR_NONE;
}

int lk_internal_frames_view(lk_engine *e, const char *who, int ring, int n_frames, const int *slots, int first, int need_sectors,
                            LkFramesView *v) {
  const std::string w(who);
  if (n_frames < 2 || n_frames > (ring ? LK_NOISE_MAX_FRAMES : 3))
    return e->fail(LK_ERROR_BAD_DOMAIN, w + (ring ? ": n_frames must be 2 .. LK_NOISE_MAX_FRAMES ring slots" : ": n_frames must be 2 or 3 image slots"));
  if (!ring) {
    for (int i = 0; i < n_frames; ++i) {
      if (slots[i] != LK_IMG_UND && slots[i] != LK_IMG_DEF && slots[i] != LK_IMG_NXT)
        return e->fail(LK_ERROR_BAD_DOMAIN, w + ": unknown slot (LK_IMG_UND, LK_IMG_DEF or LK_IMG_NXT)");
      for (int j = 0; j < i; ++j)
        if (slots[j] == slots[i])
          return e->fail(LK_ERROR_BAD_DOMAIN, w + ": an image slot is listed twice");
    }
  }
  if (need_sectors && (!e->committed || e->S <= 0))
    return e->fail(LK_ERROR_BAD_DOMAIN, w + ": no committed sectors (call lk_commit_sectors)");
  HIPCHK(hipSetDevice(e->cfg.device));
  *v = LkFramesView{};
  const int level = e->cfg.py_start;
  if (need_sectors)
    if (int rc = recommit_if_pending(e)) // (as the next solve would)
      return rc;
  {
    // (the next-frame slot and the ring are filled on their own stream, under this lock)
    std::lock_guard<std::mutex> lock(e->nxt_mu);
    if (ring && (first < 0 || first > (int)e->ring.size() - n_frames))
      return e->fail(LK_ERROR_BAD_DOMAIN, w + ": unknown ring slot (lk_sequence_reserve)");
    for (int i = 0; i < n_frames; ++i) {
      const DevImage &im = ring ? e->ring[(size_t)(first + i)] : e->img[slots[i]];
      if (!im.valid || !im.lvl[level])
        return e->fail(LK_ERROR_BAD_DOMAIN, w + (ring ? ": a ring slot is empty (lk_sequence_set_frame)" : ": the image of a slot is not set (lk_set_image)"));
      if (i > 0 && ((im.rows >> level) != v->rows || (im.cols >> level) != v->cols))
        return e->fail(LK_ERROR_BAD_DOMAIN, w + ": the frames must have the same dimensions");
      // the engine's stream must see the finished pyramid
      if (ring)
        HIPCHK(hipStreamWaitEvent(e->stream, e->ring_ready[(size_t)(first + i)], 0));
      else if (slots[i] == LK_IMG_NXT && e->nxt_pending)
        HIPCHK(hipStreamWaitEvent(e->stream, e->nxt_done, 0));
      v->frame[i] = im.lvl[level];
      v->rows = im.rows >> level;
      v->cols = im.cols >> level;
    }
  }
  v->level = level;
  v->n_frames = n_frames;
  v->stream = e->stream;
  if (need_sectors) {
    v->S = e->S;
    v->xy = e->d_xy[level].p;
    v->off = e->d_off[level].p;
    v->rect = e->d_rect[level].p;
    v->h_rect0 = e->h_rect[0].data();
    v->h_off0 = e->h_off[0].data();
    v->center = e->d_center.p;
  }
  return LK_ERROR_NONE;
}

int lk_get_stats(lk_engine *e, lk_stats *out) {
  if (!e || !out)
    return LK_ERROR_BAD_DOMAIN;
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (!e->stats_valid && e->committed) {
    // (after a frame-pipelined window: the counters of all its frames)
    const size_t rows = (size_t)e->S * (size_t)(e->stats_frames > 1 ? e->stats_frames : 1);
    std::vector<uint32_t> h(4 * rows);
    HIPCHK(hipMemcpy(h.data(), e->stats_frames > 1 ? e->d_seq_stats.p : e->d_stats.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    lk_stats s{};
    s.sectors = (uint64_t)rows;
    for (size_t i = 0; i < rows; ++i) {
      s.evaluations += h[4 * i];
      s.sample_evaluations += h[4 * i + 1];
      s.point_iterations += h[4 * i + 2];
      s.ill_conditioned_solves += h[4 * i + 3];
    }
    // 25 B per sample-evaluation + 196 B per evaluation; the backward update reads a 16-byte
    // template slot instead of the undeformed pixel: 40 B per sample-evaluation (include/lk_engine.h, lk_set_update)
    s.algorithmic_bytes = (e->stats_update == LK_UPDATE_BACKWARD ? 40ull : 25ull) * s.sample_evaluations + 196ull * s.evaluations;
    s.solve_ms = e->stats.solve_ms;
    s.pyramid_ms = e->stats.pyramid_ms;
    e->stats = s;
    e->stats_valid = true;
  }
  if (e->solve_timed) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->ev_s0, e->ev_s1) == hipSuccess)
      e->stats.solve_ms = ms;
  }
  if (e->pyr_timed) {
    float ms = 0.f;
    if (hipEventSynchronize(e->ev_p1) == hipSuccess && hipEventElapsedTime(&ms, e->ev_p0, e->ev_p1) == hipSuccess)
      e->stats.pyramid_ms = ms;
  }
  e->stats.window_safe_reruns = e->window_safe_reruns;
  *out = e->stats;
  return LK_ERROR_NONE;
}

int lk_get_sector_stats(lk_engine *e, uint32_t *out) {
  if (!e || !out)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_sector_stats: no committed sectors");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, e->d_stats.p, 4 * (size_t)e->S * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return LK_ERROR_NONE;
}
