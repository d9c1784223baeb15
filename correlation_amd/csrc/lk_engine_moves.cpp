// lk_engine_moves.cpp - what moves the committed sectors of the engine (translate, rewarp, update, restore) and the
// sector and list getters.
#include "lk_engine_state.hpp"

// Lagrangian description, CPU-engine semantics (manager_class.cpp:381-419): every sample of
// the sector moves by add_pair(offset), i.e. (int)(offset + v + 0.5f) per coordinate
// (manager_class.cpp:38-47).  A rectangle whose columns and rows all move by one integer
// stays an implicit rectangle; otherwise the sector becomes an explicit list.
static void translate_one(HostSector &h, float ox, float oy, const float *center) {
  if (h.is_rect) {
    const int sx = (int)lkroi::add_pair_round(ox, (float)h.x0) - h.x0;
    const int sy = (int)lkroi::add_pair_round(oy, (float)h.y0) - h.y0;
    bool uniform = true;
    for (int x = h.x0; x <= h.x1 && uniform; ++x)
      uniform = (int)lkroi::add_pair_round(ox, (float)x) - x == sx;
    for (int y = h.y0; y <= h.y1 && uniform; ++y)
      uniform = (int)lkroi::add_pair_round(oy, (float)y) - y == sy;
    if (uniform) {
      h.x0 += sx, h.x1 += sx, h.y0 += sy, h.y1 += sy;
    } else {
      h.xy = h.points();
      h.is_rect = false;
    }
  }
  if (!h.is_rect) {
    const size_t n = h.xy.size() / 2;
    for (size_t i = 0; i < n; ++i) {
      h.xy[2 * i] = lkroi::add_pair_round(ox, h.xy[2 * i]);
      h.xy[2 * i + 1] = lkroi::add_pair_round(oy, h.xy[2 * i + 1]);
    }
  }
  if (center) {
    h.cx = center[0];
    h.cy = center[1];
  } else { // Newton_Raphson(p, n, xy): float mean of the samples (pyramid_class.cpp:325-340)
    const std::vector<float> pts = h.points();
    lkroi::mean_center(pts.data(), (int)(pts.size() / 2), h.cx, h.cy);
  }
}

static void rewarp_one(HostSector &h, int model, const float *p, const float *center) {
  if (h.is_rect) {
    h.xy = h.points();
    h.is_rect = false;
  }
  const size_t n = h.xy.size() / 2;
  const float cx = h.cx, cy = h.cy;
  for (size_t i = 0; i < n; ++i) {
    float xd, yd;
    lkroi::warp_point(model, h.xy[2 * i], h.xy[2 * i + 1], cx, cy, p, xd, yd);
    h.xy[2 * i] = xd;
    h.xy[2 * i + 1] = yd;
  }
  if (center) {
    h.cx = center[0];
    h.cy = center[1];
  } else {
    lkroi::mean_center(h.xy.data(), (int)n, h.cx, h.cy);
  }
}

static int rewarp_on_device(lk_engine *e, const float *centers_xy, const float *offsets_xy = nullptr);

// A grid of implicit rectangles that only moved (Lagrangian description): sizes, classes, launch
// order and the (empty) explicit lists are what they were; only the per-level rectangles, the
// centres and - through the parity of the new positions - the starved-level flags change.
static int recommit_rects(lk_engine *e) {
  const int S = e->S;
  const lk_config &cfg = e->cfg;
  HIPCHK(hipSetDevice(cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream)); // the previous uploads from these host tables are done
  const std::vector<int> levels = list_levels(cfg);
  for (int s = 0; s < S; ++s) {
    const HostSector &hs = e->hs[(size_t)s];
    e->h_center[2 * (size_t)s] = hs.cx;
    e->h_center[2 * (size_t)s + 1] = hs.cy;
    for (int l : levels)
      e->h_rect[l][(size_t)s] = hs.rect_at(l);
  }
  for (int l : levels)
    HIPCHK(hipMemcpyAsync(e->d_rect[l].p, e->h_rect[l].data(), (size_t)S * sizeof(int4), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_center.p, e->h_center.data(), 2 * (size_t)S * sizeof(float), hipMemcpyHostToDevice, e->stream));
  e->stats_valid = false;
  return refresh_starved(e);
}

int lk_translate_sectors(lk_engine *e, const float *offsets_xy, const float *centers_xy) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed || !offsets_xy)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_translate_sectors: sectors are not committed");
  {
    // Explicit lists (annular / blob / point sectors) move on the device like the strict
    // Lagrangian ones; implicit rectangles stay with the host records - a rectangle that moves
    // by whole pixels stays implicit, which is O(sectors) work and keeps its faster sampling.
    bool device_path = env_int("LK_HOST_REWARP", 0) == 0 && !e->recommit_pending; // test hook, read per call
    for (int s = 0; s < e->S && device_path; ++s)
      device_path = e->h_rect[0][(size_t)s].z == 0;
    if (device_path) {
      HIPCHK(hipSetDevice(e->cfg.device));
      return rewarp_on_device(e, centers_xy, offsets_xy);
    }
  }
  {
    int rc = materialize_host(e);
    if (rc)
      return rc;
  }
  e->hs_backup.resize(e->hs.size());
  e->backup_on_device = false;
  // sectors are independent: blocks of them on a few threads when there are tens of thousands
  const int S = e->S;
  const unsigned hw = std::thread::hardware_concurrency();
  const int workers = std::max(1, std::min({S / 8192, 8, (int)(hw ? hw : 1)}));
  std::vector<char> all_rect((size_t)workers, 1);
  auto work = [&](int w) {
    bool rects = true;
    for (int s = (int)((int64_t)S * w / workers), last = (int)((int64_t)S * (w + 1) / workers); s < last; ++s) {
      HostSector &h = e->hs[(size_t)s];
      e->hs_backup[(size_t)s] = h;
      rects = rects && h.is_rect;
      translate_one(h, offsets_xy[2 * (size_t)s], offsets_xy[2 * (size_t)s + 1],
                    centers_xy ? centers_xy + 2 * (size_t)s : nullptr);
      rects = rects && h.is_rect;
    }
    all_rect[(size_t)w] = rects;
  };
  std::vector<std::thread> th;
  for (int w = 1; w < workers; ++w)
    th.emplace_back(work, w);
  work(0);
  for (std::thread &t : th)
    t.join();
  bool rects_only = true;
  for (char r : all_rect)
    rects_only = rects_only && r;
  return rects_only ? recommit_rects(e) : commit_impl(e, true);
}

// Strict Lagrangian description (manager_class.cpp:369-380): the deformed positions of the
// last solve - CorrelationClass::getDefXY0, i.e. the samples warped with the parameters of
// the LAST level-0 evaluation about the solve's centre (correlation_class.cpp:884-896) -
// become the undeformed samples of the next frame.
//
// Device path (default): the lists never leave the GPU.  One kernel warps every level-0 sample
// (implicit rectangles become explicit lists), one order-preserving compaction per coarser level
// applies the decimation rule to all sectors at once, a one-lane-per-sector kernel recomputes the
// mean centres where the caller gives none; the host reads back only the per-level offsets
// (starved-level bookkeeping).  LK_HOST_REWARP=1 keeps the host path (tests compare the two).
static int rewarp_on_device(lk_engine *e, const float *centers_xy, const float *offsets_xy) {
  Range range_("lk:rebuild moved lists");
  const int S = e->S;
  const lk_config &cfg = e->cfg;
  hipStream_t st = e->stream;
  const std::vector<int> levels = list_levels(cfg);
  std::vector<uint32_t> off0((size_t)S + 1, 0u);
  bool explicit_already = true;
  uint64_t sum = 0;
  for (int s = 0; s < S; ++s) {
    const int4 r = e->h_rect[0][(size_t)s];
    sum += r.z > 0 ? (uint32_t)r.w : e->h_off[0][(size_t)s + 1] - e->h_off[0][(size_t)s];
    explicit_already = explicit_already && r.z == 0;
    off0[(size_t)s + 1] = (uint32_t)sum;
  }
  if (sum >= 0xffffffffull)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_rewarp_sectors: more than 2^32 samples");
  const uint32_t total = (uint32_t)sum;
  HIPCHK(e->d_xy0_alt.ensure((size_t)total + 1));
  const uint32_t *dst_off = e->d_off[0].p;
  if (!explicit_already) { // (a blocking copy: the alternate table has no reader in flight)
    HIPCHK(e->d_off0_alt.ensure((size_t)S + 1));
    HIPCHK(hipMemcpy(e->d_off0_alt.p, off0.data(), ((size_t)S + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    dst_off = e->d_off0_alt.p;
  }
  LkRewarpArgs a{};
  a.src_xy = e->d_xy[0].p;
  a.src_off = e->d_off[0].p;
  a.src_rect = e->d_rect[0].p;
  a.dst_off = dst_off;
  a.dst_xy = e->d_xy0_alt.p;
  a.center = e->d_center.p;
  a.p = e->d_last_eval_p.p;
  a.n_sectors = S;
  a.total = total;
  if (offsets_xy) { // Lagrangian description: the sectors' offsets instead of the warp
    e->h_offsets.assign(offsets_xy, offsets_xy + 2 * (size_t)S);
    HIPCHK(e->d_offsets.ensure((size_t)S));
    HIPCHK(hipMemcpyAsync(e->d_offsets.p, e->h_offsets.data(), 2 * (size_t)S * sizeof(float), hipMemcpyHostToDevice, st));
    a.offset = e->d_offsets.p;
  }
  HIPCHK(lk_launch_rewarp(a, cfg.fitting_model, st));
  // The evaluation copy moves with the lists (sample by sample: it stays a permutation of them with the same offsets);
  // an implicit rectangle that becomes a list here gets one - its samples row by row, where the list proper has the
  // reference's x outer / y inner (a 19 x 19 sector: 32 consecutive samples on 19 image rows instead of 2).
  bool any_rect = false;
  for (int s = 0; s < S; ++s)
    any_rect = any_rect || e->h_rect[0][(size_t)s].z > 0;
  const bool keep_eval = (e->eval_lists || any_rect) && env_int("LK_EVAL_LISTS", 1) != 0; // test / tuning hook, read per call
  if (keep_eval) {
    HIPCHK(e->d_xy_eval0_alt.ensure((size_t)total + 1));
    LkRewarpArgs b = a;
    b.src_xy = e->eval_lists ? e->d_xy_eval[0].p : e->d_xy[0].p; // (explicit sectors of a mixed domain without a copy: list order)
    b.dst_xy = e->d_xy_eval0_alt.p;
    b.rows = 1;
    HIPCHK(lk_launch_rewarp(b, cfg.fitting_model, st));
  }
  // what lk_restore_sectors needs: the previous lists stay in the alternate buffer when they
  // were device-built too, otherwise the host records are still good
  if (e->lists_on_device) {
    e->backup_on_device = true;
  } else {
    e->hs_backup = e->hs;
    e->backup_on_device = false;
  }
  e->h_center_prev = e->h_center;
  e->eval_lists = false; // (until its coarser levels are rebuilt below)
  if (keep_eval)
    std::swap(e->d_xy_eval[0], e->d_xy_eval0_alt);
  for (HostSector &h : e->hs) // (descriptions of annular / blob sectors no longer describe the moved lists)
    h.lazy = 0;
  std::swap(e->d_xy[0], e->d_xy0_alt);
  if (!explicit_already)
    std::swap(e->d_off[0], e->d_off0_alt);
  e->h_off[0] = off0;
  for (int l : levels) {
    HIPCHK(hipMemsetAsync(e->d_rect[l].p, 0, (size_t)S * sizeof(int4), st));
    e->h_rect[l].assign((size_t)S, make_int4(0, 0, 0, 0));
  }
  HIPCHK(e->d_level_total.ensure(2 * LK_MAX_LEVELS));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)e->d_level_total.p, (int)total, 1, st));
  HIPCHK(e->d_pos.ensure((size_t)total + 1));
  HIPCHK(e->d_tiles.ensure((size_t)lk_decimate_tiles(total) + 2));
  for (size_t li = 1; li < levels.size(); ++li) {
    const int l = levels[li], pl = levels[li - 1];
    HIPCHK(e->d_xy[l].ensure((size_t)total + 1)); // any count up to the finer level's can be kept
    HIPCHK(lk_launch_decimate(e->d_xy[pl].p, e->d_off[pl].p, e->d_level_total.p + pl, total, l - pl, S, e->d_pos.p,
                              e->d_tiles.p, e->d_xy[l].p, e->d_off[l].p, e->d_level_total.p + l, st));
    e->h_off[l].resize((size_t)S + 1);
    HIPCHK(hipMemcpyAsync(e->h_off[l].data(), e->d_off[l].p, ((size_t)S + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          st));
  }
  if (keep_eval) { // the same decimation of the moved copy: the same sets, the offsets just computed
    HIPCHK(e->d_off_eval.ensure((size_t)S + 1));
    for (size_t li = 1; li < levels.size(); ++li) {
      const int l = levels[li], pl = levels[li - 1];
      HIPCHK(e->d_xy_eval[l].ensure((size_t)total + 1));
      HIPCHK(lk_launch_decimate(e->d_xy_eval[pl].p, e->d_off[pl].p, e->d_level_total.p + pl, total, l - pl, S, e->d_pos.p,
                                e->d_tiles.p, e->d_xy_eval[l].p, e->d_off_eval.p, e->d_level_total.p + LK_MAX_LEVELS + l, st));
    }
    e->eval_lists = true;
  }
  if (centers_xy) {
    e->h_center.assign(centers_xy, centers_xy + 2 * (size_t)S);
    HIPCHK(hipMemcpyAsync(e->d_center.p, e->h_center.data(), 2 * (size_t)S * sizeof(float), hipMemcpyHostToDevice, st));
  } else {
    HIPCHK(lk_launch_mean_center(e->d_xy[0].p, e->d_off[0].p, S, e->d_center.p, st));
    HIPCHK(hipMemcpyAsync(e->h_center.data(), e->d_center.p, 2 * (size_t)S * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  e->lists_on_device = true;
  e->lv_dirty = true;
  e->stats_valid = false;
  return refresh_starved(e);
}

int lk_rewarp_sectors(lk_engine *e, const float *centers_xy) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_rewarp_sectors: sectors are not committed");
  HIPCHK(hipSetDevice(e->cfg.device));
  const bool host_path = env_int("LK_HOST_REWARP", 0) != 0; // test hook, read per call
  if (!host_path && !e->recommit_pending)
    return rewarp_on_device(e, centers_xy);
  {
    int rc = materialize_host(e);
    if (rc)
      return rc;
  }
  std::vector<float> ev(6 * (size_t)e->S);
  HIPCHK(hipMemcpyAsync(ev.data(), e->d_last_eval_p.p, ev.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->hs_backup = e->hs;
  e->backup_on_device = false;
  for (int s = 0; s < e->S; ++s)
    rewarp_one(e->hs[(size_t)s], e->cfg.fitting_model, &ev[6 * (size_t)s],
               centers_xy ? centers_xy + 2 * (size_t)s : nullptr);
  return commit_impl(e, true);
}

// cudaPolygon::updatePolygon's call shape (cuda_class.cu:569, one sector, the engine's own
// last record of it) with the CPU engine's meaning: the sector moves to where update_results
// (manager_class.cpp:2406-2411) puts its centre, c + (u, v).  The re-commit is deferred to
// the next solve.  mode: deformationDescriptionEnum (0 strict Lagrangian, 1 Lagrangian, 2 Eulerian).
int lk_update_sector(lk_engine *e, int sector, int mode) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed || sector < 0 || sector >= e->S || mode < 0 || mode > 2)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_update_sector: unknown sector / mode");
  if (mode == 2)
    return LK_ERROR_NONE;
  HIPCHK(hipSetDevice(e->cfg.device));
  {
    int rc = materialize_host(e);
    if (rc)
      return rc;
  }
  lk_result r;
  float ev[6];
  HIPCHK(hipMemcpyAsync(&r, e->d_result.p + sector, sizeof(r), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(ev, e->d_last_eval_p.p + 6 * (size_t)sector, sizeof(ev), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  HostSector &h = e->hs[(size_t)sector];
  const float *m = r.resultingParameters;
  const float def_cx = h.cx + m[0], def_cy = e->P > 1 ? h.cy + m[1] : h.cy; // interpolation_class.cpp:3-43
  const float center[2] = {(float)(int)(def_cx + 0.5f), (float)(int)(def_cy + 0.5f)}; // manager_class.cpp:2087-2088
  const bool was_rect = h.is_rect;
  if (mode == 1)
    translate_one(h, def_cx - h.cx, def_cy - h.cy, h.has_center ? center : nullptr);
  else
    rewarp_one(h, e->cfg.fitting_model, ev, h.has_center ? center : nullptr);
  // A rectangle that moved by whole pixels is still an implicit rectangle of the same size: its records are
  // patched in place (O(levels) host work, one small launch; sequence state untouched), so that the reference's
  // per-sector loop - updatePolygon(i), correlate(i) for every sector (cuda_class.cu:569, manager_class.cpp:449) -
  // stays O(S).  Anything else (a sector that became a list) rebuilds everything before the next solve.
  if (was_rect && h.is_rect && e->append_ok && !e->recommit_pending && !e->lists_on_device) {
    const lk_config &cfg = e->cfg;
    LkAppendArgs a{};
    a.sector = sector;
    a.keep_state = 1;
    a.center = make_float2(h.cx, h.cy);
    a.d_center = e->d_center.p;
    e->h_center[2 * (size_t)sector] = h.cx;
    e->h_center[2 * (size_t)sector + 1] = h.cy;
    int li = 0;
    for (int l : list_levels(cfg)) {
      const int4 rc = h.rect_at(l);
      e->h_rect[l][(size_t)sector] = rc;
      a.rect[li] = rc;
      a.d_rect[li++] = e->d_rect[l].p;
      if (l == cfg.py_stop && rc.w <= starved_max(e) && !e->class_starved[e->h_class[(size_t)sector]]) {
        e->class_starved[e->h_class[(size_t)sector]] = true;
        HIPCHK(e->d_finish_list.ensure((size_t)std::max<size_t>(e->d_order.n, (size_t)e->S)));
        HIPCHK(e->d_finish_count.ensure(kNumClasses));
      }
    }
    a.n_levels = li;
    HIPCHK(lk_launch_append_sector(a, e->stream));
    return LK_ERROR_NONE;
  }
  e->recommit_pending = true;
  return LK_ERROR_NONE;
}

// Sectors the manager's loop never reached on a frame that stopped at an error
// (manager_class.cpp:520-546) keep the samples of the previous frame.
int lk_restore_sectors(lk_engine *e, int first_sector) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed || first_sector < 0)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_restore_sectors: nothing to restore");
  {
    int rc = materialize_host(e);
    if (!rc && e->backup_on_device) {
      e->hs_backup = e->hs;
      rc = lists_from_device(e, e->d_xy0_alt.p, e->h_center_prev, e->hs_backup);
      e->backup_on_device = false;
    }
    if (rc)
      return rc;
  }
  if (e->hs_backup.size() != e->hs.size())
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_restore_sectors: nothing to restore");
  for (size_t s = (size_t)first_sector; s < e->hs.size(); ++s)
    e->hs[s] = e->hs_backup[s];
  return commit_impl(e, true);
}

int lk_get_last_evaluated_parameters(lk_engine *e, float *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed || !out)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_last_evaluated_parameters: sectors are not committed");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipMemcpyAsync(out, e->d_last_eval_p.p, 6 * (size_t)e->S * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return LK_ERROR_NONE;
}

int lk_sector_count(const lk_engine *e) { return e ? (e->committed ? e->S : (int)e->hs.size()) : 0; }

int lk_get_sector_info(lk_engine *e, int sector, int *n_points, float *cx, float *cy) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (sector < 0 || (size_t)sector >= e->hs.size() || !e->hs[(size_t)sector].set)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_sector_info: unknown sector");
  if (e->lists_on_device && e->committed) { // device-built lists: counts and centres are on the host already
    const size_t q = (size_t)sector;
    const int4 r0 = e->h_rect[0][q];
    if (n_points)
      *n_points = r0.z > 0 ? r0.w : (int)(e->h_off[0][q + 1] - e->h_off[0][q]);
    if (cx)
      *cx = e->h_center[2 * q];
    if (cy)
      *cy = e->h_center[2 * q + 1];
    return LK_ERROR_NONE;
  }
  if (int rc = materialize_host(e))
    return rc;
  e->hs[(size_t)sector].realize();
  const HostSector &s = e->hs[(size_t)sector];
  if (n_points)
    *n_points = s.n0();
  if (cx)
    *cx = s.cx;
  if (cy)
    *cy = s.cy;
  return LK_ERROR_NONE;
}

int lk_get_sector_level_count(lk_engine *e, int sector, int level, int *n) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed || sector < 0 || sector >= e->S || level < 0 || level >= LK_MAX_LEVELS ||
      e->h_off[level].size() != (size_t)e->S + 1)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_sector_level_count: unknown sector/level");
  if (n) {
    const int4 r = e->h_rect[level][(size_t)sector];
    *n = r.z > 0 ? r.w : (int)(e->h_off[level][(size_t)sector + 1] - e->h_off[level][(size_t)sector]);
  }
  return LK_ERROR_NONE;
}

int lk_get_level_xy(lk_engine *e, int level, int which, int sector, float *xy, int cap, int *count) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed || sector < 0 || sector >= e->S || level < 0 || level >= LK_MAX_LEVELS ||
      e->h_off[level].size() != (size_t)e->S + 1)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_level_xy: unknown sector/level");
  if (which != 0 && !e->eval_lists)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_level_xy: the domain has no evaluation copy of its lists");
  const uint32_t b = e->h_off[level][(size_t)sector];
  const uint32_t n = e->h_rect[level][(size_t)sector].z > 0 ? 0u : e->h_off[level][(size_t)sector + 1] - b;
  if (count)
    *count = (int)n;
  if (xy && cap > 0 && n > 0) {
    const float2 *src = which ? e->d_xy_eval[level].p : e->d_xy[level].p;
    if (!src)
      return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_level_xy: the lists of this level are not on the device");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(xy, src + b, sizeof(float2) * (size_t)std::min((int)n, cap), hipMemcpyDeviceToHost));
  }
  return LK_ERROR_NONE;
}

int lk_get_und_xy(lk_engine *e, int sector, float *xy, int cap, int *count) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (sector < 0 || (size_t)sector >= e->hs.size() || !e->hs[(size_t)sector].set)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_und_xy: unknown sector");
  if (e->lists_on_device && e->committed && e->h_rect[0][(size_t)sector].z == 0) { // that sector's list only
    const uint32_t b = e->h_off[0][(size_t)sector], n = e->h_off[0][(size_t)sector + 1] - b;
    if (count)
      *count = (int)n;
    if (xy && cap > 0) {
      HIPCHK(hipSetDevice(e->cfg.device));
      HIPCHK(hipStreamSynchronize(e->stream));
      HIPCHK(hipMemcpy(xy, e->d_xy[0].p + b, sizeof(float2) * (size_t)std::min((int)n, cap), hipMemcpyDeviceToHost));
    }
    return LK_ERROR_NONE;
  }
  if (int rc = materialize_host(e))
    return rc;
  e->hs[(size_t)sector].realize();
  const HostSector &s = e->hs[(size_t)sector];
  int n = s.n0();
  if (count)
    *count = n;
  if (xy && cap > 0) {
    std::vector<float> pts = s.points();
    std::memcpy(xy, pts.data(), 2 * sizeof(float) * (size_t)std::min(n, cap));
  }
  return LK_ERROR_NONE;
}

int lk_get_def_xy(lk_engine *e, int sector, const float *p, float *xy, int cap, int *count) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed || sector < 0 || sector >= e->S || !p)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_def_xy: unknown sector");
  if (int rc = materialize_host(e))
    return rc;
  const std::vector<float> pts = e->hs[(size_t)sector].points();
  const int n = (int)(pts.size() / 2);
  if (count)
    *count = n;
  if (!xy || cap <= 0)
    return LK_ERROR_NONE;
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(e->d_warp.ensure(2 * (size_t)n));
  HIPCHK(hipMemcpyAsync(e->d_warp.p + n, pts.data(), 2 * sizeof(float) * (size_t)n, hipMemcpyHostToDevice,
                        e->stream));
  float pp[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < e->P; ++i)
    pp[i] = p[i];
  HIPCHK(hipMemcpyAsync(e->d_scratch.p, pp, sizeof(pp), hipMemcpyHostToDevice, e->stream));
  HIPCHK(lk_launch_warp_points(e->d_warp.p + n, n, e->h_center[2 * (size_t)sector],
                               e->h_center[2 * (size_t)sector + 1], e->cfg.fitting_model, e->d_scratch.p,
                               e->d_warp.p, e->stream));
  HIPCHK(hipMemcpyAsync(xy, e->d_warp.p, 2 * sizeof(float) * (size_t)std::min(n, cap),
                        hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return LK_ERROR_NONE;
}
