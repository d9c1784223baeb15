// lk_engine_sectors.cpp - the sectors of the engine: registration, the device ROI masks, the size-class analysis, the
// commit and its append path.  (What moves committed sectors, and the getters, are lk_engine_moves.cpp.)
#include "lk_engine_state.hpp"

// Level-0 lists that live on the device only (after lk_rewarp_sectors) -> HostSector records.
int lists_from_device(lk_engine *e, const float2 *d_xy0, const std::vector<float> &centers, std::vector<HostSector> &out) {
  const size_t S = (size_t)e->S, total = e->h_off[0][S];
  std::vector<float> xy(2 * total + 2);
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipMemcpyAsync(xy.data(), d_xy0, total * sizeof(float2), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (size_t s = 0; s < S; ++s) {
    HostSector &h = out[s];
    h.xy.assign(xy.begin() + 2 * (size_t)e->h_off[0][s], xy.begin() + 2 * (size_t)e->h_off[0][s + 1]);
    h.is_rect = false;
    h.lazy = 0;
    h.cx = centers[2 * s];
    h.cy = centers[2 * s + 1];
  }
  return LK_ERROR_NONE;
}

// every entry point that reads or edits e->hs calls this first
int materialize_host(lk_engine *e) {
  if (!e->lists_on_device)
    return LK_ERROR_NONE;
  int rc = lists_from_device(e, e->d_xy[0].p, e->h_center, e->hs);
  if (rc)
    return rc;
  e->lists_on_device = false;
  return LK_ERROR_NONE;
}

int lk_clear_sectors(lk_engine *e) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  e->lists_on_device = e->backup_on_device = false;
  e->hs.clear();
  e->committed = false;
  e->append_ok = false;
  e->S = 0;
  return LK_ERROR_NONE;
}

// LK_HOST_ROI=1 (test / comparison hook, read per call): annular and blob sectors are rasterised by
// the host scan at registration, as in round 1, instead of by the device mask at commit
static bool host_roi() { return env_int("LK_HOST_ROI", 0) != 0; }

static HostSector *sector_slot(lk_engine *e, int sector) {
  if (sector < 0 || materialize_host(e))
    return nullptr;
  if ((size_t)sector >= e->hs.size())
    e->hs.resize((size_t)sector + 1);
  if (sector < e->S)
    e->append_ok = false; // a committed sector is registered anew: the next commit rebuilds
  e->committed = false;
  e->hs[(size_t)sector].fresh = true;
  e->hs[(size_t)sector].lazy = 0; // (annular / blob registration sets it again)
  return &e->hs[(size_t)sector];
}

int lk_set_sector_rect(lk_engine *e, int sector, int x0, int y0, int x1, int y1) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  HostSector *s = sector_slot(e, sector);
  if (!s || x1 < x0 || y1 < y0)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sector_rect: bad rectangle");
  s->xy.clear();
  s->is_rect = true;
  s->x0 = x0;
  s->y0 = y0;
  s->x1 = x1;
  s->y1 = y1;
  s->cx = (float)(x0 + x1) * 0.5f;
  s->cy = (float)(y0 + y1) * 0.5f;
  s->has_center = true;
  s->set = true;
  return LK_ERROR_NONE;
}

int lk_set_rect_grid(lk_engine *e, float x_begin, float y_begin, float x_end, float y_end, int hs, int vs,
                     int first, int count) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (hs < 1 || vs < 1)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_rect_grid: subdivisions must be >= 1");
  const int total = hs * vs;
  if (count < 0)
    count = total - first;
  if (first < 0 || count < 0 || first + count > total)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_rect_grid: sector range outside the grid");
  lkroi::RectGrid g = lkroi::rect_grid(x_begin, y_begin, x_end, y_end, hs, vs);
  if (g.xdim < 0 || g.ydim < 0)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_rect_grid: domain smaller than the grid");
  e->lists_on_device = e->backup_on_device = false;
  e->hs.clear();
  e->hs.resize((size_t)count);
  e->committed = false;
  e->append_ok = false;
  for (int k = 0; k < count; ++k) {
    int iSector = first + k, i = iSector / vs, j = iSector % vs; // iSector = i*vs + j
    HostSector &s = e->hs[(size_t)k];
    int cx = g.cx[i], cy = g.cy[j];
    s.is_rect = true;
    s.x0 = cx - g.xdim;
    s.y0 = cy - g.ydim;
    s.x1 = cx + g.xdim;
    s.y1 = cy + g.ydim;
    s.cx = (float)cx; // manager_class.cpp:438-441 passes the integer centre
    s.cy = (float)cy;
    s.has_center = true;
    s.set = true;
  }
  return LK_ERROR_NONE;
}

int lk_set_sector_annular(lk_engine *e, int sector, float r, float dr, float a, float da, float cx, float cy,
                          int as) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  HostSector *s = sector_slot(e, sector);
  if (!s)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sector_annular: bad sector index");
  s->xy.clear();
  s->is_rect = false;
  s->flats.clear();
  if (!lkroi::annular_geometry(r, dr, a, da, cx, cy, as, s->ag))
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sector_annular: bad sector description");
  s->lazy = 1; // the samples come from the device mask at commit (or from realize())
  if (host_roi()) {
    s->realize();
    if (s->xy.empty())
      return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sector_annular: empty sector");
  }
  s->has_center = false;
  s->set = true;
  return LK_ERROR_NONE;
}

int lk_set_sectors_annular(lk_engine *e, int first_sector, int count, const float *params, int as) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (first_sector < 0 || count < 1 || !params)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sectors_annular: bad arguments");
  if (!sector_slot(e, first_sector + count - 1)) // sizes the table once, before the threads
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sectors_annular: bad sector range");
  const bool on_host = host_roi();
  const unsigned hw = std::thread::hardware_concurrency();
  const int workers = on_host ? std::max(1, std::min({count, 16, (int)(hw ? hw : 1)})) : 1;
  std::vector<int> empty((size_t)workers, 0);
  auto work = [&](int w) {
    for (int k = w; k < count; k += workers) { // interleaved: neighbouring rings have similar sizes
      const float *q = params + 6 * (size_t)k;
      HostSector &s = e->hs[(size_t)(first_sector + k)];
      s.xy.clear();
      s.is_rect = false;
      s.flats.clear();
      s.fresh = true;
      if (!lkroi::annular_geometry(q[0], q[1], q[2], q[3], q[4], q[5], as, s.ag)) {
        empty[(size_t)w] = 1;
        continue;
      }
      s.lazy = 1; // the device mask makes the list at commit; LK_HOST_ROI=1: the host scan, here
      if (on_host) {
        s.realize();
        if (s.xy.empty()) {
          empty[(size_t)w] = 1;
          continue;
        }
      }
      s.has_center = false;
      s.set = true;
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < workers; ++w)
    th.emplace_back(work, w);
  work(0);
  for (std::thread &t : th)
    t.join();
  for (int v : empty)
    if (v)
      return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sectors_annular: empty sector");
  return LK_ERROR_NONE;
}

int lk_set_sector_blob(lk_engine *e, int sector, const float *contour_xy, int n_vertices) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  HostSector *s = sector_slot(e, sector);
  if (!s || !contour_xy)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sector_blob: bad arguments");
  s->xy.clear();
  s->is_rect = false;
  s->flats.clear();
  s->lazy = 0;
  if (host_roi()) { // round 1's path: ear clipping + scan fill on a few host threads
    if (!lkroi::BlobPolygon::inside_points(contour_xy, n_vertices, s->xy) || s->xy.empty()) {
      s->set = false;
      return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sector_blob: contour is not a simple polygon");
    }
    lkroi::mean_center(s->xy.data(), (int)(s->xy.size() / 2), s->cx, s->cy);
  } else { // the ear clipper stays on the host (O(vertices^2)); the fill is the device mask's, at commit
    if (!lkroi::BlobPolygon::flat_triangles(contour_xy, n_vertices, s->flats) || s->flats.empty()) {
      s->set = false;
      return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sector_blob: contour is not a simple polygon");
    }
    s->lazy = 2;
  }
  s->has_center = false;
  s->set = true;
  return LK_ERROR_NONE;
}

int lk_set_sector_points(lk_engine *e, int sector, const float *xy, int n, int use_center, float cx,
                         float cy) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  HostSector *s = sector_slot(e, sector);
  if (!s || !xy || n < 1)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_sector_points: bad arguments");
  s->xy.assign(xy, xy + 2 * (size_t)n);
  s->is_rect = false;
  if (use_center) {
    s->cx = cx;
    s->cy = cy;
  } else {
    lkroi::mean_center(xy, n, s->cx, s->cy);
  }
  s->has_center = use_center != 0;
  s->set = true;
  return LK_ERROR_NONE;
}

// Starved levels (at most 2P samples for P parameters; always the coarsest ones) are solved
// first by the one-lane-per-sector kernel, bit-identically to the reference.  Needs h_class,
// h_rect and h_off of the coarsest level.
// (the tuning hook LK_STARVED_MAX is read at every commit and kept with the engine: the host's class table and
// the kernel's hand-over rule must agree)
// (LK_STARVED_MAX=none: kStarvedNone, see starved_max())
int refresh_starved(lk_engine *e) {
  const int S = (int)e->h_class.size();
  {
    const char *f = std::getenv("LK_STARVED_MAX"); // tuning hook (tests/tools/c4_parity.py): the one hook with a word for a value
    e->starved_max = f && std::strcmp(f, "none") == 0 ? kStarvedNone : std::max(env_int("LK_STARVED_MAX", -1), -1);
  }
  for (int c = 0; c < kNumClasses; ++c)
    e->class_starved[c] = false;
  e->force_safe = env_int("LK_FORCE_SAFE", e->force_safe) != 0; // tuning / test hook, read per commit
  const int l = e->cfg.py_stop; // counts only shrink with the level: test the coarsest
  bool any_starved = false;
  for (int s = 0; s < S; ++s) {
    const int4 r = e->h_rect[l][(size_t)s];
    const int n = r.z > 0 ? r.w : (int)(e->h_off[l][(size_t)s + 1] - e->h_off[l][(size_t)s]);
    if (n <= starved_max(e))
      e->class_starved[e->h_class[(size_t)s]] = any_starved = true;
  }
  if (any_starved) {
    HIPCHK(e->d_finish_list.ensure((size_t)S));
    HIPCHK(e->d_finish_count.ensure(kNumClasses));
  }
  return LK_ERROR_NONE;
}

// Device ROI masks: every sector of the domain is annular or a blob and registered by description.
// Replaces cudaPolygon{Annular,Blob}'s thrust rasterise + remove_if (cuda_polygon.cuh:180-292,
// cuda_polygon.cu:589-627) with the CPU engine's predicates and sample order.  Leaves d_xy / d_off
// of every level, d_center, h_off, h_center and zeroed rectangles behind; the lists stay on the device.
static int build_lists_roi_device(lk_engine *e, const std::vector<int> &levels) {
  Range range_("lk:roi masks");
  const int S = (int)e->hs.size();
  hipStream_t st = e->stream;
  std::vector<LkRoiSector> sec((size_t)S);
  std::vector<LkRoiFlat> flats;
  std::vector<uint32_t> tile_begin((size_t)S + 1, 0u);
  uint64_t tiles = 0;
  bool non_negative = true; // every coordinate the masks can produce is >= 0 and below 2^15 (lk_mean_center_int_kernel)
  for (int s = 0; s < S; ++s) {
    const HostSector &h = e->hs[(size_t)s];
    LkRoiSector &q = sec[(size_t)s];
    std::memset(&q, 0, sizeof(q));
    tile_begin[(size_t)s] = (uint32_t)tiles;
    if (h.lazy == 1) {
      const lkroi::AnnularGeometry &g = h.ag;
      q.kind = 0;
      q.x0 = g.x0, q.y0 = g.y0, q.x1 = g.x1, q.y1 = g.y1;
      q.cx = g.cx, q.cy = g.cy, q.ri2 = g.ri2, q.ro2 = g.ro2;
      q.q00x = g.q00x, q.q01x = g.q01x, q.q10x = g.q10x, q.q11x = g.q11x;
      q.q00y = g.q00y, q.q01y = g.q01y, q.q10y = g.q10y, q.q11y = g.q11y;
      q.as = g.as;
      const int64_t w = std::max(0, g.x1 - g.x0), hh = std::max(0, g.y1 - g.y0);
      if (w * hh >= (int64_t)1 << 31)
        return e->fail(LK_ERROR_BAD_DOMAIN, "lk_commit_sectors: annular sector bounding box too large");
      q.x1 = q.x0 + (int)w, q.y1 = q.y0 + (int)hh;
      // kept samples lie strictly inside the outer circle (and inside the bounding box)
      non_negative = non_negative && std::max((float)q.x0, g.cx - g.ro) >= 0.f && std::max((float)q.y0, g.cy - g.ro) >= 0.f &&
                     q.x1 < (1 << 15) && q.y1 < (1 << 15);
      tiles += (uint64_t)((w * hh + kLkRoiTile - 1) / kLkRoiTile);
    } else {
      q.kind = 1;
      q.flat_begin = (int)flats.size();
      q.flat_count = (int)h.flats.size();
      uint64_t rows = 0;
      for (const lkroi::BlobPolygon::Flat &f : h.flats) {
        LkRoiFlat d;
        d.ls = f.ls, d.li = f.li, d.rs = f.rs, d.ri = f.ri, d.j0 = f.j0, d.j1 = f.j1;
        d.row_begin = (int)rows;
        rows += (uint64_t)(f.j1 - f.j0);
        flats.push_back(d);
        // pixel range of its two end rows (the edges are straight: the extremes are there)
        for (int j : {f.j0, f.j1 - 1}) {
          const float a = std::ceil(f.ls * (float)j + f.li), b = std::ceil(f.rs * (float)j + f.ri);
          non_negative = non_negative && j >= 0 && j < (1 << 15) && a >= 0.f && b < 32768.f;
        }
      }
      tiles += rows;
    }
    if (tiles >= (uint64_t)1 << 31)
      return e->fail(LK_ERROR_BAD_DOMAIN, "lk_commit_sectors: region of interest too large for the device mask");
  }
  tile_begin[(size_t)S] = (uint32_t)tiles;
  const uint32_t n_tiles = (uint32_t)tiles;
  if (n_tiles == 0)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_commit_sectors: empty region of interest");
  HIPCHK(e->d_roi_sectors.ensure((size_t)S));
  HIPCHK(e->d_roi_flats.ensure(flats.size() + 1));
  HIPCHK(e->d_roi_tile_begin.ensure((size_t)S + 1));
  HIPCHK(hipMemcpyAsync(e->d_roi_sectors.p, sec.data(), (size_t)S * sizeof(LkRoiSector), hipMemcpyHostToDevice, st));
  if (!flats.empty())
    HIPCHK(hipMemcpyAsync(e->d_roi_flats.p, flats.data(), flats.size() * sizeof(LkRoiFlat), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(e->d_roi_tile_begin.p, tile_begin.data(), ((size_t)S + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIPCHK(e->d_level_total.ensure(2 * LK_MAX_LEVELS)); // (second half: scratch of the evaluation copy's passes)
  // (the tile table may be larger than the decimation's: both share d_tiles)
  HIPCHK(e->d_tiles.ensure(4 * (size_t)n_tiles + 2)); // (also enough for the decimation passes below in all but pathological blobs)
  HIPCHK(lk_launch_roi_count(e->d_roi_sectors.p, e->d_roi_flats.p, e->d_roi_tile_begin.p, S, n_tiles, e->d_tiles.p,
                             e->d_level_total.p, st));
  uint32_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, e->d_level_total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st)); // the list buffers are sized by the count
  if (total == 0)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_commit_sectors: empty region of interest");
  for (int l : levels) {
    HIPCHK(e->d_xy[l].ensure((size_t)total + 1));
    HIPCHK(e->d_off[l].ensure((size_t)S + 1));
    HIPCHK(e->d_rect[l].ensure((size_t)S));
    HIPCHK(hipMemsetAsync(e->d_rect[l].p, 0, (size_t)S * sizeof(int4), st));
    e->h_rect[l].assign((size_t)S, make_int4(0, 0, 0, 0));
    e->h_off[l].assign((size_t)S + 1, 0u);
  }
  HIPCHK(lk_launch_roi_fill(e->d_roi_sectors.p, e->d_roi_flats.p, e->d_roi_tile_begin.p, S, n_tiles, e->d_tiles.p,
                            e->d_xy[0].p, e->d_off[0].p, st));
  HIPCHK(hipMemcpyAsync(e->h_off[0].data(), e->d_off[0].p, ((size_t)S + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  // coarser levels: pyramid_class.cpp:289-323 for all sectors at once (the kernels of lk_rewarp_sectors)
  HIPCHK(e->d_pos.ensure((size_t)total + 1));
  HIPCHK(e->d_tiles.ensure((size_t)std::max<uint32_t>(n_tiles, (uint32_t)lk_decimate_tiles(total)) + 2));
  for (size_t li = 1; li < levels.size(); ++li) {
    const int l = levels[li], pl = levels[li - 1];
    HIPCHK(lk_launch_decimate(e->d_xy[pl].p, e->d_off[pl].p, e->d_level_total.p + pl, total, l - pl, S, e->d_pos.p,
                              e->d_tiles.p, e->d_xy[l].p, e->d_off[l].p, e->d_level_total.p + l, st));
    HIPCHK(hipMemcpyAsync(e->h_off[l].data(), e->d_off[l].p, ((size_t)S + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  // centres: the float mean of the samples in list order (correlation_class.cpp:337-339)
  HIPCHK(e->d_center.ensure((size_t)S));
  e->h_center.resize(2 * (size_t)S);
  // (the mask's coordinates are integers; non-negative ones - the ROI lies in the image - let the
  // chain be evaluated in parallel, see lk_mean_center_int_kernel)
  if (non_negative) {
    HIPCHK(e->d_mean_scratch.ensure((lk_mean_center_int_scratch_bytes(total, S) + 3) / 4));
    HIPCHK(lk_launch_mean_center_int(e->d_xy[0].p, e->d_off[0].p, total, S, e->d_mean_scratch.p, e->d_center.p, st));
  }
  else
    HIPCHK(lk_launch_mean_center(e->d_xy[0].p, e->d_off[0].p, S, e->d_center.p, st));
  HIPCHK(hipMemcpyAsync(e->h_center.data(), e->d_center.p, 2 * (size_t)S * sizeof(float), hipMemcpyDeviceToHost, st));
  // The evaluation copy: the same masks walked row by row (only annular sectors come out in another order; a blob's
  // scan lines are rows already), then the same decimation.  Same sample sets, hence the same offsets at every level.
  e->eval_lists = false;
  bool any_annular = false;
  for (int s = 0; s < S; ++s)
    any_annular = any_annular || e->hs[(size_t)s].lazy == 1;
  const bool eval_env = env_int("LK_EVAL_LISTS", 1) != 0; // test / tuning hook, read per commit
  if (any_annular && eval_env) {
    HIPCHK(e->d_off_eval.ensure((size_t)S + 1));
    uint32_t *totals = e->d_level_total.p + LK_MAX_LEVELS; // (scratch: the counts are the canonical lists')
    for (int l : levels)
      HIPCHK(e->d_xy_eval[l].ensure((size_t)total + 1));
    HIPCHK(e->d_tiles.ensure(4 * (size_t)n_tiles + 2));
    HIPCHK(lk_launch_roi_count(e->d_roi_sectors.p, e->d_roi_flats.p, e->d_roi_tile_begin.p, S, n_tiles, e->d_tiles.p, totals, st, 1));
    HIPCHK(lk_launch_roi_fill(e->d_roi_sectors.p, e->d_roi_flats.p, e->d_roi_tile_begin.p, S, n_tiles, e->d_tiles.p,
                              e->d_xy_eval[0].p, e->d_off_eval.p, st, 1));
    HIPCHK(e->d_tiles.ensure((size_t)std::max<uint32_t>(n_tiles, (uint32_t)lk_decimate_tiles(total)) + 2));
    for (size_t li = 1; li < levels.size(); ++li) {
      const int l = levels[li], pl = levels[li - 1];
      HIPCHK(lk_launch_decimate(e->d_xy_eval[pl].p, e->d_off[pl].p, e->d_level_total.p + pl, total, l - pl, S, e->d_pos.p,
                                e->d_tiles.p, e->d_xy_eval[l].p, e->d_off_eval.p, totals + l, st));
    }
    e->eval_lists = true;
  }
  HIPCHK(hipStreamSynchronize(st));
  for (int s = 0; s < S; ++s) {
    HostSector &h = e->hs[(size_t)s];
    h.n0_device = (int)(e->h_off[0][(size_t)s + 1] - e->h_off[0][(size_t)s]);
    if (h.n0_device == 0)
      return e->fail(LK_ERROR_BAD_DOMAIN, "lk_commit_sectors: sector " + std::to_string(s) + " is empty");
    h.cx = e->h_center[2 * (size_t)s];
    h.cy = e->h_center[2 * (size_t)s + 1];
  }
  e->lists_on_device = true;
  e->backup_on_device = false;
  return LK_ERROR_NONE;
}

// keep_state: a re-commit after the sample lists moved (Lagrangian descriptions) keeps the
// sequence state of the sectors (guess history, last results)
// Size classes -> lanes per sector, the launch order of the classes, starved-level flags and team widths of the
// committed domain (e->S sectors; needs h_rect / h_off).  Part of every full commit; after sectors were APPENDED
// (lk_commit_sectors' fast path) it is redone lazily by the next batch solve.
static int classify_sectors(lk_engine *e) {
  const int S = e->S;
  // size classes -> lanes per sector.  A class whose sectors are too few to fill the chip
  // (< 2048 wavefronts) and still large per lane is promoted to the next wider group.
  e->h_class.assign((size_t)S, 0);
  size_t cnt[kNumClasses] = {0, 0, 0, 0, 0, 0}, tot[kNumClasses] = {0, 0, 0, 0, 0, 0};
  for (int s = 0; s < S; ++s) {
    int n0 = level0_count(e, s), c = size_class(n0);
    e->h_class[(size_t)s] = c;
    cnt[c]++;
    tot[c] += (size_t)n0;
  }
  for (int c = 0; c + 1 < kTeamClass; ++c) { // (nothing is promoted into the team class)
    if (!cnt[c] || e->batch_invariant || e->reference_order > 0) // (the group depends on the sector alone)
      continue;
    // Wider groups shorten a sector's own critical path and cost lane packing: they pay only
    // while the narrow grouping leaves SIMDs without a wavefront (fewer wavefronts than the
    // 1024 SIMDs).  Measured on 19x19-sample sectors (scripts/quick_solve.py, LK_GRID /
    // LK_FORCE_GROUP): 1024 sectors 0.110 ms in 32-lane groups against 0.092 ms in 64-lane ones,
    // 2025 sectors 0.122 / 0.123, 4096 sectors 0.166 / 0.188, 8100 sectors 0.240 / 0.324.
    size_t waves = cnt[c] * (size_t)kGroupOfClass[c] / 64 * (size_t)e->pairs_in_flight; // (the other launches' too)
    size_t per_lane = tot[c] / cnt[c] / (size_t)kGroupOfClass[c];
    const bool small_group = kGroupOfClass[c] < 64;
    const size_t enough = kGroupOfClass[c] == 16 ? 4096 : 1024; // (16-lane groups: 10 000 sectors 0.31 against 0.27 ms)
    if ((small_group && waves < enough && per_lane >= 4) || (!small_group && waves < 2048 && per_lane >= 32)) {
      for (int s = 0; s < S; ++s)
        if (e->h_class[(size_t)s] == c)
          e->h_class[(size_t)s] = c + 1;
      cnt[c + 1] += cnt[c];
      tot[c + 1] += tot[c];
      cnt[c] = tot[c] = 0;
    }
  }
  const int force_group = env_int("LK_FORCE_GROUP", 0); // tuning experiments only (0: no class has that group)
  for (int c = 0; c < kNumClasses; ++c)
    if (kGroupOfClass[c] == force_group)
      std::fill(e->h_class.begin(), e->h_class.end(), c);
  const int force_team = env_int("LK_FORCE_TEAM", 0); // test hook: every sector gets a team of this width
  if (force_team >= 1) // (1: the team class's kernel with a single workgroup per sector)
    std::fill(e->h_class.begin(), e->h_class.end(), kTeamClass);
  e->team_w = 0;
  {
    // A handful of big sectors (one ROI in the GUI, BASELINE config 1) cannot fill the chip with
    // one workgroup each: when at most half of the CUs would be busy, every 8-wavefront sector
    // gets a team as well.  The kernel sizes each sector's team by its own sample count
    // (kTeamMinSamples per workgroup), the launch clamps the width to what is resident.
    int n_big = 0;
    for (int s = 0; s < S; ++s)
      n_big += e->h_class[(size_t)s] >= kTeamClass - 1;
    if (n_big > 0 && n_big <= kFewBigSectors && !e->batch_invariant && e->reference_order == 0)
      for (int s = 0; s < S; ++s)
        if (e->h_class[(size_t)s] == kTeamClass - 1)
          e->h_class[(size_t)s] = kTeamClass;
    int n_team = 0, n0_max = 0;
    for (int s = 0; s < S; ++s)
      if (e->h_class[(size_t)s] == kTeamClass) {
        ++n_team;
        n0_max = std::max(n0_max, level0_count(e, s));
      }
    if (n_team) {
      int w = force_team >= 1 ? force_team : (n0_max + kTeamMinSamples - 1) / kTeamMinSamples;
      const int max_team = std::min(std::max(2, env_int("LK_MAX_TEAM", kMaxTeam)), kLkMaxTeam); // tuning hook
      e->team_w = force_team == 1 ? 1 : std::min(std::max(w, 2), max_team); // the launch clamps it to what is resident
      e->team_min_samples = force_team >= 1 ? 0 : kTeamMinSamples;
      HIPCHK(e->d_team_partials.ensure((size_t)n_team * 2 * (size_t)e->team_w * 32));
      HIPCHK(e->d_team_arrivals.ensure(2 * (size_t)n_team)); // arrival counters + broken flags
    }
  }
  e->h_order.clear();
  e->h_order.reserve((size_t)S);
  for (int c = 0; c < kNumClasses; ++c) {
    e->class_begin[c] = (int)e->h_order.size();
    for (int s = 0; s < S; ++s)
      if (e->h_class[(size_t)s] == c)
        e->h_order.push_back((uint32_t)s);
  }
  e->class_begin[kNumClasses] = (int)e->h_order.size();
  // A team launch needs all its workgroups resident at once, and the one-workgroup class (one 512-thread workgroup per
  // sector, as many as there are CUs) would hold every slot until its first sectors are done: the two launches then run
  // one after the other whatever the streams say (config 3: 256 annular sectors 0.42 ms + the blob's team 0.40 ms).
  // Instead they split the slots by their share of the samples: the team gets its share (at least a quarter), the
  // one-workgroup class a persistent grid on the rest with its largest sectors first in the queue.
  e->team_share_permille = 0;
  {
    const int cb = kTeamClass - 1;
    const int n_one = e->class_begin[cb + 1] - e->class_begin[cb], n_team = e->class_begin[kTeamClass + 1] - e->class_begin[kTeamClass];
    const int share_env = env_int("LK_TEAM_SHARE", INT_MIN); // tuning hook: permille of the slots for the team class (0: no split; INT_MIN: not set)
    if (n_one > 0 && n_team > 0 && e->team_w > 1 && !e->batch_invariant && e->reference_order == 0 && share_env != 0) {
      double s_one = 0, s_team = 0;
      for (int s = 0; s < S; ++s) {
        if (e->h_class[(size_t)s] == cb)
          s_one += level0_count(e, s);
        else if (e->h_class[(size_t)s] == kTeamClass)
          s_team += level0_count(e, s);
      }
      // (its share of the samples.  Round 3 gave the team a quarter more for its all-to-all; with round 4's kernels config 3
      // measures 72 / 80 / 88 / 96 / 104 team workgroups -> 0.595 / 0.568 / 0.580 / 0.597 / 0.620 ms: 80 = the plain share)
      const int share = share_env != INT_MIN ? share_env : (int)(1000.0 * s_team / (s_team + s_one) + 0.5);
      e->team_share_permille = std::min(std::max(share, 250), 750);
      std::stable_sort(e->h_order.begin() + e->class_begin[cb], e->h_order.begin() + e->class_begin[cb + 1],
                       [&](uint32_t x, uint32_t y) { return level0_count(e, (int)x) > level0_count(e, (int)y); });
    }
  }
  {
    int rc = refresh_starved(e);
    if (rc)
      return rc;
  }
  HIPCHK(e->d_order.ensure((size_t)S));
  HIPCHK(hipMemcpy(e->d_order.p, e->h_order.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice));
  e->classes_dirty = false;
  e->bw_dirty = true;
  return LK_ERROR_NONE;
}

int commit_impl(lk_engine *e, bool keep_state) {
  Range range_("lk:commit sectors");
  if (int rc = materialize_host(e)) // (a no-op after any edit: editors fetch the lists first)
    return rc;
  const int S = (int)e->hs.size();
  if (S == 0)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_commit_sectors: no sectors");
  for (int s = 0; s < S; ++s)
    if (!e->hs[(size_t)s].set)
      return e->fail(LK_ERROR_BAD_DOMAIN, "lk_commit_sectors: sector " + std::to_string(s) + " was never set");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  const std::vector<int> levels = list_levels(e->cfg);
  // Annular / blob sectors registered by description: the device mask makes every list (level 0 by
  // lk_roi_tile_kernel, the coarser levels by the order-preserving compaction, centres by
  // lk_mean_center_kernel); only offsets and centres come back.  A domain that mixes them with
  // rectangles or explicit lists, or LK_HOST_ROI=1, takes the host scans instead (same lists).
  bool any_lazy = false, all_lazy = true;
  for (int s = 0; s < S; ++s) {
    any_lazy = any_lazy || e->hs[(size_t)s].lazy != 0;
    all_lazy = all_lazy && e->hs[(size_t)s].lazy != 0;
  }
  const bool device_roi = any_lazy && all_lazy && !host_roi();
  if (any_lazy && !device_roi)
    for (int s = 0; s < S; ++s)
      e->hs[(size_t)s].realize();
  if (any_lazy && !device_roi)
    for (int s = 0; s < S; ++s)
      if (!e->hs[(size_t)s].is_rect && e->hs[(size_t)s].xy.empty())
        return e->fail(LK_ERROR_BAD_DOMAIN, "lk_commit_sectors: sector " + std::to_string(s) + " is empty");
  e->eval_lists = false; // (only the device ROI path below builds the evaluation copy)
  if (device_roi) {
    int rc = build_lists_roi_device(e, levels);
    if (rc)
      return rc;
  }
  std::vector<std::vector<float>> cat(LK_MAX_LEVELS);
  if (!device_roi) {
  for (int l = 0; l < LK_MAX_LEVELS; ++l)
    e->h_off[l].assign(1, 0u);
  size_t total0 = 0;
  for (int s = 0; s < S; ++s)
    total0 += e->hs[(size_t)s].xy.size();
  if (total0 / 2 >= 0xffffffffull)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_commit_sectors: more than 2^32 samples");
  cat[0].reserve(total0);
  e->h_center.resize(2 * (size_t)S);
  for (int l : levels)
    e->h_rect[l].assign((size_t)S, make_int4(0, 0, 0, 0));
  // Long explicit lists (annular / blob domains) are decimated on the device: one order-
  // preserving compaction per coarser level over all sectors at once (the kernels of
  // lk_rewarp_sectors); LK_HOST_REWARP=1 keeps the restated reference loop (tests compare).
  const bool device_levels = env_int("LK_HOST_REWARP", 0) == 0 && total0 / 2 >= 32768 && levels.size() > 1; // (read per commit)
  std::vector<float> prev, cur;
  for (int s = 0; s < S; ++s) {
    const HostSector &hs = e->hs[(size_t)s];
    e->h_center[2 * (size_t)s] = hs.cx;
    e->h_center[2 * (size_t)s + 1] = hs.cy;
    if (hs.is_rect) {
      for (int l : levels) {
        e->h_rect[l][(size_t)s] = hs.rect_at(l);
        e->h_off[l].push_back((uint32_t)(cat[l].size() / 2));
      }
      continue;
    }
    cat[0].insert(cat[0].end(), hs.xy.begin(), hs.xy.end());
    e->h_off[0].push_back((uint32_t)(cat[0].size() / 2));
    if (device_levels)
      continue;
    const float *pxy = hs.xy.data();
    int pn = (int)(hs.xy.size() / 2), plevel = 0;
    for (size_t li = 1; li < levels.size(); ++li) {
      int l = levels[li];
      cur.clear();
      int kept = lkroi::decimate(pxy, pn, l - plevel, cur);
      cat[l].insert(cat[l].end(), cur.begin(), cur.end());
      e->h_off[l].push_back((uint32_t)(cat[l].size() / 2));
      prev.swap(cur);
      pxy = prev.data();
      pn = kept;
      plevel = l;
    }
  }
  for (int l : levels) {
    const bool on_device = device_levels && l > 0;
    HIPCHK(e->d_xy[l].ensure((on_device ? cat[0].size() : cat[l].size()) / 2 + 1));
    HIPCHK(e->d_off[l].ensure((size_t)S + 1));
    if (!on_device) {
      if (!cat[l].empty())
        HIPCHK(hipMemcpy(e->d_xy[l].p, cat[l].data(), cat[l].size() * sizeof(float), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(e->d_off[l].p, e->h_off[l].data(), ((size_t)S + 1) * sizeof(uint32_t),
                       hipMemcpyHostToDevice));
    }
    HIPCHK(e->d_rect[l].ensure((size_t)S));
    HIPCHK(hipMemcpy(e->d_rect[l].p, e->h_rect[l].data(), (size_t)S * sizeof(int4), hipMemcpyHostToDevice));
  }
  if (device_levels) {
    const uint32_t total = (uint32_t)(cat[0].size() / 2);
    HIPCHK(e->d_level_total.ensure(2 * LK_MAX_LEVELS)); // (second half: scratch of the evaluation copy's passes)
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)e->d_level_total.p, (int)total, 1, e->stream));
    HIPCHK(e->d_pos.ensure((size_t)total + 1));
    HIPCHK(e->d_tiles.ensure((size_t)lk_decimate_tiles(total) + 2));
    for (size_t li = 1; li < levels.size(); ++li) {
      const int l = levels[li], pl = levels[li - 1];
      HIPCHK(lk_launch_decimate(e->d_xy[pl].p, e->d_off[pl].p, e->d_level_total.p + pl, total, l - pl, S, e->d_pos.p,
                                e->d_tiles.p, e->d_xy[l].p, e->d_off[l].p, e->d_level_total.p + l, e->stream));
      e->h_off[l].resize((size_t)S + 1);
      HIPCHK(hipMemcpyAsync(e->h_off[l].data(), e->d_off[l].p, ((size_t)S + 1) * sizeof(uint32_t),
                            hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  // The row-major evaluation copy for lists that came from the host (LkLevelView::xy_eval; any permutation of a sector's
  // samples is a valid walk for the unordered sums): a stable counting sort by image row of every sector whose list
  // jumps back in y often - lists in the reference's x outer / y inner order do so once per column.  Left alone: lists
  // that are row-major already, short sectors, LK_EVAL_LISTS=0.
  {
    const bool eval_on = env_int("LK_EVAL_LISTS", 1) != 0; // test / tuning hook, read per commit
    std::vector<float> ecat[LK_MAX_LEVELS];
    bool any_sorted = false;
    std::vector<uint32_t> count;
    std::vector<float> tmp;
    auto sort_rows = [&](std::vector<float> &v, size_t b, size_t n) { // samples [b, b + n) of v: stable by (int)y
      if (n < 64)
        return false;
      int ymin = INT_MAX, ymax = INT_MIN;
      size_t back = 0;
      for (size_t k = 0; k < n; ++k) {
        const float y = v[2 * (b + k) + 1];
        if (!(y > -1e6f && y < 1e6f))
          return false; // (NaN / absurd coordinates: the solve reports them; nothing to gain here)
        const int r = (int)y;
        ymin = std::min(ymin, r), ymax = std::max(ymax, r);
        back += k > 0 && y < v[2 * (b + k) - 1];
      }
      if (back < 8 || back * 2048 < n) // (row-major already, or nearly: a column-major list jumps back once per column)
        return false;
      count.assign((size_t)(ymax - ymin) + 2, 0u);
      for (size_t k = 0; k < n; ++k)
        ++count[(size_t)((int)v[2 * (b + k) + 1] - ymin) + 1];
      for (size_t r = 1; r < count.size(); ++r)
        count[r] += count[r - 1];
      tmp.resize(2 * n);
      for (size_t k = 0; k < n; ++k) {
        const uint32_t at = count[(size_t)((int)v[2 * (b + k) + 1] - ymin)]++;
        tmp[2 * at] = v[2 * (b + k)], tmp[2 * at + 1] = v[2 * (b + k) + 1];
      }
      std::memcpy(&v[2 * b], tmp.data(), 2 * n * sizeof(float));
      return true;
    };
    if (eval_on && !cat[0].empty()) {
      for (int l : levels) {
        if (device_levels && l > 0)
          break;
        ecat[l] = cat[l];
        for (int s = 0; s < S; ++s)
          if (e->h_rect[l][(size_t)s].z == 0) {
            const size_t b = e->h_off[l][(size_t)s], n = e->h_off[l][(size_t)s + 1] - b;
            any_sorted = sort_rows(ecat[l], b, n) || any_sorted;
          }
      }
    }
    if (any_sorted) {
      for (int l : levels) {
        const bool on_device = device_levels && l > 0;
        HIPCHK(e->d_xy_eval[l].ensure((on_device ? cat[0].size() : cat[l].size()) / 2 + 1));
        if (!on_device && !ecat[l].empty())
          HIPCHK(hipMemcpy(e->d_xy_eval[l].p, ecat[l].data(), ecat[l].size() * sizeof(float), hipMemcpyHostToDevice));
      }
      if (device_levels) { // the same decimation of the copy: the same sets, the offsets already computed
        const uint32_t total = (uint32_t)(cat[0].size() / 2);
        HIPCHK(e->d_off_eval.ensure((size_t)S + 1));
        for (size_t li = 1; li < levels.size(); ++li) {
          const int l = levels[li], pl = levels[li - 1];
          HIPCHK(lk_launch_decimate(e->d_xy_eval[pl].p, e->d_off[pl].p, e->d_level_total.p + pl, total, l - pl, S, e->d_pos.p,
                                    e->d_tiles.p, e->d_xy_eval[l].p, e->d_off_eval.p, e->d_level_total.p + LK_MAX_LEVELS + l, e->stream));
        }
        HIPCHK(hipStreamSynchronize(e->stream));
      }
      e->eval_lists = true;
    }
  }
  e->lists_on_device = false;
  } // !device_roi
  HIPCHK(e->d_center.ensure((size_t)S));
  HIPCHK(hipMemcpy(e->d_center.p, e->h_center.data(), 2 * (size_t)S * sizeof(float), hipMemcpyHostToDevice));
  // Per-sector sequence state (guess history, last record, last evaluated parameters) survives a
  // commit for every sector that was not registered anew since the previous one: the reference's
  // manager registers and solves sector after sector on the first frame (resetPolygon(i), then
  // correlate(i): manager_class.cpp:340, :449) and moves them from their own records on the next
  // (updatePolygon: cuda_polygon.cu:268-415), so a commit that adds sector i must not forget 0..i-1.
  {
    const size_t old = (size_t)std::min(e->S, S);
    HIPCHK(e->d_guess.ensure_keep(6 * (size_t)S, 6 * old));
    HIPCHK(e->d_last_p.ensure_keep(6 * (size_t)S, 6 * old));
    HIPCHK(e->d_prev_p.ensure_keep(6 * (size_t)S, 6 * old));
    HIPCHK(e->d_result.ensure_keep((size_t)S, old));
    HIPCHK(e->d_stats.ensure_keep(4 * (size_t)S, 4 * old));
    HIPCHK(e->d_last_eval_p.ensure_keep(6 * (size_t)S, 6 * old));
    for (int s = 0; s < S;) { // zero the state of every run of fresh sectors
      const bool fresh = (size_t)s >= old || (!keep_state && e->hs[(size_t)s].fresh);
      int t = s + 1;
      if (fresh) {
        while (t < S && ((size_t)t >= old || (!keep_state && e->hs[(size_t)t].fresh)))
          ++t;
        const size_t n = (size_t)(t - s);
        HIPCHK(hipMemset(e->d_guess.p + 6 * (size_t)s, 0, 6 * n * sizeof(float)));
        HIPCHK(hipMemset(e->d_last_p.p + 6 * (size_t)s, 0, 6 * n * sizeof(float)));
        HIPCHK(hipMemset(e->d_prev_p.p + 6 * (size_t)s, 0, 6 * n * sizeof(float)));
        HIPCHK(hipMemset(e->d_last_eval_p.p + 6 * (size_t)s, 0, 6 * n * sizeof(float)));
        HIPCHK(hipMemset(e->d_stats.p + 4 * (size_t)s, 0, 4 * n * sizeof(uint32_t)));
        HIPCHK(hipMemset(e->d_result.p + (size_t)s, 0, n * sizeof(lk_result)));
      }
      s = t;
    }
    for (int s = 0; s < S; ++s)
      e->hs[(size_t)s].fresh = false;
  }
  e->S = S;
  {
    int rc = classify_sectors(e);
    if (rc)
      return rc;
  }
  HIPCHK(e->d_single.ensure(1));
  HIPCHK(e->d_queue.ensure(8 * kNumClasses));
  HIPCHK(hipMemset(e->d_queue.p, 0, 8 * kNumClasses * sizeof(uint32_t))); // (the SAFE pass rewinds its own queue)
  HIPCHK(e->d_handoff.ensure((size_t)S));
  HIPCHK(e->d_mid.ensure((size_t)S * kLkMidWords));
  HIPCHK(e->d_ill_list.ensure((size_t)S));
  HIPCHK(e->d_ill_count.ensure(kNumClasses)); // one list region and one counter per class: classes solve concurrently
  HIPCHK(hipMemset(e->d_ill_count.p, 0, kNumClasses * sizeof(uint32_t)));
  e->eval_cap = env_int("LK_EVAL_CAP", e->eval_cap); // tuning / test hook, read per commit
  HIPCHK(e->d_scratch.ensure(64));
  e->S = S;
  if (!keep_state) {
    e->records_S = 0;
    e->window_S = 0;
  }
  e->committed = true;
  e->lv_dirty = true;
  e->stats_valid = false;
  // may the next commit append? (plain sectors only; every per-sector buffer of this commit is S long)
  e->append_ok = !any_lazy && !e->lists_on_device;
  return LK_ERROR_NONE;
}

// lk_commit_sectors, fast path: every sector committed so far is untouched and the new ones are plain rectangles
// registered behind them - the reference's first-frame loop, resetPolygon(i) then correlate(i), sector after
// sector (manager_class.cpp:304-460).  Appending costs O(levels) host work, amortised buffer growth and ONE small
// launch that writes the sector's rectangles, offsets, centre and zeroed sequence state (the values travel in the
// kernel arguments: no staging, no synchronisation); the full commit would rebuild and re-upload all S sectors,
// O(S^2) over the loop.
static const int kMaxAppend = 64; // more new sectors than this: the full commit is cheaper
static bool can_append(const lk_engine *e) {
  const int S0 = e->S, S1 = (int)e->hs.size();
  if (!e->append_ok || S0 <= 0 || S1 <= S0 || S1 - S0 > kMaxAppend || e->recommit_pending || e->lists_on_device ||
      e->backup_on_device || !e->hs_backup.empty())
    return false;
  for (int s = S0; s < S1; ++s) {
    const HostSector &h = e->hs[(size_t)s];
    if (!h.set || !h.is_rect || h.lazy != 0 || size_class(h.n0()) >= kTeamClass - 1)
      return false;
  }
  return true;
}
static int append_rect_sectors(lk_engine *e) {
  Range range_("lk:append sectors");
  const int S0 = e->S, S1 = (int)e->hs.size();
  HIPCHK(hipSetDevice(e->cfg.device));
  const lk_config &cfg = e->cfg;
  const std::vector<int> levels = list_levels(cfg);
  // room for the new sectors (geometric growth; the committed part is kept)
  const size_t keep = (size_t)S0, want = (size_t)S1;
  {
    // A growth step reallocates: hipMalloc, a copy on the NULL stream, hipFree - none of which waits for the engine's
    // (non-blocking) stream.  Append kernels, in-place patches or an unsynchronised solve (lk_correlate_all_device /
    // _async) still queued there would write the old buffer behind the copy, and the hipFree would drop what they wrote.
    // So the stream is drained first - only on the geometric growth steps, the O(1) path of the other commits is untouched.
    bool grows = e->d_center.n < want || e->d_guess.n < 6 * want || e->d_last_p.n < 6 * want || e->d_prev_p.n < 6 * want ||
                 e->d_last_eval_p.n < 6 * want || e->d_result.n < want || e->d_stats.n < 4 * want || e->d_handoff.n < want ||
                 e->d_mid.n < want * kLkMidWords || e->d_ill_list.n < want || e->d_order.n < want || e->d_finish_list.n < want;
    for (int l : levels)
      grows = grows || e->d_rect[l].n < want || e->d_off[l].n < want + 1;
    if (grows)
      HIPCHK(hipStreamSynchronize(e->stream));
  }
  // (a failure from here on leaves the host tables as they were and sends the next commit through the full rebuild)
  const size_t rect0 = e->h_rect[0].size();
  auto undo = [&, rect0]() {
    for (int l : levels) {
      if (e->h_rect[l].size() > rect0)
        e->h_rect[l].resize(rect0);
      if (e->h_off[l].size() > rect0 + 1)
        e->h_off[l].resize(rect0 + 1);
    }
    e->h_center.resize(2 * keep);
    e->h_class.resize(keep);
    e->append_ok = false;
  };
  struct Guard {
    std::function<void()> f;
    bool armed = true;
    ~Guard() {
      if (armed)
        f();
    }
  } guard{undo};
  HIPCHK(e->d_center.reserve_keep(want, keep));
  HIPCHK(e->d_guess.reserve_keep(6 * want, 6 * keep));
  HIPCHK(e->d_last_p.reserve_keep(6 * want, 6 * keep));
  HIPCHK(e->d_prev_p.reserve_keep(6 * want, 6 * keep));
  HIPCHK(e->d_last_eval_p.reserve_keep(6 * want, 6 * keep));
  HIPCHK(e->d_result.reserve_keep(want, keep));
  HIPCHK(e->d_stats.reserve_keep(4 * want, 4 * keep));
  for (int l : levels) {
    HIPCHK(e->d_rect[l].reserve_keep(want, keep));
    HIPCHK(e->d_off[l].reserve_keep(want + 1, keep + 1));
  }
  // (scratch of the solve: contents do not survive a solve)
  if (e->d_handoff.n < want)
    HIPCHK(e->d_handoff.ensure(2 * want + 64));
  if (e->d_mid.n < want * kLkMidWords)
    HIPCHK(e->d_mid.ensure((2 * want + 64) * kLkMidWords));
  if (e->d_ill_list.n < want)
    HIPCHK(e->d_ill_list.ensure(2 * want + 64));
  if (e->d_order.n < want)
    HIPCHK(e->d_order.ensure(2 * want + 64));
  e->h_center.resize(2 * want);
  e->h_class.resize(want, 0);
  bool any_starved = false;
  for (int s = S0; s < S1; ++s) {
    HostSector &hs = e->hs[(size_t)s];
    e->h_center[2 * (size_t)s] = hs.cx;
    e->h_center[2 * (size_t)s + 1] = hs.cy;
    LkAppendArgs a{};
    a.sector = s;
    a.center = make_float2(hs.cx, hs.cy);
    a.d_center = e->d_center.p;
    a.d_guess = e->d_guess.p, a.d_last_p = e->d_last_p.p, a.d_prev_p = e->d_prev_p.p, a.d_last_eval_p = e->d_last_eval_p.p;
    a.d_result = e->d_result.p;
    a.d_stats = e->d_stats.p;
    a.n_levels = (int)levels.size();
    for (size_t li = 0; li < levels.size(); ++li) {
      const int l = levels[li];
      const int4 rc = hs.rect_at(l);
      e->h_rect[l].push_back(rc);
      e->h_off[l].push_back(e->h_off[l].back()); // (a rectangle has no list entries)
      a.rect[li] = rc;
      a.off_end[li] = e->h_off[l].back();
      a.d_rect[li] = e->d_rect[l].p;
      a.d_off[li] = e->d_off[l].p;
    }
    const int c = size_class(hs.n0()); // (promotions are a property of the whole batch: classify_sectors)
    e->h_class[(size_t)s] = c;
    const int4 top = e->h_rect[cfg.py_stop][(size_t)s];
    if (top.w <= starved_max(e))
      e->class_starved[c] = any_starved = true;
    HIPCHK(lk_launch_append_sector(a, e->stream));
    hs.fresh = false;
  }
  if (any_starved) {
    if (e->d_finish_list.n < want)
      HIPCHK(e->d_finish_list.ensure(2 * want + 64));
    HIPCHK(e->d_finish_count.ensure(kNumClasses));
  }
  guard.armed = false;
  e->S = S1;
  e->committed = true;
  e->classes_dirty = true; // the batch's size-class analysis and launch order: redone by the next batch solve
  e->lv_dirty = true;
  e->stats_valid = false;
  return LK_ERROR_NONE;
}

// lk_update_sector moved sample lists: they (and the centres) are rebuilt before anything walks them
int recommit_if_pending(lk_engine *e) {
  if (!e->recommit_pending)
    return LK_ERROR_NONE;
  e->recommit_pending = false;
  return commit_impl(e, true);
}

// sectors were appended since the last analysis of the whole domain
int reclassify_if_dirty(lk_engine *e) {
  if (!e->classes_dirty)
    return LK_ERROR_NONE;
  HIPCHK(hipStreamSynchronize(e->stream)); // (earlier launches may still read the order table)
  return classify_sectors(e);
}

int lk_commit_sectors(lk_engine *e) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  int rc = materialize_host(e);
  if (rc)
    return rc;
  if (can_append(e))
    return append_rect_sectors(e);
  return commit_impl(e, false);
}
