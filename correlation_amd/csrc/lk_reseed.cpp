// lk_reseed.cpp - host side of the recovery pass (include/lk_engine.h: lk_reseed_failed, lk_get_reseed_info,
// lk_reseed_plan).  The kernels are lk_reseed.hip; the retries are solved by the engine's own launch code
// (lk_internal_solve_set -> launch_all) on a sector set this file compacts on the device.  Also the test hook that shows the
// cell grid every neighbour pass shares (lk_internal.hpp: lk_internal_cell_grid).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"

namespace {

using Buf = LkDevBytes;

// the words that travel to the host once per round (and the bounding box once per call)
struct Words {
  uint32_t count[kLkReseedRanges]; // sectors to retry per class / backward lane-group range
  uint32_t n_failed;               // failed sectors the call found
  uint32_t pad[2];
  unsigned long long totals[6];    // retry solves, their four counters, sectors recovered
  float bbox[4];
};

struct ReseedState : LkPassSlot {
  Buf good, tried, nbrs, retry, guess, info, plan_info, fresh, keep_last_p, keep_last_eval_p, keep_stats, retry_order,
      bw_retry_order, words;
  LkCellGridBufs grid;
  Words *h_words = nullptr; // pinned
  int info_S = 0;           // sectors `info` describes (0: no lk_reseed_failed yet)
  hipError_t init() { return hipHostMalloc((void **)&h_words, sizeof(Words), hipHostMallocDefault); }
  ~ReseedState() override {
    if (h_words)
      (void)hipHostFree(h_words);
  }
};

int n_params_of(int model) { return model == LK_FM_U ? 1 : model == LK_FM_UV ? 2 : model == LK_FM_UVQ ? 3 : 6; }

int check_config(lk_engine *e, const lk_reseed_config *cfg, const char *who, bool with_rounds) {
  const std::string w(who);
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (w + ": no configuration").c_str());
  if (!std::isfinite(cfg->radius) || !(cfg->radius > 0.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (w + ": radius must be finite and positive").c_str());
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (w + ": chi_max must be finite (<= 0: the error code alone decides)").c_str());
  if (cfg->min_neighbours < 1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (w + ": min_neighbours must be at least 1").c_str());
  if (with_rounds && (cfg->max_rounds < 1 || cfg->max_rounds > 64))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (w + ": max_rounds must be in 1 .. 64").c_str());
  return LK_ERROR_NONE;
}

int ensure_common(lk_engine *e, ReseedState *st, int S) {
  const size_t n = (size_t)S;
  LK_HIPCHK(st->good.ensure(n));
  LK_HIPCHK(st->tried.ensure(n * sizeof(int32_t)));
  LK_HIPCHK(st->nbrs.ensure(n * sizeof(int32_t)));
  LK_HIPCHK(st->retry.ensure(n));
  LK_HIPCHK(st->guess.ensure(n * 6 * sizeof(float)));
  LK_HIPCHK(st->fresh.ensure(n * sizeof(lk_result)));
  LK_HIPCHK(st->words.ensure(sizeof(Words)));
  return LK_ERROR_NONE;
}

// the cell grid over the centres (lk_cell_grid.hpp: cell size = radius, table capped at a few words per sector)
int build_grid(lk_engine *e, ReseedState *st, const LkReseedView &v, float radius, const float bbox[4], LkReseedGrid *g) {
  if (!lk_cell_grid_bbox_finite(bbox))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_reseed: a sector centre is not finite");
  LK_HIPCHK(lk_cell_grid_build(st->grid, v.center, v.S, radius, bbox, v.stream, g));
  return LK_ERROR_NONE;
}

int fetch_words(lk_engine *e, ReseedState *st, hipStream_t stream) {
  LK_HIPCHK(hipMemcpyAsync(st->h_words, st->words.p, sizeof(Words), hipMemcpyDeviceToHost, stream));
  LK_HIPCHK(hipStreamSynchronize(stream));
  return LK_ERROR_NONE;
}

LkReseedPlanArgs plan_args(ReseedState *st, const LkReseedView &v, const LkReseedGrid &g, const lk_reseed_config *cfg,
                           const lk_result *rec) {
  LkReseedPlanArgs a{};
  a.grid = g;
  a.center = v.center;
  a.rec = rec;
  a.good = st->good.as<uint8_t>();
  a.tried = st->tried.as<int32_t>();
  a.guess = st->guess.as<float>();
  a.nbrs = st->nbrs.as<int32_t>();
  a.retry = st->retry.as<uint8_t>();
  a.plan_info = nullptr;
  a.n_sectors = v.S;
  a.model = v.model;
  a.min_neighbours = cfg->min_neighbours;
  a.radius = (double)cfg->radius;
  return a;
}

} // namespace

extern "C" {

int lk_reseed_failed(lk_engine *e, const lk_reseed_config *cfg, lk_result *out, int *n_recovered) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (n_recovered)
    *n_recovered = 0;
  if (int rc = check_config(e, cfg, "lk_reseed_failed", true))
    return rc;
  LkReseedView v{};
  if (int rc = lk_internal_reseed_view(e, 1, "lk_reseed_failed", &v))
    return rc;
  ReseedState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_RESEED, "hipHostMalloc (lk_reseed)", &st))
    return rc;
  st->info_S = 0;
  const int S = v.S, P = n_params_of(v.model);
  const size_t n = (size_t)S;
  if (int rc = ensure_common(e, st, S))
    return rc;
  LK_HIPCHK(st->info.ensure(n * sizeof(lk_reseed_info)));
  LK_HIPCHK(st->keep_last_p.ensure(n * 6 * sizeof(float)));
  LK_HIPCHK(st->keep_last_eval_p.ensure(n * 6 * sizeof(float)));
  LK_HIPCHK(st->keep_stats.ensure(n * 4 * sizeof(uint32_t)));
  LK_HIPCHK(st->retry_order.ensure(n * sizeof(uint32_t)));
  LK_HIPCHK(st->bw_retry_order.ensure(n * sizeof(uint32_t)));
  Words *d_words = st->words.as<Words>();

  // classify, and the centres' bounding box: the one round trip before the rounds
  LK_HIPCHK(hipMemsetAsync(d_words, 0, sizeof(Words), v.stream));
  LK_HIPCHK(lk_launch_reseed_classify(v.result, S, P, cfg->chi_max, st->good.as<uint8_t>(), st->tried.as<int32_t>(),
                                  st->info.as<lk_reseed_info>(), &d_words->n_failed, v.stream));
  LK_HIPCHK(lk_launch_reseed_bbox(v.center, S, d_words->bbox, v.stream));
  if (int rc = fetch_words(e, st, v.stream))
    return rc;
  st->info_S = S;
  if (st->h_words->n_failed > 0) {
    LkReseedGrid grid{};
    if (int rc = build_grid(e, st, v, cfg->radius, st->h_words->bbox, &grid))
      return rc;
    // everything a solve writes per sector besides its record: kept, and put back for a retry that is rejected
    LK_HIPCHK(hipMemcpyAsync(st->keep_last_p.p, v.last_p, n * 6 * sizeof(float), hipMemcpyDeviceToDevice, v.stream));
    LK_HIPCHK(hipMemcpyAsync(st->keep_last_eval_p.p, v.last_eval_p, n * 6 * sizeof(float), hipMemcpyDeviceToDevice, v.stream));
    LK_HIPCHK(hipMemcpyAsync(st->keep_stats.p, v.stats, n * 4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, v.stream));

    LkReseedCompactArgs ca{};
    ca.retry = st->retry.as<uint8_t>();
    ca.count = d_words->count;
    if (v.backward) {
      for (int g = 0; g < 3; ++g)
        ca.range[6 + g] = LkReseedRange{v.bw_order, st->bw_retry_order.as<uint32_t>(), v.bw_begin[g], v.bw_begin[g + 1]};
    } else {
      for (int c = 0; c < 6; ++c)
        ca.range[c] = LkReseedRange{v.order, st->retry_order.as<uint32_t>(), v.class_begin[c], v.class_begin[c + 1]};
    }
    LkReseedMergeArgs ma{};
    ma.retry = st->retry.as<uint8_t>();
    ma.good = st->good.as<uint8_t>();
    ma.tried = st->tried.as<int32_t>();
    ma.nbrs = st->nbrs.as<int32_t>();
    ma.fresh = st->fresh.as<lk_result>();
    ma.rec = v.result;
    ma.last_p = v.last_p;
    ma.last_eval_p = v.last_eval_p;
    ma.keep_last_p = st->keep_last_p.as<float>();
    ma.keep_last_eval_p = st->keep_last_eval_p.as<float>();
    ma.stats = v.stats;
    ma.keep_stats = st->keep_stats.as<uint32_t>();
    ma.info = st->info.as<lk_reseed_info>();
    ma.totals = d_words->totals;
    ma.n_sectors = S;
    ma.n_params = P;
    ma.chi_max = cfg->chi_max;
    const LkReseedPlanArgs pa = plan_args(st, v, grid, cfg, v.result);

    for (int round = 0; round < cfg->max_rounds; ++round) {
      LK_HIPCHK(lk_launch_reseed_plan(pa, v.stream));
      LK_HIPCHK(lk_launch_reseed_compact(ca, v.stream));
      if (int rc = fetch_words(e, st, v.stream)) // the round's one trip to the host: the counts that size the launches
        return rc;
      LkSectorSet set{};
      set.order = st->retry_order.as<uint32_t>();
      set.bw_order = st->bw_retry_order.as<uint32_t>();
      long long total = 0;
      for (int c = 0; c < 6; ++c)
        total += set.count[c] = v.backward ? 0 : (int)st->h_words->count[c];
      for (int g = 0; g < 3; ++g)
        total += set.bw_count[g] = v.backward ? (int)st->h_words->count[6 + g] : 0;
      if (total == 0) // nothing new to try: the last round recovered nothing that is anybody's neighbour
        break;
      if (int rc = lk_internal_solve_set(e, &set, st->guess.as<float>(), st->fresh.as<lk_result>()))
        return rc;
      ma.round = round;
      LK_HIPCHK(lk_launch_reseed_merge(ma, v.stream));
    }
    if (int rc = fetch_words(e, st, v.stream))
      return rc;
  }
  unsigned long long totals[5];
  for (int i = 0; i < 5; ++i)
    totals[i] = st->h_words->totals[i];
  lk_internal_reseed_stats(e, totals);
  if (n_recovered)
    *n_recovered = (int)st->h_words->totals[5];
  if (out) {
    LK_HIPCHK(hipMemcpyAsync(out, v.result, n * sizeof(lk_result), hipMemcpyDeviceToHost, v.stream));
    LK_HIPCHK(hipStreamSynchronize(v.stream));
  }
  return LK_ERROR_NONE;
}

int lk_get_reseed_info(lk_engine *e, lk_reseed_info *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  ReseedState *st = static_cast<ReseedState *>(*lk_internal_pass_slot(e, LK_PASS_RESEED));
  if (!out || !st || st->info_S <= 0 || st->info_S != lk_internal_sector_count(e))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_get_reseed_info: no lk_reseed_failed of the committed sectors");
  LK_HIPCHK(hipMemcpy(out, st->info.p, (size_t)st->info_S * sizeof(lk_reseed_info), hipMemcpyDeviceToHost));
  return LK_ERROR_NONE;
}

int lk_reseed_plan(lk_engine *e, const lk_reseed_config *cfg, const lk_result *records, float *guesses_out,
                   lk_reseed_info *info_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (int rc = check_config(e, cfg, "lk_reseed_plan", false))
    return rc;
  if (!records || !guesses_out || !info_out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_reseed_plan: null argument");
  LkReseedView v{};
  if (int rc = lk_internal_reseed_view(e, 0, "lk_reseed_plan", &v))
    return rc;
  ReseedState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_RESEED, "hipHostMalloc (lk_reseed)", &st))
    return rc;
  const int S = v.S, P = n_params_of(v.model);
  const size_t n = (size_t)S;
  if (int rc = ensure_common(e, st, S))
    return rc;
  LK_HIPCHK(st->plan_info.ensure(n * sizeof(lk_reseed_info)));
  Words *d_words = st->words.as<Words>();
  LK_HIPCHK(hipMemsetAsync(d_words, 0, sizeof(Words), v.stream));
  LK_HIPCHK(hipMemcpyAsync(st->fresh.p, records, n * sizeof(lk_result), hipMemcpyHostToDevice, v.stream));
  LK_HIPCHK(hipMemsetAsync(st->guess.p, 0, n * 6 * sizeof(float), v.stream));
  LK_HIPCHK(lk_launch_reseed_classify(st->fresh.as<lk_result>(), S, P, cfg->chi_max, st->good.as<uint8_t>(),
                                  st->tried.as<int32_t>(), st->plan_info.as<lk_reseed_info>(), &d_words->n_failed, v.stream));
  LK_HIPCHK(lk_launch_reseed_bbox(v.center, S, d_words->bbox, v.stream));
  if (int rc = fetch_words(e, st, v.stream))
    return rc;
  LkReseedGrid grid{};
  if (int rc = build_grid(e, st, v, cfg->radius, st->h_words->bbox, &grid))
    return rc;
  LkReseedPlanArgs pa = plan_args(st, v, grid, cfg, st->fresh.as<lk_result>());
  pa.plan_info = st->plan_info.as<lk_reseed_info>();
  LK_HIPCHK(lk_launch_reseed_plan(pa, v.stream));
  LK_HIPCHK(hipMemcpyAsync(guesses_out, st->guess.p, n * 6 * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipMemcpyAsync(info_out, st->plan_info.p, n * sizeof(lk_reseed_info), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  return LK_ERROR_NONE;
}

// test hook (lk_internal.hpp): the grid every neighbour pass would build, in buffers of its own that go with the call
int lk_internal_cell_grid(lk_engine *e, float radius, int *nx, int *ny, double *cell, double *x0, double *y0, uint32_t *cell_of,
                          uint32_t *start, size_t start_capacity, uint32_t *members) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!std::isfinite(radius) || !(radius > 0.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_internal_cell_grid: radius must be finite and positive");
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_internal_cell_grid", 0, -1, &v))
    return rc;
  LkPassState st;
  LkDevBytes bbox;
  LkCellGridBufs bufs;
  LK_HIPCHK(st.init());
  LK_HIPCHK(bbox.ensure(4 * sizeof(float)));
  LkReseedGrid g{};
  if (int rc = lk_pass_grid(e, "lk_internal_cell_grid", &st, bbox, bufs, v.center, v.S, radius, v.stream, &g))
    return rc;
  const size_t n = (size_t)v.S, n_cells = (size_t)g.nx * (size_t)g.ny;
  if (start && start_capacity < n_cells + 1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_internal_cell_grid: start holds fewer than nx ny + 1 words");
  if (cell_of)
    LK_HIPCHK(hipMemcpyAsync(cell_of, g.cell_of, n * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
  if (start)
    LK_HIPCHK(hipMemcpyAsync(start, g.start, (n_cells + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
  if (members)
    LK_HIPCHK(hipMemcpyAsync(members, g.members, n * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream)); // (the buffers are freed on return)
  if (nx)
    *nx = g.nx;
  if (ny)
    *ny = g.ny;
  if (cell)
    *cell = g.cell;
  if (x0)
    *x0 = g.x0;
  if (y0)
    *y0 = g.y0;
  return LK_ERROR_NONE;
}

} // extern "C"
