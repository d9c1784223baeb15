// lk_engine_solve.cpp - the solve of the engine: the level table, the launches of one pair (per size class, starved levels,
// teams, reference order, backward update), lk_correlate_all* / lk_correlate, the guess calls and the stand-alone
// diagnostic entry points.  The helpers that lk_engine_sequence.cpp shares (class fork and join, solve bracket,
// reference-order group rule) are defined here, once.
#include "lk_engine_state.hpp"

int refresh_level_views(lk_engine *e) {
  if (!e->committed)
    return e->fail(LK_ERROR_BAD_DOMAIN, "sectors are not committed (call lk_commit_sectors)");
  if (int rc = recommit_if_pending(e))
    return rc;
  const DevImage &u = e->img[LK_IMG_UND], &d = e->img[LK_IMG_DEF];
  if (!u.valid || !d.valid)
    return e->fail(LK_ERROR_BAD_DOMAIN, "undeformed and deformed images must be set before correlating");
  if (!e->lv_dirty)
    return LK_ERROR_NONE;
  // every level-0 sample must lie inside the undeformed image
  for (int l = 0; l < LK_MAX_LEVELS; ++l) {
    LkLevelView &v = e->h_lv[l];
    std::memset(&v, 0, sizeof(v));
    if (l > e->cfg.py_stop)
      continue;
    v.und = u.lvl[l];
    v.def = d.lvl[l];
    v.xy = e->d_xy[l].p;
    // (batch-invariant mode: a sector's arithmetic must not depend on HOW its list was built - device masks and moved
    // lists have the row-major copy, lists that came from the host do not - so every path walks the reference's order)
    v.xy_eval = e->eval_lists && !e->batch_invariant ? e->d_xy_eval[l].p : nullptr;
    v.off = e->d_off[l].p;
    v.rect = e->d_rect[l].p;
    v.urows = u.rows >> l;
    v.ucols = u.cols >> l;
    v.drows = d.rows >> l;
    v.dcols = d.cols >> l;
  }
  // Same buffers and geometry as the last launch (a frame loop that reuses its slots): nothing
  // to do.  Otherwise the table travels in the kernel arguments of a one-wavefront kernel:
  // stream-ordered, no staging buffer, no host synchronisation between the frames.
  if (!e->d_lv.p || std::memcmp(e->h_lv, e->h_lv_sent, sizeof(e->h_lv)) != 0) {
    HIPCHK(e->d_lv.ensure(LK_MAX_LEVELS));
    HIPCHK(lk_launch_set_views(e->h_lv, e->d_lv.p, e->stream));
    std::memcpy(e->h_lv_sent, e->h_lv, sizeof(e->h_lv));
  }
  e->lv_dirty = false;
  return LK_ERROR_NONE;
}

// Which flavour of the lane-group kernels a solve uses.  The fast flavour hands a sector whose damped system met a bad pivot
// to a second, SAFE pass; the SAFE flavour runs the reference's QR for such a system inside the kernel.  Batch-invariant mode
// takes the SAFE flavour throughout: a sector's arithmetic then is ONE kernel's from its guess to its record, whatever else
// is in the batch and whoever solves it - in particular the frame-pipelined instances (which have no second pass to hand a
// sector to) produce the very same bytes as the one-pair launches.
bool safe_flavour(const lk_engine *e) { return e->force_safe || e->batch_invariant; }

LkSolveArgs base_args(lk_engine *e, const float *d_guess, lk_result *d_result) {
  LkSolveArgs a{};
  a.lv = e->d_lv.p;
  a.center = e->d_center.p;
  a.guess = d_guess;
  a.result = d_result;
  a.last_p = e->d_last_p.p;
  a.last_eval_p = e->d_last_eval_p.p;
  a.stats = e->d_stats.p;
  a.py_start = e->cfg.py_start;
  a.py_step = e->cfg.py_step;
  a.py_stop = e->cfg.py_stop;
  a.precision = e->cfg.precision;
  a.max_iters = e->cfg.max_iters;
  a.solo = e->batch_invariant ? 0 : 1;
  a.gpu_share = e->pairs_in_flight;
  static const int align = env_int("LK_ALIGN", 1); // tuning hook, read once; alignment never changes a record's bits
  a.align = align;
  a.keep_sums = env_int("LK_KEEP_SUMS", 1) != 0 ? 1 : 0;  // test hook, read per call
  a.slot_step = env_int("LK_STEP_STATE", 1) == 0 ? 1 : 0; // test hook, read per call (tests/test_step_state_gpu.py)
  a.starved_max = starved_max(e);
  return a;
}

// Starved levels: the one-lane-per-sector kernel (bit-identical sums and QR), whose lanes park
// a sector after eval_cap evaluations, then the 16-lane finisher for the parked ones.  Both
// leave an LkHandoff record per sector for the lane-group kernel that follows.
// `c` picks the class's own region of the parked-sector lists and its own counters (classes
// solve concurrently), `first` is where the class starts in d_order, `st` its stream.
static int launch_starved(lk_engine *e, LkSolveArgs &a, int c, int first, hipStream_t st) {
  a.handoff = e->d_handoff.p;
  a.eval_cap = e->eval_cap > 0 ? e->eval_cap : 0;
  a.mid_state = e->d_mid.p;
  a.finish_list = e->d_finish_list.p + first;
  a.finish_count = e->d_finish_count.p + c;
  if (a.eval_cap > 0)
    HIPCHK(hipMemsetAsync(a.finish_count, 0, sizeof(uint32_t), st));
  HIPCHK(lk_launch_solve(a, e->cfg.fitting_model, e->cfg.interpolation, 1, st, e->launch_report_slot()));
  if (a.eval_cap > 0) {
    LkSolveArgs f = a;
    f.finisher = 1;
    f.safe = 1;
    f.align = 0; // one trip per evaluation whatever the level: rows take the next parked sector as they finish
    HIPCHK(lk_launch_solve(f, e->cfg.fitting_model, e->cfg.interpolation, 16, st, e->launch_report_slot()));
  }
  a.eval_cap = 0;
  return LK_ERROR_NONE;
}

// The lane-group kernel of one class, then the SAFE 16-lane kernel for the sectors it parked
// because a damped system met a bad pivot (the reference's rank-revealing QR decides those
// steps; on textured images the list is empty and the second launch retires at once).
static int launch_groups(lk_engine *e, LkSolveArgs &a, int group, int c, int first, hipStream_t st) {
  static const bool ill_env = env_int("LK_ILL_PASS", 1) != 0; // (read once)
  const bool with_ill_pass = !a.safe && ill_env;
  if (with_ill_pass) {
    a.mid_state = e->d_mid.p;
    a.ill_list = e->d_ill_list.p + first;
    a.ill_count = e->d_ill_count.p + c; // (rewound by the SAFE pass itself)
  }
  HIPCHK(lk_launch_solve(a, e->cfg.fitting_model, e->cfg.interpolation, group, st, e->launch_report_slot()));
  if (with_ill_pass) {
    LkSolveArgs r = a;
    r.resume = 1;
    r.safe = 1;
    r.ill_list = nullptr;
    r.ill_count = nullptr;
    r.finish_list = a.ill_list;
    r.finish_count = a.ill_count;
    r.team_w = 0;
    r.handoff = nullptr;
    r.queue = a.queue + 3;
    HIPCHK(lk_launch_solve(r, e->cfg.fitting_model, e->cfg.interpolation, 16, st, e->launch_report_slot()));
  }
  return LK_ERROR_NONE;
}

// LK_TEAM_FAULT=step (tests, read per call): a team workgroup goes missing -> the lone-workgroup fallback
static int team_fault_hook() { return env_int("LK_TEAM_FAULT", 0); }

// Team workgroups wait for each other, so two team launches that are both only partly resident
// would wait forever.  One engine never has two in flight; engines of one process take turns:
// every team launch waits for the previous one on the same device (whoever issued it).
// A turn is taken on the stream of the launch, before it; done() records the device's event behind the launch and
// ends the turn, an early return ends it without a record.
namespace {
class TeamTurn {
  std::unique_lock<std::mutex> lock_;
  hipEvent_t *done_ = nullptr;

public:
  int take(lk_engine *e, hipStream_t st) {
    static std::mutex g_team_mu;
    static hipEvent_t g_team_done[64] = {};
    if (e->cfg.device < 0 || e->cfg.device >= 64)
      return LK_ERROR_NONE;
    lock_ = std::unique_lock<std::mutex>(g_team_mu);
    done_ = &g_team_done[e->cfg.device];
    if (!*done_)
      HIPCHK(hipEventCreateWithFlags(done_, hipEventDisableTiming));
    else
      HIPCHK(hipStreamWaitEvent(st, *done_, 0));
    return LK_ERROR_NONE;
  }
  int done(lk_engine *e, hipStream_t st) {
    std::unique_lock<std::mutex> turn = std::move(lock_); // (released on every path out of here)
    if (done_)
      HIPCHK(hipEventRecord(*done_, st));
    return LK_ERROR_NONE;
  }
};
} // namespace

// Size classes are independent sector sets (own lists, counters and queue words): the first one solves on the engine's
// stream, every further one on a stream of its own forked from it and joined back, so that the tail of one class overlaps
// the others (config 3: 256 annular sectors + the blob's team).  open() marks the point of the engine's stream where
// guesses, views and images are ready; streams and events are created when a class first needs them.
int ClassFork::open() {
  if (!on)
    return LK_ERROR_NONE;
  if (!e->ev_fork)
    HIPCHK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
  HIPCHK(hipEventRecord(e->ev_fork, e->stream));
  return LK_ERROR_NONE;
}
int ClassFork::stream_of(int c, hipStream_t *st) {
  *st = e->stream;
  if (!on || n_launched == 0)
    return LK_ERROR_NONE;
  if (!e->class_stream[c]) {
    HIPCHK(hipStreamCreateWithFlags(&e->class_stream[c], hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&e->ev_join[c], hipEventDisableTiming));
  }
  *st = e->class_stream[c];
  HIPCHK(hipStreamWaitEvent(*st, e->ev_fork, 0));
  return LK_ERROR_NONE;
}
int ClassFork::join(int c, hipStream_t st) {
  if (st != e->stream) {
    HIPCHK(hipEventRecord(e->ev_join[c], st));
    HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join[c], 0));
  }
  ++n_launched;
  return LK_ERROR_NONE;
}

// What brackets every solve: the timing events on the engine's stream and, behind it, what lk_get_stats needs to know
// about the counters - how many frames they cover and which update wrote them.  The launch report starts over with it.
int solve_begin(lk_engine *e) {
  e->launch_report_begin(); // (lk_get_launch_report describes the call that starts here)
  if (e->timing)
    HIPCHK(hipEventRecord(e->ev_s0, e->stream));
  return LK_ERROR_NONE;
}
int solve_end(lk_engine *e, int stats_frames, int stats_update) {
  if (e->timing) {
    HIPCHK(hipEventRecord(e->ev_s1, e->stream));
    e->solve_timed = true;
  }
  e->stats_valid = false;
  e->stats_frames = stats_frames;
  e->stats_update = stats_update;
  return LK_ERROR_NONE;
}

// Reference-order mode, a batch: a 16-lane row per small sector, a wavefront per larger one, a 512-thread workgroup per
// sector of the two big classes - and of the class below them while its `n` sectors are no more than the CUs: a workgroup
// per sector then shortens every sector's chain, beyond that the wavefronts' throughput wins.
int reference_group_of_class(int c, int n) {
  return c == 0 ? 16 : (c >= kTeamClass - 1 || (c == kTeamClass - 2 && n <= 256)) ? 512 : 64;
}
// number_of_threads = T > 1 on the `n` sectors of one of the two big classes: the team width T the batch asks for (0: none)
static int reference_team_of_class(const lk_engine *e, int c, int n) {
  const int T = e->reference_order;
  return c >= kTeamClass - 1 && T > 1 && T <= kLkMaxTeam && (long long)n * T <= 256 && !e->batch_invariant ? T : 0;
}
// ... and a single sector (lk_correlate, lk_evaluate).  NOT the batch rule, and not to be merged with it: a lone sector
// never gets a workgroup or a team, whatever its class.
static int reference_group_of_sector(const lk_engine *e, int sector) { return e->h_class[(size_t)sector] == 0 ? 16 : 64; }

// reference-order mode: records whose first evaluation failed report the iteration count the
// previously solved sector left behind (lk_stale_iterations_kernel)
int stale_iterations(lk_engine *e, lk_result *d_result, int n) {
  if (!e->d_stale.p) {
    HIPCHK(e->d_stale.ensure(2));
    HIPCHK(hipMemsetAsync(e->d_stale.p, 0, 2 * sizeof(int), e->stream));
  }
  HIPCHK(lk_launch_stale_iterations(d_result, n, e->d_stale.p + e->stale_par, e->d_stale.p + (e->stale_par ^ 1), e->stream));
  e->stale_par ^= 1;
  return LK_ERROR_NONE;
}

// Backward mode: the sectors by lane group (from each sector's level-0 count alone) and the template slots.
static const int kBwGroups[3] = {16, 64, 512};
int bw_tables(lk_engine *e) {
  if (!e->bw_dirty && e->h_bw_base.size() == (size_t)e->S)
    return LK_ERROR_NONE;
  const int S = e->S;
  e->h_bw_order.clear();
  e->h_bw_base.assign((size_t)S, 0u);
  size_t total = 0;
  for (int s = 0; s < S; ++s) {
    e->h_bw_base[(size_t)s] = (uint32_t)total;
    total += (size_t)level0_count(e, s);
  }
  if (total > 0xffffffffull)
    return e->fail(LK_ERROR_BAD_DOMAIN, "backward update: more than 2^32 level-0 samples");
  for (int g = 0; g < 3; ++g) {
    e->bw_begin[g] = (int)e->h_bw_order.size();
    for (int s = 0; s < S; ++s)
      if (lk_bw_group(level0_count(e, s)) == kBwGroups[g])
        e->h_bw_order.push_back((uint32_t)s);
  }
  e->bw_begin[3] = (int)e->h_bw_order.size();
  HIPCHK(hipStreamSynchronize(e->stream)); // (earlier launches may still read the tables)
  HIPCHK(e->d_bw_order.ensure((size_t)S));
  HIPCHK(e->d_bw_base.ensure((size_t)S));
  HIPCHK(e->d_bw_tpl.ensure(total));
  HIPCHK(hipMemcpy(e->d_bw_order.p, e->h_bw_order.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->d_bw_base.p, e->h_bw_base.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice));
  e->bw_dirty = false;
  return LK_ERROR_NONE;
}

static LkBackwardArgs bw_args(lk_engine *e, const float *d_guess, lk_result *d_result) {
  LkBackwardArgs b{};
  b.lv = e->d_lv.p;
  b.center = e->d_center.p;
  b.guess = d_guess;
  b.result = d_result;
  b.last_p = e->d_last_p.p;
  b.last_eval_p = e->d_last_eval_p.p;
  b.stats = e->d_stats.p;
  b.tpl = e->d_bw_tpl.p;
  b.tpl_base = e->d_bw_base.p;
  b.py_start = e->cfg.py_start;
  b.py_step = e->cfg.py_step;
  b.py_stop = e->cfg.py_stop;
  b.precision = e->cfg.precision;
  b.max_iters = e->cfg.max_iters;
  b.starved_max = starved_max(e);
  return b;
}

// the sectors of `set` (nullptr: every sector of the domain - the engine's own table, bw_begin differences) with the
// backward update: one launch per lane group, on the engine's stream
static int launch_all_backward(lk_engine *e, const float *d_guess, lk_result *d_result, const LkSectorSet *set = nullptr) {
  if (int rc = bw_tables(e))
    return rc;
  Range range_("lk:solve backward");
  if (int rc = solve_begin(e))
    return rc;
  LkBackwardArgs b = bw_args(e, d_guess, d_result);
  for (int g = 0; g < 3; ++g) {
    b.order = (set ? set->bw_order : e->d_bw_order.p) + e->bw_begin[g];
    b.n_sectors = set ? set->bw_count[g] : e->bw_begin[g + 1] - e->bw_begin[g];
    if (b.n_sectors > 0)
      HIPCHK(lk_launch_backward(b, e->cfg.fitting_model, e->cfg.interpolation, kBwGroups[g], e->stream, e->launch_report_slot()));
  }
  return solve_end(e, 1, LK_UPDATE_BACKWARD);
}

// `set`: the sectors to solve - an order table with the layout of d_order (class c's sectors at the front of class c's own
// range, so that every per-class offset derived from class_begin[c] stays valid) and per-class counts.  nullptr: the
// engine's own table and the class_begin differences, i.e. every sector of the domain.
int launch_all(lk_engine *e, const float *d_guess, lk_result *d_result, const LkSectorSet *set) {
  if (int rc = reclassify_if_dirty(e))
    return rc;
  if (!set && d_result == e->d_result.p)
    e->records_S = e->S;
  if (e->update == LK_UPDATE_BACKWARD)
    return launch_all_backward(e, d_guess, d_result, set);
  const uint32_t *order = set ? set->order : e->d_order.p;
  int count[kNumClasses];
  for (int c = 0; c < kNumClasses; ++c)
    count[c] = set ? set->count[c] : e->class_begin[c + 1] - e->class_begin[c];
  Range range_("lk:solve");
  if (int rc = solve_begin(e))
    return rc;
  static const bool overlap = env_int("LK_CLASS_STREAMS", 1) != 0; // (read once)
  int n_classes = 0;
  for (int c = 0; c < kNumClasses; ++c)
    n_classes += count[c] > 0;
  ClassFork fork{e, n_classes > 1 && overlap};
  if (int rc = fork.open())
    return rc;
  for (int c = 0; c < kNumClasses; ++c) {
    int n = count[c];
    if (n <= 0)
      continue;
    hipStream_t st = nullptr;
    if (int rc = fork.stream_of(c, &st))
      return rc;
    LkSolveArgs a = base_args(e, d_guess, d_result);
    a.order = order + e->class_begin[c];
    a.n_sectors = n;
    a.queue = e->d_queue.p + 8 * c;
    a.safe = safe_flavour(e) ? 1 : 0;
    TeamTurn team_turn; // (a class that launches a team takes its turn before that launch)
    if (e->reference_order > 0) {
      // Reference-order mode: ONE launch per class, every level with the ordered sums and the
      // restated QR - a 16-lane row per small sector (four sectors share a wavefront's QR),
      // a wavefront per larger one.  No starved-level kernel, finisher, SAFE pass or team: the
      // ordered kernel is all of them.
      a.safe = 1;
      a.solo = 0;
      // Starved levels (at most 2P samples) first, by the one-lane kernel and its finisher: their sums and their QR
      // are the sequential reference's by construction, 64 sectors share one instruction stream of the QR instead of
      // four, and the records stay the same bytes (config 5: the ordered kernel then starts at level 2).  Only for
      // thread counts that leave such a level's summation sequential: T = 1, or T >= the level's sample count (every
      // chunk is one sample then, correlation_class.cpp:169-186).
      const int ref_chain = env_int("LK_REF_STARVED_CHAIN", 1); // test hook, read per call: 0 never, 2 whatever the sector count
      // ... and only where the one-lane kernel has the wavefronts to fill the chip (64 sectors each): config 5's
      // 199 809 sectors 10.0 -> 8.6 ms; config 4's 50 176 would be 784 wavefronts waiting on their own QR chains
      // (2.12 -> 2.18 ms), so they stay with the ordered kernel.
      if (ref_chain != 0 && e->class_starved[c] && e->eval_cap > 0 && (n >= 131072 || ref_chain == 2) &&
          (e->reference_order == 1 || e->reference_order >= starved_max(e))) {
        a.reference_order = 0; // (the starved-level instances; `mark_stale` keeps the stale-iteration markers coming)
        a.mark_stale = 1;
        int rc = launch_starved(e, a, c, e->class_begin[c], st);
        if (rc)
          return rc;
      }
      a.mark_stale = 1;
      a.reference_order = e->reference_order;
      // number_of_threads = T > 1 on the big classes: a TEAM of T workgroups per sector, one thread chunk of the reference
      // each (the launch falls back to one workgroup per sector when T x sectors are not all resident at once)
      if (const int T = reference_team_of_class(e, c, n)) {
        HIPCHK(e->d_team_partials.ensure((size_t)n * 2 * (size_t)T * 32));
        HIPCHK(e->d_team_arrivals.ensure(2 * (size_t)n));
        a.team_w = T;
        a.team_min_samples = 0;
        a.team_partials = e->d_team_partials.p;
        a.team_arrivals = e->d_team_arrivals.p;
        a.team_fault = team_fault_hook();
        if (int rc = team_turn.take(e, st))
          return rc;
      }
      HIPCHK(lk_launch_solve(a, e->cfg.fitting_model, e->cfg.interpolation, reference_group_of_class(c, n), st, e->launch_report_slot()));
    } else {
      if (e->team_share_permille > 0 && (c == kTeamClass || c == kTeamClass - 1))
        a.slots_permille = c == kTeamClass ? e->team_share_permille : 1000 - e->team_share_permille;
      if (c == kTeamClass) {
        a.team_w = e->team_w;
        a.team_min_samples = e->team_min_samples;
        a.team_partials = e->d_team_partials.p;
        a.team_arrivals = e->d_team_arrivals.p;
        a.team_fault = team_fault_hook();
        if (e->team_w > 1)
          if (int rc = team_turn.take(e, st))
            return rc;
      }
      if (e->class_starved[c]) // coarsest level(s) first, one lane per sector (+ finisher)
        if (int rc = launch_starved(e, a, c, e->class_begin[c], st))
          return rc;
      if (int rc = launch_groups(e, a, kGroupOfClass[c], c, e->class_begin[c], st))
        return rc;
    }
    if (int rc = team_turn.done(e, st))
      return rc;
    if (int rc = fork.join(c, st))
      return rc;
  }
  if (e->reference_order > 0 && !e->defer_stale)
    if (int rc = stale_iterations(e, d_result, e->S))
      return rc;
  return solve_end(e, 1, LK_UPDATE_FORWARD);
}

int lk_correlate_all_async(lk_engine *e) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (e->results_pending)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_correlate_all_async: the previous solve has not been waited for");
  HIPCHK(hipSetDevice(e->cfg.device));
  int rc = refresh_level_views(e);
  if (rc)
    return rc;
  if (e->h_results_n < (size_t)e->S) {
    if (e->h_results)
      HIPCHK(hipHostFree(e->h_results));
    e->h_results = nullptr;
    e->h_results_n = 0;
    HIPCHK(hipHostMalloc((void **)&e->h_results, (size_t)e->S * sizeof(lk_result), hipHostMallocDefault));
    e->h_results_n = (size_t)e->S;
  }
  if (!e->ev_results)
    HIPCHK(hipEventCreateWithFlags(&e->ev_results, hipEventDisableTiming));
  rc = launch_all(e, e->d_guess.p, e->d_result.p);
  if (rc)
    return rc;
  HIPCHK(hipMemcpyAsync(e->h_results, e->d_result.p, (size_t)e->S * sizeof(lk_result), hipMemcpyDeviceToHost,
                        e->stream));
  HIPCHK(hipEventRecord(e->ev_results, e->stream));
  e->results_pending = true;
  return LK_ERROR_NONE;
}

// Wait for an event with the latency of a polling loop: hipEventSynchronize may put the thread to sleep and wake it
// hundreds of microseconds late - more than a whole C2 solve takes.  Poll for a while first (a solve is 0.2-10 ms), then
// block.
hipError_t wait_event(hipEvent_t ev) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q != hipErrorNotReady)
      return q;
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20))
      return hipEventSynchronize(ev);
    std::this_thread::yield();
  }
}

int lk_wait_results(lk_engine *e, lk_result *out) {
  Range range_("lk:gather records");
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->results_pending || !out)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_wait_results: no solve outstanding / null buffer");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(wait_event(e->ev_results));
  e->results_pending = false;
  std::memcpy(out, e->h_results, (size_t)e->S * sizeof(lk_result));
  return LK_ERROR_NONE;
}

int lk_correlate_all_device(lk_engine *e, const void *d_guesses, void *d_results) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  HIPCHK(hipSetDevice(e->cfg.device));
  int rc = refresh_level_views(e);
  if (rc)
    return rc;
  return launch_all(e, d_guesses ? (const float *)d_guesses : e->d_guess.p,
                    d_results ? (lk_result *)d_results : e->d_result.p);
}

int lk_get_results_device(lk_engine *e, const void **d_records) {
  if (!e || !d_records)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_results_device: sectors are not committed");
  *d_records = e->d_result.p;
  return LK_ERROR_NONE;
}

int lk_correlate_all(lk_engine *e, const float *guesses, lk_result *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!out)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_correlate_all: null result buffer");
  HIPCHK(hipSetDevice(e->cfg.device));
  int rc = refresh_level_views(e);
  if (rc)
    return rc;
  if (guesses)
    HIPCHK(hipMemcpyAsync(e->d_guess.p, guesses, 6 * (size_t)e->S * sizeof(float), hipMemcpyHostToDevice,
                          e->stream));
  rc = launch_all(e, e->d_guess.p, e->d_result.p);
  if (rc)
    return rc;
  Range range_("lk:gather records");
  HIPCHK(hipMemcpyAsync(out, e->d_result.p, (size_t)e->S * sizeof(lk_result), hipMemcpyDeviceToHost,
                        e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return LK_ERROR_NONE;
}

int lk_correlate(lk_engine *e, int sector, float *guess_inout, lk_result *out) {
  Range range_("lk:correlate one sector");
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!guess_inout || !out)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_correlate: null argument");
  HIPCHK(hipSetDevice(e->cfg.device));
  int rc = refresh_level_views(e);
  if (rc)
    return rc;
  if (sector < 0 || sector >= e->S)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_correlate: unknown sector");
  float g[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < e->P; ++i)
    g[i] = guess_inout[i];
  uint32_t sidx = (uint32_t)sector;
  HIPCHK(hipMemcpyAsync(e->d_guess.p + 6 * (size_t)sector, g, sizeof(g), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_single.p, &sidx, sizeof(sidx), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  // three launch paths, one sector (d_single) on the engine's stream each, then the one tail
  if (e->update == LK_UPDATE_BACKWARD) { // the sector's own lane group: the bits of the batch solve
    if ((rc = bw_tables(e)))
      return rc;
    LkBackwardArgs b = bw_args(e, e->d_guess.p, e->d_result.p);
    b.order = e->d_single.p;
    b.n_sectors = 1;
    if ((rc = solve_begin(e)))
      return rc;
    HIPCHK(lk_launch_backward(b, e->cfg.fitting_model, e->cfg.interpolation, lk_bw_group(level0_count(e, sector)), e->stream,
                              e->launch_report_slot()));
    if ((rc = solve_end(e, 1, LK_UPDATE_BACKWARD)))
      return rc;
  } else {
    const int c = e->h_class[(size_t)sector];
    LkSolveArgs a = base_args(e, e->d_guess.p, e->d_result.p);
    a.order = e->d_single.p;
    a.n_sectors = 1;
    a.queue = e->d_queue.p;
    a.safe = safe_flavour(e) ? 1 : 0;
    if (e->reference_order > 0) { // (the ordered kernel of launch_all, with the lane group of a lone sector)
      a.safe = 1;
      a.solo = 0;
      a.reference_order = e->reference_order;
      if ((rc = solve_begin(e)))
        return rc;
      HIPCHK(lk_launch_solve(a, e->cfg.fitting_model, e->cfg.interpolation, reference_group_of_sector(e, sector), e->stream,
                             e->launch_report_slot()));
      if ((rc = stale_iterations(e, e->d_result.p + sector, 1)))
        return rc;
    } else {
      TeamTurn team_turn;
      if (c == kTeamClass) {
        a.team_w = e->team_w;
        a.team_min_samples = e->team_min_samples;
        a.team_partials = e->d_team_partials.p;
        a.team_arrivals = e->d_team_arrivals.p;
        a.team_fault = team_fault_hook();
        if (e->team_w > 1 && (rc = team_turn.take(e, e->stream)))
          return rc;
      }
      if ((rc = solve_begin(e)))
        return rc;
      if (e->class_starved[c] && (rc = launch_starved(e, a, 0, 0, e->stream)))
        return rc;
      if ((rc = launch_groups(e, a, kGroupOfClass[c], 0, 0, e->stream)))
        return rc;
      if ((rc = team_turn.done(e, e->stream)))
        return rc;
    }
    if ((rc = solve_end(e, 1, LK_UPDATE_FORWARD)))
      return rc;
  }
  HIPCHK(hipMemcpyAsync(out, e->d_result.p + sector, sizeof(lk_result), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < e->P; ++i)
    guess_inout[i] = out->resultingParameters[i]; // cuda_class.cu:289-290
  return LK_ERROR_NONE;
}

int lk_get_launch_report(lk_engine *e, lk_launch_record *out, int capacity, int *n_out, int *overflow) {
  if (!e || !n_out || (out && capacity < 0))
    return LK_ERROR_BAD_DOMAIN;
  const int kept = std::min(e->launch_report_n, (int)LK_LAUNCH_REPORT_CAPACITY);
  *n_out = kept;
  if (overflow)
    *overflow = e->launch_report_n > LK_LAUNCH_REPORT_CAPACITY ? 1 : 0;
  if (out)
    std::memcpy(out, e->launch_report, (size_t)std::min(kept, capacity) * sizeof(lk_launch_record));
  return LK_ERROR_NONE;
}

int lk_get_sector_groups(lk_engine *e, int *groups, int *team_w) {
  if (!e || !groups)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_sector_groups: sectors are not committed");
  if (e->recommit_pending || e->classes_dirty) // (read-only: the pending work belongs to the next solve, not to a query)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_sector_groups: sectors were appended or moved since the last batch solve; the classes are stale");
  for (int s = 0; s < e->S; ++s) {
    const int c = e->h_class[(size_t)s], n = e->class_begin[c + 1] - e->class_begin[c];
    groups[s] = e->reference_order > 0 ? reference_group_of_class(c, n) : kGroupOfClass[c];
    if (team_w)
      team_w[s] = e->reference_order > 0 ? (groups[s] == 512 ? reference_team_of_class(e, c, n) : 0) : c == kTeamClass ? e->team_w : 0;
  }
  return LK_ERROR_NONE;
}

int lk_adjust_initial_guess(lk_engine *e, int frame, int constant_velocity, const float *global_guess,
                            float global_cx, float global_cy) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_adjust_initial_guess: sectors are not committed");
  float gg[6] = {0, 0, 0, 0, 0, 0};
  if (global_guess)
    for (int i = 0; i < 6; ++i)
      gg[i] = global_guess[i];
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(lk_launch_guess(e->d_center.p, e->d_last_p.p, e->d_prev_p.p, e->d_guess.p, gg, global_cx, global_cy,
                         e->S, e->cfg.fitting_model, frame, constant_velocity, e->stream));
  return LK_ERROR_NONE;
}

int lk_get_guesses(lk_engine *e, float *guesses) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed || !guesses)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_guesses: sectors are not committed");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipMemcpyAsync(guesses, e->d_guess.p, 6 * (size_t)e->S * sizeof(float), hipMemcpyDeviceToHost,
                        e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return LK_ERROR_NONE;
}

// what an evaluation kernel leaves in d_scratch (the matrix, the right-hand side, chi, the out-of-image flag) -> the caller's arrays
static int evaluation_out(lk_engine *e, float *A36, float *b6, float *chi, int *error) {
  float h[44];
  HIPCHK(hipMemcpyAsync(h, e->d_scratch.p, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (A36)
    std::memcpy(A36, h, 36 * sizeof(float));
  if (b6)
    std::memcpy(b6, h + 36, 6 * sizeof(float));
  if (chi)
    *chi = h[42];
  if (error)
    *error = h[43] != 0.f ? LK_ERROR_INTERPOLATION_OUT_OF_IMAGE : LK_ERROR_NONE;
  return LK_ERROR_NONE;
}

int lk_evaluate(lk_engine *e, int sector, int level, const float *p, float *A36, float *b6, float *chi,
                int *error) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  HIPCHK(hipSetDevice(e->cfg.device));
  int rc = refresh_level_views(e);
  if (rc)
    return rc;
  if (sector < 0 || sector >= e->S || level < 0 || level > e->cfg.py_stop || !p ||
      e->h_off[level].size() != (size_t)e->S + 1)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_evaluate: unknown sector/level");
  LkEvalArgs a{};
  a.lv = e->d_lv.p;
  a.center = e->d_center.p;
  a.sector = sector;
  a.level = level;
  for (int i = 0; i < 6; ++i)
    a.p[i] = i < e->P ? p[i] : 0.f;
  a.out = e->d_scratch.p;
  a.ref_threads = e->reference_order;
  const int group = e->reference_order > 0 ? reference_group_of_sector(e, sector) : kGroupOfClass[e->h_class[(size_t)sector]];
  e->launch_report_begin();
  HIPCHK(lk_launch_eval(a, e->cfg.fitting_model, e->cfg.interpolation, group, e->stream, e->launch_report_slot()));
  return evaluation_out(e, A36, b6, chi, error);
}

int lk_evaluate_backward(lk_engine *e, int sector, int level, const float *p, float *H36, float *b6, float *chi,
                         int *error) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  HIPCHK(hipSetDevice(e->cfg.device));
  int rc = refresh_level_views(e);
  if (rc)
    return rc;
  if (sector < 0 || sector >= e->S || level < 0 || level > e->cfg.py_stop || !p ||
      e->h_off[level].size() != (size_t)e->S + 1)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_evaluate_backward: unknown sector/level");
  if (int rc2 = reclassify_if_dirty(e))
    return rc2;
  if (int rc2 = bw_tables(e))
    return rc2;
  HIPCHK(e->d_scratch.ensure(64));
  LkBackwardEvalArgs a{};
  a.lv = e->d_lv.p;
  a.center = e->d_center.p;
  a.tpl = e->d_bw_tpl.p + e->h_bw_base[(size_t)sector];
  a.sector = sector;
  a.level = level;
  for (int i = 0; i < 6; ++i)
    a.p[i] = i < e->P ? p[i] : 0.f;
  a.out = e->d_scratch.p;
  e->launch_report_begin();
  HIPCHK(lk_launch_backward_eval(a, e->cfg.fitting_model, e->cfg.interpolation, lk_bw_group(level0_count(e, sector)), e->stream,
                                 e->launch_report_slot()));
  return evaluation_out(e, H36, b6, chi, error);
}

int lk_sample(lk_engine *e, int slot, int level, const float *xy, int n, float *out4) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (slot < 0 || slot > 2 || level < 0 || level > e->cfg.py_stop || !e->img[slot].valid || !xy || !out4 ||
      n < 1)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_sample: bad arguments");
  HIPCHK(hipSetDevice(e->cfg.device));
  const DevImage &im = e->img[slot];
  DevBuf<float2> d_pts;
  DevBuf<float4> d_out;
  HIPCHK(d_pts.ensure((size_t)n));
  HIPCHK(d_out.ensure((size_t)n));
  int rc = LK_ERROR_NONE;
  hipError_t he = hipMemcpyAsync(d_pts.p, xy, 2 * sizeof(float) * (size_t)n, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess)
    he = lk_launch_sample(e->cfg.interpolation, im.lvl[level], im.rows >> level, im.cols >> level, d_pts.p, n,
                          d_out.p, e->stream);
  if (he == hipSuccess)
    he = hipMemcpyAsync(out4, d_out.p, 4 * sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, e->stream);
  if (he == hipSuccess)
    he = hipStreamSynchronize(e->stream);
  if (he != hipSuccess)
    rc = e->hipfail(he, "lk_sample");
  d_pts.release();
  d_out.release();
  return rc;
}

int lk_damped_solve(lk_engine *e, int n, const float *A, const float *b, float lambda, float scaling,
                    int reference_solver, float *dp) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!(n == 1 || n == 2 || n == 3 || n == 6) || !A || !b || !dp)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_damped_solve: n must be 1, 2, 3 or 6");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(e->d_scratch.ensure(64));
  float h[48];
  std::memset(h, 0, sizeof(h));
  for (int i = 0; i < n; ++i) {
    h[36 + i] = b[i];
    for (int j = 0; j < n; ++j)
      h[i * 6 + j] = A[i * n + j];
  }
  h[42] = lambda;
  h[43] = scaling;
  h[44] = (float)reference_solver; // 0: fast path, 1: the restated QR, 2: the same QR spread over a 16-lane row
  HIPCHK(hipMemcpyAsync(e->d_scratch.p, h, sizeof(h), hipMemcpyHostToDevice, e->stream));
  HIPCHK(lk_launch_solve_only(n, e->d_scratch.p, e->d_scratch.p + 48, e->stream));
  float o[6];
  HIPCHK(hipMemcpyAsync(o, e->d_scratch.p + 48, sizeof(o), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < n; ++i)
    dp[i] = o[i];
  return LK_ERROR_NONE;
}

// both known-answer hooks below: host arrays in, one launch, host arrays out (buffers of their own, freed on every path)
static int compare_launch(lk_engine *e, const float *in, size_t n_in, float *out, size_t n_out,
                          const std::function<hipError_t(const float *, float *)> &launch) {
  HIPCHK(hipSetDevice(e->cfg.device));
  DevBuf<float> d_in, d_out;
  hipError_t err = d_in.ensure(n_in);
  if (err == hipSuccess)
    err = d_out.ensure(n_out);
  if (err == hipSuccess)
    err = hipMemcpyAsync(d_in.p, in, n_in * sizeof(float), hipMemcpyHostToDevice, e->stream);
  if (err == hipSuccess)
    err = launch(d_in.p, d_out.p);
  if (err == hipSuccess)
    err = hipMemcpyAsync(out, d_out.p, n_out * sizeof(float), hipMemcpyDeviceToHost, e->stream);
  const hipError_t sync = hipStreamSynchronize(e->stream);
  d_in.release();
  d_out.release();
  HIPCHK(err);
  HIPCHK(sync);
  return LK_ERROR_NONE;
}

int lk_step_compare(lk_engine *e, int n, const float *in40, float *out32) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (n < 1 || !in40 || !out32)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_step_compare: n >= 1 systems of 40 floats in, 32 floats out each");
  return compare_launch(e, in40, (size_t)n * 40, out32, (size_t)n * 32,
                        [&](const float *i, float *o) { return lk_launch_step_compare(n, i, o, e->stream); });
}

int lk_reduce_compare(lk_engine *e, int n, int wide, const float *lanes, float *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (n < 1 || !lanes || !out)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_reduce_compare: n >= 1 wavefronts of 64 x 28 floats in, twice that out");
  return compare_launch(e, lanes, (size_t)n * 64 * 28, out, (size_t)n * 2 * 64 * 28,
                        [&](const float *i, float *o) { return lk_launch_reduce_compare(n, wide, i, o, e->stream); });
}
