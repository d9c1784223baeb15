// lk_engine_sequence.cpp - sequences on the engine: the ring of resident frames, the frame-pipelined windows and their
// entry points.
#include "lk_engine_state.hpp"

// ------------------------------------------------------------------------------------
// Frame-pipelined windows of a sequence (perform_multiframe_correlation's frame loop,
// manager_class.cpp:1380-1496, with the Eulerian description: the sectors stay, the deformed
// image changes, and the guess of frame f + 1 of a sector is a function of that sector's own
// earlier results, :2677-2699).  K deformed frames are resident at once (the ring); ONE launch
// per size class solves all of them, every sector advancing from frame to frame on its own
// (the SEQ instances of lk_solve_kernel), instead of one launch - and one straggler tail - per pair.
// ------------------------------------------------------------------------------------
int lk_sequence_reserve(lk_engine *e, int n_slots) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (n_slots < 1 || n_slots > 4096)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_sequence_reserve: n_slots must be in 1..4096");
  if (e->seq.outstanding)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_sequence_reserve: a window is outstanding (lk_wait_sequence)");
  HIPCHK(hipSetDevice(e->cfg.device));
  std::lock_guard<std::mutex> lock(e->nxt_mu);
  if ((int)e->ring.size() < n_slots) {
    const size_t old = e->ring.size();
    e->ring.resize((size_t)n_slots);
    e->ring_ready.resize((size_t)n_slots, nullptr);
    e->ring_fresh.resize((size_t)n_slots, 0);
    e->ring_window.resize((size_t)n_slots, 0u);
    for (size_t i = old; i < (size_t)n_slots; ++i)
      HIPCHK(hipEventCreateWithFlags(&e->ring_ready[i], hipEventDisableTiming));
  }
  return LK_ERROR_NONE;
}

static int sequence_set_frame(lk_engine *e, int slot, const void *src, bool on_device, int rows, int cols, int step,
                              hipEvent_t after = nullptr, hipEvent_t consumed = nullptr) {
  Range range_("lk:upload+pyramid (ring)");
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!src || rows < 1 || cols < 1 || step < cols)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_sequence_set_frame: bad arguments");
  HIPCHK(hipSetDevice(e->cfg.device));
  // like the next-frame slot: filled on the next-frame stream, so that the frames of window w + 1 arrive and get their
  // pyramids while window w is being solved (manager_class.cpp:1438-1447)
  std::unique_lock<std::mutex> lock(e->nxt_mu);
  if (slot < 0 || slot >= (int)e->ring.size())
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_sequence_set_frame: unknown ring slot (lk_sequence_reserve)");
  hipStream_t st = e->nxt_stream;
  if (e->ring_window[(size_t)slot]) // a window read this slot: it must be through with it (stream order on the device)
    HIPCHK(hipStreamWaitEvent(st, e->seq_done[(e->ring_window[(size_t)slot] - 1) % 4], 0));
  if (after)
    HIPCHK(hipStreamWaitEvent(st, after, 0));
  int rc = fill_image(e, e->ring[(size_t)slot], src, on_device, rows, cols, step, st, false);
  if (rc)
    return rc;
  if (consumed)
    HIPCHK(hipEventRecord(consumed, st));
  HIPCHK(hipEventRecord(e->ring_ready[(size_t)slot], st));
  e->ring_fresh[(size_t)slot] = 1;
  lock.unlock();
  if (!on_device && !host_pinned(src)) // pageable host memory: the copy must have left it
    HIPCHK(hipStreamSynchronize(st));
  return LK_ERROR_NONE;
}

int lk_sequence_set_frame(lk_engine *e, int slot, const uint8_t *host_pixels, int rows, int cols, int step) {
  return sequence_set_frame(e, slot, host_pixels, false, rows, cols, step);
}
int lk_sequence_set_frame_device(lk_engine *e, int slot, const void *device_pixels, int rows, int cols, int step) {
  return sequence_set_frame(e, slot, device_pixels, true, rows, cols, step);
}
int lk_internal_sequence_set_frame_device_after(lk_engine *e, int slot, const void *device_pixels, int rows, int cols, int step,
                                                hipEvent_t after, hipEvent_t consumed) { // (lk_internal.hpp)
  return sequence_set_frame(e, slot, device_pixels, true, rows, cols, step, after, consumed);
}

// lane group and flavour of a class inside a window (-1: the class has no frame-pipelined instance)
static int seq_group_of_class(const lk_engine *e, int c, int n) {
  if (e->reference_order > 0) {
    const int g = reference_group_of_class(c, n);
    return g == 512 ? -1 : g;
  }
  const int g = kGroupOfClass[c];
  if (g > 64)
    return -1;
  if (e->class_starved[c]) {
    // (starved levels inside the window: the 16-lane rows' finisher arithmetic - whatever width the one-pair classifier
    // promoted a class of few small sectors to, e.g. one rank's block of a sharded sequence: the rule below keeps big ones out)
    // ... which pays while the sectors are small.  Config 5's geometry (17 x 17 samples, one starved level of four) measured
    // 9.1 ms per pair in a window against 5.9 (default) / 7.4 (batch-invariant) for the one-pair chain, whose one-lane kernel
    // shares one instruction stream of the QR among 64 sectors and whose lane groups widen: such classes keep the chain, frame
    // after frame.  9 x 9 samples: 1.12 against 1.66; 7 x 7: 0.98-1.21 against 1.6-1.9.
    static const int big_n0 = env_int("LK_SEQ_STARVED_MAX_N0", 128); // tuning hook, read once
    long long n0 = 0, n_starved = 0; // (over the sectors that HAVE a starved level: a class may mix them with others)
    const int top = e->cfg.py_stop;
    for (int i = e->class_begin[c]; i < e->class_begin[c + 1]; ++i) {
      const int s = (int)e->h_order[(size_t)i];
      const int4 r = e->h_rect[top][(size_t)s];
      const int n_top = r.z > 0 ? r.w : (int)(e->h_off[top][(size_t)s + 1] - e->h_off[top][(size_t)s]);
      if (n_top <= starved_max(e)) {
        n0 += level0_count(e, s);
        ++n_starved;
      }
    }
    if (n0 > (long long)big_n0 * n_starved)
      return -1;
    return 16;
  }
  return g;
}

static bool seq_pipelinable(const lk_engine *e) {
  static const bool off = env_int("LK_SEQ_PIPELINE", 1) == 0; // comparison hook, read once
  if (off || e->update == LK_UPDATE_BACKWARD) // (the backward update has no frame-pipelined instances)
    return false;
  for (int c = 0; c < kNumClasses; ++c) {
    const int n = e->class_begin[c + 1] - e->class_begin[c];
    if (n > 0 && seq_group_of_class(e, c, n) < 0)
      return false;
  }
  return true;
}

// one window on the device: the pipelined launches, or - domains with classes that have no such instance (teams,
// workgroup-wide groups) - the frames one after the other through the ordinary launches, same buffers either way
static int launch_window(lk_engine *e) {
  lk_engine::SeqWindow &w = e->seq;
  const int S = e->S, n = w.n_frames, R = (int)e->ring.size();
  const DevImage &u0 = w.und_slot >= 0 ? e->ring[(size_t)w.und_slot] : e->img[LK_IMG_UND];
  auto def_of = [&](int i) -> DevImage & { return e->ring[(size_t)((w.first_slot + i) % R)]; };
  auto und_of = [&](int i) -> const DevImage & { return (w.reference_previous && i > 0) ? def_of(i - 1) : u0; };
  if (int rc = solve_begin(e))
    return rc;
  if (!w.pipelined) {
    // the one-pair loop on the device: images of frame i in the pair slots, guess, solve, records to their row
    DevImage keep_und = e->img[LK_IMG_UND], keep_def = e->img[LK_IMG_DEF];
    int rc = LK_ERROR_NONE;
    for (int i = 0; i < n && !rc; ++i) {
      e->img[LK_IMG_UND] = und_of(i);
      e->img[LK_IMG_DEF] = def_of(i);
      e->lv_dirty = true;
      rc = refresh_level_views(e);
      if (!rc && i > 0) {
        const float gg[6] = {0, 0, 0, 0, 0, 0};
        if (lk_launch_guess(e->d_center.p, e->d_last_p.p, e->d_prev_p.p, e->d_guess.p, gg, 0.f, 0.f, S, e->cfg.fitting_model, 1,
                            w.velocity, e->stream) != hipSuccess)
          rc = e->fail(LK_ERROR_DEVICE, "lk_correlate_sequence: guess launch failed");
      }
      if (!rc && w.want_guesses && hipMemcpyAsync(e->d_seq_guess.p + (size_t)i * 6 * (size_t)S, e->d_guess.p, 6 * (size_t)S * sizeof(float),
                                                 hipMemcpyDeviceToDevice, e->stream) != hipSuccess)
        rc = e->fail(LK_ERROR_DEVICE, "lk_correlate_sequence: guess copy failed");
      const bool timing = e->timing;
      e->timing = false; // (the window's own events bracket all frames)
      if (!rc)
        rc = launch_all(e, e->d_guess.p, e->d_seq_result.p + (size_t)i * (size_t)S);
      e->timing = timing;
      if (!rc && hipMemcpyAsync(e->d_seq_stats.p + (size_t)i * 4 * (size_t)S, e->d_stats.p, 4 * (size_t)S * sizeof(uint32_t),
                                hipMemcpyDeviceToDevice, e->stream) != hipSuccess)
        rc = e->fail(LK_ERROR_DEVICE, "lk_correlate_sequence: stats copy failed");
    }
    e->img[LK_IMG_UND] = keep_und;
    e->img[LK_IMG_DEF] = keep_def;
    e->lv_dirty = true;
    if (rc)
      return rc;
  } else {
    // per-frame image table, chain and flags of this window
    std::vector<LkSeqFrame> table((size_t)n);
    for (int i = 0; i < n; ++i) {
      const DevImage &u = und_of(i), &d = def_of(i);
      for (int l = 0; l < LK_MAX_LEVELS; ++l) {
        table[(size_t)i].und[l] = l <= e->cfg.py_stop ? u.lvl[l] : nullptr;
        table[(size_t)i].def[l] = l <= e->cfg.py_stop ? d.lvl[l] : nullptr;
      }
    }
    HIPCHK(hipMemcpyAsync(e->d_seq_img.p, table.data(), table.size() * sizeof(LkSeqFrame), hipMemcpyHostToDevice, e->stream)); // (pageable: staged before it returns)
    HIPCHK(hipMemsetAsync(e->d_seq_chain.p, 0, (size_t)S * kLkSeqChainWords * sizeof(unsigned long long), e->stream));
    HIPCHK(hipMemsetAsync(e->d_seq_flags.p, 0, 4 * sizeof(uint32_t), e->stream));
    int n_classes = 0;
    for (int c = 0; c < kNumClasses; ++c)
      n_classes += e->class_begin[c + 1] > e->class_begin[c];
    struct SafePass {
      LkSolveArgs a;
      int group;
    };
    std::vector<SafePass> safe_pass; // the classes that run the fast flavour
    ClassFork fork{e, n_classes > 1}; // classes are independent sector sets: side by side, as in launch_all
    if (int rc = fork.open())
      return rc;
    for (int c = 0; c < kNumClasses; ++c) {
      const int nc = e->class_begin[c + 1] - e->class_begin[c];
      if (nc <= 0)
        continue;
      hipStream_t st = nullptr;
      if (int rc = fork.stream_of(c, &st))
        return rc;
      LkSolveArgs a = base_args(e, e->d_guess.p, e->d_seq_result.p);
      a.stats = e->d_seq_stats.p;
      a.order = e->d_order.p + e->class_begin[c];
      a.n_sectors = nc;
      a.queue = e->d_queue.p + 8 * c;
      a.solo = 0;
      a.seq_frames = n;
      a.seq_velocity = w.velocity;
      a.seq_stride = S;
      a.seq_img = e->d_seq_img.p;
      a.seq_chain = e->d_seq_chain.p;
      a.seq_prev_p = e->d_prev_p.p;
      a.seq_prev_p_out = e->d_prev_p_alt.p;
      a.seq_guess_out = w.want_guesses ? e->d_seq_guess.p : nullptr;
      a.seq_flags = e->d_seq_flags.p;
      a.seq_fault = env_int("LK_SEQ_FAULT", 0); // test hook, read per launch: a frame that never publishes
      int flavour = (safe_flavour(e) || e->class_starved[c]) ? 1 : 0;
      if (e->reference_order > 0) {
        flavour = 2;
        a.reference_order = e->reference_order;
        a.mark_stale = 1;
      } else if (e->class_starved[c]) {
        // Sectors that spend most of their evaluations on starved levels (config 4: 7 x 7 samples, 9-16 and 1-4 at levels 1
        // and 2).  The rows of a wavefront then sit at different levels most of the time: no level alignment (it never
        // changes a bit; 1.33 -> 1.21 ms per pair).  And in the default mode - whose arithmetic is free within the
        // reference's noise - such a class takes the reference-order instance with its lanes dealt by need, which IS the
        // CPU engine's arithmetic and the fastest instance at these sizes (0.98 ms per pair).
        long long n0 = 0;
        for (int i = e->class_begin[c]; i < e->class_begin[c + 1]; ++i)
          n0 += level0_count(e, (int)e->h_order[(size_t)i]);
        static const int small_n0 = env_int("LK_SEQ_SMALL", 64); // tuning hook, read once
        // ... while the class is in the throughput regime.  With fewer sectors than lane-group rows are resident (12 288 at three
        // wavefronts per SIMD: one rank's block of a sharded sequence) the window lasts as long as its slowest sector's chain, and
        // the unified rows' steps are the shorter ones: blocks of config 4's grid, windows of 16 pairs, reference-order instance /
        // unified rows: 25 088 sectors 0.77 / 0.82 ms per pair, 12 544: 0.67 / 0.61, 6272: 0.58 / 0.50, 3136: 0.54 / 0.48.
        static const int latency_nc = env_int("LK_SEQ_LATENCY_SECTORS", 16384); // tuning hook, read once
        // (and there the rows of a wavefront are better kept in step again - alignment never changes a bit: 6272 sectors, unified
        // rows, aligned / not: 0.50 / 0.59 ms per pair)
        if (n0 <= (long long)small_n0 * nc && nc > latency_nc) {
          a.align = 0;
          if (!safe_flavour(e)) {
            flavour = 2;
            a.reference_order = 1;
            a.mark_stale = -1; // (a first evaluation that fails reports 0 iterations, like every default-mode instance)
          }
        }
      }
      a.safe = flavour != 0;
      const int group = seq_group_of_class(e, c, nc);
      HIPCHK(lk_launch_solve_seq(a, e->cfg.fitting_model, e->cfg.interpolation, group, flavour, st, e->launch_report_slot()));
      if (int rc = fork.join(c, st))
        return rc;
      if (flavour == 0)
        safe_pass.push_back({a, group});
    }
    // A bad pivot in the fast flavour (d_seq_flags[1]; textureless sectors): the window of those classes again with the
    // SAFE instances - same guesses, same history, the records and sequence state overwritten.  Decided on the device, behind
    // every class of the window: the gated launches leave at once while the flag is 0, and the window's done-event (which
    // releases its ring slots to lk_sequence_set_frame) and records follow them.  A chain and a void flag of its own: nothing
    // is reset between the passes.  (Classes that borrow the reference-order instance keep their records: they met no pivot.)
    if (!safe_pass.empty()) {
      HIPCHK(e->d_seq_chain_safe.ensure((size_t)S * kLkSeqChainWords));
      HIPCHK(hipMemsetAsync(e->d_seq_chain_safe.p, 0, (size_t)S * kLkSeqChainWords * sizeof(unsigned long long), e->stream));
      for (SafePass &sp : safe_pass) {
        sp.a.seq_chain = e->d_seq_chain_safe.p;
        sp.a.seq_flags = e->d_seq_flags.p + 2;
        sp.a.seq_gate = e->d_seq_flags.p + 1;
        sp.a.safe = 1;
        HIPCHK(lk_launch_solve_seq(sp.a, e->cfg.fitting_model, e->cfg.interpolation, sp.group, 1, e->stream, e->launch_report_slot()));
      }
    }
    // reference-order mode: the stale iteration counts, in the order the reference solves - frame by frame, sector by
    // sector, which IS the layout of the window's records
    if (e->reference_order > 0 && !e->defer_stale) {
      int rc = stale_iterations(e, e->d_seq_result.p, n * S);
      if (rc)
        return rc;
    }
    HIPCHK(hipMemcpyAsync(e->h_seq_flags, e->d_seq_flags.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  }
  // (the counters cover the window's n frames; the update they describe stays what the last one-pair launch noted - the
  // one-pair loop above, or for a pipelined window whatever solve came before it)
  if (int rc = solve_end(e, n, e->stats_update))
    return rc;
  if (w.want_host)
    HIPCHK(hipMemcpyAsync(e->h_seq_results[e->h_seq_cur], e->d_seq_result.p, (size_t)n * (size_t)S * sizeof(lk_result), hipMemcpyDeviceToHost,
                          e->stream));
  HIPCHK(hipEventRecord(e->ev_seq, e->stream));
  return LK_ERROR_NONE;
}

// one of the two alternating pinned record buffers of the windows, at least `need` records
static int ensure_host_records(lk_engine *e, int b, size_t need) {
  if (e->h_seq_results_n[b] >= need)
    return LK_ERROR_NONE;
  if (e->h_seq_results[b])
    HIPCHK(hipHostFree(e->h_seq_results[b]));
  e->h_seq_results[b] = nullptr;
  e->h_seq_results_n[b] = 0;
  HIPCHK(hipHostMalloc((void **)&e->h_seq_results[b], need * sizeof(lk_result), hipHostMallocDefault));
  e->h_seq_results_n[b] = need;
  return LK_ERROR_NONE;
}

int lk_sequence_prepare_host_records(lk_engine *e, int n_frames) {
  if (!e || n_frames < 1)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->committed)
    return e->fail(LK_ERROR_BAD_DOMAIN, "sectors are not committed (call lk_commit_sectors)");
  HIPCHK(hipSetDevice(e->cfg.device));
  // (the buffer the running window's records go to - h_seq_cur - is not touched: this is the other one, which the next launch takes)
  return ensure_host_records(e, e->h_seq_cur ^ 1, (size_t)n_frames * (size_t)e->S);
}

int lk_correlate_sequence_async(lk_engine *e, int und_slot, int first_slot, int n_frames, int reference_previous,
                                int constant_velocity, int flags) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (e->seq.outstanding || e->results_pending)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_correlate_sequence_async: the previous solve has not been waited for");
  HIPCHK(hipSetDevice(e->cfg.device));
  const int R = (int)e->ring.size();
  if (n_frames < 1 || n_frames > R || first_slot < 0 || first_slot >= R || und_slot >= R)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_correlate_sequence_async: the window does not fit the ring (lk_sequence_reserve)");
  if (und_slot < 0 && !e->img[LK_IMG_UND].valid)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_correlate_sequence_async: no undeformed image");
  if (!e->committed)
    return e->fail(LK_ERROR_BAD_DOMAIN, "sectors are not committed (call lk_commit_sectors)");
  if (int rc = recommit_if_pending(e))
    return rc;
  if (int rc = reclassify_if_dirty(e))
    return rc;
  lk_engine::SeqWindow &w = e->seq;
  w.und_slot = und_slot;
  w.first_slot = first_slot;
  w.n_frames = n_frames;
  e->window_S = e->S;
  w.reference_previous = reference_previous != 0;
  w.velocity = constant_velocity != 0;
  w.want_host = (flags & 1) != 0;
  w.want_guesses = (flags & 2) != 0;
  w.pipelined = seq_pipelinable(e);
  const int S = e->S;
  // (held until this window's done-event is on the stream: a concurrent lk_sequence_set_frame into one of its slots waits for it)
  std::unique_lock<std::mutex> ring_lock(e->nxt_mu);
  {
    // the frames of the window: built, of one geometry, and visible to the solve stream
    const DevImage &u0 = und_slot >= 0 ? e->ring[(size_t)und_slot] : e->img[LK_IMG_UND];
    if (!u0.valid)
      return e->fail(LK_ERROR_BAD_DOMAIN, "lk_correlate_sequence_async: the undeformed frame's ring slot is empty");
    for (int i = 0; i < n_frames; ++i) {
      const size_t slot = (size_t)((first_slot + i) % R);
      const DevImage &d = e->ring[slot];
      if (!d.valid || d.rows != u0.rows || d.cols != u0.cols)
        return e->fail(LK_ERROR_BAD_DOMAIN, "lk_correlate_sequence_async: empty ring slot, or frames of different sizes");
      if (e->ring_fresh[slot]) {
        HIPCHK(hipStreamWaitEvent(e->stream, e->ring_ready[slot], 0));
        e->ring_fresh[slot] = 0;
      }
      e->ring_window[slot] = e->seq_windows + 1;
    }
    if (und_slot >= 0) {
      if (e->ring_fresh[(size_t)und_slot]) {
        HIPCHK(hipStreamWaitEvent(e->stream, e->ring_ready[(size_t)und_slot], 0));
        e->ring_fresh[(size_t)und_slot] = 0;
      }
      e->ring_window[(size_t)und_slot] = e->seq_windows + 1;
    }
  }
  HIPCHK(e->d_seq_result.ensure((size_t)n_frames * (size_t)S));
  HIPCHK(e->d_seq_stats.ensure((size_t)n_frames * 4 * (size_t)S));
  if (w.want_guesses)
    HIPCHK(e->d_seq_guess.ensure((size_t)n_frames * 6 * (size_t)S));
  HIPCHK(e->d_seq_chain.ensure((size_t)S * kLkSeqChainWords));
  HIPCHK(e->d_seq_img.ensure((size_t)n_frames));
  HIPCHK(e->d_seq_flags.ensure(4));
  HIPCHK(e->d_prev_p_alt.ensure(6 * (size_t)S));
  if (!e->h_seq_flags)
    HIPCHK(hipHostMalloc((void **)&e->h_seq_flags, 4 * sizeof(uint32_t), hipHostMallocDefault));
  std::memset(e->h_seq_flags, 0, 4 * sizeof(uint32_t));
  if (w.want_host) {
    e->h_seq_cur ^= 1;
    if (int hrc = ensure_host_records(e, e->h_seq_cur, (size_t)n_frames * (size_t)S))
      return hrc;
  }
  if (!e->ev_seq)
    HIPCHK(hipEventCreateWithFlags(&e->ev_seq, hipEventDisableTiming));
  for (hipEvent_t &ev : e->seq_done)
    if (!ev)
      HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  if (w.pipelined) {
    // the level table: lists, rectangles and geometry (the images come from the per-frame table)
    DevImage keep_und = e->img[LK_IMG_UND], keep_def = e->img[LK_IMG_DEF];
    e->img[LK_IMG_UND] = und_slot >= 0 ? e->ring[(size_t)und_slot] : e->img[LK_IMG_UND];
    e->img[LK_IMG_DEF] = e->ring[(size_t)first_slot];
    e->lv_dirty = true;
    int rc = refresh_level_views(e);
    e->img[LK_IMG_UND] = keep_und;
    e->img[LK_IMG_DEF] = keep_def;
    e->lv_dirty = true;
    if (rc)
      return rc;
  }
  Range range_("lk:solve window");
  int rc = launch_window(e);
  if (rc)
    return rc;
  HIPCHK(hipEventRecord(e->seq_done[e->seq_windows % 4], e->stream));
  ++e->seq_windows;
  ring_lock.unlock();
  w.outstanding = true;
  return LK_ERROR_NONE;
}

int lk_wait_sequence(lk_engine *e, lk_result *out) {
  Range range_("lk:gather window records");
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  lk_engine::SeqWindow &w = e->seq;
  if (!w.outstanding)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_wait_sequence: no window outstanding");
  if (out && !w.want_host)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_wait_sequence: the window was launched without host records (flags & 1)");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(wait_event(e->ev_seq));
  w.outstanding = false;
  const int S = e->S, n = w.n_frames;
  if (w.pipelined) {
    if (e->h_seq_flags[1] != 0u) // (the SAFE pass of launch_window solved the fast flavour's classes again)
      ++e->window_safe_reruns;
    if (e->h_seq_flags[0] != 0u || e->h_seq_flags[2] != 0u)
      return e->fail(LK_ERROR_DEVICE, "lk_wait_sequence: a sector's wait for its previous frame ran into its bound - the window is void");
    // commit the sequence state: previous_resulting_parameters (the last frame but one), the engine's own record buffer
    if (n >= 2)
      HIPCHK(hipMemcpyAsync(e->d_prev_p.p, e->d_prev_p_alt.p, 6 * (size_t)S * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d_result.p, e->d_seq_result.p + (size_t)(n - 1) * (size_t)S, (size_t)S * sizeof(lk_result),
                          hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d_stats.p, e->d_seq_stats.p + (size_t)(n - 1) * 4 * (size_t)S, 4 * (size_t)S * sizeof(uint32_t),
                          hipMemcpyDeviceToDevice, e->stream));
  } else {
    HIPCHK(hipMemcpyAsync(e->d_result.p, e->d_seq_result.p + (size_t)(n - 1) * (size_t)S, (size_t)S * sizeof(lk_result),
                          hipMemcpyDeviceToDevice, e->stream));
  }
  if (out)
    std::memcpy(out, e->h_seq_results[e->h_seq_cur], (size_t)n * (size_t)S * sizeof(lk_result));
  return LK_ERROR_NONE;
}

int lk_sequence_host_records(lk_engine *e, const lk_result **records) {
  if (!e || !records)
    return LK_ERROR_BAD_DOMAIN;
  if (e->seq.outstanding || !e->seq.want_host || !e->h_seq_results[e->h_seq_cur])
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_sequence_host_records: no waited-for window with host records (flags & 1)");
  *records = e->h_seq_results[e->h_seq_cur];
  return LK_ERROR_NONE;
}

int lk_get_sequence_results_device(lk_engine *e, const void **d_records, const void **d_guesses) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->d_seq_result.p)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_sequence_results_device: no window was solved");
  if (d_records)
    *d_records = e->d_seq_result.p;
  if (d_guesses)
    *d_guesses = e->d_seq_guess.p;
  return LK_ERROR_NONE;
}

int lk_sequence_is_pipelined(lk_engine *e) { return e && e->seq.pipelined ? 1 : 0; }

int lk_copy_sequence_records_device(lk_engine *e, void *d_dst, size_t dst_pitch_records) {
  if (!e || !d_dst)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->d_seq_result.p || e->seq.n_frames < 1 || dst_pitch_records < (size_t)e->S)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_copy_sequence_records_device: no window was solved, or the pitch is below the sector count");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipMemcpy2DAsync(d_dst, dst_pitch_records * sizeof(lk_result), e->d_seq_result.p, (size_t)e->S * sizeof(lk_result),
                          (size_t)e->S * sizeof(lk_result), (size_t)e->seq.n_frames, hipMemcpyDeviceToDevice, e->stream));
  return LK_ERROR_NONE;
}

int lk_get_sequence_guesses(lk_engine *e, float *out) {
  if (!e || !out)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->seq.want_guesses || e->seq.outstanding || !e->d_seq_guess.p)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_sequence_guesses: the last window kept no guesses (flags & 2), or is still outstanding");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipMemcpyAsync(out, e->d_seq_guess.p, (size_t)e->seq.n_frames * 6 * (size_t)e->S * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return LK_ERROR_NONE;
}
