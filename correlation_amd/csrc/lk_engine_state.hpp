// lk_engine_state.hpp - the state of the gfx950 Lucas-Kanade engine behind include/lk_engine.h, for the engine's own host units.
//
// What lives where (HBM layout, one engine per GPU):
//   images      3 slots (und, def, nxt) x (py_stop+1) levels, row-major u8, pitch = cols,
//               two zeroed guard rows per level.  2048^2: 4 MiB + 1 MiB + 256 KiB per slot.
//   sample lists per level L: one concatenated float2 array + uint32 offsets [S+1]
//               (level 0 = the ROI's samples in the CPU engine's order, level L = the
//               decimated list of pyramid_class.cpp:301-322).
//   sector state center[S] (float2), guess[S][6], last_p[S][6], prev_p[S][6],
//               result[S] (48 B, layout of CorrelationResult), stats[S][4].
//   rectangular sectors have no list at all: int4 {x_first, y_first, width, n} per level.
//   sequences   a ring of K deformed-frame pyramids + per-window records / counters / granule chain (frame-pipelined
//               windows: lk_correlate_sequence_async - every sector advances through the frames of a window on its own).
// Everything for an image pair is resident; lk_correlate_all* is one launch per size class
// (16 / 32 / 64 lanes, 4 / 8 wavefronts, teams) on one stream, preceded by the one-lane kernel
// and its finisher when the class has a starved pyramid level.
#pragma once
#include "lk_compose.hpp"
#include "lk_strain.hpp"
#include "lk_device.hpp"
#include "lk_internal.hpp"
#include "lk_launch.hpp"
#include "lk_roi.hpp"

#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#pragma GCC visibility push(hidden)

// roctx ranges where the reference has NVTX ranges (cuda_class.cu:133,277,310-326,497-511,528,554,
// cuda_polygon.cu:237,247, cuda_pyramid.cu:219,226): upload + pyramid, sector commit / rebuild,
// solve, record gather.  `rocprofv3 --marker-trace --kernel-trace` shows them over the kernels;
// without a profiler attached a push / pop pair is two calls into an empty table.
struct Range {
  explicit Range(const char *name) { (void)roctxRangePushA(name); }
  ~Range() { (void)roctxRangePop(); }
  Range(const Range &) = delete;
  Range &operator=(const Range &) = delete;
};

struct DevImage {
  uint8_t *lvl[LK_MAX_LEVELS] = {};
  size_t cap[LK_MAX_LEVELS] = {};
  int guard_rows[LK_MAX_LEVELS] = {-1, -1, -1, -1, -1, -1, -1, -1}; // geometry the guard rows were zeroed for
  int guard_cols[LK_MAX_LEVELS] = {-1, -1, -1, -1, -1, -1, -1, -1};
  int rows = 0, cols = 0;
  bool valid = false;
};

// floor(a / 2^l) and ceil(a / 2^l) for any sign
inline int floor_shift(int a, int l) { return a >> l; }
inline int ceil_shift(int a, int l) { return -((-a) >> l); }

// the levels the engine builds sample lists for: level 0 always; first, first + step, ... <= stop, each from the previous
inline std::vector<int> list_levels(const lk_config &cfg) {
  std::vector<int> levels{0};
  for (int l = cfg.py_start == 0 ? cfg.py_step : cfg.py_start; l <= cfg.py_stop; l += cfg.py_step) // pyramid_class.cpp:299
    levels.push_back(l);
  return levels;
}

struct HostSector {
  std::vector<float> xy; // level-0 AoS (empty for rectangular sectors: generated on demand)
  bool is_rect = false;
  int x0 = 0, y0 = 0, x1 = -1, y1 = -1; // inclusive rectangle (is_rect)
  float cx = 0.f, cy = 0.f;
  bool has_center = false; // the solve centre was given (rectangular path) rather than the samples' mean
  bool set = false;
  bool fresh = true; // registered (lk_set_sector_*) since the last commit: its sequence state starts from zero
  // Annular and blob sectors are registered by their DESCRIPTION; the sample list is made by the
  // device mask at commit (lk_roi_tile_kernel) or, on demand, by the host scan (realize()).
  int lazy = 0;      // 0: xy / rectangle are the sector; 1: annular geometry `ag`; 2: blob half triangles `flats`
  lkroi::AnnularGeometry ag;
  std::vector<lkroi::BlobPolygon::Flat> flats;
  int n0_device = 0; // lazy sectors after a device commit: their sample count
  int n0() const { return is_rect ? (x1 - x0 + 1) * (y1 - y0 + 1) : (lazy ? n0_device : (int)(xy.size() / 2)); }
  void realize() {   // the host scan of a lazily registered sector: same samples, same order
    if (!lazy)
      return;
    xy.clear();
    if (lazy == 1)
      lkroi::annular_points(ag, xy);
    else
      lkroi::BlobPolygon::fill(flats, xy);
    if (!xy.empty())
      lkroi::mean_center(xy.data(), (int)(xy.size() / 2), cx, cy); // correlation_class.cpp:337-339
    lazy = 0;
  }
  // the implicit rectangle at level l, {x_first, y_first, width, n}: the decimation rule of pyramid_class.cpp:301-322 applied to a
  // full rectangle keeps exactly the coordinates divisible by 2^l, i.e. another full rectangle, same order
  int4 rect_at(int l) const {
    const int xs = ceil_shift(x0, l), xe = floor_shift(x1, l), ys = ceil_shift(y0, l), ye = floor_shift(y1, l);
    const int w = std::max(0, xe - xs + 1), h = std::max(0, ye - ys + 1);
    return make_int4(xs, ys, std::max(w, 1), w * h);
  }
  std::vector<float> points() const { // level-0 list in the CPU engine's order
    if (!is_rect)
      return xy;
    std::vector<float> v;
    v.reserve(2 * (size_t)n0());
    lkroi::rect_points(x0, y0, x1, y1, v);
    return v;
  }
};

template <class T> struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t want) {
    if (want <= n && p)
      return hipSuccess;
    if (p)
      (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc((void **)&p, std::max<size_t>(want, 1) * sizeof(T));
    if (e == hipSuccess)
      n = want;
    return e;
  }
  // grow, keeping the first `keep` elements (a commit that adds sectors keeps the state of the others)
  hipError_t ensure_keep(size_t want, size_t keep) {
    if (want <= n && p)
      return hipSuccess;
    T *q = nullptr;
    hipError_t e = hipMalloc((void **)&q, std::max<size_t>(want, 1) * sizeof(T));
    if (e != hipSuccess)
      return e;
    if (p && keep)
      e = hipMemcpy(q, p, std::min(keep, n) * sizeof(T), hipMemcpyDeviceToDevice);
    if (p)
      (void)hipFree(p);
    p = q;
    n = want;
    return e;
  }
  // the same with room to spare (sector-by-sector registration: lk_commit_sectors' append path)
  hipError_t reserve_keep(size_t want, size_t keep) {
    if (want <= n && p)
      return hipSuccess;
    return ensure_keep(std::max(want, 2 * n + 64), keep);
  }
  void release() {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

// lanes that own one sector: a 16-lane DPP row (4 sectors per wavefront), one wavefront,
// a workgroup of 4 / 8 wavefronts, or - for giant sectors (a blob over most of the image) -
// a team of up to kMaxTeam 8-wavefront workgroups
constexpr int kNumClasses = 6;
constexpr int kTeamClass = 5;
constexpr int kGroupOfClass[kNumClasses] = {16, 32, 64, 256, 512, 512};
constexpr int kTeamSamples = 32768; // level-0 samples per workgroup of a team (64 per lane)
constexpr int kMaxTeam = kLkMaxTeam; // (256: config 3's blob alone 0.405 -> 0.372 ms against 128; the launch clamps a team to what is resident)
constexpr int kTeamMinSamples = 4096; // a team workgroup is worth its all-to-all from 8 samples per lane on
constexpr int kFewBigSectors = 128;   // at most this many 8-wavefront sectors: give them teams
inline int size_class(int n0) {
  return n0 <= 512 ? 0 : (n0 <= 2048 ? 1 : (n0 <= 8192 ? 2 : (n0 <= 65536 ? 3 : (n0 <= 8 * kTeamSamples ? 4 : 5))));
}

#pragma GCC visibility pop

// (Of default visibility, as before the engine had units: the library has always exported the few inline members of this
// struct that the compiler emits out of line, and the split leaves the exported set as it was.)
struct lk_engine {
  lk_config cfg{};
  int P = 0;
  hipStream_t own_stream = nullptr, stream = nullptr, nxt_stream = nullptr;
  hipEvent_t nxt_done = nullptr, ev_s0 = nullptr, ev_s1 = nullptr, ev_p0 = nullptr, ev_p1 = nullptr;
  // size classes are independent sector sets: every class after the first solves on its own
  // stream (forked from / joined into `stream`), so that one class's tail overlaps the others
  hipStream_t class_stream[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool nxt_pending = false, solve_timed = false, pyr_timed = false;
  bool batch_invariant = false; // lk_set_batch_invariant
  DevBuf<int> d_stale;          // reference-order mode: reached_iterations as the last solved sector left it ([2], alternating)
  int stale_par = 0;
  bool defer_stale = false;     // lk_group member: the markers are resolved over the gathered records, in global sector order
  int reference_order = 0;      // lk_set_reference_order: 0 = off, T = the reference's number_of_threads to reproduce
  int update = LK_UPDATE_FORWARD; // lk_set_update
  // backward mode (lk_backward.hip): the sectors by lane group (16 / 64 / 512 lanes, from the level-0 count alone), each
  // sector's first template slot (prefix of the level-0 counts) and the slots; rebuilt after every classify_sectors
  bool bw_dirty = true;
  std::vector<uint32_t> h_bw_order, h_bw_base;
  int bw_begin[4] = {0, 0, 0, 0};
  DevBuf<uint32_t> d_bw_order, d_bw_base;
  DevBuf<float4> d_bw_tpl;
  int stats_update = LK_UPDATE_FORWARD; // the mode of the solve the counters describe
  int pairs_in_flight = 1;      // lk_set_pairs_in_flight: launches that share the GPU
  bool timing = true; // HIP events around pyramid builds and solves (lk_stats.solve_ms / pyramid_ms)
  std::mutex nxt_mu;
  std::string err;

  DevImage img[3];
  LkLevelView h_lv[LK_MAX_LEVELS]{}, h_lv_sent[LK_MAX_LEVELS]{};
  DevBuf<LkLevelView> d_lv;
  bool lv_dirty = true;

  std::vector<HostSector> hs; // staging until commit
  std::vector<HostSector> hs_backup; // the lists before the last lk_translate / lk_rewarp_sectors
  bool committed = false;
  // Sector-by-sector registration (the reference's first-frame loop: resetPolygon(i), correlate(i),
  // manager_class.cpp:340, :449): a commit that only ADDS rectangles behind the committed ones appends them
  // (O(1) host work and one small launch per sector) instead of rebuilding everything; the size-class
  // analysis of the whole domain is then redone lazily, by the next batch solve.
  bool append_ok = false;     // the committed state can be extended in place (plain sectors, no pending rebuilds)
  bool classes_dirty = false; // h_order / class_begin / promotions are stale (sectors were appended)
  bool recommit_pending = false; // lk_update_sector moved sample lists: rebuild before the next solve
  // lk_rewarp_sectors rebuilds the lists on the device: hs[].xy / cx / cy are stale until a host
  // consumer asks for them (materialize_host); the previous level-0 lists stay in d_xy0_alt
  bool lists_on_device = false, backup_on_device = false;
  DevBuf<float2> d_xy0_alt;
  DevBuf<uint32_t> d_off0_alt, d_pos, d_tiles, d_level_total;
  DevBuf<LkRoiSector> d_roi_sectors; // device ROI masks (commit of annular / blob sectors)
  DevBuf<LkRoiFlat> d_roi_flats;
  DevBuf<uint32_t> d_roi_tile_begin;
  std::vector<float> h_center_prev, h_offsets;
  DevBuf<float2> d_offsets;
  int S = 0;
  std::vector<uint32_t> h_off[LK_MAX_LEVELS];
  DevBuf<float2> d_xy[LK_MAX_LEVELS];
  // the row-major evaluation copy of the lists (LkLevelView::xy_eval; same offsets): built with the device ROI masks
  // when the domain has annular sectors, dropped when the lists move (Lagrangian descriptions)
  DevBuf<float2> d_xy_eval[LK_MAX_LEVELS];
  DevBuf<uint32_t> d_off_eval;   // scratch: the offsets the second pass computes (equal to d_off)
  DevBuf<float2> d_xy_eval0_alt; // level 0 of the copy while the lists move (lk_rewarp_sectors)
  bool eval_lists = false;
  DevBuf<uint32_t> d_off[LK_MAX_LEVELS];
  DevBuf<int4> d_rect[LK_MAX_LEVELS];
  std::vector<int4> h_rect[LK_MAX_LEVELS];
  std::vector<float> h_center; // [S][2]
  DevBuf<float2> d_center;
  DevBuf<float> d_guess, d_last_p, d_prev_p, d_last_eval_p;
  DevBuf<lk_result> d_result;
  DevBuf<uint32_t> d_stats;
  DevBuf<uint32_t> d_order;
  std::vector<uint32_t> h_order; // sectors grouped by size class
  int class_begin[kNumClasses + 1] = {0, 0, 0, 0, 0, 0, 0};
  bool class_starved[kNumClasses] = {false, false, false, false, false, false}; // a sector of the class has a starved level
  int team_share_permille = 0; // > 0: the team class and the one-workgroup class of this domain split the resident slots (classify_sectors)
  bool force_safe = false; // LK_FORCE_SAFE: QR fallback for ill-conditioned systems in the lane-group kernels
  std::vector<int> h_class; // size class of every sector
  DevBuf<uint32_t> d_single, d_queue;
  DevBuf<LkHandoff> d_handoff;
  DevBuf<uint32_t> d_mid, d_finish_list, d_finish_count; // stragglers of the starved-level kernel
  DevBuf<uint32_t> d_ill_list, d_ill_count;              // sectors whose damped system met a bad pivot
  DevBuf<uint32_t> d_mean_scratch;                       // chunk table / sums / maps of lk_mean_center_int_kernel
  int starved_max = -1; // LK_STARVED_MAX as read by the last commit (-1: the default, 2 P; kStarvedNone: no level is starved)
  int eval_cap = 20; // evaluations a lane of the starved-level kernel spends on one sector (0: no cap; config 4: 12 / 16 / 20 / 24 / 32 -> 2.00 / 1.91 / 1.88 / 1.92 / 2.08 ms)
  int team_w = 0; // workgroups per sector of the team class
  int team_min_samples = 0; // per-sector team sizing (0: every team has team_w workgroups)
  DevBuf<float> d_team_partials;
  DevBuf<uint32_t> d_team_arrivals;
  DevBuf<float> d_scratch; // 64 floats for the stand-alone entry points
  DevBuf<float2> d_warp;
  DevBuf<lk_guess_match> d_gs_match; // lk_search_guesses: the matches of the last search
  int gs_count = 0;                  //   for this many sectors (0: no search yet)
  // Frame-pipelined windows (lk_correlate_sequence_async): a ring of resident deformed-frame pyramids, filled on the
  // next-frame stream, and the buffers of one window - records and counters per frame, the per-sector granule chain that
  // hands a sector's parameters from frame to frame, the per-frame image table, two flag words.
  std::vector<DevImage> ring;
  std::vector<hipEvent_t> ring_ready;   // per slot: its pyramid is built (recorded on nxt_stream)
  std::vector<char> ring_fresh;         // per slot: ring_ready has to be waited for by the next window that reads it
  std::vector<unsigned> ring_window;    // per slot: the last window that read it (+ 1; 0: none)
  hipEvent_t seq_done[4] = {nullptr, nullptr, nullptr, nullptr}; // recorded behind window w on the engine's stream: [w % 4]
  unsigned seq_windows = 0;             // windows launched so far
  uint64_t window_safe_reruns = 0;      // windows solved again with the SAFE flavour (lk_stats)
  DevBuf<lk_result> d_seq_result;       // [frames][S]
  DevBuf<uint32_t> d_seq_stats;         // [frames][S][4]
  DevBuf<float> d_seq_guess;            // [frames][S][6] (LK_SEQ_CHECK / tests)
  DevBuf<unsigned long long> d_seq_chain, d_seq_chain_safe; // (the SAFE pass behind the fast flavour has a chain of its own)
  DevBuf<LkSeqFrame> d_seq_img;
  DevBuf<uint32_t> d_seq_flags;         // [4]: wait bound hit, bad pivot in the fast flavour; wait bound hit in the SAFE pass
  DevBuf<float> d_prev_p_alt;           // previous_resulting_parameters as the window's last frame leaves them
  struct SeqWindow {
    int und_slot = -1, first_slot = 0, n_frames = 0, reference_previous = 0, velocity = 0, want_host = 0, want_guesses = 0;
    bool pipelined = false, outstanding = false;
  } seq;
  uint32_t *h_seq_flags = nullptr;      // pinned [4]
  lk_result *h_seq_results[2] = {nullptr, nullptr}; // pinned [frames][S], alternating by window: the caller may digest window w's
  size_t h_seq_results_n[2] = {0, 0};               //   records (lk_sequence_host_records) while window w + 1 is being solved
  int h_seq_cur = 0;                                // buffer of the window launched last
  hipEvent_t ev_seq = nullptr;
  int stats_frames = 1;                 // frames the counters of the last solve cover (a window: its frames)
  lk_result *h_results = nullptr; // pinned: where lk_correlate_all_async leaves the records
  size_t h_results_n = 0;
  hipEvent_t ev_results = nullptr;
  bool results_pending = false;
  bool stats_valid = false;
  lk_stats stats{};
  int records_S = 0;        // sectors the engine-held records of a batch solve cover (0: no solve since the commit)
  int window_S = 0;         // sectors the device records of the last window cover (0: no window since the commit; lk_track_points)
  LkPassSlot *pass[LK_PASS_COUNT] = {}; // what the add-on passes keep between their calls (lk_pass.hpp), deleted by lk_destroy
  // lk_get_launch_report: the launches of the most recent solving call, in the order the host issued them.  Fixed capacity:
  // a launch past it is counted and not kept (its record goes to the spare slot at the end).
  lk_launch_record launch_report[LK_LAUNCH_REPORT_CAPACITY + 1] = {};
  int launch_report_n = 0; // launches of the call so far (may exceed the capacity)
  void launch_report_begin() { launch_report_n = 0; }
  lk_launch_record *launch_report_slot() {
    const int i = launch_report_n++;
    return &launch_report[i < LK_LAUNCH_REPORT_CAPACITY ? i : LK_LAUNCH_REPORT_CAPACITY];
  }

  int fail(int code, const std::string &what) {
    err = what;
    return code;
  }
  int hipfail(hipError_t e, const char *where) {
    err = std::string(where) + ": " + hipGetErrorString(e);
    return LK_ERROR_DEVICE;
  }
};

#define HIPCHK(call)                                                                                  \
  do {                                                                                                \
    hipError_t _e = (call);                                                                           \
    if (_e != hipSuccess)                                                                             \
      return e->hipfail(_e, #call);                                                                   \
  } while (0)

#pragma GCC visibility push(hidden)

// Environment hooks, all through this one parse.  A hook read ONCE per process is a
//   static const int x = env_int("LK_X", fallback);
// a hook that tests flip between calls is a plain call at its site and is read again every time.
inline int env_int(const char *name, int fallback) {
  const char *f = std::getenv(name);
  return f ? std::atoi(f) : fallback;
}

// LK_STARVED_MAX=none: no level is starved - "at most -1 samples" - so that the lane groups solve every level themselves, a level
// without a sample included (tests/test_step_state_gpu.py)
constexpr int kStarvedNone = -2;
inline int starved_max(const lk_engine *e) { return e->starved_max == kStarvedNone ? -1 : e->starved_max >= 0 ? e->starved_max : 2 * e->P; }

inline int level0_count(const lk_engine *e, int s) { // samples of a sector at level 0, from the committed tables
  const int4 r = e->h_rect[0][(size_t)s];
  return r.z > 0 ? r.w : (int)(e->h_off[0][(size_t)s + 1] - e->h_off[0][(size_t)s]);
}

// What crosses the engine's units (hidden: none of it is part of the library's interface).
// lk_engine_images.cpp
bool host_pinned(const void *p);
int fill_image(lk_engine *e, DevImage &im, const void *src, bool src_on_device, int rows, int cols, int step, hipStream_t st,
               bool timed);
// lk_engine_sectors.cpp
int lists_from_device(lk_engine *e, const float2 *d_xy0, const std::vector<float> &centers, std::vector<HostSector> &out);
int materialize_host(lk_engine *e);
int refresh_starved(lk_engine *e);
int commit_impl(lk_engine *e, bool keep_state);
int recommit_if_pending(lk_engine *e);
int reclassify_if_dirty(lk_engine *e);
// lk_engine_solve.cpp
int refresh_level_views(lk_engine *e);
bool safe_flavour(const lk_engine *e);
LkSolveArgs base_args(lk_engine *e, const float *d_guess, lk_result *d_result);
int stale_iterations(lk_engine *e, lk_result *d_result, int n);
int bw_tables(lk_engine *e);
int reference_group_of_class(int c, int n);
int launch_all(lk_engine *e, const float *d_guess, lk_result *d_result, const LkSectorSet *set = nullptr);
hipError_t wait_event(hipEvent_t ev);
int solve_begin(lk_engine *e);
int solve_end(lk_engine *e, int stats_frames, int stats_update);
struct ClassFork {
  lk_engine *e;
  bool on;            // more than one class to launch (and LK_CLASS_STREAMS allows): they solve side by side
  int n_launched = 0; // classes joined so far: the first one stays on the engine's stream
  int open();
  int stream_of(int c, hipStream_t *st);
  int join(int c, hipStream_t st);
};

#pragma GCC visibility pop
