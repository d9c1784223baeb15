// lk_device.hpp - shared host/device structs of the gfx950 Lucas-Kanade engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lk_engine.h"

// One pyramid level as the solve kernel sees it.  Images are row-major u8 with
// pitch == cols (pyramid_class.cpp:153,177: step = cols) and two zeroed guard rows.
struct LkLevelView {
  const uint8_t *und;  // undeformed image, level L
  const uint8_t *def;  // deformed image, level L
  const float2 *xy;    // concatenated per-sector sample lists of level L (AoS x,y)
  const float2 *xy_eval; // the same lists with every sector's samples in row-major order (y outer, x inner), or null:
                         //     what the lane groups of the default mode walk - neighbouring lanes then read neighbouring
                         //     pixels of one image row.  The reference's order (x outer, y inner for annular sectors,
                         //     manager_class.cpp:907-918) puts 64 consecutive samples on 64 image rows: 64 cache lines
                         //     per load instruction.  Sums in the reference's order (starved levels, reference-order
                         //     mode) and the centres use `xy`.
  const uint32_t *off; // [S+1] start of each sector's list in xy
  const int4 *rect;    // [S] implicit rectangular sectors: {x_first, y_first, width, n} at this
                       //     level (the same sample SET as manager_class.cpp:1607-1611 + the
                       //     decimation of pyramid_class.cpp:301-322); width == 0 means
                       //     "use the explicit list"
  int urows, ucols;    // und dims at this level (rows0 >> L, pyramid_class.cpp:447-477)
  int drows, dcols;    // def dims
};

// What the starved-level kernel (one lane per sector) leaves for the lane-group kernel.
struct LkHandoff {
  float p[6];        // parameters in the scale of `level_old`
  int level;         // next pyramid level to solve; < py_start: the sector is finished
  int level_old;     // level the parameters are scaled for
  int reached;       // reached_iterations so far (correlation_class.cpp:452)
  uint32_t n_evals, n_sample_evals, n_point_iters;
};

// Frame-pipelined solve (lk_correlate_sequence*): the image pair of one frame of the window, level by level.
// The sample lists, rectangles and dimensions are those of LkLevelView (an Eulerian sequence: the sectors stay,
// only the images change from frame to frame).
struct LkSeqFrame {
  const uint8_t *und[LK_MAX_LEVELS];
  const uint8_t *def[LK_MAX_LEVELS];
};
// What one frame of a sector hands to the next: its returned parameters as six 8-byte granules {tag = frame + 1, float
// bits}, two slots per sector (frame parity) - one 128-byte line per sector.  A granule is written by ONE write-through
// store and read by write-through-aware loads; the tag is the flag, so no fence and no ordering between the six is needed
// (the consumer takes a value only when its tag is the frame it waits for).
constexpr int kLkSeqChainWords = 16; // uint64 per sector: [2 slots][8] (6 used)

constexpr int kLkMaxTeam = 256; // workgroups per team at most (the kernel stages a team's partial sums in LDS: 32 floats each)
constexpr int kLkMidWords = 32; // Cold (23) + p (6) + phase

struct LkSolveArgs {
  const LkLevelView *lv; // [LK_MAX_LEVELS] in device memory
  const float2 *center;  // [S] level-0 centre of each sector
  const float *guess;    // [S][6]
  lk_result *result;     // [S]
  float *last_p;         // [S][6] copy of the returned parameters (sequence state), may be null
  float *last_eval_p;    // [S][6] parameters of the LAST evaluation at level 0 - what CorrelationClass::getDefXY0
                         //   warps with (correlation_class.cpp:884-896); may be null
  uint32_t *stats;       // [S][4]: evaluations, sample evaluations, point iterations, -
  const uint32_t *order; // optional [n_sectors] indirection (size classes), may be null
  // teams: a giant sector is shared by team_w workgroups of the 512-thread kernel (0/1: off)
  int team_w;
  int team_min_samples;  // a sector's team has ceil(n0 / team_min_samples) workgroups (<= team_w)
  float *team_partials;  // [n_sectors][2][team_w][32]: per-workgroup sums, double-buffered by step parity
  uint32_t *team_arrivals; // [2][n_sectors]: monotonic arrival counters, then "team is broken" flags (zeroed per launch)
  int team_fault;          // test hook (LK_TEAM_FAULT = step): rank 1 of every team goes missing at that step
  // Stragglers of the starved-level kernel: after `eval_cap` evaluations a lane parks its sector
  // mid-level (kLkMidWords words of state) and appends it to `finish_list`; the 16-lane
  // finisher (`finisher` = 1) resumes it with reference-order sums spread over 16 lanes.
  int eval_cap;
  int finisher;
  int resume;              // 1: this launch takes its sectors, in the middle of a level, from finish_list
  // Fast-flavour kernels hand a sector whose damped system met a bad pivot to the SAFE 16-lane
  // kernel (resume = 1, the reference's QR) instead of zeroing that parameter's step:
  uint32_t *ill_list;      // [S] or null
  uint32_t *ill_count;     // [1]
  uint32_t *mid_state;    // [S][kLkMidWords]
  uint32_t *finish_list;  // [S]
  uint32_t *finish_count; // [1], zeroed before the starved-level kernel
  LkHandoff *handoff;    // [S] written by the starved-level kernel, read by the others (may be null)
  uint32_t *queue;       // next unclaimed slot of this launch (persistent mode), zeroed per launch
  int n_sectors;         // sectors in this launch
  int chunk;             // non-persistent: ceil(#workgroups / 8), XCD-contiguous chunk length
  int align;             // 1: the sectors of a wavefront (16/32-lane groups) descend the pyramid together
  int solo;              // 1: an idle half-wavefront may join its partner's sector (32-lane groups)
  int safe;              // 1: reference-exact handling of starved / ill-conditioned levels
  int reference_order;   // T > 0 (SAFE 16- / 64-lane kernels): every level with the reference's summation order for
                         //   number_of_threads = T and its QR - bit-identical records (lk_set_reference_order)
  int mark_stale;        // reference-order mode (any instance of its launch chain): a sector whose very first evaluation fails
                         //   reports the stale-iteration marker instead of 0 (lk_stale_iterations_kernel resolves it)
  int persistent;        // 1: groups pull sectors from `queue`; 0: one sector per group by position
  int rows_used;         // positional launches of 16-lane rows: rows of a wavefront that get a sector (0 / 4: all; 3, 2: the
                         //   reference-order rows deal the idle rows' lanes to the wavefront's sectors)
  int starved_max;       // a level with at most this many samples is "starved" (default 2 P)
  int keep_sums;         // 1 (default): a rejected trip continues from the kept sums of the last good parameters;
                         //   0 (LK_KEEP_SUMS=0, tests): it evaluates there again, as the reference does - same records
  int gpu_share;         // launches that may hold the GPU at the same time (>= 1): bounds a team launch's width
  int slots_permille;    // 0: the launch may use every resident workgroup slot; else its share of them in 1/1000 - the
                         //   team class and the one-workgroup class of one batch split the chip so that both are resident
                         //   at once (a team launch: bounds its width; the one-workgroup class: a persistent grid of that size)
  int py_start, py_step, py_stop;
  float precision;
  int max_iters;
  // Frame-pipelined solve of a sequence window (the SEQ instances): seq_frames > 0.  Tickets of the persistent queue
  // are (frame, sector) pairs drawn FRAME-MAJOR (ticket t: frame t / n_sectors, sector order[t % n_sectors]); the group
  // that draws (f, s) waits - without blocking the other sectors of its wavefront - until frame f - 1 of sector s has
  // published its parameters, forms the guess of managerClass::adjust_initial_guess (manager_class.cpp:2677-2699) from
  // them, solves, writes result[f * seq_stride + s] and publishes in turn.  Every wait targets a ticket that was drawn
  // earlier, i.e. one a running or finished wavefront holds: the grid drains whatever is resident.
  int seq_frames;
  int seq_velocity;             // 1: guess = 2 p(f-1) - p(f-2) (Eulerian description, first image as the reference), 0: p(f-1)
  int seq_stride;               // records per frame in `result` / `stats` / `seq_guess_out` (the engine's sector count)
  const LkSeqFrame *seq_img;    // [seq_frames]
  unsigned long long *seq_chain; // [S][kLkSeqChainWords] granules, zeroed before the launch
  const float *seq_prev_p;      // [S][6] previous_resulting_parameters before the window (p(f-2) of the window's frame 1)
  float *seq_prev_p_out;        // [S][6] ... and after it (written by the window's last frame; a buffer of its own)
  float *seq_guess_out;         // optional [seq_frames][seq_stride][6]: the guesses the frames were solved from
  uint32_t *seq_flags;          // [0]: a wait ran into its bound (the launch is void); [1]: a fast-flavour solve met a bad pivot
  const uint32_t *seq_gate;     // the SAFE pass behind a window's fast flavour: that pass's seq_flags[1] - the launch does
                                //   nothing while it is 0 (nullptr: no gate)
  int seq_fault;                // test hook (LK_SEQ_FAULT = f + 1): frame f of the launch's first sector never publishes - the bounded wait's exit
  int slot_step;                // test hook (LK_STEP_STATE=0), fast 32-lane instance of the six-parameter models: 1 = every step moves the whole
                                //   cold slot through LDS (the earlier form of the step, kept for the side-by-side test) - same records
};

// ROI -> level-0 sample lists on the device (cudaPolygon's mask + compaction, cuda_polygon.cuh:180-292,
// cuda_polygon.cu:589-627, with the CPU engine's predicates and sample order: SURVEY.md 8a-a10).
// The work is cut into TILES whose outputs are consecutive in the final list:
//   annular sector  candidates = the bounding box walked x outer / y inner (manager_class.cpp:902-925),
//                   1024 candidates per tile, the predicate (:907-918) keeps some of them;
//   blob sector     one tile per scan line of each flat-sided half triangle, in the ear clipper's
//                   order (polygon_class.cpp:283-403); every pixel of the line is kept.
struct LkRoiSector {
  int kind;               // 0 annular, 1 blob
  int x0, y0, x1, y1;     // annular: candidates fx in [x0, x1), j in [y0, y1)
  float cx, cy, ri2, ro2; // annular: centre, squared radii
  float q00x, q01x, q10x, q11x, q00y, q01y, q10y, q11y; // annular: wedge corners (outer ones with the 1.2 "sag")
  int as;                 // annular: 1 = full ring (no wedge test)
  int flat_begin, flat_count; // blob: its half triangles in the flat table
};
struct LkRoiFlat { // one flat-sided half triangle: rows j0 .. j1-1, pixels ceil(ls*j+li) .. ceil(rs*j+ri)-1
  float ls, li, rs, ri;
  int j0, j1;
  int row_begin; // index of its first scan line among the sector's tiles
};
constexpr int kLkRoiTile = 1024;

struct LkRewarpArgs { // level-0 sample lists moved by the last level-0 evaluation's parameters (or by an offset)
  const float2 *src_xy;    // lists before (explicit sectors)
  const uint32_t *src_off; // [S+1]
  const int4 *src_rect;    // [S] implicit rectangles before (width 0: explicit)
  const uint32_t *dst_off; // [S+1] prefix of the level-0 counts: every sector explicit afterwards
  float2 *dst_xy;
  const float2 *center;    // [S] centres of the last solve
  const float *p;          // [S][6]
  const float2 *offset;    // [S] Lagrangian description: samples move by add_pair(offset) instead of the warp
  int n_sectors;
  uint32_t total;          // dst_off[S]
  int rows;                // 1: an implicit rectangle is walked row by row (y outer, x inner) - the evaluation copy of the lists
};

// One rectangular sector appended behind the committed ones (lk_commit_sectors' fast path): everything the
// device needs to know about it travels in the kernel arguments.
struct LkAppendArgs {
  int sector, n_levels;
  int keep_state; // 1: a committed rectangle that moved (lk_update_sector): rectangles and centre only
  float2 center;
  float2 *d_center;
  float *d_guess, *d_last_p, *d_prev_p, *d_last_eval_p; // [S][6] sequence state: zeroed
  lk_result *d_result;                                   // [S]: zeroed
  uint32_t *d_stats;                                     // [S][4]: zeroed
  int4 rect[LK_MAX_LEVELS];        // per committed level (in list order): the sector's implicit rectangle
  uint32_t off_end[LK_MAX_LEVELS]; //   and off[sector + 1] (= off[sector]: a rectangle has no list entries)
  int4 *d_rect[LK_MAX_LEVELS];
  uint32_t *d_off[LK_MAX_LEVELS];
};

struct LkEvalArgs { // stand-alone evaluation (known-answer tests)
  const LkLevelView *lv;
  const float2 *center;
  int sector, level;
  float p[6];
  float *out; // [36 + 6 + 1 + 1]: A row-major 6x6 (upper), b, chi, error
  int ref_threads; // > 0: the reference's summation order for number_of_threads = ref_threads (evaluate_ordered)
};

// Automatic initial guess (lk_guess_search.hip): one workgroup per sector.
struct LkGuessSearchArgs {
  const uint8_t *und, *def; // level-L images, pitch == cols
  int urows, ucols, drows, dcols;
  const float2 *xy;         // level-L lists, [S+1] offsets, [S] implicit rectangles (LkLevelView)
  const uint32_t *off;
  const int4 *rect;
  float *guess;             // [S][6] in: centres; out: the winners of OK sectors (g[0], g[1] only)
  float *prev_p;            // [S][6] out: = guess (the frame-0 rule's previous_resulting_parameters)
  lk_guess_match *match;    // [S]
  int n_sectors, level, radius, has_v, min_samples;
  float min_score;
  int win_bytes;            // LDS bytes for the staged deformed window (a larger window is read from global memory)
};
constexpr int kLkGsThreads = 256;
constexpr int kLkGsChunk = 1024; // template samples staged in LDS at a time (uint32 partial sums per chunk are exact)

// Rotation-aware automatic guess (lk_rotated_search.hip): one workgroup per (sector, angle) writes an LkRotAngleRecord, one
// lane group per sector reduces them to an lk_rotated_match, the guess and the profile.
struct LkRotAngleRecord { // 32 bytes
  double best, runner_up; // -2 where there is none
  int shift_x, shift_y, n_valid, status; // status: LK_GS_* of this angle alone, LK_GS_OK where it has a scored candidate
};
struct LkRotatedSearchArgs {
  LkGuessSearchArgs gs;      // images, lists, guesses, history, level, radius, min_samples, min_score, win_bytes (match unused)
  const float2 *center;      // [S] the committed level-0 centres
  const float2 *cos_sin;     // [n_angles] {c_k, s_k}, the table of lk_rotation_table
  LkRotAngleRecord *angle;   // [S][n_angles]
  double *profile;           // [S][n_angles] best score per angle, -2 where an angle has none
  lk_rotated_match *match;   // [S]
  int n_angles, model;
  double angle_center, angle_step;
};
constexpr int kLkRsReduceThreads = 64; // lanes of the reduce kernel's group

// Stereo guess along the epipolar curve (lk_epipolar_search.hip): one workgroup per (sector, run) scores a run of stations that
// share one template map - with shape = 1 the stations of one node, run k being node k's; with shape = 0, where every station
// shares the identity, a stretch of the curve - and writes an LkEpNodeRecord and its stations' part of the profile; one lane
// group per sector reduces the records to an lk_epipolar_match and the guess.
struct LkEpNodeRecord { // 32 bytes
  double best;          // -2 where the run has no scored candidate
  int station, band_offset, n_valid; // the run's winner: m (of the sector's curve) and b
  int status;           // -1: the run is empty; else LK_GS_* of the sector's template, LK_GS_NO_CANDIDATE or LK_GS_OK
  int pad[2];
};
struct LkEpipolarSearchArgs {
  LkGuessSearchArgs gs;           // images, lists, guesses, history, level, radius (the band), min_samples, min_score, win_bytes
  const float2 *center;           // [S] the committed level-0 centres
  const lk_epipolar_curve *curve; // [S] lk_epipolar_curves' table
  const int32_t *other;           // [stations] of all sectors, a curve's at its first_index
  const int32_t *node;            // [stations]
  const double *inv_depth;        // [stations]
  const float4 *shape;            // [S][n_nodes] {a11, a12, a21, a22} (shape = 1)
  const int2 *run;                // [S][n_runs] {first m, stations} of a run on its sector's curve (no stations: none)
  LkEpNodeRecord *rec;            // [S][n_runs]
  double *profile;                // [stations]
  lk_epipolar_match *match;       // [S]
  int n_nodes, n_runs, with_shape; // with_shape: n_runs == n_nodes
  int max_run, max_cand;          // the longest run of the launch in stations and in candidates: sizes the dynamic LDS
};

// Backward (inverse-compositional) update (lk_backward.hip, lk_set_update): one lane group per sector for its whole
// coarse-to-fine solve.  The group is chosen from the sector's level-0 sample count alone (kLkBwGroup*), so that a
// sector's record does not depend on what else is solved with it.
struct LkBackwardArgs {
  const LkLevelView *lv;  // [LK_MAX_LEVELS] in device memory
  const float2 *center;   // [S] level-0 centre of each sector
  const float *guess;     // [S][6]
  lk_result *result;      // [S]
  float *last_p;          // [S][6] or null
  float *last_eval_p;     // [S][6] or null
  uint32_t *stats;        // [S][4] or null
  const uint32_t *order;  // [n_sectors] the sectors of this launch
  float4 *tpl;            // template slots {T, dT/dx, dT/dy, 0}: a sector's level-L samples at tpl[tpl_base[s] + k]
  const uint32_t *tpl_base; // [S] prefix of the level-0 counts
  int n_sectors;
  int py_start, py_step, py_stop;
  float precision;
  int max_iters;
  int starved_max;
};
struct LkBackwardEvalArgs { // lk_evaluate_backward: template pass + one evaluation of one sector
  const LkLevelView *lv;
  const float2 *center;
  float4 *tpl;
  int sector, level;
  float p[6];
  float *out; // [36 + 6 + 1 + 1]: H row-major 6x6 (full), b, chi, error
};
constexpr int kLkBwSmall = 512;   // level-0 samples up to which a 16-lane row owns a sector
constexpr int kLkBwMedium = 8192; // ... a wavefront; above: a 512-thread workgroup
__host__ __device__ inline int lk_bw_group(int n0) { return n0 <= kLkBwSmall ? 16 : n0 <= kLkBwMedium ? 64 : 512; }

// Recovery of failed sectors (lk_reseed.hip, include/lk_engine.h: lk_reseed_failed): the uniform cell grid over the sector
// centres and the per-sector words of one call.
struct LkReseedGrid {
  double x0, y0, cell; // origin (the centres' minimum) and cell size (>= radius)
  int nx, ny;          // cells; cell index = iy * nx + ix, so the cells ix - 1 .. ix + 1 of a row are neighbours in memory
  const uint32_t *start;   // [nx * ny + 1] first member of each cell
  const uint32_t *members; // [S] sector indices, ascending within a cell
  const uint32_t *cell_of; // [S]
};
struct LkReseedPlanArgs {
  LkReseedGrid grid;
  const float2 *center;    // [S]
  const lk_result *rec;    // [S] the records the neighbours' parameters are read from
  const uint8_t *good;     // [S]
  const int32_t *tried;    // [S] good neighbours behind the last guess that was tried (0: none)
  float *guess;            // [S][6] out, for the sectors to retry
  int32_t *nbrs;           // [S] out: good neighbours found (failed sectors)
  uint8_t *retry;          // [S] out: 1 = solve this sector in this round
  lk_reseed_info *plan_info; // lk_reseed_plan: status / neighbours of every sector (else null)
  int n_sectors, model, min_neighbours;
  double radius;
};
struct LkReseedRange { // one class's range of an order table: src[begin .. end) -> the flagged ones to dst[begin ..], in order
  const uint32_t *src;
  uint32_t *dst;
  int begin, end;
};
constexpr int kLkReseedRanges = 9; // six size classes + the backward mode's three lane-group ranges
struct LkReseedCompactArgs {
  LkReseedRange range[kLkReseedRanges];
  const uint8_t *retry; // [S]
  uint32_t *count;      // [kLkReseedRanges]
};
struct LkReseedMergeArgs {
  const uint8_t *retry;      // [S] the sectors this round solved
  uint8_t *good;             // [S]
  int32_t *tried;            // [S]
  const int32_t *nbrs;       // [S]
  const lk_result *fresh;    // [S] the retry's records
  lk_result *rec;            // [S] the engine-held records
  float *last_p, *last_eval_p;            // [S][6] as the retry left them; restored from the copies for a rejected sector
  const float *keep_last_p, *keep_last_eval_p;
  uint32_t *stats;           // [S][4] likewise
  const uint32_t *keep_stats;
  lk_reseed_info *info;      // [S]
  unsigned long long *totals; // [6]: retry solves, their four counters summed, sectors recovered
  int n_sectors, n_params, round;
  float chi_max;
};
constexpr int kLkReseedGroup = 16; // lanes per failed sector of the planning kernel

// Strain field (lk_strain.hip, include/lk_engine.h: lk_strain_field): a windowed plane fit of (u, v) over the good sectors
// within `radius` of each sector, on the recovery pass's cell grid.
struct LkStrainArgs {
  LkReseedGrid grid;
  const float2 *center;  // [S]
  const lk_result *rec;  // [S]
  const uint8_t *good;   // [S] the good rule, evaluated once per call (lk_pack_prep_kernel)
  const float4 *pack;    // [S] {cx, cy, u, v} of a good sector, cx = NaN for a failed one (the packed variants)
  lk_strain *out;        // [S]
  int n_sectors, has_v, min_neighbours, tensor;
  double radius;
};

// Material-point tracks (lk_track.hip, include/lk_engine.h: lk_track_points): the windowed plane fit of lk_strain_field at the
// points' own positions, frame after frame of one call, on the recovery pass's cell grid.
struct LkTrackArgs {
  LkReseedGrid grid;     // over the centres: the same in every frame of the call
  const float4 *pack;    // [F][S] {cx, cy, u, v} of a good sector, cx = NaN for one that is not (lk_pack_prep_kernel)
  double *state;         // [Q][8] {X, Y, x, y, Fxx, Fxy, Fyx, Fyy}: read before frame 0, written after the last frame
  lk_track *out;         // [F][Q]
  int n_points, n_frames, n_sectors, min_neighbours, tensor, mode;
  double radius;
};

// Global motion per frame (lk_motion.hip, include/lk_engine.h: lk_rigid_motion): the sums of every frame's fit set in
// chunks of `chunk` sectors, the fit of lk_motion.hpp, the residuals to it, and the records with the motion taken out.
struct LkMotionFit;
constexpr int kLkMotionPartial = 14; // doubles of a chunk: {n, the 11 sums, sectors trimmed, 0}, or {sum r^2, max r^2, 0 ...}
struct LkMotionArgs {
  const float4 *pack;      // [F][S] {cx, cy, u, v} of a good sector, cx = NaN for one that is not (lk_pack_prep_kernel)
  const uint8_t *fit_mask; // [S] or null
  uint8_t *keep;           // [F][S] 1: the sector is in the fit set of the running pass (sums kernel -> residual kernel)
  double *partial;         // [F][chunks][kLkMotionPartial]
  double *sums;            // [F][12] {n, the 11 sums} of the last pass that ran
  LkMotionFit *fit;        // [F] the running pass's fit in double; the sums kernel of the next pass trims against it
  lk_motion *out;          // [F]
  const lk_result *rec;    // [F][S] the removal's input
  const float2 *center;    // [S]
  lk_result *rec_out;      // [F][S]
  int n_frames, n_sectors, chunk, chunks, kind, min_sectors, model, pass;
  double ox, oy;           // the origin of the sums: the centre of the centres' bounding box
  double reject;           // (double)cfg->reject; <= 0: no trimming
};

// Lens distortion (lk_lens.hip, include/lk_engine.h: lk_lens_fit, lk_lens_correct).  The fit: every frame's sums of the rows
// of lk_lens.hpp in chunks of `chunk` sectors, then the chunks joined; the correction: a thread per (frame, sector).
struct LkLensFitArgs {
  const float4 *pack;      // [F][S] {cx, cy, u, v} of a good sector, cx = NaN for one that is not (lk_pack_prep_kernel)
  const uint8_t *fit_mask; // [S] or null
  const double *nuisance;  // [F][6] the frames' nuisance parameters of this evaluation
  double *partial;         // [F][chunks][len]
  double *sums;            // [F][len], len = lk_lens_sums_len(Q): {n, the triangle, n_outside}
  lk_lens lens;
  int n_frames, n_sectors, chunk, chunks, nuisance_kind;
  double ox, oy;           // o of the nuisance: the centre of the centres' bounding box
};
struct LkLensCorrectArgs {
  const float4 *pack;      // [F][S] as above: the good rule, evaluated once per record
  const lk_result *rec;    // [F][S]
  const float2 *center;    // [S]
  lk_result *rec_out;      // [F][S]
  float2 *centres_out;     // [S] U(X)
  uint8_t *status;         // [F][S]
  lk_lens lens;
  int n_frames, n_sectors, model;
};

// A two-camera rig (lk_stereo.hip, include/lk_engine.h: lk_stereo_points, lk_stereo_strain).
struct LkStereoRig {       // what a kernel reads of a rig: the two cameras and F, formed once on the host
  lk_camera cam[2];
  double F[9];
};
struct LkStereoPointsArgs { // a thread per (frame, sector), the reference state as the first frame of `out`
  LkStereoRig rig;
  const float2 *center;    // [S]
  const lk_result *ref1;   // [S]
  const lk_result *rec0;   // [F][S] (null with n_frames = 0, as rec1)
  const lk_result *rec1;   // [F][S]
  lk_stereo_point *out;    // [1 + F][S]: the reference state, then the frames
  int n_frames, n_sectors, model;
  float chi_max;
};
struct LkStereoStrainArgs { // a lane group per (frame, sector) on the recovery pass's cell grid
  LkReseedGrid grid;
  const float2 *center;         // [S]
  const lk_stereo_point *ref;   // [S]
  const lk_stereo_point *pts;   // [F][S]
  lk_stereo_surface *out;       // [F][S]
  int n_frames, n_sectors, min_neighbours;
  double radius;
};

// Outlier flags (lk_outlier.hip, include/lk_engine.h: lk_flag_outliers): one pass of the (detrended) normalised median test.
struct LkOutlierArgs {
  LkReseedGrid grid;
  const float2 *center;  // [S]
  const uint8_t *good;   // [S] the good rule, evaluated once per call (lk_pack_prep_kernel)
  const float4 *pack;    // [S] {cx, cy, u, v}; cx = NaN for a sector that is not good or was flagged in the pass before
  lk_outlier *out;       // [S]
  int n_sectors, min_neighbours, detrend;
  int lds_rows;          // floats of a component a lane may stash (0 .. kLkOutlierRows); a fuller window is re-walked
  float eps, threshold;
  double radius;
};
constexpr int kLkOutlierRows = 16;

// What a pass that evaluates every sector once at its record's parameters reads (lk_sector_eval.hpp; filled from the
// engine's view by lk_pass_sector_eval, lk_pass.hpp): the images, lists and rectangles of one pyramid level - the finest
// level the solve reaches - under LkLevelView's names (`def` may be a ring slot's pyramid), the centres, the records, and
// the sectors of one launch.
struct LkSectorEvalArgs {
  const uint8_t *und, *def; // level-L images, pitch == cols
  int urows, ucols, drows, dcols;
  const float2 *xy;         // level-L lists in the reference's order, [S+1] offsets, [S] implicit rectangles
  const uint32_t *off;
  const int4 *rect;
  const float2 *center;     // [S] level-0 centres
  const lk_result *rec;     // [S]
  const uint32_t *order;    // [n_sectors] the sectors of this launch (one lane group's)
};

// Per-sector uncertainty (lk_uncertainty.hip, include/lk_engine.h: lk_parameter_uncertainty).
struct LkUncertaintyArgs {
  LkSectorEvalArgs ev;
  lk_uncertainty *out;      // [S]
  double *sums;             // [S][28] or null: A (upper triangle, row-major), b, chi in the layout of Sums<P>, then zeros
  int n_sectors, level;
};

// Photometry (lk_residual.hip, include/lk_engine.h: lk_photometry): the same walk with the grey-value sums instead of the
// normal matrix, over the good sectors.
struct LkPhotometryArgs {
  LkSectorEvalArgs ev;
  struct lk_photometry *out; // [S]
  double *sums;             // [S][8] or null (lk_residual.hpp: kLkPhotoSums)
  int n_sectors, level;
  float chi_max;
};

// ZNSSD refinement (lk_znssd.hip, include/lk_engine.h: lk_refine_znssd): the same walk inside a Levenberg-Marquardt loop
// per lane group, from records (ev.rec) or from guesses.
struct LkZnssdArgs {
  LkSectorEvalArgs ev;      // ev.rec: [S] the seed records, read when guess is null
  const float *guess;       // [S][6] level-0 seeds or null
  const int32_t *count0;    // [S] level-0 sample counts (the records' numberOfPoints)
  lk_result *rec_out;       // [S]
  struct lk_znssd *out;     // [S]
  double *sums;             // [S][45] or null (lk_znssd.hpp: kLkZnSums)
  int n_sectors, level, max_iters;
  float chi_max, precision, lambda0;
};

// B-spline refinement (lk_spline.hip, include/lk_engine.h: lk_refine_spline): the ZNSSD pass's arguments and the coefficient
// image its sampler reads in place of zn.ev.def.
struct LkSplineArgs {
  LkZnssdArgs zn;
  const float *coef;        // [zn.ev.drows][zn.ev.dcols]
};

// Weighted refinement (lk_weighted.hip, include/lk_engine.h: lk_refine_weighted): the ZNSSD pass's arguments (zn.out is not
// used), the mask over the undeformed level image and the window.
struct LkWeightedArgs {
  LkZnssdArgs zn;
  const uint8_t *mask;      // [zn.ev.urows][zn.ev.ucols], nonzero = use, or null: every pixel
  struct lk_weighted *out;  // [S]
  float inv;                // log2(e) / (2 sigma_L^2), or 0: no window
  float min_fraction;
};

// Second-order refinement (lk_quadratic.hip, include/lk_engine.h: lk_refine_quadratic): the ZNSSD pass's loop on twelve
// parameters; the engine's model only says how a seed is read and a record written.
struct LkQuadraticArgs {
  LkSectorEvalArgs ev;      // ev.rec: [S] the seed records, read when guess is null
  const float *guess;       // [S][6] level-0 seeds in the engine model's meaning, or null
  const float *second;      // [S][6] level-0 second-order seeds, or null: zeros
  const int32_t *count0;    // [S] level-0 sample counts (the records' numberOfPoints)
  lk_result *rec_out;       // [S]
  struct lk_quadratic *out; // [S]
  double *sums;             // [S][88] or null (lk_quadratic.hpp: kLkQdSums)
  int n_sectors, level, max_iters, model;
  float chi_max, precision, lambda0;
};

// Composed refinement (lk_composed.hip, include/lk_engine.h: lk_refine_composed).  Order 1: the weighted pass's arguments -
// wt.out takes the info, widened to struct lk_composed afterwards - and the coefficient image of a spline sampler.
struct LkComposedFirstArgs {
  LkWeightedArgs wt;
  const float *coef;        // [wt.zn.ev.drows][wt.zn.ev.dcols]
};
// Order 2: the second-order pass's arguments (qd.out is not used), the coefficient image of a spline sampler or null, the
// mask and the window as LkWeightedArgs.
struct LkComposedSecondArgs {
  LkQuadraticArgs qd;
  const float *coef;        // [qd.ev.drows][qd.ev.dcols] or null: the engine's interpolator
  const uint8_t *mask;      // [qd.ev.urows][qd.ev.ucols], nonzero = use, or null: every pixel
  struct lk_composed *out;  // [S]
  float inv;                // log2(e) / (2 sigma_L^2), or 0: no window
  float min_fraction;
};

// Residual map (lk_residual.hip, include/lk_engine.h: lk_residual_map): what a pixel needs of a sector, 48 bytes.
struct LkMapSector {
  float cx0, cy0; // level-0 centre; cx0 = NaN for a sector that is not good (it then fails the distance test by itself)
  float cx, cy;   // level-L centre, as the solve scales it
  float p[6];     // level-L parameters (translate<>), zeros behind the model's P
  float pad[2];
};
struct LkResidualMapArgs {
  LkReseedGrid grid;         // over the level-0 centres, cell = radius
  const uint8_t *und, *def;  // level-L images, pitch == cols
  int urows, ucols, drows, dcols;
  const LkMapSector *pack;   // [S]
  float *warped, *residual;  // [h][w] of the window, each may be null
  int32_t *owner;
  uint32_t *fallback;        // [1] tiles whose candidates did not fit into LDS (zeroed before the launch)
  int n_sectors, level;
  int x0, y0, w, h;          // the window in level-L pixels, inside the undeformed image
  int tiles_x;
  double r2;                 // (double)radius squared
};
constexpr int kLkMapTileW = 32, kLkMapTileH = 8; // pixels per workgroup: x fastest, a wavefront covers two rows of 32

// Field map (lk_field.hip, include/lk_engine.h: lk_field_map): the windowed plane fit at the nodes of a regular grid, a
// thread per node, in tiles of kLkMapTileW x kLkMapTileH nodes.
struct LkFieldArgs {
  LkReseedGrid grid;         // over the level-0 centres, cell = radius
  const float4 *pack;        // [S] {cx, cy, u, v} of a good sector, cx = NaN for one that is not (lk_pack_prep_kernel)
  float *maps;               // [C][ny][nx], the selected channels in ascending bit order; null when channels == 0
  int32_t *neighbours;       // [ny][nx] or null
  uint8_t *status;           // [ny][nx] or null
  uint32_t *fallback;        // [1] tiles whose candidates were not staged in LDS (zeroed before the launch)
  int n_sectors, min_neighbours, tensor, iterations;
  int x0, y0, nx, ny, stride; // node (i, j) is the level-0 position (x0 + i stride, y0 + j stride)
  int tiles_x;
  int walk;                  // != 0: no tile stages (the LK_FIELD_WALK hook)
  uint32_t channels;
  double r2;                 // (double)radius squared
};

// Speckle quality (lk_pattern.hip, include/lk_engine.h: lk_pattern_quality, lk_suggest_subset).  The sector pass walks the
// level-L lists over ONE image slot (ev.und = ev.def = that image; ev.rec is not read).
struct LkPatternArgs {
  LkSectorEvalArgs ev;
  struct lk_pattern *out;   // [S]
  long long *sums;          // [S][9] or null (lk_pattern.hpp: kLkPatternSums)
  double *mig_sum;          // [S] or null
  int n_sectors, level;
  int grey_low, grey_high;
  float noise_sigma, max_saturated;
};
// The summed-area tables of gx2^2 and gy2^2 over a whole level-L image: two uint32 planes of rows x pitch words that wrap,
// plane 1 (gy2^2) behind plane 0.  pitch = cols rounded up to 4, so that a thread's four columns are one aligned 16-byte
// access; the columns behind cols repeat the row's total.
constexpr int kLkSatThreads = 256;                           // row step: threads of the workgroup that owns an image row
constexpr int kLkSatPixels = 4;                              //   consecutive pixels per thread
constexpr int kLkSatRowTile = kLkSatThreads * kLkSatPixels;  //   pixels per pass of the workgroup; a longer row carries on
constexpr int kLkSatBandRows = 32;                           // column step: rows per band
constexpr int kLkSatColThreads = 64;                         //   a wavefront per band and 256 columns, four columns per lane
struct LkSatArgs {
  const uint8_t *img;       // level-L image, pitch == cols
  int rows, cols, pitch;
  uint32_t *table;          // [2][rows][pitch]
  uint32_t *band;           // [2][n_bands][pitch] band totals, then their exclusive prefix over the bands
  int n_bands;
};
struct LkSubsetArgs {
  const uint32_t *table;    // [2][rows][pitch]
  int rows, cols, pitch;
  const float2 *points;     // [n_points] level-L positions
  struct lk_subset *out;    // [n_points]
  uint32_t *sums;           // [n_points][n_cand][2] or null: Gxx, Gyy of every candidate box
  int n_points, n_cand, half_min, half_step;
  uint32_t threshold;       // T = ceil(4 sssig_min)
  float noise_sigma;
};

// Camera noise (lk_noise.hip, include/lk_engine.h: lk_camera_noise, lk_sector_noise; the arithmetic is lk_noise.hpp).
// The K frames are level-L images of one geometry, each its own allocation (16-byte aligned), pitch == cols.
struct LkNoiseFrameArgs {
  const uint8_t *frame[LK_NOISE_MAX_FRAMES]; // the first n_frames are read
  const uint8_t *mask;         // [rows][cols] (16-byte aligned), nonzero = use, or null: every pixel
  int n_frames, rows, cols;
  int x0, y0, w, h;            // the region, inside the frame
  unsigned long long *bins;    // [256][2] {count, sum q}, zeroed before the launch
  unsigned long long *frame_sums; // [n_frames], zeroed before the launch
};
struct LkNoiseSectorArgs {
  LkSectorEvalArgs ev;         // und = def = frame[0] with the frames' dimensions; rec is not read
  const uint8_t *frame[LK_NOISE_MAX_FRAMES];
  long long *sums;             // [S][3] n, sum q, sum s1
  int n_frames, n_sectors, level;
};
