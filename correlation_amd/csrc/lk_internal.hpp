// lk_internal.hpp - what lk_group.cpp needs from the engine and the kernels beyond the public C-ABI
// (same shared library; nothing here is part of include/*.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lk_engine.h"

// Reference-order mode inside a group: a member engine leaves the "stale iteration count" markers of its
// records unresolved (see lk_stale_iterations_kernel); the group resolves them over the gathered records in
// GLOBAL sector order with one group-level carry, so that a shard whose first sectors fail their very
// first evaluation reports what the last sector of the shard before it left behind - as the serial
// reference does (correlation_class.cpp:413-419, :870; lk_launch.hpp: lk_launch_stale_iterations_blocks / _window).
int lk_internal_set_defer_stale(lk_engine *e, int on);
int lk_internal_reference_order(const lk_engine *e);

// Frames that reach a member through a collective on the group's communication stream: the engine's fill (upload copy +
// pyramid, on the engine's stream or - LK_IMG_NXT, ring slots - its next-frame stream) waits for `after` on the device
// instead of the host waiting for the collective, and records `consumed` behind the last kernel that reads the pixels
// (the next collective into that buffer waits for it).  Either event may be null.
int lk_internal_set_image_device_after(lk_engine *e, int slot, const void *device_pixels, int rows, int cols, int step,
                                       hipEvent_t after, hipEvent_t consumed);
int lk_internal_sequence_set_frame_device_after(lk_engine *e, int slot, const void *device_pixels, int rows, int cols, int step,
                                                hipEvent_t after, hipEvent_t consumed);
// 1: a solve of this engine launches teams of workgroups that wait for each other (collectives stay in stream order then)
int lk_internal_team_launches(const lk_engine *e);
int lk_internal_sector_count(const lk_engine *e);

// Automatic initial guess (lk_guess_search.cpp): what the search needs of the engine.  The accessor finishes pending
// rebuilds of the lists, makes the engine's stream wait for a ring slot's pyramid, and sizes the match buffer [S].
struct LkGuessSearchView {
  hipStream_t stream;
  int S, model, level;
  const uint8_t *und, *def; // level-L images (def: LK_IMG_DEF or the ring slot)
  int urows, ucols, drows, dcols;
  const float2 *xy;         // level-L lists in the reference's order, [S+1] offsets, [S] implicit rectangles (device)
  const uint32_t *off;
  const int4 *rect;
  const int4 *h_rect;       // [S] the same rectangles on the host (width 0: explicit list)
  const uint32_t *h_off;    // [S+1]
  float *d_guess, *d_prev_p; // [S][6] engine-held guesses and previous_resulting_parameters
  lk_guess_match *d_match;  // [S]
  const float2 *center;     // [S] the committed level-0 centres (device; lk_search_rotated)
};
// refusals are prefixed with `who`, the function the caller called
int lk_internal_guess_search_view(lk_engine *e, int level, int def_slot, LkGuessSearchView *v, const char *who = "lk_search_guesses");
// level -1: py_stop (v->level says which)
int lk_internal_guess_search_matches(lk_engine *e, lk_guess_match **d_match, hipStream_t *stream);
// the engine's stream, its device made current (lk_get_rotated_search_info / _profile wait on it)
int lk_internal_engine_stream(lk_engine *e, hipStream_t *stream);
int lk_internal_fail(lk_engine *e, int code, const char *what);
int lk_internal_hipfail(lk_engine *e, hipError_t err, const char *where);
// the sector count the match buffer holds results for (set by lk_search_guesses; 0: none yet)
int *lk_internal_guess_search_count(lk_engine *e);

// ---- recovery of failed sectors (lk_reseed.cpp) ------------------------------------------------------------------
// A subset of the committed sectors for one solve, in the layout of the engine's own order tables: the retries of size
// class c (forward modes) at order[class_begin[c] ..], count[c] of them; of backward lane-group range g at
// bw_order[bw_begin[g] ..], bw_count[g] of them.  Only the tables of the engine's current update mode are read.
struct LkSectorSet {
  const uint32_t *order;
  int count[6];
  const uint32_t *bw_order;
  int bw_count[3];
};
// What the recovery pass needs of the engine.  The accessor finishes pending rebuilds of the lists and of the size
// classes (so that the tables below are the ones the next solve uses); need_solve: the engine must hold the records of a
// batch solve of the committed sectors.
struct LkReseedView {
  hipStream_t stream;
  int S, model, backward;
  const float2 *center;     // [S]
  lk_result *result;        // [S] the engine-held records
  float *last_p, *last_eval_p; // [S][6]
  uint32_t *stats;          // [S][4]
  const uint32_t *order;    // [S] sectors by size class, class c at [class_begin[c], class_begin[c + 1])
  int class_begin[7];
  const uint32_t *bw_order; // [S] sectors by backward lane group (backward mode only, else null)
  int bw_begin[4];
};
int lk_internal_reseed_view(lk_engine *e, int need_solve, const char *who, LkReseedView *v);
// the engine's own solve (launch_all: its current mode, its streams, its launch chain) on the sectors of `set`
int lk_internal_solve_set(lk_engine *e, const LkSectorSet *set, const float *d_guess, lk_result *d_result);
// lk_get_stats after the pass: the counters of the retry solves {sectors, evaluations, sample evaluations, point
// iterations, ill-conditioned solves}
int lk_internal_reseed_stats(lk_engine *e, const unsigned long long totals[5]);

// ---- the add-on passes (lk_pass.hpp has the host plumbing they share) -----------------------------------------------------
// What a pass keeps between its calls hangs on its entry of one table of the engine: made by the pass on first use
// (lk_pass_state), deleted by lk_destroy through the virtual destructor.
struct LkPassSlot {
  virtual ~LkPassSlot() = default;
};
enum LkPass { LK_PASS_RESEED, LK_PASS_STRAIN, LK_PASS_UNCERTAINTY, LK_PASS_OUTLIER, LK_PASS_TRACK, LK_PASS_RESIDUAL, LK_PASS_PATTERN,
              LK_PASS_FIELD, LK_PASS_ZNSSD, LK_PASS_QUADRATIC, LK_PASS_SPLINE, LK_PASS_WEIGHTED, LK_PASS_COMPOSED, LK_PASS_ROTATED, LK_PASS_MOTION, LK_PASS_NOISE, LK_PASS_LENS, LK_PASS_STEREO, LK_PASS_EPIPOLAR, LK_PASS_COUNT };
LkPassSlot **lk_internal_pass_slot(lk_engine *e, int which);

// What a post-processing pass reads of the engine (lk_strain_field, lk_parameter_uncertainty, lk_flag_outliers,
// lk_track_points, lk_photometry, lk_residual_map, lk_field_map, lk_rigid_motion, lk_lens_fit, lk_lens_correct, lk_stereo_points, lk_stereo_strain).  Allowed in every mode, reference-order included.  `need` says what the
// call depends on; every refusal is prefixed with `who`, the function the caller called.
enum : unsigned {
  LK_VIEW_RECORDS = 1u, // the engine-held records of a finished batch solve of the committed sectors (`result`)
  LK_VIEW_WINDOW = 2u,  // a window of the committed sectors that has been waited for (`window`, read in place)
  // The level-L images and lists, L = py_start, the finest level the solve reaches; def_slot: -1 (LK_IMG_DEF) or a ring
  // slot, whose pyramid the engine's stream then waits for.  The pass walks the lists, so a pending rebuild of them
  // (lk_update_sector) is finished as the next solve would.  Without this flag it stays pending: the call reads the centres
  // alone, and the ones held until then are the ones the engine-held records were solved at.
  LK_VIEW_IMAGES = 4u,
};
struct LkPassView {
  hipStream_t stream;
  int S, model, interp, level;
  const uint8_t *und, *def; // level-L images (LK_VIEW_IMAGES, else null, as the lists)
  int urows, ucols, drows, dcols;
  const float2 *xy;         // level-L lists in the reference's order, [S+1] offsets, [S] implicit rectangles (device)
  const uint32_t *off;
  const int4 *rect;
  const int4 *h_rect0;      // [S] the level-0 rectangles on the host (width 0: explicit list)
  const uint32_t *h_off0;   // [S+1] the level-0 offsets on the host
  const float2 *center;     // [S]
  lk_result *result;        // [S] the engine-held records; lk_flag_outliers with mark = 1 writes their errorCode words, every
                            // other pass only reads
  const lk_result *window;  // [window_frames][S] the device records of the last window (LK_VIEW_WINDOW, else null)
  int window_frames;
};
int lk_internal_pass_view(lk_engine *e, const char *who, unsigned need, int def_slot, LkPassView *v);
// What a pass reads that looks at ONE image (lk_pattern_quality, lk_suggest_subset): the level-L pyramid of `slot`
// (LK_IMG_UND, LK_IMG_DEF or LK_IMG_NXT, whose fill the engine's stream then waits for), L = py_start, as both `und` and
// `def` of the view with its dimensions - no other slot has to be set.  need_sectors: the committed sectors with the
// level-L lists, a pending rebuild of them finished first as for LK_VIEW_IMAGES; without it the call needs no sectors and
// the view has S = 0 and no lists.  Allowed in every mode; every refusal is prefixed with `who`.
int lk_internal_image_view(lk_engine *e, const char *who, int slot, int need_sectors, LkPassView *v);
// What a pass reads that looks at K frames of one scene (lk_camera_noise, lk_sector_noise): the level-L pyramids, L =
// py_start, of the image slots slots[0 .. n_frames - 1] (ring == 0: 2 or 3 distinct slots of LK_IMG_UND / _DEF / _NXT, under
// lk_internal_image_view's checks and its wait for LK_IMG_NXT) or of the ring slots first .. first + n_frames - 1 (ring != 0:
// 2 .. LK_NOISE_MAX_FRAMES, under level_images' range check and its wait for each slot's pyramid), all of one geometry.
// need_sectors: the committed sectors with the level-L lists, a pending rebuild of them finished first.  Allowed in every
// mode; every refusal is prefixed with `who`.
struct LkFramesView {
  hipStream_t stream;
  int level, n_frames;
  const uint8_t *frame[LK_NOISE_MAX_FRAMES];
  int rows, cols;           // of every frame at level L
  int S;                    // need_sectors, else 0 and no lists
  const float2 *xy;
  const uint32_t *off;
  const int4 *rect;
  const int4 *h_rect0;
  const uint32_t *h_off0;
  const float2 *center;
};
int lk_internal_frames_view(lk_engine *e, const char *who, int ring, int n_frames, const int *slots, int first, int need_sectors,
                            LkFramesView *v);

// Bench hooks (scripts/*_bench.py; exported, not part of include/*.h): of the last call of a pass, the HIP-event time of its
// device part - for the passes with a cell grid the bounding box with its round trip, the grid kernels, the prep and the
// pass's own kernels - and what the call chose.  The two events are recorded by every call; the time is read here.
extern "C" {
// the lane group and variant that ran, the expected members of a sector's 3 x 3 cells
int lk_internal_strain_last(lk_engine *e, float *device_ms, int *group, int *packed, double *members);
// the sectors each lane group (16, 64, 512 lanes) took
int lk_internal_uncertainty_last(lk_engine *e, float *device_ms, int *count3);
// the lane group, the LDS rows a lane may stash, the expected members of a sector's 3 x 3 cells
int lk_internal_outlier_last(lk_engine *e, float *device_ms, int *group, int *lds_rows, double *members);
// the lane group, the expected members of a position's 3 x 3 cells
int lk_internal_track_last(lk_engine *e, float *device_ms, int *group, double *members);
// lk_photometry or lk_residual_map: the pixel tiles of a map (0 after lk_photometry) and how many of them walked global
// memory because their candidates did not fit into LDS
int lk_internal_residual_last(lk_engine *e, float *device_ms, int *tiles, int *fallback_tiles);
// lk_pattern_quality or lk_suggest_subset: the two tile constants of the table build (pixels a workgroup scans per pass of
// the row step, rows per band of the column step), and of that time the table build and the query (both 0 after
// lk_pattern_quality)
int lk_internal_pattern_last(lk_engine *e, float *device_ms, int *row_tile, int *band_rows, float *build_ms, float *query_ms);
// lk_field_map: the node tiles of the map and how many of them walked global memory because their candidates did not fit
// into LDS (all of them under LK_FIELD_WALK=1)
int lk_internal_field_last(lk_engine *e, float *device_ms, int *tiles, int *fallback_tiles);
// lk_refine_znssd: the sectors each lane group (16, 64, 512 lanes) took
int lk_internal_znssd_last(lk_engine *e, float *device_ms, int *count3);
// lk_refine_quadratic: the same
int lk_internal_quadratic_last(lk_engine *e, float *device_ms, int *count3);
// lk_refine_spline: the same, and of that time the build of the coefficient image
int lk_internal_spline_last(lk_engine *e, float *device_ms, int *count3, float *build_ms);
// lk_refine_weighted: as lk_internal_znssd_last
int lk_internal_weighted_last(lk_engine *e, float *device_ms, int *count3);
// lk_refine_composed: as lk_internal_weighted_last; the time covers the coefficient image of a spline sampler
int lk_internal_composed_last(lk_engine *e, float *device_ms, int *count3);
// lk_rigid_motion: the chunk size and the chunks per frame; the time covers the pack, the passes and the removal (not the
// bounding box's round trip, which comes before, and not the copies of the records)
int lk_internal_motion_last(lk_engine *e, float *device_ms, int *chunk, int *chunks);
// lk_camera_noise or lk_sector_noise: the workgroups of the frame kernel (0 after lk_sector_noise); the time covers the
// clearing of the tables and the kernels, not the upload of a mask or the copies of the results
int lk_internal_noise_last(lk_engine *e, float *device_ms, int *workgroups);
// lk_lens_fit or lk_lens_correct: the chunk size and the chunks per frame (both 0 after lk_lens_correct) and the evaluations
// of the fit; the time covers the pack and the kernels of every evaluation with the downloads and host steps between them
// (lk_lens_fit) or the pack and the correction (lk_lens_correct), not the bounding box's round trip or the copies of records
int lk_internal_lens_last(lk_engine *e, float *device_ms, int *chunk, int *chunks, int *evaluations, float *eval_ms);
// lk_stereo_points or lk_stereo_strain: the lane group and the expected members of a sector's 3 x 3 cells (both 0 after
// lk_stereo_points) and the frames of the points held on the device (-1: none); the time covers the kernels - for
// lk_stereo_strain with the bounding box's round trip and the grid - not the copies of records, points or results
int lk_internal_stereo_last(lk_engine *e, float *device_ms, int *group, double *members, int *held_frames);
// lk_search_epipolar: its two kernels by HIP events (waits for them), the host's time for the curve table, the candidates of
// all sectors, the LDS window bound of the launch and the longest run of stations one workgroup takes
int lk_internal_epipolar_last(lk_engine *e, float *search_ms, float *reduce_ms, double *curves_ms, long long *candidates,
                              int *win_bytes, int *max_run);
// Test hook (tests/test_cell_grid_gpu.py), no pass's last call: the cell grid over the committed centres that a neighbour pass
// builds for `radius` (lk_pass_grid, in buffers of its own), its geometry and its tables - cell_of [S], start [nx ny + 1] (the
// caller's array holds start_capacity words; 4 S + 1025 always suffice), members [S]; any pointer may be null.  Changes no
// engine state; allowed in every mode.
int lk_internal_cell_grid(lk_engine *e, float radius, int *nx, int *ny, double *cell, double *x0, double *y0, uint32_t *cell_of,
                          uint32_t *start, size_t start_capacity, uint32_t *members);
}
