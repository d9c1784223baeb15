// lk_launch.hpp - the kernel launchers: what the host code (lk_engine*.cpp, lk_group.cpp, lk_guess_search.cpp) calls
// and the .hip files define.  Every file on either side includes this header, so each declaration meets its definition
// in front of a compiler.  Same shared library; nothing here is part of include/*.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lk_device.hpp"

// ---- lk_kernels.hip: the forward solve and the known-answer entry points
// rep (these three launchers and the two of lk_backward.hip): where to note the instance launched and what the launcher
// decided for it (lk_get_launch_report); nullptr: nowhere
hipError_t lk_launch_solve(const LkSolveArgs &a, int model, int interp, int group, hipStream_t st, lk_launch_record *rep = nullptr);
// flavour: 0 fast (root-free Cholesky; a bad pivot raises the gate of the SAFE pass behind it), 1 SAFE (the QR inside the
// kernel), 2 reference order (a.reference_order = T)
hipError_t lk_launch_solve_seq(const LkSolveArgs &a, int model, int interp, int group, int flavour, hipStream_t st,
                               lk_launch_record *rep = nullptr);
hipError_t lk_launch_eval(const LkEvalArgs &a, int model, int interp, int group, hipStream_t st, lk_launch_record *rep = nullptr);
hipError_t lk_launch_solve_only(int n, const float *d_in, float *d_out, hipStream_t st);
hipError_t lk_launch_step_compare(int n, const float *d_in, float *d_out, hipStream_t st);
hipError_t lk_launch_reduce_compare(int n, int wide, const float *d_in, float *d_out, hipStream_t st);
hipError_t lk_launch_sample(int interp, const uint8_t *def, int rows, int cols, const float2 *pts, int n,
                            float4 *out, hipStream_t st);

// ---- lk_backward.hip: the inverse-compositional solve
// rep: as lk_launch_solve's (roles LK_LAUNCH_BACKWARD and LK_LAUNCH_BACKWARD_EVAL)
hipError_t lk_launch_backward(const LkBackwardArgs &a, int model, int interp, int group, hipStream_t st,
                              lk_launch_record *rep = nullptr);
hipError_t lk_launch_backward_eval(const LkBackwardEvalArgs &a, int model, int interp, int group, hipStream_t st,
                                   lk_launch_record *rep = nullptr);

// ---- lk_guess_search.hip: the integer-pixel ZNCC search
hipError_t lk_launch_guess_search(const LkGuessSearchArgs &a, hipStream_t st);
// LDS left for the staged window: 64 KB per workgroup minus the scores, the template chunk and the reduction arrays
int lk_guess_search_window_budget(int radius, int has_v);

// ---- lk_rotated_search.hip: the same search over angle and shift
// one workgroup per (sector, angle): the per-angle records
hipError_t lk_launch_rotated_search(const LkRotatedSearchArgs &a, hipStream_t st);
// one lane group per sector: the winner across angles, the guess, the history, the match and the profile
hipError_t lk_launch_rotated_reduce(const LkRotatedSearchArgs &a, hipStream_t st);

// ---- lk_epipolar_search.hip: the same search along the epipolar curve of a calibrated rig
// one workgroup per (sector, run of stations that share a template map): the per-run records and the profile
hipError_t lk_launch_epipolar_search(const LkEpipolarSearchArgs &a, hipStream_t st);
// one lane group per sector: the winner across the runs, the guess, the history and the match
hipError_t lk_launch_epipolar_reduce(const LkEpipolarSearchArgs &a, hipStream_t st);
// LDS left for the staged window of a launch whose longest run has max_run stations and max_cand candidates
int lk_epipolar_search_window_budget(int max_run, int max_cand);

// ---- lk_kernels.hip: pyramids and the level table
hipError_t lk_launch_pyramid(const uint8_t *src, int srows, int scols, uint8_t *dst, hipStream_t st);
hipError_t lk_launch_set_views(const LkLevelView *h_views, LkLevelView *d_views, hipStream_t st);
// copy (src -> l0, skipped when src == l0) + levels 1 and 2 in one launch
hipError_t lk_launch_pyramid2(int n_images, const uint8_t *const *src, const int *step, int rows, int cols,
                              uint8_t *const *l0, uint8_t *const *l1, uint8_t *const *l2, hipStream_t st);

// ---- lk_kernels.hip: sample lists on the device
hipError_t lk_launch_warp_points(const float2 *xy, int n, float cx, float cy, int model, const float *d_p,
                                 float2 *out, hipStream_t st);
hipError_t lk_launch_rewarp(const LkRewarpArgs &a, int model, hipStream_t st);
int lk_decimate_tiles(uint32_t n_max);
// One level of pyramid_class.cpp:289-323 for all sectors: xy_prev[*n_prev] (at most n_max) ->
// xy_out, off_prev[S+1] -> off_out[S+1], *n_out = samples kept.  pos: n_max words,
// tiles: lk_decimate_tiles(n_max) + 1 words.
hipError_t lk_launch_decimate(const float2 *xy_prev, const uint32_t *off_prev, const uint32_t *n_prev, uint32_t n_max,
                              int level_delta, int n_sectors, uint32_t *pos, uint32_t *tiles, float2 *xy_out,
                              uint32_t *off_out, uint32_t *n_out, hipStream_t st);
// pass 1: per-tile counts -> exclusive prefix in place (tiles[n_tiles] = total, also *n_out)
hipError_t lk_launch_roi_count(const LkRoiSector *sectors, const LkRoiFlat *flats, const uint32_t *tile_begin, int n_sectors,
                               uint32_t n_tiles, uint32_t *tiles, uint32_t *n_out, hipStream_t st, int rows = 0);
// pass 2: the samples and the per-sector offsets
hipError_t lk_launch_roi_fill(const LkRoiSector *sectors, const LkRoiFlat *flats, const uint32_t *tile_begin, int n_sectors,
                              uint32_t n_tiles, const uint32_t *tiles, float2 *xy, uint32_t *off, hipStream_t st, int rows = 0);
hipError_t lk_launch_mean_center(const float2 *xy, const uint32_t *off, int n_sectors, float2 *center, hipStream_t st);
// integer, non-negative sample lists (device-masked annular / blob sectors): the same mean, evaluated in parallel
// scratch: lk_mean_center_int_scratch_bytes(total, n_sectors) bytes (chunk table, exact chunk sums, chunk maps)
size_t lk_mean_center_int_scratch_bytes(uint32_t n_samples, int n_sectors);
hipError_t lk_launch_mean_center_int(const float2 *xy, const uint32_t *off, uint32_t n_samples, int n_sectors, void *scratch,
                                     float2 *center, hipStream_t st);

// ---- lk_kernels.hip: per-sector state
hipError_t lk_launch_guess(const float2 *center, const float *last_p, float *prev_p, float *guess,
                           const float *global_guess, float gcx, float gcy, int n_sectors, int model,
                           int frame, int constant_velocity, hipStream_t st);
hipError_t lk_launch_append_sector(const LkAppendArgs &a, hipStream_t st);
// reference-order mode: the stale iteration counts of n records resolved in sector order (lk_stale_iterations_kernel)
hipError_t lk_launch_stale_iterations(lk_result *r, int n, const int *carry_in, int *carry_out, hipStream_t st);
// the same resolution over n_ranks padded blocks of `cap` records holding the shards [r*S/G, (r+1)*S/G)
hipError_t lk_launch_stale_iterations_blocks(lk_result *all, int n_sectors, int n_ranks, int cap, const int *carry_in,
                                             int *carry_out, hipStream_t st);
// reference-order mode, a window of `frames` frames gathered as n_ranks blocks of [frames][cap] records: the stale
// iteration counts resolved in the order the reference solves - frame by frame, sector by sector
hipError_t lk_launch_stale_iterations_window(lk_result *all, int n_sectors, int n_ranks, int cap, int frames, const int *carry_in,
                                             int *carry_out, hipStream_t st);

// ---- lk_reseed.hip: the recovery pass around the solve (lk_reseed_failed / lk_reseed_plan)
// {min x, min y, max x, max y} of the centres
hipError_t lk_launch_reseed_bbox(const float2 *center, int n_sectors, float *out4, hipStream_t st);
// good / failed flags, tried = 0, info initialised, *n_failed += failed sectors (zero it first)
hipError_t lk_launch_reseed_classify(const lk_result *rec, int n_sectors, int n_params, float chi_max, uint8_t *good,
                                     int32_t *tried, lk_reseed_info *info, uint32_t *n_failed, hipStream_t st);
// the cell grid: count -> exclusive scan -> scatter -> members ordered by sector index within a cell.
// cell_of, unordered, members: [S]; start, cursor: [nx * ny + 1]
hipError_t lk_launch_reseed_grid(const float2 *center, int n_sectors, double x0, double y0, double cell, int nx, int ny,
                                 uint32_t *cell_of, uint32_t *start, uint32_t *cursor, uint32_t *unordered, uint32_t *members,
                                 hipStream_t st);
hipError_t lk_launch_reseed_plan(const LkReseedPlanArgs &a, hipStream_t st);
hipError_t lk_launch_reseed_compact(const LkReseedCompactArgs &a, hipStream_t st);
hipError_t lk_launch_reseed_merge(const LkReseedMergeArgs &a, hipStream_t st);

// ---- lk_strain.hip: the strain field (lk_strain_field), and the pack of every pass that fits its plane
// for the n_frames * n_sectors records of a call: good[f * S + s] (where good is not null) by the shared good rule and
// pack[f * S + s] = {cx, cy, u, v} (cx = NaN for a sector that is not good; v = 0 without one); canonical_zero != 0: u + 0
// and v + 0, so that a -0 is packed as +0
hipError_t lk_launch_pack_prep(const lk_result *rec, const float2 *center, int n_sectors, int n_frames, int model, float chi_max,
                               int canonical_zero, uint8_t *good, float4 *pack, hipStream_t st);
// group: 16 or 64 lanes per sector; packed != 0: the neighbours' data come from a.pack, else from a.center / a.good / a.rec
hipError_t lk_launch_strain(const LkStrainArgs &a, int group, int packed, hipStream_t st);

// ---- lk_uncertainty.hip: per-sector uncertainty (lk_parameter_uncertainty)
// group: 16, 64 or 512 lanes per sector (lk_bw_group of the level-0 sample count); a.order lists that group's sectors
hipError_t lk_launch_uncertainty(const LkUncertaintyArgs &a, int model, int interp, int group, hipStream_t st);

// ---- lk_outlier.hip: the outlier flags (lk_flag_outliers)
// between two passes: pack[s].x = NaN for a sector that is not good or that `flags` (the pass before) has flagged, else cx
hipError_t lk_launch_outlier_exclude(const lk_outlier *flags, const float2 *center, const uint8_t *good, int n_sectors,
                                     float4 *pack, hipStream_t st);
// one pass; group: 16 or 64 lanes per sector
hipError_t lk_launch_outlier(const LkOutlierArgs &a, int group, hipStream_t st);
// errorCode = LK_ERROR_OUTLIER in the records of the flagged sectors
hipError_t lk_launch_outlier_mark(const lk_outlier *flags, int n_sectors, lk_result *rec, hipStream_t st);

// ---- lk_track.hip: material-point tracks (lk_track_points)
// every point through every frame in one launch; group: 16 or 64 lanes per point
hipError_t lk_launch_track(const LkTrackArgs &a, int group, hipStream_t st);

// ---- lk_residual.hip: photometry and the residual map (lk_photometry, lk_residual_map)
// group: 16, 64 or 512 lanes per sector (lk_bw_group of the level-0 sample count); a.order lists that group's sectors
hipError_t lk_launch_photometry(const LkPhotometryArgs &a, int model, int interp, int group, hipStream_t st);
// pack[s] of every sector by the shared good rule: centres of both levels, parameters at `level`
hipError_t lk_launch_map_prep(const lk_result *rec, const float2 *center, int n_sectors, int model, int level, float chi_max,
                              LkMapSector *pack, hipStream_t st);
// one workgroup per tile of kLkMapTileW x kLkMapTileH pixels of the window; *n_tiles = the tiles launched
hipError_t lk_launch_residual_map(const LkResidualMapArgs &a, int model, int interp, int *n_tiles, hipStream_t st);

// ---- lk_znssd.hip: the ZNSSD refinement (lk_refine_znssd)
// group: 16, 64 or 512 lanes per sector (lk_bw_group of the level-0 sample count); a.ev.order lists that group's sectors.
// One launch carries every sector of the group from its seed to its final record.
hipError_t lk_launch_znssd(const LkZnssdArgs &a, int model, int interp, int group, hipStream_t st);

// ---- lk_spline.hip: the B-spline refinement (lk_refine_spline, lk_spline_coefficients, lk_spline_sample)
// order: 3 or 5.  The coefficient image [rows][cols] of a level image (pitch == cols; rows, cols >= 2): the row step, then
// the column step in place; the kernel boundary on the stream is the only ordering between them
hipError_t lk_launch_spline_build(int order, const uint8_t *img, int rows, int cols, float *coef, hipStream_t st);
// a thread per point: out[k] = {W, Wx, Wy, 1}, or zeros where the sampler's window leaves the image
hipError_t lk_launch_spline_sample(int order, const float *coef, int rows, int cols, const float2 *pts, int n, float4 *out,
                                   hipStream_t st);
// as lk_launch_znssd, sampling a.coef
hipError_t lk_launch_spline(const LkSplineArgs &a, int model, int order, int group, hipStream_t st);

// ---- lk_weighted.hip: the weighted refinement (lk_refine_weighted)
// as lk_launch_znssd, every sample under a.mask and the window of a.inv; the info goes to a.out
hipError_t lk_launch_weighted(const LkWeightedArgs &a, int model, int interp, int group, hipStream_t st);

// ---- lk_quadratic.hip: the second-order refinement (lk_refine_quadratic)
// as lk_launch_znssd; the engine's model travels in a.model (the kernel has no model template)
hipError_t lk_launch_quadratic(const LkQuadraticArgs &a, int interp, int group, hipStream_t st);

// ---- lk_composed.hip: the composed refinement (lk_refine_composed)
// order 1 under a spline sampler (spline: 3 or 5); under the engine's interpolator the call launches lk_launch_weighted
hipError_t lk_launch_composed_first(const LkComposedFirstArgs &a, int model, int spline, int group, hipStream_t st);
// order 2; spline: 3 or 5, or 0: the interpolator `interp`
hipError_t lk_launch_composed_second(const LkComposedSecondArgs &a, int interp, int spline, int group, hipStream_t st);
// a thread per sector: the info of a first-order call and its records -> struct lk_composed (n_par: the engine model's P)
hipError_t lk_launch_composed_info(const struct lk_weighted *in, const lk_result *rec, int n_par, int n, struct lk_composed *out,
                                   hipStream_t st);

// ---- lk_pattern.hip: speckle quality (lk_pattern_quality, lk_suggest_subset)
// group: 16, 64 or 512 lanes per sector (lk_bw_group of the level-0 sample count); a.ev.order lists that group's sectors
hipError_t lk_launch_pattern(const LkPatternArgs &a, int group, hipStream_t st);
// the two tables of one image: a row step, then the column step's three kernels (band totals, their prefix over the bands,
// the seeded band scans); the kernel boundaries on the stream are the only ordering between workgroups
hipError_t lk_launch_sat_build(const LkSatArgs &a, hipStream_t st);
// a thread per point: every candidate's box sums from the four corners, the smallest passing candidate, the record
hipError_t lk_launch_subset_query(const LkSubsetArgs &a, hipStream_t st);

// ---- lk_noise.hip: camera noise from static frames (lk_camera_noise, lk_sector_noise)
// one launch over the region: the 256-bin table {count, sum q} and the per-frame sums, added to a.bins and a.frame_sums
// (zeroed by the caller); *n_blocks = the workgroups launched; hipErrorInvalidValue for a pointer that is not 16-byte aligned
hipError_t lk_launch_noise_frames(const LkNoiseFrameArgs &a, int *n_blocks, hipStream_t st);
// group: 16, 64 or 512 lanes per sector; a.ev.order lists that group's sectors
hipError_t lk_launch_noise_sectors(const LkNoiseSectorArgs &a, int group, hipStream_t st);

// ---- lk_field.hip: dense displacement and strain maps (lk_field_map)
// one workgroup per tile of kLkMapTileW x kLkMapTileH nodes; weight, frame: LK_FIELD_*; *n_tiles = the tiles launched
hipError_t lk_launch_field_map(const LkFieldArgs &a, int weight, int frame, int *n_tiles, hipStream_t st);

// ---- lk_motion.hip: the global motion per frame (lk_rigid_motion)
// pass a.pass of every frame: the sums of the fit set (one workgroup per chunk and frame), the fit, the residual sums, the
// residual's close - four kernels; a.chunks = the chunks of a.chunk sectors that cover a.n_sectors
hipError_t lk_launch_motion_pass(const LkMotionArgs &a, hipStream_t st);
// a thread per (frame, sector): a.rec without the motion a.out[f] -> a.rec_out
hipError_t lk_launch_motion_remove(const LkMotionArgs &a, hipStream_t st);

// ---- lk_lens.hip: lens distortion (lk_lens_fit, lk_lens_correct)
// one evaluation of the fit: the sums of every frame's rows (one workgroup per chunk and frame), then the chunks joined by
// ascending index into a.sums - two kernels; a.chunks = the chunks of a.chunk sectors that cover a.n_sectors
hipError_t lk_launch_lens_sums(const LkLensFitArgs &a, hipStream_t st);
// a thread per (frame, sector): a.rec without the lens -> a.rec_out, a.status; frame 0's threads write a.centres_out
hipError_t lk_launch_lens_correct(const LkLensCorrectArgs &a, hipStream_t st);

// ---- lk_stereo.hip: a two-camera rig (lk_stereo_points, lk_stereo_strain)
// a thread per (frame, sector) of a.n_frames + 1 frames, the reference state first: the triangulated points -> a.out
hipError_t lk_launch_stereo_points(const LkStereoPointsArgs &a, hipStream_t st);
// group: 16 or 64 lanes per (frame, sector)
hipError_t lk_launch_stereo_strain(const LkStereoStrainArgs &a, int group, hipStream_t st);
