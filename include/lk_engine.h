/* lk_engine.h - C-ABI of the MI355X (gfx950) Lucas-Kanade correlation engine.
 *
 * Drop-in boundary for the hot path of namascar/correlation: everything the reference's
 * managerClass asks of its GPU engine `CudaClass` (cuda_class.cuh:46-79) and of its CPU
 * engine `CorrelationClass` (correlation_class.hpp:132-179) for ONE image pair:
 * image pyramids, ROI -> sample lists, and the per-sector coarse-to-fine
 * Levenberg-Marquardt solve.  Plain C types only; no OpenCV / Qt / torch types.
 *
 * Conventions
 *  - every function returns an `lk_error` (the reference's errorEnum values,
 *    enums.hpp:25-35); the engine never calls exit() (the reference does on CUDA errors,
 *    cuda_class.cu:52-56).  lk_last_error_string() describes the last failure.
 *  - the caller owns every buffer it passes in or receives results in; the engine copies
 *    during the call and never returns pointers into its own memory (the reference
 *    returns a pointer to engine-owned pinned memory, cuda_polygon.cuh:339-340).
 *  - results follow the CPU engine's semantics (SURVEY.md section 8a-a13 lists where the
 *    reference's CUDA path differs): look-ahead parameters are returned, `iterations` is
 *    the last pyramid level's trip count, chi is the 1/n-scaled last_good_chi.
 *  - one caller thread at a time, except lk_set_image(LK_IMG_NXT) which may overlap a
 *    running lk_correlate_* (manager_class.cpp:1438-1447 prefetches the next frame).
 */
#ifndef LK_ENGINE_H
#define LK_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LK_MAX_LEVELS 8
#define LK_MAX_PARAMS 6

/* errorEnum, enums.hpp:25-35 (same numeric values) */
typedef enum {
  LK_ERROR_NONE = 0,
  LK_ERROR_MODEL_OUT_OF_IMAGE = 1,
  LK_ERROR_INTERPOLATION_OUT_OF_IMAGE = 2,
  LK_ERROR_CORRELATION_MAX_ITERS_REACHED = 3,
  LK_ERROR_BAD_DOMAIN = 4,
  LK_ERROR_SOLVER = 5, /* error_cuSolver */
  LK_ERROR_DEVICE = 6, /* error_cuda: any HIP failure */
  LK_ERROR_MULTITHREAD = 7,
  /* Extension (not a value of the reference's errorEnum): the record converged, but lk_flag_outliers with mark = 1 found
   * its displacement inconsistent with its neighbourhood.  No solve produces it.  It is not LK_ERROR_NONE, so the "good"
   * rule of the recovery pass, the strain field and the uncertainty pass rejects such a record. */
  LK_ERROR_OUTLIER = 8
} lk_error;

/* interpolationModelEnum, enums.hpp:10-15 */
typedef enum {
  LK_IM_NEAREST = 0,
  LK_IM_BILINEAR = 1,
  LK_IM_BICUBIC = 2,
  /* Extension (not a value of the reference's interpolationModelEnum): the same bicubic
   * surface - the reference's 16-coefficient patch is the Catmull-Rom spline in exact
   * arithmetic - evaluated in separable form, 4 + 4 weights and their derivatives.  It is
   * closer to the exact spline than the reference's monomial evaluation (whose cancellation
   * costs ~1e-3 grey levels), so it agrees with LK_IM_BICUBIC to that rounding, not bit for bit,
   * and whole solves agree to ~1e-5 relative chi rather than inside the reference's own noise.
   * About 40 % fewer instructions per sample.  Never selected implicitly. */
  LK_IM_BICUBIC_SEPARABLE = 3
} lk_interpolation;
/* fittingModelEnum, enums.hpp:17-23: p = (u), (u,v), (u,v,q), (u,v,ux,uy,vx,vy) */
typedef enum { LK_FM_U = 0, LK_FM_UV = 1, LK_FM_UVQ = 2, LK_FM_UVUXUYVXVY = 3 } lk_fitting_model;
/* ImageType, enums.hpp:94-99 */
typedef enum { LK_IMG_UND = 0, LK_IMG_DEF = 1, LK_IMG_NXT = 2 } lk_image_slot;

/* CorrelationClass ctor arguments (correlation_class.hpp:132-137) +
 * CudaClass::set_* (cuda_class.cu:77-102) + resetImagePyramids' start/step/stop (:475) */
typedef struct {
  int interpolation;   /* lk_interpolation, default im_bicubic (mainapp.cpp:64) */
  int fitting_model;   /* lk_fitting_model */
  float precision;     /* required_precision, default 1e-3 */
  int max_iters;       /* maximum_iterations, default 50 */
  int py_start, py_step, py_stop; /* pyramid levels, default 0/1/2 */
  int device;          /* HIP device ordinal this engine lives on */
} lk_config;

/* layout-identical to CorrelationResult (domains.hpp:110-118), 48 bytes */
typedef struct {
  float resultingParameters[6];
  float chi;
  int numberOfPoints;
  int iterations;
  int errorCode; /* lk_error */
  float undCenterX;
  float undCenterY;
} lk_result;

/* counters of the last lk_correlate_* call, for the bench */
typedef struct {
  uint64_t sectors;
  uint64_t evaluations;       /* warp+sample+accumulate passes over one sector */
  uint64_t sample_evaluations;/* sum over evaluations of the sector's n_L */
  uint64_t point_iterations;  /* per sector and level: LM trips + 1 (evaluation #0) */
  uint64_t algorithmic_bytes; /* 25*sample_evaluations + 196*evaluations */
  uint64_t ill_conditioned_solves; /* damped solves (outside starved levels) that met a bad pivot */
  float solve_ms;             /* HIP-event time of the solve kernel(s) of the last call */
  float pyramid_ms;           /* HIP-event time of the last pyramid build */
  uint64_t window_safe_reruns;/* since lk_create: frame-pipelined windows whose fast flavour met a bad pivot and were
                               * solved again with the SAFE flavour */
} lk_stats;

typedef struct lk_engine lk_engine;

/* ---- life cycle ------------------------------------------------------------------- */
/* CudaClass::initialize (cuda_class.cu:39-75): number of usable devices */
int lk_device_count(void);
/* CorrelationClass ctor / CudaClass ctor + set_* */
int lk_create(const lk_config *cfg, lk_engine **out);
void lk_destroy(lk_engine *e);
const char *lk_last_error_string(const lk_engine *e);
/* run all engine work on a caller-provided hipStream_t (NULL = engine's own stream) */
int lk_set_stream(lk_engine *e, void *hip_stream);
/* HIP events around pyramid builds and solves (the DEBUG_TIME_* prints of defines.hpp:29-72):
 * on by default; off removes four event records per frame from the stream and leaves
 * lk_stats.solve_ms / pyramid_ms at their last values */
int lk_set_timing(lk_engine *e, int enabled);
/* A sector's record is always deterministic for a given batch.  By default it may differ in
 * the last bits between batches of different composition (a half-wavefront that runs out of
 * work joins its neighbour's sector, which changes the summation grouping - the same kind of
 * difference the reference shows between thread counts, correlation_class.cpp:169-186,253-275).
 * enabled = 1 switches that off (and fixes the lane group by the sector's own size instead of
 * the batch's): a sector then gets the same bits in any batch, shard or single-sector call
 * (about 20 % slower on small grids).  Call it before lk_commit_sectors. */
int lk_set_batch_invariant(lk_engine *e, int enabled);
/* Reference-order mode.  threads = T > 0: every evaluation of every sector at every pyramid level
 * adds its A, b and chi in the CPU engine's own order for number_of_threads = T - rounded
 * product, then rounded add, sample by sample (x outer / y inner for rectangles,
 * interpolation_class.cpp:722-749), in T contiguous chunks joined in thread order
 * (correlation_class.cpp:169-186, :253-275) - and every damped system goes through the restated
 * ColPivHouseholderQR (correlation_class.cpp:742-747).  The 48-byte records are then bit-identical
 * to CorrelationClass::Newton_Raphson's (as restated by the repository's CPU checker) for that
 * thread count (T = 1: one running sum; the reference's compile-time default is 20, defines.hpp).  The records
 * are also independent of batch composition.  The sample work stays parallel (a 16-lane row or a
 * wavefront per sector forms the per-sample products and transposes them through LDS; only the
 * additions of each sum run as a chain; the lanes of a wavefront are dealt to its four sectors by need), so the
 * mode costs 1.1-1.9x the default's time (measured, round 3: config 2 0.46 against 0.24 ms, config 4 2.1 against
 * 1.9 ms, config 5 8.6 against 5.4 ms), not the serial loop's.  threads = 0 (default): lane-parallel sums and the root-free Cholesky solve,
 * which differ from the reference by summation order and solver rounding only.
 * May be called at any time; the lane groups are re-chosen before the next solve. */
int lk_set_reference_order(lk_engine *e, int threads);
/* Update scheme of the LM solve (updateEnum, enums.hpp:39: the reference's GUI option "Update: Forward / Backward",
 * which its engine stores and never reads).  May be called at any time; the next solve uses the new mode.
 * LK_UPDATE_FORWARD (default): the forward-additive scheme of correlation_class.cpp:349-640 - every evaluation samples the
 *   deformed image with its gradient and rebuilds A; p += dp.
 * LK_UPDATE_BACKWARD: the inverse-compositional scheme (IC-GN).  For sector s at level L, with the forward solve's
 *   level-L samples x_i and centre c:
 *   template  T_i = und_L at the node (int)(x_i + 0.5f) (clamped), grad T_i = the interpolation model's gradient at that
 *             integer node (what lk_sample(LK_IMG_UND, L, node) returns), G_i = grad T_i . dW/dp at x_i - c,
 *             H = sum G_i G_i^T - once per sector and level.  A node the sampler flags as out of the image gives the
 *             record LK_ERROR_INTERPOLATION_OUT_OF_IMAGE, as a failed evaluation #0 does.
 *   evaluation V_i = T_i - def_L(W(x_i; p)) (the value-only form of the engine's sampler), b = sum G_i V_i,
 *             chi = sum V_i^2 - the same chi and 1/n scaling as the forward mode.
 *   step      delta = the damped solve of (H/n, b/n), H_ii *= 1 + lambda (compute_model_parameters,
 *             correlation_class.cpp:642-700), by the engine's device solver (root-free Cholesky, pivoted-QR fallback, QR on
 *             starved levels); the new parameters are W(p) o W(-delta)^-1 (lk_compose_inverse).  A singular step
 *             (|det A_q| < 1e-6) counts as a diverging one: no evaluation, lambda x 10, the next trip starts from the
 *             last good parameters.
 *   control   the reference's LM loop otherwise: lambda x 0.4 down to 1e-9 / x 10 up to 1e9, the saved / tentative /
 *             last-good parameter sets with the look-ahead step, the delta_chi rule, max_iters, error codes, iteration
 *             counting, level-to-level translation; the record, lk_get_last_evaluated_parameters and the per-sector
 *             counters as in the forward mode.  A rejected trip evaluates nothing: the kept b of the last good
 *             parameters and the larger lambda give the next step.  A sector whose first evaluation fails reports the
 *             iteration count of its own earlier levels (0 at the first), as the forward default mode does.
 *   counters  lk_stats.evaluations / sample_evaluations count deformed-image passes (template passes are not counted);
 *             algorithmic_bytes = 40 B per sample evaluation (16 B deformed window, 16 B template slot, 8 B list entry)
 *             + 196 B per evaluation.
 *   records   a sector's record depends on that sector, its images and its guess only: bit-identical in any batch, shard,
 *             single-sector lk_correlate, lk_set_pairs_in_flight setting and sequence window (lk_set_batch_invariant has
 *             no effect).  Sequence windows run their frames one after the other (lk_sequence_is_pipelined() == 0).
 * Backward mode and reference-order mode exclude each other: whichever is set second returns LK_ERROR_BAD_DOMAIN. */
#define LK_UPDATE_FORWARD 0
#define LK_UPDATE_BACKWARD 1
int lk_set_update(lk_engine *e, int mode);
/* Independent image pairs can be solved side by side: one engine per pair in flight, each on
 * its own stream (lk_set_stream).  A solve ends in a tail of slow sectors that leaves most of
 * the GPU idle; the next pair's solve fills it (C2: 0.26 ms per pair one at a time, 0.15 ms
 * with three in flight).  n tells the engine how many launches share the GPU so that it keeps
 * the narrow, better-packed lane groups it would otherwise widen to shorten a lone solve
 * (default 1), and it bounds the width of the multi-workgroup teams that solve giant sectors:
 * team workgroups wait for each other, so engines whose team launches can be on the GPU at the
 * same time MUST declare it.  Call it before lk_commit_sectors.  Tracked sequences cannot use this: the
 * guess of pair k+1 needs the result of pair k (manager_class.cpp:2602-2707). */
int lk_set_pairs_in_flight(lk_engine *e, int n);
/* block until everything queued by this engine has finished */
int lk_synchronize(lk_engine *e);

/* ---- images and pyramids ---------------------------------------------------------- */
/* CorrelationClass::set_undeformed/deformed/next_image (correlation_class.cpp:38-51),
 * CudaClass::resetImagePyramids / resetNextPyramid (cuda_class.cu:475-559): upload the
 * level-0 pixels (monochrome u8, `step` bytes per row) and build levels 1..py_stop.
 * File decoding stays with the caller. */
int lk_set_image(lk_engine *e, int slot, const uint8_t *host_pixels, int rows, int cols, int step);
/* Frames in PINNED host memory ("pinned staging + hipMemcpyAsync on a dedicated stream"; the reference uploads
 * from pageable cv::Mat pixels, cuda_pyramid.cu:83-103).  lk_pin_host_memory page-locks a caller's frame buffer
 * (hipHostRegister; hipHostMalloc'ed memory needs nothing).  lk_set_image / lk_sequence_set_frame from pinned memory
 * return as soon as the copy is ENQUEUED - with LK_IMG_NXT or a ring slot on the next-frame stream, i.e. beside a running
 * solve, without a helper thread - instead of waiting for it as they do for pageable memory.  The buffer must stay
 * unchanged until the frame has been used: until the next lk_correlate_* that reads it has returned, or lk_synchronize. */
int lk_pin_host_memory(void *ptr, size_t bytes);
int lk_unpin_host_memory(void *ptr);
/* same, pixels already in this device's memory (used after an RCCL broadcast) */
int lk_set_image_device(lk_engine *e, int slot, const void *device_pixels, int rows, int cols, int step);
/* CudaClass::resetImagePyramids(und, def, ...) (cuda_class.cu:475-519): both frames of a pair,
 * already in this device's memory, uploaded and reduced in one launch */
int lk_set_image_pair_device(lk_engine *e, const void *und_pixels, int und_step, const void *def_pixels,
                             int def_step, int rows, int cols);
/* CorrelationClass::set_und_image_from_def / set_def_image_from_nxt
 * (correlation_class.cpp:53-61), CudaClass::makeUndPyramidFromDef / makeDefPyramidFromNxt
 * (cuda_class.cu:561-567): pointer rotation, no copies */
int lk_rotate_und_from_def(lk_engine *e);
int lk_rotate_def_from_nxt(lk_engine *e);
/* download one pyramid level (cudaImage::testPyramid, cuda_pyramid.cu:304-346);
 * host_out may be NULL to query the size */
int lk_get_pyramid_level(lk_engine *e, int slot, int level, uint8_t *host_out, int *rows, int *cols);

/* ---- sectors (ROI -> sample lists) ------------------------------------------------ */
/* forget all sectors */
int lk_clear_sectors(lk_engine *e);
/* CudaClass::resetPolygon(iSector,x0,y0,x1,y1) (cuda_class.cu:574-582) with the CPU
 * path's sample order (x outer, y inner, inclusive; manager_class.cpp:1596-1614) and
 * centre ((x0+x1)/2,(y0+y1)/2) = the integer centre the manager passes (:438-441) */
int lk_set_sector_rect(lk_engine *e, int sector, int x0, int y0, int x1, int y1);
/* the whole rectangular prologue (manager_class.cpp:276-310): hs*vs sectors,
 * iSector = i*vs + j; registers sectors [first, first+count) of that grid as engine
 * sectors 0..count-1 (count<0: all) - the multi-GPU shard entry point */
int lk_set_rect_grid(lk_engine *e, float x_begin, float y_begin, float x_end, float y_end,
                     int hs, int vs, int first, int count);
/* CudaClass::resetPolygon(iSector,r,dr,a,da,cx,cy,as) (cuda_class.cu:584-594) with the
 * CPU path's predicate and order (manager_class.cpp:816-940); centre = float mean */
int lk_set_sector_annular(lk_engine *e, int sector, float r, float dr, float a, float da,
                          float cx, float cy, int as);
/* the sectors first_sector .. first_sector+count-1 of an annular domain in one call - the sector
 * loop of perform_single_frame_correlation_annular (manager_class.cpp:600-720) - rasterised by a
 * few host threads, one sector each at a time (every list is the sequential scan's).
 * params [count][6] = {r, dr, a, da, cx, cy} per sector. */
int lk_set_sectors_annular(lk_engine *e, int first_sector, int count, const float *params, int as);
/* CudaClass::resetPolygon(v_points) (cuda_class.cu:596-605) with polygonBlob_class
 * semantics (polygon_class.cpp:224-429); LK_ERROR_BAD_DOMAIN on a self-intersecting
 * contour (manager_class.cpp:1028-1031) */
int lk_set_sector_blob(lk_engine *e, int sector, const float *contour_xy, int n_vertices);
/* CorrelationClass::Newton_Raphson(p, n, xy) / (p, n, cx, cy, xy)
 * (correlation_class.cpp:306-343): explicit AoS sample list; use_center=0 -> float mean */
int lk_set_sector_points(lk_engine *e, int sector, const float *xy, int n, int use_center,
                         float cx, float cy);
/* build per-level sample lists (pyramid_class.cpp:289-362) and upload; must be called
 * after the lk_set_sector_* calls and before lk_correlate_*.  Annular and blob sectors are
 * registered by their description and rasterised HERE (on the device): a sector that turns
 * out to be empty is reported by this call (LK_ERROR_BAD_DOMAIN, the message names the
 * sector), not by lk_set_sector_annular / _blob - unless LK_HOST_ROI=1, where the host scan
 * runs at registration like the reference's (manager_class.cpp:1028-1031).  Sectors registered since the
 * previous commit start with zeroed sequence state (guess history, last record); every other
 * sector keeps its state, so the reference's first-frame loop - resetPolygon(i), correlate(i),
 * sector after sector (manager_class.cpp:340, :449) - can commit once per sector and still
 * move every sector from its own record on the next frame (lk_update_sector). */
int lk_commit_sectors(lk_engine *e);
/* Domain tracking between the frames of a sequence, CPU-engine semantics (the CUDA engine's
 * cudaPolygon::updatePolygon, cuda_polygon.cu:268-415, moves by its own lastGood
 * parameters instead).  Both keep the per-sector sequence state (guess history).
 *  - Lagrangian (manager_class.cpp:381-419): sample (x,y) -> ((int)(ox+x+0.5f), (int)(oy+y+0.5f))
 *    with the sector's offset (ox,oy) = new und centre - past und centre (add_pair, :38-47);
 *  - strict Lagrangian (manager_class.cpp:369-380): the deformed sample positions of the last
 *    solve (CorrelationClass::getDefXY0, correlation_class.cpp:884-896: warped with the
 *    parameters of the last level-0 evaluation) become the undeformed samples.
 * offsets_xy [S][2]; centers_xy [S][2] = centres for the next solve (the rectangular path
 * passes integers, manager_class.cpp:438-441) or NULL = float mean of the new samples.
 * Both rebuild the lists of every pyramid level on the device (the samples never visit the
 * host), except that lk_translate_sectors keeps grids of implicit rectangles on the host
 * records: a rectangle that moves by whole pixels stays implicit. */
int lk_translate_sectors(lk_engine *e, const float *offsets_xy, const float *centers_xy);
int lk_rewarp_sectors(lk_engine *e, const float *centers_xy);
/* one sector, from the engine's own last record of it - the call shape of
 * CudaClass::updatePolygon(iSector, deformationDescription) (cuda_class.cu:569) with the CPU
 * manager's meaning; mode = deformationDescriptionEnum (0 strict Lagrangian, 1 Lagrangian,
 * 2 Eulerian = nothing).  The lists are rebuilt before the next solve. */
int lk_update_sector(lk_engine *e, int sector, int mode);
/* undo the last lk_translate_sectors / lk_rewarp_sectors for sectors >= first_sector: the
 * sectors a frame never reached because it stopped at an error (manager_class.cpp:520-546) */
int lk_restore_sectors(lk_engine *e, int first_sector);
/* [S][6]: the parameters the last evaluation of each sector ran at (level-0 scale) */
int lk_get_last_evaluated_parameters(lk_engine *e, float *out);
int lk_sector_count(const lk_engine *e);
/* CorrelationClass::get_number_of_points / get_und_x/y_center (correlation_class.cpp:850-868) */
int lk_get_sector_info(lk_engine *e, int sector, int *n_points, float *cx, float *cy);
/* number of samples of a sector at a pyramid level (pyramid_class.cpp:437-439) */
int lk_get_sector_level_count(lk_engine *e, int sector, int level, int *n);
/* CudaClass::getUndXY0ToCPU / CorrelationClass::getUndXY0 (cuda_class.cu:607-609):
 * returns the count; copies min(count, cap) AoS pairs */
int lk_get_und_xy(lk_engine *e, int sector, float *xy, int cap, int *count);
/* Diagnostics: the explicit sample list of a sector at a pyramid level as the device holds it (pyramid_class.cpp:289-323:
 * the decimated lists).  which = 0: the reference's order - what the centres, the starved levels and the reference-order
 * mode walk.  which = 1: the row-major evaluation copy the lane groups of the default mode walk (annular sectors rasterised
 * by the device masks, lists from the host in the reference's x outer / y inner order, moved lists; the same samples row by
 * row, so that neighbouring lanes read neighbouring pixels) -
 * LK_ERROR_BAD_DOMAIN when the domain has none.  Implicit rectangles have no list (count 0). */
int lk_get_level_xy(lk_engine *e, int level, int which, int sector, float *xy, int cap, int *count);
/* CudaClass::getDefXY0ToCPU / CorrelationClass::getDefXY0 (cuda_class.cu:611-613,
 * kModel_inPlace correlationKernel.cu:56-110): level-0 samples warped by p */
int lk_get_def_xy(lk_engine *e, int sector, const float *p, float *xy, int cap, int *count);

/* ---- the solve -------------------------------------------------------------------- */
/* CudaClass::correlate(iSector, guess, results) (cuda_class.cu:104-293) /
 * CorrelationClass::Newton_Raphson: one sector; guess is in/out like the reference
 * (cuda_class.cu:289-290, correlation_class.cpp:360) */
int lk_correlate(lk_engine *e, int sector, float *guess_inout, lk_result *out);
/* all sectors in one device-resident batch (one launch per size class).
 * guesses: [S][6] host floats (unused slots ignored); out: [S] host records */
int lk_correlate_all(lk_engine *e, const float *guesses, lk_result *out);
/* same with device buffers, asynchronous on the engine's stream; d_guesses may be NULL
 * to use the engine-held guesses written by lk_adjust_initial_guess; d_results may be NULL to
 * leave the records in the engine's own record buffer (lk_get_results_device).  Note that
 * lk_update_sector moves a sector by the engine's OWN record of it: a caller that solves into a
 * buffer of its own and then calls lk_update_sector must copy the records back (lk_group does). */
int lk_correlate_all_device(lk_engine *e, const void *d_guesses, void *d_results);
/* the engine's own record buffer, [S] lk_result in device memory (valid until the next commit) */
int lk_get_results_device(lk_engine *e, const void **d_records);
/* lk_correlate_all with the engine-held guesses (lk_adjust_initial_guess) that does not wait: the
 * records follow the solve into an engine-owned pinned buffer; lk_wait_results blocks until they
 * are there and copies them to out [S].  One solve may be outstanding.  A frame loop uses the
 * pair to keep the host's per-frame bookkeeping off the GPU's critical path (lk_sequence_run). */
int lk_correlate_all_async(lk_engine *e);
int lk_wait_results(lk_engine *e, lk_result *out);

/* ---- frame-pipelined windows of a sequence ----------------------------------------- */
/* perform_multiframe_correlation's frame loop (manager_class.cpp:1380-1496) for the Eulerian description: the
 * sectors stay where they are, every frame brings a new deformed image, and the guess of frame f + 1 of a sector is
 * a function of that SECTOR's own earlier results (adjust_initial_guess, :2677-2699: p(f), or 2 p(f) - p(f-1) with the
 * first image as the reference) - it waits for no other sector.  One launch per pair pays the slow tail of every
 * pair: a launch lasts as long as its slowest sector.  Here K deformed frames are resident at once (a ring of
 * pyramids, filled on the next-frame stream like LK_IMG_NXT, :1438-1447) and ONE launch per size class solves the
 * whole window: its work items are (frame, sector) pairs drawn frame-major from a device-wide queue, and a sector's
 * parameters travel from frame to frame through a per-sector chain in device memory; the group that draws (f, s)
 * before (f - 1, s) is done waits for it without blocking the other sectors of its wavefront.
 * Records: the arithmetic of a (frame, sector) is the one-pair kernels' - in batch-invariant and in reference-order
 * mode the window's records are byte-identical to solving the pairs one after the other with
 * lk_adjust_initial_guess + lk_correlate_all*.  The default mode uses the fixed lane groups and the fast flavour
 * inside a window; if a damped system meets a bad pivot there, the same launch solves the window of the fast classes again
 * with the SAFE flavour (a pass gated on the device), before the window's ring slots are released and its records copied
 * (lk_stats.window_safe_reruns counts such windows).
 * Domains with sectors of more than 8192 samples (workgroup-wide groups, teams), and classes of more than 128 samples per
 * sector that have a starved pyramid level (config 5's geometry: their one-pair launch chain is the faster form), have
 * no pipelined instance: their windows run the frames one after the other on the device - same interface, same records. */
/* a ring of n_slots resident deformed-frame pyramids (grows; never shrinks) */
int lk_sequence_reserve(lk_engine *e, int n_slots);
/* upload + pyramid of one frame into ring slot `slot`, on the next-frame stream: may overlap a running
 * lk_correlate_* / window (the one concurrent call of section 8b's threading contract); a slot that a window
 * still reads is overwritten only after that window (stream order on the device) */
int lk_sequence_set_frame(lk_engine *e, int slot, const uint8_t *host_pixels, int rows, int cols, int step);
int lk_sequence_set_frame_device(lk_engine *e, int slot, const void *device_pixels, int rows, int cols, int step);
/* solve frames i = 0 .. n_frames-1 of a window: deformed image = ring slot (first_slot + i) % n_slots; undeformed
 * image = LK_IMG_UND (und_slot < 0) or ring slot und_slot for frame 0 and, with reference_previous, the previous
 * frame's deformed image for the others (image roles of manager_class.cpp:1386-1407).  Frame 0 starts from the
 * engine-held guesses (lk_adjust_initial_guess for that frame of the sequence, or whatever the caller put there),
 * every later frame from the guess rule above; the sequence state the next lk_adjust_initial_guess reads is left as
 * n_frames one-pair solves would leave it.  flags: 1 = copy the records to the host (lk_wait_sequence's out),
 * 2 = keep the guesses every frame started from (lk_get_sequence_results_device).  Does not wait. */
int lk_correlate_sequence_async(lk_engine *e, int und_slot, int first_slot, int n_frames, int reference_previous,
                                int constant_velocity, int flags);
/* block until the window is solved; out: [n_frames][S] records (frame-major) or NULL.  LK_ERROR_DEVICE if the
 * window is void (a bounded wait inside the kernel gave up: cannot happen unless the device loses wavefronts). */
int lk_wait_sequence(lk_engine *e, lk_result *out);
/* (flags & 1) the waited-for window's records [n_frames][S] in the engine's own pinned host memory - no copy; two buffers
 * alternate, so the pointer stays valid while the NEXT window is launched and solved (until the launch after that): a
 * frame loop digests window w while window w + 1 runs (lk_sequence_run) */
int lk_sequence_host_records(lk_engine *e, const lk_result **records);
/* page-locks, ahead of time, the record buffer the NEXT lk_correlate_sequence_async(..., flags & 1) of up to n_frames will
 * use (locking the 38 MB of a 16-pair window of 50 176 sectors takes 7 ms; the launch does it itself otherwise).  May be
 * called from another thread than the one that launches and waits, between a launch and the next one - a frame loop does
 * it beside its uploads and beside the running window (lk_sequence_run). */
int lk_sequence_prepare_host_records(lk_engine *e, int n_frames);
/* the window's records [n_frames][S] and (flags & 2) guesses [n_frames][S][6] in device memory */
int lk_get_sequence_results_device(lk_engine *e, const void **d_records, const void **d_guesses);
/* the last window's records into a caller's device buffer, frame f at d_dst + f * dst_pitch_records records
 * (dst_pitch_records >= S; the padded blocks of an all-gather), asynchronously on the engine's stream */
int lk_copy_sequence_records_device(lk_engine *e, void *d_dst, size_t dst_pitch_records);
/* 1: the last window ran on the frame-pipelined instances, 0: frame after frame */
int lk_sequence_is_pipelined(lk_engine *e);
/* (flags & 2) the guesses every frame of the last window started from, [n_frames][S][6], to the host */
int lk_get_sequence_guesses(lk_engine *e, float *guesses);

/* managerClass::adjust_initial_guess (manager_class.cpp:2602-2707), batched on the
 * device for every sector: frame 0 -> global guess + strain*(sector centre - global
 * centre); later frames -> constant_velocity ? 2*p_prev - p_prevprev : p_prev, where
 * p_prev are the results of the previous lk_correlate_all*. */
int lk_adjust_initial_guess(lk_engine *e, int frame, int constant_velocity,
                            const float *global_guess, float global_cx, float global_cy);
/* copy the engine-held guesses ([S][6]) to the host */
int lk_get_guesses(lk_engine *e, float *guesses);

/* ---- automatic initial guess: integer-pixel ZNCC search ------------------------------ */
/* The reference GUI's "Initial Guess: Automatic" (initialGuessEnum ic_Auto, enums.hpp:41; never implemented there).
 * Per sector, at pyramid level L: template = the sector's level-L samples, positions rounded (int)(v + 0.5f) and clamped
 * to the undeformed image like the solve's reads, values of the u8 level-L undeformed image; centre c = floor(g / 2^L + 0.5)
 * of the sector's guess g[0], g[1]; candidates c + (i, j), |i|, |j| <= radius (j = 0 for LK_FM_U) whose every shifted
 * sample lies inside the level-L deformed image.  Exact int64 sums St, Stt, Sd, Sdd, Std give
 * score = (n Std - St Sd) / sqrt((n Stt - St^2)(n Sdd - Sd^2)) (a candidate with n Sdd == Sd^2 is not valid).  Winner: the
 * highest score; ties go to the smaller i^2 + j^2, then the smaller j, then the smaller i.  Runner-up: the best score at
 * Chebyshev distance >= 2 from the winner (-2: none).  An OK sector gets g[0] = (c_x + i) 2^L and, for models with v,
 * g[1] = (c_y + j) 2^L; g[2..5] and the guesses of the other sectors stay as they were, bit for bit.  The results go to the
 * engine-held guesses and to the sequence history frame 0 leaves (previous_resulting_parameters = initial guess), so a
 * window or pair loop started afterwards continues as if they had been frame 0's guesses.  Integer sums: a sector gets
 * the same bits in any batch, shard or mode. */
enum {
  LK_GS_OK = 0,
  LK_GS_TEXTURELESS = 1,  /* n Stt == St^2 */
  LK_GS_NO_CANDIDATE = 2, /* no valid candidate */
  LK_GS_TOO_FEW = 3,      /* n < min_samples */
  LK_GS_TOO_LARGE = 4,    /* n > 2^22 */
  LK_GS_WEAK = 5          /* best score <= min_score */
};
#define LK_GS_MAX_RADIUS 32
#define LK_GS_MAX_SAMPLES (1 << 22)
typedef struct {
  int level;       /* -1 = py_stop; must be a level the engine builds */
  int radius;      /* R, pixels of that level, 0 .. LK_GS_MAX_RADIUS */
  int min_samples; /* <= 0: 9 */
  float min_score;
  int def_slot;    /* -1: LK_IMG_DEF; k >= 0: ring slot k (lk_sequence_set_frame) */
} lk_guess_search;
typedef struct {
  int center_x, center_y, shift_x, shift_y; /* level-L pixels; the winner is centre + shift */
  int n_samples, n_valid, status;           /* n_valid: candidates with a score; status: LK_GS_* (checked in the
                                             * order TOO_LARGE, TOO_FEW, TEXTURELESS, NO_CANDIDATE, WEAK) */
  double score, runner_up;                  /* -2 where there is none */
} lk_guess_match;
/* guesses_inout NULL: search about the engine-held guesses (asynchronous, engine stream);
 * else host [S][6]: centres in, refined guesses out (synchronous) - and engine-held either way */
int lk_search_guesses(lk_engine *e, const lk_guess_search *cfg, float *guesses_inout);
/* the matches of the last lk_search_guesses, [S] (waits for it) */
int lk_get_guess_search_info(lk_engine *e, lk_guess_match *out);

/* ---- rotation-aware automatic initial guess: ZNCC search over angle and shift ---------------- */
/* lk_search_guesses run at every angle theta_k = angle_center + k angle_step, k = -K .. K (K = n_half), for specimens that
 * rotate between the two frames (LK_FM_UVQ, LK_FM_UVUXUYVXVY; LK_FM_U and LK_FM_UV have no parameter that could carry an
 * angle and are refused with LK_ERROR_BAD_DOMAIN, as are n_half < 0, 2K+1 > LK_RS_MAX_ANGLES, a step that is not > 0 while
 * K > 0, a centre or step that is not finite, and whatever lk_search_guesses refuses of `search`).
 *   template   exactly lk_search_guesses': the sector's level-L samples in the reference's order, rounded (int)(v + 0.5f) and
 *              clamped to the undeformed image, u8 values of the level-L undeformed image; St, Stt and the checks TOO_LARGE,
 *              TOO_FEW, TEXTURELESS as there.
 *   table      lk_rotation_table: theta_k = (double)angle_center + k (double)angle_step, c_k = (float)cos(theta_k),
 *              s_k = (float)sin(theta_k), built on the host once per call; the kernels call no trigonometric function.
 *   position   of template sample (x, y) at angle k, every step in float32 and rounded on its own (no fused multiply-add):
 *              C = (cx0, cy0) 2^-L with (cx0, cy0) the committed level-0 centre (lk_get_sector_info); dx = (float)x - Cx,
 *              dy = (float)y - Cy; rx = c dx - s dy, ry = s dx + c dy; X = (int)floorf((Cx + rx) + 0.5f), Y likewise.  A
 *              positive angle is counter-clockwise in image coordinates as Warp<UVUXUYVXVY> sees it.  Candidate (k, i, j)
 *              reads the level-L deformed pixel (X + c_x + i, Y + c_y + j), nearest neighbour, (c_x, c_y) = lk_search_guesses'
 *              rounded centre of g[0], g[1].  Several samples may land on one pixel; n stays the template's count.
 *   validity   every deformed sample of the candidate inside the level-L deformed image (per angle a rectangle of shifts,
 *              from the rotated bounding box) and n Sdd != Sd^2.  The score is lk_search_guesses' exact expression.
 *   winner     over (k, i, j): the higher score, then the smaller |k|, then the smaller k, then lk_search_guesses' rule
 *              (the smaller i^2 + j^2, then the smaller j, then the smaller i).  Statuses are checked in lk_search_guesses'
 *              order; NO_CANDIDATE: no valid candidate at any angle.
 *   guess      an OK sector gets g[0], g[1] as lk_search_guesses writes them and, LK_FM_UVUXUYVXVY: g[2] = c - 1.f,
 *              g[3] = 0.f - s, g[4] = s, g[5] = c - 1.f; LK_FM_UVQ: g[2] = s (the linearised warp's best q), g[3..5] untouched.
 *              A sector that is not OK keeps its six words, bit for bit.  Engine-held guesses and the sequence history are
 *              written as lk_search_guesses writes them.
 *   refined    angle_refined = (float)(theta_k + t angle_step), t = 0.5 (s- - s+) / (s- - 2 s0 + s+) from the best scores of
 *              the angles k-1, k, k+1 of the winner, clamped to [-0.5, 0.5]; t = 0 unless both neighbours have a score and
 *              the denominator is negative.  Reported only: the guess uses the table's c_k, s_k.
 * A sector without a winner reports shift 0, angle_index 0, score and runner-ups -2 and theta_0 as both angles.  With
 * n_half = 0 and angle_center = 0 the pass equals lk_search_guesses: the same g[0], g[1] and shared match fields, byte for
 * byte (an affine OK sector gets g[2..5] = +0.0f).  Integer sums, unfused float steps: a sector gets the same bits in any
 * batch and mode, whatever other sectors or angles are in the call. */
#define LK_RS_MAX_ANGLES 361
typedef struct {
  lk_guess_search search;   /* level, radius, min_samples, min_score, def_slot: lk_search_guesses' meaning */
  float angle_center;       /* radians, counter-clockwise in image coordinates as Warp<UVUXUYVXVY> sees it */
  float angle_step;         /* radians, > 0 (ignored when n_half == 0) */
  int n_half;               /* K: angles theta_k = center + k step, k = -K .. K; 2K+1 <= LK_RS_MAX_ANGLES */
} lk_rotated_search;
typedef struct {            /* 64 bytes, one per sector */
  int center_x, center_y, shift_x, shift_y;    /* as lk_guess_match, at the winning angle */
  int n_samples, n_valid, status, angle_index; /* n_valid: scored candidates over ALL angles; status: LK_GS_*; k of the winner */
  double score, runner_up;  /* runner_up: lk_guess_match's rule, inside the winning angle */
  double angle_runner_up;   /* best per-angle score among angles with |k - k_win| >= 2; -2: none */
  float angle, angle_refined; /* theta_k_win; the same plus the parabola's offset */
} lk_rotated_match;
/* guesses_inout as for lk_search_guesses (NULL: about the engine-held guesses, asynchronous on the engine stream) */
int lk_search_rotated(lk_engine *e, const lk_rotated_search *cfg, float *guesses_inout);
/* the matches of the last lk_search_rotated, [S] (waits for it) */
int lk_get_rotated_search_info(lk_engine *e, lk_rotated_match *out);
/* its best score per angle, [S][2K+1], -2 where an angle has no score (waits for it) */
int lk_get_rotated_search_profile(lk_engine *e, double *best_per_angle);
/* host: {c_k, s_k}, [2K+1][2], the table the kernels read; LK_ERROR_BAD_DOMAIN for a bad n_half, step or centre */
int lk_rotation_table(const lk_rotated_search *cfg, float *cos_sin_out);

/* ---- stereo initial guess: ZNCC search along the epipolar curve ------------------------------ */
/* The cross-camera pair of a calibrated rig (lk_stereo_points below: camera 0's reference frame as LK_IMG_UND, a frame of
 * camera 1 as the deformed image) has its match on one curve: the image in camera 1 of camera 0's ray through the sector's
 * centre, cut to a depth range.  lk_search_epipolar scores lk_search_guesses' template at the integer stations of that curve
 * and in a band of +-B pixels across it, instead of a square of (2R+1)^2 shifts about a given centre (csrc/lk_epipolar_search.hip,
 * csrc/lk_epipolar_search.cpp).  The incoming g[0], g[1] are not a search centre here: the curve is.
 *   curve      lk_epipolar_curves, on the host, in double, with the camera functions of lk_stereo_project / lk_stereo_triangulate
 *              (csrc/lk_stereo.hpp), once per call.  Of sector s, at level L, with N = n_nodes:
 *                start     c = the committed level-0 centre (lk_get_sector_info) widened to double; m = c undistorted in camera
 *                          0; the ray o + z d of m with d = R0^T K0^-1 (m, 1), so that z is the depth along camera 0's axis.
 *                nodes     rho_near = 1 / z_near, rho_far = 1 / z_far (the sector's depth_range entry where one is given);
 *                          rho_k = rho_near + k ((rho_far - rho_near) / (N - 1)), k = 0 .. N-1; P_k = o + (1 / rho_k) d;
 *                          q_k = P_k projected into camera 1, lens included; w_k = (q_k - c) / 2^L, a displacement in level-L
 *                          pixels as g / 2^L is for the other searches.
 *                axis      a = x if |w_{N-1}.x - w_0.x| >= |w_{N-1}.y - w_0.y|, else y; b is the other coordinate.
 *                stations  lo, hi = the smaller and the larger of w_0.a, w_{N-1}.a; the integers t = ceil(lo) .. floor(hi), or,
 *                          where there is none, the single station t = floor((lo + hi) / 2 + 0.5).  Index m = t - t_first.
 *                segment   of station t: the segments [k, k+1] taken in the order of increasing a (k = 0, 1, .. where
 *                          w_{N-1}.a >= w_0.a, else k = N-2, N-3, ..), the first whose larger a-end is >= t, or the last of
 *                          them where there is none (the single station only): where t lies inside the node range this is the
 *                          first segment that contains t.  lambda = (t - w_k.a) / (w_{k+1}.a - w_k.a), 0 for a zero
 *                          denominator, clamped to [0, 1] (which changes it for the single station only).
 *                          other(t) = floor(w_k.b + lambda (w_{k+1}.b - w_k.b) + 0.5);  node(t) = lambda < 0.5 ? k : k+1;
 *                          inv_depth(t) = rho_k + lambda (rho_{k+1} - rho_k).
 *                shape     (shape = 1) A_k, the 2 x 2 Jacobian at c of the map camera-0 pixel -> camera-1 pixel induced by the
 *                          plane through P_k with normal `normal` (a world vector; all zero: camera 0's optical axis, the third
 *                          row of R0), by central differences with a step of one level-0 pixel: f(p) = p undistorted in camera
 *                          0, its ray met with the plane at z = ((P_k - o) . n) / (d . n), projected into camera 1;
 *                          A_k = {(f(c + ex) - f(c - ex)).x / 2, (f(c + ey) - f(c - ey)).x / 2, the same of .y}, rounded to four
 *                          floats {a11, a12, a21, a22}.  A point fails where the undistortion or the projection refuses it, d . n
 *                          is 0, z is not > 0 or a value is not finite.
 *                status    LK_GS_NO_CURVE: c outside camera 0's lens; a node the projection refuses (or a w_k that is not
 *                          finite or not below 2^30 in size); node a-coordinates that are not monotone (equal neighbours are);
 *                          a shape point that fails.  LK_GS_TOO_LONG: more than LK_EP_MAX_STATIONS stations, or a run of
 *                          stations of one node times 2B+1 above LK_EP_MAX_GROUP.  Such a curve has no stations.  Else 0.
 *   candidates (m, b), |b| <= B: the level-L displacement (t, other(t) + b) for axis x, (other(t) + b, t) for axis y.
 *   template   lk_search_guesses', bit for bit: the samples, their rounding and clamping, St, Stt, TOO_LARGE, TOO_FEW,
 *              TEXTURELESS.
 *   position   template sample (x, y) reads the level-L deformed pixel (X, Y) + displacement, nearest neighbour.  shape = 0:
 *              (X, Y) = (x, y).  shape = 1: lk_search_rotated's form with the full matrix A of node(t) about C = c 2^-L, every
 *              float32 product and sum rounded on its own: dx = (float)x - Cx, dy = (float)y - Cy; rx = a11 dx + a12 dy,
 *              ry = a21 dx + a22 dy; X = (int)floorf((Cx + rx) + 0.5f), Y likewise.
 *   validity   every sample of the candidate inside the level-L deformed image, and n Sdd != Sd^2.  The score is
 *              lk_search_guesses' expression from exact integer sums.
 *   winner     the higher score, then the smaller |b|, then the smaller b, then the smaller m.
 *   reported   profile[m] = the best score of station m over b, -2 where it has none;  runner_up = the best profile[m'] with
 *              |m' - m_win| >= 2 (-2: none): the ambiguity along the curve;  n_valid = scored candidates over the whole curve;
 *              station_refined = (float)(m_win + t) with t lk_search_rotated's parabola offset over profile[m_win - 1 ..
 *              m_win + 1] (0 unless both neighbours exist and have a score and the denominator is negative; clamped to
 *              [-0.5, 0.5]);  inv_depth = (float)(inv_depth(m_win) + |t| (inv_depth(m_win + sign t) - inv_depth(m_win))).  Both
 *              are reported only.
 *   status     checked in this order: NO_CURVE, TOO_LONG, TOO_LARGE, TOO_FEW, TEXTURELESS, NO_CANDIDATE, WEAK (best <=
 *              min_score).
 *   guess      an OK sector gets g[0], g[1] = (float)((double)displacement * 2^L), as the other searches form them; with
 *              shape = 1 also g[2..5] = (a11 - 1.f, a12, a21, a22 - 1.f) of the winner's node, lk_search_rotated's layout; with
 *              shape = 0 g[2..5] stay as they were.  A sector that is not OK keeps its six words, bit for bit.  The engine-held
 *              guesses and the sequence history are written as lk_search_guesses writes them.
 *   match      lk_epipolar_match; a sector without a winner reports zeros and scores of -2.
 *   errors     LK_ERROR_BAD_DOMAIN with a message that starts with the function's name: whatever lk_search_guesses refuses of
 *              `search` but the radius; LK_FM_U; shape = 1 on a model other than LK_FM_UVUXUYVXVY; a band outside 0 ..
 *              LK_EP_MAX_BAND; n_nodes outside 2 .. LK_EP_MAX_NODES; depths that are not 0 < z_near <= z_far, both finite, in
 *              the configuration or in an entry of depth_range; a shape other than 0 or 1; a normal that is not finite;
 *              non-zero reserved words; cams NULL or a camera that lk_stereo_project refuses.
 *   bytes      integer sums, unfused float steps, one table built on the host: a sector's match, profile and guess are the same
 *              bits in any batch, mode, ring slot or call, whatever other sectors are in the launch. */
#define LK_GS_NO_CURVE 6    /* further values of the LK_GS_* statuses */
#define LK_GS_TOO_LONG 7
#define LK_EP_MAX_BAND 8
#define LK_EP_MAX_NODES 33
#define LK_EP_MAX_STATIONS 2048
#define LK_EP_MAX_GROUP 4096
typedef struct lk_epipolar_search {   /* 80 bytes */
  lk_guess_search search;   /* level, min_samples, min_score, def_slot: lk_search_guesses' meaning; radius: the band B */
  int     n_nodes;          /* N, 2 .. LK_EP_MAX_NODES */
  int     shape;            /* 0: the template is shifted; 1: mapped by the plane-induced Jacobian of the station's node */
  int     reserved[3];      /* must be 0 */
  double  z_near, z_far;    /* depth along camera 0's optical axis, 0 < z_near <= z_far */
  double  normal[3];        /* shape = 1: the world normal of the surface; all zero: camera 0's optical axis */
} lk_epipolar_search;
typedef struct lk_epipolar_curve {    /* 32 bytes, one per sector */
  int32_t axis;             /* 0: stations along x; 1: along y */
  int32_t first_station;    /* t of station 0, level-L pixels */
  int32_t n_stations;
  int32_t first_index;      /* of station 0 in the station arrays */
  int32_t status;           /* 0, LK_GS_NO_CURVE or LK_GS_TOO_LONG */
  int32_t reserved[3];
} lk_epipolar_curve;
typedef struct lk_epipolar_match {    /* 64 bytes, one per sector */
  int32_t shift_x, shift_y; /* the winner's displacement, level-L pixels */
  int32_t station;          /* m of the winner */
  int32_t band_offset;      /* b of the winner */
  int32_t node;             /* node(t) of the winner's station */
  int32_t n_samples, n_valid, status; /* status: LK_GS_* */
  double  score, runner_up; /* -2 where there is none */
  float   station_refined, inv_depth;
  int32_t reserved[2];
} lk_epipolar_match;
struct lk_camera;             /* (defined with lk_stereo_points below) */
/* cams: [2]; depth_range: NULL or host [S][2] {z_near, z_far} per sector; guesses_inout as for lk_search_guesses (NULL: the
 * engine-held guesses, asynchronous on the engine stream) */
int lk_search_epipolar(lk_engine *e, const lk_epipolar_search *cfg, const struct lk_camera *cams, const double *depth_range,
                       float *guesses_inout);
/* the matches of the last lk_search_epipolar, [S] (waits for it) */
int lk_get_epipolar_search_info(lk_engine *e, lk_epipolar_match *out);
/* its curves [S] (or NULL) and its best score per station, concatenated: sector s at curves_out[s].first_index, n_stations
 * values, -2 where a station has no score (waits for it); *n_stations_out (or NULL): the length of the profile.  profile_out
 * NULL: the curves and the length alone */
int lk_get_epipolar_search_profile(lk_engine *e, lk_epipolar_curve *curves_out, double *profile_out, int *n_stations_out);
/* Host, needs no engine: the table the kernels read, of n centres [n][2] (level-0 pixels of camera 0) at pyramid level
 * `level` >= 0 (cfg->search.level is not read; of `search` only the radius is).  curves_out [n]; *n_stations_out: the stations
 * of all curves together.  The station arrays other_out, node_out, inv_depth_out [capacity] and shape_out [n][N][4] (read only
 * with cfg->shape = 1) may all be NULL to ask for the curves and the count alone; otherwise capacity must be at least that
 * count.  LK_ERROR_BAD_DOMAIN for what `errors` lists of the configuration, the cameras and depth_range, for n < 1, a level
 * outside 0 .. 30, a null centres, curves_out or n_stations_out, or a capacity that is too small. */
int lk_epipolar_curves(const lk_epipolar_search *cfg, const struct lk_camera *cams, int n, const float *centres,
                       const double *depth_range, int level, lk_epipolar_curve *curves_out, int *n_stations_out, int capacity, int32_t *other_out,
                       int32_t *node_out, double *inv_depth_out, float *shape_out);

/* ---- recovery pass: re-solve failed sectors from their converged neighbours ------------- */
/* lk_reseed_failed repairs the engine-held records of the last lk_correlate_all* / lk_wait_results after the fact: a sector
 * that failed is given a guess extrapolated from neighbours that converged and is solved again; what was recovered seeds
 * the next ring in the next round.  Everything stays on the device between the rounds (csrc/lk_reseed.hip); the host reads
 * ten small integers per round to size the launches.
 *   good      a sector is GOOD when its record has LK_ERROR_NONE, finite parameters (the model's P) and finite chi and,
 *             if chi_max > 0, chi <= chi_max.  Every other sector is FAILED.
 *   rounds    each round computes a guess for every failed sector that has at least min_neighbours good sectors within
 *             `radius` (centre to centre, level-0 pixels, distance <= radius, tested in double) and has not been tried with
 *             that very neighbour set; the sectors that got a guess are solved in ONE batch.  The neighbours are the sectors
 *             good at the start of the round, so a sector recovered in round r seeds others from round r + 1 on.  The call
 *             ends after max_rounds, or earlier when a round finds nothing to try (which is what follows a round that
 *             recovered nothing).
 *   guess     the plain mean, over the sector's good neighbours, of each neighbour's parameters carried to the sector's
 *             centre by the rule lk_adjust_initial_guess applies to the global guess (manager_class.cpp:2602-2707), with
 *             (dx, dy) = c_sector - c_neighbour:
 *               LK_FM_UVUXUYVXVY  g0 = p0 + dx p2 + dy p3, g1 = p1 + dx p4 + dy p5, g2..g5 = p2..p5
 *               LK_FM_UVQ         g0 = p0 - dy p2, g1 = p1 + dx p2, g2 = p2
 *               LK_FM_U / _UV     g = p
 *             Differences, products and sums are formed in double from the float centres and parameters (no fused
 *             multiply-add: each product and each sum is rounded to double); the mean sum / count is rounded to float once.
 *             A float64 restatement reproduces it up to the order of the double sum.  That order is fixed: the neighbours
 *             are visited cell by cell of a grid of cell size `radius` over the centres (rows iy - 1, iy, iy + 1, each from
 *             ix - 1 to ix + 1), by ascending sector index within a cell, dealt to 16 lanes in turn and summed by a
 *             fixed butterfly - the same bits on every run.
 *   retry     the solve is the engine's own in its current mode (forward default, batch-invariant or backward) through its
 *             ordinary launch code, on the retried sectors only.  The new record replaces the old one only if it is good
 *             by the rule above and, if the old record had LK_ERROR_NONE and a finite chi, its chi is lower than the old one.
 *             Otherwise the sector is LK_RESEED_NOT_IMPROVED and is tried again only if a later round gives it more good
 *             neighbours.
 *   kept      for a sector that was not replaced - never tried, tried and rejected, or good - the record, the engine-held
 *             last parameters (which lk_adjust_initial_guess continues from), lk_get_last_evaluated_parameters and the
 *             per-sector counters (lk_get_sector_stats) are byte for byte what they were before the call.  For a replaced
 *             sector they are the retry's.  The engine-held guesses (lk_get_guesses) never change.
 *   counters  lk_get_stats after the call describes the retry solves, summed over the rounds (sectors = solves, a sector
 *             tried twice counts twice; all zero when nothing was tried); solve_ms is the last round's solve.
 *   errors    LK_ERROR_BAD_DOMAIN with a message: no committed sectors; no batch solve of them yet (or one not waited for);
 *             a bad configuration (radius or chi_max not finite, radius <= 0, min_neighbours < 1, max_rounds outside
 *             1..64); reference-order mode is on - that mode's records are by definition the CPU engine's, and the CPU
 *             engine has no such pass.
 *   scope     one engine, one pair.  Sequence windows (lk_correlate_sequence_async), lk_tracker / lk_sequence_run, lk_group
 *             and the CudaClass adapter do not call it and are not changed by it. */
enum {
  LK_RESEED_GOOD = 0,          /* good when the call began: never touched */
  LK_RESEED_RECOVERED = 1,     /* a retry was accepted */
  LK_RESEED_NO_NEIGHBOUR = 2,  /* failed, and never had min_neighbours good neighbours: never tried */
  LK_RESEED_NOT_IMPROVED = 3,  /* failed, tried, every retry rejected */
  LK_RESEED_PLANNED = 4        /* lk_reseed_plan only: failed, and guesses_out holds a guess for it */
};
typedef struct lk_reseed_config {
  float chi_max;       /* a record with error_none and chi > chi_max counts as failed; <= 0: the error code alone decides */
  float radius;        /* neighbours of a sector: sectors whose centre lies within this many level-0 pixels of its centre */
  int min_neighbours;  /* >= 1; a failed sector with fewer good neighbours waits for a later round */
  int max_rounds;      /* 1..64 */
} lk_reseed_config;
typedef struct lk_reseed_info {   /* one per sector */
  int32_t status;      /* LK_RESEED_* */
  int32_t round;       /* round (from 0) in which the sector was recovered, else -1 */
  int32_t neighbours;  /* good neighbours behind the last guess that was tried (0 if none was); lk_reseed_plan: good
                        * neighbours found (failed sectors; 0 for good ones) */
  float chi_before;    /* chi of the record the call found */
} lk_reseed_info;
/* out: [S] the records after the pass, or NULL; n_recovered: sectors replaced, or NULL.  Synchronous. */
int lk_reseed_failed(lk_engine *e, const lk_reseed_config *cfg, lk_result *out, int *n_recovered);
/* [S] what the last lk_reseed_failed did (also after a call that found nothing to do) */
int lk_get_reseed_info(lk_engine *e, lk_reseed_info *out);
/* the planning step of one round alone, on records the caller supplies [S]: nothing is solved and no engine state
 * changes (max_rounds is not used).  guesses_out [S][6]: the guess of every LK_RESEED_PLANNED sector, zeros elsewhere;
 * info_out [S]: status GOOD / NO_NEIGHBOUR / PLANNED, round -1.  Needs committed sectors only. */
int lk_reseed_plan(lk_engine *e, const lk_reseed_config *cfg, const lk_result *records, float *guesses_out,
                   lk_reseed_info *info_out);

/* ---- strain field: a windowed plane fit of the solved displacements ----------------------- */
/* lk_strain_field turns one displacement record per sector into one strain record per sector: a pointwise least-squares
 * plane fit of (u, v) over the good sectors of a strain window, the displacement gradients of that plane, the strain
 * tensor of the gradients and its principal values (csrc/lk_strain.hip).
 *   data      of a sector: position = the engine's committed centre c (lk_get_sector_info), not undCenterX/Y of the record;
 *             displacement u = p[0] and v = p[1]; LK_FM_U has v = 0 everywhere, hence vx = vy = 0.  The per-sector
 *             gradient parameters of LK_FM_UVUXUYVXVY are not used.
 *   good      the recovery pass's rule (one shared device function): LK_ERROR_NONE, finite parameters (the model's P),
 *             finite chi and, if chi_max > 0, chi <= chi_max.
 *   window    of sector s: every good sector j, s itself included when good, with dx^2 + dy^2 <= r^2, where
 *             (dx, dy) = c_j - c_s is formed in double from the float centres and r = (double)radius.  Each product and
 *             each sum is rounded to double (no fused multiply-add).  n = the number of such sectors.
 *   fit       all in double, in the window's coordinates x = dx, y = dy: the sums Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu,
 *             Sv, Sxv, Syv; the centred moments Cxx = Sxx - Sx Sx / n, Cxy = Sxy - Sx Sy / n, Cyy = Syy - Sy Sy / n,
 *             Cxu = Sxu - Sx Su / n, Cyu = Syu - Sy Su / n, Cxv, Cyv alike; D = Cxx Cyy - Cxy Cxy;
 *               ux = (Cyy Cxu - Cxy Cyu) / D,  uy = (Cxx Cyu - Cxy Cxu) / D,  vx, vy by the same formulas from Cxv, Cyv;
 *               u = Su / n - ux (Sx / n) - uy (Sy / n)  (the plane at c_s),  v alike.
 *             A second walk over the same window sums the squared residuals ru = u_j - (u + ux dx + uy dy), rv alike;
 *             residual = sqrt(sum(ru^2 + rv^2) / n).  Each output is rounded to float once.
 *   tensor    lk_strain_from_gradient (one function for the kernel and the host, csrc/lk_strain.hpp) of the four float
 *             gradients as stored, computed in double, each result rounded to float:
 *               Green-Lagrange  exx = ux + (ux^2 + vx^2) / 2,  eyy = vy + (uy^2 + vy^2) / 2,
 *                               exy = (uy + vx) / 2 + (ux uy + vx vy) / 2
 *               small           exx = ux,  eyy = vy,  exy = (uy + vx) / 2
 *               e1, e2 = (exx + eyy) / 2 +- sqrt(((exx - eyy) / 2)^2 + exy^2),  theta = atan2(2 exy, exx - eyy) / 2.
 *             A record's six tensor fields are a function of its four gradient fields alone.
 *   status    checked in this order: TOO_FEW  n < min_neighbours;  DEGENERATE  Cxx Cyy == 0 or D <= 1e-6 Cxx Cyy (the
 *             centres of the window on a line: one minus their squared correlation is at most 1e-6; scale-free);
 *             FILLED  the fit is valid but s itself is not good - its values are interpolated from its neighbours;
 *             OK  otherwise.  TOO_FEW and DEGENERATE: every float field is 0, neighbours = n.
 *   order     fixed, as for the recovery pass: the window is visited cell by cell of a grid of cell size `radius` over the
 *             centres (rows iy - 1, iy, iy + 1, each from ix - 1 to ix + 1), by ascending sector index within a cell,
 *             dealt to the lanes of a group (16 or 64, chosen from the sector count and the number of cells) in turn and
 *             summed by a fixed butterfly: the same bytes on every run for the same domain, records and configuration.
 *             A float64 restatement reproduces it up to the order of the double sums.
 *   modes     allowed in every mode, reference-order mode included: the call reads records and writes nothing of the
 *             engine's - records, guesses, last parameters, counters and lk_get_reseed_info stay byte for byte.  It also
 *             starts nothing the engine has put off: a rebuild of the sample lists that waits for the next solve (after
 *             lk_update_sector turned a sector into a list, or after a change of mode) keeps waiting, and the centres are
 *             the ones the engine holds at the time of the call.  Sectors that lk_translate_sectors, lk_rewarp_sectors or
 *             lk_update_sector have already moved are fitted at their new centres: for records solved before the move,
 *             call lk_strain_field before moving the sectors.
 *   errors    LK_ERROR_BAD_DOMAIN with a message: null configuration or output; no committed sectors; records == NULL
 *             before any batch solve of the committed sectors, or with one still in flight; radius not finite or <= 0;
 *             chi_max not finite; min_neighbours < 3; unknown tensor.
 *   scope     one engine.  lk_group, lk_tracker, the report CSV and the CudaClass adapter do not call it; per-frame strain
 *             of a sequence window is had by passing each frame's records. */
enum { LK_STRAIN_OK = 0, LK_STRAIN_FILLED = 1, LK_STRAIN_TOO_FEW = 2, LK_STRAIN_DEGENERATE = 3 };
enum { LK_STRAIN_GREEN_LAGRANGE = 0, LK_STRAIN_SMALL = 1 };
typedef struct lk_strain_config {
  float radius;        /* strain window: sectors whose centre lies within this many level-0 pixels (<=, tested in double) */
  float chi_max;       /* the recovery pass's "good" rule; <= 0: the error code alone decides */
  int min_neighbours;  /* >= 3, counting the sector itself when it is good */
  int tensor;          /* LK_STRAIN_GREEN_LAGRANGE / LK_STRAIN_SMALL */
} lk_strain_config;
typedef struct lk_strain {     /* 64 bytes, one per sector */
  float u, v;                  /* the fitted plane at the sector's centre */
  float ux, uy, vx, vy;        /* displacement gradients */
  float exx, eyy, exy, e1, e2, theta;  /* tensor, principal strains e1 >= e2, angle of e1 in radians */
  float residual;              /* sqrt(sum(ru^2 + rv^2) / n) of the fit, pixels */
  int32_t neighbours, status, reserved;
} lk_strain;
/* records: host [S], or NULL = the engine-held records of the last batch solve (after lk_reseed_failed: the repaired ones).
 * Synchronous.  Changes no engine state. */
int lk_strain_field(lk_engine *e, const lk_strain_config *cfg, const lk_result *records, lk_strain *out);
/* the kernel's own tensor function compiled for the host, like lk_compose_inverse: grad = {ux, uy, vx, vy},
 * out6 = {exx, eyy, exy, e1, e2, theta}.  LK_ERROR_BAD_DOMAIN for an unknown tensor or a null pointer. */
int lk_strain_from_gradient(int tensor, const float *grad4, float *out6);

/* ---- outlier flags: the (detrended) normalised median test of the solved field ------------- */
/* lk_flag_outliers is the spatial validity check of the solved displacements: a sector that converged cleanly to the wrong
 * place (a neighbouring speckle, a reflection, a crack edge) has LK_ERROR_NONE and an unremarkable chi, and the "good" rule
 * passes it.  The test compares each sector's displacement with the median of its neighbours', normalised by their median
 * absolute deviation (Westerweel & Scarano 2005) - by default after taking the window's least-squares plane out of both,
 * since a displacement gradient of a few percent otherwise hides half-pixel outliers and flags healthy edge sectors
 * (csrc/lk_outlier.hip).
 *   data      of a sector: position = the engine's committed centre c; displacement u = p[0] + 0.0f and v = p[1] + 0.0f
 *             (v = 0 for LK_FM_U), so -0 enters as +0.
 *   good      the shared rule of the recovery pass and the strain field (one device function): LK_ERROR_NONE, finite
 *             parameters (the model's P), finite chi and, if chi_max > 0, chi <= chi_max.
 *   window    of sector s: every sector j != s that is good, was not flagged in the pass before, and has
 *             dx^2 + dy^2 <= r^2, where (dx, dy) = c_j - c_s is formed in double from the float centres and
 *             r = (double)radius.  n = the number of such sectors; s itself is never counted.
 *   detrend   = 1: the plane of lk_strain_field's `fit` paragraph over that window - the same sums, moments, D and
 *             DEGENERATE rule, all in double without fused multiply-add: u0 = Su / n - ux (Sx / n) - uy (Sy / n);
 *             e_j = (float)(u_j - (u0 + ux dx_j + uy dy_j)), e_s = (float)(u_s - u0); v alike.
 *             = 0: e_j = u_j, e_s = u_s (the plain Westerweel-Scarano test); no fit, and no DEGENERATE status.
 *   median    of n floats x: (float)(((double)x[(n - 1) / 2] + (double)x[n / 2]) / 2) of the values sorted as IEEE numbers
 *             (a zero of either sign counts as +0).  It does not depend on the order the window is visited in.
 *   test      per component: med = median(e_j); mad = median((float)fabs((double)e_j - (double)med));
 *             ratio = (float)(fabs((double)e_s - (double)med) / ((double)mad + (double)eps)).  The sector is flagged when
 *             max(ratio_u, ratio_v) > threshold, compared on the double values before the rounding to float.
 *   status    checked in this order: TOO_FEW  n < min_neighbours;  DEGENERATE  detrend only: Cxx Cyy == 0 or
 *             D <= 1e-6 Cxx Cyy (the window's centres on a line);  NOT_GOOD  s itself fails the good rule: med and mad are
 *             reported, both ratios are 0, the sector is never flagged;  FLAGGED;  OK.  TOO_FEW and DEGENERATE: every float
 *             field is 0.  neighbours = n always.
 *   passes    pass 0 excludes nothing; pass k leaves the sectors flagged in pass k - 1 (and only those) out of every
 *             window - they are still tested themselves.  The records and flags returned are the last pass's, and
 *             n_flagged counts them.  Two passes cure the usual false flag: a healthy neighbour whose plane was bent by
 *             the outlier next to it.
 *   order     plain mode: every float field is independent of the visiting order, hence of the lane group and of whether
 *             the window was kept in LDS.  Detrended mode: the plane's sums are added in lk_strain_field's fixed order
 *             (cell by cell, by ascending sector index within a cell, dealt to 16 or 64 lanes, a fixed butterfly): the same
 *             bytes on every run; a float64 restatement reproduces them up to the order of the double sums.
 *   records   records == NULL reads the engine-held records of the last batch solve (after lk_reseed_failed: the repaired
 *             ones), else the caller's [S].  records_out, if not NULL, receives the records that were read, with
 *             errorCode = LK_ERROR_OUTLIER in the flagged sectors when mark = 1.  mark = 1 with records == NULL writes that
 *             code into the engine-held records of the flagged sectors as well: the only engine state the call ever
 *             changes.  A following lk_reseed_failed then retries those sectors and keeps them out of its neighbour means;
 *             a following lk_strain_field(records = NULL) fills them from their neighbours.  With mark = 0 nothing of the
 *             engine moves - records, guesses, last parameters, counters, lk_get_reseed_info - and, as for
 *             lk_strain_field, a rebuild of the sample lists that waits for the next solve keeps waiting.
 *   modes     allowed in every mode, reference-order mode included; but mark = 1 on engine-held records is refused in
 *             reference-order mode: that mode's records are by definition the CPU engine's.
 *   errors    LK_ERROR_BAD_DOMAIN with a message: null configuration or output; no committed sectors; records == NULL
 *             before any batch solve of the committed sectors, or with one still in flight; radius not finite or <= 0;
 *             chi_max not finite; eps or threshold not finite or <= 0; min_neighbours < 4 with detrend (a plane has three
 *             unknowns and the sector itself is not counted), < 3 without; detrend or mark not 0 / 1; passes outside 1..4.
 *   scope     one engine.  lk_group, lk_tracker, the report CSV and the CudaClass adapter do not call it.  No weights inside
 *             the window; lk_parameter_uncertainty's sigma does not enter eps. */
enum { LK_OUTLIER_OK = 0, LK_OUTLIER_FLAGGED = 1, LK_OUTLIER_TOO_FEW = 2, LK_OUTLIER_DEGENERATE = 3, LK_OUTLIER_NOT_GOOD = 4 };
typedef struct lk_outlier_config {
  float radius;        /* window: sectors whose centre lies within this many level-0 pixels (<=, tested in double) */
  float chi_max;       /* the shared "good" rule; <= 0: the error code alone decides */
  float eps;           /* noise floor of the normalisation, pixels; > 0 */
  float threshold;     /* flagged when max(ratio_u, ratio_v) > threshold; > 0 */
  int min_neighbours;  /* >= 4 with detrend, >= 3 without; the sector itself is never counted */
  int detrend;         /* 1: test the residual to the window's plane; 0: the plain Westerweel-Scarano test */
  int passes;          /* 1..4: pass k leaves the sectors flagged in pass k - 1 out of every window */
  int mark;            /* 1: flagged sectors get errorCode = LK_ERROR_OUTLIER in the records the call returns / holds */
} lk_outlier_config;
typedef struct lk_outlier {       /* 32 bytes, one per sector, of the last pass */
  float med_u, med_v;             /* median of the window's (detrended) u, v */
  float mad_u, mad_v;             /* median of |e_j - med| */
  float ratio_u, ratio_v;
  int32_t neighbours, status;
} lk_outlier;
/* records: host [S] or NULL; out: [S]; records_out: host [S] or NULL; n_flagged: or NULL.  Synchronous. */
int lk_flag_outliers(lk_engine *e, const lk_outlier_config *cfg, const lk_result *records, lk_outlier *out,
                     lk_result *records_out, int *n_flagged);
/* the kernel's own selection and ratio arithmetic compiled for the host (csrc/lk_outlier.hpp): the record of a sector whose
 * window holds the n values e_u, e_v and whose own values are es_u, es_v (status OK or FLAGGED, neighbours = n).
 * LK_ERROR_BAD_DOMAIN for a null pointer, n < 1, a value that is not finite, or eps / threshold not finite or <= 0. */
int lk_outlier_from_window(int n, const float *e_u, const float *e_v, float es_u, float es_v, float eps, float threshold,
                           lk_outlier *out);

/* ---- per-sector uncertainty: the covariance of the solved parameters ---------------------- */
/* lk_parameter_uncertainty gives every sector the standard deviation of each solved parameter: one evaluation at the
 * record's parameters, the Gauss-Newton normal matrix A and the residual chi of that evaluation, Cov(p) = s^2 A^-1 with
 * s^2 = chi / (n - P) (csrc/lk_uncertainty.hip).  chi alone is a residual, not an error bar: a sector on a one-directional
 * texture converges with a small chi and a useless u (the aperture problem) - and a long uncertainty ellipse.
 *   level     L = py_start, the finest level the solve reaches.  p = the record's resultingParameters brought to level L's
 *             scale by the rule the solve uses between levels (translate_model_parameters, pyramid_class.cpp:260-287:
 *             p[0] and p[1] times 2^-L).  The samples are the sector's level-L list or implicit rectangle (a rectangle row
 *             by row, a list in its order), the centre is the committed centre times 2^-L as in the solve.
 *   sample    the forward evaluation, whatever lk_set_update says: (xd, yd) = W(x_i; p) by the model, the deformed image's
 *             value and gradient there by the engine's interpolation, V_i = und(node) - def(xd, yd), J_i = gradient times
 *             dW/dp - the device functions and the float arithmetic of the forward solve.  The products J_a J_b, J_a V and
 *             V^2 are formed in double from those floats and summed in double (no fused multiply-add).  A (upper
 *             triangle, row-major), b and chi are the 28 sums of a sector, in that order, padded with zeros for P < 6.
 *   order     the lane group is fixed by the sector's own level-0 sample count: 16 lanes up to 512 samples, 64 up to 8192,
 *             512 above (the backward solve's groups).  Lane j takes the samples j, j + G, j + 2G, ...; the lanes' sums
 *             are added by a fixed butterfly, then in a fixed order across rows and wavefronts.  A sector's sums and
 *             record are the same bytes in any batch, shard or mode.  A float64 restatement reproduces the sums up to the
 *             order of the double sums.
 *   record    lk_uncertainty_from_sums (one function for the kernel and the host, csrc/lk_uncertainty.hpp), all in double:
 *             C_ab = A_ab / sqrt(A_aa A_bb); an unpivoted L D L^T of C and from it C^-1;
 *             Cov_ab = s^2 (C^-1)_ab / sqrt(A_aa A_bb); sigma[k] = sqrt(Cov_kk), times 2^L for k < 2 (level-0 pixels).
 *             The ellipse is that of the 2 x 2 block (c00, c01, c11) of u and v in level-0 pixels (Cov times 4^L), by the
 *             formulas of the strain tensor's principal values: sigma_major, sigma_minor = sqrt((c00 + c11) / 2 +-
 *             sqrt(((c00 - c11) / 2)^2 + c01^2)), theta = atan2(2 c01, c00 - c11) / 2, rho_uv = c01 / sqrt(c00 c11).
 *             LK_FM_U: sigma_major = sigma[0], rho_uv = sigma_minor = theta = sssig_y = 0.  noise = sqrt(s^2);
 *             sssig_x = A_00 / n, sssig_y = A_11 / n.  Each output is rounded to float once.
 *   status    checked in this order: BAD_RECORD  the record is not LK_ERROR_NONE or has a non-finite parameter or chi (the
 *             recovery pass's "good" rule with chi_max = 0; the sector is not evaluated);  OUT_OF_IMAGE  the sampler
 *             flagged a sample;  TOO_FEW  n <= P;  SINGULAR  some A_aa == 0, or a pivot of the L D L^T of the
 *             unit-diagonal C is <= 1e-10 (scale-free).  For every status but OK the float fields are 0, n_points = n; the
 *             sums of a BAD_RECORD or OUT_OF_IMAGE sector are reported as 0.
 *   modes     allowed in every mode, reference-order mode included.  The call reads records and images and writes nothing
 *             of the engine's: records, guesses, last parameters, counters, lk_get_reseed_info and the strain field stay
 *             byte for byte.  A rebuild of the sample lists that waits for the next solve (lk_update_sector) is carried
 *             out first, as lk_search_guesses does: the pass walks the lists.
 *   errors    LK_ERROR_BAD_DOMAIN with a message: null configuration or output; no committed sectors; records == NULL
 *             before any batch solve of the committed sectors, or with one still in flight; the images are not set; a bad
 *             def_slot.
 *   scope     one engine, the undeformed image is LK_IMG_UND.  lk_group, lk_tracker, the report CSV, the CudaClass
 *             adapter, lk_reseed_failed and lk_strain_field do not call it.  Windows with reference_previous are not
 *             covered (their undeformed image is the previous frame). */
enum { LK_UNC_OK = 0, LK_UNC_BAD_RECORD = 1, LK_UNC_OUT_OF_IMAGE = 2, LK_UNC_TOO_FEW = 3, LK_UNC_SINGULAR = 4 };
typedef struct lk_uncertainty_config {
  int def_slot;   /* -1: LK_IMG_DEF; k >= 0: ring slot k (lk_sequence_set_frame), as for lk_search_guesses */
  int reserved;
} lk_uncertainty_config;
typedef struct lk_uncertainty {          /* 64 bytes, one per sector */
  float sigma[6];                        /* standard deviation of p[k], level-0 scale; 0 for k >= P */
  float noise;                           /* s = sqrt(chi / (n - P)), grey levels */
  float rho_uv;                          /* Cov01 / (sigma0 sigma1); 0 for LK_FM_U */
  float sigma_major, sigma_minor, theta; /* principal axes of the 2x2 (u, v) covariance, level-0 pixels; angle of the major axis */
  float sssig_x, sssig_y;                /* A00 / n, and A11 / n for models with v (mean squared image gradient) */
  int32_t n_points, status, reserved;
} lk_uncertainty;
/* records: host [S], or NULL = the engine-held records of the last finished batch solve.  out: [S].  sums_out: [S][28]
 * doubles or NULL.  Synchronous.  Changes no engine state. */
int lk_parameter_uncertainty(lk_engine *e, const lk_uncertainty_config *cfg, const lk_result *records, lk_uncertainty *out,
                             double *sums_out);
/* the kernel's own function compiled for the host: the record of n samples with the 28 sums `sums28` evaluated at `level`
 * (status OK, TOO_FEW or SINGULAR).  LK_ERROR_BAD_DOMAIN for an unknown model, a level outside 0 .. LK_MAX_LEVELS - 1 or a
 * null pointer. */
int lk_uncertainty_from_sums(int model, int n, const double *sums28, int level, lk_uncertainty *out);

/* ---- material-point tracks: chosen points carried through a solved sequence ---------------- */
/* lk_track_points answers what a sequence is usually recorded for: where a chosen material point is in every frame, how much
 * it has strained since the reference configuration, and (lk_gauges_from_tracks) how far apart two such points are - the
 * virtual extensometer.  Per frame and point it is lk_strain_field's windowed least-squares plane of the good sectors, taken
 * around the point's own position instead of a sector centre, and composed from frame to frame (csrc/lk_track.hip,
 * DESIGN.md section 18).
 *   data      of a sector: position = the engine's committed centre c (lk_get_sector_info), the same in every frame of the
 *             call; displacement u = p[0] and v = p[1], v = 0 for LK_FM_U.  The record's gradient parameters are not used.
 *   good      the shared rule of the recovery pass and the strain field (one device function): LK_ERROR_NONE, finite
 *             parameters (the model's P), finite chi and, if chi_max > 0, chi <= chi_max; evaluated once per (frame, sector).
 *   records   source = LK_TRACK_RECORDS_CALLER: `records` is host [n_frames][S].  _ENGINE: records == NULL and n_frames == 1;
 *             the engine-held records of the last finished batch solve are read.  _WINDOW: records == NULL; the device records
 *             of the last window that was waited for (lk_wait_sequence) are read where lk_get_sequence_results_device shows
 *             them, without a host copy; n_frames is 0 or that window's frame count.  A solve or window that is still in
 *             flight, or that does not exist - a window solved before the last lk_commit_sectors does not - is refused.
 *   window    of a point at position x in frame f: every good sector j of frame f with dx^2 + dy^2 <= r^2, where
 *             (dx, dy) = c_j - x is formed in double from the float centre and the double position and r = (double)radius.
 *             Each product and each sum is rounded to double (no fused multiply-add).  n = the number of such sectors; there
 *             is no "sector itself".
 *   fit       lk_strain_field's `fit` paragraph, all in double, in the window's coordinates x = dx, y = dy: the sums Sx, Sy,
 *             Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv; the centred moments Cxx = Sxx - Sx Sx / n, Cxy = Sxy - Sx Sy / n,
 *             Cyy = Syy - Sy Sy / n, Cxu = Sxu - Sx Su / n, Cyu = Syu - Sy Su / n, Cxv, Cyv alike; D = Cxx Cyy - Cxy Cxy;
 *               gux = (Cyy Cxu - Cxy Cyu) / D,  guy = (Cxx Cyu - Cxy Cxu) / D,  gvx, gvy by the same formulas from Cxv, Cyv;
 *               du = Su / n - gux (Sx / n) - guy (Sy / n)  (the plane at the position),  dv alike.
 *             There is no residual pass.
 *   degenerate lk_strain_field's rule, Cxx Cyy == 0 or D <= 1e-6 Cxx Cyy, and in addition Cxx <= 2^-40 Sxx or
 *             Cyy <= 2^-40 Syy.  At a sector centre a row or column of centres has dy or dx exactly 0 and the first rule
 *             fires; seen from a position off the lattice (a point beyond the edge of the domain sees one row) the same
 *             window has Cyy = Syy - Sy Sy / n of the order of 1e-16 Syy - the rounding of the sums, whose sign and size
 *             depend on their order - and D and Cxx Cyy both scale with it.  A centred moment below 2^-40 of its raw sum is
 *             that rounding, not a spread of the centres (a real spread of one pitch in a window of r pitches and n sectors
 *             is about (1 / r)^2 / n of the raw sum).
 *   step      LK_TRACK_TOTAL (every frame's records are displacements from the reference configuration): the fit is centred
 *             at the reference position (X, Y) in every frame; x_f = X + du, y_f = Y + dv, F_f = I + g.  The frames are
 *             independent of each other.
 *             LK_TRACK_INCREMENTAL (frame f's records are displacements from frame f - 1, a reference_previous window, the
 *             sectors staying where they are): the fit is centred at x_{f-1}, with x_{-1} = X; x_f = x_{f-1} + (du, dv);
 *             F_f = (I + g) F_{f-1} with F_{-1} = I, each product and each sum rounded to double.
 *             Position and F are carried in double from frame to frame; each output is rounded to float once per frame:
 *             x, y; u = (float)(x - X), v alike; ux = (float)(Fxx - 1), uy = (float)Fxy, vx = (float)Fyx,
 *             vy = (float)(Fyy - 1); the six tensor fields are lk_strain_from_gradient of those four floats, so `tensor`
 *             is that of the TOTAL gradient in both modes.
 *   status    checked in this order: BAD_POINT  X or Y is not finite (every frame of the point);  LOST  INCREMENTAL only: an
 *             earlier frame of this point was not OK, or the state passed in is not finite;  TOO_FEW  n < min_neighbours;
 *             DEGENERATE  the `degenerate` paragraph;  OK.  For every status but OK the float fields are 0 and
 *             neighbours = n, with n = 0 for BAD_POINT and LOST (no window is formed).  In TOTAL mode a failed frame does not
 *             affect the next one.
 *   state     state_inout, if not NULL, is [n_points][8] doubles {X, Y, x, y, Fxx, Fxy, Fyx, Fyy}.  With points_xy
 *             ([n_points][2] floats, the reference positions) the call starts fresh from {X, Y, X, Y, 1, 0, 0, 1} and the
 *             state is output only; with points_xy == NULL it continues from the state; passing neither is an error.  On
 *             return it holds the state after the last frame; a frame that is not OK leaves x, y and F as NaN (X, Y stay),
 *             which is what makes the rest of an INCREMENTAL chain LOST.  Two calls on frames 0 .. k - 1 and k .. F - 1, the
 *             second continuing from the first's state, give the same bytes as one call on 0 .. F - 1: this is how a
 *             sequence longer than one window is tracked.
 *   order     fixed, as for lk_strain_field: the candidates are the members of the 3 x 3 cells around the position's cell
 *             of a grid of cell size `radius` over the centres (rows iy - 1, iy, iy + 1, each from ix - 1 to ix + 1), by
 *             ascending sector index within a cell, dealt to the lanes of a group (16 or 64, chosen from the sector count and
 *             the number of cells - not from the points) in turn and summed by a fixed butterfly.  The position's cell is
 *             floor((x - x0) / cell) as for a centre, clamped to [-2, nx + 1] and [-2, ny + 1]: one cell beyond the grid
 *             (-1, nx) the range still reaches the grid's edge cells; farther out (-2, nx + 1: more than `radius` from every
 *             centre) there are no candidates and nothing is walked.  A point's records depend on that point, the centres, the records and the configuration only - not
 *             on the other points of the call or on their count.  A float64 restatement reproduces them up to the order of
 *             the double sums.
 *   modes     allowed in every mode, reference-order mode included: the call writes nothing of the engine's - records,
 *             guesses, last parameters, counters and lk_get_reseed_info stay byte for byte - and, as for lk_strain_field, a
 *             rebuild of the sample lists that waits for the next solve keeps waiting.
 *   errors    LK_ERROR_BAD_DOMAIN with a message, `out` untouched: null configuration or output; no committed sectors;
 *             n_points < 1; n_frames < 1 where a frame count is required (CALLER, ENGINE); radius not finite or <= 0; chi_max
 *             not finite; min_neighbours < 3; unknown tensor, mode or source; neither points_xy nor state_inout; CALLER
 *             without records; ENGINE or WINDOW with records; ENGINE with n_frames != 1, before any batch solve or with one
 *             in flight; WINDOW with an n_frames that is neither 0 nor the window's, before any window or with one in flight.
 *   scope     one engine.  lk_group, lk_tracker, the report CSV and the CudaClass adapter do not call it.  No weights inside
 *             the window, no quadratic fit.  The cell grid assumes the centres of the call: a Lagrangian sequence whose
 *             sectors move between frames is tracked with one call per frame, continuing from the state. */
enum { LK_TRACK_OK = 0, LK_TRACK_TOO_FEW = 1, LK_TRACK_DEGENERATE = 2, LK_TRACK_LOST = 3, LK_TRACK_BAD_POINT = 4 };
enum { LK_TRACK_TOTAL = 0, LK_TRACK_INCREMENTAL = 1 };
enum { LK_TRACK_RECORDS_CALLER = 0, LK_TRACK_RECORDS_ENGINE = 1, LK_TRACK_RECORDS_WINDOW = 2 };
typedef struct lk_track_config {
  float radius;        /* window: good sectors whose centre lies within this many level-0 pixels of the point (<=, in double) */
  float chi_max;       /* the shared good rule; <= 0: the error code alone decides */
  int min_neighbours;  /* >= 3 */
  int tensor;          /* LK_STRAIN_GREEN_LAGRANGE / LK_STRAIN_SMALL, of the TOTAL gradient */
  int mode;            /* LK_TRACK_TOTAL: every frame's records are displacements from the reference configuration;
                          LK_TRACK_INCREMENTAL: frame f's records are displacements from frame f - 1 (reference_previous) */
  int source;          /* LK_TRACK_RECORDS_* */
} lk_track_config;
typedef struct lk_track {   /* 64 bytes, one per (frame, point), frame-major */
  float x, y;               /* the point in frame f, level-0 pixels */
  float u, v;               /* x - X, y - Y */
  float ux, uy, vx, vy;     /* total displacement gradient F - I */
  float exx, eyy, exy, e1, e2, theta;   /* lk_strain_from_gradient of the four floats above */
  int32_t neighbours, status;
} lk_track;
/* points_xy: [n_points][2] or NULL; records: host [n_frames][S] or NULL (see `records`); state_inout: [n_points][8] doubles or
 * NULL; out: [n_frames][n_points] (source WINDOW with n_frames = 0: the window's frame count).  Synchronous.  Changes no
 * engine state. */
int lk_track_points(lk_engine *e, const lk_track_config *cfg, int n_points, const float *points_xy,
                    int n_frames, const lk_result *records, double *state_inout, lk_track *out);
/* the kernel's own per-frame function compiled for the host (csrc/lk_track.hpp): n and the 11 sums of the `fit` paragraph, in
 * its order, of the window around the position the mode centres the fit at, and the state {X, Y, x, y, Fxx, Fxy, Fyx, Fyy}
 * -> the new state (in place) and the record.  LK_ERROR_BAD_DOMAIN for a null pointer, n < 0, min_neighbours < 3 or an
 * unknown mode or tensor. */
int lk_track_step(int mode, int min_neighbours, int n, const double *sums11, double *state8, int tensor, lk_track *out);
/* virtual extensometers, host only, in double: per frame f and gauge g = (i, j) = pairs_ij[2 g], pairs_ij[2 g + 1] the four
 * floats out4[(f * n_gauges + g) * 4 ..]: the length L of the segment between the float positions of points i and j; the
 * engineering strain (L - L0) / L0, with L0 the length between the reference positions (x - u, y - v); the logarithmic strain
 * ln(L / L0); the rotation of the segment against its reference direction in radians (atan2 of the cross and the dot
 * product).  All four are 0 when either end is not LK_TRACK_OK in that frame or L0 = 0.  LK_ERROR_BAD_DOMAIN for a null
 * pointer, n_frames, n_points or n_gauges < 1, or a pair index outside 0 .. n_points - 1 (out4 untouched). */
int lk_gauges_from_tracks(int n_frames, int n_points, const lk_track *tracks, int n_gauges, const int32_t *pairs_ij, float *out4);

/* ---- global motion: the motion of a frame as a whole, and the records without it ----------- */
/* A specimen that slips in its grips, a camera that sags or a re-mounted part puts a translation and a rotation of many
 * pixels under a deformation of a few hundredths, and LK_STRAIN_SMALL is not invariant under rotation (a rigid rotation by
 * 2 degrees reads exx = eyy = cos 2 - 1 = -6.1e-4).  lk_rigid_motion fits ONE motion x -> c + t + A (x - c) to the good
 * sectors of every frame - a translation, a rigid motion, a similarity or an affine map - and, where asked, returns the
 * records with that motion taken out, for the passes downstream (csrc/lk_motion.hip, csrc/lk_motion.hpp, DESIGN.md section
 * 29).
 *   data      of a sector: position x = the engine's committed centre (lk_get_sector_info), the same in every frame of the
 *             call; displacement u = p[0], v = p[1] (v = 0 for LK_FM_U); x' = x + (u, v).
 *   good      the shared rule of the recovery pass, the strain field and the tracks (one device function): LK_ERROR_NONE,
 *             finite parameters (the model's P), finite chi and, if chi_max > 0, chi <= chi_max; once per (frame, sector).
 *   records   cfg->source, with lk_track_points' rules and refusals: LK_TRACK_RECORDS_CALLER: `records` is host
 *             [n_frames][S].  _ENGINE: records == NULL and n_frames == 1; the engine-held records of the last finished batch
 *             solve.  _WINDOW: records == NULL; the device records of the last window that was waited for are read where
 *             lk_get_sequence_results_device shows them, without a host copy; n_frames is 0 or that window's frame count.
 *   fit set   of a frame, pass 0: the good sectors with fit_mask[s] != 0 (all good sectors when fit_mask is NULL) - the mask
 *             selects a datum region, a grip or a static background.  Pass k > 0 (cfg->passes > 1): the same sectors minus
 *             those whose residual r_j to pass k - 1's fit exceeds the threshold, r_j > (double)reject * rms_{k-1}, compared
 *             in double before anything is rounded to float; the trimming is not cumulative (a sector that pass 1 left out
 *             is back in pass 2 if pass 1's fit brings it under its threshold).  A frame whose pass is not LK_MOTION_OK runs
 *             no further pass.
 *   sums      the count n and the eleven sums Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv of lk_strain_field's `fit`
 *             paragraph over the fit set, in double, with x, y relative to the origin o = the centre of the bounding box of
 *             all centres, o = ((double)min + (double)max) / 2 per axis of the float centres.  Each product and each sum is
 *             rounded to double (no fused multiply-add).  sums_out, if not NULL, receives {n, the eleven sums} of every
 *             frame's last pass, [n_frames][12] doubles.
 *   fit       one function for the kernel and the host (csrc/lk_motion.hpp, lk_motion_from_sums), from the centred moments
 *             of lk_strain_field: Cxx = Sxx - Sx Sx / n, Cxy, Cyy, Cxu = Sxu - Sx Su / n, Cyu, Cxv, Cyv alike.
 *               c = o + (Sx, Sy) / n  (the centroid of the fit set),  t = (Su, Sv) / n  (its displacement)
 *               TRANSLATION  A = I
 *               RIGID        num = Cxv - Cyu,  den = Cxx + Cxu + Cyy + Cyv,  h = sqrt(num^2 + den^2),
 *                            A = [[den, -num], [num, den]] / h  (2-D Procrustes: the rotation nearest the scatter)
 *               SIMILARITY   A = [[den, -num], [num, den]] / (Cxx + Cyy)
 *               AFFINE       A = I + g,  g = the plane gradients ux, uy, vx, vy of lk_strain_field's `fit` paragraph
 *             Nothing but + - * / sqrt on the way to c, t, A, scale and rms: the host and the device give the same bytes.
 *             theta = atan2(ayx - axy, axx + ayy) alone uses atan2 and is informational; scale = sqrt(|det A|).  Each
 *             output is rounded to float once.
 *   status    checked in this order: TOO_FEW  n < min_sectors;  DEGENERATE  RIGID and SIMILARITY: Cxx + Cyy == 0 or
 *             h == 0; AFFINE: lk_strain_field's rule, Cxx Cyy == 0 or D <= 1e-6 Cxx Cyy, or det A == 0 (a map that folds
 *             the plane onto a line cannot be taken out again); TRANSLATION is never degenerate.  For a frame that is not
 *             OK every float field is 0, n_fit = n, and its records_out are the input records unchanged.
 *   residual  a second reduction over the fit set, in double and with the fit before its rounding to float:
 *             r_j = |x'_j - (c + t + A (x_j - c))|,  rms = sqrt(sum r_j^2 / n),  max_residual = max r_j.
 *   removal   records_out, if not NULL, receives [n_frames][S] records: every good record of a frame whose motion is OK,
 *             inside the fit set or not, is lk_motion_remove of it - with the 64-byte motion as stored, in double, each
 *             output rounded to float once:
 *               x'' = c + A^-1 (x' - c - t),  (u'', v'') = x'' - x,  A^-1 the closed-form inverse of the 2 x 2 matrix.
 *             This un-rotates the deformed positions; it does not subtract the displacement field t + (A - I)(x - c), which
 *             differs from it at large rotations.  The local deformation gradient becomes F'' = A^-1 F:
 *             LK_FM_UVUXUYVXVY  F = [[1 + p2, p3], [p4, 1 + p5]], p2 .. p5 rewritten;  LK_FM_UVQ  F = [[1, -q], [q, 1]],
 *             q'' = (F''yx - F''xy) / 2;  LK_FM_UV  u and v alone;  LK_FM_U  u alone, and only LK_MOTION_TRANSLATION is
 *             accepted.  chi, the counts, the error code and undCenterX/Y are copied.  Records that are not good are copied
 *             unchanged.
 *   order     fixed: the sectors of a frame are cut into chunks of a constant size by ascending index (2048; the tuning
 *             hook LK_MOTION_CHUNK=64 makes a small domain span several); within a chunk sector chunk * size + i goes to
 *             lane i mod 256 of one workgroup, every lane adds what it is dealt in ascending order, and the lanes are
 *             joined by a fixed butterfly within a wavefront and by ascending wavefront; the chunks are added by ascending
 *             chunk index.  A frame's motion, sums and output records are the same bytes alone, inside a longer call, from
 *             any source and on every run.  A float64 restatement reproduces them up to the order of the double sums.
 *   modes     allowed in every mode, reference-order mode included: the call writes nothing of the engine's - records,
 *             guesses, last parameters, counters and lk_get_reseed_info stay byte for byte - and a rebuild of the sample
 *             lists that waits for the next solve keeps waiting.
 *   errors    LK_ERROR_BAD_DOMAIN with a message, `out` untouched: lk_track_points' for the sources (null configuration
 *             or output; no committed sectors; CALLER without records or with n_frames < 1; ENGINE or WINDOW with records;
 *             ENGINE with n_frames != 1, before any batch solve or with one in flight; WINDOW with an n_frames that is
 *             neither 0 nor the window's, before any window or with one in flight; unknown source), and: unknown kind;
 *             passes outside 1 .. 4; passes > 1 with reject <= 0; min_sectors below the kind's minimum (1, 2, 2, 3);
 *             non-zero reserved words; reject or chi_max not finite; LK_FM_U with a kind other than TRANSLATION.
 *   scope     one engine; records_out is a host array.  Not covered: composing the motions of a reference_previous window
 *             into totals (each frame's motion is that of its own records), device-resident records_out, lk_group,
 *             lk_tracker, the report CSV and the CudaClass adapter. */
enum { LK_MOTION_TRANSLATION = 0, LK_MOTION_RIGID = 1, LK_MOTION_SIMILARITY = 2, LK_MOTION_AFFINE = 3 };
enum { LK_MOTION_OK = 0, LK_MOTION_TOO_FEW = 1, LK_MOTION_DEGENERATE = 2 };
typedef struct lk_motion_config {
  int   kind;          /* LK_MOTION_* */
  int   source;        /* LK_TRACK_RECORDS_CALLER / _ENGINE / _WINDOW, with lk_track_points' rules and refusals */
  float chi_max;       /* the shared good rule; <= 0: the error code alone decides */
  float reject;        /* > 0: pass k > 0 leaves out sectors whose residual to pass k-1's fit exceeds reject * rms of pass k-1; <= 0: no trimming */
  int   passes;        /* 1..4; > 1 requires reject > 0 */
  int   min_sectors;   /* >= 1 / 2 / 2 / 3 for the four kinds */
  int   reserved[2];   /* must be 0 */
} lk_motion_config;
typedef struct lk_motion {      /* 64 bytes, one per frame, of the last pass */
  float cx, cy;                 /* centroid of the fit set, level-0 pixels */
  float tx, ty;                 /* displacement of that centroid */
  float axx, axy, ayx, ayy;     /* linear part A: I, R, sR or the affine matrix */
  float theta, scale;           /* atan2(ayx - axy, axx + ayy); sqrt(|det A|) */
  float rms, max_residual;      /* of |x'_j - (c + t + A (x_j - c))| over the fit set, pixels */
  int32_t n_fit, n_rejected, status, passes_run;  /* sectors fitted; sectors the last pass trimmed; LK_MOTION_*; passes that ran */
} lk_motion;
/* records: host [n_frames][S] or NULL (see `records`); fit_mask: host [S] or NULL; out: [n_frames] (source WINDOW with
 * n_frames = 0: the window's frame count); records_out: host [n_frames][S] or NULL; sums_out: [n_frames][12] doubles or NULL.
 * Synchronous.  Changes no engine state. */
int lk_rigid_motion(lk_engine *e, const lk_motion_config *cfg, int n_frames, const lk_result *records,
                    const uint8_t *fit_mask, lk_motion *out, lk_result *records_out, double *sums_out);
/* the kernel's own fit compiled for the host (csrc/lk_motion.hpp): the count n and the eleven sums of the `sums` paragraph
 * relative to origin_xy = {ox, oy} -> the record.  rms, max_residual, n_rejected and passes_run, which the sums do not hold,
 * are 0.  LK_ERROR_BAD_DOMAIN for a null pointer, n < 0, an unknown kind or a min_sectors below the kind's minimum. */
int lk_motion_from_sums(int kind, int min_sectors, int n, const double *sums11, const double *origin_xy, lk_motion *out);
/* the displacement field of a motion at n positions, host, in double: d(x) = t + (A - I)(x - c) from the motion's float
 * fields, uv_out[2 i ..] rounded to float once; zeros for a motion that is not OK.  LK_ERROR_BAD_DOMAIN for a null pointer
 * or n < 1. */
int lk_motion_apply(const lk_motion *m, int n, const float *xy, float *uv_out);
/* the kernel's own removal of one record compiled for the host (the `removal` paragraph): `in` at the centre (cx, cy) ->
 * `out`.  The caller applies the good rule; a motion that is not OK copies the record.  LK_ERROR_BAD_DOMAIN for a null
 * pointer, an unknown model, LK_FM_U with an A that is not the identity, or an A without an inverse (out untouched). */
int lk_motion_remove(int model, const lk_motion *m, float cx, float cy, const lk_result *in, lk_result *out);

/* ---- lens distortion: fitted to records of a rigidly shifted specimen, and taken out of records ---- */
/* The records hold displacements measured in the distorted image.  A barrel distortion of 3 % at the corner turns a pure
 * 12 px translation into a field that bends by 0.1 px rms, which lk_strain_field reads as 5e-3 of strain.  lk_lens_fit finds
 * the lens from records of the unloaded specimen translated a few times (Pan et al. 2013, Yoneyama et al. 2006);
 * lk_lens_correct takes a lens out of any records (csrc/lk_lens.hpp, csrc/lk_lens.hip, csrc/lk_lens.cpp).
 *   model     Brown-Conrady in OpenCV's convention with one normalising radius rn > 0 (level-0 pixels) in place of the focal
 *             lengths.  With rho = (x_u - c) / rn and r2 = rho . rho:
 *               D(x_u) = c + rn [ rho (1 + k1 r2 + k2 r2^2) + (2 p1 rx ry + p2 (r2 + 2 rx^2),  p1 (r2 + 2 ry^2) + 2 p2 rx ry) ]
 *             carries an undistorted position to where the camera shows it.  J_D = dD/dx_u is closed-form and symmetric.
 *   inverse   U = D^-1 by Newton's iteration on rho with J_D, from rho_d, always 6 steps (the error squares: 5e-2, 3e-3, 1e-5,
 *             1e-10 at a rim distortion of 5 %).  If J_D has det <= 0 (or is not finite) at an iterate or at the result the
 *             point is OUTSIDE the model's domain: that is a status, and nothing computed from it is written.
 *   bytes     double arithmetic, only + - * /, no fused multiply-add: the host functions below and the kernels give the same
 *             bytes.
 *   good      the shared rule of lk_rigid_motion (`good` there), with cfg->chi_max.
 *   records   cfg->source = LK_TRACK_RECORDS_CALLER / _ENGINE / _WINDOW with lk_track_points' rules and refusals, exactly as
 *             lk_rigid_motion (`records` there); a window is read in place.
 *
 * lk_lens_correct
 *   For every good record, with X the committed centre and x = X + (u, v)  (v = 0 for LK_FM_U):
 *     X_u = U(X),  x_u = U(x),  (u', v') = x_u - X_u;  the record's own gradient becomes F' = J_D(x_u)^-1 F J_D(X_u),
 *   written back in the model's layout as lk_motion_remove does: LK_FM_UVUXUYVXVY p2 .. p5;  LK_FM_UVQ F = [[1, -q], [q, 1]],
 *   q' = (F'yx - F'xy) / 2;  LK_FM_UV and LK_FM_U the displacement alone (LK_FM_U: u' alone is written).  Each output is
 *   rounded to float once; chi, the counts, the error code and undCenterX/Y are copied.
 *   status_out [n_frames][S]: 0 corrected;  1 not good, copied;  2 X or x outside the model's domain, copied.
 *   centres_out [S][2] receives U(X) as floats (X itself where X is outside).  The committed centres stay where they are, so
 *   the passes downstream see corrected displacements at uncorrected positions: a gradient they form over those positions
 *   is off by the local stretch of the lens, an error of distortion x strain (3 % of a strain, at the corner, for the lens
 *   above) - second order, and removable by handing them centres_out where they take positions.
 *   One thread per (frame, sector); the call changes no engine state and is allowed in every mode.
 *
 * lk_lens_fit
 *   nuisance  what a frame's true motion may be, N(X_u), with o the centre of the centres' bounding box as in lk_rigid_motion:
 *               LK_LENS_TRANSLATION  Q = 2  N = t
 *               LK_LENS_SIMILARITY   Q = 4  N = t + a (X_u - o) + b (X_u - o)^perp,  (x, y)^perp = (-y, x)
 *               LK_LENS_AFFINE       Q = 6  N = t + G (X_u - o),  G = [[gxx, gxy], [gyx, gyy]]
 *             A frame's nuisance parameters {tx, ty | a, b | gxx, gxy, gyx, gyy} are state of the fit and start at 0.
 *   fit set   the good records with fit_mask[s] != 0 (all good records when fit_mask is NULL); a frame with fewer than
 *             cfg->min_sectors of them is skipped (LK_LENS_FRAME_TOO_FEW).  A member with X or x outside the domain is
 *             counted in n_outside and adds nothing.
 *   rows      per member r = U(X + u) - U(X) - N(U(X)) and, per component, one row W = 7 + Q wide,
 *               a = [dr/dk1, dr/dk2, dr/dp1, dr/dp2, dr/dcx, dr/dcy | dr/dn (Q) | r],
 *             analytic: dU/dtheta = -J_D^-1 dD/dtheta at the undistorted point, dD/dc = I - J_D,
 *             dr/dtheta = dx_u/dtheta - (I + grad N) dX_u/dtheta.  All six lens columns are always formed.
 *   sums      per frame 2 + W (W + 1) / 2 doubles: {n, the upper triangle, row-major, of sum (a_x a_x^T + a_y a_y^T),
 *             n_outside} - 47, 68 or 93 doubles.  Order: lk_rigid_motion's (chunks of 2048 sectors by ascending index, the
 *             test hook LK_LENS_CHUNK=64; one workgroup per (chunk, frame); each lane adds ascending; a fixed butterfly within a
 *             wavefront, wavefronts ascending, chunks ascending).  A frame's sums are the same bytes alone, inside a longer
 *             call, from any source and on every run.  sums_out, if not NULL, receives [2][n_frames][that many]: the sums of
 *             the first evaluation (at init, nuisance 0) and of the last (at the result).
 *   step      lk_lens_step_from_sums, host, double: every used frame's nuisance block is eliminated by Schur complement
 *             (a Cholesky of its Jacobi-scaled Q x Q block), the lens block of the free parameters is Jacobi-scaled and
 *             factored by Cholesky; a pivot <= 1e-10 on either unit diagonal, a diagonal <= 0 or no usable frame gives
 *             LK_LENS_DEGENERATE (no translation at all; one parameter too many).  While k1 = k2 = p1 = p2 = 0 exactly the
 *             centre's columns are zero, so lk_lens_fit holds the centre in such an iteration.
 *   loop      per iteration one evaluation on the device (the chunk sums and their join), one small download, one step;
 *             stop when max_j |delta_j| / s_j <= tol, s = 1 for the coefficients and rn for the centre, else after
 *             max_iters: LK_LENS_MAX_ITERS.  A last evaluation at the result gives rms = sqrt(sum |r|^2 / n_records), sigma
 *             = sqrt of the diagonal of s^2 S^-1 with S the reduced lens block and s^2 = sum |r|^2 / (2 n_records - free
 *             parameters - Q frames used) (0 for held parameters), n_records, n_frames_used, n_outside.  rms_before is that
 *             of init with every frame's nuisance at its own best value.  A degenerate step ends the loop with the lens as
 *             it stood.
 *   errors    LK_ERROR_BAD_DOMAIN with a message, outputs untouched: the sources' refusals; a null configuration, lens or
 *             output; rn not finite or <= 0 or any other field of the lens not finite; a non-zero `reserved` of the lens or
 *             the configuration; and for the fit: empty or unknown bits in `free`; unknown nuisance; the centre free with
 *             LK_LENS_AFFINE (to first order a shift of the centre is an affine field, which the nuisance absorbs);
 *             LK_FM_U; max_iters outside 1 .. 32; tol negative or not finite; min_sectors < Q; chi_max not finite.
 *   scope     not covered: resampling frames into undistorted coordinates; trimming passes; k3 and thin-prism terms;
 *             lk_group, lk_tracker, the report CSV and the CudaClass adapter. */
typedef struct lk_lens { double cx, cy, rn, k1, k2, p1, p2, reserved; } lk_lens;   /* 64 bytes; reserved must be 0 */
enum { LK_LENS_TRANSLATION = 0, LK_LENS_SIMILARITY = 1, LK_LENS_AFFINE = 2 };
enum { LK_LENS_FREE_K1 = 1, LK_LENS_FREE_K2 = 2, LK_LENS_FREE_P1 = 4, LK_LENS_FREE_P2 = 8, LK_LENS_FREE_CENTRE = 16 };
enum { LK_LENS_OK = 0, LK_LENS_MAX_ITERS = 1, LK_LENS_DEGENERATE = 2 };
enum { LK_LENS_FRAME_OK = 0, LK_LENS_FRAME_TOO_FEW = 1 };
typedef struct lk_lens_config {       /* lk_lens_correct */
  int   source;        /* LK_TRACK_RECORDS_* */
  float chi_max;       /* the shared good rule; <= 0: the error code alone decides */
  int   reserved[2];   /* must be 0 */
} lk_lens_config;
typedef struct lk_lens_fit_config {
  int      source;       /* LK_TRACK_RECORDS_* */
  float    chi_max;
  int      min_sectors;  /* per frame, >= Q */
  unsigned free;         /* LK_LENS_FREE_* bits; held parameters keep init's values */
  int      nuisance;     /* LK_LENS_TRANSLATION / _SIMILARITY / _AFFINE */
  int      max_iters;    /* 1 .. 32 */
  double   tol;          /* >= 0 */
  int      reserved[2];  /* must be 0 */
} lk_lens_fit_config;                 /* 40 bytes */
typedef struct lk_lens_result {       /* 160 bytes: what lk_lens_fit returns */
  lk_lens lens;
  double  sigma[6];                   /* of k1, k2, p1, p2, cx, cy; 0 for held parameters */
  double  rms_before, rms, last_step; /* pixels, pixels, max_j |delta_j| / s_j of the last step taken */
  int32_t status, iterations, n_records, n_frames_used, n_outside, reserved;
} lk_lens_result;
typedef struct lk_lens_frame {        /* 64 bytes */
  double  nuisance[6];                /* {tx, ty, ...}; those beyond Q are 0 */
  double  rms;
  int32_t n, status;                  /* members of the fit set; LK_LENS_FRAME_* */
} lk_lens_frame;
typedef struct lk_lens_step {         /* 136 bytes */
  double  delta[6];                   /* the step of k1, k2, p1, p2, cx, cy; 0 for held parameters */
  double  sigma[6];
  double  chi2, chi2_profiled, scaled_step; /* sum |r|^2 of the used frames; the same with every frame's nuisance at its best */
  int32_t status, n_records, n_frames_used, n_outside;
} lk_lens_step;
/* n positions xy [n][2] in doubles -> xy_out [n][2].  LK_ERROR_BAD_DOMAIN for a null pointer, n < 1 or a lens that the
 * `errors` paragraph refuses.  lk_lens_undistort: status_out [n] (or NULL) 0, or 2 for a position outside the model's domain,
 * which is copied. */
int lk_lens_distort(const lk_lens *lens, int n, const double *xy, double *xy_out);
int lk_lens_undistort(const lk_lens *lens, int n, const double *xy, double *xy_out, uint8_t *status_out);
/* the kernel's own correction of one record compiled for the host: `in` at the centre (cx, cy) -> `out`, *status (or NULL) 0 or
 * 2.  The caller applies the good rule.  LK_ERROR_BAD_DOMAIN for a null pointer, an unknown model or a refused lens. */
int lk_lens_correct_record(int model, const lk_lens *lens, float cx, float cy, const lk_result *in, lk_result *out, int *status);
/* one Gauss-Newton step from the sums [n_frames][2 + W (W + 1) / 2] of the `sums` paragraph.  nuisance_delta: [n_frames][6]
 * or NULL, the step of every frame's nuisance (0 for a skipped frame).  With a status other than LK_LENS_OK delta, sigma and
 * nuisance_delta are 0; chi2, n_records, n_frames_used and n_outside are filled regardless.  LK_ERROR_BAD_DOMAIN for a null
 * pointer, an unknown nuisance, an empty or unknown `free`, rn not finite or <= 0, n_frames < 1 or min_sectors < Q. */
int lk_lens_step_from_sums(int nuisance, unsigned free, double rn, int min_sectors, int n_frames, const double *sums,
                           lk_lens_step *out, double *nuisance_delta);
/* records: host [n_frames][S] or NULL (see `records`); records_out: host [n_frames][S]; centres_out: [S][2] floats or NULL;
 * status_out: [n_frames][S] or NULL.  Synchronous.  Changes no engine state. */
int lk_lens_correct(lk_engine *e, const lk_lens_config *cfg, const lk_lens *lens, int n_frames, const lk_result *records,
                    lk_result *records_out, float *centres_out, uint8_t *status_out);
/* init: the start, and the values of the held parameters; fit_mask: host [S] or NULL; out: one record; frames_out: [n_frames]
 * or NULL; sums_out: see `sums`, or NULL.  Synchronous.  Changes no engine state. */
int lk_lens_fit(lk_engine *e, const lk_lens_fit_config *cfg, const lk_lens *init, int n_frames, const lk_result *records,
                const uint8_t *fit_mask, lk_lens_result *out, lk_lens_frame *frames_out, double *sums_out);

/* ---- a two-camera rig: 3-D points from matched records, and strain measured in the specimen's own surface ---- */
/* Every pass above reads a record as a displacement in the image plane of one camera: a 1 % out-of-plane motion at 400 mm
 * stand-off reads as 2.5e-3 of dilatation in lk_strain_field, and a tube or a dome has no image plane at all.  With a second,
 * calibrated camera lk_stereo_points turns matched records into 3-D points and lk_stereo_strain turns a field of 3-D points
 * into the strain of the surface (csrc/lk_stereo.hpp, csrc/lk_stereo.hip, csrc/lk_stereo.cpp).  The
 * matching is the existing solve: a cross-camera pair is an image pair (camera 0's reference frame as the undeformed image,
 * a frame of camera 1 as the deformed one).  The calibration of the rig is input.
 *   data      one engine serves camera 0; its sectors are committed on camera 0's reference frame.  With c the committed
 *             centre widened to double, u = p[0], v = p[1] (v = 0 for LK_FM_U), all records solved against camera 0's
 *             reference frame:
 *               ref1 [S]      camera 0 reference -> camera 1 reference: the reference state's pixels are c and c + (u, v)
 *               rec0 [F][S]   camera 0 reference -> camera 0's frame f:  pixel 0 of frame f is c + (u, v)
 *               rec1 [F][S]   camera 0 reference -> camera 1's frame f:  pixel 1 of frame f is c + (u, v)
 *   camera    lk_camera: x_cam = R X + t; the undistorted pixel (fx x/z + skew y/z + cx, fy y/z + cy); then lk_lens_distort
 *             of `lens` (lk_lens_fit's model, in pixels - a fitted lens plugs in unchanged).  Back: lk_lens_undistort, then
 *             K^-1.  A lens with k1 = k2 = p1 = p2 = 0 is the identity, exactly, and its other fields are not read.
 *   triangulation  lk_stereo_triangulate of one pair of pixels, in double, + - * / sqrt only, no fused multiply-add: the
 *             host function and the kernel give the same bytes.
 *               1. both pixels undistorted (6 Newton steps each, lk_lens_undistort's);
 *               2. the rays o_k = -R_k^T t_k, d_k = R_k^T K_k^-1 (m_k, 1) in the world frame;
 *               3. the start: the midpoint of the common perpendicular, from a = d0.d0, b = d0.d1, c = d1.d1, d = d0.(o0 - o1),
 *                  e = d1.(o0 - o1), det = a c - b^2, s = (b e - c d) / det, t = (a e - b d) / det;
 *               4. always 7 Gauss-Newton steps on the four reprojection residuals (observed - projected, undistorted
 *                  pixels) over X: J^T J (3 x 3) factored as L D L^T in one written order.
 *             residual[4] = the residuals at the result {x0, y0, x1, y1};  epipolar = the signed distance, in undistorted
 *             pixels of camera 1, of pixel 1 from the line F (m0, 1), F = K1^-T [t_r]x R_r K0^-1 formed once on the host
 *             (lk_stereo_fundamental; R_r = R1 R0^T, t_r = t1 - R_r t0);  angle = atan2(|d0 x d1|, d0 . d1) in radians.
 *   status    of a point, checked in this order: LK_STEREO_BAD_RECORD  a record it reads is not good (the shared rule with
 *             cfg->chi_max; every frame's point reads ref1 too) or a pixel is not finite;  LK_STEREO_OUTSIDE_LENS  a pixel
 *             outside a lens's domain;  LK_STEREO_PARALLEL  det <= 1e-12 a c (the rays within 1e-6 rad; scale-free), or a
 *             result that is not finite;  LK_STEREO_BEHIND  s <= 0 or t <= 0, or an iterate with z <= 0 in a camera;  else
 *             LK_STEREO_OK.  A point that is not OK has every numeric field 0, never NaN.
 *   lk_stereo_points  one launch, one thread per (frame, sector), the reference state as frame -1: ref_out [S] from ref1,
 *             out [F][S] from rec0 and rec1.  n_frames = 0 with rec0 = rec1 = out = NULL gives the shape alone.  The points stay
 *             on the device for a following lk_stereo_strain.  A frame's bytes are the same alone and inside a longer call.
 *
 * lk_stereo_strain: per (frame, sector) the strain of the surface through the 3-D points, measured in the surface
 *   window    lk_strain_field's (`window`, `order` there): the members of the 3 x 3 cells around c_s within cfg->radius of it,
 *             (dx, dy) = c_j - c_s in double.  A member is good when its reference point and its point of the frame are both
 *             LK_STEREO_OK.  n = their count.
 *   fit       least-squares planes over (dx, dy) of six functions: X, Y, Z of the reference point and U = P_f - P_ref (three
 *             components, formed in double per member).  23 double sums: n, Sx, Sy, Sxx, Sxy, Syy and Sf, Sxf, Syf of each;
 *             the moments, D and the solve are lk_strain_field's (`fit` there).
 *   tensor    a1 = dP/dx, a2 = dP/dy (reference tangents);  b_i = a_i + dU/d(x, y);  G = [a_i . a_j],  g = [b_i . b_j];
 *             Ra = the upper-triangular factor of G: r11 = sqrt(G11), r12 = G12 / r11, r22 = sqrt(G22 - r12^2);
 *             C = Ra^-T g Ra^-1;  E = (C - I) / 2 = {exx, exy; exy, eyy}, the Green-Lagrange strain in the orthonormal
 *             tangent basis e1 = a1 / |a1|, e2 perpendicular to e1 in the tangent plane, n = e1 x e2.  E is exact for any
 *             homogeneous 3-D affine map of a plane, whatever its pose and whatever the image parametrisation (DESIGN.md
 *             section 32).  e1, e2, theta: lk_strain_from_gradient's formulas;  biot_k = sqrt(1 + 2 e_k) - 1;  normal = the
 *             fitted displacement at c_s along n.
 *   residual  a second walk sums the squared 3-D misfit of the three displacement planes;  residual = sqrt(sum / n).
 *   status    checked in this order: TOO_FEW  n < cfg->min_neighbours;  DEGENERATE  lk_strain_field's rule, or
 *             G11 G22 - G12^2 <= 1e-12 G11 G22 (the surface seen edge-on);  FILLED  a valid fit at a sector whose own points
 *             are not both OK;  OK.  TOO_FEW and DEGENERATE: every float field is 0, neighbours = n.
 *   sources   ref_points [S] and points [n_frames][S] from the caller, or both NULL: the arrays the last lk_stereo_points
 *             left on the device, with that call's n_frames.  Both sources give the same bytes.
 *   bytes     lane groups of 16 or 64 per (frame, sector), each with its own fixed order (the host picks as lk_strain_field
 *             does; test hook LK_STEREO_GROUP=16 / 64).  Within a group size a record's bytes are the same on every run,
 *             alone or in a longer call and from either source.  Across the two group sizes neighbours and status are the
 *             same (unless a window sits at a threshold) and the float fields agree within the rounding of double sums
 *             taken in another order.  Lane 0 rounds each output to float once.
 *   modes     both calls are synchronous, allowed in every mode, and change no engine state (lk_strain_field's `modes`).
 *   errors    LK_ERROR_BAD_DOMAIN with a message, outputs untouched: no committed sectors; a null configuration, rig, ref1,
 *             ref_out or output; n_frames < 0 (lk_stereo_points) or < 1 (lk_stereo_strain) or above 65534; frame arguments
 *             that are null with n_frames > 0 or not null with n_frames = 0; chi_max not finite; radius not finite or <= 0;
 *             min_neighbours < 3; non-zero reserved words; a camera that lk_stereo_project refuses; one point array null and
 *             the other not; device-held points with no lk_stereo_points before, with another n_frames or another sector
 *             count.
 *   scope     not covered: calibration of the rig; dense 3-D maps (the epipolar-constrained search is lk_search_epipolar); lk_group, lk_tracker, the
 *             report CSV and the CudaClass adapter. */
typedef struct lk_camera {            /* 256 bytes */
  double  fx, fy, cx, cy, skew;       /* pixels; fx, fy > 0 */
  double  R[9], t[3];                 /* row-major rotation and translation: x_cam = R X + t */
  lk_lens lens;                       /* pixel domain; all four coefficients 0: no lens */
  double  reserved[7];                /* must be 0 */
} lk_camera;
enum { LK_STEREO_OK = 0, LK_STEREO_BAD_RECORD = 1, LK_STEREO_OUTSIDE_LENS = 2, LK_STEREO_PARALLEL = 3, LK_STEREO_BEHIND = 4 };
enum { LK_STEREO_SURFACE_OK = 0, LK_STEREO_SURFACE_FILLED = 1, LK_STEREO_SURFACE_TOO_FEW = 2, LK_STEREO_SURFACE_DEGENERATE = 3 };
typedef struct lk_stereo_point {      /* 64 bytes */
  double  X, Y, Z;                    /* world units */
  float   residual[4];                /* {x0, y0, x1, y1}: observed - projected, undistorted pixels */
  float   epipolar, angle;            /* undistorted pixels of camera 1; radians */
  int32_t status, reserved[3];        /* LK_STEREO_* */
} lk_stereo_point;
typedef struct lk_stereo_config {     /* 16 bytes; lk_stereo_points reads chi_max, lk_stereo_strain radius and min_neighbours */
  float radius;          /* strain window in level-0 pixels of camera 0's reference frame (<=, tested in double) */
  float chi_max;         /* the shared good rule; <= 0: the error code alone decides */
  int   min_neighbours;  /* >= 3, counting the sector itself when it is good */
  int   reserved;        /* must be 0 */
} lk_stereo_config;
typedef struct lk_stereo_surface {    /* 128 bytes, one per (frame, sector) */
  float   X, Y, Z;                    /* the fitted reference point at c_s */
  float   U, V, W;                    /* the fitted displacement at c_s */
  float   nx, ny, nz;                 /* the unit normal of the reference surface, e1 x e2 */
  float   exx, eyy, exy, e1, e2, theta; /* Green-Lagrange in (e1, e2); principal strains e1 >= e2, angle of the first from the basis vector e1 */
  float   biot1, biot2;               /* sqrt(1 + 2 e_k) - 1 */
  float   normal;                     /* (U, V, W) . n */
  float   residual;                   /* world units */
  int32_t neighbours, status;         /* LK_STEREO_SURFACE_* */
  int32_t reserved[11];
} lk_stereo_surface;
/* Host functions: the kernels' own code compiled for the host; no GPU needed.  LK_ERROR_BAD_DOMAIN for a null pointer, n < 1
 * or a refused camera: non-zero reserved words, intrinsics, R or t that are not finite, fx or fy <= 0, an R with an entry of
 * R^T R more than 1e-9 off the identity, or - unless all four coefficients are 0 - a lens that lk_lens_distort refuses.
 * lk_stereo_project: world points xyz [n][3] -> pixels xy_out [n][2] as the camera shows them; status_out [n] (or NULL) 0, or 1
 * for a point that is not in front of the camera (its pixel is 0, 0). */
int lk_stereo_project(const lk_camera *cam, int n, const double *xyz, double *xy_out, uint8_t *status_out);
/* F [9], row-major, of cams [2] (see `triangulation`) */
int lk_stereo_fundamental(const lk_camera *cams, double *F_out);
/* n pairs of pixels x0 [n][2] in camera 0 and x1 [n][2] in camera 1 -> out [n] */
int lk_stereo_triangulate(const lk_camera *cams, int n, const double *x0, const double *x1, lk_stereo_point *out);
/* one window: the count n >= 0, sums23 = {Sx, Sy, Sxx, Sxy, Syy, then Sf, Sxf, Syf of X, Y, Z, U, V, W}, whether the sector's
 * own points are OK, and the second walk's sum of squared misfits -> the record; planes_out [18] (or NULL) receives
 * {f0, fx, fy} of the six planes in double.  LK_ERROR_BAD_DOMAIN for a null pointer, n < 0 or min_neighbours < 3. */
int lk_stereo_surface_from_sums(int n, const double *sums23, int min_neighbours, int self_good, double residual_sum,
                                lk_stereo_surface *out, double *planes_out);
/* cams: [2]; ref1: host [S]; rec0, rec1: host [n_frames][S]; ref_out: [S]; out: [n_frames][S].  Synchronous. */
int lk_stereo_points(lk_engine *e, const lk_stereo_config *cfg, const lk_camera *cams, const lk_result *ref1, int n_frames,
                     const lk_result *rec0, const lk_result *rec1, lk_stereo_point *ref_out, lk_stereo_point *out);
/* ref_points: host [S] and points: host [n_frames][S], or both NULL; out: [n_frames][S].  Synchronous. */
int lk_stereo_strain(lk_engine *e, const lk_stereo_config *cfg, int n_frames, const lk_stereo_point *ref_points,
                     const lk_stereo_point *points, lk_stereo_surface *out);

/* ---- photometry and the back-warped residual map: the grey values once more ---------------- */
/* chi is a plain sum of squared grey-level differences: a frame that is 20 % darker gives every sector a large chi although
 * the match is perfect.  lk_photometry evaluates every good sector once at its record's parameters and reports the
 * zero-mean normalised cross-correlation (ZNCC) of the two patches, the gain and offset between them and the residual that
 * is left with and without them.  lk_residual_map pulls the deformed frame back into the reference configuration with the
 * solved field, pixel by pixel, and subtracts the undeformed image (csrc/lk_residual.hip).
 *   level     both passes work at L = py_start with the record's parameters brought to that level and the committed centre
 *             times 2^-L, exactly as lk_parameter_uncertainty (`level` there).
 *   good      the shared rule (csrc/lk_good.hpp): LK_ERROR_NONE, finite parameters (the model's P), finite chi and, if
 *             chi_max > 0, chi <= chi_max.
 *
 * lk_photometry
 *   sample    lk_parameter_uncertainty's walk and lane groups (16 / 64 / 512 lanes from the level-0 sample count; lane j
 *             takes the samples j, j + G, ...).  Per sample, in float: f = the undeformed node, g = the deformed image at
 *             W(x; p) by the engine's interpolation (the solve's device functions), V = f - g.
 *   sums      eight doubles per sector: sum f, sum g, sum f^2, sum g^2, sum f g, sum V^2 - each product formed in double
 *             from the floats (exact or rounded once, no fused multiply-add) - then the number of samples the sampler
 *             flagged, and max |V| (a float maximum carried in a double; order-independent).  The sums are added by the
 *             uncertainty pass's fixed butterfly, so a sector's eight numbers and its record are the same bytes in any
 *             batch, shard or mode.  A float64 restatement reproduces the six sums up to the order of the double additions.
 *   record    lk_photometry_from_sums (one function for the kernel and the host, csrc/lk_residual.hpp), in double without
 *             fused multiply-add, each output rounded to float once; with N = (double)n:
 *               mean_f = Sf / N, mean_g = Sg / N;  vf = N Sff - Sf Sf, vg = N Sgg - Sg Sg, c = N Sfg - Sf Sg;
 *               std_f = sqrt(vf) / N, std_g = sqrt(vg) / N (population);  zncc = c / sqrt(vf vg);
 *               gain = c / vf, offset = mean_g - gain mean_f (least squares g ~ gain f + offset);
 *               rms = sqrt(SVV / N);  rms_zn = std_g sqrt(max(0, 1 - zncc^2)), what is left of g after gain and offset
 *               are removed;  znssd = 2 (1 - zncc);  max_abs = max |V|.
 *   status    checked in this order: BAD_RECORD  the record is not good (not evaluated; sums and floats 0);  OUT_OF_IMAGE
 *             the sampler flagged a sample (sums and floats 0);  TOO_FEW  n < 2 (floats 0);  FLAT  vx <= 1e-12 N Sxx for
 *             x = f or x = g, i.e. N sum x^2 - (sum x)^2 <= 1e-12 N sum x^2 - a scale-free rule like the uncertainty
 *             pass's pivot rule: a patch whose variance is below 1e-12 of its mean square has no contrast to normalise
 *             by.  mean_f, mean_g, std_f, std_g (a negative vx counts as 0), rms and max_abs are still filled; zncc, gain,
 *             offset, rms_zn and znssd are 0.  OK otherwise.  n_points = n in every case; reserved words are 0.
 *
 * lk_residual_map
 *   window    x0, y0, w, h in pixels of the level-L undeformed image; all four 0: the whole level-L image.  The three
 *             outputs are [h][w] row-major; each may be NULL, not all three.
 *   owner     pixel (x, y) of the level-L undeformed image has the level-0 position (X, Y) = (x 2^L, y 2^L).  Its owner is
 *             the good sector with the smallest d2 = (X - cx)^2 + (Y - cy)^2 among those with d2 <= radius^2: the
 *             differences are doubles formed from the float centre and the double position, each square rounded, one
 *             rounded sum, no fused multiply-add; radius^2 is the double square of the float radius.  Equal d2 goes to the
 *             lowest sector index.  A sector that is not good never owns a pixel.  No candidate: owner = -1.
 *             lk_map_owner is the same rule on the host, by brute force.
 *   values    with owner s: (xd, yd) = W((float)x, (float)y; p_s) about s's level-L centre, then the engine's
 *             interpolation of the deformed image there - the solve's device functions, in float.  If the sampler flags
 *             the position: owner = -2 - s, warped = residual = NaN.  Otherwise warped = that value, residual = f - warped
 *             with f the level-L undeformed pixel, owner = s.  Pixels without an owner have NaN in both float maps.
 *   order     nothing is summed: a pixel's three values depend on that pixel, the centres, the records and the
 *             configuration only.  The sectors are found on the recovery pass's cell grid with cell size = radius; a tile
 *             of pixels searches the members of the cells it can reach from LDS, or - when they do not fit - every pixel
 *             walks its own 3 x 3 cells in global memory.  Both give the same owner: the pair (d2, index) is compared.
 *
 *   modes     both calls are allowed in every mode, reference-order mode included, write nothing of the engine's - records,
 *             guesses, last parameters, counters, the strain field and the uncertainty records stay byte for byte - carry
 *             out a rebuild of the sample lists that waits for the next solve first, as lk_parameter_uncertainty does, and
 *             synchronise the engine's stream before they return.
 *   errors    LK_ERROR_BAD_DOMAIN with a message, outputs untouched: null configuration; no output; non-zero reserved
 *             words; chi_max not finite; radius not finite or <= 0; a window that is not inside the level-L image; and
 *             what lk_parameter_uncertainty refuses (its accessor is used, its messages carry its name): no committed
 *             sectors; records == NULL before any batch solve of the committed sectors, or with one in flight; images not
 *             set; a bad def_slot.
 *   scope     one engine, the undeformed image is LK_IMG_UND.  lk_group, lk_tracker, the report CSV and the CudaClass
 *             adapter do not call them; windows with reference_previous are not covered; the maps are host arrays; zncc
 *             does not enter the good rule; the solve's criterion stays the plain sum of squares; no colour frames. */
enum { LK_PHOTO_OK = 0, LK_PHOTO_BAD_RECORD = 1, LK_PHOTO_OUT_OF_IMAGE = 2, LK_PHOTO_TOO_FEW = 3, LK_PHOTO_FLAT = 4 };
typedef struct lk_photometry_config {
  int def_slot;      /* -1: LK_IMG_DEF; k >= 0: ring slot k, as for lk_parameter_uncertainty */
  float chi_max;     /* the shared good rule; <= 0: the error code alone decides */
  int reserved[2];   /* must be 0 */
} lk_photometry_config;
/* (the record shares its name with the function: it is a struct tag without a typedef, written `struct lk_photometry`) */
struct lk_photometry {                    /* 64 bytes, one per sector */
  int32_t n_points, status;
  float mean_f, mean_g, std_f, std_g;     /* undeformed (f) and back-warped deformed (g) patch, grey levels */
  float zncc;
  float gain, offset;                     /* g ~ gain f + offset */
  float rms, rms_zn;                      /* sqrt(sum V^2 / n); the same after gain and offset are removed */
  float znssd;                            /* 2 (1 - zncc) */
  float max_abs;                          /* max |V| */
  int32_t reserved[3];
};
/* records: host [S], or NULL = the engine-held records of the last finished batch solve.  out: [S].  sums_out: [S][8]
 * doubles or NULL.  Synchronous.  Changes no engine state. */
int lk_photometry(lk_engine *e, const lk_photometry_config *cfg, const lk_result *records, struct lk_photometry *out,
                  double *sums_out);
/* the kernel's own function compiled for the host: the record of one sector of n samples with the eight sums `sums8`
 * (status OK, TOO_FEW or FLAT; OUT_OF_IMAGE if the flagged count sums8[6] is not 0).  LK_ERROR_BAD_DOMAIN for a null
 * pointer or n < 0. */
int lk_photometry_from_sums(int n, const double *sums8, struct lk_photometry *out);
typedef struct lk_residual_map_config {
  int def_slot;      /* as lk_photometry_config */
  float chi_max;
  float radius;      /* level-0 pixels, finite and > 0 */
  int x0, y0, w, h;  /* window in level-L pixels of the undeformed image; all 0: the whole level-L image */
  int reserved;      /* must be 0 */
} lk_residual_map_config;
/* records: host [S] or NULL (as lk_photometry).  warped, residual, owner: host [h][w], each may be NULL (not all three).
 * Synchronous.  Changes no engine state. */
int lk_residual_map(lk_engine *e, const lk_residual_map_config *cfg, const lk_result *records, float *warped, float *residual,
                    int32_t *owner);
/* the owner rule on the host, by brute force over n centres {cx, cy} (good: [n] bytes, 0 = not good, or NULL = all good):
 * the owner of the level-0 position (X, Y), or -1.  INT32_MIN for a null centres pointer with n > 0, n < 0 or a radius
 * that is not finite and positive. */
int lk_map_owner(int n, const float *centers_xy, const uint8_t *good, double X, double Y, double radius);

/* ---- ZNSSD refinement: a sub-pixel solve that does not mind the lighting ------------------- */
/* lk_photometry shows that a high chi comes from lighting; lk_refine_znssd repairs the match.  It takes records or guesses
 * as seeds and refines every sector by Levenberg-Marquardt on the zero-mean normalised sum of squared differences, with
 * gain and offset eliminated in closed form, in a kernel of its own (csrc/lk_znssd.hip).  Refined
 * records come out; the user hands them to lk_strain_field, lk_field_map, lk_flag_outliers and the rest through their
 * `records` argument.  With guesses from lk_search_guesses - which scores by ZNCC - the pair is a lighting-robust pipeline
 * in which no batch solve runs.
 *   level     L = py_start, as the other evaluation passes: the seed goes to level L by the solve's parameter translation
 *             and the result comes back the same way; the committed centre times 2^-L.
 *   seeds     guesses == NULL: `records` [S] on the host or, records == NULL, the engine-held records of the last finished
 *             batch solve.  A record that fails the shared good rule (chi_max as for lk_photometry) is LK_ZN_BAD_SEED: its 48
 *             bytes are copied to records_out and nothing is evaluated.  guesses != NULL (records must be NULL): host
 *             [S][6] in level-0 scale, the shape lk_search_guesses and lk_get_guesses return; every sector whose first P
 *             guesses are finite is refined, any other is LK_ZN_BAD_SEED with errorCode LK_ERROR_BAD_DOMAIN and the guess
 *             as its parameters.
 *   sample    lk_parameter_uncertainty's walk and lane groups (16 / 64 / 512 lanes from the level-0 sample count; lane j
 *             takes the samples j, j + G, ...).  Per sample, in float, the solve's device functions: f = the undeformed
 *             node, g, g_x, g_y = the deformed image and its gradient at W(x; p), H = dg/dp.
 *   sums      45 doubles for six parameters (kLkZnSums; a smaller model's come first, zeros behind): Sf, Sg, Sff, Sgg, Sfg,
 *             SH[P], SHH[P (P + 1) / 2] upper triangle row-major, SHf[P], SHg[P], then the samples the sampler flagged.
 *             Every product is formed in double from the floats without fused multiply-add; the sums are added by the
 *             uncertainty pass's fixed butterfly.  A sector's sums, and therefore its whole trajectory, record and info,
 *             are the same bytes in any batch, shard, mode or ring slot.
 *   step      lk_znssd_step_from_sums (one function for the kernel and the host, csrc/lk_znssd.hpp), in double without
 *             fused multiply-add; with N = (double)n:
 *               vf = N Sff - Sf Sf, vg = N Sgg - Sg Sg, c = N Sfg - Sf Sg;
 *               LK_ZN_TOO_FEW if n < P + 2;  LK_ZN_FLAT by photometry's rule, vx <= 1e-12 N Sxx for x = f or g;
 *               gain = c / vg, offset = (Sf - gain Sg) / N (least squares f ~ gain g + offset), zncc = c / sqrt(vf vg),
 *               crit = max(0, 1 - c c / (vf vg)) = the smallest sum (f - gain g - offset)^2 over sum (f - mean f)^2;
 *               LK_ZN_NEGATIVE if c <= 0 (the four numbers above are filled);
 *               A_kl = gain^2 (SHH_kl - SH_k SH_l / N) / N,  b_k = gain ((SHf_k - SH_k Sf / N) - gain (SHg_k - SH_k Sg / N)) / N,
 *               diag(A) times (1 + lambda), A delta = b: the Gauss-Newton step of the criterion.  A is scaled to a diagonal
 *               of 1 + lambda and factored as L D L^T without pivoting, the uncertainty pass's factorisation and
 *               scale-free pivot rule: A_kk <= 0 or a pivot <= 1e-10 is LK_ZN_SINGULAR.
 *   loop      in the kernel, one launch per lane group.  Evaluate at the seed: a flagged sample is LK_ZN_OUT_OF_IMAGE, a
 *             refusal of the step function is the status; neither is iterated.  lambda = lambda0.  Then trips, up to
 *             max_iters: delta from the kept sums; LK_ZN_SINGULAR: lambda *= 10 without an evaluation; else evaluate at
 *             (float)((double)p + delta) and accept when no sample is flagged, the criterion is not refused and crit' <
 *             crit strictly - then p and the sums are replaced and lambda = max(0.1 lambda, 1e-9) - else lambda *= 10.
 *             lambda >= 1e9: LK_ZN_STALLED.  An accepted step with max_k w_k |delta_k| < precision: LK_ZN_CONVERGED, with
 *             w = 1 for the translations (level-L pixels) and w = max(1, sqrt(n_L) / 2) for every other parameter - the
 *             half-width of a square subset, so the test bounds how far any sample moved.  A step that small whose
 *             evaluation is neither flagged nor refused but does not lower crit is LK_ZN_CONVERGED too, p and lambda
 *             unchanged: the float sample positions leave a noise of a few 1e-5 of crit, below which a step of less than
 *             the precision cannot be told from none, and without this rule such a sector would climb to STALLED.  No
 *             trips left:
 *             LK_ZN_MAX_ITERS (also after max_iters = 0, which evaluates the seed only).  The returned state is always the
 *             best accepted one.
 *   records   records_out [S]: the refined parameters in level-0 scale (zeros behind P), the committed centre, the level-0
 *             count, iterations = the trips taken, chi = (Sff - 2 Sfg + Sgg) / n_L of the kept sums in double - the mean
 *             squared difference that lk_evaluate's chi, scaled by 1 / n as the solve scales it, gives at the returned
 *             parameters up to its float summation - so chi_max keeps its meaning downstream (0 for LK_ZN_OUT_OF_IMAGE).
 *             errorCode: CONVERGED -> LK_ERROR_NONE; MAX_ITERS, STALLED -> LK_ERROR_CORRELATION_MAX_ITERS_REACHED;
 *             OUT_OF_IMAGE -> LK_ERROR_INTERPOLATION_OUT_OF_IMAGE; TOO_FEW, FLAT, NEGATIVE, SINGULAR -> LK_ERROR_SOLVER.
 *   info      n_points = n_L; evaluations = the passes over the samples; zncc, gain, offset and znssd (= crit) at the
 *             returned parameters, each a double rounded to float once; zncc_seed at the seed; shift = |(u, v) returned -
 *             (u, v) seed| in level-0 pixels; lambda = the final damping; last_step = max_k w_k |delta_k| of the last
 *             accepted step.  BAD_SEED and OUT_OF_IMAGE: floats and sums 0.  FLAT and TOO_FEW: the seed's sums, floats 0.
 *   modes     allowed in every mode, reference-order mode included; synchronous; writes nothing of the engine's; carries
 *             out a rebuild of the sample lists that waits for the next solve first, as lk_parameter_uncertainty does.
 *   errors    LK_ERROR_BAD_DOMAIN with a message, outputs untouched: null configuration; records_out and info_out both
 *             NULL (either alone may be); non-zero reserved words; records and guesses both given; chi_max, precision or
 *             lambda0 not finite; and what lk_parameter_uncertainty refuses (its accessor is used, its messages carry this
 *             function's name): no committed sectors; records == guesses == NULL before any batch solve of the committed
 *             sectors, or with one in flight; images not set; a bad def_slot.
 *   defaults  max_iters < 0 is 50 and precision <= 0 is 1e-3, lk_config's defaults: the pass reads the engine through the
 *             accessor of the add-on passes, which does not carry the engine's configuration.  The Python method passes
 *             the engine's own values.  lambda0 <= 0 is 1e-3.
 *   scope     one engine, level py_start only - no coarser levels, so the seed must lie within the sampler's reach of the
 *             answer (a pixel or two; lk_search_guesses brings it there); the engine-held records are never written;
 *             lk_group, lk_tracker, the report CSV and the CudaClass adapter do not call it; windows with
 *             reference_previous are not covered; inputs and outputs are host arrays; no colour frames; lk_solve_kernel
 *             and lk_backward_kernel keep the plain sum of squares. */
enum { LK_ZN_CONVERGED = 0, LK_ZN_MAX_ITERS = 1, LK_ZN_STALLED = 2,   /* lambda reached 1e9 */
       LK_ZN_BAD_SEED = 3, LK_ZN_OUT_OF_IMAGE = 4, LK_ZN_TOO_FEW = 5, LK_ZN_FLAT = 6,
       LK_ZN_NEGATIVE = 7,  /* c <= 0 at the seed: anti-correlated patches */
       LK_ZN_SINGULAR = 8 };
typedef struct lk_znssd_config {
  int def_slot;       /* as lk_photometry_config */
  float chi_max;      /* good rule for record seeds; <= 0: error code alone */
  int max_iters;      /* LM trips; 0: evaluate the seed only; < 0: 50 */
  float precision;    /* <= 0: 1e-3 */
  float lambda0;      /* <= 0: 1e-3 */
  int reserved[3];    /* must be 0 */
} lk_znssd_config;
/* (a struct tag without a typedef, as struct lk_photometry) */
struct lk_znssd {     /* 64 bytes, one per sector */
  int32_t n_points, status, iterations, evaluations;
  float zncc, gain, offset, znssd;     /* at the returned parameters; f ~ gain g + offset */
  float zncc_seed;                     /* at the seed */
  float shift;                         /* |(u, v) returned - (u, v) seed|, level-0 pixels */
  float lambda, last_step;             /* final damping; max weighted |delta| of the last accepted step */
  int32_t reserved[4];
};
/* records: host [S], or NULL = the engine-held records (guesses == NULL), or guesses: host [S][6].  records_out: [S],
 * info_out: [S], either may be NULL, not both.  sums_out: [S][45] doubles or NULL, the kept sums at the returned parameters.
 * Synchronous.  Changes no engine state. */
int lk_refine_znssd(lk_engine *e, const lk_znssd_config *cfg, const lk_result *records, const float *guesses,
                    lk_result *records_out, struct lk_znssd *info_out, double *sums_out);
/* the kernel's own function compiled for the host: criterion and damped step of one sector of n samples with the sums `sums`
 * (the model's layout, 45 doubles or fewer).  *status = 0, or LK_ZN_TOO_FEW, LK_ZN_FLAT, LK_ZN_NEGATIVE or LK_ZN_SINGULAR;
 * delta6 (zeros behind P, and all zeros unless *status = 0), crit and gain_offset2 may each be NULL.  LK_ERROR_BAD_DOMAIN
 * (outputs untouched) for a null sums or status pointer, an unknown model, n < 0 or a lambda that is negative or not
 * finite. */
int lk_znssd_step_from_sums(int model, int n, const double *sums, float lambda, double *delta6, double *crit,
                            double *gain_offset2, int32_t *status);

/* ---- second-order refinement: a subset model that can bend ------------------------------------ */
/* Every solve of the engine, lk_refine_znssd included, matches a subset with an affine shape function at most.  Where the
 * displacement curves inside a subset - next to a hole, a notch, a bend - that model is too poor and the answer carries a
 * systematic error that grows with the subset.  lk_refine_quadratic is lk_refine_znssd with second-order shape functions
 * (Lu & Cary 2000): the same seeds, level, walk, sampler, criterion, loop, statuses (LK_ZN_*), records and refusals, on
 * twelve parameters, in a kernel of its own (csrc/lk_quadratic.hip).  What is not said here is as
 * for lk_refine_znssd.
 *   model     p = (u, v, ux, uy, vx, vy, uxx, uxy, uyy, vxx, vxy, vyy), whatever the engine's fitting model is:
 *               x' = x + u + ux dx + uy dy + uxx dx^2 / 2 + uxy dx dy + uyy dy^2 / 2,  y' alike with v,
 *             dx = x - cx, dy = y - cy about the committed centre (times 2^-L).  In float, without contraction:
 *               hxx = 0.5f (dx dx), hxy = dx dy, hyy = 0.5f (dy dy),
 *               x' = (((((x + p0) + p2 dx) + p3 dy) + p6 hxx) + p7 hxy) + p8 hyy,  y' from p1, p4, p5, p9, p10, p11;
 *             with zero second-order terms these are the bits of the affine warp of the solve.
 *   level     L = py_start.  Seeds go to level L and results come back by the solve's translation: u and v times 2^-L, the
 *             four gradients unchanged, the six second-order terms times 2^L (and 2^-L on the way back).
 *   seeds     `records` and `guesses` as for lk_refine_znssd (the good rule with the engine model's P; guesses [S][6] in the
 *             engine model's meaning).  The engine model maps onto the first six parameters by its own warp: LK_FM_U: u;
 *             LK_FM_UV: u, v; LK_FM_UVQ: u, v, uy = -q, vx = q; LK_FM_UVUXUYVXVY: all six; the rest 0.  second: host
 *             [S][6] = (uxx, uxy, uyy, vxx, vxy, vyy) in level-0 scale, NULL = zeros; with it, feeding (records_out,
 *             info.p + 6) back in continues a refinement.  A sector whose second-order seeds are not all finite is
 *             LK_ZN_BAD_SEED like one whose guesses are not: errorCode LK_ERROR_BAD_DOMAIN, the first-order seed as its
 *             parameters.  (A record that fails the good rule is copied, as for lk_refine_znssd.)
 *   sums      88 doubles per evaluation (kLkQdSums), from the floats f, g, gx, gy, dx, dy of a sample; every product is
 *             formed in double and rounded once, no fused multiply-add.  X = (double)dx, X2 = X X, X3 = X2 X, X4 = X2 X2,
 *             Y alike; the 15 monomials M[k] = X^a Y^b, a + b <= 4, by degree, then by falling a, each formed as Xa Yb:
 *               [0..4]    Sf, Sg, Sff, Sgg, Sfg
 *               [5..49]   sum w M[k] for w = gx gx, then gx gy, then gy gy; k = 0 .. 14 each
 *               [50..61]  sum t for t = gx M[k], k = 0 .. 5, then t = gy M[k]
 *               [62..73]  sum t f over the same twelve t
 *               [74..85]  sum t g over the same twelve t
 *               [86]      0
 *               [87]      the samples the sampler flagged
 *             H of the twelve parameters is gx or gy times a monomial of degree <= 2 times 1 or 1/2, so SH, SHH, SHf and
 *             SHg of lk_refine_znssd's step are these moments times 1, 1/2 or 1/4, exactly.  The kernel forms the sums in
 *             three sweeps over the samples ([0..4], [50..73], [87]; [5..19], [74..85]; [20..49]); every sweep computes a
 *             sample's floats identically and adds in the uncertainty pass's fixed order, so a sector's sums, trajectory,
 *             record and info are the same bytes in any batch, shard, mode or ring slot.
 *   step      lk_quadratic_step_from_sums (one function for the kernel and the host, csrc/lk_quadratic.hpp): the
 *             criterion and the formulas of lk_znssd_step_from_sums with P = 12 - LK_ZN_TOO_FEW if n < 14; FLAT,
 *             NEGATIVE; A, b; the scaling to a diagonal of 1 + lambda; the unpivoted L D L^T; LK_ZN_SINGULAR for A_kk <= 0
 *             or a pivot <= 1e-10.
 *   loop      lk_refine_znssd's, with the weights, for h = max(1, sqrt(n_L) / 2): 1 for u, v; h for the four gradients;
 *             h^2 / 2 for uxx, uyy, vxx, vyy; h^2 for uxy, vxy - so max_k w_k |delta_k| bounds how far any sample moved.
 *   records   records_out [S] as lk_refine_znssd's - chi = (Sff - 2 Sfg + Sgg) / n_L, the counts, the centre, the
 *             errorCode mapping - with the parameters in the engine model's own layout, so that every downstream pass
 *             reads them as it reads the solve's: LK_FM_U: u; LK_FM_UV: u, v; LK_FM_UVQ: u, v, q = (vx - uy) / 2 in
 *             float; LK_FM_UVUXUYVXVY: the six first-order terms; zeros behind P.  The twelve parameters are in the info.
 *   info      as struct lk_znssd, and p[12] in level-0 scale (zeros for BAD_SEED and OUT_OF_IMAGE), shift from (u, v)
 *             both, and bend = h0^2 max(|uxx| / 2 + |uxy| + |uyy| / 2, |vxx| / 2 + |vxy| + |vyy| / 2), h0 = sqrt(n_0) / 2: the
 *             second-order displacement at the rim of the subset in level-0 pixels - where it is large, the affine model
 *             was under-matched.  BAD_SEED and OUT_OF_IMAGE: floats and sums 0.  FLAT and TOO_FEW: the seed's sums, p and
 *             bend the seed's, the other floats 0.
 *   modes     as lk_refine_znssd: every mode, synchronous, nothing of the engine is written.
 *   errors    as lk_refine_znssd, with this function's name in the messages.
 *   defaults  as lk_refine_znssd.
 *   scope     as lk_refine_znssd; and no batch solve or sequence window gets second-order terms, lk_result stays 48 bytes. */
typedef struct lk_quadratic_config {
  int def_slot;       /* the words of lk_znssd_config */
  float chi_max;
  int max_iters;
  float precision;
  float lambda0;
  int reserved[3];    /* must be 0 */
} lk_quadratic_config;
struct lk_quadratic { /* 128 bytes, one per sector */
  int32_t n_points, status, iterations, evaluations;   /* status: LK_ZN_* */
  float p[12];                         /* level-0 scale, the order above */
  float zncc, gain, offset, znssd;     /* as struct lk_znssd */
  float zncc_seed, shift, lambda, last_step;
  float bend;                          /* second-order displacement at the subset rim, level-0 pixels */
  int32_t reserved[7];
};
/* records, guesses, records_out, info_out: as lk_refine_znssd.  second: host [S][6] or NULL.  sums_out: [S][88] doubles or
 * NULL, the kept sums at the returned parameters.  Synchronous.  Changes no engine state. */
int lk_refine_quadratic(lk_engine *e, const lk_quadratic_config *cfg, const lk_result *records, const float *guesses,
                        const float *second, lk_result *records_out, struct lk_quadratic *info_out, double *sums_out);
/* the kernel's own function compiled for the host: criterion and damped step of one sector of n samples with the 88 sums
 * `sums88`.  *status = 0, or LK_ZN_TOO_FEW, LK_ZN_FLAT, LK_ZN_NEGATIVE or LK_ZN_SINGULAR; delta12 (all zeros unless
 * *status = 0), crit and gain_offset2 may each be NULL.  LK_ERROR_BAD_DOMAIN (outputs untouched) for a null sums or status
 * pointer, n < 0 or a lambda that is negative or not finite. */
int lk_quadratic_step_from_sums(int n, const double *sums88, float lambda, double *delta12, double *crit,
                                double *gain_offset2, int32_t *status);

/* ---- B-spline refinement: a sub-pixel solve without the bicubic's interpolation bias ---------- */
/* Every other sub-pixel solve of the engine reads the deformed image through the Keys / Catmull-Rom cubic, whose phase error
 * gives a measured displacement a systematic error that follows its sub-pixel part (about 0 at 0 and 0.5 px, opposite signs
 * at 0.25 and 0.75 px).  lk_refine_spline is lk_refine_znssd with g, g_x and g_y taken from a cubic or quintic B-spline of
 * the prefiltered deformed image (Unser's recursive filter; Schreier, Braasch & Sutton 2000), in kernels of its own
 * (csrc/lk_spline.hip).  What is not said here is as for lk_refine_znssd: seeds, level, walk, lane
 * groups, warp, the 45 sums, criterion and step (lk_znssd_step_from_sums), loop, statuses (LK_ZN_*), records, info.
 *   image     f stays the u8 node of the undeformed level image.  The engine's `interpolation` plays no part.
 *   prefilter every call builds the float coefficient image [rows][cols] of the level-py_start deformed image anew (no
 *             cache that could go stale).  Along every row, then along every column, for a line s[0 .. N - 1], in float,
 *             each product and each sum rounded:
 *               s[k] = lam s[k],  lam = prod (1 - z)(1 - 1 / z) = 6 (order 3) or 120 (order 5);
 *               then per pole z - order 3: sqrt(3) - 2; order 5: sqrt(67.5 - sqrt(4436.25)) + sqrt(26.25) - 6.5, then
 *               sqrt(67.5 + sqrt(4436.25)) - sqrt(26.25) - 6.5; each the float nearest the double value -
 *               c[0] = s[0] + sum zp_k s[k], k = 1 .. min(N, 28) - 1 added in ascending k, zp_1 = z, zp_(k + 1) = zp_k z;
 *               c[k] = s[k] + z c[k - 1] up to N - 1;
 *               c[N - 1] = (z / (z z - 1)) (z c[N - 2] + c[N - 1]);   c[k] = z (c[k + 1] - c[k]) down to 0
 *             (the mirror boundary).  A line is filtered in this order whatever the launch, so the coefficients are the
 *             same bytes in any call.
 *   sampler   at (x, y): ix = (int)x, t = x - ix, alike in y; nodes ix - 1 .. ix + 2 (order 3) or ix - 2 .. ix + 3 (order 5).
 *             Valid for x > 1 && x < cols - 2 (order 3, the bicubic's rule) or x > 2 && x < cols - 3 (order 5), alike in y;
 *             anything else is a flagged sample, LK_ZN_OUT_OF_IMAGE.  The weights w[] and the derivative weights g[] are
 *             the pieces of the uniform B-spline as polynomials in t, every coefficient the float nearest the fraction,
 *             by Horner's rule with one fused multiply-add per power (lk_spline_weights is that function on the host).
 *             Per image row j: v_j = fma(wx[n], c[n], ... fma(wx[1], c[1], wx[0] c[0])) and d_j alike with gx; then, folded
 *             in row by row from j = 0, W = fma(wy[j], v_j, W), Wx = fma(wy[j], d_j, Wx), Wy = fma(gy[j], v_j, Wy).
 *   modes     as lk_refine_znssd: every mode, synchronous, nothing of the engine is written.
 *   errors    as lk_refine_znssd, with this function's name in the messages; and an order that is not 0, 3 or 5; a level
 *             image with a side below 8.
 *   defaults  as lk_refine_znssd; order 0 is 5.
 *   scope     as lk_refine_znssd.  lk_refine_quadratic keeps the engine's interpolator: lk_refine_composed gives it this
 *             sampler.  The batch solve, the backward solve and the sequence windows keep theirs too. */
typedef struct lk_spline_config {
  int def_slot;       /* the words and defaults of lk_znssd_config */
  float chi_max;
  int max_iters;
  float precision;
  float lambda0;
  int order;          /* 3 or 5; 0: 5 */
  int reserved[2];    /* must be 0 */
} lk_spline_config;
/* records, guesses, records_out, info_out, sums_out: as lk_refine_znssd.  Synchronous.  Changes no engine state. */
int lk_refine_spline(lk_engine *e, const lk_spline_config *cfg, const lk_result *records, const float *guesses,
                     lk_result *records_out, struct lk_znssd *info_out, double *sums_out);
/* The coefficient image of the level-py_start image of `slot` (LK_IMG_UND, LK_IMG_DEF or LK_IMG_NXT), out: host
 * [rows][cols] floats of that level.  Needs no sectors and no other slot; allowed in every mode; changes no engine state.
 * LK_ERROR_BAD_DOMAIN with a message: a null output, a bad order, a slot that is not set, a side below 8. */
int lk_spline_coefficients(lk_engine *e, int slot, int order, float *out);
/* The pass's sampler at n points xy [n][2] (level-py_start pixels of the image of `slot`): out4 [n][4] = W, Wx, Wy, ok with
 * ok = 1, or four zeros where the sampler's window leaves the image.  Otherwise as lk_spline_coefficients. */
int lk_spline_sample(lk_engine *e, int slot, int order, const float *xy, int n, float *out4);
/* the kernel's weight function on the host: w6 and g6 take the order + 1 weights and derivative weights at the fraction t,
 * zeros behind them.  LK_ERROR_BAD_DOMAIN for a null pointer, an order that is not 0, 3 or 5, or a t that is not finite. */
int lk_spline_weights(int order, float t, float *w6, float *g6);

/* ---- weighted refinement: subsets that stop at an edge, a window that weights the centre ------ */
/* Every other sub-pixel solve of the engine gives all samples of a sector the same weight.  A sector that straddles the
 * specimen's edge, a hole's rim, an open crack or a highlight then contains pixels that do not move with the material, and
 * the solve is biased by as much as they disagree; and under a curved displacement the affine model's error grows with the
 * second moment of the subset.  lk_refine_weighted is lk_refine_znssd with a weight per sample inside the ZNSSD sums: a
 * pixel mask over the undeformed image times a Gaussian window about the committed centre, in a kernel of its own
 * (csrc/lk_weighted.hip).  What is not said here is as for lk_refine_znssd: seeds, level, walk, lane
 * groups, warp, the engine's interpolator, loop, statuses (LK_ZN_*), the record layout, refusals, modes.
 *   weight    of the sample q of a sector with the committed centre (cx, cy) at level L = py_start: w = m g.
 *             m = 1 without a mask, or where the mask byte at the sample's undeformed node - the node f is read at,
 *             ((int)(x + 0.5f), (int)(y + 0.5f)) - is nonzero; else 0.  g = 1 for sigma == 0, else the window below at
 *             (q.x - cx, q.y - cy) with sigma_L = sigma 2^-L.  Rectangles and sample lists alike.
 *   window    lk_weight_window (one function for the kernel and the host, csrc/lk_weighted.hpp), in float:
 *             r2 = fma(dy, dy, dx dx), t = r2 inv with inv = (float)(log2(e) / (2 sigma_L^2)) formed once on the host in
 *             double; the window is 2^-t: k = (int)(t + 0.5f), x = t - k, 2^-x by the Taylor polynomial of degree 7 of
 *             exp(-x ln 2), every coefficient the float nearest (-ln 2)^j / j!, by Horner's rule with one fused multiply-add
 *             per power, then ldexpf(.., -k).  t >= 126: 0.  No library exponential: host and device give the same bits.
 *             Within 1e-6 relative of exp(-r^2 / (2 sigma^2)) in double over the subset the window is made for, |dx|,
 *             |dy| <= 3 sigma (the float rounding of t alone is a relative 2^-23 t ln 2 of the result).
 *   prologue  per sector, before the loop, one pass over the weights and one reduction in the fixed order of the sums:
 *             n_valid = the samples with w > 0, Sw = sum w, Sww = sum w^2, sum w dx, sum w dy (dx, dy in float as above;
 *             products and sums in double).  N = Sw; n_eff = Sw^2 / Sww; the centroid offset = (sum w d / Sw) 2^L.
 *             n_valid < P + 2, or n_valid < min_fraction n_L (in double): LK_ZN_TOO_FEW - no pixel of either image is read,
 *             evaluations = 0, floats and sums 0 (weight_sum, n_eff and the centroid are filled; all 0 for n_valid = 0).
 *   sums      a sample with w == 0 is skipped before anything of it is read: it is never sampled and never flagged, so a
 *             mask over the columns whose warped positions leave the deformed image rescues a sector that is
 *             LK_ZN_OUT_OF_IMAGE as a whole.  Every other term of lk_refine_znssd's 45 sums is formed exactly as there,
 *             then multiplied by (double)w - a rounded product - then added; the flagged count is not weighted.  sums_out
 *             is [S][45] in the same layout.  With every w = 1 (sigma == 0 and no mask, or a mask of ones) the sums, and
 *             with them the records and the first 48 bytes of the info, are lk_refine_znssd's bytes.
 *   step      lk_weighted_step_from_sums: the arithmetic of lk_znssd_step_from_sums with N = Sw in place of (double)n and
 *             n_valid in the too-few test.  The weights of the convergence test keep n_L, the full count: the test bounds
 *             how far any sample of the support moved.
 *   records   as lk_refine_znssd's, with chi = (Sff - 2 Sfg + Sgg) / Sw of the kept sums; the centre stays the committed
 *             one and numberOfPoints the level-0 count: the solve reports the affine map at the committed centre, and
 *             centroid_dx, centroid_dy tell how far the centroid of the data lies from it.
 *   errors    as lk_refine_znssd, with this function's name in the messages; and a sigma that is negative or not finite
 *             (or so small that inv is not a finite float); min_fraction outside [0, 1]; mask dimensions that are not
 *             those of the level-py_start undeformed image; a mask without dimensions, or dimensions without a mask.
 *   defaults  as lk_refine_znssd.
 *   scope     as lk_refine_znssd; the engine's interpolator only - the B-spline sampler and the twelve-parameter model with
 *             weights are lk_refine_composed's; no batch solve, backward solve or sequence window gets weights; the mask lives on the
 *             undeformed configuration only (no mask on the deformed image).  The mask is uploaded by every call: nothing
 *             is cached that could go stale. */
typedef struct lk_weighted_config {
  int def_slot;       /* the words and defaults of lk_znssd_config */
  float chi_max;
  int max_iters;
  float precision;
  float lambda0;
  float sigma;        /* Gaussian window, standard deviation in level-0 pixels; 0: no window (w = 1) */
  float min_fraction; /* in [0, 1]; a sector with n_valid < min_fraction * n_L is LK_ZN_TOO_FEW; 0: the P + 2 rule alone */
  int mask_rows, mask_cols;   /* of `mask`: the level-py_start undeformed image's; 0, 0 with mask == NULL */
  int reserved[3];    /* must be 0 */
} lk_weighted_config;
struct lk_weighted {  /* 80 bytes, one per sector: struct lk_znssd's first 48 bytes, then the weights' */
  int32_t n_points, status, iterations, evaluations;   /* status: LK_ZN_*; n_points = n_L */
  float zncc, gain, offset, znssd;     /* as struct lk_znssd, of the weighted sums */
  float zncc_seed, shift, lambda, last_step;
  int32_t n_valid;                     /* samples with w > 0 */
  float weight_sum, n_eff;             /* Sw; Sw^2 / Sww */
  float centroid_dx, centroid_dy;      /* centroid of the weights - committed centre, level-0 pixels.  Unit weights: exactly
                                        * 0 for a rectangle; for a sample list the committed centre is the float32 nearest
                                        * the samples' mean, so that rounding is left (below one float32 step of the centre) */
  int32_t reserved[3];
};
/* mask: host [mask_rows][mask_cols] bytes, nonzero = use, or NULL.  records, guesses, records_out, sums_out: as
 * lk_refine_znssd; info_out: [S] or NULL (not both outputs).  Synchronous.  Changes no engine state. */
int lk_refine_weighted(lk_engine *e, const lk_weighted_config *cfg, const uint8_t *mask, const lk_result *records,
                       const float *guesses, lk_result *records_out, struct lk_weighted *info_out, double *sums_out);
/* the kernel's window function on the host: *w = the window at (dx, dy) for inv = log2(e) / (2 sigma^2).
 * LK_ERROR_BAD_DOMAIN for a null pointer, an inv that is negative or not finite, or an offset that is not finite. */
int lk_weight_window(float inv, float dx, float dy, float *w);
/* lk_znssd_step_from_sums for n_valid samples of total weight N (N = n_valid gives its bits).  LK_ERROR_BAD_DOMAIN also for
 * an N that is negative or not finite. */
int lk_weighted_step_from_sums(int model, int n_valid, double N, const double *sums, float lambda, double *delta6,
                               double *crit, double *gain_offset2, int32_t *status);

/* ---- composed refinement: model order, sampler and weights chosen independently --------------- */
/* lk_refine_quadratic, lk_refine_spline and lk_refine_weighted each give lk_refine_znssd one more capability: a model that
 * bends, a sampler without the bicubic's phase error, weights with a mask.  lk_refine_composed gives them together: next to
 * a hole a subset needs the mask AND the model that bends, and a strain map without bands needs the spline sampler under
 * whichever model and weights were chosen.  The kernels are the two shared loop bodies with the samplers and the weight
 * policy of the four passes (csrc/lk_composed.hip).  Every rule is the one of the pass whose option is
 * chosen; what is not said here is said there.
 *   order     1: the engine's model, lk_refine_znssd's parameters, 45 sums (sums_out [S][45]).  2: the twelve parameters
 *             of lk_refine_quadratic, its warp, its 88 sums in three sweeps (sums_out [S][88]), its step, its convergence
 *             weights, its record layout.
 *   sampler   0: the engine's interpolator.  3 / 5: the cubic / quintic B-spline of lk_refine_spline - its prefilter, run by
 *             every call on the level-py_start deformed image, its sampler, its validity rule.
 *   weights   lk_refine_weighted's: w = mask(node) window(q - centre), sigma = 0 and mask == NULL give w = 1; its prologue
 *             (n_valid, Sw, Sww, the centroid), the skip of a sample with w == 0 before anything of it is read - in all
 *             three sweeps with order 2 -, N = Sw, min_fraction.  The too-few rule is n_valid < P + 2, P = 12 with order 2.
 *   seeds     lk_refine_quadratic's: records or guesses in the engine model's meaning; `second` [S][6] with order 2 only.
 *             Level, statuses (LK_ZN_*), the BAD_SEED rules and the record that passes through: as there.
 *   sums      order 1: lk_refine_weighted's (under a spline sampler lk_refine_spline's g, g_x, g_y).  Order 2: every term of
 *             the 88 sums is lk_refine_quadratic's term, then multiplied by (double)w - a rounded product - then added; the
 *             flagged count is not weighted.  Which sweep holds a sum changes no bit of it.
 *   step      lk_composed_step_from_sums: lk_weighted_step_from_sums (order 1) or the arithmetic of
 *             lk_quadratic_step_from_sums with N = Sw in place of (double)n and n_valid in the too-few test (order 2).  The
 *             weights of the convergence test keep n_L.
 *   records   as the chosen order's, with chi = (Sff - 2 Sfg + Sgg) / Sw of the kept sums.
 *   info      struct lk_composed: struct lk_quadratic's words up to bend, then struct lk_weighted's n_valid, weight_sum,
 *             n_eff, centroid_dx, centroid_dy.  Order 1: p[0 .. P - 1] = the engine model's parameters as in the record
 *             (zeros behind them; all zeros for BAD_SEED and OUT_OF_IMAGE), bend = 0.
 *   reduces   with unit weights and the matching options the records, the shared info words and the sums are the bytes of
 *             lk_refine_znssd (1, 0), lk_refine_spline (1, 3 / 5) and lk_refine_quadratic (2, 0); (1, 0) with weights is
 *             lk_refine_weighted's kernel itself.
 *   modes     as lk_refine_znssd: every mode, synchronous, nothing of the engine is written; nothing is cached between calls.
 *   errors    the union of the four passes' refusals with this function's name in the messages, outputs untouched; and an
 *             order that is not 1 or 2; a sampler that is not 0, 3 or 5; `second` given with order 1.
 *   defaults  as lk_refine_znssd.
 *   scope     as lk_refine_znssd; no mask on the deformed image; no sampler or model beyond these. */
typedef struct lk_composed_config {
  int def_slot;       /* the words and defaults of lk_znssd_config */
  float chi_max;
  int max_iters;
  float precision;
  float lambda0;
  int order;          /* 1: the engine's model; 2: twelve parameters */
  int sampler;        /* 0: the engine's interpolator; 3 / 5: cubic / quintic B-spline */
  float sigma;        /* the words of lk_weighted_config */
  float min_fraction;
  int mask_rows, mask_cols;
  int reserved[5];    /* must be 0 */
} lk_composed_config;
struct lk_composed {  /* 128 bytes, one per sector: the layout of struct lk_quadratic */
  int32_t n_points, status, iterations, evaluations;   /* status: LK_ZN_* */
  float p[12];                         /* level-0 scale; order 1: the engine model's P parameters, zeros behind them */
  float zncc, gain, offset, znssd;     /* of the weighted sums */
  float zncc_seed, shift, lambda, last_step;
  float bend;                          /* as struct lk_quadratic; 0 with order 1 */
  int32_t n_valid;                     /* as struct lk_weighted */
  float weight_sum, n_eff;
  float centroid_dx, centroid_dy;
  int32_t reserved[2];
};
/* mask: as lk_refine_weighted.  records, guesses, second, records_out: as lk_refine_quadratic; info_out: [S] or NULL (not
 * both outputs).  sums_out: [S][45] (order 1) or [S][88] (order 2) doubles or NULL.  Synchronous.  Changes no engine state. */
int lk_refine_composed(lk_engine *e, const lk_composed_config *cfg, const uint8_t *mask, const lk_result *records,
                       const float *guesses, const float *second, lk_result *records_out, struct lk_composed *info_out,
                       double *sums_out);
/* criterion and step of either order for n_valid samples of total weight N.  order 1: lk_weighted_step_from_sums of `model`,
 * delta12 zeros behind P.  order 2: lk_quadratic_step_from_sums with N in place of (double)n (N = n_valid gives its bits);
 * the model plays no part.  LK_ERROR_BAD_DOMAIN (outputs untouched) as those two, and for an order that is not 1 or 2. */
int lk_composed_step_from_sums(int order, int model, int n_valid, double N, const double *sums, float lambda,
                               double *delta12, double *crit, double *gain_offset2, int32_t *status);

/* ---- field map: dense displacement and strain maps on a regular grid of nodes ---------------- */
/* lk_field_map gives the full-field picture a DIC user looks at first: u, v, the gradients, the strain tensor and its
 * principal values on a regular grid of nodes - every pixel, or every stride-th - drawn in the reference image or over the
 * deformed frame, for a colour map or for comparison with an FE result on the same grid.  Per node it is lk_track_points'
 * windowed least-squares plane (LK_TRACK_TOTAL) around the node's position, optionally with a weight that falls to zero at
 * the rim of the window, so that the map has no steps where a sector enters or leaves it (csrc/lk_field.hip, DESIGN.md
 * section 22).  The call reads no image: the nodes need not lie inside any.
 *   data      lk_strain_field's and lk_track_points': position of a sector = the engine's committed centre c; u = p[0],
 *             v = p[1], v = 0 for LK_FM_U; the record's gradient parameters are not used.
 *   good      the shared rule (one device function): LK_ERROR_NONE, finite parameters (the model's P), finite chi and, if
 *             chi_max > 0, chi <= chi_max.
 *   nodes     node (i, j), 0 <= i < nx, 0 <= j < ny, is the level-0 position (x0 + i stride, y0 + j stride): exact doubles
 *             formed from the integers (in 64-bit arithmetic).
 *   window    of a position (X, Y): every good sector with d2 = dx^2 + dy^2 <= r2, where dx = (double)cx - X, dy alike,
 *             each product and the sum rounded to double (no fused multiply-add) and r2 = (double)radius squared.  n = the
 *             number of such sectors, the members.
 *   weight    LK_FIELD_UNIFORM: w = 1.  LK_FIELD_BISQUARE: t = 1.0 - d2 / r2, w = t t.  A member on the rim has w = 0 and
 *             still counts in n.
 *   sums      in the order the members are met (`order`): W += w; with wx = w x and wy = w y (x = dx, y = dy) the eleven
 *             sums Sx += wx, Sy += wy, Sxx += wx x, Sxy += wx y, Syy += wy y, Su += w u, Sxu += wx u, Syu += wy u, Sv += w v,
 *             Sxv += wx v, Syv += wy v, each product and each sum rounded to double.  With w = 1 these are the bits of
 *             lk_track_points' sums added in that order.
 *   fit       lk_field_from_sums (one function for the kernel and the host, csrc/lk_field.hpp): lk_strain_field's `fit`
 *             formulas with n replaced by W - Cxx = Sxx - Sx Sx / W, ..., D = Cxx Cyy - Cxy Cxy, ux = (Cyy Cxu - Cxy Cyu) / D,
 *             ..., u0 = Su / W - ux (Sx / W) - uy (Sy / W) (the plane at the position), v0 alike.  Status, checked in this
 *             order: TOO_FEW  n < min_neighbours;  DEGENERATE  not W > 0, Cxx Cyy == 0, not Cxx > 2^-40 Sxx, not
 *             Cyy > 2^-40 Syy, or not D > 1e-6 Cxx Cyy (lk_track_points' `degenerate` paragraph on the weighted moments);
 *             OK.  The twelve values u0, v0, ux, uy, vx, vy - each rounded to float once - and lk_strain_from_gradient of
 *             those four float gradients: exx, eyy, exy, e1, e2, theta.
 *   frame     LK_FIELD_REFERENCE: one fit at the node.  The twelve values, X0 = Y0 = the node, MISFIT = 0.
 *             LK_FIELD_DEFORMED: the node x is a position on the deformed frame, and the map shows the material point that
 *             moved there.  X_0 = x; for k = 0 .. K - 1, K = iterations: X_{k+1} = x - (u0, v0) of the fit at X_k, in
 *             double; there is no early exit.  The twelve values are those of the fit at X_K - Lagrangian gradients and
 *             strain, drawn at the deformed position; X0, Y0 = (float)X_K; MISFIT = (float)hypot(ex, ey) with
 *             ex = (X_K + u0) - x, ey alike, of that last fit: how far the point found is from moving onto the node.  If any
 *             of the K + 1 fits is not OK, the node gets that fit's status and n and no later fit is made.
 *   outputs   maps is [C][ny][nx] floats, C = the number of bits set in `channels`, the planes in ascending bit order;
 *             neighbours (n of the node's last fit) and status (LK_FIELD_*) are [ny][nx], each may be NULL.  A node without
 *             a fit has NaN in every float channel, like lk_residual_map.
 *   order     fixed: the members of a position are met cell by cell of a grid of cell size `radius` over the centres - the
 *             rows iy - 1, iy, iy + 1 of cells ascending, the cells ix - 1 .. ix + 1 ascending within a row, ascending
 *             sector index within a cell (the position's cell as for lk_track_points, clamped to [-2, nx + 1]) - and summed
 *             by one thread.  A tile of 32 x 8 nodes keeps the members of all cells its nodes reach in LDS in that same
 *             order and every node scans them all; when they do not fit, or an iterate of the deformed frame leaves them,
 *             the node walks its own 3 x 3 cells in global memory.  A superset of cells adds only sectors farther than a
 *             cell = radius away, which fail the distance test.  A node's bytes therefore depend on that node, the centres,
 *             the records and the configuration only - not on the window it is part of, the stride, the channel selection,
 *             the tile or the path taken.  A float64 restatement reproduces them up to the order of the double sums.
 *   modes     allowed in every mode, reference-order mode included: the call writes nothing of the engine's - records,
 *             guesses, last parameters, counters and the other passes' outputs stay byte for byte - and, as for
 *             lk_strain_field, a rebuild of the sample lists that waits for the next solve keeps waiting.  Synchronous.
 *   errors    LK_ERROR_BAD_DOMAIN with a message, outputs untouched: what lk_strain_field refuses (null configuration; no
 *             committed sectors; records == NULL before any batch solve of the committed sectors, or with one in flight;
 *             radius not finite or <= 0; chi_max not finite; min_neighbours < 3; unknown tensor); an unknown weight or
 *             frame; iterations outside 1 .. 16 in the deformed frame; nx, ny or stride < 1; nx ny > 2^31 - 1; unknown
 *             channel bits; channels == 0 with both integer maps NULL; maps == NULL with channels != 0; non-zero reserved
 *             words.
 *   scope     one engine; the maps are host arrays.  lk_group, lk_tracker, the report CSV and the CudaClass adapter do not
 *             call it.  No image is read or drawn: a channel is a plain [ny][nx] float array (README: one written as CSV). */
enum { LK_FIELD_OK = 0, LK_FIELD_TOO_FEW = 1, LK_FIELD_DEGENERATE = 2 };
enum { LK_FIELD_UNIFORM = 0, LK_FIELD_BISQUARE = 1 };    /* weight */
enum { LK_FIELD_REFERENCE = 0, LK_FIELD_DEFORMED = 1 };  /* frame */
/* channel bits, in this order in the output */
enum { LK_FIELD_U = 1 << 0, LK_FIELD_V = 1 << 1, LK_FIELD_UX = 1 << 2, LK_FIELD_UY = 1 << 3, LK_FIELD_VX = 1 << 4,
       LK_FIELD_VY = 1 << 5, LK_FIELD_EXX = 1 << 6, LK_FIELD_EYY = 1 << 7, LK_FIELD_EXY = 1 << 8, LK_FIELD_E1 = 1 << 9,
       LK_FIELD_E2 = 1 << 10, LK_FIELD_THETA = 1 << 11, LK_FIELD_X0 = 1 << 12, LK_FIELD_Y0 = 1 << 13,
       LK_FIELD_MISFIT = 1 << 14, LK_FIELD_ALL = (1 << 15) - 1 };
typedef struct lk_field_map_config {
  float radius, chi_max;        /* as lk_strain_config */
  int min_neighbours, tensor;
  int weight;                   /* LK_FIELD_UNIFORM / LK_FIELD_BISQUARE */
  int frame;                    /* LK_FIELD_REFERENCE / LK_FIELD_DEFORMED */
  int iterations;               /* K, 1 .. 16; read in the deformed frame only */
  int x0, y0, nx, ny, stride;   /* nodes (x0 + i stride, y0 + j stride), level-0 pixels; nx, ny, stride >= 1 */
  uint32_t channels;            /* LK_FIELD_U | ... : the planes of `maps` */
  int reserved[3];              /* must be 0 */
} lk_field_map_config;
/* records: host [S], or NULL = the engine-held records of the last finished batch solve.  maps: host [C][ny][nx] (NULL only
 * with channels == 0); neighbours, status: host [ny][nx] or NULL.  Synchronous.  Changes no engine state. */
int lk_field_map(lk_engine *e, const lk_field_map_config *cfg, const lk_result *records, float *maps, int32_t *neighbours,
                 uint8_t *status);
/* the kernel's own fit compiled for the host (csrc/lk_field.hpp): n, W and the eleven sums of the `sums` paragraph ->
 * *status and the twelve floats {u, v, ux, uy, vx, vy, exx, eyy, exy, e1, e2, theta} (all NaN unless *status is LK_FIELD_OK).
 * LK_ERROR_BAD_DOMAIN for a null pointer, n < 0, min_neighbours < 3 or an unknown tensor. */
int lk_field_from_sums(int min_neighbours, int n, double W, const double *sums11, int tensor, float *out12, int32_t *status);

/* ---- speckle quality: is the pattern good enough, and how large must the subsets be ---------------- */
/* Every pass above judges a field after the solve.  These two answer what a user asks before the first one, from one image
 * alone: lk_pattern_quality gives every committed sector the classical figures of its speckle pattern - the sum of squared
 * subset intensity gradients (SSSIG) and the mean intensity gradient (MIG) of Pan et al., the structure tensor and the
 * displacement error it predicts for a given camera noise, the saturated fraction; lk_suggest_subset gives, for any points,
 * the smallest square subset around each whose SSSIG reaches a threshold - it needs no sectors: it is what one runs to
 * choose them (csrc/lk_pattern.hip).
 *   level     both calls work at L = py_start and read ONE image slot, cfg->slot = LK_IMG_UND, LK_IMG_DEF or LK_IMG_NXT; only
 *             that slot has to be set.  Ring slots are out of scope.
 *   pixels    I(x, y) of the level-L image, u8 taken as integers.  The doubled central differences use clamped neighbours:
 *               gx2 = I(min(x + 1, cols - 1), y) - I(max(x - 1, 0), y),  gy2 alike in y;
 *             the gradient is gx2 / 2, so every sum below is an integer: Gxx = sum gx2^2, Gyy = sum gy2^2,
 *             Gxy = sum gx2 gy2, and SSSIG_x = Gxx / 4, SSSIG_y = Gyy / 4.
 *
 * lk_pattern_quality
 *   samples   the sector's level-L list or implicit rectangle, by lk_parameter_uncertainty's walk and lane groups (16 / 64 /
 *             512 lanes from the level-0 sample count; lane j takes the samples j, j + G, ...).  A sample's pixel is its node
 *             ((int)(x + 0.5f), (int)(y + 0.5f)), clamped to the image, read from the chosen slot.
 *   sums      nine int64 per sector, in this order: sum I, sum I^2, Gxx, Gyy, Gxy, n_low = the samples with I <= grey_low,
 *             n_high = those with I >= grey_high, min I, max I.  Integer sums are the same bits in any order.  And one
 *             double: mig_sum = sum sqrt((double)(gx2^2 + gy2^2)), added in the uncertainty pass's fixed order, so a
 *             sector's numbers and its record are the same bytes in any batch or mode.
 *   record    lk_pattern_from_sums (one function for the kernel and the host, csrc/lk_pattern.hpp): the sums converted to
 *             double first, all in double without fused multiply-add, each output rounded to float once; N = (double)n:
 *               mean = S1 / N;  std = sqrt(max(0, N S2 - S1 S1)) / N (population);  grey_min, grey_max;
 *               frac_low = n_low / N, frac_high = n_high / N;  sssig_x = Gxx / 4, sssig_y = Gyy / 4 (sums, as Pan's);
 *               mig = mig_sum / (2 N);
 *               det = Gxx Gyy - Gxy Gxy;  sigma_u = s sqrt(8 Gyy / det), sigma_v = s sqrt(8 Gxx / det) with
 *               s = noise_sigma (<= 0 means 1): Cov = 2 s^2 G^-1 - noise s in both images, G the structure tensor in
 *               gradient units - so c00 = s^2 (8 Gyy / det), c11 = s^2 (8 Gxx / det), c01 = s^2 (-8 Gxy / det);
 *               sigma_major = sqrt((c00 + c11) / 2 + sqrt(((c00 - c11) / 2)^2 + c01^2)), theta = atan2(2 c01, c00 - c11) / 2,
 *               the ellipse formulas of lk_parameter_uncertainty.  Level-L pixels.
 *             The image decides the record, not the fitting model: it is always two-dimensional.
 *   status    checked in this order: TOO_FEW  n < 2 (every field but n_points is 0);  FLAT  Gxx + Gyy == 0;  APERTURE
 *             det <= 1e-6 Gxx Gyy in double (one of them 0 included; scale-free, lk_strain_field's degenerate rule);
 *             SATURATED  (double)(n_low + n_high) > (double)max_saturated N;  OK.  FLAT and APERTURE leave the four sigma
 *             fields and theta at 0; everything else is filled.
 *
 * lk_suggest_subset
 *   candidates half-widths h = half_min, half_min + half_step, ... <= half_max, with 1 <= half_min <= half_max <=
 *             LK_PATTERN_MAX_HALF and half_step >= 1; n_cand = (half_max - half_min) / half_step + 1.
 *   point     (x, y), a float position in level-L pixels; its node is ((int)(x + 0.5f), (int)(y + 0.5f)).  A position that
 *             is not finite or a node outside the image: BAD_POINT (every other field and the point's sums are 0).
 *   box       of a candidate: node +- h, clipped to the image.  Gxx and Gyy of a box are sums over its pixels of the
 *             definitions above (the clamped neighbours are those of the IMAGE, not of the box).
 *   rule      T = ceil(4 (double)sssig_min) as an integer; a candidate passes when Gxx >= T and Gyy >= T, compared as
 *             integers.  The suggestion is the smallest passing candidate (status OK); if none passes the status is NONE and
 *             the box reported is the largest candidate's.  Nested boxes of non-negative terms make the rule monotone.
 *   record    half, status, n_pixels and clipped (0 / 1) of the reported box, sssig_x = Gxx / 4, sssig_y = Gyy / 4, and Pan's
 *             sigma_u = s sqrt(2 / sssig_x), sigma_v = s sqrt(2 / sssig_y) in double, rounded to float once (0 where the
 *             sum is 0).  A point's record depends on that point, the image and the configuration only.
 *   tables    the call builds summed-area tables of gx2^2 and gy2^2 over the whole level-L image, on every call, and answers
 *             every candidate from four corners.  The tables are uint32 and wrap: a clipped box has at most 257 x 257 pixels
 *             of at most 255^2 each, 4 294 836 225 < 2^32 in all, so the four-corner difference modulo 2^32 is the exact sum
 *             although the table itself wraps many times.  That is why LK_PATTERN_MAX_HALF is 128; it halves the footprint
 *             and the traffic against 64-bit tables.
 *
 *   modes     both calls are allowed in every mode, reference-order mode included, and change no engine state: records,
 *             guesses, last parameters, counters and lk_get_reseed_info stay byte for byte.  lk_pattern_quality carries out a
 *             rebuild of the sample lists that waits for the next solve first, as lk_parameter_uncertainty does.  Both
 *             synchronise the engine's stream before they return.
 *   errors    LK_ERROR_BAD_DOMAIN with a message prefixed by the function's name, outputs untouched: null configuration or
 *             output; unknown slot, or slot not set; non-zero reserved words; grey_low / grey_high outside 0 .. 255;
 *             noise_sigma or max_saturated not finite; lk_pattern_quality without committed sectors; lk_suggest_subset with
 *             n_points < 1, null points, a bad candidate range, or a threshold that is not finite, <= 0 or above 2^32 - 1.
 *   scope     one engine, one grey image.  lk_group, lk_tracker, the report CSV and the CudaClass adapter do not call them. */
#define LK_PATTERN_MAX_HALF 128
enum { LK_PATTERN_OK = 0, LK_PATTERN_TOO_FEW = 1, LK_PATTERN_FLAT = 2, LK_PATTERN_APERTURE = 3, LK_PATTERN_SATURATED = 4 };
enum { LK_SUBSET_OK = 0, LK_SUBSET_NONE = 1, LK_SUBSET_BAD_POINT = 2 };
typedef struct lk_pattern_config {
  int slot;                 /* LK_IMG_UND, LK_IMG_DEF or LK_IMG_NXT */
  int grey_low, grey_high;  /* 0 .. 255: I <= grey_low counts as low, I >= grey_high as high */
  float noise_sigma;        /* camera noise in grey levels; <= 0: 1 */
  float max_saturated;      /* SATURATED when (n_low + n_high) / n exceeds it */
  int reserved[3];          /* must be 0 */
} lk_pattern_config;
/* (struct tags without typedefs, as struct lk_photometry) */
struct lk_pattern {                       /* 64 bytes, one per sector */
  int32_t n_points, status;
  float mean, std;                        /* grey levels; population standard deviation */
  int32_t grey_min, grey_max;
  float frac_low, frac_high;
  float sssig_x, sssig_y;                 /* Gxx / 4, Gyy / 4 */
  float mig;                              /* mean intensity gradient */
  float sigma_u, sigma_v;                 /* predicted standard deviation of u and v, level-L pixels */
  float sigma_major, theta;               /* major axis of that covariance and its angle */
  int32_t reserved;
};
/* out: [S].  sums_out: [S][9] int64 or NULL.  mig_sum_out: [S] doubles or NULL.  Synchronous.  Changes no engine state. */
int lk_pattern_quality(lk_engine *e, const lk_pattern_config *cfg, struct lk_pattern *out, int64_t *sums_out, double *mig_sum_out);
/* the kernel's own function compiled for the host: the record of one sector of n samples with the nine sums `sums9` and
 * mig_sum.  LK_ERROR_BAD_DOMAIN for a null pointer, n < 0, or a noise_sigma or max_saturated that is not finite. */
int lk_pattern_from_sums(int n, const int64_t *sums9, double mig_sum, float noise_sigma, float max_saturated, struct lk_pattern *out);
typedef struct lk_subset_config {
  int slot;                           /* as lk_pattern_config */
  int half_min, half_max, half_step;  /* candidates: box side = 2 h + 1 */
  float sssig_min;                    /* the threshold on SSSIG_x and SSSIG_y, squared grey levels */
  float noise_sigma;                  /* as lk_pattern_config */
  int reserved[2];                    /* must be 0 */
} lk_subset_config;
struct lk_subset {                    /* 32 bytes, one per point */
  int32_t half, status;               /* the suggested half-width (NONE: the largest candidate; BAD_POINT: 0) */
  int32_t n_pixels, clipped;          /* of the reported box: pixels after clipping to the image; 1 if it was clipped */
  float sssig_x, sssig_y;
  float sigma_u, sigma_v;             /* s sqrt(2 / sssig) */
};
/* points_xy: [n_points][2] level-L positions.  out: [n_points].  sums_out: [n_points][n_cand][2] uint32 {Gxx, Gyy} of every
 * candidate box, or NULL.  Synchronous.  Changes no engine state; needs no committed sectors. */
int lk_suggest_subset(lk_engine *e, const lk_subset_config *cfg, int n_points, const float *points_xy, struct lk_subset *out,
                      uint32_t *sums_out);

/* ---- camera noise: the photon-transfer curve from static frames ---------------------------------- */
/* lk_pattern_quality and lk_suggest_subset predict a displacement error "for a given camera noise", lk_parameter_uncertainty
 * reports a residual in which camera noise, misfit and interpolation error are mixed, lk_flag_outliers has a noise floor.
 * These two calls measure the camera's part on its own, the way an experiment starts: K frames of the unloaded, unmoved
 * specimen.  The temporal variance of every pixel, binned by the pixel's mean grey level, is the photon-transfer curve
 * var(g) = a + b g - a: read noise and quantisation, b: the gain of the shot noise.  lk_camera_noise gives the curve and
 * the pooled figures of a region, lk_sector_noise the noise of every committed sector over its own samples
 * (csrc/lk_noise.hip, csrc/lk_noise.hpp).
 *   level     both calls work at L = py_start, the level of lk_pattern_quality: the sigma is the one its noise_sigma means.
 *   frames    cfg->source = LK_NOISE_IMAGES: the image slots slots[0 .. n_frames - 1] (LK_IMG_UND, LK_IMG_DEF, LK_IMG_NXT,
 *             distinct; K = n_frames is 2 or 3);  LK_NOISE_RING: the ring slots first .. first + n_frames - 1 (no wrap;
 *             K = 2 .. LK_NOISE_MAX_FRAMES).  Every frame must be set and all must have the same level-L dimensions.
 *   integers  the GPU produces integers only, so its outputs are the same bytes on every run, for every grid and every
 *             decomposition of a region.  Per counted pixel with its K values x_f (u8 taken as integers):
 *               s1 = sum x_f,  s2 = sum x_f^2,  q = K s2 - s1^2  (= K sum_f (x_f - mean)^2; K = 2: (a - b)^2; < 2^25),
 *               g = (2 s1 + K) / (2 K) in integer division: the rounded temporal mean, 0 .. 255.
 *
 * lk_camera_noise
 *   pixels    the region x0 .. x1, y0 .. y1 of the level-L frame, inclusive (all four 0: the whole frame), and of those the
 *             pixels whose mask byte is nonzero (mask: [rows][cols] of the level-L frame, or NULL: all).
 *   tables    bins[g] = {count, sum q} over the counted pixels of bin g, [256][2] int64;  frame_sums[f] = sum of x_f over
 *             the counted pixels, [K] int64;  N = sum count.
 *   record    lk_noise_from_bins (host only) from the tables, in double, each float field rounded once.  The integer
 *             combinations below are formed exactly (128-bit) before the one division:
 *               var = SQ / (N K (K - 1)) with SQ = sum_g sum q_g (the pooled temporal variance);  sigma = sqrt(var);
 *               mean = sum_f frame_sums[f] / (K N);
 *               o_f = frame_sums[f] / N - mean, the offset of frame f (from the integer K frame_sums[f] - sum frame_sums);
 *               flicker = sqrt(sum o_f^2 / K);
 *               var_detrended = (SQ / K - N sum o_f^2) / ((N - 1)(K - 1)), not below 0: the variance left when every
 *               frame's own offset is taken out - an identity, no second pass over the pixels;
 *               sigma_detrended = sqrt(var_detrended);
 *               a, b: the count-weighted least-squares line var_g = a + b g over the bins with count >= min_count and
 *               grey_low <= g <= grey_high, var_g = sum q_g / (count_g K (K - 1)); bins_used of them; a negative a or b is
 *               reported as fitted;  fit_rms = sqrt(sum count_g (var_g - a - b g)^2 / sum count_g) over those bins (0 with
 *               two bins: the line passes through both);
 *               sigma_at_mean = sqrt(max(a + b mean, 0)).
 *   status    LK_NOISE_TOO_FEW  N < 2: every field but n_pixels and n_frames is 0;  LK_NOISE_NO_MODEL  fewer than two
 *             usable bins: a = var, b = 0, fit_rms = 0, the pooled fields valid;  LK_NOISE_OK.
 *
 * lk_sector_noise
 *   samples   the sector's level-L list or implicit rectangle in lk_pattern_quality's walk and lane groups.  A sample's
 *             pixel is its node ((int)(x + 0.5f), (int)(y + 0.5f)); a sample outside the frame - x + 0.5f or y + 0.5f below
 *             0 or not below the frame's size, as floats - is skipped and not counted.  The region, the mask, grey_low, grey_high and min_count of the configuration are ignored.
 *   sums      three int64 per sector: n = the counted samples, sum q, sum s1.
 *   record    lk_noise_from_sums (host only): var = sum q / (n K (K - 1)), sigma = sqrt(var), mean = sum s1 / (n K);
 *             LK_NOISE_TOO_FEW for n < 2 (every field but n is 0), else LK_NOISE_OK.
 *
 *   modes     both calls are allowed in every mode and change no engine state: records, guesses, counters and the launch
 *             report stay byte for byte.  lk_sector_noise carries out a pending rebuild of the sample lists first, as
 *             lk_pattern_quality does.  Both synchronise the engine's stream before they return.
 *   errors    LK_ERROR_BAD_DOMAIN with a message prefixed by the function's name, outputs untouched: null configuration or
 *             output; non-zero reserved words; an unknown source; n_frames out of range; unknown or repeated image slots, or
 *             one not set; unknown or empty ring slots; frames of unequal dimensions; an empty region or one outside the
 *             frame; grey_low / grey_high outside 0 .. 255; min_count < 2 (these three lk_camera_noise only);
 *             lk_sector_noise without committed sectors.  The two host functions return LK_ERROR_BAD_DOMAIN for a null
 *             pointer, n_frames outside 2 .. LK_NOISE_MAX_FRAMES, a negative table entry, and lk_noise_from_bins also for
 *             greys outside 0 .. 255 or min_count < 2.
 *   scope     one engine, grey frames.  lk_group, lk_tracker and the CudaClass adapter do not call them. */
#define LK_NOISE_MAX_FRAMES 16
enum { LK_NOISE_IMAGES = 0, LK_NOISE_RING = 1 };
enum { LK_NOISE_OK = 0, LK_NOISE_TOO_FEW = 1, LK_NOISE_NO_MODEL = 2 };
typedef struct lk_noise_config {        /* 64 bytes */
  int32_t source;                       /* LK_NOISE_IMAGES or LK_NOISE_RING */
  int32_t n_frames;                     /* K */
  int32_t slots[3];                     /* LK_NOISE_IMAGES: the first n_frames are read */
  int32_t first;                        /* LK_NOISE_RING: the first ring slot */
  int32_t x0, y0, x1, y1;               /* region in level-L pixels, inclusive; all 0: the whole frame */
  int32_t grey_low, grey_high;          /* bins outside are left out of the line fit (clipping shrinks their variance) */
  int32_t min_count;                    /* a bin enters the fit with at least this many pixels; >= 2 */
  int32_t reserved[3];                  /* must be 0 */
} lk_noise_config;
struct lk_noise {                       /* 96 bytes */
  int64_t n_pixels;                     /* N */
  double var, var_detrended;            /* squared grey levels */
  double a, b;                          /* var(g) = a + b g */
  int32_t status, n_frames, bins_used;
  float sigma, sigma_detrended, flicker;
  float mean, sigma_at_mean, fit_rms;
  int32_t reserved[5];
};
struct lk_sector_noise {                /* 32 bytes, one per sector */
  int32_t n, status;
  float sigma, mean;
  double var;
  int32_t reserved[2];
};
/* mask: [rows][cols] of the level-L frame, nonzero = use, or NULL.  bins_out: [256][2] int64 or NULL.  frame_sums_out: [K]
 * int64 or NULL.  Synchronous.  Changes no engine state; needs no committed sectors. */
int lk_camera_noise(lk_engine *e, const lk_noise_config *cfg, const uint8_t *mask, struct lk_noise *out, int64_t *bins_out,
                    int64_t *frame_sums_out);
/* out: [S].  sums_out: [S][3] int64 {n, sum q, sum s1} or NULL.  Synchronous.  Changes no engine state. */
int lk_sector_noise(lk_engine *e, const lk_noise_config *cfg, struct lk_sector_noise *out, int64_t *sums_out);
/* host only, no engine: the record of the tables bins [256][2] and frame_sums [n_frames] */
int lk_noise_from_bins(int n_frames, const int64_t *bins, const int64_t *frame_sums, int grey_low, int grey_high, int min_count,
                       struct lk_noise *out);
/* host only, no engine: the record of one sector's three sums */
int lk_noise_from_sums(int n_frames, const int64_t *sums3, struct lk_sector_noise *out);

/* ---- stand-alone pieces (known-answer tests, same kernels as the batch path) ------- */
/* one evaluation of one sector at one level: raw sums A (6x6 row-major, upper valid),
 * b, chi (unscaled), error flag (apply_model_and_interpolate, correlation_class.cpp:131) */
int lk_evaluate(lk_engine *e, int sector, int level, const float *p, float *A36, float *b6,
                float *chi, int *error);
/* value and gradient of image `slot` at pyramid `level` at n arbitrary points
 * (InterpolationClass::get_interpolation, interpolation_class.cpp:79-226), with the
 * engine's interpolation model: out4[k] = {W, dW/dx, dW/dy, out_of_image ? 1 : 0} */
int lk_sample(lk_engine *e, int slot, int level, const float *xy, int n, float *out4);
/* compute_model_parameters + solve (correlation_class.cpp:642-768) on the device.
 * reference_solver = 0: the engine's normal choice (root-free Cholesky, falling back to the
 * reference's pivoted QR when a pivot is small); 1: the pivoted QR always, as the solve
 * kernel does on starved pyramid levels (at most 2P samples); 2: the same QR spread over a
 * 16-lane row, as the finisher of parked sectors runs it (bit-identical to 1) */
int lk_damped_solve(lk_engine *e, int n, const float *A_rowmajor_upper, const float *b,
                    float lambda, float scaling, int reference_solver, float *dp);
/* Known-answer hooks of the fast 32-lane solve instance of the six-parameter models, which leaves the 28 sums of an
 * evaluation spread over the lanes of a 16-lane row and solves from there.
 * lk_step_compare: n systems of 40 floats (28 raw sums: upper triangle row-major, b, chi; lambda; scaling; p[6]; 4 unused).
 * One launch runs the register solver and the scattered one on each; out32 per system: x[6], p[6], flag, 3 unused of the
 * register solver, then x[6], p[6], flag, "all 64 lanes agree" (1 / 0), 2 unused of the scattered one.
 * lk_reduce_compare: n wavefronts of 64 lanes x 28 partial sums; out[n][2][64][28]: every lane's totals by the all-reduce
 * of the 32-lane groups (wide != 0: of the whole wavefront, "solo"), then by the reduce-scatter read back in every lane. */
int lk_step_compare(lk_engine *e, int n, const float *in40, float *out32);
int lk_reduce_compare(lk_engine *e, int n, int wide, const float *lanes, float *out);
/* backward mode's template pass + one evaluation of one sector at one level (lk_set_update), by the lane group its solve
 * uses, whatever the mode: H (6x6 row-major, full), b, chi (all unscaled), error flag (template node or deformed sample
 * out of the image) */
int lk_evaluate_backward(lk_engine *e, int sector, int level, const float *p, float *H36, float *b6, float *chi,
                         int *error);
/* backward mode's parameter update on the host, the kernel's function: p_out = W(p) o W(delta)^-1 (the solve passes
 * delta = -step).  Returns 1 for a singular delta (|det A_delta| < 1e-6; p_out untouched), 0 otherwise,
 * LK_ERROR_BAD_DOMAIN for a bad model or a null pointer.  P = 1, 2, 3, 6 floats per parameter set. */
int lk_compose_inverse(int model, const float *p, const float *delta, float *p_out);

int lk_get_stats(lk_engine *e, lk_stats *out);
/* the same counters per sector of the last solve, registration order:
 * out[s] = {evaluations, sample evaluations, point iterations, ill-conditioned solves} */
int lk_get_sector_stats(lk_engine *e, uint32_t *out_4_per_sector);

/* Which instance of the solve / evaluation kernel a launch ran, as the host decided it (no device word is read). */
typedef enum {
  LK_LAUNCH_MAIN = 0,      /* the lane-group launch of a size class (or of one sector, or of a window) */
  LK_LAUNCH_STARVED = 1,   /* the one-lane kernel of the starved levels, in front of the main launch */
  LK_LAUNCH_FINISHER = 2,  /* the 16-lane finisher of the sectors the one-lane kernel parked */
  LK_LAUNCH_SAFE_PASS = 3, /* the SAFE pass behind a fast launch: 16-lane rows for one pair, the window again for a window */
  LK_LAUNCH_EVAL = 4,      /* the evaluation kernel (lk_evaluate) */
  LK_LAUNCH_BACKWARD = 5,  /* the backward update's lane-group launch: one per non-empty group, in the order 16, 64, 512 */
  LK_LAUNCH_BACKWARD_EVAL = 6 /* the backward evaluation kernel (lk_evaluate_backward): one workgroup of `group` threads */
} lk_launch_role;
typedef enum { LK_FLAVOUR_FAST = 0, LK_FLAVOUR_SAFE = 1, LK_FLAVOUR_REFERENCE = 2 } lk_launch_flavour;
#define LK_LAUNCH_REPORT_CAPACITY 64 /* six classes x four launches, a window's SAFE pass per class, and room to spare */
typedef struct {
  int model;      /* lk_fitting_model of the instance */
  int interp;     /* lk_interpolation of the instance */
  int group;      /* lanes per sector: 1, 16, 32, 64, 256, 512 */
  int threads;    /* threads per workgroup */
  int flavour;    /* lk_launch_flavour */
  int seq;        /* 1: a frame-pipelined (SEQ) instance */
  int role;       /* lk_launch_role */
  int sectors;    /* sectors given to the launch */
  int team_w;     /* workgroups per sector after the launcher's clamp to what is resident (0: no team) */
  int persistent; /* 1: the workgroups draw sectors from the queue */
  int grid;       /* workgroups launched */
  int reserved;
} lk_launch_record;
/* The launches of the engine's most recent solving call - lk_correlate, lk_correlate_all*, lk_correlate_sequence_async
 * (its SAFE re-run included; a window that runs as the one-pair loop reports its last frame), lk_evaluate and
 * lk_evaluate_backward - in the order the host issued them.  A backward solve (lk_set_update) reports one LK_LAUNCH_BACKWARD
 * record per non-empty lane group (flavour SAFE; seq, team_w and persistent 0; threads 256 for 16 and 64 lanes, 512 for 512).
 * out: room for `capacity` records, or NULL to ask for the count alone.  *n_out = records the call made (at most
 * LK_LAUNCH_REPORT_CAPACITY are kept); *overflow = 1 if it made more than are kept.  Host state only: no device call, no
 * synchronisation. */
int lk_get_launch_report(lk_engine *e, lk_launch_record *out, int capacity, int *n_out, int *overflow);
/* Lanes per sector of the next one-pair batch solve (lk_correlate_all*), registration order: groups[s] is the lane group of
 * sector s's size class after promotions and the LK_FORCE_* hooks, or - in reference-order mode - of the batch rule there
 * (a 16-lane row, a wavefront, or a 512-thread workgroup for the big classes).  team_w[s] (may be NULL) is the number of
 * workgroups per sector the engine asks for, before the launcher's clamp to what is resident, and 0 for a sector that gets
 * no team: outside reference-order mode the team class reports 512 lanes and its width (1 under LK_FORCE_TEAM=1: one
 * workgroup); in reference-order mode with T > 1 threads a 512-lane sector of either big class reports T where the batch
 * launches a team of T workgroups, else 0.  Read-only, host state only: no device call, nothing is rebuilt - while a
 * rebuild is pending (sectors appended or moved since the last batch solve) the call fails with LK_ERROR_BAD_DOMAIN. */
int lk_get_sector_groups(lk_engine *e, int *groups, int *team_w);

#ifdef __cplusplus
}
#endif
#endif /* LK_ENGINE_H */
