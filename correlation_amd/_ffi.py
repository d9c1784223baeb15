"""ctypes binding of include/lk_engine.h (the C-ABI shared library liblk_engine.so).

The library is the product; there is no Python or CPU fallback.  Importing this module
raises if the library has not been built (python -m correlation_amd.build).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LK_ENGINE_LIB") or os.path.join(_HERE, "liblk_engine.so")  # (LK_ENGINE_LIB: tuning builds)

LK_MAX_LEVELS = 8

# enums (include/lk_engine.h)
IM_NEAREST, IM_BILINEAR, IM_BICUBIC = 0, 1, 2
IM_BICUBIC_SEPARABLE = 3   # extension: same surface, separable evaluation (include/lk_engine.h)
FM_U, FM_UV, FM_UVQ, FM_UVUXUYVXVY = 0, 1, 2, 3
IMG_UND, IMG_DEF, IMG_NXT = 0, 1, 2
(ERROR_NONE, ERROR_MODEL_OUT_OF_IMAGE, ERROR_INTERPOLATION_OUT_OF_IMAGE,
 ERROR_CORRELATION_MAX_ITERS_REACHED, ERROR_BAD_DOMAIN, ERROR_SOLVER, ERROR_DEVICE,
 ERROR_MULTITHREAD) = range(8)

ERROR_OUTLIER = 8   # extension: set by lk_flag_outliers with mark = 1 (include/lk_engine.h)

N_PARAMS = {FM_U: 1, FM_UV: 2, FM_UVQ: 3, FM_UVUXUYVXVY: 6}
UPDATE_FORWARD, UPDATE_BACKWARD = 0, 1   # lk_set_update (updateEnum, enums.hpp:39)


class LkConfig(C.Structure):
    _fields_ = [("interpolation", C.c_int), ("fitting_model", C.c_int),
                ("precision", C.c_float), ("max_iters", C.c_int),
                ("py_start", C.c_int), ("py_step", C.c_int), ("py_stop", C.c_int),
                ("device", C.c_int)]


class LkStats(C.Structure):
    _fields_ = [("sectors", C.c_uint64), ("evaluations", C.c_uint64),
                ("sample_evaluations", C.c_uint64), ("point_iterations", C.c_uint64),
                ("algorithmic_bytes", C.c_uint64), ("ill_conditioned_solves", C.c_uint64), ("solve_ms", C.c_float),
                ("pyramid_ms", C.c_float), ("window_safe_reruns", C.c_uint64)]


# launch report (include/lk_engine.h: lk_get_launch_report)
(LAUNCH_MAIN, LAUNCH_STARVED, LAUNCH_FINISHER, LAUNCH_SAFE_PASS, LAUNCH_EVAL, LAUNCH_BACKWARD, LAUNCH_BACKWARD_EVAL) = range(7)
FLAVOUR_FAST, FLAVOUR_SAFE, FLAVOUR_REFERENCE = range(3)
LAUNCH_REPORT_CAPACITY = 64


class LkLaunchRecord(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("model", "interp", "group", "threads", "flavour", "seq", "role", "sectors", "team_w",
                                       "persistent", "grid", "reserved")]


# automatic initial guess (include/lk_engine.h: lk_search_guesses)
GS_OK, GS_TEXTURELESS, GS_NO_CANDIDATE, GS_TOO_FEW, GS_TOO_LARGE, GS_WEAK = range(6)
GS_MAX_RADIUS = 32
GS_MAX_SAMPLES = 1 << 22


class LkGuessSearch(C.Structure):
    _fields_ = [("level", C.c_int), ("radius", C.c_int), ("min_samples", C.c_int), ("min_score", C.c_float),
                ("def_slot", C.c_int)]


class LkGuessMatch(C.Structure):
    _fields_ = [("center_x", C.c_int), ("center_y", C.c_int), ("shift_x", C.c_int), ("shift_y", C.c_int),
                ("n_samples", C.c_int), ("n_valid", C.c_int), ("status", C.c_int),
                ("score", C.c_double), ("runner_up", C.c_double)]


# lk_guess_match as a numpy record (same layout as LkGuessMatch)
GUESS_MATCH_DTYPE = np.dtype({"names": [f for f, _ in LkGuessMatch._fields_],
                              "formats": [np.int32] * 7 + [np.float64] * 2,
                              "offsets": [getattr(LkGuessMatch, f).offset for f, _ in LkGuessMatch._fields_],
                              "itemsize": C.sizeof(LkGuessMatch)})

# rotation-aware automatic initial guess (include/lk_engine.h: lk_search_rotated)
RS_MAX_ANGLES = 361


class LkRotatedSearch(C.Structure):
    _fields_ = [("search", LkGuessSearch), ("angle_center", C.c_float), ("angle_step", C.c_float), ("n_half", C.c_int)]


class LkRotatedMatch(C.Structure):
    _fields_ = [("center_x", C.c_int), ("center_y", C.c_int), ("shift_x", C.c_int), ("shift_y", C.c_int),
                ("n_samples", C.c_int), ("n_valid", C.c_int), ("status", C.c_int), ("angle_index", C.c_int),
                ("score", C.c_double), ("runner_up", C.c_double), ("angle_runner_up", C.c_double),
                ("angle", C.c_float), ("angle_refined", C.c_float)]


# lk_rotated_match as a numpy record (same layout as LkRotatedMatch)
ROTATED_MATCH_DTYPE = np.dtype({"names": [f for f, _ in LkRotatedMatch._fields_],
                                "formats": [np.int32] * 8 + [np.float64] * 3 + [np.float32] * 2,
                                "offsets": [getattr(LkRotatedMatch, f).offset for f, _ in LkRotatedMatch._fields_],
                                "itemsize": C.sizeof(LkRotatedMatch)})
assert ROTATED_MATCH_DTYPE.itemsize == 64

# stereo initial guess along the epipolar curve (include/lk_engine.h: lk_search_epipolar)
GS_NO_CURVE, GS_TOO_LONG = 6, 7
EP_MAX_BAND, EP_MAX_NODES, EP_MAX_STATIONS, EP_MAX_GROUP = 8, 33, 2048, 4096


class LkEpipolarSearch(C.Structure):
    _fields_ = [("search", LkGuessSearch), ("n_nodes", C.c_int), ("shape", C.c_int), ("reserved", C.c_int * 3),
                ("z_near", C.c_double), ("z_far", C.c_double), ("normal", C.c_double * 3)]


class LkEpipolarCurve(C.Structure):
    _fields_ = [("axis", C.c_int32), ("first_station", C.c_int32), ("n_stations", C.c_int32), ("first_index", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32 * 3)]


class LkEpipolarMatch(C.Structure):
    _fields_ = [("shift_x", C.c_int32), ("shift_y", C.c_int32), ("station", C.c_int32), ("band_offset", C.c_int32),
                ("node", C.c_int32), ("n_samples", C.c_int32), ("n_valid", C.c_int32), ("status", C.c_int32),
                ("score", C.c_double), ("runner_up", C.c_double), ("station_refined", C.c_float), ("inv_depth", C.c_float),
                ("reserved", C.c_int32 * 2)]


# lk_epipolar_curve and lk_epipolar_match as numpy records (same layouts as the structures)
EPIPOLAR_CURVE_DTYPE = np.dtype([(k, np.int32) for k in ("axis", "first_station", "n_stations", "first_index", "status")] +
                                [("reserved", np.int32, (3,))])
EPIPOLAR_MATCH_DTYPE = np.dtype([(k, np.int32) for k in ("shift_x", "shift_y", "station", "band_offset", "node", "n_samples",
                                                         "n_valid", "status")] +
                                [("score", np.float64), ("runner_up", np.float64), ("station_refined", np.float32),
                                 ("inv_depth", np.float32), ("reserved", np.int32, (2,))])
assert C.sizeof(LkEpipolarSearch) == 80 and LkEpipolarSearch.z_near.offset == 40
assert EPIPOLAR_CURVE_DTYPE.itemsize == C.sizeof(LkEpipolarCurve) == 32
assert EPIPOLAR_MATCH_DTYPE.itemsize == C.sizeof(LkEpipolarMatch) == 64

# recovery pass (include/lk_engine.h: lk_reseed_failed)
RESEED_GOOD, RESEED_RECOVERED, RESEED_NO_NEIGHBOUR, RESEED_NOT_IMPROVED, RESEED_PLANNED = range(5)


class LkReseedConfig(C.Structure):
    _fields_ = [("chi_max", C.c_float), ("radius", C.c_float), ("min_neighbours", C.c_int), ("max_rounds", C.c_int)]


# lk_reseed_info as a numpy record
RESEED_INFO_DTYPE = np.dtype([("status", np.int32), ("round", np.int32), ("neighbours", np.int32),
                              ("chi_before", np.float32)])
assert RESEED_INFO_DTYPE.itemsize == 16

# strain field (include/lk_engine.h: lk_strain_field)
STRAIN_OK, STRAIN_FILLED, STRAIN_TOO_FEW, STRAIN_DEGENERATE = range(4)
STRAIN_GREEN_LAGRANGE, STRAIN_SMALL = 0, 1


class LkStrainConfig(C.Structure):
    _fields_ = [("radius", C.c_float), ("chi_max", C.c_float), ("min_neighbours", C.c_int), ("tensor", C.c_int)]


# lk_strain as a numpy record
STRAIN_DTYPE = np.dtype([(k, np.float32) for k in ("u", "v", "ux", "uy", "vx", "vy", "exx", "eyy", "exy", "e1", "e2", "theta",
                                                   "residual")] +
                        [("neighbours", np.int32), ("status", np.int32), ("reserved", np.int32)])
assert STRAIN_DTYPE.itemsize == 64

# per-sector uncertainty (include/lk_engine.h: lk_parameter_uncertainty)
UNC_OK, UNC_BAD_RECORD, UNC_OUT_OF_IMAGE, UNC_TOO_FEW, UNC_SINGULAR = range(5)
UNC_SUMS = 28   # doubles per sector: A (upper triangle, row-major), b, chi, zeros


class LkUncertaintyConfig(C.Structure):
    _fields_ = [("def_slot", C.c_int), ("reserved", C.c_int)]


# lk_uncertainty as a numpy record
UNCERTAINTY_DTYPE = np.dtype([("sigma", np.float32, (6,))] +
                             [(k, np.float32) for k in ("noise", "rho_uv", "sigma_major", "sigma_minor", "theta", "sssig_x",
                                                        "sssig_y")] +
                             [("n_points", np.int32), ("status", np.int32), ("reserved", np.int32)])
assert UNCERTAINTY_DTYPE.itemsize == 64

# outlier flags (include/lk_engine.h: lk_flag_outliers)
OUTLIER_OK, OUTLIER_FLAGGED, OUTLIER_TOO_FEW, OUTLIER_DEGENERATE, OUTLIER_NOT_GOOD = range(5)


class LkOutlierConfig(C.Structure):
    _fields_ = [("radius", C.c_float), ("chi_max", C.c_float), ("eps", C.c_float), ("threshold", C.c_float),
                ("min_neighbours", C.c_int), ("detrend", C.c_int), ("passes", C.c_int), ("mark", C.c_int)]


# lk_outlier as a numpy record
OUTLIER_DTYPE = np.dtype([(k, np.float32) for k in ("med_u", "med_v", "mad_u", "mad_v", "ratio_u", "ratio_v")] +
                         [("neighbours", np.int32), ("status", np.int32)])
assert OUTLIER_DTYPE.itemsize == 32

# material-point tracks (include/lk_engine.h: lk_track_points)
TRACK_OK, TRACK_TOO_FEW, TRACK_DEGENERATE, TRACK_LOST, TRACK_BAD_POINT = range(5)
TRACK_TOTAL, TRACK_INCREMENTAL = 0, 1
TRACK_RECORDS_CALLER, TRACK_RECORDS_ENGINE, TRACK_RECORDS_WINDOW = range(3)


class LkTrackConfig(C.Structure):
    _fields_ = [("radius", C.c_float), ("chi_max", C.c_float), ("min_neighbours", C.c_int), ("tensor", C.c_int),
                ("mode", C.c_int), ("source", C.c_int)]


# lk_track as a numpy record
TRACK_DTYPE = np.dtype([(k, np.float32) for k in ("x", "y", "u", "v", "ux", "uy", "vx", "vy", "exx", "eyy", "exy", "e1", "e2",
                                                  "theta")] +
                       [("neighbours", np.int32), ("status", np.int32)])
assert TRACK_DTYPE.itemsize == 64

# global motion per frame (include/lk_engine.h: lk_rigid_motion)
MOTION_TRANSLATION, MOTION_RIGID, MOTION_SIMILARITY, MOTION_AFFINE = range(4)
MOTION_OK, MOTION_TOO_FEW, MOTION_DEGENERATE = range(3)
MOTION_MIN_SECTORS = {MOTION_TRANSLATION: 1, MOTION_RIGID: 2, MOTION_SIMILARITY: 2, MOTION_AFFINE: 3}


class LkMotionConfig(C.Structure):
    _fields_ = [("kind", C.c_int), ("source", C.c_int), ("chi_max", C.c_float), ("reject", C.c_float), ("passes", C.c_int),
                ("min_sectors", C.c_int), ("reserved", C.c_int * 2)]


# lk_motion as a numpy record
MOTION_DTYPE = np.dtype([(k, np.float32) for k in ("cx", "cy", "tx", "ty", "axx", "axy", "ayx", "ayy", "theta", "scale", "rms",
                                                   "max_residual")] +
                        [(k, np.int32) for k in ("n_fit", "n_rejected", "status", "passes_run")])
assert MOTION_DTYPE.itemsize == 64 and C.sizeof(LkMotionConfig) == 32

# lens distortion (include/lk_engine.h: lk_lens_fit, lk_lens_correct)
LENS_TRANSLATION, LENS_SIMILARITY, LENS_AFFINE = range(3)
LENS_FREE_K1, LENS_FREE_K2, LENS_FREE_P1, LENS_FREE_P2, LENS_FREE_CENTRE = 1, 2, 4, 8, 16
LENS_OK, LENS_MAX_ITERS, LENS_DEGENERATE = range(3)
LENS_FRAME_OK, LENS_FRAME_TOO_FEW = range(2)
LENS_Q = {LENS_TRANSLATION: 2, LENS_SIMILARITY: 4, LENS_AFFINE: 6}
LENS_CORRECTED, LENS_NOT_GOOD, LENS_OUTSIDE = range(3)   # status of a record of lk_lens_correct


def lens_sums_len(nuisance):
    """doubles of a frame's sums: {n, the upper triangle of the W x W products (W = 7 + Q), n_outside}"""
    w = 7 + LENS_Q[int(nuisance)]
    return w * (w + 1) // 2 + 2


class LkLensConfig(C.Structure):
    _fields_ = [("source", C.c_int), ("chi_max", C.c_float), ("reserved", C.c_int * 2)]


class LkLensFitConfig(C.Structure):
    _fields_ = [("source", C.c_int), ("chi_max", C.c_float), ("min_sectors", C.c_int), ("free", C.c_uint), ("nuisance", C.c_int),
                ("max_iters", C.c_int), ("tol", C.c_double), ("reserved", C.c_int * 2)]


# lk_lens, lk_lens_result, lk_lens_frame and lk_lens_step as numpy records
LENS_DTYPE = np.dtype([(k, np.float64) for k in ("cx", "cy", "rn", "k1", "k2", "p1", "p2", "reserved")])
LENS_PARAMS = ("k1", "k2", "p1", "p2", "cx", "cy")   # the order of sigma, delta and the lens columns of a row
LENS_RESULT_DTYPE = np.dtype([("lens", LENS_DTYPE), ("sigma", np.float64, 6), ("rms_before", np.float64), ("rms", np.float64),
                              ("last_step", np.float64)] +
                             [(k, np.int32) for k in ("status", "iterations", "n_records", "n_frames_used", "n_outside", "reserved")])
LENS_FRAME_DTYPE = np.dtype([("nuisance", np.float64, 6), ("rms", np.float64), ("n", np.int32), ("status", np.int32)])
LENS_STEP_DTYPE = np.dtype([("delta", np.float64, 6), ("sigma", np.float64, 6), ("chi2", np.float64), ("chi2_profiled", np.float64),
                            ("scaled_step", np.float64)] +
                           [(k, np.int32) for k in ("status", "n_records", "n_frames_used", "n_outside")])
assert LENS_DTYPE.itemsize == 64 and LENS_RESULT_DTYPE.itemsize == 160 and LENS_FRAME_DTYPE.itemsize == 64
assert LENS_STEP_DTYPE.itemsize == 136 and C.sizeof(LkLensConfig) == 16 and C.sizeof(LkLensFitConfig) == 40

# a two-camera rig (include/lk_engine.h: lk_stereo_points, lk_stereo_strain)
STEREO_OK, STEREO_BAD_RECORD, STEREO_OUTSIDE_LENS, STEREO_PARALLEL, STEREO_BEHIND = range(5)
STEREO_SURFACE_OK, STEREO_SURFACE_FILLED, STEREO_SURFACE_TOO_FEW, STEREO_SURFACE_DEGENERATE = range(4)
STEREO_SUMS = 23   # Sx, Sy, Sxx, Sxy, Syy, then Sf, Sxf, Syf of X, Y, Z, U, V, W


class LkStereoConfig(C.Structure):
    _fields_ = [("radius", C.c_float), ("chi_max", C.c_float), ("min_neighbours", C.c_int), ("reserved", C.c_int)]


# lk_camera, lk_stereo_point and lk_stereo_surface as numpy records
CAMERA_DTYPE = np.dtype([(k, np.float64) for k in ("fx", "fy", "cx", "cy", "skew")] +
                        [("R", np.float64, (3, 3)), ("t", np.float64, 3), ("lens", LENS_DTYPE), ("reserved", np.float64, 7)])
STEREO_POINT_DTYPE = np.dtype([("X", np.float64), ("Y", np.float64), ("Z", np.float64), ("residual", np.float32, 4),
                               ("epipolar", np.float32), ("angle", np.float32), ("status", np.int32), ("reserved", np.int32, 3)])
STEREO_SURFACE_FLOATS = ("X", "Y", "Z", "U", "V", "W", "nx", "ny", "nz", "exx", "eyy", "exy", "e1", "e2", "theta", "biot1", "biot2",
                         "normal", "residual")
STEREO_SURFACE_DTYPE = np.dtype([(k, np.float32) for k in STEREO_SURFACE_FLOATS] +
                                [("neighbours", np.int32), ("status", np.int32), ("reserved", np.int32, 11)])
assert CAMERA_DTYPE.itemsize == 256 and STEREO_POINT_DTYPE.itemsize == 64 and STEREO_SURFACE_DTYPE.itemsize == 128
assert C.sizeof(LkStereoConfig) == 16

# photometry and the residual map (include/lk_engine.h: lk_photometry, lk_residual_map)
PHOTO_OK, PHOTO_BAD_RECORD, PHOTO_OUT_OF_IMAGE, PHOTO_TOO_FEW, PHOTO_FLAT = range(5)
PHOTO_SUMS = 8   # doubles per sector: sum f, sum g, sum f^2, sum g^2, sum f g, sum V^2, flagged samples, max |V|
MAP_NO_OWNER = -1   # owner map: no good sector within the radius; -2 - s: sector s owns the pixel, the sampler flagged it


class LkPhotometryConfig(C.Structure):
    _fields_ = [("def_slot", C.c_int), ("chi_max", C.c_float), ("reserved", C.c_int * 2)]


class LkResidualMapConfig(C.Structure):
    _fields_ = [("def_slot", C.c_int), ("chi_max", C.c_float), ("radius", C.c_float), ("x0", C.c_int), ("y0", C.c_int),
                ("w", C.c_int), ("h", C.c_int), ("reserved", C.c_int)]


# struct lk_photometry as a numpy record
PHOTOMETRY_DTYPE = np.dtype([("n_points", np.int32), ("status", np.int32)] +
                            [(k, np.float32) for k in ("mean_f", "mean_g", "std_f", "std_g", "zncc", "gain", "offset", "rms",
                                                       "rms_zn", "znssd", "max_abs")] +
                            [("reserved", np.int32, (3,))])
assert PHOTOMETRY_DTYPE.itemsize == 64 and C.sizeof(LkPhotometryConfig) == 16 and C.sizeof(LkResidualMapConfig) == 32

# ZNSSD refinement (include/lk_engine.h: lk_refine_znssd)
(ZN_CONVERGED, ZN_MAX_ITERS, ZN_STALLED, ZN_BAD_SEED, ZN_OUT_OF_IMAGE, ZN_TOO_FEW, ZN_FLAT, ZN_NEGATIVE,
 ZN_SINGULAR) = range(9)
ZN_SUMS = 45   # doubles per sector: Sf, Sg, Sff, Sgg, Sfg, SH[P], SHH[P (P + 1) / 2], SHf[P], SHg[P], flagged samples, zeros
# what the configurations and the info records of the five refinement passes share: the head; the counts, the criterion, the weights
_REFINE_HEAD = [("def_slot", C.c_int), ("chi_max", C.c_float), ("max_iters", C.c_int), ("precision", C.c_float), ("lambda0", C.c_float)]
_ZN_COUNTS = [(k, np.int32) for k in ("n_points", "status", "iterations", "evaluations")]
_ZN_FLOATS = [(k, np.float32) for k in ("zncc", "gain", "offset", "znssd", "zncc_seed", "shift", "lambda", "last_step")]
_ZN_WEIGHTS = [("n_valid", np.int32)] + [(k, np.float32) for k in ("weight_sum", "n_eff", "centroid_dx", "centroid_dy")]


class LkZnssdConfig(C.Structure):
    _fields_ = _REFINE_HEAD + [("reserved", C.c_int * 3)]


# struct lk_znssd as a numpy record
ZNSSD_DTYPE = np.dtype(_ZN_COUNTS + _ZN_FLOATS + [("reserved", np.int32, (4,))])
assert ZNSSD_DTYPE.itemsize == 64 and C.sizeof(LkZnssdConfig) == 32

# second-order refinement (include/lk_engine.h: lk_refine_quadratic); the statuses are ZN_*
QD_SUMS = 88   # doubles per sector: Sf, Sg, Sff, Sgg, Sfg, 3 x 15 moments of gx gx, gx gy, gy gy, 12 sums t, t f, t g, 0, flagged
QD_PARAMS = 12


class LkQuadraticConfig(C.Structure):
    _fields_ = _REFINE_HEAD + [("reserved", C.c_int * 3)]


# struct lk_quadratic as a numpy record
QUADRATIC_DTYPE = np.dtype(_ZN_COUNTS + [("p", np.float32, (12,))] + _ZN_FLOATS + [("bend", np.float32), ("reserved", np.int32, (7,))])
assert QUADRATIC_DTYPE.itemsize == 128 and C.sizeof(LkQuadraticConfig) == 32

# B-spline refinement (include/lk_engine.h: lk_refine_spline); statuses ZN_*, info ZNSSD_DTYPE, sums ZN_SUMS
class LkSplineConfig(C.Structure):
    _fields_ = _REFINE_HEAD + [("order", C.c_int), ("reserved", C.c_int * 2)]


assert C.sizeof(LkSplineConfig) == 32

# weighted refinement (include/lk_engine.h: lk_refine_weighted); statuses ZN_*, sums ZN_SUMS
LOG2E = 1.4426950408889634   # log2(e): inv = float32(LOG2E / (2 sigma_L^2)) is the window's scale


class LkWeightedConfig(C.Structure):
    _fields_ = _REFINE_HEAD + [("sigma", C.c_float), ("min_fraction", C.c_float), ("mask_rows", C.c_int), ("mask_cols", C.c_int),
                               ("reserved", C.c_int * 3)]


# struct lk_weighted as a numpy record: ZNSSD_DTYPE's first 48 bytes, then the weights'
WEIGHTED_DTYPE = np.dtype(_ZN_COUNTS + _ZN_FLOATS + _ZN_WEIGHTS + [("reserved", np.int32, (3,))])
assert WEIGHTED_DTYPE.itemsize == 80 and C.sizeof(LkWeightedConfig) == 48


# composed refinement (include/lk_engine.h: lk_refine_composed); statuses ZN_*, sums ZN_SUMS (order 1) or QD_SUMS (order 2)
class LkComposedConfig(C.Structure):
    _fields_ = _REFINE_HEAD + [("order", C.c_int), ("sampler", C.c_int), ("sigma", C.c_float), ("min_fraction", C.c_float),
                               ("mask_rows", C.c_int), ("mask_cols", C.c_int), ("reserved", C.c_int * 5)]


# struct lk_composed as a numpy record: QUADRATIC_DTYPE up to bend, then WEIGHTED_DTYPE's words of the weights
COMPOSED_DTYPE = np.dtype(_ZN_COUNTS + [("p", np.float32, (12,))] + _ZN_FLOATS + [("bend", np.float32)] + _ZN_WEIGHTS +
                          [("reserved", np.int32, (2,))])
assert COMPOSED_DTYPE.itemsize == 128 and C.sizeof(LkComposedConfig) == 64

# speckle quality (include/lk_engine.h: lk_pattern_quality, lk_suggest_subset)
PATTERN_OK, PATTERN_TOO_FEW, PATTERN_FLAT, PATTERN_APERTURE, PATTERN_SATURATED = range(5)
SUBSET_OK, SUBSET_NONE, SUBSET_BAD_POINT = range(3)
PATTERN_SUMS = 9       # int64 per sector: sum I, sum I^2, Gxx, Gyy, Gxy, n_low, n_high, min I, max I
PATTERN_MAX_HALF = 128


class LkPatternConfig(C.Structure):
    _fields_ = [("slot", C.c_int), ("grey_low", C.c_int), ("grey_high", C.c_int), ("noise_sigma", C.c_float),
                ("max_saturated", C.c_float), ("reserved", C.c_int * 3)]


class LkSubsetConfig(C.Structure):
    _fields_ = [("slot", C.c_int), ("half_min", C.c_int), ("half_max", C.c_int), ("half_step", C.c_int),
                ("sssig_min", C.c_float), ("noise_sigma", C.c_float), ("reserved", C.c_int * 2)]


# struct lk_pattern and struct lk_subset as numpy records
PATTERN_DTYPE = np.dtype([("n_points", np.int32), ("status", np.int32), ("mean", np.float32), ("std", np.float32),
                          ("grey_min", np.int32), ("grey_max", np.int32)] +
                         [(k, np.float32) for k in ("frac_low", "frac_high", "sssig_x", "sssig_y", "mig", "sigma_u", "sigma_v",
                                                    "sigma_major", "theta")] +
                         [("reserved", np.int32)])
SUBSET_DTYPE = np.dtype([(k, np.int32) for k in ("half", "status", "n_pixels", "clipped")] +
                        [(k, np.float32) for k in ("sssig_x", "sssig_y", "sigma_u", "sigma_v")])
assert PATTERN_DTYPE.itemsize == 64 and SUBSET_DTYPE.itemsize == 32
assert C.sizeof(LkPatternConfig) == 32 and C.sizeof(LkSubsetConfig) == 32

# camera noise (include/lk_engine.h: lk_camera_noise, lk_sector_noise)
NOISE_IMAGES, NOISE_RING = 0, 1
NOISE_OK, NOISE_TOO_FEW, NOISE_NO_MODEL = range(3)
NOISE_MAX_FRAMES = 16
NOISE_BINS = 256       # int64 pairs {count, sum q}
NOISE_SUMS = 3         # int64 per sector: n, sum q, sum s1


class LkNoiseConfig(C.Structure):
    _fields_ = [("source", C.c_int32), ("n_frames", C.c_int32), ("slots", C.c_int32 * 3), ("first", C.c_int32),
                ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
                ("grey_low", C.c_int32), ("grey_high", C.c_int32), ("min_count", C.c_int32), ("reserved", C.c_int32 * 3)]


# struct lk_noise and struct lk_sector_noise as numpy records
NOISE_DTYPE = np.dtype([("n_pixels", np.int64)] + [(k, np.float64) for k in ("var", "var_detrended", "a", "b")] +
                       [(k, np.int32) for k in ("status", "n_frames", "bins_used")] +
                       [(k, np.float32) for k in ("sigma", "sigma_detrended", "flicker", "mean", "sigma_at_mean", "fit_rms")] +
                       [("reserved", np.int32, (5,))])
SECTOR_NOISE_DTYPE = np.dtype([("n", np.int32), ("status", np.int32), ("sigma", np.float32), ("mean", np.float32),
                               ("var", np.float64), ("reserved", np.int32, (2,))])
assert NOISE_DTYPE.itemsize == 96 and SECTOR_NOISE_DTYPE.itemsize == 32 and C.sizeof(LkNoiseConfig) == 64

# field map (include/lk_engine.h: lk_field_map)
FIELD_OK, FIELD_TOO_FEW, FIELD_DEGENERATE = range(3)
FIELD_UNIFORM, FIELD_BISQUARE = 0, 1
FIELD_REFERENCE, FIELD_DEFORMED = 0, 1
FIELD_CHANNELS = ("u", "v", "ux", "uy", "vx", "vy", "exx", "eyy", "exy", "e1", "e2", "theta", "x0", "y0", "misfit")
(FIELD_U, FIELD_V, FIELD_UX, FIELD_UY, FIELD_VX, FIELD_VY, FIELD_EXX, FIELD_EYY, FIELD_EXY, FIELD_E1, FIELD_E2, FIELD_THETA,
 FIELD_X0, FIELD_Y0, FIELD_MISFIT) = (1 << i for i in range(15))
FIELD_ALL = (1 << 15) - 1


class LkFieldMapConfig(C.Structure):
    _fields_ = [("radius", C.c_float), ("chi_max", C.c_float), ("min_neighbours", C.c_int), ("tensor", C.c_int),
                ("weight", C.c_int), ("frame", C.c_int), ("iterations", C.c_int), ("x0", C.c_int), ("y0", C.c_int),
                ("nx", C.c_int), ("ny", C.c_int), ("stride", C.c_int), ("channels", C.c_uint32), ("reserved", C.c_int * 3)]


assert C.sizeof(LkFieldMapConfig) == 64

# layout of lk_result == CorrelationResult (domains.hpp:110-118), 48 bytes
RESULT_DTYPE = np.dtype([("p", np.float32, (6,)), ("chi", np.float32),
                         ("n_points", np.int32), ("iterations", np.int32),
                         ("error_code", np.int32), ("und_cx", np.float32),
                         ("und_cy", np.float32)])
assert RESULT_DTYPE.itemsize == 48

# every symbol include/lk_engine.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int)
SYMBOLS = {
    "lk_device_count": (C.c_int, []),
    "lk_create": (C.c_int, [C.POINTER(LkConfig), C.POINTER(_P)]),
    "lk_destroy": (None, [_P]),
    "lk_last_error_string": (C.c_char_p, [_P]),
    "lk_set_stream": (C.c_int, [_P, _P]),
    "lk_set_timing": (C.c_int, [_P, C.c_int]),
    "lk_set_batch_invariant": (C.c_int, [_P, C.c_int]),
    "lk_set_reference_order": (C.c_int, [_P, C.c_int]),
    "lk_set_update": (C.c_int, [_P, C.c_int]),
    "lk_set_pairs_in_flight": (C.c_int, [_P, C.c_int]),
    "lk_synchronize": (C.c_int, [_P]),
    "lk_set_image": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "lk_pin_host_memory": (C.c_int, [_P, C.c_size_t]),
    "lk_unpin_host_memory": (C.c_int, [_P]),
    "lk_set_image_device": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "lk_set_image_pair_device": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "lk_rotate_und_from_def": (C.c_int, [_P]),
    "lk_rotate_def_from_nxt": (C.c_int, [_P]),
    "lk_get_pyramid_level": (C.c_int, [_P, C.c_int, C.c_int, _P, _I, _I]),
    "lk_clear_sectors": (C.c_int, [_P]),
    "lk_set_sector_rect": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "lk_set_rect_grid": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                   C.c_int, C.c_int, C.c_int]),
    "lk_set_sector_annular": (C.c_int, [_P, C.c_int, C.c_float, C.c_float, C.c_float,
                                        C.c_float, C.c_float, C.c_float, C.c_int]),
    "lk_set_sectors_annular": (C.c_int, [_P, C.c_int, C.c_int, _F, C.c_int]),
    "lk_set_sector_blob": (C.c_int, [_P, C.c_int, _F, C.c_int]),
    "lk_set_sector_points": (C.c_int, [_P, C.c_int, _F, C.c_int, C.c_int, C.c_float, C.c_float]),
    "lk_commit_sectors": (C.c_int, [_P]),
    "lk_translate_sectors": (C.c_int, [_P, _F, _F]),
    "lk_rewarp_sectors": (C.c_int, [_P, _F]),
    "lk_restore_sectors": (C.c_int, [_P, C.c_int]),
    "lk_update_sector": (C.c_int, [_P, C.c_int, C.c_int]),
    "lk_get_last_evaluated_parameters": (C.c_int, [_P, _F]),
    "lk_sector_count": (C.c_int, [_P]),
    "lk_get_sector_info": (C.c_int, [_P, C.c_int, _I, _F, _F]),
    "lk_get_sector_level_count": (C.c_int, [_P, C.c_int, C.c_int, _I]),
    "lk_get_und_xy": (C.c_int, [_P, C.c_int, _F, C.c_int, _I]),
    "lk_get_level_xy": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _F, C.c_int, _I]),
    "lk_get_def_xy": (C.c_int, [_P, C.c_int, _F, _F, C.c_int, _I]),
    "lk_correlate": (C.c_int, [_P, C.c_int, _F, _P]),
    "lk_correlate_all": (C.c_int, [_P, _F, _P]),
    "lk_correlate_all_device": (C.c_int, [_P, _P, _P]),
    "lk_get_results_device": (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    "lk_correlate_all_async": (C.c_int, [_P]),
    "lk_wait_results": (C.c_int, [_P, _P]),
    "lk_sequence_reserve": (C.c_int, [_P, C.c_int]),
    "lk_sequence_set_frame": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "lk_sequence_set_frame_device": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "lk_correlate_sequence_async": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "lk_wait_sequence": (C.c_int, [_P, _P]),
    "lk_get_sequence_results_device": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "lk_sequence_is_pipelined": (C.c_int, [_P]),
    "lk_sequence_host_records": (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    "lk_sequence_prepare_host_records": (C.c_int, [_P, C.c_int]),
    "lk_copy_sequence_records_device": (C.c_int, [_P, _P, C.c_size_t]),
    "lk_get_sequence_guesses": (C.c_int, [_P, _F]),
    "lk_adjust_initial_guess": (C.c_int, [_P, C.c_int, C.c_int, _F, C.c_float, C.c_float]),
    "lk_get_guesses": (C.c_int, [_P, _F]),
    "lk_search_guesses": (C.c_int, [_P, C.POINTER(LkGuessSearch), _F]),
    "lk_get_guess_search_info": (C.c_int, [_P, _P]),
    "lk_search_rotated": (C.c_int, [_P, C.POINTER(LkRotatedSearch), _F]),
    "lk_get_rotated_search_info": (C.c_int, [_P, _P]),
    "lk_get_rotated_search_profile": (C.c_int, [_P, _P]),
    "lk_search_epipolar": (C.c_int, [_P, C.POINTER(LkEpipolarSearch), _P, _P, _F]),
    "lk_get_epipolar_search_info": (C.c_int, [_P, _P]),
    "lk_get_epipolar_search_profile": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int)]),
    "lk_epipolar_curves": (C.c_int, [C.POINTER(LkEpipolarSearch), _P, C.c_int, _F, _P, C.c_int, _P, C.POINTER(C.c_int), C.c_int,
                                     _P, _P, _P, _P]),
    "lk_rotation_table": (C.c_int, [C.POINTER(LkRotatedSearch), _F]),
    "lk_reseed_failed": (C.c_int, [_P, C.POINTER(LkReseedConfig), _P, _I]),
    "lk_get_reseed_info": (C.c_int, [_P, _P]),
    "lk_reseed_plan": (C.c_int, [_P, C.POINTER(LkReseedConfig), _P, _F, _P]),
    "lk_strain_field": (C.c_int, [_P, C.POINTER(LkStrainConfig), _P, _P]),
    "lk_strain_from_gradient": (C.c_int, [C.c_int, _F, _F]),
    "lk_parameter_uncertainty": (C.c_int, [_P, C.POINTER(LkUncertaintyConfig), _P, _P, _P]),
    "lk_uncertainty_from_sums": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, _P]),
    "lk_flag_outliers": (C.c_int, [_P, C.POINTER(LkOutlierConfig), _P, _P, _P, _I]),
    "lk_outlier_from_window": (C.c_int, [C.c_int, _F, _F, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "lk_track_points": (C.c_int, [_P, C.POINTER(LkTrackConfig), C.c_int, _F, C.c_int, _P, _P, _P]),
    "lk_track_step": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P]),
    "lk_gauges_from_tracks": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, _P, _F]),
    "lk_rigid_motion": (C.c_int, [_P, C.POINTER(LkMotionConfig), C.c_int, _P, _P, _P, _P, _P]),
    "lk_motion_from_sums": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "lk_motion_apply": (C.c_int, [_P, C.c_int, _F, _F]),
    "lk_motion_remove": (C.c_int, [C.c_int, _P, C.c_float, C.c_float, _P, _P]),
    "lk_lens_distort": (C.c_int, [_P, C.c_int, _P, _P]),
    "lk_lens_undistort": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "lk_lens_correct_record": (C.c_int, [C.c_int, _P, C.c_float, C.c_float, _P, _P, C.POINTER(C.c_int)]),
    "lk_lens_step_from_sums": (C.c_int, [C.c_int, C.c_uint, C.c_double, C.c_int, C.c_int, _P, _P, _P]),
    "lk_lens_correct": (C.c_int, [_P, C.POINTER(LkLensConfig), _P, C.c_int, _P, _P, _P, _P]),
    "lk_lens_fit": (C.c_int, [_P, C.POINTER(LkLensFitConfig), _P, C.c_int, _P, _P, _P, _P, _P]),
    "lk_stereo_project": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "lk_stereo_fundamental": (C.c_int, [_P, _P]),
    "lk_stereo_triangulate": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "lk_stereo_surface_from_sums": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_double, _P, _P]),
    "lk_stereo_points": (C.c_int, [_P, C.POINTER(LkStereoConfig), _P, _P, C.c_int, _P, _P, _P, _P]),
    "lk_stereo_strain": (C.c_int, [_P, C.POINTER(LkStereoConfig), C.c_int, _P, _P, _P]),
    "lk_photometry": (C.c_int, [_P, C.POINTER(LkPhotometryConfig), _P, _P, _P]),
    "lk_photometry_from_sums": (C.c_int, [C.c_int, _P, _P]),
    "lk_residual_map": (C.c_int, [_P, C.POINTER(LkResidualMapConfig), _P, _P, _P, _P]),
    "lk_map_owner": (C.c_int, [C.c_int, _F, _P, C.c_double, C.c_double, C.c_double]),
    "lk_refine_znssd": (C.c_int, [_P, C.POINTER(LkZnssdConfig), _P, _F, _P, _P, _P]),
    "lk_znssd_step_from_sums": (C.c_int, [C.c_int, C.c_int, _P, C.c_float, _P, _P, _P, _P]),
    "lk_refine_quadratic": (C.c_int, [_P, C.POINTER(LkQuadraticConfig), _P, _F, _F, _P, _P, _P]),
    "lk_refine_spline": (C.c_int, [_P, C.POINTER(LkSplineConfig), _P, _F, _P, _P, _P]),
    "lk_spline_coefficients": (C.c_int, [_P, C.c_int, C.c_int, _F]),
    "lk_spline_sample": (C.c_int, [_P, C.c_int, C.c_int, _F, C.c_int, _F]),
    "lk_spline_weights": (C.c_int, [C.c_int, C.c_float, _F, _F]),
    "lk_quadratic_step_from_sums": (C.c_int, [C.c_int, _P, C.c_float, _P, _P, _P, _P]),
    "lk_refine_weighted": (C.c_int, [_P, C.POINTER(LkWeightedConfig), _P, _P, _F, _P, _P, _P]),
    "lk_weight_window": (C.c_int, [C.c_float, C.c_float, C.c_float, _F]),
    "lk_weighted_step_from_sums": (C.c_int, [C.c_int, C.c_int, C.c_double, _P, C.c_float, _P, _P, _P, _P]),
    "lk_refine_composed": (C.c_int, [_P, C.POINTER(LkComposedConfig), _P, _P, _F, _F, _P, _P, _P]),
    "lk_composed_step_from_sums": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, _P, C.c_float, _P, _P, _P, _P]),
    "lk_field_map": (C.c_int, [_P, C.POINTER(LkFieldMapConfig), _P, _P, _P, _P]),
    "lk_field_from_sums": (C.c_int, [C.c_int, C.c_int, C.c_double, _P, C.c_int, _F, _I]),
    "lk_pattern_quality": (C.c_int, [_P, C.POINTER(LkPatternConfig), _P, _P, _P]),
    "lk_pattern_from_sums": (C.c_int, [C.c_int, _P, C.c_double, C.c_float, C.c_float, _P]),
    "lk_suggest_subset": (C.c_int, [_P, C.POINTER(LkSubsetConfig), C.c_int, _F, _P, _P]),
    "lk_camera_noise": (C.c_int, [_P, C.POINTER(LkNoiseConfig), _P, _P, _P, _P]),
    "lk_sector_noise": (C.c_int, [_P, C.POINTER(LkNoiseConfig), _P, _P]),
    "lk_noise_from_bins": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "lk_noise_from_sums": (C.c_int, [C.c_int, _P, _P]),
    "lk_evaluate": (C.c_int, [_P, C.c_int, C.c_int, _F, _F, _F, _F, _I]),
    "lk_evaluate_backward": (C.c_int, [_P, C.c_int, C.c_int, _F, _F, _F, _F, _I]),
    "lk_compose_inverse": (C.c_int, [C.c_int, _F, _F, _F]),
    "lk_sample": (C.c_int, [_P, C.c_int, C.c_int, _F, C.c_int, _F]),
    "lk_damped_solve": (C.c_int, [_P, C.c_int, _F, _F, C.c_float, C.c_float, C.c_int, _F]),
    "lk_step_compare": (C.c_int, [_P, C.c_int, _F, _F]),
    "lk_reduce_compare": (C.c_int, [_P, C.c_int, C.c_int, _F, _F]),
    "lk_get_stats": (C.c_int, [_P, C.POINTER(LkStats)]),
    "lk_get_sector_stats": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "lk_get_launch_report": (C.c_int, [_P, C.POINTER(LkLaunchRecord), C.c_int, _I, _I]),
    "lk_get_sector_groups": (C.c_int, [_P, _I, _I]),
    # include/lk_tracker.h
    "lk_tracker_create": (C.c_int, [_P, C.POINTER(_P)]),
    "lk_tracker_destroy": (None, [_P]),
    "lk_tracker_last_error": (C.c_char_p, [_P]),
    "lk_tracker_set_rect_domain": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                             C.c_int, C.c_int]),
    "lk_tracker_set_annular_domain": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]),
    "lk_tracker_set_blob_domain": (C.c_int, [_P, _F, C.c_int, C.c_float, C.c_float]),
    "lk_tracker_sector_count": (C.c_int, [_P]),
    "lk_tracker_enable_report": (C.c_int, [_P, C.c_int]),
    "lk_tracker_blob_contour": (C.c_int, [_P, C.POINTER(_F), _I]),
    "lk_tracker_begin_frame": (C.c_int, [_P, C.c_int, _P, _F]),
    "lk_tracker_end_frame": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_char_p, _P, _I, _I]),
    "lk_tracker_get_results": (C.c_int, [_P, _P]),
    "lk_tracker_set_guess_search": (C.c_int, [_P, C.POINTER(LkGuessSearch)]),
    "lk_tracker_override_guesses": (C.c_int, [_P, _F]),
    "lk_tracker_report": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lk_sequence_frame": (C.c_int, [_P, _P, C.c_int, C.c_char_p, C.c_char_p, _I]),
    "lk_sequence_run": (C.c_int, [_P, _P, C.c_int, _P, _P, _I]),
    "lk_roi_rect_grid": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _I, _I, _I]),
    "lk_roi_annular_points": (C.c_int64, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                          _F, C.c_int64]),
    "lk_roi_blob_points": (C.c_int64, [_F, C.c_int, _F, C.c_int64]),
    "lk_roi_decimate": (C.c_int, [_F, C.c_int, C.c_int, _F]),
    # include/lk_group.h
    "lk_group_create": (C.c_int, [C.POINTER(LkConfig), C.c_int, _I, C.POINTER(_P)]),
    "lk_group_destroy": (None, [_P]),
    "lk_group_last_error_string": (C.c_char_p, [_P]),
    "lk_group_size": (C.c_int, [_P]),
    "lk_group_comm_ranks": (C.c_int, [_P]),
    "lk_group_engine": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "lk_group_shard": (C.c_int, [_P, C.c_int, _I, _I]),
    "lk_group_shard_range": (C.c_int, [C.c_int, C.c_int, C.c_int, _I, _I]),
    "lk_group_set_image": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "lk_group_set_image_device": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "lk_group_rotate_und_from_def": (C.c_int, [_P]),
    "lk_group_rotate_def_from_nxt": (C.c_int, [_P]),
    "lk_group_clear_sectors": (C.c_int, [_P]),
    "lk_group_set_sector_rect": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "lk_group_set_rect_grid": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]),
    "lk_group_set_sector_annular": (C.c_int, [_P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                              C.c_float, C.c_int]),
    "lk_group_set_sector_points": (C.c_int, [_P, C.c_int, _F, C.c_int, C.c_int, C.c_float, C.c_float]),
    "lk_group_commit_sectors": (C.c_int, [_P]),
    "lk_group_sector_count": (C.c_int, [_P]),
    "lk_group_correlate_all": (C.c_int, [_P, _F, _P]),
    "lk_group_adjust_initial_guess": (C.c_int, [_P, C.c_int, C.c_int, _F, C.c_float, C.c_float]),
    "lk_group_sequence_reserve": (C.c_int, [_P, C.c_int]),
    "lk_group_sequence_set_frames": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]),
    "lk_group_sequence_set_frames_device": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "lk_group_correlate_sequence_async": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "lk_group_wait_sequence": (C.c_int, [_P, _P]),
    "lk_group_sequence_records": (C.c_int, [_P, _P]),
    "lk_group_sequence_records_device": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "lk_group_probe_overlap": (C.c_int, [_P, C.c_int, _F]),
    "lk_group_records_device": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "lk_group_block_records": (C.c_int, [_P]),
    "lk_group_synchronize": (C.c_int, [_P]),
    "lk_group_get_stats": (C.c_int, [_P, C.POINTER(LkStats)]),
    "lk_load_pgm": (C.c_int, [C.c_char_p, C.POINTER(C.POINTER(C.c_uint8)), _I, _I]),
    "lk_load_image": (C.c_int, [C.c_char_p, C.POINTER(C.POINTER(C.c_uint8)), _I, _I]),
    "lk_decode_image": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint8)), _I, _I]),
    "lk_free_image": (None, [C.POINTER(C.c_uint8)]),
}


def _load_torch_first():
    """PyTorch wheels bundle their own ROCm runtime (libamdhip64, libhsa-runtime64, librccl, libroctx64).
    A process that loads the system copies first (through liblk_engine.so) and torch's copies later has
    two HSA runtimes, and the one that comes second finds no GPU ("No HIP GPUs are available").  With
    torch imported first both resolve to the same copies.  Python harness only: a C/C++ consumer of the
    library links the system ROCm and never meets torch.  LK_NO_TORCH_PRELOAD=1 skips it."""
    if os.environ.get("LK_NO_TORCH_PRELOAD"):
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load_library(path=LIB_PATH):
    _load_torch_first()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP engine is the product and there is no fallback. "
            "Build it with `python -m correlation_amd.build` (hipcc, gfx950).")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


def fptr(a):
    return a.ctypes.data_as(_F)


_compose_lib = None


def compose_inverse(model, p, delta):
    """The backward update's W(p) o W(delta)^-1 (lk_compose_inverse, host, the kernel's function): the new parameter set
    [6] as float32, or None for a singular delta."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    pp = np.zeros(6, np.float32)
    dd = np.zeros(6, np.float32)
    pp[:len(p)] = np.asarray(p, np.float32)[:6]
    dd[:len(delta)] = np.asarray(delta, np.float32)[:6]
    out = np.zeros(6, np.float32)
    rc = _compose_lib.lk_compose_inverse(int(model), fptr(pp), fptr(dd), fptr(out))
    if rc == 1:
        return None
    if rc != 0:
        raise ValueError(f"lk_compose_inverse: bad model {model}")
    return out


def rotation_table(angle_step, n_half, angle_center=0.0):
    """lk_rotation_table (host, the table the kernels of lk_search_rotated read): float32 [2 n_half + 1][2], {cos, sin} of
    theta_k = angle_center + k angle_step, k = -n_half .. n_half."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    cfg = LkRotatedSearch(LkGuessSearch(-1, 0, 0, 0.0, -1), float(angle_center), float(angle_step), int(n_half))
    out = np.zeros((max(2 * int(n_half) + 1, 1), 2), np.float32)
    if _compose_lib.lk_rotation_table(C.byref(cfg), fptr(out)) != 0:
        raise ValueError("lk_rotation_table: bad n_half, angle_step or angle_center")
    return out


def strain_from_gradient(tensor, grad4):
    """lk_strain_from_gradient (host, the kernel's function): {exx, eyy, exy, e1, e2, theta} as float32 [6] of the
    displacement gradient {ux, uy, vx, vy}."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    g = np.ascontiguousarray(grad4, np.float32).reshape(4)
    out = np.zeros(6, np.float32)
    if _compose_lib.lk_strain_from_gradient(int(tensor), fptr(g), fptr(out)) != 0:
        raise ValueError(f"lk_strain_from_gradient: bad tensor {tensor}")
    return out


def uncertainty_from_sums(model, n, sums28, level=0):
    """lk_uncertainty_from_sums (host, the kernel's function): the UNCERTAINTY_DTYPE record of n samples whose 28 sums
    (A upper triangle row-major, b, chi, zeros) were evaluated at pyramid `level`."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.ascontiguousarray(sums28, np.float64).reshape(UNC_SUMS)
    out = np.zeros(1, UNCERTAINTY_DTYPE)
    if _compose_lib.lk_uncertainty_from_sums(int(model), int(n), s.ctypes.data_as(_P), int(level),
                                             out.ctypes.data_as(_P)) != 0:
        raise ValueError(f"lk_uncertainty_from_sums: bad model {model} or level {level}")
    return out[0]


def outlier_from_window(e_u, e_v, es_u, es_v, eps, threshold):
    """lk_outlier_from_window (host, the kernel's selection and ratio arithmetic): the OUTLIER_DTYPE record of a sector
    whose window holds the values e_u, e_v [n] and whose own values are es_u, es_v."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    u = np.ascontiguousarray(e_u, np.float32).reshape(-1)
    v = np.ascontiguousarray(e_v, np.float32).reshape(-1)
    if len(u) != len(v):
        raise ValueError("lk_outlier_from_window: e_u and e_v differ in length")
    out = np.zeros(1, OUTLIER_DTYPE)
    if _compose_lib.lk_outlier_from_window(len(u), fptr(u), fptr(v), float(es_u), float(es_v), float(eps), float(threshold),
                                           out.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_outlier_from_window: an empty window, a value that is not finite, or eps / threshold <= 0")
    return out[0]


def photometry_from_sums(n, sums8):
    """lk_photometry_from_sums (host, the kernel's function): the PHOTOMETRY_DTYPE record of one sector of n samples whose
    eight sums are sums8 (sum f, sum g, sum f^2, sum g^2, sum f g, sum V^2, flagged samples, max |V|)."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.ascontiguousarray(sums8, np.float64).reshape(PHOTO_SUMS)
    out = np.zeros(1, PHOTOMETRY_DTYPE)
    if _compose_lib.lk_photometry_from_sums(int(n), s.ctypes.data_as(_P), out.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_photometry_from_sums: n < 0")
    return out[0]


def _step_from_sums(name, head, sums, n_sums, lam, n_delta, refused):
    """What the four *_step_from_sums wrappers share: lib.name(*head, sums, lam, delta, crit, gain_offset, status), `sums` padded
    with zeros to n_sums doubles; ValueError(name: refused) where the library refuses.  Returns (status, delta, crit, gain, offset)."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.zeros(n_sums, np.float64)
    flat = np.asarray(sums, np.float64).reshape(-1)
    s[:len(flat)] = flat
    delta, crit, go, status = np.zeros(n_delta, np.float64), C.c_double(), np.zeros(2, np.float64), C.c_int32(-1)
    if getattr(_compose_lib, name)(*head, s.ctypes.data_as(_P), float(lam), delta.ctypes.data_as(_P), C.byref(crit),
                                   go.ctypes.data_as(_P), C.byref(status)) != 0:
        raise ValueError(f"{name}: {refused}")
    return status.value, delta, crit.value, float(go[0]), float(go[1])


def znssd_step_from_sums(model, n, sums, lam):
    """lk_znssd_step_from_sums (host, the kernel's function): (status, delta [6], crit, gain, offset) of one sector of n
    samples whose sums, in the model's layout, are `sums` (ZN_SUMS doubles or fewer), at the damping `lam`."""
    return _step_from_sums("lk_znssd_step_from_sums", (int(model), int(n)), sums, ZN_SUMS, lam, 6,
                           f"bad model {model}, n < 0 or a bad lambda")


def quadratic_step_from_sums(n, sums, lam):
    """lk_quadratic_step_from_sums (host, the kernel's function): (status, delta [12], crit, gain, offset) of one sector of n
    samples whose QD_SUMS sums are `sums`, at the damping `lam`."""
    return _step_from_sums("lk_quadratic_step_from_sums", (int(n),), np.asarray(sums, np.float64).reshape(QD_SUMS), QD_SUMS, lam,
                           QD_PARAMS, "n < 0 or a bad lambda")


def spline_weights(order, t):
    """lk_spline_weights (host, the kernel's function): (w, g), the order + 1 float32 weights and derivative weights of the
    B-spline sampler at the fraction t."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    w, g = np.zeros(6, np.float32), np.zeros(6, np.float32)
    if _compose_lib.lk_spline_weights(int(order), float(t), fptr(w), fptr(g)) != 0:
        raise ValueError(f"lk_spline_weights: order {order} is not 3 or 5, or t is not finite")
    n = (int(order) or 5) + 1
    return w[:n], g[:n]


def weight_window(inv, dx, dy):
    """lk_weight_window (host, the kernel's function): the float32 window 2^-(r2 inv) at the offset (dx, dy), inv =
    float32(LOG2E / (2 sigma^2))."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    w = np.zeros(1, np.float32)
    if _compose_lib.lk_weight_window(float(inv), float(dx), float(dy), fptr(w)) != 0:
        raise ValueError(f"lk_weight_window: inv {inv} is negative or not finite, or the offset is not finite")
    return w[0]


def weighted_step_from_sums(model, n_valid, N, sums, lam):
    """lk_weighted_step_from_sums (host, the kernel's function): (status, delta [6], crit, gain, offset) of one sector of
    n_valid samples of total weight N whose weighted sums, in the model's layout, are `sums`, at the damping `lam`."""
    return _step_from_sums("lk_weighted_step_from_sums", (int(model), int(n_valid), float(N)), sums, ZN_SUMS, lam, 6,
                           f"bad model {model}, n_valid < 0, or a bad N or lambda")


def composed_step_from_sums(order, model, n_valid, N, sums, lam):
    """lk_composed_step_from_sums (host, the kernels' function): (status, delta [12], crit, gain, offset) of one sector of
    n_valid samples of total weight N whose weighted sums are `sums` - the model's layout, ZN_SUMS or fewer, with order 1
    (delta: zeros behind P); QD_SUMS with order 2, where the model plays no part - at the damping `lam`."""
    return _step_from_sums("lk_composed_step_from_sums", (int(order), int(model), int(n_valid), float(N)), sums, QD_SUMS, lam,
                           QD_PARAMS, f"bad order {order} or model {model}, n_valid < 0, or a bad N or lambda")


def pattern_from_sums(n, sums9, mig_sum, noise_sigma=1.0, max_saturated=1.0):
    """lk_pattern_from_sums (host, the kernel's function): the PATTERN_DTYPE record of one sector of n samples whose nine
    integer sums are sums9 (sum I, sum I^2, Gxx, Gyy, Gxy, n_low, n_high, min I, max I) and whose gradient-magnitude sum is
    mig_sum."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.ascontiguousarray(sums9, np.int64).reshape(PATTERN_SUMS)
    out = np.zeros(1, PATTERN_DTYPE)
    if _compose_lib.lk_pattern_from_sums(int(n), s.ctypes.data_as(_P), float(mig_sum), float(noise_sigma), float(max_saturated),
                                         out.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_pattern_from_sums: n < 0, or a noise_sigma or max_saturated that is not finite")
    return out[0]


def noise_from_bins(n_frames, bins, frame_sums, grey_low=0, grey_high=255, min_count=2):
    """lk_noise_from_bins (host, no engine): the NOISE_DTYPE record of the tables of K = n_frames static frames - bins
    [256][2] int64 {count, sum q} and frame_sums [K] int64."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    b = np.ascontiguousarray(bins, np.int64).reshape(NOISE_BINS, 2)
    f = np.ascontiguousarray(frame_sums, np.int64).reshape(-1)
    out = np.zeros(1, NOISE_DTYPE)
    if len(f) != int(n_frames) or _compose_lib.lk_noise_from_bins(int(n_frames), b.ctypes.data_as(_P), f.ctypes.data_as(_P), int(grey_low),
                                                                  int(grey_high), int(min_count), out.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_noise_from_bins: n_frames outside 2 .. 16, a negative table entry, greys outside 0 .. 255 or "
                         "min_count < 2")
    return out[0]


def noise_from_sums(n_frames, sums3):
    """lk_noise_from_sums (host, no engine): the SECTOR_NOISE_DTYPE record of one sector's sums {n, sum q, sum s1}."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.ascontiguousarray(sums3, np.int64).reshape(NOISE_SUMS)
    out = np.zeros(1, SECTOR_NOISE_DTYPE)
    if _compose_lib.lk_noise_from_sums(int(n_frames), s.ctypes.data_as(_P), out.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_noise_from_sums: n_frames outside 2 .. 16 or a negative sum")
    return out[0]


def map_owner(centers, X, Y, radius, good=None):
    """lk_map_owner (host, the residual map's owner rule by brute force): the index of the good sector whose centre
    (centers [n][2], level-0 pixels) is nearest to the level-0 position (X, Y) within `radius`, ties to the lowest index;
    -1 without one."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    c = np.ascontiguousarray(centers, np.float32).reshape(-1, 2)
    g = None
    if good is not None:
        g = np.ascontiguousarray(good, np.uint8).reshape(-1)
        if len(g) != len(c):
            raise ValueError("lk_map_owner: good and centers differ in length")
    r = _compose_lib.lk_map_owner(len(c), fptr(c), g.ctypes.data_as(_P) if g is not None else None, float(X), float(Y),
                                  float(radius))
    if r < -1:
        raise ValueError("lk_map_owner: the radius must be finite and positive")
    return r


def track_step(mode, min_neighbours, n, sums11, state8, tensor=STRAIN_GREEN_LAGRANGE):
    """lk_track_step (host, the kernel's per-frame function): the window's count n and 11 sums and the state
    {X, Y, x, y, Fxx, Fxy, Fyx, Fyy} -> (the TRACK_DTYPE record, the new state as float64 [8])."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.ascontiguousarray(sums11, np.float64).reshape(11)
    st = np.array(state8, np.float64).reshape(8)
    out = np.zeros(1, TRACK_DTYPE)
    if _compose_lib.lk_track_step(int(mode), int(min_neighbours), int(n), s.ctypes.data_as(_P), st.ctypes.data_as(_P),
                                  int(tensor), out.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_track_step: n < 0, min_neighbours < 3, or an unknown mode or tensor")
    return out[0], st


def field_from_sums(min_neighbours, n, W, sums11, tensor=STRAIN_GREEN_LAGRANGE):
    """lk_field_from_sums (host, the kernel's fit of one node): the window's count n, weight sum W and 11 weighted sums ->
    (status, float32 [12] = u, v, ux, uy, vx, vy, exx, eyy, exy, e1, e2, theta; all NaN unless the status is FIELD_OK)."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.ascontiguousarray(sums11, np.float64).reshape(11)
    out = np.zeros(12, np.float32)
    status = C.c_int(-1)
    if _compose_lib.lk_field_from_sums(int(min_neighbours), int(n), float(W), s.ctypes.data_as(_P), int(tensor), fptr(out),
                                       C.byref(status)) != 0:
        raise ValueError("lk_field_from_sums: n < 0, min_neighbours < 3 or an unknown tensor")
    return status.value, out


def gauges_from_tracks(tracks, pairs):
    """lk_gauges_from_tracks (host): tracks [F][Q] (TRACK_DTYPE) and pairs [G][2] of point indices -> float32 [F][G][4] =
    length, engineering strain, logarithmic strain, rotation of the segment in radians."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    t = np.ascontiguousarray(tracks, TRACK_DTYPE)
    if t.ndim != 2:
        raise ValueError("lk_gauges_from_tracks: tracks must be [n_frames][n_points]")
    ij = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    out = np.zeros((t.shape[0], len(ij), 4), np.float32)
    if _compose_lib.lk_gauges_from_tracks(t.shape[0], t.shape[1], t.ctypes.data_as(_P), len(ij), ij.ctypes.data_as(_P),
                                          fptr(out)) != 0:
        raise ValueError("lk_gauges_from_tracks: no frames, points or gauges, or a pair index outside the points")
    return out


def motion_from_sums(kind, n, sums11, origin_xy, min_sectors=None):
    """lk_motion_from_sums (host, the kernel's fit): the fit set's count n and 11 sums relative to origin_xy -> the
    MOTION_DTYPE record (rms, max_residual, n_rejected and passes_run are 0: the sums do not hold them)."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.ascontiguousarray(sums11, np.float64).reshape(11)
    o = np.ascontiguousarray(origin_xy, np.float64).reshape(2)
    out = np.zeros(1, MOTION_DTYPE)
    if min_sectors is None:
        min_sectors = MOTION_MIN_SECTORS.get(int(kind), 1)
    if _compose_lib.lk_motion_from_sums(int(kind), int(min_sectors), int(n), s.ctypes.data_as(_P), o.ctypes.data_as(_P),
                                        out.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_motion_from_sums: n < 0, an unknown kind or a min_sectors below the kind's minimum")
    return out[0]


def motion_apply(motion, xy):
    """lk_motion_apply (host): the displacement t + (A - I)(x - c) of one MOTION_DTYPE record at xy [n][2] -> float32 [n][2]."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    m = np.ascontiguousarray(motion, MOTION_DTYPE).reshape(1)
    p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.zeros_like(p)
    if _compose_lib.lk_motion_apply(m.ctypes.data_as(_P), len(p), fptr(p), fptr(out)) != 0:
        raise ValueError("lk_motion_apply: no positions")
    return out


def motion_remove(model, motion, centers, records, good=None):
    """lk_motion_remove (host, the kernel's removal) over one frame: records [S] at centers [S][2] without the MOTION_DTYPE
    record `motion` -> records [S].  good [S]: the records to rewrite (the caller's good rule); None: all of them."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    m = np.ascontiguousarray(motion, MOTION_DTYPE).reshape(1)
    c = np.ascontiguousarray(centers, np.float32).reshape(-1, 2)
    rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(len(c))
    out = rec.copy()
    one = np.zeros(1, RESULT_DTYPE)
    for s in range(len(c)):
        if good is not None and not good[s]:
            continue
        if _compose_lib.lk_motion_remove(int(model), m.ctypes.data_as(_P), float(c[s, 0]), float(c[s, 1]),
                                         rec[s:s + 1].ctypes.data_as(_P), one.ctypes.data_as(_P)) != 0:
            raise ValueError("lk_motion_remove: an unknown model, FM_U with an A that is not the identity, or an A without an inverse")
        out[s] = one[0]
    return out


def make_lens(cx, cy, rn, k1=0.0, k2=0.0, p1=0.0, p2=0.0):
    """one LENS_DTYPE record"""
    lens = np.zeros(1, LENS_DTYPE)
    lens[0] = (cx, cy, rn, k1, k2, p1, p2, 0.0)
    return lens[0]


def _lens_points(lens, xy):
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    one = np.ascontiguousarray(lens, LENS_DTYPE).reshape(1)
    p = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    return one, p, np.zeros_like(p)


def lens_distort(lens, xy):
    """lk_lens_distort (host, the kernel's model): undistorted positions xy [n][2] -> where the camera shows them, float64."""
    one, p, out = _lens_points(lens, xy)
    if _compose_lib.lk_lens_distort(one.ctypes.data_as(_P), len(p), p.ctypes.data_as(_P), out.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_lens_distort: no positions, or a lens that is not finite, has rn <= 0 or a reserved word")
    return out


def lens_undistort(lens, xy, return_status=False):
    """lk_lens_undistort (host, the kernel's Newton iteration): distorted positions xy [n][2] -> float64 [n][2]; with
    return_status also uint8 [n]: 0, or LENS_OUTSIDE for a position outside the model's domain (copied)."""
    one, p, out = _lens_points(lens, xy)
    status = np.zeros(len(p), np.uint8)
    if _compose_lib.lk_lens_undistort(one.ctypes.data_as(_P), len(p), p.ctypes.data_as(_P), out.ctypes.data_as(_P),
                                      status.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_lens_undistort: no positions, or a lens that is not finite, has rn <= 0 or a reserved word")
    return (out, status) if return_status else out


def lens_correct_records(model, lens, centers, records, good=None):
    """lk_lens_correct_record (host, the kernel's correction) over one frame: records [S] at centers [S][2] without the lens ->
    (records [S], status uint8 [S]).  good [S]: the records to rewrite (the caller's good rule); None: all of them."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    one_lens = np.ascontiguousarray(lens, LENS_DTYPE).reshape(1)
    c = np.ascontiguousarray(centers, np.float32).reshape(-1, 2)
    rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(len(c))
    out = rec.copy()
    status = np.full(len(c), LENS_NOT_GOOD, np.uint8)
    one = np.zeros(1, RESULT_DTYPE)
    st = C.c_int()
    for s in range(len(c)):
        if good is not None and not good[s]:
            continue
        if _compose_lib.lk_lens_correct_record(int(model), one_lens.ctypes.data_as(_P), float(c[s, 0]), float(c[s, 1]),
                                               rec[s:s + 1].ctypes.data_as(_P), one.ctypes.data_as(_P), C.byref(st)) != 0:
            raise ValueError("lk_lens_correct_record: an unknown model or a refused lens")
        out[s] = one[0]
        status[s] = st.value
    return out, status


def lens_step_from_sums(nuisance, free, rn, sums, min_sectors=None):
    """lk_lens_step_from_sums (host): the sums [F][lens_sums_len(nuisance)] of one evaluation -> (the LENS_STEP_DTYPE record,
    float64 [F][6] = the step of every frame's nuisance)."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.ascontiguousarray(sums, np.float64)
    n = lens_sums_len(nuisance) if int(nuisance) in LENS_Q else 1
    s = s.reshape(-1, n)
    if min_sectors is None:
        min_sectors = LENS_Q.get(int(nuisance), 2)
    out = np.zeros(1, LENS_STEP_DTYPE)
    dn = np.zeros((len(s), 6), np.float64)
    if _compose_lib.lk_lens_step_from_sums(int(nuisance), int(free), float(rn), int(min_sectors), len(s), s.ctypes.data_as(_P),
                                           out.ctypes.data_as(_P), dn.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_lens_step_from_sums: an unknown nuisance, an empty or unknown free, rn <= 0 or min_sectors < Q")
    return out[0], dn


def make_camera(fx, fy, cx, cy, R=None, t=(0.0, 0.0, 0.0), skew=0.0, lens=None):
    """one CAMERA_DTYPE record: x_cam = R X + t, then the pinhole, then `lens` (a LENS_DTYPE record in pixels; None: no lens)"""
    cam = np.zeros(1, CAMERA_DTYPE)
    cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["skew"] = fx, fy, cx, cy, skew
    cam["R"][0] = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    cam["t"][0] = np.asarray(t, np.float64).reshape(3)
    if lens is not None:
        cam["lens"][0] = np.ascontiguousarray(lens, LENS_DTYPE).reshape(1)[0]
    return cam[0]


def _rig(cams):
    """cams: two CAMERA_DTYPE records -> a contiguous [2] array"""
    rig = np.zeros(2, CAMERA_DTYPE)
    rig[0], rig[1] = cams[0], cams[1]
    return rig


def stereo_project(cam, xyz, return_status=False):
    """lk_stereo_project (host, the kernel's camera): world points xyz [n][3] -> pixels float64 [n][2] as the camera shows them;
    with return_status also uint8 [n]: 0, or 1 for a point that is not in front of the camera (pixel 0, 0)."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    one = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
    p = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    out, status = np.zeros((len(p), 2)), np.zeros(len(p), np.uint8)
    if _compose_lib.lk_stereo_project(one.ctypes.data_as(_P), len(p), p.ctypes.data_as(_P), out.ctypes.data_as(_P),
                                      status.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_stereo_project: no points, or a camera that is refused")
    return (out, status) if return_status else out


def stereo_fundamental(cams):
    """lk_stereo_fundamental (host): F float64 [3][3] of the rig, (m1, 1)^T F (m0, 1) = 0 for undistorted pixels of one point."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    rig, F = _rig(cams), np.zeros((3, 3))
    if _compose_lib.lk_stereo_fundamental(rig.ctypes.data_as(_P), F.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_stereo_fundamental: a camera that is refused")
    return F


def stereo_triangulate(cams, x0, x1):
    """lk_stereo_triangulate (host, the kernel's function): pixels x0 [n][2] of camera 0 and x1 [n][2] of camera 1 ->
    STEREO_POINT_DTYPE [n]."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    rig = _rig(cams)
    a, b = np.ascontiguousarray(x0, np.float64).reshape(-1, 2), np.ascontiguousarray(x1, np.float64).reshape(-1, 2)
    out = np.zeros(len(a), STEREO_POINT_DTYPE)
    if len(a) != len(b) or _compose_lib.lk_stereo_triangulate(rig.ctypes.data_as(_P), len(a), a.ctypes.data_as(_P), b.ctypes.data_as(_P),
                                                              out.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_stereo_triangulate: no pairs, x0 and x1 of different lengths, or a camera that is refused")
    return out


def stereo_surface_from_sums(n, sums23, min_neighbours=3, self_good=True, residual_sum=0.0, return_planes=False):
    """lk_stereo_surface_from_sums (host, the kernel's function): the STEREO_SURFACE_DTYPE record of a window of n members
    with the STEREO_SUMS sums; with return_planes also float64 [6][3] = {f0, fx, fy} of the planes of X, Y, Z, U, V, W."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    s = np.ascontiguousarray(sums23, np.float64).reshape(STEREO_SUMS)
    out, planes = np.zeros(1, STEREO_SURFACE_DTYPE), np.zeros((6, 3))
    if _compose_lib.lk_stereo_surface_from_sums(int(n), s.ctypes.data_as(_P), int(min_neighbours), int(bool(self_good)), float(residual_sum),
                                                out.ctypes.data_as(_P), planes.ctypes.data_as(_P)) != 0:
        raise ValueError("lk_stereo_surface_from_sums: n < 0 or min_neighbours < 3")
    return (out[0], planes) if return_planes else out[0]


def epipolar_config(z_near, z_far, level=-1, band=1, n_nodes=17, shape=0, normal=None, min_samples=0, min_score=0.0, def_slot=-1):
    """an LkEpipolarSearch (include/lk_engine.h: lk_epipolar_search); normal None: camera 0's optical axis"""
    nrm = (0.0, 0.0, 0.0) if normal is None else tuple(float(v) for v in np.asarray(normal, np.float64).reshape(3))
    return LkEpipolarSearch(LkGuessSearch(int(level), int(band), int(min_samples), float(min_score), int(def_slot)), int(n_nodes),
                            int(shape), (C.c_int * 3)(0, 0, 0), float(z_near), float(z_far), (C.c_double * 3)(*nrm))


def _depth_range(depth_range, n):
    if depth_range is None:
        return None
    dr = np.ascontiguousarray(depth_range, np.float64)
    if dr.shape != (n, 2):
        raise ValueError("depth_range must be [n][2]")
    return dr


def epipolar_curves(cams, centres, z_near, z_far, level, band=1, n_nodes=17, shape=0, normal=None, depth_range=None, cfg=None):
    """lk_epipolar_curves (host, the table the kernels of lk_search_epipolar read) of centres [n][2] at pyramid `level`:
    -> dict(curves EPIPOLAR_CURVE_DTYPE [n], other int32 [stations], node int32 [stations], inv_depth float64 [stations],
    shape float32 [n][n_nodes][4] or None).  cfg: an LkEpipolarSearch that replaces the keyword arguments."""
    global _compose_lib
    if _compose_lib is None:
        _compose_lib = load_library()
    if cfg is None:
        cfg = epipolar_config(z_near, z_far, level, band, n_nodes, shape, normal)
    rig = _rig(cams)
    cen = np.ascontiguousarray(centres, np.float32).reshape(-1, 2)
    n = len(cen)
    dr = _depth_range(depth_range, n)
    curves, count = np.zeros(max(n, 1), EPIPOLAR_CURVE_DTYPE), C.c_int(0)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(_P)
    fn = _compose_lib.lk_epipolar_curves
    if fn(C.byref(cfg), ptr(rig), n, fptr(cen), ptr(dr), int(level), ptr(curves), C.byref(count), 0, None, None, None, None) != 0:
        raise ValueError("lk_epipolar_curves: a configuration, camera, depth range, level or centre list that is refused")
    m = max(count.value, 1)
    other, node, inv_depth = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.float64)
    shp = np.zeros((n, cfg.n_nodes, 4), np.float32) if cfg.shape else None
    if fn(C.byref(cfg), ptr(rig), n, fptr(cen), ptr(dr), int(level), ptr(curves), C.byref(count), m, ptr(other), ptr(node),
          ptr(inv_depth), ptr(shp)) != 0:
        raise ValueError("lk_epipolar_curves: refused")
    k = count.value
    return dict(curves=curves[:n], other=other[:k], node=node[:k], inv_depth=inv_depth[:k], shape=shp)
