"""correlation_amd - MI355X (gfx950) Lucas-Kanade image-correlation engine.

The product is the C-ABI library `liblk_engine.so` (include/lk_engine.h) built from
correlation_amd/csrc/ by `python -m correlation_amd.build`.  This package is the thin
Python host used by the tests and the benchmark; it holds no compute path of its own
and fails loudly if the library is missing.
"""
from ._ffi import (ERROR_BAD_DOMAIN, ERROR_CORRELATION_MAX_ITERS_REACHED, ERROR_DEVICE,  # noqa: F401
                   ERROR_INTERPOLATION_OUT_OF_IMAGE, ERROR_NONE, FM_U, FM_UV, FM_UVQ,
                   FM_UVUXUYVXVY, IM_BICUBIC, IM_BICUBIC_SEPARABLE, IM_BILINEAR, IM_NEAREST, IMG_DEF, IMG_NXT, IMG_UND,
                   LIB_PATH, N_PARAMS, RESULT_DTYPE, SYMBOLS, UPDATE_BACKWARD, UPDATE_FORWARD, compose_inverse,
                   load_library)
from ._ffi import (FLAVOUR_FAST, FLAVOUR_REFERENCE, FLAVOUR_SAFE, LAUNCH_BACKWARD, LAUNCH_BACKWARD_EVAL,  # noqa: F401
                   LAUNCH_EVAL, LAUNCH_FINISHER, LAUNCH_MAIN, LAUNCH_REPORT_CAPACITY, LAUNCH_SAFE_PASS, LAUNCH_STARVED)
from ._ffi import (GS_NO_CANDIDATE, GS_OK, GS_TEXTURELESS, GS_TOO_FEW, GS_TOO_LARGE, GS_WEAK,  # noqa: F401
                   GUESS_MATCH_DTYPE)
from ._ffi import ROTATED_MATCH_DTYPE, RS_MAX_ANGLES, rotation_table  # noqa: F401
from ._ffi import (EP_MAX_BAND, EP_MAX_GROUP, EP_MAX_NODES, EP_MAX_STATIONS, EPIPOLAR_CURVE_DTYPE, EPIPOLAR_MATCH_DTYPE,  # noqa: F401
                   GS_NO_CURVE, GS_TOO_LONG, epipolar_curves)
from ._ffi import (RESEED_GOOD, RESEED_INFO_DTYPE, RESEED_NO_NEIGHBOUR, RESEED_NOT_IMPROVED, RESEED_PLANNED,  # noqa: F401
                   RESEED_RECOVERED)
from ._ffi import (STRAIN_DEGENERATE, STRAIN_DTYPE, STRAIN_FILLED, STRAIN_GREEN_LAGRANGE, STRAIN_OK, STRAIN_SMALL,  # noqa: F401
                   STRAIN_TOO_FEW, strain_from_gradient)
from ._ffi import (UNC_BAD_RECORD, UNC_OK, UNC_OUT_OF_IMAGE, UNC_SINGULAR, UNC_SUMS, UNC_TOO_FEW,  # noqa: F401
                   UNCERTAINTY_DTYPE, uncertainty_from_sums)
from ._ffi import (ERROR_OUTLIER, OUTLIER_DEGENERATE, OUTLIER_DTYPE, OUTLIER_FLAGGED, OUTLIER_NOT_GOOD, OUTLIER_OK,  # noqa: F401
                   OUTLIER_TOO_FEW, outlier_from_window)
from ._ffi import (TRACK_BAD_POINT, TRACK_DEGENERATE, TRACK_DTYPE, TRACK_INCREMENTAL, TRACK_LOST, TRACK_OK,  # noqa: F401
                   TRACK_RECORDS_CALLER, TRACK_RECORDS_ENGINE, TRACK_RECORDS_WINDOW, TRACK_TOO_FEW, TRACK_TOTAL,
                   gauges_from_tracks, track_step)
from ._ffi import (MOTION_AFFINE, MOTION_DEGENERATE, MOTION_DTYPE, MOTION_MIN_SECTORS, MOTION_OK, MOTION_RIGID,  # noqa: F401
                   MOTION_SIMILARITY, MOTION_TOO_FEW, MOTION_TRANSLATION, motion_apply, motion_from_sums, motion_remove)
from ._ffi import (LENS_AFFINE, LENS_CORRECTED, LENS_DEGENERATE, LENS_DTYPE, LENS_FRAME_DTYPE, LENS_FRAME_OK,  # noqa: F401
                   LENS_FRAME_TOO_FEW, LENS_FREE_CENTRE, LENS_FREE_K1, LENS_FREE_K2, LENS_FREE_P1, LENS_FREE_P2, LENS_MAX_ITERS,
                   LENS_NOT_GOOD, LENS_OK, LENS_OUTSIDE, LENS_PARAMS, LENS_Q, LENS_RESULT_DTYPE, LENS_SIMILARITY, LENS_STEP_DTYPE,
                   LENS_TRANSLATION, lens_correct_records, lens_distort, lens_step_from_sums, lens_sums_len, lens_undistort,
                   make_lens)
from ._ffi import (CAMERA_DTYPE, STEREO_BAD_RECORD, STEREO_BEHIND, STEREO_OK, STEREO_OUTSIDE_LENS, STEREO_PARALLEL,  # noqa: F401
                   STEREO_POINT_DTYPE, STEREO_SUMS, STEREO_SURFACE_DEGENERATE, STEREO_SURFACE_DTYPE, STEREO_SURFACE_FILLED,
                   STEREO_SURFACE_FLOATS, STEREO_SURFACE_OK, STEREO_SURFACE_TOO_FEW, make_camera, stereo_fundamental, stereo_project,
                   stereo_surface_from_sums, stereo_triangulate)
from ._ffi import (MAP_NO_OWNER, PHOTO_BAD_RECORD, PHOTO_FLAT, PHOTO_OK, PHOTO_OUT_OF_IMAGE, PHOTO_SUMS,  # noqa: F401
                   PHOTO_TOO_FEW, PHOTOMETRY_DTYPE, map_owner, photometry_from_sums)
from ._ffi import (ZN_BAD_SEED, ZN_CONVERGED, ZN_FLAT, ZN_MAX_ITERS, ZN_NEGATIVE, ZN_OUT_OF_IMAGE, ZN_SINGULAR,  # noqa: F401
                   ZN_STALLED, ZN_SUMS, ZN_TOO_FEW, ZNSSD_DTYPE, znssd_step_from_sums)
from ._ffi import QD_PARAMS, QD_SUMS, QUADRATIC_DTYPE, quadratic_step_from_sums  # noqa: F401
from ._ffi import spline_weights  # noqa: F401
from ._ffi import WEIGHTED_DTYPE, weight_window, weighted_step_from_sums  # noqa: F401
from ._ffi import COMPOSED_DTYPE, composed_step_from_sums  # noqa: F401
from ._ffi import (PATTERN_APERTURE, PATTERN_DTYPE, PATTERN_FLAT, PATTERN_MAX_HALF, PATTERN_OK, PATTERN_SATURATED,  # noqa: F401
                   PATTERN_SUMS, PATTERN_TOO_FEW, SUBSET_BAD_POINT, SUBSET_DTYPE, SUBSET_NONE, SUBSET_OK, pattern_from_sums)
from ._ffi import (NOISE_BINS, NOISE_DTYPE, NOISE_IMAGES, NOISE_MAX_FRAMES, NOISE_NO_MODEL, NOISE_OK, NOISE_RING,  # noqa: F401
                   NOISE_SUMS, NOISE_TOO_FEW, SECTOR_NOISE_DTYPE, noise_from_bins, noise_from_sums)
from ._ffi import (FIELD_ALL, FIELD_BISQUARE, FIELD_CHANNELS, FIELD_DEFORMED, FIELD_DEGENERATE, FIELD_E1, FIELD_E2,  # noqa: F401
                   FIELD_EXX, FIELD_EXY, FIELD_EYY, FIELD_MISFIT, FIELD_OK, FIELD_REFERENCE, FIELD_THETA, FIELD_TOO_FEW, FIELD_U,
                   FIELD_UNIFORM, FIELD_UX, FIELD_UY, FIELD_V, FIELD_VX, FIELD_VY, FIELD_X0, FIELD_Y0, field_from_sums)
from .engine import HipCorrelationEngine, LkError  # noqa: F401
from . import speckle  # noqa: F401
from . import tracker  # noqa: F401
from .group import HipCorrelationGroup  # noqa: F401
