"""HipCorrelationEngine - thin Python host mirror of the reference's GPU engine surface
(`CudaClass`, cuda_class.cuh:46-79) on top of the C-ABI in include/lk_engine.h.

Method names follow the reference so call sites read like manager_class.cpp; every call
goes straight into liblk_engine.so (HIP).  Used by tests/ and bench.py; the C++ adapter a
maintainer would compile into the Qt application is include/lk_cuda_class_adapter.hpp.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import (FM_U, FM_UV, FM_UVQ, FM_UVUXUYVXVY, IM_BICUBIC, IM_BILINEAR,  # noqa: F401
                   IM_NEAREST, IMG_DEF, IMG_NXT, IMG_UND, RESULT_DTYPE, LkConfig, LkStats)

_ABSENT = object()   # (HipCorrelationEngine._refine) in place of an argument that a refinement pass does not have


class LkError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"lk_engine error {code}: {message}")
        self.code = code


class HipCorrelationEngine:
    _lib = None

    def __init__(self, interpolation=IM_BICUBIC, fitting_model=FM_UVUXUYVXVY, precision=1e-3,
                 max_iters=50, py_start=0, py_step=1, py_stop=2, device=0):
        if HipCorrelationEngine._lib is None:
            HipCorrelationEngine._lib = _ffi.load_library()
        self.lib = HipCorrelationEngine._lib
        self.cfg = LkConfig(interpolation, fitting_model, precision, max_iters, py_start, py_step,
                            py_stop, device)
        self.n_params = _ffi.N_PARAMS[fitting_model]
        self._seq_frames = 0   # frames of the last window this object launched (correlate_sequence_async)
        self._rs_angles = 1    # angles of the last search_rotated
        self._h = C.c_void_p()
        rc = self.lib.lk_create(C.byref(self.cfg), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise LkError(rc, "lk_create failed (no usable HIP device, or bad configuration)")

    # ---- plumbing -----------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            msg = self.lib.lk_last_error_string(self._h)
            raise LkError(rc, msg.decode() if msg else "")
        return rc

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.lk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def device_count():  # CudaClass::initialize
        if HipCorrelationEngine._lib is None:
            HipCorrelationEngine._lib = _ffi.load_library()
        return HipCorrelationEngine._lib.lk_device_count()

    def set_stream(self, hip_stream):
        self._chk(self.lib.lk_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_timing(self, enabled):
        self._chk(self.lib.lk_set_timing(self._h, int(bool(enabled))))

    def set_batch_invariant(self, enabled):
        self._chk(self.lib.lk_set_batch_invariant(self._h, int(bool(enabled))))

    def set_reference_order(self, threads=1):
        """Bit-identical records to the CPU engine with number_of_threads = threads (0: off)."""
        self._chk(self.lib.lk_set_reference_order(self._h, int(threads)))

    def set_update(self, mode):
        """UPDATE_FORWARD (default) or UPDATE_BACKWARD, the inverse-compositional solve (lk_set_update)."""
        self._chk(self.lib.lk_set_update(self._h, int(mode)))

    def set_pairs_in_flight(self, n):
        """lk_set_pairs_in_flight: how many engines solve side by side on this GPU (before commit)."""
        self._chk(self.lib.lk_set_pairs_in_flight(self._h, int(n)))

    def synchronize(self):
        self._chk(self.lib.lk_synchronize(self._h))

    # ---- images (resetImagePyramids / resetNextPyramid / make*PyramidFrom*) -------------
    def set_image(self, slot, pixels):
        a = np.ascontiguousarray(pixels, dtype=np.uint8)
        assert a.ndim == 2
        self._chk(self.lib.lk_set_image(self._h, slot, a.ctypes.data_as(C.c_void_p), a.shape[0],
                                        a.shape[1], a.strides[0]))

    def set_image_device(self, slot, dev_ptr, rows, cols, step=None):
        self._chk(self.lib.lk_set_image_device(self._h, slot, C.c_void_p(dev_ptr), rows, cols,
                                               cols if step is None else step))

    def set_image_pair_device(self, und_ptr, def_ptr, rows, cols, und_step=None, def_step=None):
        self._chk(self.lib.lk_set_image_pair_device(self._h, C.c_void_p(und_ptr), cols if und_step is None else und_step,
                                                    C.c_void_p(def_ptr), cols if def_step is None else def_step,
                                                    rows, cols))

    def set_undeformed_image(self, px):
        self.set_image(IMG_UND, px)

    def set_deformed_image(self, px):
        self.set_image(IMG_DEF, px)

    def set_next_image(self, px):
        self.set_image(IMG_NXT, px)

    def makeUndPyramidFromDef(self):
        self._chk(self.lib.lk_rotate_und_from_def(self._h))

    def makeDefPyramidFromNxt(self):
        self._chk(self.lib.lk_rotate_def_from_nxt(self._h))

    def get_pyramid_level(self, slot, level):
        r, c = C.c_int(), C.c_int()
        self._chk(self.lib.lk_get_pyramid_level(self._h, slot, level, None, C.byref(r), C.byref(c)))
        out = np.empty((r.value, c.value), np.uint8)
        self._chk(self.lib.lk_get_pyramid_level(self._h, slot, level, out.ctypes.data_as(C.c_void_p),
                                                C.byref(r), C.byref(c)))
        return out

    # ---- sectors (resetPolygon overloads) -----------------------------------------------
    def clear_sectors(self):
        self._chk(self.lib.lk_clear_sectors(self._h))

    def resetPolygon_rect(self, sector, x0, y0, x1, y1):
        self._chk(self.lib.lk_set_sector_rect(self._h, sector, x0, y0, x1, y1))

    def resetPolygon_annular(self, sector, r, dr, a, da, cx, cy, as_):
        self._chk(self.lib.lk_set_sector_annular(self._h, sector, r, dr, a, da, cx, cy, as_))

    def set_sectors_annular(self, first_sector, params, as_):
        """lk_set_sectors_annular: params [count][6] = (r, dr, a, da, cx, cy) per sector."""
        q = np.ascontiguousarray(params, np.float32).reshape(-1, 6)
        self._chk(self.lib.lk_set_sectors_annular(self._h, int(first_sector), len(q), _ffi.fptr(q), int(as_)))

    def resetPolygon_blob(self, sector, contour_xy):
        c = np.ascontiguousarray(contour_xy, dtype=np.float32).reshape(-1, 2)
        self._chk(self.lib.lk_set_sector_blob(self._h, sector, _ffi.fptr(c), c.shape[0]))

    def set_sector_points(self, sector, xy, center=None):
        a = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        cx, cy = (center if center is not None else (0.0, 0.0))
        self._chk(self.lib.lk_set_sector_points(self._h, sector, _ffi.fptr(a), a.shape[0],
                                                int(center is not None), cx, cy))

    def set_rect_grid(self, x_begin, y_begin, x_end, y_end, hs, vs, first=0, count=-1):
        self._chk(self.lib.lk_set_rect_grid(self._h, x_begin, y_begin, x_end, y_end, hs, vs, first,
                                            count))

    def commit_sectors(self):
        self._chk(self.lib.lk_commit_sectors(self._h))

    def translate_sectors(self, offsets, centers=None):
        """Lagrangian description: move every sector's samples by add_pair(offset)."""
        o = np.ascontiguousarray(offsets, np.float32).reshape(-1, 2)
        c = None if centers is None else np.ascontiguousarray(centers, np.float32).reshape(-1, 2)
        self._chk(self.lib.lk_translate_sectors(self._h, _ffi.fptr(o), None if c is None else _ffi.fptr(c)))

    def rewarp_sectors(self, centers=None):
        """Strict Lagrangian description: und samples <- def samples of the last solve."""
        c = None if centers is None else np.ascontiguousarray(centers, np.float32).reshape(-1, 2)
        self._chk(self.lib.lk_rewarp_sectors(self._h, None if c is None else _ffi.fptr(c)))

    def update_sector(self, sector, mode):
        """CudaClass::updatePolygon(iSector, deformationDescription), CPU-manager semantics."""
        self._chk(self.lib.lk_update_sector(self._h, sector, mode))

    def restore_sectors(self, first_sector):
        self._chk(self.lib.lk_restore_sectors(self._h, first_sector))

    def last_evaluated_parameters(self):
        out = np.zeros((self.n_sectors, 6), np.float32)
        self._chk(self.lib.lk_get_last_evaluated_parameters(self._h, _ffi.fptr(out)))
        return out

    @property
    def n_sectors(self):
        return self.lib.lk_sector_count(self._h)

    def sector_info(self, sector):
        n, cx, cy = C.c_int(), C.c_float(), C.c_float()
        self._chk(self.lib.lk_get_sector_info(self._h, sector, C.byref(n), C.byref(cx), C.byref(cy)))
        return n.value, cx.value, cy.value

    def sector_level_count(self, sector, level):
        n = C.c_int()
        self._chk(self.lib.lk_get_sector_level_count(self._h, sector, level, C.byref(n)))
        return n.value

    def getUndXY0ToCPU(self, sector):
        n = C.c_int()
        self._chk(self.lib.lk_get_und_xy(self._h, sector, None, 0, C.byref(n)))
        out = np.empty((n.value, 2), np.float32)
        self._chk(self.lib.lk_get_und_xy(self._h, sector, _ffi.fptr(out), n.value, C.byref(n)))
        return out

    def level_xy(self, level, sector, evaluation_copy=False):
        """the device's sample list of a sector at a pyramid level: the reference's order, or the row-major copy
        the lane groups of the default mode walk (lk_get_level_xy)"""
        n = C.c_int()
        self._chk(self.lib.lk_get_level_xy(self._h, level, int(evaluation_copy), sector, None, 0, C.byref(n)))
        out = np.empty((n.value, 2), np.float32)
        if n.value:
            self._chk(self.lib.lk_get_level_xy(self._h, level, int(evaluation_copy), sector, _ffi.fptr(out), n.value, C.byref(n)))
        return out

    def getDefXY0ToCPU(self, sector, p):
        pp = np.zeros(6, np.float32)
        pp[:len(p)] = p
        n = C.c_int()
        self._chk(self.lib.lk_get_def_xy(self._h, sector, _ffi.fptr(pp), None, 0, C.byref(n)))
        out = np.empty((n.value, 2), np.float32)
        self._chk(self.lib.lk_get_def_xy(self._h, sector, _ffi.fptr(pp), _ffi.fptr(out), n.value,
                                         C.byref(n)))
        return out

    # ---- solve --------------------------------------------------------------------------
    def correlate(self, sector, initial_guess):
        """CudaClass::correlate: returns (result record, updated guess)."""
        g = np.zeros(6, np.float32)
        g[:self.n_params] = np.asarray(initial_guess, np.float32)[:self.n_params]
        out = np.zeros(1, RESULT_DTYPE)
        self._chk(self.lib.lk_correlate(self._h, sector, _ffi.fptr(g), out.ctypes.data_as(C.c_void_p)))
        return out[0], g

    def correlate_all(self, guesses=None):
        S = self.n_sectors
        out = np.zeros(S, RESULT_DTYPE)
        if guesses is None:
            gp = None
        else:
            g = np.zeros((S, 6), np.float32)
            ga = np.asarray(guesses, np.float32)
            if ga.ndim == 1:
                g[:, :ga.shape[0]] = ga
            else:
                g[:, :ga.shape[1]] = ga
            gp = _ffi.fptr(g)
        self._chk(self.lib.lk_correlate_all(self._h, gp, out.ctypes.data_as(C.c_void_p)))
        return out

    def correlate_all_device(self, d_guesses_ptr, d_results_ptr):
        self._chk(self.lib.lk_correlate_all_device(self._h, C.c_void_p(d_guesses_ptr),
                                                   C.c_void_p(d_results_ptr)))

    def correlate_all_async(self):
        """lk_correlate_all_async: the engine-held guesses, no waiting; wait_results() fetches."""
        self._chk(self.lib.lk_correlate_all_async(self._h))

    def wait_results(self):
        out = np.zeros(self.n_sectors, RESULT_DTYPE)
        self._chk(self.lib.lk_wait_results(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- frame-pipelined windows (lk_correlate_sequence_async) --------------------------
    def sequence_reserve(self, n_slots):
        self._chk(self.lib.lk_sequence_reserve(self._h, int(n_slots)))

    def sequence_set_frame(self, slot, pixels):
        a = np.ascontiguousarray(pixels, dtype=np.uint8)
        assert a.ndim == 2
        self._chk(self.lib.lk_sequence_set_frame(self._h, int(slot), a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1],
                                                 a.strides[0]))

    def sequence_set_frame_device(self, slot, dev_ptr, rows, cols, step=None):
        self._chk(self.lib.lk_sequence_set_frame_device(self._h, int(slot), C.c_void_p(dev_ptr), rows, cols,
                                                        cols if step is None else step))

    def correlate_sequence_async(self, n_frames, first_slot=0, und_slot=-1, reference_previous=False,
                                 constant_velocity=True, host_records=True, keep_guesses=False):
        self._seq_frames = int(n_frames)
        self._chk(self.lib.lk_correlate_sequence_async(self._h, int(und_slot), int(first_slot), int(n_frames),
                                                       int(bool(reference_previous)), int(bool(constant_velocity)),
                                                       (1 if host_records else 0) | (2 if keep_guesses else 0)))

    def wait_sequence(self, host_records=True):
        """records [n_frames][S] of the window (or None when the window keeps them on the device)"""
        out = np.zeros((self._seq_frames, self.n_sectors), RESULT_DTYPE) if host_records else None
        self._chk(self.lib.lk_wait_sequence(self._h, out.ctypes.data_as(C.c_void_p) if host_records else None))
        return out

    def correlate_sequence(self, n_frames, **kw):
        self.correlate_sequence_async(n_frames, **kw)
        return self.wait_sequence(kw.get("host_records", True))

    def sequence_results_device(self):
        r, g = C.c_void_p(), C.c_void_p()
        self._chk(self.lib.lk_get_sequence_results_device(self._h, C.byref(r), C.byref(g)))
        return r.value, g.value

    def copy_sequence_records_device(self, dst_ptr, pitch_records):
        self._chk(self.lib.lk_copy_sequence_records_device(self._h, C.c_void_p(dst_ptr), C.c_size_t(int(pitch_records))))

    def sequence_guesses(self):
        g = np.zeros((self._seq_frames, self.n_sectors, 6), np.float32)
        self._chk(self.lib.lk_get_sequence_guesses(self._h, _ffi.fptr(g)))
        return g

    @property
    def sequence_is_pipelined(self):
        return bool(self.lib.lk_sequence_is_pipelined(self._h))

    def adjust_initial_guess(self, frame, constant_velocity, global_guess, global_center):
        g = np.zeros(6, np.float32)
        g[:len(global_guess)] = global_guess
        self._chk(self.lib.lk_adjust_initial_guess(self._h, frame, int(constant_velocity),
                                                   _ffi.fptr(g), global_center[0], global_center[1]))

    def get_guesses(self):
        g = np.zeros((self.n_sectors, 6), np.float32)
        self._chk(self.lib.lk_get_guesses(self._h, _ffi.fptr(g)))
        return g

    # ---- automatic initial guess (the GUI's "Initial Guess: Automatic") -----------------------
    def search_guesses(self, radius, level=-1, guesses=None, min_samples=0, min_score=0.0, def_slot=-1):
        """Integer-pixel ZNCC search of every sector at pyramid `level` (-1: py_stop) within +-radius pixels of that level
        about its guess (include/lk_engine.h: lk_search_guesses).  guesses None: about the engine-held guesses, on the
        engine's stream, returns None; else [S][6] centres, returns the refined [S][6] (also engine-held)."""
        cfg = _ffi.LkGuessSearch(int(level), int(radius), int(min_samples), float(min_score), int(def_slot))
        if guesses is None:
            self._chk(self.lib.lk_search_guesses(self._h, C.byref(cfg), None))
            return None
        g = np.array(guesses, np.float32).reshape(self.n_sectors, 6)
        self._chk(self.lib.lk_search_guesses(self._h, C.byref(cfg), _ffi.fptr(g)))
        return g

    def guess_search_info(self):
        """The matches of the last search_guesses: a GUESS_MATCH_DTYPE array [S]."""
        out = np.zeros(self.n_sectors, _ffi.GUESS_MATCH_DTYPE)
        self._chk(self.lib.lk_get_guess_search_info(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- rotation-aware automatic initial guess: the same search over angle and shift ------------
    def search_rotated(self, radius, angle_step, n_half, angle_center=0.0, level=-1, guesses=None, min_samples=0,
                       min_score=0.0, def_slot=-1):
        """search_guesses at every angle angle_center + k angle_step (radians), k = -n_half .. n_half; an OK sector also gets
        the winning rotation in g[2..5] (affine) or g[2] (FM_UVQ) (include/lk_engine.h: lk_search_rotated).  guesses as for
        search_guesses."""
        cfg = _ffi.LkRotatedSearch(_ffi.LkGuessSearch(int(level), int(radius), int(min_samples), float(min_score), int(def_slot)),
                                   float(angle_center), float(angle_step), int(n_half))
        g = None if guesses is None else np.array(guesses, np.float32).reshape(self.n_sectors, 6)
        self._chk(self.lib.lk_search_rotated(self._h, C.byref(cfg), None if g is None else _ffi.fptr(g)))
        self._rs_angles = 2 * int(n_half) + 1
        return g

    def rotated_search_info(self):
        """The matches of the last search_rotated: a ROTATED_MATCH_DTYPE array [S]."""
        out = np.zeros(self.n_sectors, _ffi.ROTATED_MATCH_DTYPE)
        self._chk(self.lib.lk_get_rotated_search_info(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def rotated_search_profile(self):
        """The best score per angle of the last search_rotated: float64 [S][2 n_half + 1], -2 where an angle has none."""
        out = np.zeros((self.n_sectors, self._rs_angles), np.float64)
        self._chk(self.lib.lk_get_rotated_search_profile(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    @staticmethod
    def rotation_table(angle_step, n_half, angle_center=0.0):
        """lk_rotation_table: the {cos, sin} table search_rotated uploads, float32 [2 n_half + 1][2]."""
        return _ffi.rotation_table(angle_step, n_half, angle_center)

    # ---- stereo initial guess: the same search along the epipolar curve of a calibrated rig ------
    def search_epipolar(self, cams, z_near, z_far, level=-1, band=1, n_nodes=17, shape=0, normal=None, depth_range=None,
                        guesses=None, min_samples=0, min_score=0.0, def_slot=-1):
        """search_guesses' template scored at the integer stations of every sector's epipolar curve in camera 1 - camera 0's ray
        through the sector's centre between the depths z_near and z_far (depth_range [S][2]: per sector) - and +-band pixels
        across it (include/lk_engine.h: lk_search_epipolar).  cams: two CAMERA_DTYPE records; shape 1: the template is mapped by
        the Jacobian the plane of `normal` induces and an OK sector also gets g[2..5].  guesses as for search_guesses (their
        first two words are no search centre here)."""
        cfg = _ffi.epipolar_config(z_near, z_far, level, band, n_nodes, shape, normal, min_samples, min_score, def_slot)
        rig = None if cams is None else _ffi._rig(cams)
        dr = _ffi._depth_range(depth_range, self.n_sectors)
        g = None if guesses is None else np.array(guesses, np.float32).reshape(self.n_sectors, 6)
        self._chk(self.lib.lk_search_epipolar(self._h, C.byref(cfg), None if rig is None else rig.ctypes.data_as(C.c_void_p),
                                              None if dr is None else dr.ctypes.data_as(C.c_void_p),
                                              None if g is None else _ffi.fptr(g)))
        return g

    def epipolar_search_info(self):
        """The matches of the last search_epipolar: an EPIPOLAR_MATCH_DTYPE array [S]."""
        out = np.zeros(self.n_sectors, _ffi.EPIPOLAR_MATCH_DTYPE)
        self._chk(self.lib.lk_get_epipolar_search_info(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def epipolar_search_profile(self):
        """The last search_epipolar's curves (EPIPOLAR_CURVE_DTYPE [S]) and its best score per station, float64, concatenated:
        sector s at curves[s]["first_index"], curves[s]["n_stations"] values, -2 where a station has none."""
        curves, count = np.zeros(max(self.n_sectors, 1), _ffi.EPIPOLAR_CURVE_DTYPE), C.c_int(0)
        self._chk(self.lib.lk_get_epipolar_search_profile(self._h, curves.ctypes.data_as(C.c_void_p), None, C.byref(count)))
        prof = np.zeros(max(count.value, 1), np.float64)
        self._chk(self.lib.lk_get_epipolar_search_profile(self._h, curves.ctypes.data_as(C.c_void_p), prof.ctypes.data_as(C.c_void_p),
                                                          C.byref(count)))
        return curves[:self.n_sectors], prof[:count.value]

    def epipolar_last(self):
        """bench hook: (search kernel ms, reduce kernel ms, host curve table ms, candidates, LDS window bytes, longest run)"""
        a, b, c, n, w, r = C.c_float(0), C.c_float(0), C.c_double(0), C.c_longlong(0), C.c_int(0), C.c_int(0)
        fn = self.lib.lk_internal_epipolar_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_longlong),
                       C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._chk(fn(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n), C.byref(w), C.byref(r)))
        return a.value, b.value, c.value, n.value, w.value, r.value

    # ---- recovery pass: failed sectors re-solved from their converged neighbours ---------------
    def reseed_failed(self, radius, chi_max=0.0, min_neighbours=1, max_rounds=8, want_records=True):
        """lk_reseed_failed on the records of the last correlate_all: returns (records [S] or None, sectors recovered)."""
        cfg = _ffi.LkReseedConfig(float(chi_max), float(radius), int(min_neighbours), int(max_rounds))
        out = np.zeros(self.n_sectors, RESULT_DTYPE) if want_records else None
        n = C.c_int()
        self._chk(self.lib.lk_reseed_failed(self._h, C.byref(cfg), out.ctypes.data_as(C.c_void_p) if want_records else None,
                                            C.byref(n)))
        return out, n.value

    def reseed_info(self):
        """What the last reseed_failed did: a RESEED_INFO_DTYPE array [S]."""
        out = np.zeros(self.n_sectors, _ffi.RESEED_INFO_DTYPE)
        self._chk(self.lib.lk_get_reseed_info(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def reseed_plan(self, records, radius, chi_max=0.0, min_neighbours=1):
        """lk_reseed_plan: one round's planning step on the caller's records [S]: (guesses [S][6], info [S]); nothing is
        solved and no engine state changes."""
        cfg = _ffi.LkReseedConfig(float(chi_max), float(radius), int(min_neighbours), 1)
        rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(self.n_sectors)
        g = np.zeros((self.n_sectors, 6), np.float32)
        info = np.zeros(self.n_sectors, _ffi.RESEED_INFO_DTYPE)
        self._chk(self.lib.lk_reseed_plan(self._h, C.byref(cfg), rec.ctypes.data_as(C.c_void_p), _ffi.fptr(g),
                                          info.ctypes.data_as(C.c_void_p)))
        return g, info

    def cell_grid(self, radius):
        """Test hook (lk_internal_cell_grid): the cell grid a neighbour pass builds over the committed centres for `radius`,
        as a dict: nx, ny, cell, x0, y0 and the tables cell_of uint32 [S], start uint32 [nx ny + 1], members uint32 [S].
        No engine state changes."""
        S = self.n_sectors
        nx, ny, cell, x0, y0 = C.c_int(), C.c_int(), C.c_double(), C.c_double(), C.c_double()
        cell_of, members = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
        start = np.zeros(4 * S + 1025, np.uint32)      # the sizing rule caps the table at 4 S + 1024 cells
        fn = self.lib.lk_internal_cell_grid
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                       C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self._chk(fn(self._h, float(radius), C.byref(nx), C.byref(ny), C.byref(cell), C.byref(x0), C.byref(y0),
                     cell_of.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p), start.size,
                     members.ctypes.data_as(C.c_void_p)))
        return dict(nx=nx.value, ny=ny.value, cell=cell.value, x0=x0.value, y0=y0.value, cell_of=cell_of,
                    start=start[:nx.value * ny.value + 1].copy(), members=members)

    # ---- strain field: windowed plane fit of the solved displacements ------------------------------
    def strain_field(self, radius, chi_max=0.0, min_neighbours=3, tensor=_ffi.STRAIN_GREEN_LAGRANGE, records=None):
        """lk_strain_field: a STRAIN_DTYPE array [S] from the engine-held records of the last batch solve (after
        reseed_failed: the repaired ones) or, records given, from those [S]; no engine state changes."""
        cfg = _ffi.LkStrainConfig(float(radius), float(chi_max), int(min_neighbours), int(tensor))
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(self.n_sectors)
        out = np.zeros(self.n_sectors, _ffi.STRAIN_DTYPE)
        self._chk(self.lib.lk_strain_field(self._h, C.byref(cfg), rec.ctypes.data_as(C.c_void_p) if rec is not None else None,
                                           out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- per-sector uncertainty: covariance of the solved parameters ----------------------------------
    def parameter_uncertainty(self, records=None, def_slot=-1, return_sums=False):
        """lk_parameter_uncertainty: an UNCERTAINTY_DTYPE array [S] from the engine-held records of the last batch solve
        or, records given, from those [S]; with return_sums also the 28 double sums of every sector [S][28].  No engine
        state changes."""
        cfg = _ffi.LkUncertaintyConfig(int(def_slot), 0)
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(self.n_sectors)
        out = np.zeros(self.n_sectors, _ffi.UNCERTAINTY_DTYPE)
        sums = np.zeros((self.n_sectors, _ffi.UNC_SUMS), np.float64) if return_sums else None
        self._chk(self.lib.lk_parameter_uncertainty(self._h, C.byref(cfg),
                                                    rec.ctypes.data_as(C.c_void_p) if rec is not None else None,
                                                    out.ctypes.data_as(C.c_void_p),
                                                    sums.ctypes.data_as(C.c_void_p) if return_sums else None))
        return (out, sums) if return_sums else out

    # ---- outlier flags: the (detrended) normalised median test ----------------------------------------
    def flag_outliers(self, radius, chi_max=0.0, eps=0.02, threshold=3.0, min_neighbours=None, detrend=True, passes=1,
                      mark=False, records=None, return_records=False):
        """lk_flag_outliers: (OUTLIER_DTYPE array [S], sectors flagged) from the engine-held records of the last batch
        solve or, records given, from those [S]; with return_records also the records that were read, the flagged ones
        carrying ERROR_OUTLIER when mark is set.  mark on the engine-held records writes that code into them: the only
        engine state the call changes."""
        if min_neighbours is None:
            min_neighbours = 4 if detrend else 3
        cfg = _ffi.LkOutlierConfig(float(radius), float(chi_max), float(eps), float(threshold), int(min_neighbours),
                                   int(detrend), int(passes), int(mark))
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(self.n_sectors)
        out = np.zeros(self.n_sectors, _ffi.OUTLIER_DTYPE)
        rec_out = np.zeros(self.n_sectors, RESULT_DTYPE) if return_records else None
        n = C.c_int()
        self._chk(self.lib.lk_flag_outliers(self._h, C.byref(cfg), rec.ctypes.data_as(C.c_void_p) if rec is not None else None,
                                            out.ctypes.data_as(C.c_void_p),
                                            rec_out.ctypes.data_as(C.c_void_p) if return_records else None, C.byref(n)))
        return (out, n.value, rec_out) if return_records else (out, n.value)

    @staticmethod
    def outlier_from_window(e_u, e_v, es_u, es_v, eps, threshold):
        """lk_outlier_from_window: the kernel's selection and ratio arithmetic on the host (no engine needed)."""
        return _ffi.outlier_from_window(e_u, e_v, es_u, es_v, eps, threshold)

    # ---- photometry and the back-warped residual map ----------------------------------------------------
    def photometry(self, records=None, def_slot=-1, chi_max=0.0, return_sums=False):
        """lk_photometry: a PHOTOMETRY_DTYPE array [S] (ZNCC, gain, offset, residuals of every good sector at its record's
        parameters) from the engine-held records of the last batch solve or, records given, from those [S]; with
        return_sums also the eight double sums of every sector [S][8].  No engine state changes."""
        cfg = _ffi.LkPhotometryConfig(int(def_slot), float(chi_max))
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(self.n_sectors)
        out = np.zeros(self.n_sectors, _ffi.PHOTOMETRY_DTYPE)
        sums = np.zeros((self.n_sectors, _ffi.PHOTO_SUMS), np.float64) if return_sums else None
        self._chk(self.lib.lk_photometry(self._h, C.byref(cfg), rec.ctypes.data_as(C.c_void_p) if rec is not None else None,
                                         out.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p) if return_sums else None))
        return (out, sums) if return_sums else out

    def residual_map(self, radius, window=None, records=None, def_slot=-1, chi_max=0.0, want=("warped", "residual", "owner")):
        """lk_residual_map: the deformed frame pulled back into the reference configuration by the solved field, at pyramid
        level py_start.  window = (x0, y0, w, h) in that level's pixels, None: the whole image.  Returns (warped float32 [h][w],
        residual float32 [h][w], owner int32 [h][w]); an output not named in `want` is None.  owner: the sector, -1 without a
        good sector within `radius` (level-0 pixels), -2 - s where sector s owns the pixel but the position left the deformed
        image; the float maps are NaN in both cases.  No engine state changes."""
        x0, y0, w, h = (0, 0, 0, 0) if window is None else (int(t) for t in window)
        cfg = _ffi.LkResidualMapConfig(int(def_slot), float(chi_max), float(radius), x0, y0, w, h, 0)
        if window is None:
            r, c = C.c_int(), C.c_int()
            self._chk(self.lib.lk_get_pyramid_level(self._h, _ffi.IMG_UND, self.cfg.py_start, None, C.byref(r), C.byref(c)))
            h, w = r.value, c.value
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(self.n_sectors)
        shape = (max(h, 0), max(w, 0))
        warped = np.zeros(shape, np.float32) if "warped" in want else None
        residual = np.zeros(shape, np.float32) if "residual" in want else None
        owner = np.zeros(shape, np.int32) if "owner" in want else None

        def ptr(a):
            return a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.lib.lk_residual_map(self._h, C.byref(cfg), ptr(rec), ptr(warped), ptr(residual), ptr(owner)))
        return warped, residual, owner

    def residual_last(self):
        """Bench hook: (device ms, pixel tiles, tiles that took the global-memory fall-back) of the last photometry or
        residual_map call."""
        ms, tiles, fb = C.c_float(), C.c_int(), C.c_int()
        fn = self.lib.lk_internal_residual_last
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._chk(fn(self._h, C.byref(ms), C.byref(tiles), C.byref(fb)))
        return ms.value, tiles.value, fb.value

    @staticmethod
    def photometry_from_sums(n, sums8):
        """lk_photometry_from_sums: the kernel's record arithmetic on the host (no engine needed)."""
        return _ffi.photometry_from_sums(n, sums8)

    @staticmethod
    def map_owner(centers, X, Y, radius, good=None):
        """lk_map_owner: the residual map's owner rule on the host (no engine needed)."""
        return _ffi.map_owner(centers, X, Y, radius, good)

    # ---- what the five refinement passes share ----------------------------------------------------------------
    def _refine(self, name, cfg_type, head, words, info_dtype, n_sums, return_sums, records, guesses, second=_ABSENT, mask=_ABSENT):
        """One call of the refinement pass `name`.  head: (def_slot, chi_max, max_iters, precision, lambda0), max_iters < 0 and
        precision <= 0 taking the engine's own; words: the configuration's words behind them, a mask's dimensions following.
        second, mask: _ABSENT in a pass without the argument.  Returns (records, info) and, with return_sums, the sums."""
        def_slot, chi_max, max_iters, precision, lambda0 = head
        S, m = self.n_sectors, None if mask is None or mask is _ABSENT else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        if m is not None and m.ndim != 2:
            raise ValueError(name[3:] + ": mask must be [rows][cols]")
        if mask is not _ABSENT:
            words += m.shape if m is not None else (0, 0)
        cfg = cfg_type(int(def_slot), float(chi_max), int(max_iters) if max_iters >= 0 else int(self.cfg.max_iters),
                       float(precision) if precision > 0 else float(self.cfg.precision), float(lambda0), *words)
        rec = None if records is None else np.ascontiguousarray(records, RESULT_DTYPE).reshape(S)
        g, g2 = (None if a is None or a is _ABSENT else np.ascontiguousarray(a, np.float32).reshape(S, 6) for a in (guesses, second))
        out, info = np.zeros(S, RESULT_DTYPE), np.zeros(S, info_dtype)
        sums = np.zeros((S, n_sums), np.float64) if return_sums else None

        def ptr(a, as_type=C.c_void_p):
            return a.ctypes.data_as(as_type) if a is not None else None
        args = [ptr(m)] * (mask is not _ABSENT) + [ptr(rec), ptr(g, _ffi._F)] + [ptr(g2, _ffi._F)] * (second is not _ABSENT)
        self._chk(getattr(self.lib, name)(self._h, C.byref(cfg), *args, ptr(out), ptr(info), ptr(sums)))
        return (out, info, sums) if return_sums else (out, info)

    def _refine_last(self, name, extra=False):
        """A refinement pass's bench hook: (device ms, count3) and, with extra, one more float behind them."""
        ms, cnt, more = C.c_float(), (C.c_int * 3)(), C.c_float()
        fn = getattr(self.lib, name)
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)] + [C.POINTER(C.c_float)] * extra
        self._chk(fn(self._h, C.byref(ms), cnt, *[C.byref(more)] * extra))
        return (ms.value, tuple(cnt), more.value) if extra else (ms.value, tuple(cnt))

    # ---- ZNSSD refinement: the sub-pixel solve that does not mind the lighting ----------------------------
    def refine_znssd(self, records=None, guesses=None, def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0, lambda0=0.0,
                     return_sums=False):
        """lk_refine_znssd: every sector refined by Levenberg-Marquardt on the zero-mean normalised criterion at pyramid
        level py_start, from `guesses` [S][6] (level-0 scale, as search_guesses returns them) or from records - those
        given [S], else the engine-held ones of the last batch solve.  max_iters < 0 and precision <= 0: the engine's own.
        Returns (records RESULT_DTYPE [S], info ZNSSD_DTYPE [S]) and, with return_sums, the 45 double sums of every sector
        at the returned parameters [S][45].  No engine state changes."""
        return self._refine("lk_refine_znssd", _ffi.LkZnssdConfig, (def_slot, chi_max, max_iters, precision, lambda0), (),
                            _ffi.ZNSSD_DTYPE, _ffi.ZN_SUMS, return_sums, records, guesses)

    def znssd_last(self):
        """Bench hook: (device ms, the sectors the 16-, 64- and 512-lane groups took) of the last refine_znssd call."""
        return self._refine_last("lk_internal_znssd_last")

    @staticmethod
    def znssd_step_from_sums(model, n, sums, lam):
        """lk_znssd_step_from_sums: the kernel's criterion and step on the host (no engine needed)."""
        return _ffi.znssd_step_from_sums(model, n, sums, lam)

    # ---- second-order refinement: a subset model that can bend ----------------------------------------------
    def refine_quadratic(self, records=None, guesses=None, second=None, def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0,
                         lambda0=0.0, return_sums=False):
        """lk_refine_quadratic: refine_znssd with second-order shape functions - twelve parameters (u, v, ux, uy, vx, vy, uxx,
        uxy, uyy, vxx, vxy, vyy) whatever the engine's model, which only says how `guesses` [S][6] and the records are read
        and the returned records written.  second: [S][6] second-order seeds in level-0 scale (None: zeros); feeding
        (records, info["p"][:, 6:]) back in continues a refinement.  Returns (records RESULT_DTYPE [S], info QUADRATIC_DTYPE
        [S]) and, with return_sums, the 88 double sums of every sector at the returned parameters.  No engine state changes."""
        return self._refine("lk_refine_quadratic", _ffi.LkQuadraticConfig, (def_slot, chi_max, max_iters, precision, lambda0), (),
                            _ffi.QUADRATIC_DTYPE, _ffi.QD_SUMS, return_sums, records, guesses, second=second)

    def quadratic_last(self):
        """Bench hook: (device ms, the sectors the 16-, 64- and 512-lane groups took) of the last refine_quadratic call."""
        return self._refine_last("lk_internal_quadratic_last")

    @staticmethod
    def quadratic_step_from_sums(n, sums, lam):
        """lk_quadratic_step_from_sums: the kernel's criterion and step on the host (no engine needed)."""
        return _ffi.quadratic_step_from_sums(n, sums, lam)

    # ---- B-spline refinement: the sub-pixel solve without the bicubic's interpolation bias ------------------
    def refine_spline(self, records=None, guesses=None, order=5, def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0,
                      lambda0=0.0, return_sums=False):
        """lk_refine_spline: refine_znssd with the deformed image and its gradient taken from a cubic (order 3) or quintic
        (order 5) B-spline of the prefiltered level-py_start image; the engine's interpolation plays no part.  Arguments and
        return as refine_znssd: (records RESULT_DTYPE [S], info ZNSSD_DTYPE [S]) and, with return_sums, the 45 double sums
        [S][45].  No engine state changes."""
        return self._refine("lk_refine_spline", _ffi.LkSplineConfig, (def_slot, chi_max, max_iters, precision, lambda0), (int(order),),
                            _ffi.ZNSSD_DTYPE, _ffi.ZN_SUMS, return_sums, records, guesses)

    def spline_last(self):
        """Bench hook: (device ms, the sectors the 16-, 64- and 512-lane groups took, of that time the build of the
        coefficient image) of the last refine_spline call."""
        return self._refine_last("lk_internal_spline_last", extra=True)

    def spline_coefficients(self, slot, order=5):
        """lk_spline_coefficients: the float32 B-spline coefficient image [rows][cols] of the level-py_start image of `slot`,
        as the pass builds it.  Needs no sectors; no engine state changes."""
        r, c = C.c_int(), C.c_int()
        self._chk(self.lib.lk_get_pyramid_level(self._h, int(slot), self.cfg.py_start, None, C.byref(r), C.byref(c)))
        out = np.zeros((r.value, c.value), np.float32)
        self._chk(self.lib.lk_spline_coefficients(self._h, int(slot), int(order), _ffi.fptr(out)))
        return out

    def spline_sample(self, slot, xy, order=5):
        """lk_spline_sample: [n][4] float32 = W, Wx, Wy, ok of the pass's sampler at the points xy [n][2] (level-py_start
        pixels of the image of `slot`); ok = 1, or a row of zeros where the sampler's window leaves the image."""
        a = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.zeros((a.shape[0], 4), np.float32)
        self._chk(self.lib.lk_spline_sample(self._h, int(slot), int(order), _ffi.fptr(a), a.shape[0], _ffi.fptr(out)))
        return out

    @staticmethod
    def spline_weights(order, t):
        """lk_spline_weights: the sampler's weights and derivative weights on the host (no engine needed)."""
        return _ffi.spline_weights(order, t)

    # ---- weighted refinement: a pixel mask and a Gaussian window inside the ZNSSD sums ------------------------
    def refine_weighted(self, records=None, guesses=None, sigma=0.0, mask=None, min_fraction=0.0, def_slot=-1, chi_max=0.0,
                        max_iters=-1, precision=0.0, lambda0=0.0, return_sums=False):
        """lk_refine_weighted: refine_znssd with the weight w = mask(node) * window(q - centre) on every sample.  sigma: the
        standard deviation of the Gaussian window in level-0 pixels (0: no window); mask: [rows][cols] of the level-py_start
        undeformed image, nonzero = use (None: every pixel); min_fraction: a sector with fewer than min_fraction * n_L
        samples of positive weight is ZN_TOO_FEW.  The other arguments as refine_znssd.  Returns (records RESULT_DTYPE [S],
        info WEIGHTED_DTYPE [S]) and, with return_sums, the 45 weighted double sums [S][45].  No engine state changes."""
        return self._refine("lk_refine_weighted", _ffi.LkWeightedConfig, (def_slot, chi_max, max_iters, precision, lambda0),
                            (float(sigma), float(min_fraction)), _ffi.WEIGHTED_DTYPE, _ffi.ZN_SUMS, return_sums, records, guesses,
                            mask=mask)

    def weighted_last(self):
        """Bench hook: (device ms, the sectors the 16-, 64- and 512-lane groups took) of the last refine_weighted call."""
        return self._refine_last("lk_internal_weighted_last")

    @staticmethod
    def weight_window(inv, dx, dy):
        """lk_weight_window: the kernel's window function on the host (no engine needed)."""
        return _ffi.weight_window(inv, dx, dy)

    @staticmethod
    def weighted_step_from_sums(model, n_valid, N, sums, lam):
        """lk_weighted_step_from_sums: the kernel's criterion and step for weighted sums on the host (no engine needed)."""
        return _ffi.weighted_step_from_sums(model, n_valid, N, sums, lam)

    # ---- composed refinement: model order, sampler and weights chosen independently ---------------------------
    def refine_composed(self, records=None, guesses=None, second=None, order=2, sampler=0, sigma=0.0, mask=None, min_fraction=0.0,
                        def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0, lambda0=0.0, return_sums=False):
        """lk_refine_composed: order 1 (the engine's model, refine_znssd's parameters) or 2 (refine_quadratic's twelve),
        sampler 0 (the engine's interpolator), 3 or 5 (refine_spline's cubic or quintic B-spline), and refine_weighted's
        sigma, mask and min_fraction, each chosen independently.  second: [S][6] second-order seeds, order 2 only.  Returns
        (records RESULT_DTYPE [S], info COMPOSED_DTYPE [S]) and, with return_sums, the weighted double sums [S][45] (order 1)
        or [S][88] (order 2).  No engine state changes."""
        return self._refine("lk_refine_composed", _ffi.LkComposedConfig, (def_slot, chi_max, max_iters, precision, lambda0),
                            (int(order), int(sampler), float(sigma), float(min_fraction)), _ffi.COMPOSED_DTYPE,
                            _ffi.QD_SUMS if int(order) == 2 else _ffi.ZN_SUMS, return_sums, records, guesses, second=second, mask=mask)

    def composed_last(self):
        """Bench hook: (device ms, the sectors the 16-, 64- and 512-lane groups took) of the last refine_composed call."""
        return self._refine_last("lk_internal_composed_last")

    @staticmethod
    def composed_step_from_sums(order, model, n_valid, N, sums, lam):
        """lk_composed_step_from_sums: the kernels' criterion and step of either order on the host (no engine needed)."""
        return _ffi.composed_step_from_sums(order, model, n_valid, N, sums, lam)

    # ---- speckle quality: is the pattern good enough, how large must the subsets be ----------------------
    def pattern_quality(self, slot=_ffi.IMG_UND, grey_low=0, grey_high=255, noise_sigma=1.0, max_saturated=1.0,
                        return_sums=False):
        """lk_pattern_quality: a PATTERN_DTYPE array [S] (mean, contrast, SSSIG, MIG, saturated fractions and the predicted
        displacement error of every committed sector) from the level-py_start image of `slot` alone; with return_sums also
        the nine int64 sums [S][9] and the gradient-magnitude sums [S].  No engine state changes."""
        cfg = _ffi.LkPatternConfig(int(slot), int(grey_low), int(grey_high), float(noise_sigma), float(max_saturated))
        out = np.zeros(self.n_sectors, _ffi.PATTERN_DTYPE)
        sums = np.zeros((self.n_sectors, _ffi.PATTERN_SUMS), np.int64) if return_sums else None
        mig = np.zeros(self.n_sectors, np.float64) if return_sums else None
        self._chk(self.lib.lk_pattern_quality(self._h, C.byref(cfg), out.ctypes.data_as(C.c_void_p),
                                              sums.ctypes.data_as(C.c_void_p) if return_sums else None,
                                              mig.ctypes.data_as(C.c_void_p) if return_sums else None))
        return (out, sums, mig) if return_sums else out

    def suggest_subset(self, points, sssig_min, half_min=5, half_max=40, half_step=1, slot=_ffi.IMG_UND, noise_sigma=1.0,
                       return_sums=False):
        """lk_suggest_subset: a SUBSET_DTYPE array [Q], for every point [Q][2] (level-py_start pixels of the image of `slot`)
        the smallest half-width of half_min, half_min + half_step, ... <= half_max whose box has SSSIG_x and SSSIG_y >=
        sssig_min; with return_sums also Gxx and Gyy of every candidate box, uint32 [Q][n_cand][2].  Needs no sectors; no
        engine state changes."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        cfg = _ffi.LkSubsetConfig(int(slot), int(half_min), int(half_max), int(half_step), float(sssig_min), float(noise_sigma))
        n_cand = max((int(half_max) - int(half_min)) // max(int(half_step), 1) + 1, 1)
        out = np.zeros(len(pts), _ffi.SUBSET_DTYPE)
        sums = np.zeros((len(pts), n_cand, 2), np.uint32) if return_sums else None
        self._chk(self.lib.lk_suggest_subset(self._h, C.byref(cfg), len(pts), _ffi.fptr(pts), out.ctypes.data_as(C.c_void_p),
                                             sums.ctypes.data_as(C.c_void_p) if return_sums else None))
        return (out, sums) if return_sums else out

    def pattern_last(self):
        """Bench hook: (device ms, pixels per pass of the row step, rows per band of the column step, table build ms, query
        ms) of the last pattern_quality or suggest_subset call (the last two 0 after pattern_quality)."""
        ms, build, query = C.c_float(), C.c_float(), C.c_float()
        tile, band = C.c_int(), C.c_int()
        fn = self.lib.lk_internal_pattern_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float),
                       C.POINTER(C.c_float)]
        self._chk(fn(self._h, C.byref(ms), C.byref(tile), C.byref(band), C.byref(build), C.byref(query)))
        return ms.value, tile.value, band.value, build.value, query.value

    @staticmethod
    def pattern_from_sums(n, sums9, mig_sum, noise_sigma=1.0, max_saturated=1.0):
        """lk_pattern_from_sums: the kernel's record arithmetic on the host (no engine needed)."""
        return _ffi.pattern_from_sums(n, sums9, mig_sum, noise_sigma, max_saturated)

    # ---- camera noise: the photon-transfer curve from static frames ---------------------------------------
    @staticmethod
    def _noise_config(slots, ring_first, n_frames, region=None, grey_low=0, grey_high=255, min_count=2):
        cfg = _ffi.LkNoiseConfig()
        if ring_first is None:
            s = [int(k) for k in slots]
            cfg.source, cfg.n_frames = _ffi.NOISE_IMAGES, len(s)
            for i, k in enumerate(s[:3]):
                cfg.slots[i] = k
        else:
            cfg.source, cfg.n_frames, cfg.first = _ffi.NOISE_RING, int(n_frames), int(ring_first)
        if region is not None:
            cfg.x0, cfg.y0, cfg.x1, cfg.y1 = (int(k) for k in region)
        cfg.grey_low, cfg.grey_high, cfg.min_count = int(grey_low), int(grey_high), int(min_count)
        return cfg

    def camera_noise(self, slots=(_ffi.IMG_UND, _ffi.IMG_DEF), ring_first=None, n_frames=None, region=None, mask=None,
                     grey_low=0, grey_high=255, min_count=2, return_tables=False):
        """lk_camera_noise: the NOISE_DTYPE record (pooled temporal variance, flicker, detrended variance, the line var(g) =
        a + b g) of K static frames at level py_start - the image slots `slots` (2 or 3 of them) or, with ring_first, the
        ring slots ring_first .. ring_first + n_frames - 1 - over `region` (x0, y0, x1, y1 inclusive; None: the whole frame)
        and the nonzero pixels of `mask` ([rows][cols] of that level).  With return_tables also the int64 tables bins
        [256][2] {count, sum q} and frame_sums [K].  Needs no sectors; no engine state changes."""
        cfg = self._noise_config(slots, ring_first, n_frames, region, grey_low, grey_high, min_count)
        m = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        if m is not None and ring_first is None:   # (the library cannot see the size of a caller's mask)
            r, c = C.c_int(), C.c_int()
            self._chk(self.lib.lk_get_pyramid_level(self._h, cfg.slots[0], self.cfg.py_start, None, C.byref(r), C.byref(c)))
            assert m.shape == (r.value, c.value), f"mask {m.shape} on level-py_start frames {(r.value, c.value)}"
        assert m is None or m.ndim == 2
        out = np.zeros(1, _ffi.NOISE_DTYPE)
        bins = np.zeros((_ffi.NOISE_BINS, 2), np.int64) if return_tables else None
        sums = np.zeros(max(cfg.n_frames, 1), np.int64) if return_tables else None
        self._chk(self.lib.lk_camera_noise(self._h, C.byref(cfg), m.ctypes.data_as(C.c_void_p) if m is not None else None,
                                           out.ctypes.data_as(C.c_void_p),
                                           bins.ctypes.data_as(C.c_void_p) if return_tables else None,
                                           sums.ctypes.data_as(C.c_void_p) if return_tables else None))
        return (out[0], bins, sums) if return_tables else out[0]

    def sector_noise(self, slots=(_ffi.IMG_UND, _ffi.IMG_DEF), ring_first=None, n_frames=None, return_sums=False):
        """lk_sector_noise: a SECTOR_NOISE_DTYPE array [S], the temporal noise of the same K frames over every committed
        sector's own level-py_start samples (those outside the frame are not counted); with return_sums also the int64 sums
        [S][3] {n, sum q, sum s1}.  No engine state changes."""
        cfg = self._noise_config(slots, ring_first, n_frames)
        out = np.zeros(self.n_sectors, _ffi.SECTOR_NOISE_DTYPE)
        sums = np.zeros((self.n_sectors, _ffi.NOISE_SUMS), np.int64) if return_sums else None
        self._chk(self.lib.lk_sector_noise(self._h, C.byref(cfg), out.ctypes.data_as(C.c_void_p),
                                           sums.ctypes.data_as(C.c_void_p) if return_sums else None))
        return (out, sums) if return_sums else out

    def noise_last(self):
        """Bench hook: (device ms, workgroups of the frame kernel) of the last camera_noise or sector_noise call (0
        workgroups after sector_noise)."""
        ms, wg = C.c_float(), C.c_int()
        fn = self.lib.lk_internal_noise_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        self._chk(fn(self._h, C.byref(ms), C.byref(wg)))
        return ms.value, wg.value

    @staticmethod
    def noise_from_bins(n_frames, bins, frame_sums, grey_low=0, grey_high=255, min_count=2):
        """lk_noise_from_bins: the record of the tables on the host (no engine needed)."""
        return _ffi.noise_from_bins(n_frames, bins, frame_sums, grey_low, grey_high, min_count)

    @staticmethod
    def noise_from_sums(n_frames, sums3):
        """lk_noise_from_sums: a sector's record from its three sums on the host (no engine needed)."""
        return _ffi.noise_from_sums(n_frames, sums3)

    # ---- field map: dense displacement and strain maps on a regular grid of nodes ------------------------
    def field_map(self, radius, window, stride=1, channels=("u", "v"), weight=_ffi.FIELD_UNIFORM, frame=_ffi.FIELD_REFERENCE,
                  iterations=4, records=None, chi_max=0.0, min_neighbours=3, tensor=_ffi.STRAIN_GREEN_LAGRANGE,
                  want=("neighbours", "status")):
        """lk_field_map: the windowed (optionally bisquare-weighted) plane fit of the good sectors at every node
        (x0 + i stride, y0 + j stride) of window = (x0, y0, nx, ny), level-0 pixels, in the reference frame or - frame =
        FIELD_DEFORMED, `iterations` fixed-point steps - at the material point that moved onto the node.  channels: names of
        FIELD_CHANNELS or a mask of FIELD_* bits.  Returns a dict: every selected channel by name as float32 [ny][nx] (NaN
        where a node has no fit), plus "neighbours" int32 [ny][nx] and "status" uint8 [ny][nx] (those named in `want`).  No
        engine state changes."""
        if isinstance(channels, int):
            mask = int(channels)
        else:
            mask = 0
            for name in channels:
                mask |= 1 << _ffi.FIELD_CHANNELS.index(name)
        x0, y0, nx, ny = (int(t) for t in window)
        cfg = _ffi.LkFieldMapConfig(float(radius), float(chi_max), int(min_neighbours), int(tensor), int(weight), int(frame),
                                    int(iterations), x0, y0, nx, ny, int(stride), mask & 0xffffffff)
        names = [k for i, k in enumerate(_ffi.FIELD_CHANNELS) if mask >> i & 1]
        shape = (max(ny, 0), max(nx, 0))
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(self.n_sectors)
        maps = np.zeros((len(names),) + shape, np.float32) if names else None
        nbrs = np.zeros(shape, np.int32) if "neighbours" in want else None
        status = np.zeros(shape, np.uint8) if "status" in want else None

        def ptr(a):
            return a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.lib.lk_field_map(self._h, C.byref(cfg), ptr(rec), ptr(maps), ptr(nbrs), ptr(status)))
        out = {k: maps[c] for c, k in enumerate(names)}
        if nbrs is not None:
            out["neighbours"] = nbrs
        if status is not None:
            out["status"] = status
        return out

    def field_last(self):
        """Bench hook: (device ms, node tiles, tiles that walked global memory) of the last field_map call."""
        ms, tiles, fb = C.c_float(), C.c_int(), C.c_int()
        fn = self.lib.lk_internal_field_last
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._chk(fn(self._h, C.byref(ms), C.byref(tiles), C.byref(fb)))
        return ms.value, tiles.value, fb.value

    @staticmethod
    def field_from_sums(min_neighbours, n, W, sums11, tensor=_ffi.STRAIN_GREEN_LAGRANGE):
        """lk_field_from_sums: the kernel's fit of one node on the host (no engine needed)."""
        return _ffi.field_from_sums(min_neighbours, n, W, sums11, tensor)

    # ---- material-point tracks: chosen points carried through a solved sequence --------------------------
    def track_points(self, points, radius, n_frames=None, records=None, mode=_ffi.TRACK_TOTAL, source=None, state=None,
                     chi_max=0.0, min_neighbours=3, tensor=_ffi.STRAIN_GREEN_LAGRANGE):
        """lk_track_points: (TRACK_DTYPE array [F][Q], state float64 [Q][8]).  points [Q][2] start fresh; points None
        continues from `state` (the second value of an earlier call).  source None: TRACK_RECORDS_CALLER when records
        [F][S] are given, else TRACK_RECORDS_ENGINE (the last batch solve, one frame); TRACK_RECORDS_WINDOW reads the device
        records of the last waited-for window in place.  No engine state changes."""
        if source is None:
            source = _ffi.TRACK_RECORDS_CALLER if records is not None else _ffi.TRACK_RECORDS_ENGINE
        S = self.n_sectors
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(-1, S)
            if n_frames is None:
                n_frames = rec.shape[0]
            elif int(n_frames) > rec.shape[0]:
                raise ValueError("track_points: fewer frames of records than n_frames")
        elif source == _ffi.TRACK_RECORDS_WINDOW and not n_frames:
            # (0 / None: the window's own frame count, which sizes the output; with no window launched by this object the
            # library is asked for 0 frames, refuses for want of a window and writes nothing)
            n_frames = self._seq_frames
            if n_frames == 0 and self.lib.lk_get_sequence_results_device(self._h, None, None) == 0:
                raise ValueError("track_points: a window this object did not launch is held; pass its n_frames")
        elif n_frames is None:
            n_frames = 1
        pts = None
        if points is not None:
            pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
            st = np.zeros((len(pts), 8), np.float64)
        elif state is None:
            raise ValueError("track_points: neither points nor a state to continue from")
        else:
            st = np.array(state, np.float64).reshape(-1, 8)
        cfg = _ffi.LkTrackConfig(float(radius), float(chi_max), int(min_neighbours), int(tensor), int(mode), int(source))
        out = np.zeros((max(int(n_frames), 0), len(st)), _ffi.TRACK_DTYPE)
        self._chk(self.lib.lk_track_points(self._h, C.byref(cfg), len(st), _ffi.fptr(pts) if pts is not None else None,
                                           int(n_frames), rec.ctypes.data_as(C.c_void_p) if rec is not None else None,
                                           st.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out, st

    @staticmethod
    def track_step(mode, min_neighbours, n, sums11, state8, tensor=_ffi.STRAIN_GREEN_LAGRANGE):
        """lk_track_step: the kernel's per-frame function on the host (no engine needed)."""
        return _ffi.track_step(mode, min_neighbours, n, sums11, state8, tensor)

    @staticmethod
    def gauges_from_tracks(tracks, pairs):
        """lk_gauges_from_tracks: virtual extensometers between tracked points (host, no engine needed)."""
        return _ffi.gauges_from_tracks(tracks, pairs)

    # ---- global motion: the motion of a frame as a whole, and the records without it ---------------------
    def rigid_motion(self, kind=_ffi.MOTION_RIGID, n_frames=None, records=None, source=None, fit_mask=None, reject=0.0,
                     passes=1, chi_max=0.0, min_sectors=None, return_records=False, return_sums=False):
        """lk_rigid_motion: the MOTION_DTYPE array [F]; with return_records and / or return_sums a tuple (motion, the records
        [F][S] with the motion taken out, float64 [F][12] = the fit set's count and 11 sums), the parts asked for in that
        order.  source None: TRACK_RECORDS_CALLER when records [F][S] are given, else TRACK_RECORDS_ENGINE (the last batch
        solve, one frame); TRACK_RECORDS_WINDOW reads the device records of the last waited-for window in place.  fit_mask [S]:
        the sectors that may enter the fit.  min_sectors None: the kind's minimum.  No engine state changes."""
        if source is None:
            source = _ffi.TRACK_RECORDS_CALLER if records is not None else _ffi.TRACK_RECORDS_ENGINE
        S = self.n_sectors
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(-1, S)
            if n_frames is None:
                n_frames = rec.shape[0]
            elif int(n_frames) > rec.shape[0]:
                raise ValueError("rigid_motion: fewer frames of records than n_frames")
        elif source == _ffi.TRACK_RECORDS_WINDOW and not n_frames:
            # (as track_points: the window's own frame count sizes the outputs)
            n_frames = self._seq_frames
            if n_frames == 0 and self.lib.lk_get_sequence_results_device(self._h, None, None) == 0:
                raise ValueError("rigid_motion: a window this object did not launch is held; pass its n_frames")
        elif n_frames is None:
            n_frames = 1
        mask = None
        if fit_mask is not None:
            mask = np.ascontiguousarray(np.asarray(fit_mask) != 0, np.uint8).reshape(-1)
            if len(mask) != S:
                raise ValueError("rigid_motion: fit_mask must have one entry per sector")
        if min_sectors is None:
            min_sectors = _ffi.MOTION_MIN_SECTORS.get(int(kind), 1)
        cfg = _ffi.LkMotionConfig(int(kind), int(source), float(chi_max), float(reject), int(passes), int(min_sectors))
        F = max(int(n_frames), 0)
        out = np.zeros(F, _ffi.MOTION_DTYPE)
        rec_out = np.zeros((F, S), RESULT_DTYPE) if return_records else None
        sums = np.zeros((F, 12), np.float64) if return_sums else None

        def ptr(a):
            return a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.lib.lk_rigid_motion(self._h, C.byref(cfg), int(n_frames), ptr(rec), ptr(mask), ptr(out), ptr(rec_out),
                                           ptr(sums)))
        if not return_records and not return_sums:
            return out
        return (out,) + ((rec_out,) if return_records else ()) + ((sums,) if return_sums else ())

    def motion_last(self):
        """Bench hook: (device ms, chunk size, chunks per frame) of the last rigid_motion call."""
        ms, chunk, chunks = C.c_float(), C.c_int(), C.c_int()
        fn = self.lib.lk_internal_motion_last
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._chk(fn(self._h, C.byref(ms), C.byref(chunk), C.byref(chunks)))
        return ms.value, chunk.value, chunks.value

    @staticmethod
    def motion_from_sums(kind, n, sums11, origin_xy, min_sectors=None):
        """lk_motion_from_sums: the kernel's fit on the host (no engine needed)."""
        return _ffi.motion_from_sums(kind, n, sums11, origin_xy, min_sectors)

    @staticmethod
    def motion_apply(motion, xy):
        """lk_motion_apply: the displacement field of a motion at positions (host, no engine needed)."""
        return _ffi.motion_apply(motion, xy)

    @staticmethod
    def motion_remove(model, motion, centers, records, good=None):
        """lk_motion_remove: the kernel's removal on the host (no engine needed)."""
        return _ffi.motion_remove(model, motion, centers, records, good)

    # ---- lens distortion (include/lk_engine.h: lk_lens_fit, lk_lens_correct) -------------
    def _lens_records(self, who, n_frames, records, source):
        """the records / n_frames / source arguments shared by lens_fit and lens_correct, as rigid_motion's"""
        if source is None:
            source = _ffi.TRACK_RECORDS_CALLER if records is not None else _ffi.TRACK_RECORDS_ENGINE
        S = self.n_sectors
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(-1, S)
            if n_frames is None:
                n_frames = rec.shape[0]
            elif int(n_frames) > rec.shape[0]:
                raise ValueError(who + ": fewer frames of records than n_frames")
        elif source == _ffi.TRACK_RECORDS_WINDOW and not n_frames:
            n_frames = self._seq_frames
            if n_frames == 0 and self.lib.lk_get_sequence_results_device(self._h, None, None) == 0:
                raise ValueError(who + ": a window this object did not launch is held; pass its n_frames")
        elif n_frames is None:
            n_frames = 1
        return int(source), int(n_frames), rec

    def lens_default(self):
        """The start of lens_fit: the centre of the bounding box of the committed centres, rn = half its diagonal, no
        distortion (a LENS_DTYPE record)."""
        c = np.float32([self.sector_info(s)[1:] for s in range(self.n_sectors)]).astype(np.float64)
        lo, hi = c.min(axis=0), c.max(axis=0)
        return _ffi.make_lens((lo[0] + hi[0]) / 2.0, (lo[1] + hi[1]) / 2.0, float(np.hypot(*(hi - lo))) / 2.0)

    def lens_fit(self, free=_ffi.LENS_FREE_K1, nuisance=_ffi.LENS_TRANSLATION, init=None, n_frames=None, records=None, source=None,
                 fit_mask=None, chi_max=0.0, min_sectors=None, max_iters=10, tol=1e-8, return_frames=False, return_sums=False):
        """lk_lens_fit: the lens from records of a rigidly shifted specimen -> one LENS_RESULT_DTYPE record; with return_frames
        and / or return_sums a tuple (result, LENS_FRAME_DTYPE [F], float64 [2][F][lens_sums_len(nuisance)] = the sums of the
        first and of the last evaluation), the parts asked for in that order.  free: LENS_FREE_* bits; init None:
        lens_default().  records / source / n_frames as rigid_motion.  min_sectors None: the nuisance's Q.  No engine state
        changes."""
        source, n_frames, rec = self._lens_records("lens_fit", n_frames, records, source)
        S = self.n_sectors
        mask = None
        if fit_mask is not None:
            mask = np.ascontiguousarray(np.asarray(fit_mask) != 0, np.uint8).reshape(-1)
            if len(mask) != S:
                raise ValueError("lens_fit: fit_mask must have one entry per sector")
        if init is None:
            init = self.lens_default()
        lens = np.ascontiguousarray(init, _ffi.LENS_DTYPE).reshape(1)
        if min_sectors is None:
            min_sectors = _ffi.LENS_Q.get(int(nuisance), 2)
        cfg = _ffi.LkLensFitConfig(source, float(chi_max), int(min_sectors), int(free), int(nuisance), int(max_iters), float(tol))
        F = max(n_frames, 0)
        out = np.zeros(1, _ffi.LENS_RESULT_DTYPE)
        frames = np.zeros(F, _ffi.LENS_FRAME_DTYPE) if return_frames else None
        sums = np.zeros((2, F, _ffi.lens_sums_len(nuisance)), np.float64) if return_sums and int(nuisance) in _ffi.LENS_Q else None

        def ptr(a):
            return a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.lib.lk_lens_fit(self._h, C.byref(cfg), ptr(lens), n_frames, ptr(rec), ptr(mask), ptr(out), ptr(frames), ptr(sums)))
        if not return_frames and not return_sums:
            return out[0]
        return (out[0],) + ((frames,) if return_frames else ()) + ((sums,) if return_sums else ())

    def lens_correct(self, lens, n_frames=None, records=None, source=None, chi_max=0.0, return_centres=False, return_status=False):
        """lk_lens_correct: the records [F][S] with the lens (a LENS_DTYPE record) taken out; with return_centres and / or
        return_status a tuple (records, float32 [S][2] = U(centre), uint8 [F][S] = LENS_CORRECTED / _NOT_GOOD / _OUTSIDE), the
        parts asked for in that order.  records / source / n_frames as rigid_motion.  No engine state changes."""
        source, n_frames, rec = self._lens_records("lens_correct", n_frames, records, source)
        S = self.n_sectors
        one = np.ascontiguousarray(lens, _ffi.LENS_DTYPE).reshape(1)
        cfg = _ffi.LkLensConfig(source, float(chi_max))
        F = max(n_frames, 0)
        out = np.zeros((F, S), RESULT_DTYPE)
        cen = np.zeros((S, 2), np.float32) if return_centres else None
        status = np.zeros((F, S), np.uint8) if return_status else None

        def ptr(a):
            return a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.lib.lk_lens_correct(self._h, C.byref(cfg), ptr(one), n_frames, ptr(rec), ptr(out), ptr(cen), ptr(status)))
        if not return_centres and not return_status:
            return out
        return (out,) + ((cen,) if return_centres else ()) + ((status,) if return_status else ())

    def lens_last(self):
        """Bench hook: (device ms, chunk size, chunks per frame, evaluations, ms of the last evaluation's kernels) of the last
        lens_fit or lens_correct call."""
        ms, chunk, chunks, evals, eval_ms = C.c_float(), C.c_int(), C.c_int(), C.c_int(), C.c_float()
        fn = self.lib.lk_internal_lens_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]
        self._chk(fn(self._h, C.byref(ms), C.byref(chunk), C.byref(chunks), C.byref(evals), C.byref(eval_ms)))
        return ms.value, chunk.value, chunks.value, evals.value, eval_ms.value

    # ---- a two-camera rig (include/lk_engine.h: lk_stereo_points, lk_stereo_strain) ---------
    def stereo_points(self, cams, ref1, rec0=None, rec1=None, chi_max=0.0):
        """lk_stereo_points: cams = two CAMERA_DTYPE records; ref1 [S] = camera 0 reference -> camera 1 reference; rec0, rec1
        [F][S] = camera 0 reference -> frame f of camera 0 / of camera 1 (both None: the shape alone) -> (STEREO_POINT_DTYPE [S]
        of the reference state, STEREO_POINT_DTYPE [F][S]).  The points stay on the device for stereo_strain().  No engine state
        changes."""
        S = self.n_sectors
        rig = _ffi._rig(cams)
        ref1 = np.ascontiguousarray(ref1, RESULT_DTYPE).reshape(-1)
        if (rec0 is None) != (rec1 is None):
            raise ValueError("stereo_points: rec0 and rec1 must both be given or both be None")
        if rec0 is not None:
            rec0, rec1 = np.ascontiguousarray(rec0, RESULT_DTYPE), np.ascontiguousarray(rec1, RESULT_DTYPE)
            rec0, rec1 = rec0.reshape(-1, rec0.shape[-1]), rec1.reshape(-1, rec1.shape[-1])
            if rec0.shape != rec1.shape or rec0.shape[1] != S:
                raise ValueError("stereo_points: rec0 and rec1 must both be [n_frames][n_sectors]")
        if len(ref1) != S:
            raise ValueError("stereo_points: ref1 must have one record per sector")
        F = 0 if rec0 is None else len(rec0)
        ref_out = np.zeros(S, _ffi.STEREO_POINT_DTYPE)
        out = np.zeros((F, S), _ffi.STEREO_POINT_DTYPE)
        cfg = _ffi.LkStereoConfig(0.0, float(chi_max), 0, 0)

        def ptr(a):
            return a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.lib.lk_stereo_points(self._h, C.byref(cfg), ptr(rig), ptr(ref1), F, ptr(rec0), ptr(rec1), ptr(ref_out),
                                            ptr(out) if F else None))
        return ref_out, out

    def stereo_strain(self, radius, ref_points=None, points=None, n_frames=None, min_neighbours=3):
        """lk_stereo_strain: the strain of the surface through the 3-D points, per (frame, sector) -> STEREO_SURFACE_DTYPE [F][S].
        ref_points [S] and points [F][S] (both None: the points the last stereo_points left on the device, whose frame count
        n_frames then defaults to).  No engine state changes."""
        S = self.n_sectors
        if (ref_points is None) != (points is None):
            raise ValueError("stereo_strain: ref_points and points must both be given or both be None")
        if points is not None:
            ref_points = np.ascontiguousarray(ref_points, _ffi.STEREO_POINT_DTYPE).reshape(-1)
            points = np.ascontiguousarray(points, _ffi.STEREO_POINT_DTYPE)
            points = points.reshape(-1, points.shape[-1])
            if len(ref_points) != S or points.shape[1] != S:
                raise ValueError("stereo_strain: ref_points must be [n_sectors] and points [n_frames][n_sectors]")
            if n_frames is None:
                n_frames = len(points)
            elif n_frames != len(points):
                raise ValueError("stereo_strain: n_frames differs from the frames of points")
        elif n_frames is None:
            n_frames = self.stereo_last()[3]
        F = max(int(n_frames), 0)
        out = np.zeros((F, S), _ffi.STEREO_SURFACE_DTYPE)
        cfg = _ffi.LkStereoConfig(float(radius), 0.0, int(min_neighbours), 0)

        def ptr(a):
            return a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.lib.lk_stereo_strain(self._h, C.byref(cfg), int(n_frames), ptr(ref_points), ptr(points), ptr(out)))
        return out

    def stereo_last(self):
        """Bench hook: (device ms, lane group, expected members of a sector's 3 x 3 cells, frames of the points held on the
        device) of the last stereo_points or stereo_strain call (group and members 0 after stereo_points)."""
        ms, group, members, held = C.c_float(), C.c_int(), C.c_double(), C.c_int()
        fn = self.lib.lk_internal_stereo_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        self._chk(fn(self._h, C.byref(ms), C.byref(group), C.byref(members), C.byref(held)))
        return ms.value, group.value, members.value, held.value

    # ---- stand-alone pieces -------------------------------------------------------------
    def evaluate(self, sector, level, p):
        pp = np.zeros(6, np.float32)
        pp[:len(p)] = p
        A = np.zeros((6, 6), np.float32)
        b = np.zeros(6, np.float32)
        chi, err = C.c_float(), C.c_int()
        self._chk(self.lib.lk_evaluate(self._h, sector, level, _ffi.fptr(pp), _ffi.fptr(A),
                                       _ffi.fptr(b), C.byref(chi), C.byref(err)))
        return A, b, chi.value, err.value

    def evaluate_backward(self, sector, level, p):
        """Template pass + one backward-mode evaluation: H (6x6, full), b, chi (unscaled), error."""
        pp = np.zeros(6, np.float32)
        pp[:len(p)] = p
        H = np.zeros((6, 6), np.float32)
        b = np.zeros(6, np.float32)
        chi, err = C.c_float(), C.c_int()
        self._chk(self.lib.lk_evaluate_backward(self._h, sector, level, _ffi.fptr(pp), _ffi.fptr(H),
                                                _ffi.fptr(b), C.byref(chi), C.byref(err)))
        return H, b, chi.value, err.value

    def sample(self, slot, level, xy):
        a = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.zeros((a.shape[0], 4), np.float32)
        self._chk(self.lib.lk_sample(self._h, slot, level, _ffi.fptr(a), a.shape[0], _ffi.fptr(out)))
        return out

    def damped_solve(self, A, b, lam, scaling, reference_solver=False):
        A = np.ascontiguousarray(A, np.float32)
        n = A.shape[0]
        b = np.ascontiguousarray(b, np.float32)
        dp = np.zeros(n, np.float32)
        self._chk(self.lib.lk_damped_solve(self._h, n, _ffi.fptr(A), _ffi.fptr(b), lam, scaling,
                                           int(reference_solver), _ffi.fptr(dp)))
        return dp

    def step_compare(self, systems):
        """[n][40] float32 (28 sums, lambda, scaling, p[6], 4 unused) -> [n][2][16]: x[6], p[6], flag, ... of the register
        solver and of the scattered one (include/lk_engine.h: lk_step_compare)."""
        a = np.ascontiguousarray(systems, np.float32).reshape(-1, 40)
        out = np.zeros((a.shape[0], 2, 16), np.float32)
        self._chk(self.lib.lk_step_compare(self._h, a.shape[0], _ffi.fptr(a), _ffi.fptr(out)))
        return out

    def reduce_compare(self, lanes, wide=False):
        """[n][64][28] float32 partial sums -> [n][2][64][28]: all-reduce and reduce-scatter totals in every lane."""
        a = np.ascontiguousarray(lanes, np.float32).reshape(-1, 64, 28)
        out = np.zeros((a.shape[0], 2, 64, 28), np.float32)
        self._chk(self.lib.lk_reduce_compare(self._h, a.shape[0], int(bool(wide)), _ffi.fptr(a), _ffi.fptr(out)))
        return out

    def stats(self):
        s = LkStats()
        self._chk(self.lib.lk_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in LkStats._fields_}

    def sector_stats(self):
        """[S][4] uint32 of the last solve: evaluations, sample evaluations, point iterations, ill-conditioned solves."""
        out = np.zeros((self.n_sectors, 4), np.uint32)
        self._chk(self.lib.lk_get_sector_stats(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def launch_report(self):
        """The kernel launches of the most recent solving call (correlate, correlate_all*, a sequence window, evaluate,
        evaluate_backward) in launch order: a list of dicts with the fields of lk_launch_record (include/lk_engine.h) but
        `reserved`.  Raises if the call made more launches than the engine keeps."""
        rec = (_ffi.LkLaunchRecord * _ffi.LAUNCH_REPORT_CAPACITY)()
        n, over = C.c_int(), C.c_int()
        self._chk(self.lib.lk_get_launch_report(self._h, rec, _ffi.LAUNCH_REPORT_CAPACITY, C.byref(n), C.byref(over)))
        if over.value:
            raise RuntimeError(f"launch report overflow: more than {_ffi.LAUNCH_REPORT_CAPACITY} launches in one call")
        return [{k: getattr(rec[i], k) for k, _ in _ffi.LkLaunchRecord._fields_ if k != "reserved"} for i in range(n.value)]

    def sector_groups(self):
        """(groups, team_w), int32 [S] each: lanes per sector of the next one-pair batch solve and, for a sector of the team
        class (512 lanes), the workgroups per sector the engine asks for (lk_get_sector_groups)."""
        groups, team = np.zeros(self.n_sectors, np.int32), np.zeros(self.n_sectors, np.int32)
        self._chk(self.lib.lk_get_sector_groups(self._h, groups.ctypes.data_as(C.POINTER(C.c_int)),
                                                team.ctypes.data_as(C.POINTER(C.c_int))))
        return groups, team
