#!/usr/bin/env python3
"""Every output of the add-on passes and of the backward solve on one seeded scene, for comparing two builds of the
library byte for byte - the check behind a change of the passes' device code that must not change a result.

    LK_ENGINE_LIB=/path/to/liblk_engine.so python scripts/pass_outputs.py OUT.npz     (LK_ENGINE_LIB unset: the tree's own)
    python scripts/pass_outputs.py --compare A.npz B.npz                              (exit status 1 if any array differs)

Two scenes of one 256 x 256 speckle pair: `mix`, the sectors of tests/test_uncertainty_gpu.py (361, 49, 899 and 10000
samples and an annular list: 16, 64 and 512 lanes all occur), and `grid`, 24 x 24 rectangular sectors for the passes that
look for neighbours.  Both are solved once; then a few records are made bad (an error code, a NaN parameter, an infinite
chi) and one u becomes -0.  Every variant below runs in a child process of its own - the lane group and the variant of a
pass are chosen by environment variables that the library reads per call, and a fault must not reach the next one - under
a time limit, and the first failure ends the run.  The arrays of all variants go into one .npz, `variant/array`.

The `solve_all_*`, `correlate_one*`, `window_*` and `reseed_failed` variants are the engine's own launch paths - for a change of
the host side of the solve (lk_engine_solve.cpp, lk_engine_sequence.cpp) that must not change a record: lk_correlate_all of
`mix` in every mode, without class streams and with forced teams; lk_correlate on each of its sectors; one window of four
frames (`mix_small`: mix without the 10 000-sample rectangle, so that it is frame-pipelined; `grid` with a starved level);
a recovery pass that re-solves a sector subset.  `--only REGEX` runs some of the variants.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRUTH = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)
RECTS = [(8, 8, 26, 26), (40, 8, 46, 14), (8, 60, 38, 88), (140, 140, 239, 239)]
ANNULAR = [(20.0, 12.0, 0.3, 0.9, 70.0, 190.0, 6)]
RADIUS = 25.0        # 2.5 pitches of the grid: windows of about 20 sectors
TINY_RADIUS = 4.0    # less than a pitch: every window is TOO_FEW
WIDE_RADIUS = 300.0  # one cell holds the whole grid, 576 sectors: more than a tile of the map keeps in LDS, so it falls back
CHILD_SECONDS = 180


def solved(scene, model, interp, update=None):
    """(engine, records of its solve with a few made bad)"""
    import correlation_amd as ca
    und, dfm = ca.speckle.speckle_pair(256, 256, p=TRUTH, seed=5)
    e = ca.HipCorrelationEngine(interpolation=interp, fitting_model=model, precision=1e-3, py_stop=2)
    if update is not None:
        e.set_update(update)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    if scene == "mix":
        for s, r in enumerate(RECTS):
            e.resetPolygon_rect(s, *r)
        for k, q in enumerate(ANNULAR):
            e.resetPolygon_annular(len(RECTS) + k, *q)
    else:
        e.set_rect_grid(8.0, 8.0, 247.0, 247.0, 24, 24)
    e.commit_sectors()
    g = np.zeros((e.n_sectors, 6), np.float32)
    g[:, :2] = TRUTH[:2]
    rec = e.correlate_all(g).copy()
    S = e.n_sectors
    if scene == "mix":
        rec["error_code"][1] = 3
    else:
        rec["error_code"][np.arange(7, S, 37)] = 3
        rec["p"][45, 1] = np.nan
        rec["chi"][210] = np.inf
        rec["p"][101, 0] = -0.0
    return e, rec


def fields(prefix, a):
    """a structured array as one plain array per field"""
    return {prefix + "." + k: np.ascontiguousarray(a[k]) for k in a.dtype.names}


def run_strain():
    import correlation_amd as ca
    e, rec = solved("grid", ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
    out = fields("records", rec)
    out.update(fields("strain", e.strain_field(RADIUS, records=rec)))
    out.update(fields("strain_chi_max", e.strain_field(RADIUS, chi_max=float(np.median(rec["chi"])), records=rec)))
    out.update(fields("strain_too_few", e.strain_field(TINY_RADIUS, records=rec)))
    return out


def run_outlier():
    import correlation_amd as ca
    e, rec = solved("grid", ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
    rec["p"][[88, 301], 0] += 0.7   # two sectors to flag
    out = {}
    for name, kw in (("detrend", dict(detrend=True, passes=2)), ("plain", dict(detrend=False)),
                     ("too_few", dict(detrend=True, radius=TINY_RADIUS))):
        kw.setdefault("radius", RADIUS)
        flags, n, marked = e.flag_outliers(mark=True, records=rec, return_records=True, **kw)
        out.update(fields("outlier_" + name, flags))
        out["outlier_" + name + ".flagged"] = np.array([n])
        out["outlier_" + name + ".error_code"] = marked["error_code"].copy()
    return out


def run_track():
    import correlation_amd as ca
    e, rec = solved("grid", ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
    frames = np.stack([rec.copy() for _ in range(3)])
    for f in range(3):   # frame f: f + 1 times the solved field
        frames["p"][f] *= np.float32(f + 1)
    frames["error_code"][1][60:64] = 3
    rng = np.random.default_rng(11)
    pts = rng.uniform(0.0, 255.0, (61, 2)).astype(np.float32)
    pts[0] = (-400.0, 90.0)   # far off the grid in x: no cell at all
    pts[1] = (90.0, 700.0)    # ... in y
    pts[2] = (-20.0, -20.0)   # one cell beyond the grid: its range still reaches the corner cells
    pts[3] = (np.nan, 50.0)
    out = {}
    for mode, name in ((ca._ffi.TRACK_TOTAL, "total"), (ca._ffi.TRACK_INCREMENTAL, "incremental")):
        for radius, tag in ((RADIUS, ""), (TINY_RADIUS, "_too_few")):
            tr, st = e.track_points(pts, radius, records=frames, mode=mode)
            out.update(fields("track_" + name + tag, tr))
            out["track_" + name + tag + ".state"] = st
    return out


def run_motion():
    import correlation_amd as ca
    e, rec = solved("grid", ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
    frames = np.stack([rec.copy() for _ in range(3)])
    for f in range(3):   # frame f: f + 1 times the solved field
        frames["p"][f] *= np.float32(f + 1)
    frames["error_code"][1][60:64] = 3
    frames["p"][2][[88, 301], 0] += 5.0   # two sectors for the second pass to trim
    mask = np.arange(e.n_sectors) % 24 < 6
    out = {}
    for kind, name in enumerate(("translation", "rigid", "similarity", "affine")):
        for tag, kw in (("", {}), ("_masked", dict(fit_mask=mask)), ("_trimmed", dict(reject=3.0, passes=2)),
                        ("_too_few", dict(min_sectors=e.n_sectors + 1))):
            m, removed, sums = e.rigid_motion(kind, records=frames, return_records=True, return_sums=True, **kw)
            out.update(fields("motion_" + name + tag, m))
            out.update(fields("motion_" + name + tag + ".records", removed))
            out["motion_" + name + tag + ".sums"] = sums
    return out


def run_lens():
    import correlation_amd as ca
    e, rec = solved("grid", ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
    start = e.lens_default()
    true = ca.make_lens(start["cx"] + 5.0, start["cy"] - 4.0, start["rn"], -0.03, 0.008)
    cen = np.float32([e.sector_info(s)[1:] for s in range(e.n_sectors)]).astype(np.float64)
    seen = ca.lens_undistort(true, cen)
    frames = np.stack([rec.copy() for _ in range(4)])
    for f, t in enumerate(((12.0, 0.0), (-12.0, 0.0), (0.0, 9.0), (8.0, -6.0))):   # a shifted specimen seen through the lens
        frames["p"][f][:, :2] = ca.lens_distort(true, seen + np.float64(t)) - cen
    frames["error_code"][1][60:64] = 3
    mask = np.arange(e.n_sectors) % 24 < 18
    out = {}
    four = ca.LENS_FREE_K1 | ca.LENS_FREE_K2 | ca.LENS_FREE_CENTRE
    for nuisance, name, free in ((ca.LENS_TRANSLATION, "translation", four), (ca.LENS_SIMILARITY, "similarity", four),
                                 (ca.LENS_AFFINE, "affine", ca.LENS_FREE_K1 | ca.LENS_FREE_K2)):
        for tag, kw in (("", {}), ("_masked", dict(fit_mask=mask)), ("_too_few", dict(min_sectors=e.n_sectors + 1))):
            fit, per_frame, sums = e.lens_fit(free, nuisance, records=frames, return_frames=True, return_sums=True, **kw)
            out["lens_" + name + tag + ".fit"] = np.frombuffer(fit.tobytes(), np.uint8)
            out["lens_" + name + tag + ".frames"] = np.frombuffer(per_frame.tobytes(), np.uint8)
            out["lens_" + name + tag + ".sums"] = sums
    fixed, centres, status = e.lens_correct(true, records=frames, return_centres=True, return_status=True)
    out.update(fields("lens_correct.records", fixed))
    out["lens_correct.centres"], out["lens_correct.status"] = centres, status
    return out


def run_stereo():
    """a plane Z = 400 + 0.2 X seen by two cameras 20 degrees apart (no calibration involved: the records are exact
    projections), stretched and pushed back a little more in each of three frames"""
    import correlation_amd as ca
    e, rec = solved("grid", ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
    cen = np.float32([e.sector_info(s)[1:] for s in range(e.n_sectors)]).astype(np.float64)
    th = np.deg2rad(20.0)
    R1 = np.float64([[np.cos(th), 0.0, np.sin(th)], [0.0, 1.0, 0.0], [-np.sin(th), 0.0, np.cos(th)]])
    C1 = np.float64([400.0 * np.sin(th), 0.0, 400.0 * (1.0 - np.cos(th))])
    cams = [ca.make_camera(800.0, 800.0, 127.5, 127.5, lens=ca.make_lens(126.0, 117.0, 147.785, -0.03, 0.008)),
            ca.make_camera(800.0, 802.0, 127.5, 125.5, R=R1, t=-R1 @ C1, skew=0.05, lens=ca.make_lens(130.0, 125.0, 150.0, 0.02, 0.0, 1e-3, -5e-4))]
    m = (ca.lens_undistort(cams[0]["lens"], cen) - 127.5) / 800.0          # camera 0's rays (x, y, 1) through the centres
    depth = 400.0 / (1.0 - 0.2 * m[:, 0])
    P = np.stack([m[:, 0] * depth, m[:, 1] * depth, depth], 1)

    def records(pixels, bad):
        out = rec.copy()
        out["p"][:, :2] = (pixels - cen).astype(np.float32)
        out["error_code"][:] = 0
        out["chi"][:] = 0.5
        out["error_code"][bad] = 3
        return out

    frames = [P * [1.0 + 0.01 * k, 1.0 - 0.005 * k, 1.0] + [0.5 * k, 0.0, 2.0 * k] for k in (1, 2, 3)]
    ref1 = records(ca.stereo_project(cams[1], P), [40, 41])
    rec0 = np.stack([records(ca.stereo_project(cams[0], X), [100]) for X in frames])
    rec1 = np.stack([records(ca.stereo_project(cams[1], X), [575]) for X in frames])
    ref_pts, pts = e.stereo_points(cams, ref1, rec0, rec1)
    out = {"stereo.ref_points": np.frombuffer(ref_pts.tobytes(), np.uint8), "stereo.points": np.frombuffer(pts.tobytes(), np.uint8)}
    for name, radius in (("", RADIUS), ("_tiny", TINY_RADIUS)):
        out["stereo.surface" + name] = np.frombuffer(e.stereo_strain(radius).tobytes(), np.uint8)
    out["stereo.surface_caller"] = np.frombuffer(e.stereo_strain(RADIUS, ref_pts, pts).tobytes(), np.uint8)
    return out


def run_plan():
    import correlation_amd as ca
    out = {}
    for model, name in ((ca.FM_UVUXUYVXVY, "affine"), (ca.FM_UVQ, "uvq")):
        e, rec = solved("grid", model, ca.IM_BICUBIC)
        g, info = e.reseed_plan(rec, RADIUS, min_neighbours=2)
        out["plan_" + name + ".guess"] = g
        out.update(fields("plan_" + name, info))
        e.close()
    return out


def run_map():
    import correlation_amd as ca
    e, rec = solved("grid", ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
    out = {}
    for radius, window, name in ((RADIUS, None, "staged"), (WIDE_RADIUS, None, "fallback"), (RADIUS, (3, 5, 77, 41), "window")):
        warped, residual, owner = e.residual_map(radius, window=window, records=rec)
        _, tiles, fallback = e.residual_last()
        assert (fallback > 0) == (name == "fallback"), (name, tiles, fallback)
        out.update({"map_%s.warped" % name: warped, "map_%s.residual" % name: residual, "map_%s.owner" % name: owner,
                    "map_%s.tiles" % name: np.array([tiles, fallback])})
    return out


def run_field():
    import correlation_amd as ca
    e, rec = solved("grid", ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
    out = {}
    window = (-40, -37, 333, 331)   # ragged tiles, two radii beyond the grid
    for name, kw in (("uniform", dict()), ("bisquare", dict(weight=ca.FIELD_BISQUARE)),
                     ("deformed", dict(weight=ca.FIELD_BISQUARE, frame=ca.FIELD_DEFORMED, iterations=4)),
                     ("stride", dict(stride=3)), ("too_few", dict(radius=TINY_RADIUS)), ("wide", dict(radius=WIDE_RADIUS))):
        kw.setdefault("radius", RADIUS)
        got = e.field_map(kw.pop("radius"), window, channels=ca.FIELD_ALL, records=rec, **kw)
        _, tiles, fallback = e.field_last()
        assert fallback == (tiles if os.environ.get("LK_FIELD_WALK") == "1" else 0), (name, tiles, fallback)
        out.update({"field_%s.%s" % (name, k): v for k, v in got.items()})
    return out


def run_evaluate():
    import correlation_amd as ca
    out = {}
    for scene in ("mix", "grid"):
        for model, interp, name in ((ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, "affine_bicubic"), (ca.FM_UV, ca.IM_BILINEAR, "uv_bilinear"),
                                    (ca.FM_UVQ, ca.IM_BICUBIC_SEPARABLE, "uvq_separable"), (ca.FM_U, ca.IM_NEAREST, "u_nearest")):
            e, rec = solved(scene, model, interp)
            unc, usums = e.parameter_uncertainty(records=rec, return_sums=True)
            pho, psums = e.photometry(records=rec, return_sums=True)
            tag = "%s_%s" % (scene, name)
            out.update(fields("uncertainty_" + tag, unc))
            out.update(fields("photometry_" + tag, pho))
            out["uncertainty_" + tag + ".sums"] = usums
            out["photometry_" + tag + ".sums"] = psums
            e.close()
    return out


def run_backward():
    import correlation_amd as ca
    out = {}
    for scene in ("mix", "grid"):
        for model, interp, name in ((ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, "affine_bicubic"), (ca.FM_UV, ca.IM_BILINEAR, "uv_bilinear")):
            e, _ = solved(scene, model, interp, update=ca.UPDATE_BACKWARD)
            g = np.zeros((e.n_sectors, 6), np.float32)
            g[:, :2] = TRUTH[:2]
            out.update(fields("backward_%s_%s" % (scene, name), e.correlate_all(g)))   # (the solve's own records, none made bad)
            e.close()
    return out


def run_pattern():
    import correlation_amd as ca
    out = {}
    rng = np.random.default_rng(13)
    pts = rng.uniform(-3.0, 258.0, (97, 2)).astype(np.float32)
    pts[5] = (np.nan, 40.0)
    for scene in ("mix", "grid"):
        e, _ = solved(scene, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
        for slot, name in ((ca.IMG_UND, "und"), (ca.IMG_DEF, "def")):
            pat, sums, mig = e.pattern_quality(slot=slot, grey_low=20, grey_high=235, noise_sigma=0.75, max_saturated=0.3,
                                               return_sums=True)
            tag = "pattern_%s_%s" % (scene, name)
            out.update(fields(tag, pat))
            out[tag + ".sums"] = sums
            out[tag + ".mig_sum"] = mig
        sub, box = e.suggest_subset(pts, 1e5, 2, 40, 3, return_sums=True)
        out.update(fields("subset_" + scene, sub))
        out["subset_" + scene + ".sums"] = box
        e.close()
    return out


def run_noise():
    import correlation_amd as ca
    out = {}
    for scene in ("mix", "grid"):
        e, _ = solved(scene, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)
        rec, bins, frame_sums = e.camera_noise(grey_low=20, grey_high=235, min_count=5, return_tables=True)
        out.update(fields("noise_" + scene, np.array([rec])))
        out["noise_" + scene + ".bins"] = bins
        out["noise_" + scene + ".frame_sums"] = frame_sums
        sec, sums = e.sector_noise(return_sums=True)
        out.update(fields("sector_noise_" + scene, sec))
        out["sector_noise_" + scene + ".sums"] = sums
        e.close()
    return out


def run_znssd():
    import correlation_amd as ca
    out = {}
    for scene in ("mix", "grid"):
        for model, interp, name in ((ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, "affine_bicubic"), (ca.FM_UV, ca.IM_BILINEAR, "uv_bilinear"),
                                    (ca.FM_UVQ, ca.IM_BICUBIC_SEPARABLE, "uvq_separable"), (ca.FM_U, ca.IM_BICUBIC, "u_bicubic")):
            e, rec = solved(scene, model, interp)
            g = np.zeros((e.n_sectors, 6), np.float32)
            g[:, :2] = TRUTH[:2]
            for seeds, kw in (("records", dict(records=rec)), ("guesses", dict(guesses=g)), ("one_trip", dict(guesses=g, max_iters=1))):
                refined, info, sums = e.refine_znssd(return_sums=True, **kw)
                tag = "znssd_%s_%s_%s" % (scene, name, seeds)
                out.update(fields(tag + ".records", refined))
                out.update(fields(tag, info))
                out[tag + ".sums"] = sums
            e.close()
    return out


def run_spline():
    import correlation_amd as ca
    out = {}
    for scene in ("mix", "grid"):
        for model, name in ((ca.FM_UVUXUYVXVY, "affine"), (ca.FM_UV, "uv"), (ca.FM_UVQ, "uvq"), (ca.FM_U, "u")):
            e, rec = solved(scene, model, ca.IM_BICUBIC)
            g = np.zeros((e.n_sectors, 6), np.float32)
            g[:, :2] = TRUTH[:2]
            for order in (3, 5):
                for seeds, kw in (("records", dict(records=rec)), ("guesses", dict(guesses=g))):
                    refined, info, sums = e.refine_spline(order=order, return_sums=True, **kw)
                    tag = "spline%d_%s_%s_%s" % (order, scene, name, seeds)
                    out.update(fields(tag + ".records", refined))
                    out.update(fields(tag, info))
                    out[tag + ".sums"] = sums
            if model == ca.FM_U:
                for order in (3, 5):
                    out["spline%d_%s_coefficients" % (order, scene)] = e.spline_coefficients(ca.IMG_DEF, order)
            e.close()
    return out


def run_weighted():
    import correlation_amd as ca
    out = {}
    mask = np.ones((256, 256), np.uint8)
    mask[:, 100:108] = 0
    mask[30:34, :] = 0
    for scene in ("mix", "grid"):
        for model, interp, name in ((ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, "affine_bicubic"), (ca.FM_UV, ca.IM_BILINEAR, "uv_bilinear"),
                                    (ca.FM_UVQ, ca.IM_BICUBIC_SEPARABLE, "uvq_separable"), (ca.FM_U, ca.IM_BICUBIC, "u_bicubic")):
            e, rec = solved(scene, model, interp)
            g = np.zeros((e.n_sectors, 6), np.float32)
            g[:, :2] = TRUTH[:2]
            for seeds, kw in (("unit", dict(records=rec)), ("window", dict(guesses=g, sigma=3.0)), ("mask", dict(guesses=g, mask=mask)),
                              ("both", dict(records=rec, sigma=3.0, mask=mask, min_fraction=0.5))):
                refined, info, sums = e.refine_weighted(return_sums=True, **kw)
                tag = "weighted_%s_%s_%s" % (scene, name, seeds)
                out.update(fields(tag + ".records", refined))
                out.update(fields(tag, info))
                out[tag + ".sums"] = sums
            e.close()
    return out


def run_quadratic():
    import correlation_amd as ca
    out = {}
    for scene in ("mix", "grid"):
        for model, interp, name in ((ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, "affine_bicubic"), (ca.FM_UV, ca.IM_BILINEAR, "uv_bilinear"),
                                    (ca.FM_UVQ, ca.IM_BICUBIC_SEPARABLE, "uvq_separable"), (ca.FM_U, ca.IM_BICUBIC, "u_bicubic")):
            e, rec = solved(scene, model, interp)
            g = np.zeros((e.n_sectors, 6), np.float32)
            g[:, :2] = TRUTH[:2]
            g2 = np.tile(np.float32([1e-4, -1e-4, 5e-5, -5e-5, 1e-4, -1e-4]), (e.n_sectors, 1))
            for seeds, kw in (("records", dict(records=rec)), ("guesses", dict(guesses=g)), ("second", dict(guesses=g, second=g2)),
                              ("one_trip", dict(guesses=g, max_iters=1))):
                refined, info, sums = e.refine_quadratic(return_sums=True, **kw)
                tag = "quadratic_%s_%s_%s" % (scene, name, seeds)
                out.update(fields(tag + ".records", refined))
                out.update(fields(tag, info))
                out[tag + ".sums"] = sums
            e.close()
    return out


def run_composed():
    import correlation_amd as ca
    out = {}
    mask = np.ones((256, 256), np.uint8)
    mask[:, 100:108] = 0
    mask[30:34, :] = 0
    for scene in ("mix", "grid"):
        for model, interp, name in ((ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, "affine_bicubic"), (ca.FM_UV, ca.IM_BILINEAR, "uv_bilinear"),
                                    (ca.FM_UVQ, ca.IM_BICUBIC_SEPARABLE, "uvq_separable"), (ca.FM_U, ca.IM_BICUBIC, "u_bicubic")):
            e, rec = solved(scene, model, interp)
            g = np.zeros((e.n_sectors, 6), np.float32)
            g[:, :2] = TRUTH[:2]
            g2 = np.tile(np.float32([1e-4, -1e-4, 5e-5, -5e-5, 1e-4, -1e-4]), (e.n_sectors, 1))
            for order in (1, 2):
                for sampler in (0, 3, 5):
                    for seeds, kw in (("unit", dict(records=rec)), ("both", dict(guesses=g, sigma=3.0, mask=mask, min_fraction=0.5)),
                                      ("second", dict(guesses=g, second=g2, mask=mask))):
                        if seeds == "second" and order == 1:
                            continue
                        refined, info, sums = e.refine_composed(order=order, sampler=sampler, return_sums=True, **kw)
                        tag = "composed%d%d_%s_%s_%s" % (order, sampler, scene, name, seeds)
                        out.update(fields(tag + ".records", refined))
                        out.update(fields(tag, info))
                        out[tag + ".sums"] = sums
            e.close()
    return out


# ---- the solve's own launch paths (lk_engine_solve.cpp, lk_engine_sequence.cpp): records of the engine itself -----------
MODES = ("default", "batch_invariant", "reference_order1", "reference_order4", "backward")


def committed(scene, mode, py_stop=2):
    """(engine with the pair and the scene's sectors committed in `mode`, its guesses); `mix_small`: mix without its
    10 000-sample rectangle, whose lane group has no frame-pipelined instance"""
    import correlation_amd as ca
    und, dfm = ca.speckle.speckle_pair(256, 256, p=TRUTH, seed=5)
    e = ca.HipCorrelationEngine(interpolation=ca.IM_BICUBIC, fitting_model=ca.FM_UVUXUYVXVY, precision=1e-3, py_stop=py_stop)
    if mode == "batch_invariant":
        e.set_batch_invariant(True)
    elif mode.startswith("reference_order"):
        e.set_reference_order(int(mode[len("reference_order"):]))
    elif mode == "backward":
        e.set_update(ca.UPDATE_BACKWARD)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    if scene == "grid":
        e.set_rect_grid(8.0, 8.0, 247.0, 247.0, 24, 24)
    else:
        rects = RECTS if scene == "mix" else RECTS[:3]
        for s, r in enumerate(rects):
            e.resetPolygon_rect(s, *r)
        for k, q in enumerate(ANNULAR):
            e.resetPolygon_annular(len(rects) + k, *q)
    e.commit_sectors()
    g = np.zeros((e.n_sectors, 6), np.float32)
    g[:, :2] = TRUTH[:2]
    return e, g


def solve_all(mode):
    def run():
        e, g = committed("mix", mode)
        out = fields("all", e.correlate_all(g))
        out["all.sector_stats"] = e.sector_stats()
        return out
    return run


def correlate_one(modes):
    def run():
        out = {}
        for mode in modes:
            e, g = committed("mix", mode)
            for s in range(e.n_sectors):   # 361, 49, 899 and 10 000 samples and the annular list: every lane group
                rec, guess = e.correlate(s, g[s])
                out.update(fields("one_%s_%d" % (mode, s), np.array([rec])))
                out["one_%s_%d.guess" % (mode, s)] = guess
            out["one_%s.sector_stats" % mode] = e.sector_stats()
            e.close()
        return out
    return run


def window(scene, mode, py_stop=2):
    def run():
        import correlation_amd as ca
        e, g = committed(scene, mode, py_stop)
        e.sequence_reserve(4)
        for f in range(4):   # frame f: (f + 1) / 2 of the pair's deformation
            e.sequence_set_frame(f, ca.speckle.speckle_pair(256, 256, p=tuple(0.5 * (f + 1) * t for t in TRUTH), seed=5)[1])
        g[:, :2] *= np.float32(0.5)
        e.correlate_all(g)   # (leaves the guesses of frame 0 with the engine)
        rec = e.correlate_sequence(4, keep_guesses=True)
        out = fields("window", rec)
        out["window.guesses"] = e.sequence_guesses()
        out["window.pipelined"] = np.array([int(e.sequence_is_pipelined)])
        out["window.after"] = e.correlate_all()   # (the sequence state the window leaves behind)
        return out
    return run


def run_reseed():
    import correlation_amd as ca
    e, g = committed("grid", "batch_invariant")
    clean = e.correlate_all(g)
    chi_max = 4.0 * float(clean["chi"][clean["error_code"] == 0].max())
    g[7::37, 0] = 300.0   # beyond the image: these sectors fail by their error code
    out = fields("before", e.correlate_all(g))
    rec, n = e.reseed_failed(RADIUS, chi_max=chi_max, min_neighbours=1, max_rounds=2)
    out.update(fields("reseeded", rec))
    out.update(fields("info", e.reseed_info()))
    out["recovered"] = np.array([n])
    return out


# (name, environment, function)
SOLVES = [("solve_all_" + m, {}, solve_all(m)) for m in MODES[:4]]
SOLVES += [("solve_all_class_streams0", {"LK_CLASS_STREAMS": "0"}, solve_all("default")),
           ("solve_all_force_team2", {"LK_FORCE_TEAM": "2"}, solve_all("default")),
           ("correlate_one", {}, correlate_one(("default", "reference_order1", "backward"))),
           ("correlate_one_force_team2", {"LK_FORCE_TEAM": "2"}, correlate_one(("default", "reference_order1", "backward"))),
           ("window_default", {}, window("mix_small", "default")),
           ("window_batch_invariant", {}, window("mix_small", "batch_invariant")),   # (several classes side by side)
           ("window_pipeline0", {"LK_SEQ_PIPELINE": "0"}, window("mix_small", "default")),
           ("window_reference_order", {}, window("mix_small", "reference_order1")),
           ("window_grid_starved", {}, window("grid", "default", py_stop=3)),
           ("reseed_failed", {}, run_reseed)]
VARIANTS = [("strain_g%d_packed%d" % (g, p), {"LK_STRAIN_GROUP": str(g), "LK_STRAIN_PACKED": str(p)}, run_strain)
            for g in (16, 64) for p in (0, 1)]
VARIANTS += [("outlier_g%d_cap%s" % (g, cap), {"LK_OUTLIER_GROUP": str(g), "LK_OUTLIER_LDS_CAP": cap}, run_outlier)
             for g in (16, 64) for cap in ("0", "100000")]
VARIANTS += [("track_g%d" % g, {"LK_TRACK_GROUP": str(g)}, run_track) for g in (16, 64)]
VARIANTS += [("field_walk%d" % w, {"LK_FIELD_WALK": str(w)}, run_field) for w in (0, 1)]
VARIANTS += [("motion_chunk%d" % c, {"LK_MOTION_CHUNK": str(c)}, run_motion) for c in (64, 2048)]
VARIANTS += [("lens_chunk%d" % c, {"LK_LENS_CHUNK": str(c)}, run_lens) for c in (64, 2048)]
VARIANTS += [("stereo_g%d" % g, {"LK_STEREO_GROUP": str(g)}, run_stereo) for g in (16, 64)]
VARIANTS += [("plan", {}, run_plan), ("map", {}, run_map), ("evaluate", {}, run_evaluate), ("backward", {}, run_backward),
             ("pattern", {}, run_pattern), ("noise", {}, run_noise), ("znssd", {}, run_znssd), ("quadratic", {}, run_quadratic),
             ("spline", {}, run_spline), ("weighted", {}, run_weighted), ("composed", {}, run_composed)]
VARIANTS += SOLVES


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("ONLY in one file: " + k)
    same = 0
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes():
            same += 1
            continue
        n = int((x.view(np.uint8) != y.view(np.uint8)).sum()) if x.shape == y.shape and x.dtype == y.dtype else -1
        print("DIFFERS: %s (%s %s / %s %s, bytes that differ: %d)" % (k, x.dtype, x.shape, y.dtype, y.shape, n))
        bad.append(k)
    print("%d arrays equal byte for byte, %d not" % (same, len(bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--variant", help=argparse.SUPPRESS)   # (the child)
    ap.add_argument("--only", metavar="REGEX", help="run the variants whose name matches (default: all)")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if not args.out:
        ap.error("an output file, or --compare A B")
    if args.variant:
        fn = {name: f for name, _, f in VARIANTS}[args.variant]
        np.savez(args.out, **fn())
        return 0
    merged = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, env, _ in VARIANTS:
            if args.only and not re.search(args.only, name):
                continue
            part = os.path.join(tmp, name + ".npz")
            try:
                status = subprocess.run([sys.executable, os.path.abspath(__file__), part, "--variant", name],
                                        env=dict(os.environ, **env), timeout=CHILD_SECONDS).returncode
            except subprocess.TimeoutExpired:
                status = "none within %d s" % CHILD_SECONDS
            if status != 0:
                print("variant %s failed (exit status %s): stopping" % (name, status), flush=True)
                return 1
            with np.load(part) as z:
                merged.update({name + "/" + k: z[k] for k in z.files})
            print("variant %s: %d arrays" % (name, len(merged)), flush=True)
    np.savez(args.out, **merged)
    print("%d arrays -> %s" % (len(merged), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
