"""Non-square frames and pairs of unequal size.  Every kernel's argument block carries urows, ucols, drows and dcols on their
own; on a square pair of equal frames the four are one number, and rows swapped with columns, an undeformed dimension where
the deformed one belongs, a pitch of the wrong image or a border rule on the wrong axis change nothing.  Here they do: the
frames are 150 x 232 (wide) and 232 x 150 (tall), the unequal pair's deformed frame is 11 rows and 19 columns short of
that, so that the four numbers differ at every pyramid level, and most sectors lie where a transposed bound clamps or
rejects them (tests/frame_shapes_ref.py).  No new reference and no new tolerance: reference-order mode against the CPU
oracle by bytes, everything else with the helpers and bounds of the existing test of the same operation."""
import numpy as np
import pytest

import correlation_amd as ca

import backward_ref as BACKWARD   # solve_ref, close: the backward restatement on the oracle alone
import frame_shapes_ref as fs

pytestmark = pytest.mark.gpu

ZERO = np.zeros(6, np.float32)
ORIENTATIONS = ["wide", "tall"]
PAIRS = ["equal", "unequal"]
# the four models with the bicubic sampler, the six-parameter model with the other two
SOLVE_CASES = [(m, ca.IM_BICUBIC) for m in fs.MODELS] + [(ca.FM_UVUXUYVXVY, ca.IM_NEAREST), (ca.FM_UVUXUYVXVY, ca.IM_BILINEAR)]
CASE_IDS = ["u", "uv", "uvq", "affine", "affine_nearest", "affine_bilinear"]

PARITY = fs.module("test_parity_gpu")             # compare_results, make_pair's OraclePair
REFORDER = fs.module("test_reference_order_gpu")  # assert_same_bytes


def engine_of(frames, model=ca.FM_UVUXUYVXVY, interp=ca.IM_BICUBIC, mode="default"):
    e = ca.HipCorrelationEngine(interpolation=interp, fitting_model=model)
    if mode == "batch_invariant":
        e.set_batch_invariant(True)
    elif mode.startswith("reference_order"):
        e.set_reference_order(int(mode.split(":")[1]) if ":" in mode else 1)
    e.set_undeformed_image(frames[0])
    e.set_deformed_image(frames[1])
    return e


def grid_engine(oracle, orientation, which, model=ca.FM_UVUXUYVXVY, interp=ca.IM_BICUBIC, mode="default"):
    e = engine_of(fs.pair(orientation, which), model, interp, mode)
    fs.grid(oracle, orientation).register(e)
    e.commit_sectors()
    return e


def yardsticks(oracle, orientation, which, model, interp, rects=False):
    """compare_results' three oracle runs on the grid: T = 1 (the target), T = 8 and the exact solver (the yardsticks)"""
    return tuple(fs.oracle_records(oracle, orientation, which, model, interp, threads=t, solver=s, rects=rects)
                 for t, s in ((1, 0), (8, 0), (1, 2)))


def counted(oracle, orientation, which, model=ca.FM_UVUXUYVXVY, interp=ca.IM_BICUBIC, label="", rects=False):
    want = fs.oracle_records(oracle, orientation, which, model, interp, rects=rects)
    fs.assert_oracle_counts(oracle, orientation, which, want, label, max_iterations=3 if interp == ca.IM_BICUBIC else None)
    return want


# ---- 1. the sampler ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [ca.IM_NEAREST, ca.IM_BILINEAR, ca.IM_BICUBIC], ids=["nearest", "bilinear", "bicubic"])
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_sampler_bit_exact_on_the_cropped_frame(oracle, orientation, interp):
    """test_sampling_bit_exact's comparison on levels 0 to 2 of the cropped deformed frame (139 x 213 or 221 x 131), with
    all four validity boundaries and their float neighbours on both sides"""
    dfm = fs.pair(orientation, "unequal")[1]
    e = ca.HipCorrelationEngine(interpolation=interp)
    e.set_deformed_image(dfm)
    o = oracle.Oracle(interp=interp)
    o.set_image(1, dfm)
    rng = np.random.default_rng(17)
    f32, inf = np.float32, np.float32(np.inf)
    for lvl in (0, 1, 2):
        img = o.get_level(1, lvl)
        h, w = img.shape
        assert (h, w) == (dfm.shape[0] >> lvl, dfm.shape[1] >> lvl) and h != w
        assert e.get_pyramid_level(ca.IMG_DEF, lvl).shape == (h, w)
        pts = np.stack([rng.uniform(-2, w + 2, 1500), rng.uniform(-2, h + 2, 1500)], 1).astype(np.float32)
        pts[:50] = np.round(pts[:50])           # exact pixel centres
        edge = []
        # x on a validity boundary and next to it, y mid-range, then the same in y: 1 and w - 2 are the bicubic sampler's
        # boundaries, 0 and w - 1 those of the other two
        for b in (f32(0.0), f32(1.0), f32(w - 2.0), f32(w - 1.0)):
            edge += [(v, f32(h * 0.5 + 0.25)) for v in (np.nextafter(b, -inf), b, np.nextafter(b, inf))]
        for b in (f32(0.0), f32(1.0), f32(h - 2.0), f32(h - 1.0)):
            edge += [(f32(w * 0.5 + 0.25), v) for v in (np.nextafter(b, -inf), b, np.nextafter(b, inf))]
        pts = np.concatenate([pts, np.array(edge, np.float32)])
        got = e.sample(ca.IMG_DEF, lvl, pts)
        want = oracle.interpolate_many(interp, img, pts)
        assert np.array_equal(got[:, 3], want[:, 3]), \
            f"level {lvl} ({h} x {w}): out-of-image flags differ at {pts[got[:, 3] != want[:, 3]][:6].tolist()}"
        assert 0 < want[:, 3].sum() < len(pts)
        for axis in (want[-24:-12, 3], want[-12:, 3]):     # per axis: on each end of it some boundary points in, some out
            assert 0 < axis[:6].sum() < 6 and 0 < axis[6:].sum() < 6, axis
        ok = want[:, 3] == 0
        assert np.array_equal(got[ok, :3].view(np.uint32), want[ok, :3].view(np.uint32)), \
            f"level {lvl} ({h} x {w}): {np.count_nonzero((got[ok, :3] != want[ok, :3]).any(1))} samples differ"
    e.close()


# ---- 2. one evaluation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,interp", SOLVE_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_evaluation_sums_on_the_unequal_pair(oracle, orientation, model, interp):
    """A, b and chi of one evaluation at levels 0 to 2 on the far-corner sector that is still inside the cropped frame:
    bit-equal to the oracle in reference-order mode (test_evaluation_sums_are_bit_identical), within test_evaluation_sums'
    bounds in default mode"""
    frames = fs.pair(orientation, "unequal")
    g = fs.grid(oracle, orientation)
    s = g.far_valid
    xy, (cx, cy) = g.lists[s], (float(v) for v in g.centers[s])
    x0, y0 = g.corners[s]
    assert (x0 > frames[1].shape[0]) if orientation == "wide" else (y0 > frames[1].shape[1])   # past the other axis' bound
    o = oracle.Oracle(interp=interp, model=model)
    o.set_image(0, frames[0])
    o.set_image(1, frames[1])
    P = ca.N_PARAMS[model]
    p = np.array([1.1, -0.6, 0.003, -0.002, 0.001, 0.002], np.float32)[:P]
    if model == ca.FM_UVQ:
        p[2] = 0.002
    for mode in ("reference_order", "default"):
        e = engine_of(frames, model, interp, mode)
        e.set_sector_points(0, xy, center=(cx, cy))
        e.commit_sectors()
        for lvl in (0, 1, 2):
            lxy = xy if lvl == 0 else oracle.decimate(xy, lvl)
            assert e.sector_level_count(0, lvl) == len(lxy)
            pl = p.copy()
            pl[:min(P, 2)] /= (1 << lvl)
            A, b, chi, err = e.evaluate(0, lvl, pl)
            Ao, bo, chio, erro = oracle.evaluate(interp, model, o.get_level(0, lvl), o.get_level(1, lvl), lxy,
                                                 np.float32(cx) * np.float32(1.0 / (1 << lvl)),
                                                 np.float32(cy) * np.float32(1.0 / (1 << lvl)), pl)
            assert err == erro == 0, (mode, lvl, err, erro)
            iu = np.triu_indices(P)
            if mode == "reference_order":
                assert np.array_equal(A[:P, :P][iu], Ao[:P, :P][iu]), (lvl, len(lxy))
                assert np.array_equal(b[:P], bo[:P]) and np.float32(chi) == np.float32(chio), (lvl, len(lxy))
            else:
                scale = np.abs(Ao[:P, :P]).max()
                assert np.allclose(A[:P, :P][iu], Ao[:P, :P][iu], rtol=2e-5, atol=2e-6 * scale), lvl
                assert np.allclose(b[:P], bo[:P], rtol=2e-5, atol=2e-6 * np.abs(bo).max()), lvl
                assert abs(chi - chio) <= 2e-5 * chio, lvl
        e.close()
    o.close()


# ---- 3. whole solves --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,interp", SOLVE_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("which", PAIRS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_grid_records_are_the_oracles_bytes(oracle, orientation, which, model, interp):
    """reference-order mode, one thread and the reference's twenty: the 48-byte records of all 60 sectors, the 15
    out-of-image records of the unequal pair included"""
    counted(oracle, orientation, which, model, interp, "reference order")
    g = fs.grid(oracle, orientation)
    for threads in (1, 20):
        want = fs.oracle_records(oracle, orientation, which, model, interp, threads=threads)
        e = grid_engine(oracle, orientation, which, model, interp, f"reference_order:{threads}")
        got = e.correlate_all(ZERO)
        REFORDER.assert_same_bytes(got, want, f"{orientation} {which} model {model} interp {interp} T={threads}")
        if threads == 1:
            expected = fs.lane_groups([len(x) for x in g.lists], "reference_order")
            fs.assert_lane_groups(e, expected, [len(x) for x in g.lists])
            print("sample loops:", sorted(set(expected)), "lanes per sector")
            one, _ = e.correlate(g.far_valid, np.zeros(ca.N_PARAMS[model], np.float32))
            REFORDER.assert_same_bytes(one, want[g.far_valid], "single-sector entry point")
        e.close()


@pytest.mark.parametrize("model,interp", SOLVE_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("which", PAIRS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_grid_default_mode_within_the_yardsticks(oracle, orientation, which, model, interp):
    counted(oracle, orientation, which, model, interp, "default mode")
    g = fs.grid(oracle, orientation)
    e = grid_engine(oracle, orientation, which, model, interp)
    got = e.correlate_all(ZERO)
    expected = fs.lane_groups([len(x) for x in g.lists])
    fs.assert_lane_groups(e, expected, [len(x) for x in g.lists])
    print("sample loops:", sorted(set(expected)), "lanes per sector")
    PARITY.compare_results(got, yardsticks(oracle, orientation, which, model, interp),
                           f"{orientation} {which} model {model} interp {interp}")
    e.close()


@pytest.mark.parametrize("which", PAIRS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_batch_invariant_sectors_alone_and_in_the_batch(oracle, orientation, which):
    """a corner, one of the 15, the far valid corner and an interior sector: solved alone they have the bytes they have in
    the batch of 60"""
    want = counted(oracle, orientation, which, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, "batch invariant")
    g = fs.grid(oracle, orientation)
    e = grid_engine(oracle, orientation, which, mode="batch_invariant")
    full = e.correlate_all(ZERO)
    expected = fs.lane_groups([len(x) for x in g.lists], "batch_invariant")
    fs.assert_lane_groups(e, expected, [len(x) for x in g.lists])
    print("sample loops:", sorted(set(expected)), "lanes per sector")
    PARITY.compare_results(full, yardsticks(oracle, orientation, which, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC), "batch invariant")
    chosen = [0, len(g) - 1, g.far_valid, g.interior]
    assert g.edge[len(g) - 1] and not g.edge[[0, g.far_valid, g.interior]].any()
    for s in chosen:
        one, _ = e.correlate(s, ZERO)
        assert one.tobytes() == full[s].tobytes(), s
    e.close()
    for s in chosen:
        e = engine_of(fs.pair(orientation, which), mode="batch_invariant")
        g.register(e, sectors=[s])
        e.commit_sectors()
        alone = e.correlate_all(ZERO)
        assert alone[0].tobytes() == full[s].tobytes(), s
        assert alone[0]["error_code"] == want[s]["error_code"]
        e.close()


@pytest.mark.parametrize("which", PAIRS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_grid_as_implicit_rectangles(oracle, orientation, which):
    """the same 60 sectors registered as rectangles, which the sample loops walk themselves (rw > 0) instead of reading a
    list: the oracle's bytes in reference-order mode (16-lane rows), compare_results' bounds in default (64 lanes after the
    batch's promotions) and batch-invariant mode"""
    want = counted(oracle, orientation, which, label="implicit rectangles", rects=True)
    g = fs.grid(oracle, orientation)
    yard = yardsticks(oracle, orientation, which, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, rects=True)
    for mode in ("reference_order:1", "default", "batch_invariant"):
        e = engine_of(fs.pair(orientation, which), mode=mode)
        g.register_rects(e)
        e.commit_sectors()
        assert len(e.level_xy(0, g.far_valid)) == 0 and np.array_equal(e.getUndXY0ToCPU(g.far_valid), g.lists[g.far_valid])
        assert np.array_equal(np.float32([e.sector_info(s)[1:3] for s in range(len(g))]), g.rect_centers)
        got = e.correlate_all(ZERO)
        expected = fs.lane_groups([len(x) for x in g.lists], mode.split(":")[0])
        fs.assert_lane_groups(e, expected, [len(x) for x in g.lists])
        print(f"{mode}: sample loops", sorted(set(expected)), "lanes per sector")
        if mode.startswith("reference_order"):
            REFORDER.assert_same_bytes(got, want, f"{orientation} {which} implicit rectangles")
        else:
            PARITY.compare_results(got, yard, f"{orientation} {which} implicit rectangles {mode}")
        e.close()


# The grid's sectors have 400 samples: a 16-lane row in reference-order and batch-invariant mode.  The other sample loops
# run on sectors of other sizes and kinds in the same frames, placed in the far part of the frame like the grid's:
def other_sectors(oracle, orientation):
    """[(kind, arguments, sample list, centre or None)]: a 61 x 61 implicit rectangle, an annular wedge, an explicit list
    (every other sample of a rectangle) inside the cropped frame and one that straddles its right (tall: its bottom) edge -
    valid on the equal pair at every level, out of the image on the unequal one"""
    if orientation == "wide":
        big, ann, inside, across = (140, 60, 200, 120), (np.float32(-0.5), 116.0, 75.0), (150, 20, 190, 50), (178, 96, 218, 126)
    else:
        big, ann, inside, across = (50, 140, 110, 200), (np.float32(np.pi / 2 - 0.5), 75.0, 116.0), (20, 150, 50, 190), (80, 178, 110, 218)
    out = [("rect", big, oracle.rect_points(*big), ((big[0] + big[2]) * 0.5, (big[1] + big[3]) * 0.5))]
    ann = (30.0, 35.0, ann[0], np.float32(1.0), ann[1], ann[2], 4)        # radii 30 to 65, one radian about the long axis
    out.append(("annular", ann, oracle.annular_points(*ann), None))       # (centre: the float mean of the samples)
    for r in (inside, across):
        out.append(("points", r, oracle.rect_points(*r)[::2].copy(), ((r[0] + r[2]) * 0.5, (r[1] + r[3]) * 0.5)))
    return out


def other_domain(oracle, orientation, e=None):
    """the four sectors above and three of the grid (the far valid corner, one of the 15, an interior one): registered on
    `e`; returns (lists, centres or None per sector)"""
    g = fs.grid(oracle, orientation)
    lists, cens = [], []
    for s, (kind, args, xy, cen) in enumerate(other_sectors(oracle, orientation)):
        if e is not None and kind == "rect":
            e.resetPolygon_rect(s, *args)
        elif e is not None and kind == "annular":
            e.resetPolygon_annular(s, *[float(v) if i < 6 else v for i, v in enumerate(args)])
        elif e is not None:
            e.set_sector_points(s, xy, center=cen)
        lists.append(xy)
        cens.append(cen)
    picked = [g.far_valid, len(g) - 1, g.interior]
    if e is not None:
        g.register(e, first=len(lists), sectors=picked)
    lists += [g.lists[s] for s in picked]
    cens += [tuple(float(v) for v in g.centers[s]) for s in picked]
    return lists, cens


def other_oracle(oracle, frames, lists, cens, threads=1, solver=0):
    """the annular sector's centre is the float mean of its samples (centre not given): solved on its own call"""
    o = oracle.Oracle(n_threads=threads, solver=solver)
    o.set_image(0, frames[0])
    o.set_image(1, frames[1])
    out = np.zeros(len(lists), oracle.RESULT_DTYPE)
    given = [k for k, c in enumerate(cens) if c is not None]
    mean = [k for k, c in enumerate(cens) if c is None]
    out[given] = o.correlate_sectors([lists[k] for k in given], centers=np.array([cens[k] for k in given], np.float32))
    out[mean] = o.correlate_sectors([lists[k] for k in mean])
    o.close()
    return out


@pytest.mark.parametrize("which", PAIRS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_wavefront_workgroup_and_team_sample_loops(oracle, orientation, which, monkeypatch):
    """the wavefront flavour of reference-order mode by bytes; the lane groups default mode picks, 32-lane groups, 4-wavefront
    workgroups and teams of 8-wavefront workgroups (the pipelined explicit-list loop) within compare_results' bounds"""
    frames = fs.pair(orientation, which)
    lists, cens = other_domain(oracle, orientation)
    counts = [len(x) for x in lists]
    want = other_oracle(oracle, frames, lists, cens)
    expect = [0, 0, 0, 0 if which == "equal" else fs.OUT_OF_IMAGE, 0, 0 if which == "equal" else fs.OUT_OF_IMAGE, 0]
    print(f"{orientation} {which} pair: samples per sector {counts}, oracle error codes {want['error_code'].tolist()}")
    assert want["error_code"].tolist() == expect and counts[0] == 61 * 61 and min(counts[1:4]) > 512
    assert np.array_equal(want["n_points"], counts)

    def run(mode, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        e = engine_of(frames, mode=mode)
        other_domain(oracle, orientation, e)
        e.commit_sectors()
        for k, xy in enumerate(lists):
            assert np.array_equal(e.getUndXY0ToCPU(k), xy), f"sector {k} sample list"
        got = e.correlate_all(ZERO)
        if mode != "default":     # (default mode: lanes without work join a neighbour's sector, the sums depend on the batch)
            one, _ = e.correlate(1, ZERO)
            assert one.tobytes() == got[1].tobytes()
        groups = fs.lane_groups(counts, mode.split(":")[0], env.get("LK_FORCE_GROUP", 0), env.get("LK_FORCE_TEAM", 0))
        fs.assert_lane_groups(e, groups, counts)
        e.close()
        for k in env:
            monkeypatch.delenv(k)
        print(f"{mode} {env}: lanes per sector {groups}")
        return got

    for threads in (1, 20):
        REFORDER.assert_same_bytes(run(f"reference_order:{threads}"), other_oracle(oracle, frames, lists, cens, threads),
                                   f"{orientation} {which} T={threads}")
    yard = (want, other_oracle(oracle, frames, lists, cens, 8), other_oracle(oracle, frames, lists, cens, 1, 2))
    for env in ({}, {"LK_FORCE_GROUP": 32}, {"LK_FORCE_GROUP": 256}, {"LK_FORCE_TEAM": 2}):
        PARITY.compare_results(run("default", **env), yard, f"{orientation} {which} {env}")
    PARITY.compare_results(run("batch_invariant"), yard, f"{orientation} {which} batch invariant")


# ---- 4. the searches --------------------------------------------------------------------------------------------------------
SEARCH = fs.module("test_guess_search_gpu")       # check_against_reference (ref_search)
ROTATED = fs.module("test_rotated_search_gpu")    # its own check_against_reference


def search_guesses_near_truth(n):
    g = np.zeros((n, 6), np.float32)
    g[:, :2] = fs.TRUTH[:2]
    g[:, 2:] = np.float32([1e-3, -2e-3, 5e-4, 1e-3])     # (words a search must carry through)
    return g


@pytest.mark.parametrize("level,radius", [(0, 8), (1, 4)])
@pytest.mark.parametrize("model", [ca.FM_UVUXUYVXVY, ca.FM_UVQ], ids=["affine", "uvq"])
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_searches_on_the_unequal_pair(oracle, orientation, model, level, radius):
    """lk_search_guesses and lk_search_rotated (five angles about zero) against their numpy brute forces: exact integer
    sums, compared with equality.  The radius reaches past the cropped right and bottom edges, so the candidate ranges of
    the sectors next to them are clipped by the DEFORMED frame's columns and rows."""
    counted(oracle, orientation, "unequal", model, label="searches")
    g = fs.grid(oracle, orientation)
    e = grid_engine(oracle, orientation, "unequal", model)
    guesses = search_guesses_near_truth(len(g))
    full = (2 * radius + 1) ** 2
    info, _ = SEARCH.check_against_reference(e, guesses, level, radius)
    clipped = (info["n_valid"] > 0) & (info["n_valid"] < full)
    found = clipped & (info["status"] == ca.GS_OK) & (info["score"] > 0.5)
    print(f"{orientation} level {level} radius {radius}: {int(clipped.sum())} sectors with a clipped candidate range, "
          f"{int(found.sum())} of them OK with a score above 0.5; {int((info['n_valid'] == full).sum())} unclipped, "
          f"{int((info['n_valid'] == 0).sum())} without a candidate")
    assert g.edge[found].any() and (info["n_valid"] == full).any()      # clipped at a cropped edge, found all the same
    rinfo, _, _ = ROTATED.check_against_reference(e, guesses, level, radius, 2 * ROTATED.DEG, 2)
    rfound = (rinfo["n_valid"] > 0) & (rinfo["n_valid"] < 5 * full) & (rinfo["status"] == ca.GS_OK) & (rinfo["score"] > 0.5)
    assert g.edge[rfound].any() and (rinfo["n_valid"] == 5 * full).any()
    e.close()


# ---- 5. sequence windows ----------------------------------------------------------------------------------------------------
WINDOW = fs.module("test_sequence_window_gpu")    # make_engine, loop, window


@pytest.mark.parametrize("mode", ["reference_order:1", "reference_order:20", "batch_invariant"])
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_window_records_on_non_square_frames(oracle, orientation, mode):
    """three pairs of a four-frame sequence: the window's records are the one-pair loop's bytes; in reference-order mode
    frame 1 is the oracle's; a window that holds a frame of another size is refused"""
    rows, cols = fs.SHAPES[orientation]
    frames = ca.speckle.speckle_sequence(rows, cols, 4)
    g = fs.grid(oracle, orientation)
    n, c = 3, ((cols - 1) * 0.5, (rows - 1) * 0.5)
    a, b = WINDOW.make_engine(mode), WINDOW.make_engine(mode)
    for e in (a, b):
        e.set_undeformed_image(frames[0])
        g.register(e)
        e.commit_sectors()
    g_loop, r_loop = WINDOW.loop(a, frames, 0, n, center=c)
    b.sequence_reserve(n)
    g_win, r_win = WINDOW.window(b, frames, 0, n, center=c)
    print(f"{orientation} {mode}: pipelined {b.sequence_is_pipelined}; error codes per frame "
          f"{[np.bincount(r['error_code'], minlength=3).tolist() for r in r_loop]}")
    assert b.sequence_is_pipelined, "the 16-lane class of 400-sample sectors has a frame-pipelined instance"
    assert (r_loop["error_code"] == 0).mean() > 0.9
    for f in range(n):
        assert g_win[f].tobytes() == g_loop[f].tobytes(), f"guesses of frame {f}"
        assert r_win[f].tobytes() == r_loop[f].tobytes(), f"records of frame {f}"
    if mode.startswith("reference_order"):
        o = oracle.Oracle(n_threads=int(mode.split(":")[1]))
        o.set_image(0, frames[0])
        o.set_image(1, frames[1])
        REFORDER.assert_same_bytes(r_win[0], o.correlate_sectors(g.lists, centers=g.centers), f"{orientation} {mode} frame 1")
        o.close()
    b.sequence_set_frame(1, np.ascontiguousarray(frames[2].T))      # cols x rows
    with pytest.raises(ca.LkError) as err:
        b.correlate_sequence(n)
    assert err.value.code == ca.ERROR_BAD_DOMAIN
    b.sequence_set_frame(1, np.ascontiguousarray(frames[2][:-1]))   # one row short
    with pytest.raises(ca.LkError) as err:
        b.correlate_sequence(n)
    assert err.value.code == ca.ERROR_BAD_DOMAIN
    a.close()
    b.close()


# ---- 6. the backward update -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("model", [ca.FM_UVUXUYVXVY, ca.FM_UV], ids=["affine", "uv"])
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_backward_solves_on_the_unequal_pair(oracle, orientation, model):
    """the inverse-compositional solve of the grid, registered as implicit rectangles, against solve_ref, within close()'s
    bounds; the 15 sectors that leave the cropped frame carry the out-of-image code"""
    want = counted(oracle, orientation, "unequal", model, ca.IM_BICUBIC, "backward", rects=True)
    g = fs.grid(oracle, orientation)
    e = engine_of(fs.pair(orientation, "unequal"), model)
    g.register_rects(e)               # (domain "rect" of test_backward_gpu.py: implicit rectangles)
    e.commit_sectors()
    e.set_update(ca.UPDATE_BACKWARD)
    got = e.correlate_all(ZERO)
    n = BACKWARD.P[model]
    frames = BACKWARD.Frames(oracle, ca.IM_BICUBIC, *fs.pair(orientation, "unequal"))
    assert np.array_equal(got["error_code"] == fs.OUT_OF_IMAGE, g.edge) and np.array_equal(got["error_code"] == 0, ~g.edge)
    assert np.array_equal(got["error_code"], want["error_code"])      # (the forward oracle's codes: the same sectors leave)
    it_diff = 0
    for s in range(len(g)):
        assert tuple(e.sector_info(s)[1:3]) == tuple(g.rect_centers[s])
        p, chi, it, err = BACKWARD.solve_ref(BACKWARD.Problem(frames, model, g.lists[s], g.rect_centers[s]), ZERO)
        r = got[s]
        assert r["error_code"] == err, (s, r, err)
        it_diff += int(r["iterations"] != it)
        assert abs(int(r["iterations"]) - it) <= 1, (s, r["iterations"], it)
        if err == ca.ERROR_NONE:
            assert BACKWARD.close(r["p"][:n], p[:n]), (s, r["p"], p)
            assert BACKWARD.close(r["chi"], chi), (s, r["chi"], chi)
    print(f"{orientation} model {model}: iteration counts differ on {it_diff} of {len(g)} sectors")
    assert it_diff <= max(1, len(g) // 100)
    e.close()


# ---- 7. the passes that index an image themselves ---------------------------------------------------------------------------
RESIDUAL = fs.module("test_residual_gpu")         # check_map, check_photometry
UNCERTAINTY = fs.module("test_uncertainty_gpu")   # check_against_oracle
PATTERN = fs.module("test_pattern_gpu")           # check_sectors


def near_truth_records(n):
    rec = np.zeros(n, ca.RESULT_DTYPE)
    rec["p"][:] = np.float32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001])
    rec["chi"] = 1.0
    return rec


def leaves_at_level_0(oracle, orientation):
    """the sectors whose level-0 samples leave the cropped frame under near_truth_records: the last grid column alone (the
    last grid row leaves it at the coarser levels only: 11 rows are cut, 19 columns)"""
    g = fs.grid(oracle, orientation)
    return np.arange(len(g)) // g.ny == g.nx - 1


@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_residual_map_on_the_unequal_pair(oracle, orientation):
    """check_map at level 0: the whole undeformed frame (its width no multiple of the 32 x 8 tile, the wide frame's height
    neither) and a window across the cropped edge, where owned pixels lose their deformed sample"""
    counted(oracle, orientation, "unequal", label="residual map")
    und, dfm = fs.pair(orientation, "unequal")
    g = fs.grid(oracle, orientation)
    e = grid_engine(oracle, orientation, "unequal")
    rec = near_truth_records(len(g))
    rows, cols = und.shape
    assert cols % 32 and (rows % 8 or orientation == "tall")      # (232 rows are 29 tiles: the tall frame is ragged in x alone)
    _, _, o = RESIDUAL.check_map(oracle, e, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, rec, (0, 0, cols, rows))
    assert (o >= 0).any() and (o == -1).any() and (o < -1).any()
    lost = np.argwhere(o < -1)
    assert (lost[:, 1] >= dfm.shape[1] - 6).any() and (lost[:, 0] >= dfm.shape[0] - 6).any()    # past the right and the bottom edge
    _, _, o = RESIDUAL.check_map(oracle, e, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, rec, (dfm.shape[1] - 21, dfm.shape[0] - 13, 37, 19))
    assert (o >= 0).any() and (o < -1).any()
    e.close()


@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_photometry_and_uncertainty_on_the_unequal_pair(oracle, orientation):
    """both passes on the grid with records near the truth, through the checks of their own tests; the sectors that leave
    the cropped frame at level 0 carry the out-of-image status, with solved records all 15 are bad records"""
    counted(oracle, orientation, "unequal", label="photometry and uncertainty")
    g = fs.grid(oracle, orientation)
    model, interp = ca.FM_UVUXUYVXVY, ca.IM_BICUBIC
    e = grid_engine(oracle, orientation, "unequal")
    rec = near_truth_records(len(g))
    leaves = leaves_at_level_0(oracle, orientation)
    out, sums = e.photometry(records=rec, return_sums=True)
    RESIDUAL.check_photometry(oracle, e, model, interp, rec, out, sums, 0, [])
    assert np.array_equal(out["status"] == ca.PHOTO_OUT_OF_IMAGE, leaves) and np.array_equal(out["status"] == ca.PHOTO_OK, ~leaves)
    unc, usums = e.parameter_uncertainty(records=rec, return_sums=True)
    UNCERTAINTY.check_against_oracle(oracle, e, model, interp, rec, unc, usums, 0, [], 0)
    assert np.array_equal(unc["status"] == ca.UNC_OUT_OF_IMAGE, leaves) and np.array_equal(unc["status"] == ca.UNC_OK, ~leaves)
    solved = e.correlate_all(ZERO)
    assert np.array_equal(solved["error_code"] == fs.OUT_OF_IMAGE, g.edge)
    out, sums = e.photometry(return_sums=True)
    RESIDUAL.check_photometry(oracle, e, model, interp, solved, out, sums, 0, [])
    assert np.array_equal(out["status"] == ca.PHOTO_BAD_RECORD, g.edge) and np.array_equal(out["status"] == ca.PHOTO_OK, ~g.edge)
    unc, usums = e.parameter_uncertainty(return_sums=True)
    UNCERTAINTY.check_against_oracle(oracle, e, model, interp, solved, unc, usums, 0, [], 0)
    assert np.array_equal(unc["status"] == ca.UNC_BAD_RECORD, g.edge) and np.array_equal(unc["status"] == ca.UNC_OK, ~g.edge)
    e.close()


@pytest.mark.parametrize("which,slot", [("equal", ca.IMG_UND), ("unequal", ca.IMG_DEF)], ids=["undeformed", "cropped_deformed"])
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_pattern_quality_at_the_right_and_bottom_border(orientation, which, slot):
    """the sector sums, exact, on sectors that touch the right border, the bottom border and the corner of the frame, where
    the gradient clamps its neighbour to cols - 1 or rows - 1; an interior sector beside them"""
    frames = fs.pair(orientation, which)
    rows, cols = frames[slot].shape
    rects = [(cols - 20, 30, cols - 1, 49), (30, rows - 20, 49, rows - 1), (cols - 25, rows - 25, cols - 1, rows - 1),
             (cols - 1, 60, cols - 1, 100), (60, rows - 1, 100, rows - 1), (60, 60, 90, 80)]
    e = PATTERN.make_engine({ca.IMG_UND: frames[0], ca.IMG_DEF: frames[1]}, rects)
    out, sums, mig = e.pattern_quality(slot=slot, return_sums=True, **PATTERN.QUALITY)
    status = PATTERN.check_sectors(e, e.get_pyramid_level(slot, 0), 0, rects, out, sums, mig)
    print(f"{orientation} slot {slot} ({rows} x {cols}): status {status}")
    e.close()


COMPOSED = fs.module("test_composed_gpu")         # device_sampler, NEAR, SECOND, SIGMA


@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_composed_refinement_on_the_unequal_pair(oracle, orientation):
    """lk_refine_composed with everything switched on - order 2, the quintic spline of the coefficient image
    [drows][dcols], a column mask [urows][ucols], a Gaussian window - on eight interior sectors: the weighted sums of the
    seed evaluation and the info derived from them against the restatement, in the form and with the bounds of
    test_sums_and_info_of_the_seed_evaluation; whole runs against composed_ref.refine, as test_rim_of_a_hole compares
    them; the transposed mask is refused"""
    import composed_ref as cr
    import quadratic_ref as qr
    import weighted_ref as wr
    import znssd_ref as zr
    counted(oracle, orientation, "unequal", label="composed refinement")
    und, dfm = fs.pair(orientation, "unequal")
    g = fs.grid(oracle, orientation)
    ix, iy = np.divmod(np.arange(len(g)), g.ny)
    inner = np.flatnonzero((ix >= 1) & (ix < g.nx - 1) & (iy >= 1) & (iy < g.ny - 1))
    picked = inner[np.linspace(0, len(inner) - 1, 8).astype(int)].tolist()      # eight of them, the far ones included
    assert len(set(picked)) == 8 and g.far_valid in picked
    model, interp, order, sampler = ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, 2, 5
    mask = np.ones(und.shape, np.uint8)
    for s in picked:                                     # three columns cut out of every sector
        mask[:, g.corners[s][0] + 6:g.corners[s][0] + 9] = 0
    assert mask.shape == und.shape != dfm.shape
    inv = wr.inv_of(COMPOSED.SIGMA)
    e = engine_of((und, dfm))
    g.register(e, sectors=picked)
    e.commit_sectors()
    fn = COMPOSED.device_sampler(e, sampler)
    seeds = np.zeros((8, 6), np.float32)
    seeds[:, :2] = fs.TRUTH[:2]
    seeds[:, 2:] = COMPOSED.NEAR[2:]
    second = np.tile(COMPOSED.SECOND, (8, 1))
    rec, info, sums = e.refine_composed(guesses=seeds, second=second, order=order, sampler=sampler, sigma=COMPOSED.SIGMA, mask=mask,
                                        max_iters=0, return_sums=True)
    assert sums.shape == (8, ca.QD_SUMS)
    worst = 0.0
    for k, s in enumerate(picked):
        xy, (cx, cy) = g.lists[s], (float(v) for v in g.centers[s])
        n = len(xy)
        w = wr.sample_weights(xy, cx, cy, inv, mask)
        live = w > 0
        assert int(live.sum()) == n - 3 * fs.SIDE
        p12 = np.concatenate([seeds[k], COMPOSED.SECOND])
        f, gg, gx, gy, dx, dy, bad = qr.sample_floats(oracle, interp, und, dfm, xy, cx, cy, p12, fn)
        assert not bad[live].any()
        terms = cr.weighted_terms(f[live], gg[live], gx[live], gy[live], dx[live], dy[live], w[live])
        bound = 64.0 * n * 2.0 ** -53 * np.abs(terms).sum(axis=0)
        err = np.abs(sums[k][:qr.FLAGGED] - terms.sum(axis=0))
        assert (err <= bound).all(), (s, err, bound)
        assert not sums[k][qr.FLAGGED:].any(), (s, sums[k][qr.FLAGGED:])
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        i = info[k]
        pro = wr.prologue(xy, cx, cy, w)
        N = wr.device_sum(w.astype(np.float64), wr.group_of(n))
        assert i["n_points"] == n and i["n_valid"] == pro["n_valid"] == int(live.sum()), (s, i)
        assert i["weight_sum"].tobytes() == np.float32(N).tobytes(), (s, i, N)
        assert abs(float(i["n_eff"]) - pro["n_eff"]) <= 4 * 2.0 ** -24 * pro["n_eff"], (s, i, pro)
        status, delta, crit, gain, offset = ca.composed_step_from_sums(order, model, pro["n_valid"], N, sums[k], zr.LAMBDA0)
        zncc = cr.criterion(pro["n_valid"], N, sums[k])[4]
        assert status == 0 and i["status"] == ca.ZN_MAX_ITERS, (s, status, i)
        for name, want in (("gain", gain), ("offset", offset), ("znssd", crit), ("zncc", zncc), ("zncc_seed", zncc)):
            assert i[name].tobytes() == np.float32(want).tobytes(), (s, name, i[name], want)
        assert (i["iterations"], i["evaluations"]) == (0, 1) and i["shift"] == 0 and i["last_step"] == 0 and not i["reserved"].any()
        assert i["p"].tobytes() == p12.tobytes() and i["bend"].tobytes() == np.float32(qr.bend(p12, n)).tobytes(), (s, i)
        r = rec[k]
        V = (f[live] - gg[live]).astype(np.float64)
        chi = (w[live].astype(np.float64) * V * V).sum() / pro["sw"]
        assert r["p"].tobytes() == seeds[k].tobytes() and abs(float(r["chi"]) - chi) <= 1e-6 * chi, (s, r, chi)
        assert r["error_code"] == ca.ERROR_CORRELATION_MAX_ITERS_REACHED and r["n_points"] == n
    print(f"{orientation}: sectors {picked}, worst sum error / bound {worst:.3g}")
    # whole runs from the true translation and zero gradients, against composed_ref.refine of every sector with the pass's own
    # sampler, the mask and the window - test_rim_of_a_hole's comparison: the restatement's statuses, and the distance of
    # (u, v) to the analytic map at the sector's centre at most 1.5 times the restatement's, largest and mean
    start = np.zeros((8, 6), np.float32)
    start[:, :2] = fs.TRUTH[:2]
    rec, info = e.refine_composed(guesses=start, order=order, sampler=sampler, sigma=COMPOSED.SIGMA, mask=mask)
    rows, cols = und.shape
    cen = g.centers[picked].astype(np.float64)
    truth = np.stack([fs.TRUTH[0] + fs.TRUTH[2] * (cen[:, 0] - cols / 2.0) + fs.TRUTH[3] * (cen[:, 1] - rows / 2.0),
                      fs.TRUTH[1] + fs.TRUTH[4] * (cen[:, 0] - cols / 2.0) + fs.TRUTH[5] * (cen[:, 1] - rows / 2.0)], 1)
    restated = [cr.refine(oracle, und, dfm, g.lists[s], float(g.centers[s][0]), float(g.centers[s][1]), start[k], sigma=COMPOSED.SIGMA,
                          mask=mask, sampler=fn)[0] for k, s in enumerate(picked)]
    err_ref = cr.uv_error([r["p"] for r in restated], truth)
    err = cr.uv_error(info["p"], truth)
    close_to = np.abs(info["p"][:, :2].astype(np.float64) - np.array([r["p"][:2] for r in restated], np.float64)).max()
    print(f"{orientation}: statuses {info['status'].tolist()} (restated {[int(r['status']) for r in restated]}); largest |(u, v) - truth| "
          f"{err.max():.6f} px (restated {err_ref.max():.6f}, allowed {1.5 * err_ref.max():.6f}), mean {err.mean():.6f} px (restated "
          f"{err_ref.mean():.6f}, allowed {1.5 * err_ref.mean():.6f}); largest |(u, v) - restated (u, v)| {close_to:.2e} px")
    assert info["status"].tolist() == [int(r["status"]) for r in restated]
    assert (info["status"] == ca.ZN_CONVERGED).all() and (rec["error_code"] == 0).all(), info["status"]
    assert err.max() <= 1.5 * err_ref.max() and err.mean() <= 1.5 * err_ref.mean(), (err, err_ref)
    with pytest.raises(ca.LkError) as refused:
        e.refine_composed(guesses=seeds, order=order, sampler=sampler, sigma=COMPOSED.SIGMA, mask=np.ascontiguousarray(mask.T))
    assert refused.value.code == ca.ERROR_BAD_DOMAIN
    e.close()
