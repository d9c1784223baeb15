"""The geometry and the case lists of the pass-instance tests (test_pass_instances_host.py, test_pass_instances_gpu.py): one
set of sectors on znssd_ref's 256 x 256 pair that puts a sector on either side of both thresholds of lk_bw_group (512 / 513
and 8192 / 8193 level-0 samples), gives every lane group an implicit rectangle and a list, and a sector smaller than a row of
lanes; and thin adapters to the checkers of the per-pass tests.  No restatement lives here: the references are
backward_ref.py, znssd_ref.py, weighted_ref.py, uncertainty_ref.py and residual_ref.py."""
import functools

import numpy as np

import correlation_amd as ca

import backward_ref as br
import weighted_ref as wr
import znssd_ref as zr

F32 = np.float32
MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
INTERPS = [ca.IM_NEAREST, ca.IM_BILINEAR, ca.IM_BICUBIC, ca.IM_BICUBIC_SEPARABLE]
CASES = [(m, i) for m in MODELS for i in INTERPS]                      # the sixteen (model, interpolator) pairs
ORACLE_CASES = [(m, i) for m, i in CASES if i in br.ORACLE_INTERPS]    # the twelve the oracle has a sampler for
MODEL_NAME = {ca.FM_U: "u", ca.FM_UV: "uv", ca.FM_UVQ: "uvq", ca.FM_UVUXUYVXVY: "affine"}
INTERP_NAME = {ca.IM_NEAREST: "nearest", ca.IM_BILINEAR: "bilinear", ca.IM_BICUBIC: "bicubic", ca.IM_BICUBIC_SEPARABLE: "separable"}


# what the tests measured, for tests/tools/pass_instances_report.py: (pass, model, interpolator, group) -> worst deviation /
# bound (and, for the backward solves, what else the report prints); the backward instances the launch reports named
MEASURED = {}
SEEN = set()


def note(what, case, ratios):
    """the worst of (sector, deviation / bound) per lane group"""
    g = groups()
    for s, r in ratios:
        key = (what, case[0], case[1], g[s])
        MEASURED[key] = max(MEASURED.get(key, 0.0), float(r))


def case_id(case):
    return f"{MODEL_NAME[case[0]]}-{INTERP_NAME[case[1]]}"


# ---- the sectors, in batch order ------------------------------------------------------------------------------------------
# (kind, definition, level-0 samples).  The order alternates the groups (16, 64, 16, 512, 16, 64, 16, 512): no two sectors
# of a group are neighbours in the batch.  Every sector keeps 8 px to the border: the bicubic's reach (2 px) plus the 1.3 px
# shift of znssd_ref.TRUTH with room for the 0.002 gradient terms over the frame.
WIDE = (8, 8, 135, 71)                 # 128 x 64 = 8192
SHIFT_Y = 72                           # the point list: WIDE's nodes moved down by 72 rows, plus the node right of its first row
SECTORS = [
    ("rect", (142, 52, 144, 54), 9),          # 3 x 3: fewer samples than one row of lanes; 4 samples at level 1, 1 at level 2
    ("rect", (144, 100, 170, 118), 513),        # 27 x 19: the first count of the 64-lane group
    ("rect", (172, 32, 190, 50), 361),         # 19 x 19
    ("rect", (150, 150, 245, 245), 9216),      # 96 x 96: znssd_ref's 512-lane sector
    ("rect", (180, 68, 211, 83), 512),        # 32 x 16: the last count of the 16-lane group
    ("rect", WIDE, 8192),                      # the last count of the 64-lane group
    ("annular", zr.ANNULAR[0], None),          # znssd_ref's list sector: at most 512, no multiple of 16
    ("points", None, 8193),                    # the first count of the 512-lane group, as a registered point list
]
N_SECTORS = len(SECTORS)
TINY, RING, LIST = 0, 6, 7
RECTS = [d if k == "rect" else None for k, d, _ in SECTORS]    # what the per-pass checkers take: None marks a list sector
NEAR = F32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001])      # the seed of the per-pass seed evaluations
MASK_BAND = (60, 70)                   # the weighted pass's mask removes these columns ... (WIDE and its shifted list)
MASK_BAND_BIG = (225, 235)            # ... and these (the 96 x 96 sector)
SIGMA = 40.0                           # the weighted pass's Gaussian window


def point_list():
    xy = zr.rect_rows(*WIDE)
    xy[:, 1] += SHIFT_Y
    return np.concatenate([xy, F32([[WIDE[2] + 1, WIDE[1] + SHIFT_Y]])])


@functools.lru_cache(maxsize=None)
def _lists():
    from oracle import lk_oracle as lo
    out = []
    for kind, d, _ in SECTORS:
        if kind == "rect":
            xy = zr.rect_rows(*d)
            assert np.array_equal(np.sort(xy.view("f4,f4"), axis=0), np.sort(lo.rect_points(*d).view("f4,f4"), axis=0))
        elif kind == "annular":
            xy = np.asarray(lo.annular_points(*d), F32).reshape(-1, 2)
        else:
            xy = point_list()
        xy.setflags(write=False)
        out.append(xy)
    return tuple(out)


def lists():
    """the level-0 samples of every sector in the order the passes walk them (rectangles row by row, lists as registered)"""
    return list(_lists())


def centres():
    """float32 centres, as the engine commits them: the mean of the samples"""
    return [(F32(l[:, 0].astype(np.float64).mean()), F32(l[:, 1].astype(np.float64).mean())) for l in lists()]


def counts():
    return [len(l) for l in lists()]


def groups():
    """the lane group of every sector: lk_bw_group of its level-0 count"""
    return [wr.group_of(n) for n in counts()]


def count3():
    g = groups()
    return tuple(g.count(k) for k in (16, 64, 512))


def make_engine(und, dfm, model, interp, **cfg):
    cfg.setdefault("precision", zr.PRECISION)
    cfg.setdefault("py_stop", 2)
    e = ca.HipCorrelationEngine(interpolation=interp, fitting_model=model, py_start=0, **cfg)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    for s, (kind, d, _) in enumerate(SECTORS):
        if kind == "rect":
            e.resetPolygon_rect(s, *d)
        elif kind == "annular":
            e.resetPolygon_annular(s, *d)
        else:
            e.set_sector_points(s, point_list())
    e.commit_sectors()
    return e


def check_engine_geometry(e):
    """the engine's level-0 counts are the fixture's and its committed centres the fixture's to the last bit or the one next to
    it (the device's mean of a list is a float sum in another order) -> the committed centres, which the GPU tests use"""
    n0 = [int(e.sector_info(s)[0]) for s in range(N_SECTORS)]
    assert n0 == counts(), (n0, counts())
    out = []
    for s, (cx, cy) in enumerate(centres()):
        got = tuple(F32(v) for v in e.sector_info(s)[1:3])
        assert abs(got[0] - cx) <= np.spacing(cx) and abs(got[1] - cy) <= np.spacing(cy), (s, got, cx, cy)
        out.append(got)
    return out


def weighted_mask():
    m = np.ones((256, 256), np.uint8)
    m[:, MASK_BAND[0]:MASK_BAND[1]] = 0
    m[:, MASK_BAND_BIG[0]:MASK_BAND_BIG[1]] = 0
    return m


def truth_seeds(scale=1.0):
    """zero-gradient seeds at the true translation"""
    return zr.zero_gradient_seeds(N_SECTORS) * F32(scale)


# ---- the backward reference on this geometry ---------------------------------------------------------------------------------
def backward_problems(oracle, model, interp, und, dfm, sampler=None, centres_=None):
    frames = br.Frames(oracle, interp, und, dfm, sampler=sampler)
    return [br.Problem(frames, model, xy, c0) for xy, c0 in zip(lists(), centres_ if centres_ is not None else centres())]


# The whole solves start at NEAR and run the levels 1 and 0.  From a zero guess over three levels the restatement alone breaks
# the cap below: the coarsest level of the small sectors (18 to 35 samples for six parameters) amplifies the last bits of the
# sums, and the loop's stopping rule (a relative change of chi below 1e-3) leaves a part of that in the result - up to 1e-5 px
# and 6e-6 in the gradient terms between the float64 and the float32 run.
# The four small rectangles sit where the twelve oracle-backed cases settle with a margin, found by a scan of positions with
# the restatement alone (no GPU): the 19 x 19, 27 x 19 and 32 x 16 ones where the two runs are 0.005 of the rule's bound apart
# (most positions settle).  Of the positions of the 3 x 3 one - nine samples for up to six parameters - about one in five
# hundred settles in every case; this one does by 0.02 of the rule's bound.
BW_PY = (0, 1, 1)


def backward_guesses(interp):
    g = np.zeros((N_SECTORS, 6), F32)
    g[:] = NEAR
    return g


UNSETTLED_CAP = {ca.IM_NEAREST: 2, ca.IM_BILINEAR: 0, ca.IM_BICUBIC: 0, ca.IM_BICUBIC_SEPARABLE: 0}


def backward_runs(problems, model, interp, guesses=None, py=BW_PY):
    """-> (float64 runs, float32 runs, settled flags) of every sector; guesses: backward_guesses unless given"""
    g = backward_guesses(interp) if guesses is None else guesses
    r64 = [br.solve_ref(pb, g[s], precision=zr.PRECISION, py=py) for s, pb in enumerate(problems)]
    r32 = [br.solve_ref(pb, g[s], precision=zr.PRECISION, py=py, acc=np.float32) for s, pb in enumerate(problems)]
    return r64, r32, [br.settled(model, a, b) for a, b in zip(r64, r32)]
