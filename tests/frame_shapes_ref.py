"""The fixture of tests/test_frame_shapes_gpu.py: frame pairs whose four dimensions (rows and columns of the undeformed and
of the deformed frame) all differ at every pyramid level, a grid of sectors that reaches into the part of the frame a
transposed bound would clamp or reject, the CPU oracle's records on it, and the helpers of other test modules loaded
by file.  Plain numpy and the oracle: no engine, no GPU."""
import functools
import importlib.util
import os

import numpy as np

import correlation_amd as ca

HERE = os.path.dirname(os.path.abspath(__file__))
TRUTH = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)
SHAPES = {"wide": (150, 232), "tall": (232, 150)}      # (rows, cols): no dimension a multiple of 4
CROP = (11, 19)                                        # rows, columns the unequal pair's deformed frame is short of
SIDE, PITCH, FIRST = 20, 21, 8                         # sectors of 20 x 20 samples every 21 pixels from pixel 8 on
MODELS = (ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY)
OUT_OF_IMAGE = ca.ERROR_INTERPOLATION_OUT_OF_IMAGE


@functools.lru_cache(maxsize=None)
def module(name):
    """tests/<name>.py as a module of its own (its helpers, not its tests)"""
    spec = importlib.util.spec_from_file_location("frame_shapes_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _frames(orientation):
    rows, cols = SHAPES[orientation]
    und, dfm = ca.speckle.speckle_pair(rows, cols, p=TRUTH, seed=7)
    cut = np.ascontiguousarray(dfm[:rows - CROP[0], :cols - CROP[1]])
    for a in (und, dfm, cut):
        a.setflags(write=False)
    return und, dfm, cut


def pair(orientation, which):
    """(und, dfm) of the "equal" or the "unequal" pair"""
    und, dfm, cut = _frames(orientation)
    return und, (dfm if which == "equal" else cut)


def level_shapes(orientation, which, levels=3):
    """[(urows, ucols, drows, dcols)] per pyramid level"""
    und, dfm = pair(orientation, which)
    return [(und.shape[0] >> l, und.shape[1] >> l, dfm.shape[0] >> l, dfm.shape[1] >> l) for l in range(levels)]


class Grid:
    """the sectors of one orientation: x outer, y inner (sector = ix * ny + iy)"""

    def __init__(self, oracle, orientation):
        rows, cols = SHAPES[orientation]
        self.xs = list(range(FIRST, cols - (SIDE - 1), PITCH))
        self.ys = list(range(FIRST, rows - (SIDE - 1), PITCH))
        self.nx, self.ny = len(self.xs), len(self.ys)
        self.corners = [(x0, y0) for x0 in self.xs for y0 in self.ys]
        self.lists = [oracle.rect_points(x0, y0, x0 + SIDE - 1, y0 + SIDE - 1) for x0, y0 in self.corners]
        self.centers = np.array([(x0 + 9, y0 + 9) for x0, y0 in self.corners], np.float32)
        self.rect_centers = np.array([(x0 + 9.5, y0 + 9.5) for x0, y0 in self.corners], np.float32)
        ix, iy = np.divmod(np.arange(len(self.corners)), self.ny)
        self.edge = (ix == self.nx - 1) | (iy == self.ny - 1)      # the last grid column and the last grid row
        self.far_valid = (self.nx - 2) * self.ny + self.ny - 2      # second-to-last row and column
        self.interior = (self.nx // 2) * self.ny + self.ny // 2

    def __len__(self):
        return len(self.corners)

    def register(self, e, first=0, sectors=None):
        for k, s in enumerate(range(len(self)) if sectors is None else sectors):
            e.set_sector_points(first + k, self.lists[s], center=tuple(float(v) for v in self.centers[s]))

    def register_rects(self, e):
        """the same samples as implicit rectangles (lk_set_sector_rect): the engine walks them itself and takes the
        rectangle's own centre, (x0 + 9.5, y0 + 9.5) = self.rect_centers"""
        for s, (x0, y0) in enumerate(self.corners):
            e.resetPolygon_rect(s, x0, y0, x0 + SIDE - 1, y0 + SIDE - 1)


@functools.lru_cache(maxsize=None)
def grid(oracle, orientation):
    return Grid(oracle, orientation)


@functools.lru_cache(maxsize=None)
def oracle_records(oracle, orientation, which, model=ca.FM_UVUXUYVXVY, interp=ca.IM_BICUBIC, threads=1, solver=0, rects=False):
    """the CPU oracle's records of the grid (py_stop 2, zero guess); computed once per case and read-only.  rects: about
    the centres the engine gives implicit rectangles (Grid.register_rects)"""
    und, dfm = pair(orientation, which)
    o = oracle.Oracle(interp=interp, model=model, n_threads=threads, solver=solver)
    o.set_image(0, und)
    o.set_image(1, dfm)
    g = grid(oracle, orientation)
    want = o.correlate_sectors(g.lists, centers=g.rect_centers if rects else g.centers)
    o.close()
    want.setflags(write=False)
    return want


def assert_oracle_counts(oracle, orientation, which, want, label, max_iterations=3):
    """what the oracle gives on this fixture, asserted before anything is compared with it: 60 sectors; all of them
    error 0 on the equal pair; on the unequal pair the last grid row and column (15 sectors: inside the undeformed frame,
    outside the cropped deformed one) carry the out-of-image code and the other 45 error 0.  (At most 3 iterations with the
    bicubic sampler; the nearest sampler's staircase takes up to 19: pass max_iterations=None.)"""
    g = grid(oracle, orientation)
    ok, out = want["error_code"] == 0, want["error_code"] == OUT_OF_IMAGE
    print(f"{label}: {orientation} {which} pair, levels (urows, ucols, drows, dcols) {level_shapes(orientation, which)}: "
          f"oracle {int(ok.sum())} sectors with error 0 / {int(out.sum())} out of the image")
    assert len(want) == len(g) == 60 and int(g.edge.sum()) == 15
    if which == "equal":
        assert ok.all(), want["error_code"]
    else:
        assert np.array_equal(out, g.edge) and np.array_equal(ok, ~g.edge), want["error_code"]
    assert (want["n_points"] == SIDE * SIDE).all()
    assert max_iterations is None or want["iterations"][ok].max() <= max_iterations


# ---- which sample loop runs: the host's choice of a lane group per sector, restated for the printed lines -------------------
GROUP_OF_CLASS = (16, 32, 64, 256, 512, 512)     # lk_engine_state.hpp: kGroupOfClass; the last class is the team's
TEAM_CLASS = 5


def size_class(n0):
    return 0 if n0 <= 512 else 1 if n0 <= 2048 else 2 if n0 <= 8192 else 3 if n0 <= 65536 else 4 if n0 <= 8 * 32768 else 5


def lane_groups(counts, mode="default", force_group=0, force_team=0):
    """The lane group the host is EXPECTED to pick per sector - a restatement that assert_lane_groups holds against the
    engine's own answer (sector_groups()) wherever it is printed: keep it in step with the host's thresholds.
    Lanes per sector for a batch of level-0 sample counts (classify_sectors of lk_engine_sectors.cpp and
    reference_group_of_sector of lk_engine_solve.cpp, one pair in flight): in "reference_order" a 16-lane row or a
    wavefront; in "batch_invariant" the size class alone; in "default" mode the batch's promotions and the two
    environment hooks the tests use.  Returns a list of strings such as "64" or "team of 2 x 512"."""
    cls = [size_class(n) for n in counts]
    if mode == "reference_order":
        return ["16" if c == 0 else "64" for c in cls]
    if mode == "default":
        for c in range(TEAM_CLASS - 1):
            members = [i for i, k in enumerate(cls) if k == c]
            if not members:
                continue
            g = GROUP_OF_CLASS[c]
            waves = len(members) * g // 64
            per_lane = sum(counts[i] for i in members) // len(members) // g
            if (g < 64 and waves < (4096 if g == 16 else 1024) and per_lane >= 4) or (g >= 64 and waves < 2048 and per_lane >= 32):
                for i in members:
                    cls[i] = c + 1
    if force_group in GROUP_OF_CLASS[:4]:
        cls = [GROUP_OF_CLASS.index(force_group)] * len(cls)
    if force_team >= 1:
        cls = [TEAM_CLASS] * len(cls)
    elif mode == "default" and 0 < sum(c >= TEAM_CLASS - 1 for c in cls) <= 128:
        cls = [TEAM_CLASS if c == TEAM_CLASS - 1 else c for c in cls]
    return [f"team of {force_team} x 512" if c == TEAM_CLASS and force_team >= 1 else
            "team x 512" if c == TEAM_CLASS else str(GROUP_OF_CLASS[c]) for c in cls]


def assert_lane_groups(e, expected, counts=None):
    """lane_groups' strings against sector_groups() of the committed engine `e`: the lanes per sector, and for a team the
    width the engine asks for.  A team whose width the batch decides ("team x 512") needs `counts`, the level-0 sample
    counts: classify_sectors asks for ceil(largest team sector / 4096) workgroups, at least 2 and at most 256."""
    groups, team = e.sector_groups()
    assert len(expected) == len(groups)
    n0_max = max([n for n, want in zip(counts or [], expected) if want == "team x 512"], default=0)
    for s, want in enumerate(expected):
        if want.startswith("team of "):
            assert (groups[s], team[s]) == (512, int(want.split()[2])), (s, want, groups[s], team[s])
        elif want == "team x 512":
            assert counts is not None, "a batch-sized team needs the sample counts"
            assert (groups[s], team[s]) == (512, min(max(-(-n0_max // 4096), 2), 256)), (s, want, groups[s], team[s], n0_max)
        else:
            assert (groups[s], team[s]) == (int(want), 0), (s, want, groups[s], team[s])
