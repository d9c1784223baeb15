"""The shared cell grid (csrc/lk_cell_grid.hpp, the grid kernels of csrc/lk_reseed.hip, csrc/lk_neighbours.hpp) on the layouts
of tests/cell_grid_ref.py, where the grid leaves the regime of the other tests' regular lattices: cells grown beyond the
radius, more than 1024 cells in the one-workgroup scan, all sectors in one cell, one row of cells, centres on a cell boundary
to the last bit, free positions up to and beyond two cells outside the grid, centres far from the origin.

  tables     the grid's own tables (HipCorrelationEngine.cell_grid) against the restatement, and each layout's condition
  passes     every pass that looks for neighbours - lk_strain_field, lk_flag_outliers, lk_reseed_plan, lk_track_points,
             lk_field_map, the owner map of lk_residual_map, lk_stereo_strain - against its brute-force float64 restatement,
             with that pass's own checker and tolerance (the strain checker's pitch is the layout's nominal one, radius /
             2.5); counts, statuses and owners exact; the same bytes from a second call
  hooks      the lane groups and storage paths the passes have environment hooks for, on `clustered`
  free       track points, field nodes and map pixels inside the grid, within one cell outside each side, between one and
             two cells and beyond, on `clustered` and `boundary`
  shuffle    `clustered` committed in a shuffled sector order

Sectors are one-sample lists at the layout's centres (lk_set_sector_points with use_center = 1); every pass takes the caller's
records, so nothing is solved.  Each test prints `cell_grid <layout> <pass>: worst error / tolerance`; profiles/cell_grid.txt
holds those of one run."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import speckle
import cell_grid_ref as cg
import outlier_ref as oref
import residual_ref as rr
import stereo_ref as sr
from field_ref import clear_of_the_noise_threshold, field_reference
from test_field_gpu import all_bytes, check_against_reference as check_field
from test_outlier_gpu import COMBOS, check as check_outliers, set_hooks
from test_reseed_gpu import plan_reference
from test_residual_gpu import decode
from test_strain_gpu import check_against_reference as check_strain, strain_reference
from test_track_gpu import check_against_reference as check_track
from track_ref import fresh_state, is_good, track_reference

pytestmark = pytest.mark.gpu

MODEL = ca.FM_UVUXUYVXVY
FRAME = (256, 256)
RECORD_ONLY = ("offset",)               # no images under these centres: the map is left out


def make_engine(pair, cen):
    e = ca.HipCorrelationEngine(fitting_model=MODEL, precision=1e-3, py_stop=2)
    e.set_undeformed_image(pair[0])
    e.set_deformed_image(pair[1])
    inside = np.clip(np.round(cen), 8, 247).astype(np.float32)       # the one sample: a pixel of the frame, wherever the centre is
    for s in range(len(cen)):
        e.set_sector_points(s, inside[s:s + 1], center=(float(cen[s, 0]), float(cen[s, 1])))
    e.commit_sectors()
    assert e.n_sectors == len(cen)
    got = np.float32([e.sector_info(s)[1:] for s in range(0, len(cen), max(1, len(cen) // 50))])
    assert got.tobytes() == cen[::max(1, len(cen) // 50)].tobytes()
    return e


class World:
    """one engine per layout, made on first use, with its grid, records and scale"""

    def __init__(self, pair):
        self.pair, self.made = pair, {}

    def __call__(self, name):
        if name not in self.made:
            first = None
            if name == "boundary":      # the lattice alone says where the cell boundaries are; the centres on them change nothing
                lattice = cg.boundary()
                with make_engine(self.pair, lattice.cen) as e0:
                    first = e0.cell_grid(lattice.radius)
            lay = cg.layout(name, first)
            e = make_engine(self.pair, lay.cen)
            rec = cg.records(lay)
            good = is_good(rec, 6, cg.CHI_MAX)
            self.made[name] = dict(lay=lay, e=e, first=first, grid=e.cell_grid(lay.radius), rec=rec, good=good,
                                   U=float(np.abs(rec["p"][good][:, :2]).max()))
        return self.made[name]

    def close(self):
        for w in self.made.values():
            w["e"].close()


@pytest.fixture(scope="module")
def world():
    w = World(speckle.speckle_pair(256, 256, p=(1.3, -0.7, 0.002, 0.0, 0.0, -0.001), seed=5))
    yield w
    w.close()


def last_call(e, name, kinds):
    """a pass's lk_internal_*_last hook: what its last call chose, after the device time; kinds: "i" int, "d" double"""
    fn = getattr(e.lib, name)
    vals = [C.c_int() if k == "i" else C.c_double() for k in kinds]
    ms = C.c_float()
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_float)] + [C.POINTER(type(v)) for v in vals]
    assert fn(e._h, C.byref(ms), *[C.byref(v) for v in vals]) == 0, name
    return [v.value for v in vals]


def report(layout, what, worst):
    print(f"cell_grid {layout} {what}: worst error / tolerance {worst:.3g}")


# ---- 1. the tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cg.NAMES)
def test_tables_and_the_layout_s_condition(world, name):
    w = world(name)
    lay, grid, e = w["lay"], w["grid"], w["e"]
    S, cells = len(lay.cen), grid["nx"] * grid["ny"]
    cg.check_tables(lay.cen, grid)
    again = e.cell_grid(lay.radius)
    assert all(np.array_equal(grid[k], again[k]) for k in grid)
    count = np.diff(grid["start"].astype(np.int64))
    print(f"cell_grid {name}: {S} sectors, {grid['nx']} x {grid['ny']} cells of {grid['cell']:.6g} px for radius {lay.radius}, "
          f"at most {count.max()} members in a cell, {int((count == 0).sum())} cells empty")
    assert cells <= 4 * S + 1024
    if name in ("clustered", "sparse_line", "offset"):
        assert cg.grew(lay, grid) and cells > 1024
    else:
        assert grid["cell"] == cg.documented_cell(lay.radius) or name == "coincident"
    if name == "sparse_line":
        assert grid["ny"] == 1 and grid["nx"] > 1024 and grid["nx"] % 1024 != 0
    if name == "dense":
        assert 1024 < cells <= 4 * S + 1024 and cells % 1024 != 0 and not cg.grew(lay, grid)
    if name == "coincident":
        assert count.max() >= 100 and (count > 0).sum() <= 3    # (the two centres a radius apart may share a grown cell)
    if name == "one_point":
        assert (grid["nx"], grid["ny"]) == (1, 1) and grid["start"].tolist() == [0, S] and grid["members"].tolist() == list(range(S))
    if name == "boundary":
        first = w["first"]
        assert all(first[k] == grid[k] for k in ("nx", "ny", "cell", "x0", "y0")) and not cg.grew(lay, grid)
        # a centre one ulp below a boundary and the one on it lie in neighbouring cells; the maximum corner is in the last cell
        ix = grid["cell_of"] % grid["nx"]
        extra = slice(cg.BOUNDARY_N ** 2, None)
        assert len(set(ix[extra].tolist())) >= cg.BOUNDARY_N - 2
        t = (lay.cen[extra].astype(np.float64) - np.float64([grid["x0"], grid["y0"]])) / grid["cell"]
        k = np.round(t)
        on = (np.abs(t - k) * grid["cell"] < 1e-3) & (k > 0)
        assert (np.floor(t) < k)[on].sum() >= 15 and (np.floor(t) == k)[on].sum() >= 15       # both sides of the boundaries
        assert grid["cell_of"][cg.BOUNDARY_N ** 2 - 1] == cells - 1
    if name == "offset":
        base = world("clustered")["grid"]
        assert (grid["nx"], grid["ny"], grid["cell"]) == (base["nx"], base["ny"], base["cell"])
        assert np.array_equal(grid["cell_of"], base["cell_of"]) and np.array_equal(grid["members"], base["members"])


# ---- 2. every pass on every layout ----------------------------------------------------------------------------------------------
def cover_window(lay, size=64):
    """size x size nodes over the whole layout and a margin around it -> (window, stride)"""
    c = lay.cen.astype(np.float64)
    lo, hi = np.floor(c.min(axis=0)) - 3, np.ceil(c.max(axis=0)) + 3
    stride = max(1, int(np.ceil((hi - lo).max() / (size - 1))))
    return (int(lo[0]), int(lo[1]), size, size), stride


def map_window(lay, size=64):
    """size x size pixels of the frame around the centre nearest to the centres' mean"""
    c = lay.cen.astype(np.float64)
    mid = c[np.argmin(((c - c.mean(axis=0)) ** 2).sum(1))]
    x0 = int(np.clip(round(mid[0]) - size // 2, 0, FRAME[0] - size))
    y0 = int(np.clip(round(mid[1]) - size // 2, 0, FRAME[1] - size))
    return (x0, y0, size, size)


def owner_reference(cen, good, radius, window, rows=16):
    x0, y0, w, h = window
    return np.concatenate([rr.brute_owner(cen, good, radius, x0, y0 + j, w, min(rows, h - j)) for j in range(0, h, rows)])


def degenerate_only(name):
    return name in ("coincident", "one_point")


@pytest.mark.parametrize("name", cg.NAMES)
def test_strain_field(world, name):
    w = world(name)
    lay, e, rec = w["lay"], w["e"], w["rec"]
    ref = strain_reference(lay.cen, rec, MODEL, lay.radius, cg.CHI_MAX, 3)
    ratio = ref[3][np.isfinite(ref[3])]
    assert not ((ratio > 1e-9) & (ratio < 1e-3)).any()
    live = np.isin(ref[2], (ca.STRAIN_OK, ca.STRAIN_FILLED))
    if degenerate_only(name):
        assert np.isin(ref[2], (ca.STRAIN_DEGENERATE, ca.STRAIN_TOO_FEW)).all()
    else:
        assert 2 * live.sum() >= len(live)
    got = e.strain_field(lay.radius, chi_max=cg.CHI_MAX, min_neighbours=3, records=rec)
    report(name, "strain", check_strain(got, ref, w["U"], name, pitch=cg.pitch(lay)))
    assert got.tobytes() == e.strain_field(lay.radius, chi_max=cg.CHI_MAX, min_neighbours=3, records=rec).tobytes()
    if name == "one_point":
        assert (got["status"] == ca.STRAIN_DEGENERATE).all() and (got["neighbours"] == w["good"].sum()).all()


@pytest.mark.parametrize("name", cg.NAMES)
def test_flag_outliers(world, name):
    w = world(name)
    lay, e, rec = w["lay"], w["e"], w["rec"]
    for detrend, min_nb in ((1, 4), (0, 3)):
        ref = oref.flag_reference(lay.cen, rec, MODEL, lay.radius, cg.CHI_MAX, min_neighbours=min_nb, detrend=bool(detrend), passes=2)
        kw = dict(chi_max=cg.CHI_MAX, min_neighbours=min_nb, detrend=detrend, passes=2, records=rec)
        got, n = e.flag_outliers(lay.radius, **kw)
        report(name, f"outliers detrend={detrend}", check_outliers(got, n, ref, w["U"], detrend, (name, detrend)))
        assert got.tobytes() == e.flag_outliers(lay.radius, **kw)[0].tobytes()
        if degenerate_only(name) and detrend:
            assert np.isin(ref[0]["status"], (ca.OUTLIER_DEGENERATE, ca.OUTLIER_TOO_FEW)).all()
        if name == "one_point" and detrend:
            assert (got["neighbours"] == w["good"].sum() - w["good"]).all()      # all the good ones but the sector itself


@pytest.mark.parametrize("name", cg.NAMES)
def test_reseed_plan(world, name):
    w = world(name)
    lay, e, rec = w["lay"], w["e"], w["rec"]
    for min_nb in (1, 4):
        status, nbrs, want = plan_reference(lay.cen, rec, MODEL, lay.radius, cg.CHI_MAX, min_nb)
        guess, info = e.reseed_plan(rec, lay.radius, chi_max=cg.CHI_MAX, min_neighbours=min_nb)
        assert np.array_equal(info["status"], status) and np.array_equal(info["neighbours"], nbrs), (name, min_nb)
        assert (info["round"] == -1).all() and np.array_equal(info["chi_before"], rec["chi"], equal_nan=True)
        ulp = np.spacing(np.abs(want))
        err = np.abs(guess.astype(np.float64) - want.astype(np.float64))
        assert (err <= ulp).all(), (name, min_nb)
        assert not guess[status != ca.RESEED_PLANNED].any()
        again = e.reseed_plan(rec, lay.radius, chi_max=cg.CHI_MAX, min_neighbours=min_nb)
        assert guess.tobytes() == again[0].tobytes() and info.tobytes() == again[1].tobytes()
        report(name, f"reseed plan min_neighbours={min_nb}", float((err / ulp).max()))
    assert (status != ca.RESEED_GOOD).sum() == (~w["good"]).sum() > 0
    if name == "one_point":     # a failed sector's neighbours: every good one
        assert (nbrs[~w["good"]] == w["good"].sum()).all() and (status[~w["good"]] == ca.RESEED_PLANNED).all()


def track_case(w, pts):
    lay, e, rec = w["lay"], w["e"], w["rec"]
    assert cg.rim_is_exact(lay.cen, lay.radius, pts[np.isfinite(pts).all(axis=1)])
    ref = track_reference(lay.cen, rec[None], MODEL, fresh_state(pts), lay.radius, cg.CHI_MAX, 3, ca.STRAIN_GREEN_LAGRANGE, ca.TRACK_TOTAL)
    assert clear_of_the_noise_threshold(ref[5])
    got, state = e.track_points(pts, lay.radius, records=rec[None], mode=ca.TRACK_TOTAL, chi_max=cg.CHI_MAX)
    worst = check_track(got, ref, w["U"], lay.name)
    again = e.track_points(pts, lay.radius, records=rec[None], mode=ca.TRACK_TOTAL, chi_max=cg.CHI_MAX)
    assert got.tobytes() == again[0].tobytes() and state.tobytes() == again[1].tobytes()
    return got, ref, worst


@pytest.mark.parametrize("name", cg.NAMES)
def test_track_points(world, name):
    w = world(name)
    lay, grid = w["lay"], w["grid"]
    pts = cg.free_points(lay.cen, grid)
    if name == "sparse_line":            # and 1/8 px beside every square: above and below the row they are outside the one row of cells
        pts = np.concatenate([pts, np.float32(cg.sparse_line_points(lay))])
    got, ref, worst = track_case(w, pts)
    report(name, "track", worst)
    if name == "sparse_line":
        assert grid["ny"] == 1
        band_y = cg.band_of(pts[:, 1].astype(np.float64), grid["y0"], grid["y0"] + grid["cell"], grid["cell"])
        band_x = cg.band_of(pts[:, 0].astype(np.float64), grid["x0"], grid["x0"] + grid["nx"] * grid["cell"], grid["cell"])
        outside = (band_y == 1) & (got["neighbours"][0] > 0)
        print(f"  track points within one cell above or below the row of cells, with neighbours: {int(outside.sum())}; "
              f"left or right of it: {int(((band_x == 1) & (got['neighbours'][0] > 0)).sum())}")
        assert (outside & (pts[:, 1] > 128.125)).sum() >= 10 and (outside & (pts[:, 1] < 128.0)).sum() >= 10
        assert ((band_x == 1) & (got["neighbours"][0] > 0)).any()
    if degenerate_only(name):
        assert np.isin(ref[2], (ca.TRACK_DEGENERATE, ca.TRACK_TOO_FEW)).all() and (ref[2] == ca.TRACK_DEGENERATE).any()
    else:
        assert (ref[2] == ca.TRACK_OK).sum() >= 10


def field_case(w, window, stride=1):
    lay, e, rec = w["lay"], w["e"], w["rec"]
    kw = dict(stride=stride, chi_max=cg.CHI_MAX)
    ref = field_reference(lay.cen, rec, MODEL, lay.radius, window, **kw)
    assert clear_of_the_noise_threshold(ref["spread"])
    got = e.field_map(lay.radius, window, channels=ca.FIELD_ALL, records=rec, **kw)
    worst = check_field(got, ref, w["U"], (lay.name, window))
    assert all_bytes(got) == all_bytes(e.field_map(lay.radius, window, channels=ca.FIELD_ALL, records=rec, **kw))
    return got, ref, worst


def nodes_of(window, stride=1):
    x0, y0, nx, ny = window
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([x0 + ii * stride, y0 + jj * stride], 2).astype(np.float64)


@pytest.mark.parametrize("name", cg.NAMES)
def test_field_map(world, name):
    w = world(name)
    # (the nodes are integers and sparse_line's radius is 1/8 px: only a window of stride 1 over the row has nodes with neighbours)
    window, stride = (cg.sparse_line_window(w["lay"]), 1) if name == "sparse_line" else cover_window(w["lay"])
    assert cg.rim_is_exact(w["lay"].cen, w["lay"].radius, nodes_of(window, stride).reshape(-1, 2))
    got, ref, worst = field_case(w, window, stride)
    report(name, f"field stride {stride}", worst)
    seen = np.bincount(ref["status"].ravel(), minlength=3)
    print(f"  field nodes: statuses {seen.tolist()}, {int((ref['neighbours'] > 0).sum())} with neighbours")
    if degenerate_only(name):
        assert seen[ca.FIELD_OK] == 0 and seen[ca.FIELD_DEGENERATE] > 0
    elif name == "sparse_line":          # a node sees a fit only on the (x, 128) corner of a square with an integer x, all three good
        assert seen[ca.FIELD_OK] >= 2 and (ref["neighbours"] > 0).sum() >= 4
        assert (got["neighbours"][ref["status"] == ca.FIELD_OK] == 3).all()
    else:
        assert seen[ca.FIELD_OK] >= 20


@pytest.mark.parametrize("name", [n for n in cg.NAMES if n not in RECORD_ONLY])
def test_owner_map(world, name):
    w = world(name)
    lay, e, rec = w["lay"], w["e"], w["rec"]
    good = rr.good_records(rec, MODEL, cg.CHI_MAX)
    assert np.array_equal(good, w["good"])
    window = cg.sparse_line_window(lay) if name == "sparse_line" else map_window(lay)
    assert cg.rim_is_exact(lay.cen, lay.radius, nodes_of(window).reshape(-1, 2))
    want = owner_reference(lay.cen, good, lay.radius, window)
    owner = e.residual_map(lay.radius, window, records=rec, chi_max=cg.CHI_MAX, want=("owner",))[2]
    assert np.array_equal(decode(owner), want), (name, int((decode(owner) != want).sum()))
    assert owner.tobytes() == e.residual_map(lay.radius, window, records=rec, chi_max=cg.CHI_MAX, want=("owner",))[2].tobytes()
    _, tiles, fallback = e.residual_last()
    print(f"cell_grid {name} owner map: {int((want >= 0).sum())} of {want.size} pixels owned, exact; {fallback} of {tiles} tiles walked global memory")
    assert (want >= 0).any() and ((want == -1).any() or name in ("dense", "boundary"))
    assert not np.isin(want[want >= 0], np.flatnonzero(~good)).any()


def stereo_case(w):
    lay, rec = w["lay"], w["rec"]
    ref_pts, pts = cg.stereo_points(lay, rec)
    ref = sr.surface_reference(lay.cen, ref_pts, pts, lay.radius, 3)
    ratio, edge = ref[3][..., 0], ref[3][..., 1]
    assert not ((ratio > 1e-9) & (ratio < 1e-3)).any() and not (edge < 1e-3).any()
    return ref_pts, pts, ref


@pytest.mark.parametrize("name", cg.NAMES)
def test_stereo_strain(world, name):
    w = world(name)
    lay, e = w["lay"], w["e"]
    ref_pts, pts, ref = stereo_case(w)
    got = e.stereo_strain(lay.radius, ref_pts, pts, min_neighbours=3)
    report(name, "stereo strain", sr.check_surface(got, ref, name))
    assert got.tobytes() == e.stereo_strain(lay.radius, ref_pts, pts, min_neighbours=3).tobytes()
    if degenerate_only(name):
        assert np.isin(ref[2], (ca.STEREO_SURFACE_DEGENERATE, ca.STEREO_SURFACE_TOO_FEW)).all()
    else:
        assert 2 * np.isin(ref[2], (ca.STEREO_SURFACE_OK, ca.STEREO_SURFACE_FILLED)).sum() >= ref[2].size


# ---- 3. lane groups and storage paths, where the cells have grown -----------------------------------------------------------------
def test_lane_groups_and_storage_paths_on_clustered(world, monkeypatch):
    """The lane group is chosen from 9 S / cells expected members, which says little once the cells have grown: every forced
    choice must still meet the restatement (the order of the double sums differs by design) and give the default's integers;
    the walked field map and the plain outlier test give the default's bytes."""
    w = world("clustered")
    lay, e, rec, U = w["lay"], w["e"], w["rec"], w["U"]
    assert cg.grew(lay, w["grid"])

    def env(**kw):
        for k, v in kw.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)

    ref = strain_reference(lay.cen, rec, MODEL, lay.radius, cg.CHI_MAX, 3)
    for group, packed in ((None, None), ("16", "1"), ("64", "1"), ("16", "0"), ("64", "0")):
        env(LK_STRAIN_GROUP=group, LK_STRAIN_PACKED=packed)
        got = e.strain_field(lay.radius, chi_max=cg.CHI_MAX, records=rec)
        ran_group, ran_packed, members = last_call(e, "lk_internal_strain_last", "iid")
        if group is None:       # the default: 16 lanes, packed - 9 S / cells says 1.6 members where a window holds up to 15
            assert (ran_group, ran_packed) == (16, 1) and members < 2.0
        else:
            assert (ran_group, ran_packed) == (int(group), int(packed))
        report("clustered", f"strain group {group} packed {packed}", check_strain(got, ref, U, (group, packed), pitch=cg.pitch(lay)))
    env(LK_STRAIN_GROUP=None, LK_STRAIN_PACKED=None)

    for detrend in (0, 1):
        oref_ = oref.flag_reference(lay.cen, rec, MODEL, lay.radius, cg.CHI_MAX, min_neighbours=4, detrend=bool(detrend), passes=2)
        first = None
        for group, cap in COMBOS:
            set_hooks(monkeypatch, group, cap)
            got, n = e.flag_outliers(lay.radius, chi_max=cg.CHI_MAX, min_neighbours=4, detrend=detrend, passes=2, records=rec)
            ran_group, ran_rows, _ = last_call(e, "lk_internal_outlier_last", "iid")
            if group is None:
                default_rows = ran_rows
                assert ran_group == 16 and ran_rows > 2
            else:
                assert ran_group == int(group) and ran_rows == (default_rows if cap is None else int(cap) // int(group))
            report("clustered", f"outliers detrend={detrend} group {group} cap {cap}", check_outliers(got, n, oref_, U, detrend, (detrend, group, cap)))
            first = got if first is None else first
            if not detrend:
                assert got.tobytes() == first.tobytes()
    set_hooks(monkeypatch, None, None)

    pts = cg.free_points(lay.cen, w["grid"])
    tref = track_reference(lay.cen, rec[None], MODEL, fresh_state(pts), lay.radius, cg.CHI_MAX, 3, ca.STRAIN_GREEN_LAGRANGE, ca.TRACK_TOTAL)
    for group in (None, "16", "64"):
        env(LK_TRACK_GROUP=group)
        got, _ = e.track_points(pts, lay.radius, records=rec[None], mode=ca.TRACK_TOTAL, chi_max=cg.CHI_MAX)
        assert last_call(e, "lk_internal_track_last", "id")[0] == (16 if group is None else int(group))
        report("clustered", f"track group {group}", check_track(got, tref, U, group))
    env(LK_TRACK_GROUP=None)

    ref_pts, spts, sref = stereo_case(w)
    for group in (None, "16", "64"):
        env(LK_STEREO_GROUP=group)
        got = e.stereo_strain(lay.radius, ref_pts, spts, min_neighbours=3)
        assert e.stereo_last()[1] == (16 if group is None else int(group))
        report("clustered", f"stereo strain group {group}", sr.check_surface(got, sref, group))
    env(LK_STEREO_GROUP=None)

    window, stride = cover_window(lay)
    out = {}
    for walk in ("0", "1"):
        env(LK_FIELD_WALK=walk)
        out[walk] = e.field_map(lay.radius, window, stride=stride, channels=ca.FIELD_ALL, records=rec, chi_max=cg.CHI_MAX)
        _, tiles, fallback = e.field_last()
        print(f"cell_grid clustered field LK_FIELD_WALK={walk}: {fallback} of {tiles} tiles walked global memory")
        assert tiles == 16 and fallback == (tiles if walk == "1" else 0), (walk, tiles, fallback)
    env(LK_FIELD_WALK=None)
    assert all_bytes(out["0"]) == all_bytes(out["1"]) and np.isfinite(out["0"]["u"]).sum() > 20


def test_map_walks_global_memory_when_one_cell_holds_more_than_a_tile_stages(world, monkeypatch):
    """The residual map has no hook for its storage path: a tile walks global memory when the cells it reaches hold more
    members than its LDS takes (512).  600 sectors on one centre are one cell of 600: every tile near it takes the walk, whose
    one row is the whole member table; the field map stages them (1024) unless told to walk."""
    lay = cg.one_point()
    cen = np.float32(np.tile(lay.cen[:1], (600, 1)))
    rec = cg.records(cg.Layout("one_point", cen, lay.radius))
    good = rr.good_records(rec, MODEL, cg.CHI_MAX)
    window = map_window(lay, size=32)
    with make_engine(world.pair, cen) as e:
        grid = e.cell_grid(lay.radius)
        cg.check_tables(cen, grid)
        assert (grid["nx"], grid["ny"]) == (1, 1) and grid["members"].tolist() == list(range(600))
        owner = e.residual_map(lay.radius, window, records=rec, chi_max=cg.CHI_MAX, want=("owner",))[2]
        _, tiles, fallback = e.residual_last()
        assert tiles == 4 and 0 < fallback <= tiles, (tiles, fallback)
        want = owner_reference(cen, good, lay.radius, window)
        assert np.array_equal(decode(owner), want) and (want >= 0).sum() >= 20 and (want == -1).any()
        assert set(want[want >= 0].tolist()) == {int(np.flatnonzero(good)[0])}          # the lowest good index of the 600
        out = {}
        for walk in ("0", "1"):
            monkeypatch.setenv("LK_FIELD_WALK", walk)
            out[walk] = e.field_map(lay.radius, window, channels=ca.FIELD_ALL, records=rec, chi_max=cg.CHI_MAX)
            assert e.field_last()[2] == (0 if walk == "0" else e.field_last()[1])
        monkeypatch.delenv("LK_FIELD_WALK")
        assert all_bytes(out["0"]) == all_bytes(out["1"])
        ref = field_reference(cen, rec, MODEL, lay.radius, window, chi_max=cg.CHI_MAX)
        check_field(out["0"], ref, 1.0, "600 on one centre")
        assert (ref["status"] == ca.FIELD_DEGENERATE).sum() >= 20 and ref["neighbours"].max() == good.sum()


# ---- 4. free positions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clustered", "boundary"])
def test_free_positions_inside_and_up_to_beyond_two_cells_outside(world, name):
    w = world(name)
    lay, e, rec, grid = w["lay"], w["e"], w["rec"], w["grid"]
    # track points: on centres, and in the four windows over the sides
    pts = np.concatenate([cg.free_points(lay.cen, grid, seed=1), np.float32([[1e6, 100.0]])])
    band = cg.bands_of_points(pts, grid)
    assert all((band == b).sum() >= 10 for b in range(3)) and (band == 3).sum() >= 10
    got, ref, worst = track_case(w, pts)
    report(name, "track, free positions", worst)
    far = cg.nearest_distance(lay.cen, pts) > lay.radius
    assert far[band == 3].all() and (~far[band <= 2]).any() and (~far[band == 1]).any()
    assert not got["neighbours"][0][far].any() and (got["status"][0][far] == ca.TRACK_TOO_FEW).all()
    for b in range(4):
        print(f"  track points {cg.BANDS[b]}: {int((band == b).sum())}, of them with neighbours {int((got['neighbours'][0][band == b] > 0).sum())}")
    # field nodes and map pixels: a window over each side of the grid
    good = rr.good_records(rec, MODEL, cg.CHI_MAX)
    worst_field, near_nodes, near_pixels = 0.0, 0, 0     # (near: within one cell outside the grid, and with a neighbour)
    for window, clipped in zip(cg.side_windows(lay.cen, grid), cg.side_windows(lay.cen, grid, frame=FRAME)):
        nodes = nodes_of(window).reshape(-1, 2)
        band = cg.bands_of_points(nodes, grid)
        assert all((band == b).any() for b in range(4)), window
        assert cg.rim_is_exact(lay.cen, lay.radius, nodes)
        fgot, fref, worst = field_case(w, window)
        worst_field = max(worst_field, worst)
        far = (cg.nearest_distance(lay.cen, nodes) > lay.radius).reshape(fref["status"].shape)
        assert far.ravel()[band == 3].all()
        near_nodes += int((fref["neighbours"].ravel()[band == 1] > 0).sum())
        assert not fgot["neighbours"][far].any() and (fgot["status"][far] == ca.FIELD_TOO_FEW).all()
        pixels = nodes_of(clipped).reshape(-1, 2)
        pband = cg.bands_of_points(pixels, grid)
        assert all((pband == b).any() for b in range(4)), clipped
        want = owner_reference(lay.cen, good, lay.radius, clipped)
        owner = e.residual_map(lay.radius, clipped, records=rec, chi_max=cg.CHI_MAX, want=("owner",))[2]
        assert np.array_equal(decode(owner), want), (name, clipped)
        pfar = (cg.nearest_distance(lay.cen, pixels) > lay.radius).reshape(want.shape)
        assert (owner[pfar] == -1).all()
        near_pixels += int((want.ravel()[pband == 1] >= 0).sum())
    print(f"  within one cell outside the grid: {near_nodes} field nodes with neighbours, {near_pixels} map pixels with an owner")
    assert near_nodes > 0 and near_pixels > 0
    report(name, "field, free positions", worst_field)


# ---- 5. a shuffled sector order ---------------------------------------------------------------------------------------------------
def test_shuffled_sector_order_on_clustered(world):
    """The same centres and records committed in another order.  What the header promises to be independent of the visiting
    order - every integer, the plain outlier test's floats - comes back byte for byte under the permutation; the sums of the
    plane fits are added in sector order, so their floats meet the restatement's tolerance instead."""
    w = world("clustered")
    lay, e, rec, U = w["lay"], w["e"], w["rec"], w["U"]
    S = len(lay.cen)
    perm = np.random.default_rng(99).permutation(S)          # shuffled sector i is sector perm[i]
    cen2, rec2 = lay.cen[perm], rec[perm]

    def back(a):
        out = np.zeros_like(a)
        out[..., perm] = a
        return out

    with make_engine(world.pair, cen2) as e2:
        grid2 = e2.cell_grid(lay.radius)
        cg.check_tables(cen2, grid2)
        assert np.array_equal(back(grid2["cell_of"]), w["grid"]["cell_of"])
        kw = dict(chi_max=cg.CHI_MAX, records=rec)
        kw2 = dict(chi_max=cg.CHI_MAX, records=rec2)
        # strain
        a, b = e.strain_field(lay.radius, **kw), back(e2.strain_field(lay.radius, **kw2))
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["neighbours"], b["neighbours"])
        ref = strain_reference(lay.cen, rec, MODEL, lay.radius, cg.CHI_MAX, 3)
        report("clustered", "strain, shuffled", check_strain(b, ref, U, "shuffled", pitch=cg.pitch(lay)))
        # outliers: plain mode byte for byte, detrended within the tolerance
        a, na = e.flag_outliers(lay.radius, min_neighbours=3, detrend=0, passes=2, **kw)
        b, nb = e2.flag_outliers(lay.radius, min_neighbours=3, detrend=0, passes=2, **kw2)
        assert na == nb and a.tobytes() == back(b).tobytes()
        b, nb = e2.flag_outliers(lay.radius, min_neighbours=4, detrend=1, passes=2, **kw2)
        oref_ = oref.flag_reference(lay.cen, rec, MODEL, lay.radius, cg.CHI_MAX, min_neighbours=4, detrend=True, passes=2)
        report("clustered", "outliers detrend=1, shuffled", check_outliers(back(b), nb, oref_, U, 1, "shuffled"))
        # the plan
        status, nbrs, want = plan_reference(lay.cen, rec, MODEL, lay.radius, cg.CHI_MAX, 1)
        guess, info = e2.reseed_plan(rec2, lay.radius, chi_max=cg.CHI_MAX, min_neighbours=1)
        assert np.array_equal(back(info["status"]), status) and np.array_equal(back(info["neighbours"]), nbrs)
        moved = np.zeros_like(guess)
        moved[perm] = guess
        guess = moved
        assert (np.abs(guess.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
        # free positions do not move: tracks, nodes, pixels
        pts = cg.free_points(lay.cen, w["grid"])
        a, _ = e.track_points(pts, lay.radius, records=rec[None], mode=ca.TRACK_TOTAL, chi_max=cg.CHI_MAX)
        b, _ = e2.track_points(pts, lay.radius, records=rec2[None], mode=ca.TRACK_TOTAL, chi_max=cg.CHI_MAX)
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["neighbours"], b["neighbours"])
        tref = track_reference(lay.cen, rec[None], MODEL, fresh_state(pts), lay.radius, cg.CHI_MAX, 3, ca.STRAIN_GREEN_LAGRANGE, ca.TRACK_TOTAL)
        report("clustered", "track, shuffled", check_track(b, tref, U, "shuffled"))
        window = cg.side_windows(lay.cen, w["grid"])[1]
        a = e.field_map(lay.radius, window, channels=ca.FIELD_ALL, **kw)
        b = e2.field_map(lay.radius, window, channels=ca.FIELD_ALL, **kw2)
        assert a["status"].tobytes() == b["status"].tobytes() and a["neighbours"].tobytes() == b["neighbours"].tobytes()
        fref = field_reference(lay.cen, rec, MODEL, lay.radius, window, chi_max=cg.CHI_MAX)
        report("clustered", "field, shuffled", check_field(b, fref, U, "shuffled"))
        # the owner is the lowest index among equally near sectors: the shuffled map against the rule on the shuffled centres
        mw = map_window(lay)
        good2 = rr.good_records(rec2, MODEL, cg.CHI_MAX)
        owner2 = e2.residual_map(lay.radius, mw, records=rec2, chi_max=cg.CHI_MAX, want=("owner",))[2]
        want2 = owner_reference(cen2, good2, lay.radius, mw)
        assert np.array_equal(decode(owner2), want2)
        owner = decode(e.residual_map(lay.radius, mw, records=rec, chi_max=cg.CHI_MAX, want=("owner",))[2])
        assert np.array_equal(owner >= 0, want2 >= 0)
        c, px = lay.cen.astype(np.float64), nodes_of(mw)
        held = owner >= 0                                                      # as near, whichever of two equally near sectors
        assert np.array_equal(((c[owner[held]] - px[held]) ** 2).sum(1), ((c[perm[want2[held]]] - px[held]) ** 2).sum(1))
        # stereo strain
        ref_pts, spts, sref = stereo_case(w)
        b = e2.stereo_strain(lay.radius, ref_pts[perm], spts[:, perm], min_neighbours=3)
        report("clustered", "stereo strain, shuffled", sr.check_surface(back(b), sref, "shuffled"))
