"""Conditions on the inputs of tests/test_cell_grid_gpu.py, computed from the float64 restatements alone (no GPU): the layouts
are what tests/cell_grid_ref.py says they are, the windows are not vacuous, and no window sits where a changed summation
order could flip a status or a membership.  The seeds of the layouts and records were chosen so that these hold."""
import numpy as np
import pytest

import correlation_amd as ca
import cell_grid_ref as cg
import outlier_ref as oref
from test_strain_gpu import strain_reference

LIVE = [n for n in cg.NAMES if n not in ("coincident", "one_point")]
REFERENCES = {}


def strain_ref(name):
    if name not in REFERENCES:
        lay = cg.layout(name)
        REFERENCES[name] = (lay, strain_reference(lay.cen, cg.records(lay), ca.FM_UVUXUYVXVY, lay.radius, cg.CHI_MAX, 3))
    return REFERENCES[name]


@pytest.mark.parametrize("name", cg.NAMES)
def test_layouts_are_what_they_say(name):
    lay = cg.layout(name)
    c = lay.cen.astype(np.float64)
    assert lay.cen.dtype == np.float32 and lay.radius == np.float32(lay.radius) and len(c) <= 3025
    if name == "offset":
        assert np.array_equal(c - np.float64(cg.OFFSET), cg.layout("clustered").cen.astype(np.float64))
    else:
        assert c.min() >= 0.0 and c.max() <= 255.0
    exact = cg.is_exact(lay.cen)
    if name == "boundary":
        lat = cg.boundary_lattice()
        assert np.array_equal(lay.cen[:len(lat)], lat) and exact[:len(lat)].all() and not exact[len(lat):].all()
        assert (lay.cen == lay.cen.max(axis=0)).all(axis=1).any()          # the bounding box's maximum corner is a centre
        # the added centres sit on the documented cell boundaries as floats, on them, one ulp below or one ulp above
        cell = cg.documented_cell(lay.radius)
        on = np.float32(cg.BOUNDARY_X0 + np.arange(1, cg.BOUNDARY_N - 1) * cell)
        extra = lay.cen[len(lat):]
        kind = np.stack([np.isin(np.nextafter(extra, np.float32(np.inf)), on), np.isin(extra, on),
                         np.isin(np.nextafter(extra, np.float32(-np.inf)), on)])            # below, on, above [3][63][2]
        assert len(extra) == 63 and kind.any(axis=(0, 2)).all() and (kind.sum(axis=(1, 2)) >= 20).all()
        assert kind.any(axis=0).all(axis=1).sum() == 4                                      # on a boundary in x and in y
        # and the record of the lattice point each of them stands in for is bad
        bad = ~oref.is_good(cg.records(lay), 6, cg.CHI_MAX)
        d = np.abs(c[:len(lat), None, :] - c[None, len(lat):, :]).max(axis=2)
        assert (d.min(axis=0) < 2e-4).all() and bad[:len(lat)][(d < 2e-4).any(axis=1)].all()
    else:
        assert exact.all()
    assert cg.rim_is_exact(lay.cen, lay.radius)
    d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(2) if len(c) <= 700 else None
    r2 = float(np.float32(lay.radius)) ** 2
    if name in ("sparse_line", "boundary", "coincident"):
        assert (d2 == r2).any()                                            # neighbours at exactly the radius
    if name == "clustered":
        assert len(c) == 600
        own = d2[:15, :15]
        assert own.max() <= r2 and np.sqrt(own.max()) > 0.7 * lay.radius   # a cluster is about one radius across
    if name == "sparse_line":
        assert len(c) == 100 and np.ptp(c[:, 1]) == lay.radius
    if name == "coincident":
        assert len(c) == 300 and len({tuple(r) for r in lay.cen}) == 3
    if name == "one_point":
        assert len(c) == 64 and len({tuple(r) for r in lay.cen}) == 1


@pytest.mark.parametrize("name", LIVE)
def test_windows_are_not_vacuous_and_clear_of_the_thresholds(name):
    lay, ref = strain_ref(name)
    vals, nbrs, status, ratio = ref
    live = np.isin(status, (ca.STRAIN_OK, ca.STRAIN_FILLED))
    print(f"{name}: statuses {np.bincount(status, minlength=4).tolist()}, neighbours {nbrs.min()}..{nbrs.max()}, median {np.median(nbrs)}")
    assert 2 * live.sum() >= len(status)
    r = ratio[np.isfinite(ratio)]
    assert not ((r > 1e-9) & (r < 1e-3)).any(), r[(r > 1e-9) & (r < 1e-3)]
    if name == "dense":
        assert np.median(nbrs) >= 5
    bad = ~oref.is_good(cg.records(lay), 6, cg.CHI_MAX)
    if name == "boundary":               # (the lattice points that a centre on a cell boundary stands in for are bad besides)
        bad = bad[cg.BOUNDARY_N ** 2:]
    assert 0.10 <= bad.mean() <= 0.20, bad.mean()


@pytest.mark.parametrize("name", ["coincident", "one_point"])
def test_coincident_centres_are_degenerate_or_too_few(name):
    lay, ref = strain_ref(name)
    assert np.isin(ref[2], (ca.STRAIN_DEGENERATE, ca.STRAIN_TOO_FEW)).all() and (ref[2] == ca.STRAIN_DEGENERATE).any()
    if name == "one_point":
        good = oref.is_good(cg.records(lay), 6, cg.CHI_MAX)
        assert (ref[1] == good.sum()).all() and (ref[2] == ca.STRAIN_DEGENERATE).all()


@pytest.mark.parametrize("name", LIVE)
def test_no_outlier_ratio_sits_at_the_threshold(name):
    """tests/test_outlier_gpu.py's condition on the inputs, for the detrended comparison of the GPU test"""
    lay = cg.layout(name)
    rec = cg.records(lay)
    want, ratio, _ = oref.flag_reference(lay.cen, rec, ca.FM_UVUXUYVXVY, lay.radius, cg.CHI_MAX, 0.02, 3.0, 4, True, 1)
    good = oref.is_good(rec, 6, cg.CHI_MAX)
    U = float(np.abs(rec["p"][good][:, :2]).max())
    tol = oref.tolerances(want, U, 0.02)
    live = np.isin(want["status"], (ca.OUTLIER_OK, ca.OUTLIER_FLAGGED))
    for k, key in enumerate(("ratio_u", "ratio_v")):
        assert (np.abs(ratio[live, k] - 3.0) > tol[key][live]).all()


def test_tables_restatement_on_a_hand_made_grid():
    cen = np.float32([[0, 0], [3.9, 0], [4, 0], [8, 4], [0.5, 4], [8, 0], [1, 1]])
    grid = dict(nx=3, ny=2, cell=4.0, x0=0.0, y0=0.0)
    cell_of, start, members = cg.tables_reference(cen, grid)
    assert cell_of.tolist() == [0, 0, 1, 5, 3, 2, 0]         # (8, 4) would be cell (2, 1): the last one, no clamp needed here
    assert start.tolist() == [0, 3, 4, 5, 6, 6, 7] and members.tolist() == [0, 1, 6, 2, 5, 4, 3]
    grid = dict(nx=2, ny=1, cell=4.0, x0=0.0, y0=0.0)        # a grid too small for them: the clamp
    assert cg.tables_reference(cen, grid)[0].tolist() == [0, 0, 1, 1, 0, 1, 0]
    assert cg.band_of(np.float64([5, -0.5, -4, -4.5, -8.5, 12.5, 16.5, 30]), 0.0, 12.0, 4.0).tolist() == [0, 1, 1, 2, 3, 1, 2, 3]


def test_sparse_line_has_nodes_and_points_with_neighbours():
    """The field map's and the owner map's nodes are integers and the radius of `sparse_line` is 1/8 px: the window of
    cg.sparse_line_window holds squares with an integer x, whose corner nodes have neighbours and fits; the track points of
    cg.sparse_line_points lie 1/8 px above and below the row, outside its one row of cells, one radius from a corner."""
    import residual_ref as rr
    from field_ref import field_reference
    lay = cg.layout("sparse_line")
    rec = cg.records(lay)
    window = cg.sparse_line_window(lay)
    assert window[2:] == (64, 64) and window[1] <= 128 < window[1] + 64
    ref = field_reference(lay.cen, rec, ca.FM_UVUXUYVXVY, lay.radius, window, chi_max=cg.CHI_MAX)
    assert (ref["status"] == ca.FIELD_OK).sum() >= 2 and (ref["neighbours"] > 0).sum() >= 4
    own = rr.brute_owner(lay.cen, rr.good_records(rec, ca.FM_UVUXUYVXVY, cg.CHI_MAX), lay.radius, *window)
    assert (own >= 0).sum() >= 4
    pts = cg.sparse_line_points(lay)
    c = lay.cen.astype(np.float64)
    at = (((pts[:, None, :] - c[None, :, :]) ** 2).sum(2) == lay.radius ** 2).sum(1)
    assert len(pts) == 100 and (at >= 1).all() and ((pts[:, 1] > 128.125) | (pts[:, 1] < 128.0)).sum() == 50
