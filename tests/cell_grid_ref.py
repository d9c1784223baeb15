"""The layouts of tests/test_cell_grid_gpu.py and tests/test_cell_grid_host.py, and a numpy restatement of what the tables of
the shared cell grid hold (csrc/lk_cell_grid.hpp, csrc/lk_neighbours.hpp, the grid kernels of csrc/lk_reseed.hip).

The restatement takes the grid's geometry - nx, ny, cell, x0, y0 - as the library reports it (HipCorrelationEngine.cell_grid)
and says what the tables must then contain; it does not restate the rule that sizes the grid:
  cell_of   iy nx + ix, with ix = the floor of (c.x - x0) / cell in double, clamped to 0 .. nx - 1, iy alike
  start     the exclusive prefix of the cells' member counts, start[nx ny] = S
  members   the sectors of cell k at start[k] .. start[k + 1] - 1, ascending by sector index: a permutation of 0 .. S - 1

Layouts are functions of fixed seeds.  Every coordinate is a multiple of 1/8 px (the few centres that `boundary` puts on
the cell boundaries excepted), so every difference, square and sum of squares is exact in double on both sides, and a
neighbour AT the radius is one on both sides.  Except for `offset`, all centres lie inside a 256 x 256 frame.

  clustered    40 clusters of 15 sectors, cluster diameter = radius = 2.5 px, spread over 40 .. 216: the radius is small
               against the domain, the cells grow beyond it
  sparse_line  25 squares of four centres, side 1/8 px = radius, along one row: the row is one cell high (ny = 1), and so
               long against the radius that the cells grow; a centre's window is its square's three nearest corners, two of
               them at exactly the radius
  dense        55 x 55 lattice of pitch 4.5 px jittered by up to 1 px, radius 7 px: more than 1024 cells, no growth
  coincident   300 sectors on three centres, two of them exactly one radius apart
  one_point    64 sectors on one centre: one cell
  boundary     a 12 x 12 lattice of pitch = radius = 12 px (the four nearest neighbours at exactly the radius, the bounding
               box's maximum corner a lattice point), and 63 centres at x0 + k cell rounded to float, one ulp below or one ulp
               above, in x, in y and in both: `cell`, `x0`, `y0` are the grid's, as reported for the lattice alone.  Such a
               centre lies 1e-5 .. 1e-4 px from a lattice point, whose record is made bad: the centre on the boundary stands
               in for it in every window, and no window holds two members that nearly coincide (a window of such pairs on a
               line would have a spread of 1e-10 of its extent, where no float64 fit is meaningful)
  offset       `clustered` translated by (-5000.25, 7000.5): float spacing 2^-11 px

The nominal pitch of a layout, radius / 2.5, stands where a tolerance of the passes' checkers carries the pitch of their own
lattice."""
from collections import namedtuple

import numpy as np

import correlation_amd as ca
from records_ref import synthetic_records
from track_ref import is_good

Layout = namedtuple("Layout", "name cen radius")

CHI_MAX = 8.0
SHARE = 0.05            # of the sectors made bad in EACH of three ways (error code, NaN, chi): 15 % in all
OFFSET = (-5000.25, 7000.5)
NAMES = ("clustered", "sparse_line", "dense", "coincident", "one_point", "boundary", "offset")
BOUNDARY_N, BOUNDARY_X0, BOUNDARY_RADIUS = 12, 60.0, 12.0


def eighths(x):
    return np.round(np.asarray(x, np.float64) * 8.0) / 8.0


def is_exact(cen):
    """[S]: both coordinates are multiples of 1/8"""
    c = np.asarray(cen, np.float32).astype(np.float64) * 8.0
    return (c == np.round(c)).all(axis=1)


def clustered(seed=11):
    rng = np.random.default_rng(seed)
    mid = eighths(rng.uniform(40.0, 216.0, (40, 2)))
    k = np.arange(-10, 11) / 8.0
    ox, oy = np.meshgrid(k, k)
    disc = np.stack([ox.ravel(), oy.ravel()], 1)
    disc = disc[(disc ** 2).sum(1) <= 1.25 ** 2]
    cen = np.concatenate([m + disc[rng.permutation(len(disc))[:15]] for m in mid])
    return Layout("clustered", np.float32(cen), 2.5)


def sparse_line(seed=5):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.permutation(np.arange(8 * 8, 247 * 8, 4))[:25]) / 8.0       # at least 1/2 px between two squares
    corner = np.float64([[0, 0], [0.125, 0], [0, 0.125], [0.125, 0.125]])
    cen = np.concatenate([np.float64([xx, 128.0]) + corner for xx in x])
    return Layout("sparse_line", np.float32(cen), 0.125)


def dense(seed=3):
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(55), np.arange(55), indexing="ij")
    cen = 5.0 + 4.5 * np.stack([i.ravel(), j.ravel()], 1) + rng.integers(-8, 9, (55 * 55, 2)) / 8.0
    return Layout("dense", np.float32(cen), 7.0)


def coincident():
    three = np.float64([[64.0, 64.0], [66.0, 64.0], [192.5, 160.25]])
    return Layout("coincident", np.float32(three[np.arange(300) % 3]), 2.0)


def one_point():
    return Layout("one_point", np.float32(np.tile([[100.5, 77.25]], (64, 1))), 3.0)


def boundary_lattice():
    i, j = np.meshgrid(np.arange(BOUNDARY_N), np.arange(BOUNDARY_N), indexing="ij")
    return np.float32(BOUNDARY_X0 + BOUNDARY_RADIUS * np.stack([i.ravel(), j.ravel()], 1))


def boundary(cell=None, x0=BOUNDARY_X0, y0=BOUNDARY_X0):
    """cell None: the lattice alone, whose grid says where the cell boundaries are; else with the centres on them.  The
    boundaries 1 .. n - 2 lie inside the lattice's bounding box, so the added centres move neither the box nor the grid."""
    lat = boundary_lattice()
    if cell is None:
        return Layout("boundary", lat, BOUNDARY_RADIUS)

    def three(v):
        f = np.float32(v)
        return [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]

    k = np.arange(1, BOUNDARY_N - 1)
    row = BOUNDARY_X0 + BOUNDARY_RADIUS * np.float64([0, 5, BOUNDARY_N - 1])        # first, an inner and the last lattice line
    extra = []
    for kk in k:                                                                    # below, on and above in turn
        for j, r in enumerate(row):
            extra.append((three(x0 + kk * cell)[(kk + j) % 3], np.float32(r)))
            if (kk, j) != (5, 1):       # (where the inner lines cross, the centre on the x boundary is there already)
                extra.append((np.float32(r), three(y0 + kk * cell)[(kk + j + 1) % 3]))
    for kk in k[::3]:
        extra.append((three(x0 + kk * cell)[kk % 3], three(y0 + (BOUNDARY_N - 1 - kk) * cell)[(kk + 1) % 3]))
    cen = np.concatenate([lat, np.float32(extra)])
    assert cen[:, 0].max() == lat[:, 0].max() and cen[:, 1].max() == lat[:, 1].max() and cen.min() == lat.min()
    return Layout("boundary", cen, BOUNDARY_RADIUS)


def offset():
    base = clustered()
    cen = base.cen.astype(np.float64) + np.float64(OFFSET)
    assert (np.float32(cen) == cen).all()
    return Layout("offset", np.float32(cen), base.radius)


def documented_cell(radius):
    """the cell size of a grid that did not grow (csrc/lk_cell_grid.hpp: the radius and a hair more) - what the host test, which
    has no grid to ask, builds `boundary` with; the GPU test asserts that the library reports this very number"""
    return float(np.float32(radius)) * (1.0 + 1e-6)


def layout(name, grid=None):
    """grid: what HipCorrelationEngine.cell_grid reported for boundary()'s lattice (`boundary` only; None: the documented cell)"""
    if name == "boundary":
        if grid is None:
            return boundary(documented_cell(BOUNDARY_RADIUS))
        return boundary(grid["cell"], grid["x0"], grid["y0"])
    return {"clustered": clustered, "sparse_line": sparse_line, "dense": dense, "coincident": coincident, "one_point": one_point,
            "offset": offset}[name]()


def sparse_line_window(lay, size=64):
    """`sparse_line` for the field map and the owner map, whose nodes are integers: size x size nodes at stride 1 whose rows
    include y = 128 and whose columns hold as many squares with an integer x as any (a node sees neighbours only on such a
    square's corner: the radius is 1/8 px) -> (x0, y0, size, size)"""
    c = lay.cen.astype(np.float64)
    xs = np.unique(c[(c[:, 1] == 128.0) & (c[:, 0] == np.round(c[:, 0])), 0])
    held = [int(((xs >= x0) & (xs < x0 + size)).sum()) for x0 in range(0, 256 - size + 1)]
    return (int(np.argmax(held)), 128 - size // 2, size, size)


def sparse_line_points(lay):
    """`sparse_line` for the track points, which may lie anywhere: 1/8 px above, below, left and right of every square - one
    radius from a corner or two, and above and below the row within one (grown) cell outside the grid -> float64 [100][2]"""
    c = lay.cen.astype(np.float64)
    low = c[0::4]                                   # the corner (x, 128) of every square
    return np.concatenate([low + [0.0, 0.25], low + [0.0, -0.125], low + [0.25, 0.0], low + [-0.125, 0.0]])


def pitch(lay):
    return lay.radius / 2.5


def records(lay, seed=0, model=ca.FM_UVUXUYVXVY):
    """tests/records_ref.py's synthetic records: bad by error code, by NaN and by chi, 5 % each"""
    rng = np.random.default_rng(1000 + 10 * NAMES.index(lay.name) + seed)
    rec = synthetic_records(len(lay.cen), rng, CHI_MAX, SHARE)
    if lay.name == "boundary":          # the lattice points that a centre on a cell boundary stands in for
        n = BOUNDARY_N ** 2
        c = lay.cen.astype(np.float64)
        twin = (np.abs(c[:n, None, :] - c[None, n:, :]).max(axis=2) < 1e-2).any(axis=1)
        assert twin.sum() == len(c) - n
        rec["error_code"][:n][twin] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
    return rec


def stereo_points(lay, rec, seed=0):
    """3-D points for lk_stereo_strain from the centres alone: the reference state on a tilted plane (one world unit per two
    pixels, about the layout's first centre), one frame stretched and turned a little with a slow wave across it, and the
    sectors of the bad records without a point -> (ref_points [S], points [1][S])"""
    rng = np.random.default_rng(2000 + 10 * NAMES.index(lay.name) + seed)
    c = lay.cen.astype(np.float64) - lay.cen[0].astype(np.float64)
    X, Y = 0.5 * c[:, 0], 0.5 * c[:, 1]
    Pr = np.stack([X, Y, 400.0 + 0.25 * X - 0.15 * Y], 1)
    A = np.eye(3) + rng.uniform(-0.02, 0.02, (3, 3))
    Pf = Pr @ A.T + np.float64([2.0, -1.0, 4.0]) + 0.05 * np.sin(0.11 * X + 0.07 * Y)[:, None] * np.float64([0.3, -0.2, 1.0])
    good = is_good(rec, 6, CHI_MAX)
    ref = np.zeros(len(c), ca.STEREO_POINT_DTYPE)
    pts = np.zeros((1, len(c)), ca.STEREO_POINT_DTYPE)
    for out, P, ok in ((ref, Pr, np.ones(len(c), bool)), (pts[0], Pf, good)):
        out["X"], out["Y"], out["Z"] = np.where(ok, P[:, 0], 0.0), np.where(ok, P[:, 1], 0.0), np.where(ok, P[:, 2], 0.0)
        out["status"] = np.where(ok, ca.STEREO_OK, ca.STEREO_BAD_RECORD)
    return ref, pts


# ---- the tables -------------------------------------------------------------------------------------------------------------
def tables_reference(cen, grid):
    """-> (cell_of [S], start [nx ny + 1], members [S]) for the geometry `grid` reports"""
    c = np.asarray(cen, np.float32).astype(np.float64)
    nx, ny, cell = int(grid["nx"]), int(grid["ny"]), np.float64(grid["cell"])
    ix = np.clip(np.floor((c[:, 0] - np.float64(grid["x0"])) / cell), 0, nx - 1).astype(np.int64)
    iy = np.clip(np.floor((c[:, 1] - np.float64(grid["y0"])) / cell), 0, ny - 1).astype(np.int64)
    cell_of = iy * nx + ix
    count = np.bincount(cell_of, minlength=nx * ny)
    start = np.concatenate([[0], np.cumsum(count)])
    members = np.argsort(cell_of, kind="stable")
    return cell_of.astype(np.uint32), start.astype(np.uint32), members.astype(np.uint32)


def check_tables(cen, grid):
    cell_of, start, members = tables_reference(cen, grid)
    S = len(cen)
    assert grid["nx"] >= 1 and grid["ny"] >= 1 and len(grid["start"]) == grid["nx"] * grid["ny"] + 1
    assert np.array_equal(grid["cell_of"], cell_of), np.flatnonzero(grid["cell_of"] != cell_of)[:8]
    assert np.array_equal(grid["start"], start), np.flatnonzero(grid["start"] != start)[:8]
    assert grid["start"][0] == 0 and grid["start"][-1] == S
    assert np.array_equal(np.sort(grid["members"]), np.arange(S))
    assert np.array_equal(grid["members"], members), np.flatnonzero(grid["members"] != members)[:8]
    # every cell is at least a radius wide and the grid covers the centres' bounding box
    c = np.asarray(cen, np.float32).astype(np.float64)
    assert grid["x0"] == c[:, 0].min() and grid["y0"] == c[:, 1].min()
    assert grid["x0"] + grid["nx"] * grid["cell"] > c[:, 0].max() and grid["y0"] + grid["ny"] * grid["cell"] > c[:, 1].max()


def grew(lay, grid):
    return grid["cell"] > float(np.float32(lay.radius)) * (1.0 + 1e-6) * (1.0 + 1e-9)


# ---- free positions -----------------------------------------------------------------------------------------------------------
BANDS = ("inside", "within one cell", "one to two cells", "beyond two cells")


def band_of(p, lo, hi, cell):
    """how far a coordinate lies outside the grid's extent lo .. hi, in cells: 0 inside, 1, 2, 3 (beyond two)"""
    out = np.maximum(lo - p, p - hi)
    return np.where(out <= 0, 0, np.minimum(np.ceil(out / cell), 3)).astype(int)


def side_windows(cen, grid, size=64, frame=None):
    """Four windows of size x size integer nodes, one over each side of the grid: across the side it reaches from 3.5 cells
    outside inwards, along the side it is centred on the centre nearest to that side.  frame = (w, h): clipped to it.
    -> [(x0, y0, nx, ny)]"""
    c = np.asarray(cen, np.float32).astype(np.float64)
    cell = grid["cell"]
    lo = np.float64([grid["x0"], grid["y0"]])
    hi = lo + np.float64([grid["nx"], grid["ny"]]) * cell
    out = []
    for axis in (0, 1):
        for upper in (0, 1):
            near = c[np.argmax(c[:, axis]) if upper else np.argmin(c[:, axis])]
            o = [0, 0]
            o[axis] = int(np.ceil(hi[axis] + 3.5 * cell)) - size + 1 if upper else int(np.floor(lo[axis] - 3.5 * cell))
            o[1 - axis] = int(round(near[1 - axis])) - size // 2
            w = [o[0], o[1], size, size]
            if frame is not None:
                for a in (0, 1):
                    end = min(w[a] + w[2 + a], frame[a])
                    w[a] = max(w[a], 0)
                    w[2 + a] = end - w[a]
            out.append(tuple(w))
    return out


def free_points(cen, grid, seed=0, per_band=15):
    """track points: 40 on centres; then for every side of the grid and every band - inside, within one cell outside, one to
    two cells, two to 3.5 cells - per_band multiples of 1/8 in that band across the side and within two cells of the centre
    nearest to the side along it -> float32 [Q][2]"""
    rng = np.random.default_rng(3000 + seed)
    c = np.asarray(cen, np.float32)
    pts = [c[rng.permutation(len(c))[:40]].astype(np.float64)]
    cell = grid["cell"]
    lo = np.float64([grid["x0"], grid["y0"]])
    hi = lo + np.float64([grid["nx"], grid["ny"]]) * cell
    c = c.astype(np.float64)
    for axis in (0, 1):
        for upper in (0, 1):
            near = c[np.argmax(c[:, axis]) if upper else np.argmin(c[:, axis])]
            for a, b in ((-2.0, 0.0), (0.0, 1.0), (1.0, 2.0), (2.0, 3.5)):       # cells outside the side (negative: inside)
                out = rng.uniform(a, b, per_band) * cell
                p = np.zeros((per_band, 2))
                p[:, axis] = hi[axis] + out if upper else lo[axis] - out
                p[:, 1 - axis] = near[1 - axis] + rng.uniform(-2.0, 2.0, per_band) * cell
                pts.append(eighths(p))
    return np.float32(np.concatenate(pts))


def bands_of_points(pts, grid):
    """[Q]: the larger of the two coordinates' bands"""
    p = np.asarray(pts, np.float64)
    cell = grid["cell"]
    bx = band_of(p[:, 0], grid["x0"], grid["x0"] + grid["nx"] * cell, cell)
    by = band_of(p[:, 1], grid["y0"], grid["y0"] + grid["ny"] * cell, cell)
    return np.maximum(bx, by)


def nearest_distance(cen, pts):
    c = np.asarray(cen, np.float32).astype(np.float64)
    p = np.asarray(pts, np.float64)
    d2 = ((p[:, None, :] - c[None, :, :]) ** 2).sum(2)
    return np.sqrt(d2.min(1))


def rim_is_exact(cen, radius, positions=None):
    """A condition on the inputs: every (position, centre) pair - positions None: every pair of centres - is either exactly
    at the radius with both differences multiples of 1/8 (dx dx + dy dy is then exact however it is evaluated, and the
    pair counts on both sides) or at least 2^-48 r^2 = 32 ulp from it in d^2 (no rounding of dx dx + dy dy, fused or not, moves it across).  The
    differences themselves are exact in double for any two floats."""
    c = np.asarray(cen, np.float32).astype(np.float64)
    p = c if positions is None else np.asarray(positions, np.float64)
    r2 = float(np.float32(radius)) ** 2
    for b in range(0, len(p), 512):
        d = p[b:b + 512, None, :] - c[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        at = d2 == r2
        if (at & ~(d * 8.0 == np.round(d * 8.0)).all(axis=2)).any():
            return False
        if (~at & (np.abs(d2 - r2) < 2.0 ** -48 * r2)).any():
            return False
    return True
