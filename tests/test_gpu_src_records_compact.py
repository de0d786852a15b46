"""Compact source records on the rectilinear path (csrc/xgrid_device.h: FgCells with vstride = FG_VSTRIDE_QUAD).

A grid source on the rectilinear path keeps 64 bytes per cell -- lon[4] then lat[4] -- and no lon_min / lon_max; a cell that
fix_lon leaves with more than four vertices has its sixteen doubles in a side table, its slot in the first word of its own
record.  fg_plan_get_cell_struct(0, ...) spells the records out.  Nothing a caller can see may change, so every case compares,
bit for bit, the rectilinear path with the generic one (fg_set_search_rect(0), 128-byte records): the exchange grid, the per-cell
sums, get_cell_struct(0) (all fields, vlon / vlat eight wide with zeros beyond nv) and get_cell_area.  Under culling only nv and
area of the cells the search left out are compared (it writes nothing else of them).  Without culling and mask the indices
equal the CPU oracle's and areas / centroid integrals hold to the bars of tests/test_gpu_xgrid.py (RTOL = 1e-10).

The plans are made in ONE child process that sets FREGRID_HIP_POISON=1 before the library loads (csrc/plan.hip: every block the
pool hands out is filled with 0x7f bytes first), so that a read of something no longer written -- the second half of a record,
a box's longitudes, a slot number -- shows up as a wild value instead of a lucky zero.  (The variable is read once per process:
in the test process itself it would come too late.)

Sources and targets: C2 and C6 (a pole is a corner of eight cells: lone pole vertices, wide slots) over 36x18 (their candidates by
the lane form), C6 over 360x180 (the same cells as heavy ones); C7 (no cell listed) over 360x180; the hand-made 2x2 tile with
half-turn edges of tests/test_gpu_record_rare_cells.py over rows 150..180 of 360x180; a 24x12 lat-lon grid (its pole rows are
listed and end with four vertices: the compact record) over rows 60..120, culling off and on.  One case masks a pole cell, one
an ordinary cell (its sums must be zero).  Then: the side table with no slot (the plan must come from the generic path and be
equal), a polygon-list plan (128-byte records on the rectilinear path), fg_plan_get_polygons."""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-10
HERE = os.path.dirname(os.path.abspath(__file__))

# target: (nlon, nlat, first row, last row + 1)
TARGETS = {"36x18": (36, 18, 0, 18), "360x180": (360, 180, 0, 180), "rows 150..180 of 360x180": (360, 180, 150, 180),
           "rows 60..120 of 360x180": (360, 180, 60, 120)}
# (source, target, culling, mask: None / "pole" / "ordinary")
CASES = [("C2", "36x18", False, None), ("C6", "36x18", False, None), ("C6", "36x18", False, "pole"), ("C6", "360x180", False, None),
         ("C7", "360x180", False, None), ("C7", "360x180", False, "ordinary"),
         ("2x2 with half-turn edges", "rows 150..180 of 360x180", False, None),
         ("24x12 lat-lon", "rows 60..120 of 360x180", False, None), ("24x12 lat-lon", "rows 60..120 of 360x180", True, None)]
IDS = ["%s -> %s%s%s" % (s, t, ", culling" if c else "", ", %s cell masked" % m if m else "") for s, t, c, m in CASES]
ORDINARY = (0, 3, 2)                           # (tile, j, i) of the ordinary cell that is masked out


def _tiles(fg, src):
    if src[0] == "C":
        ni = int(src[1:])
        lon, lat = fg.gnomonic_ed_corners(ni)
        return [(ni, ni, np.ascontiguousarray(lon[t]), np.ascontiguousarray(lat[t])) for t in range(6)]
    if src.startswith("2x2"):
        lon = np.array([0.0, np.pi, 1.2 * np.pi]); lat = np.deg2rad(np.array([60.0, 70.0, 80.0]))
        return [(2, 2, np.ascontiguousarray(np.broadcast_to(lon[None, :], (3, 3))), np.ascontiguousarray(np.broadcast_to(lat[:, None], (3, 3))))]
    lo, la = fg.latlon_corners(24, 12, 0., 360., -90., 90.)
    return [(24, 12, np.ascontiguousarray(lo), np.ascontiguousarray(la))]


def _target(fg, tgt):
    nlon, nlat_all, j0, j1 = TARGETS[tgt]
    lo, la = fg.latlon_corners(nlon, nlat_all, 0., 360., -90., 90.)
    return nlon, j1 - j0, np.ascontiguousarray(lo[j0:j1 + 1]), np.ascontiguousarray(la[j0:j1 + 1])


def _masks(tiles, mask):
    if mask is None:
        return None
    masks = [np.ones((ny, nx)) for nx, ny, _, _ in tiles]
    if mask == "pole":                                       # a cell of tile 3 with the north pole for a corner
        lat = tiles[2][3]
        y = np.stack([lat[:-1, :-1], lat[:-1, 1:], lat[1:, 1:], lat[1:, :-1]])
        j, i = np.argwhere(np.any(np.abs(y) >= np.pi / 2 - 1.e-6, axis=0))[0]
        masks[2][j, i] = 0.0
    else:
        masks[ORDINARY[0]][ORDINARY[1], ORDINARY[2]] = 0.0
    return masks


# ---------------------------------------------------------------------------------------------------------------------------
# the child process: every plan of this file, under FREGRID_HIP_POISON=1
def _dump(fg, p, order, nsrc, ndst, polygons=False):
    import torch
    out = dict(p.get_xgrid(), n=p.nxgrid, stats=p.stats(), src=p.get_cell_struct(0, nsrc), a_in=p.get_cell_area(ndst)[0])
    if order == 2:
        t = torch.empty(3 * p.ncells_in, dtype=torch.float64, device="cuda:0")
        p.copy_cell_sums(t); out["sums"] = t.cpu().numpy()
    if polygons:
        out["poly"] = p.get_polygons(maxv=8)
    p.destroy()
    return out


def _grid_plan(fg, order, tiles, tgt, cull, masks, rect, wide_cap=-1, polygons=False):
    L = fg.lib()
    nlon, nlat, lo, la = tgt
    L.fg_set_search_rect(1 if rect else 0); L.fg_set_search_cull(1 if cull else 0); L.fg_set_search_wide_cap(wide_cap)
    try:
        p = fg.XgridPlan.create(order, [fg.GridConfig(nx, ny, lon, lat) for nx, ny, lon, lat in tiles], fg.GridConfig(nlon, nlat, lo, la), masks=masks)
    finally:
        L.fg_set_search_rect(1); L.fg_set_search_cull(0); L.fg_set_search_wide_cap(-1)
    return _dump(fg, p, order, sum(nx * ny for nx, ny, _, _ in tiles), nlon * nlat, polygons)


def _polygon_list(fg):
    """~300 quads and pentagons: clipped polygons of C8 x 30x16, a seeded draw (as tests/test_gpu_rect_candidates.py)"""
    lon, lat = fg.gnomonic_ed_corners(8)
    lo, la = fg.latlon_corners(30, 16)
    p = fg.XgridPlan.create(1, [fg.GridConfig(8, 8, lon[t], lat[t]) for t in range(6)], fg.GridConfig(30, 16, lo, la))
    x = p.get_xgrid(); poly = p.get_polygons(maxv=8); src = p.get_cell_struct(0, 6 * 64)
    p.destroy()
    cell = x["t_in"].astype(np.int64) * 64 + x["j_in"] * 8 + x["i_in"]
    pick = np.flatnonzero((poly["n"] == 4) | (poly["n"] == 5))
    pick = np.sort(np.random.default_rng(3).choice(pick, size=min(300, pick.size), replace=False))
    return poly["n"][pick], poly["lon"][pick], poly["lat"][pick], src["lon_avg"][cell[pick]], x["area"][pick]


def _child(path):
    sys.path.insert(0, HERE)
    import conftest
    fg = conftest.load_package()
    assert fg.lib().fg_device_count() >= 1
    out = {}
    for case in CASES:
        src, tgt, cull, mask = case
        tiles = _tiles(fg, src)
        for order in (1, 2):
            for rect in (True, False):
                out[(case, order, rect)] = _grid_plan(fg, order, tiles, _target(fg, tgt), cull, _masks(tiles, mask), rect)
    tiles = _tiles(fg, "C6")
    for order in (1, 2):
        out[("no slot", order)] = _grid_plan(fg, order, tiles, _target(fg, "360x180"), False, None, True, wide_cap=0)
    for rect in (True, False):
        out[("polygons", rect)] = _grid_plan(fg, 2, tiles, _target(fg, "36x18"), False, None, rect, polygons=True)
    n, plon, plat, lon_avg, area = _polygon_list(fg)
    nlon, nlat, lo, la = _target(fg, "36x18")
    for order in (1, 2):
        for rect in (True, False):
            fg.lib().fg_set_search_rect(1 if rect else 0)
            try:
                p = fg.XgridPlan.create_polylist(order, n, plon, plat, lon_avg, area, fg.GridConfig(nlon, nlat, lo, la))
            finally:
                fg.lib().fg_set_search_rect(1)
            out[("polylist", order, rect)] = _dump(fg, p, order, n.size, nlon * nlat)
    with open(path, "wb") as f:
        pickle.dump(out, f)


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans(gpu_ok):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "plans.pkl")
        env = dict(os.environ, FREGRID_HIP_POISON="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with open(path, "rb") as f:
            return pickle.load(f)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same_plan(r, g, order, cull, what):
    assert r["n"] == g["n"] > 0, what
    for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(r[k], g[k]), (what, k)
    for k in ["area"] + (["c1", "c2", "sums"] if order == 2 else []):
        assert same_bits(r[k], g[k]), (what, k)
    a, b = r["src"], g["src"]
    assert same_bits(a["nvert"], b["nvert"]) and same_bits(r["a_in"], g["a_in"]), what
    live = a["nvert"] > 0 if cull else np.ones(a["nvert"].shape, dtype=bool)
    for k in ("lat_min", "lat_max", "lon_min", "lon_max", "lon_avg", "vlon", "vlat"):
        assert same_bits(a[k][live], b[k][live]), (what, "source record", k)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_compact_records_give_the_generic_paths_plan(fg, plans, case, order):
    import orc
    src, tgt, cull, mask = case
    r, g = plans[(case, order, True)], plans[(case, order, False)]
    assert r["stats"]["bins"] == 0 and g["stats"]["bins"] > 0
    assert_same_plan(r, g, order, cull, IDS[CASES.index(case)])
    nv, vlon, vlat = r["src"]["nvert"], r["src"]["vlon"], r["src"]["vlat"]
    assert np.all((nv == 0) | ((nv >= 3) & (nv <= 8)))
    beyond = np.arange(8)[None, :] >= nv[:, None]
    if not cull:                                             # zeros beyond nv (a left-out cell of a culling search has nv = 0 and nothing else)
        assert np.all(vlon[beyond] == 0.0) and np.all(vlat[beyond] == 0.0)
    # the cells this file is about are there
    if src in ("C2", "C6"):
        assert r["stats"]["rare"] == 8 and np.count_nonzero(nv > 4) == 8
    elif src == "C7":
        assert r["stats"]["rare"] == 0 and np.all(nv == 4)
    elif src.startswith("2x2"):
        assert r["stats"]["rare"] == 2 and np.count_nonzero(nv > 4) == 2
    elif not cull:
        assert r["stats"]["rare"] == 48 and np.all(nv <= 4)  # the two pole rows of the 24x12 grid
    if mask == "ordinary" and order == 2:
        t, j, i = ORDINARY
        s = t * 49 + j * 7 + i
        assert nv[s] == 4 and r["a_in"][s] > 0
        assert np.all(r["sums"].reshape(3, -1)[:, s] == 0.0)
        assert not np.any((r["t_in"] == t) & (r["j_in"] == j) & (r["i_in"] == i))
    if cull or mask is not None:
        return
    tiles = _tiles(fg, src)
    nlon, nlat, lo, la = _target(fg, tgt)
    parts = [orc.orc_create_xgrid(order, nx, ny, nlon, nlat, lon, lat, lo, la, None, capacity=64 * (nx * ny + nlon * nlat) + 1024)
             for nx, ny, lon, lat in tiles]
    o = {k: np.concatenate([p[k] for p in parts]) for k in ("i_in", "j_in", "i_out", "j_out", "area") + (("clon", "clat") if order == 2 else ())}
    t_in = np.concatenate([np.full(p["n"], k, dtype=np.int32) for k, p in enumerate(parts)])
    assert r["n"] == t_in.size and np.array_equal(r["t_in"], t_in)
    for k in ("i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(r[k], o[k]), k
    assert np.max(np.abs(r["area"] - o["area"]) / o["area"]) < RTOL
    if order == 2:
        for a, k in ((r["c1"], "clon"), (r["c2"], "clat")):
            assert np.max(np.abs(a - o[k])) <= RTOL * np.max(np.abs(o[k])), k


@pytest.mark.parametrize("order", [1, 2])
def test_a_side_table_without_slots_sends_the_search_to_the_generic_path(plans, order):
    case = ("C6", "360x180", False, None)
    z, r, g = plans[("no slot", order)], plans[(case, order, True)], plans[(case, order, False)]
    assert z["stats"]["bins"] > 0 and z["stats"]["rare"] == 0       # what the generic path reports
    assert_same_plan(z, r, order, False, "no slot against the rectilinear path")
    assert_same_plan(z, g, order, False, "no slot against the generic path")


@pytest.mark.parametrize("order", [1, 2])
def test_a_polygon_list_plan_keeps_its_records(plans, order):
    r, g = plans[("polylist", order, True)], plans[("polylist", order, False)]
    assert r["stats"]["bins"] == 0 and g["stats"]["bins"] > 0
    assert_same_plan(r, g, order, False, "polygon list -> 36x18")
    assert np.any(r["src"]["nvert"] == 5)


def test_polygons_of_the_exchange_cells(plans):
    r, g = plans[("polygons", True)], plans[("polygons", False)]
    assert r["stats"]["bins"] == 0 and g["stats"]["bins"] > 0 and r["n"] == g["n"] > 0
    for k in ("n", "lon", "lat"):
        assert same_bits(r["poly"][k], g["poly"][k]), k
    assert np.any(r["poly"]["n"] > 4)
