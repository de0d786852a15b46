"""The source cells that need the general fix_lon on the rectilinear path (csrc/xgrid_kernels.hip): a cell with a vertex at a
pole or an edge of |dlon| = pi.  k_cell_struct2r (d_cell_record<true>) gives such a cell its latitude box and its corners as read, and lists it;
a wave of k_candidates_rect<true> finishes its record (d_finish_rare_cell) and makes its candidates -- as a heavy cell's where
d_rect_heavy says so, by the lane form with one live lane otherwise.

Sources: the cubed spheres C2 and C6 (even: a pole is a corner of four cells on tile 3 and of four on tile 6) and C7 (odd: the
poles lie inside a cell, no cell is listed).  Targets: 36x18 (a pole cell meets 11 columns x under 4 rows < 48: not heavy),
360x180 (heavy), rows 150..180 of 360x180 (the north pole) and rows 60..120 (no pole), the two bands with culling off and on;
one case masks a pole cell out; one source is a hand-made 2x2 tile whose western cells have edges of |dlon| = pi.

Every case, at orders 1 and 2:
  * the number of listed cells (stats()["rare"]) is what the grid implies: counted here in numpy from the corner arrays with
    the two tests of the reference's fix_lon (create_xgrid.c: |lat| >= pi/2 - 1e-6; ||dlon| - pi| < 1e-10), under culling only
    the cells whose latitude range meets the band (the reference's strict test);
  * the exchange grid, the per-cell sums and the source records (get_cell_struct(0, ...), get_cell_area) equal, bit for bit,
    those of the generic path (fg_set_search_rect(0), which keeps the general routine inline) and of the exactly sized search
    (fg_set_search_mode(1)).  A culling search writes of a source cell outside its band nv = 0 and area 0 and nothing else, so
    there only those two are compared;
  * without culling and mask: the indices equal the CPU oracle's (orc.orc_create_xgrid, tile by tile), areas within
    RTOL = 1e-10 of the value and centroid integrals within RTOL of their largest (the bars of tests/test_gpu_xgrid.py, which
    tests/test_gpu_rect.py refers to for oracle parity)."""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
RTOL = 1e-10
POLETOL, SMALL = 1.e-6, 1.e-10                 # csrc/geom.hip.h


def _cube(fg, ni):
    lon, lat = fg.gnomonic_ed_corners(ni)
    return [(ni, ni, np.ascontiguousarray(lon[t]), np.ascontiguousarray(lat[t])) for t in range(6)]


def _hand(fg):
    """one tile of 2 x 2 cells between 60 and 80 degrees north; the western cells span 0 .. pi: their south and north edges are half turns"""
    lon = np.array([0.0, np.pi, 1.2 * np.pi]); lat = np.deg2rad(np.array([60.0, 70.0, 80.0]))
    return [(2, 2, np.ascontiguousarray(np.broadcast_to(lon[None, :], (3, 3))), np.ascontiguousarray(np.broadcast_to(lat[:, None], (3, 3))))]


SOURCES = {"C2": lambda fg: _cube(fg, 2), "C6": lambda fg: _cube(fg, 6), "C7": lambda fg: _cube(fg, 7), "2x2 with half-turn edges": _hand}
# target: (nlon, nlat, first row, last row + 1)
TARGETS = {"36x18": (36, 18, 0, 18), "360x180": (360, 180, 0, 180), "rows 150..180 of 360x180": (360, 180, 150, 180),
           "rows 60..120 of 360x180": (360, 180, 60, 120)}
CASES = []
for _s in ("C2", "C6", "C7"):
    for _t in TARGETS:
        for _cull in ((False, True) if _t.startswith("rows") else (False,)):
            CASES.append((_s, _t, _cull, False))
CASES.append(("C6", "360x180", False, True))                 # a pole cell masked out
CASES.append(("C6", "36x18", False, True))
CASES.append(("2x2 with half-turn edges", "36x18", False, False))
CASES.append(("2x2 with half-turn edges", "360x180", False, False))
IDS = ["%s -> %s%s%s" % (s, t, ", culling" if c else "", ", a pole cell masked" if m else "") for s, t, c, m in CASES]
_made = {}


def rare_cells(tiles, band):
    """per tile: the cells (j, i) the reference's fix_lon does more than unwrap for; band = (lat0, lat1) of a culling search or None"""
    out = []
    for nx, ny, lon, lat in tiles:
        x = np.stack([lon[:-1, :-1], lon[:-1, 1:], lon[1:, 1:], lon[1:, :-1]])        # SW, SE, NE, NW (d_cell_record's order)
        y = np.stack([lat[:-1, :-1], lat[:-1, 1:], lat[1:, 1:], lat[1:, :-1]])
        pole = np.any(np.abs(y) >= np.pi / 2 - POLETOL, axis=0)
        dx = x - np.roll(x, 1, axis=0)
        half = np.any((np.abs(dx + np.pi) < SMALL) | (np.abs(dx - np.pi) < SMALL), axis=0)
        rare = pole | half
        if band is not None:
            rare &= ~((y.max(axis=0) <= band[0]) | (y.min(axis=0) >= band[1]))
        out.append(rare)
    return out


def setup(fg, case):
    if case in _made:
        return _made[case]
    src, tgt, cull, masked = case
    tiles = SOURCES[src](fg)
    nlon, nlat_all, j0, j1 = TARGETS[tgt]
    lo, la = fg.latlon_corners(nlon, nlat_all, 0., 360., -90., 90.)
    lo, la, nlat = np.ascontiguousarray(lo[j0:j1 + 1]), np.ascontiguousarray(la[j0:j1 + 1]), j1 - j0
    rare = rare_cells(tiles, (la[0, 0], la[-1, 0]) if cull else None)
    masks = None
    if masked:
        masks = [np.ones((ny, nx)) for nx, ny, _, _ in tiles]
        j, i = np.argwhere(rare_cells(tiles, None)[2])[0]    # a cell of tile 3 with the north pole for a corner
        masks[2][j, i] = 0.0
    c = dict(tiles=tiles, nlon=nlon, nlat=nlat, lo=lo, la=la, cull=cull, masks=masks, nrare=int(sum(r.sum() for r in rare)),
             nsrc=sum(nx * ny for nx, ny, _, _ in tiles), grids=[fg.GridConfig(nx, ny, lon, lat) for nx, ny, lon, lat in tiles],
             gout=fg.GridConfig(nlon, nlat, lo, la))
    _made[case] = c
    return c


def plan_dump(fg, c, order, rect=True, exact=False):
    import torch
    L = fg.lib()
    L.fg_set_search_rect(1 if rect else 0); L.fg_set_search_cull(1 if c["cull"] else 0); L.fg_set_search_mode(1 if exact else 0)
    try:
        p = fg.XgridPlan.create(order, c["grids"], c["gout"], masks=c["masks"])
    except fg.FregridHipError as e:
        return dict(error=e.code)
    finally:
        L.fg_set_search_rect(1); L.fg_set_search_cull(0); L.fg_set_search_mode(0)
    out = dict(p.get_xgrid(), n=p.nxgrid, stats=p.stats(), src=p.get_cell_struct(0, c["nsrc"]), a_in=p.get_cell_area(c["nlon"] * c["nlat"])[0])
    if order == 2:
        t = torch.empty(3 * p.ncells_in, dtype=torch.float64, device="cuda:0")
        p.copy_cell_sums(t); out["sums"] = t.cpu().numpy()
    p.destroy()
    return out


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
def test_listed_cells_get_the_generic_paths_records_and_exchange_cells(fg, gpu_ok, case, order):
    c = setup(fg, case)
    r = plan_dump(fg, c, order)
    g = plan_dump(fg, c, order, rect=False)
    e = plan_dump(fg, c, order, exact=True)
    if "error" in g:                                         # a source the search refuses: the same refusal from every path
        assert r == g == e, (r, g, e)
        return
    assert r["stats"]["bins"] == 0 and g["stats"]["bins"] > 0 and e["stats"]["bins"] == 0 and e["stats"]["exact_mode"] == 1
    assert r["stats"]["rare"] == e["stats"]["rare"] == c["nrare"] and g["stats"]["rare"] == 0, (r["stats"], c["nrare"])
    if case[0] == "C7":
        assert c["nrare"] == 0
    elif not c["cull"]:
        assert c["nrare"] == (2 if case[0].startswith("2x2") else 8)
    elif case[1].startswith("rows 150"):
        assert c["nrare"] == 4
    else:
        assert c["nrare"] == 0
    assert_same_plan(r, g, order, c["cull"], "generic path")
    assert_same_plan(r, e, order, c["cull"], "exactly sized search")
    nv = r["src"]["nvert"]
    assert np.all((nv == 0) | ((nv >= 3) & (nv <= 8)))
    if c["cull"] or c["masks"] is not None:
        return
    parts = [orc.orc_create_xgrid(order, nx, ny, c["nlon"], c["nlat"], lon, lat, c["lo"], c["la"], None,
                                  capacity=64 * (nx * ny + c["nlon"] * c["nlat"]) + 1024) for nx, ny, lon, lat in c["tiles"]]
    o = {k: np.concatenate([p[k] for p in parts]) for k in ("i_in", "j_in", "i_out", "j_out", "area") + (("clon", "clat") if order == 2 else ())}
    t_in = np.concatenate([np.full(p["n"], k, dtype=np.int32) for k, p in enumerate(parts)])
    assert r["n"] == t_in.size and np.array_equal(r["t_in"], t_in)
    for k in ("i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(r[k], o[k]), k
    assert np.max(np.abs(r["area"] - o["area"]) / o["area"]) < RTOL
    if order == 2:
        for a, k in ((r["c1"], "clon"), (r["c2"], "clat")):
            assert np.max(np.abs(a - o[k])) <= RTOL * np.max(np.abs(o[k])), k


def test_a_masked_pole_cell_has_its_record_and_no_exchange_cells(fg, gpu_ok):
    c = setup(fg, ("C6", "360x180", False, True))
    r = plan_dump(fg, c, 2)
    j, i = np.argwhere(c["masks"][2] == 0)[0]
    s = 2 * 36 + j * 6 + i
    assert r["src"]["nvert"][s] >= 3 and r["a_in"][s] > 0
    assert not np.any((r["t_in"] == 2) & (r["j_in"] == j) & (r["i_in"] == i))
    assert r["stats"]["rare"] == 8
