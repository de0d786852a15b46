"""The candidates of the rectilinear path as the source-record kernel makes them (d_rect_wave_candidates in k_cell_struct2r, and
in k_candidates_rect for a polygon-list source; csrc/xgrid_kernels.hip): a wave scans the counts of its 64 cells, takes its
place in a region with one atomic and writes the pairs slot by slot, every slot finding its owner lane in the scan.  Each case
below is the smallest shape that reaches one branch of that routine, and every one is compared with the generic bins path
(fg_set_search_rect(0): k_cell_struct2 / k_candidates1, which share none of it) the way tests/test_gpu_rect.py compares them:
index lists equal, areas, centroid integrals, per-cell sums and destination areas equal in bits."""
import numpy as np
import pytest

import orc
from test_gpu_rect import assert_same_plan, latlon_window, same_bits, source_grids

pytestmark = pytest.mark.gpu
D2R = np.pi / 180
RECT_HEAVY, RECT_EPS = 48, 1.e-9          # csrc/xgrid_kernels.hip


def dump(fg, order, grids, gout, masks=None, rect=True, cull=False, exact=False, want_src=False):
    """one plan -> everything assert_same_plan looks at (switches back to their defaults on the way out)"""
    L = fg.lib()
    L.fg_set_search_rect(1 if rect else 0); L.fg_set_search_cull(1 if cull else 0); L.fg_set_search_mode(1 if exact else 0)
    try:
        p = fg.XgridPlan.create(order, grids, gout, masks=masks)
        return _take(p, order, gout, want_src)
    finally:
        L.fg_set_search_rect(1); L.fg_set_search_cull(0); L.fg_set_search_mode(0)


def _take(p, order, gout, want_src=False):
    x = p.get_xgrid()                              # (before finalize: c1 / c2 are the centroid integrals)
    a_in, a_out = p.get_cell_area(gout.nx * gout.ny)
    out = dict(x, a_in=a_in, a_out=a_out, n=p.nxgrid, stats=p.stats())
    out["dst"] = p.get_cell_struct(1, gout.nx * gout.ny)
    if want_src:
        out["src"] = p.get_cell_struct(0, p.ncells_in)
    if order == 2:
        import torch
        t = torch.empty(3 * p.ncells_in, dtype=torch.float64, device="cuda:0")
        p.copy_cell_sums(t); out["sums"] = t.cpu().numpy()
    p.destroy()
    return out


def window(win, stretch=False):
    lo, la = latlon_window(*win, stretch=stretch)
    return lo, la


_generic = {}                                      # (case, order) -> the generic path's plan, made once


def both_paths(fg, name, order, grids, win, stretch=False, want_src=False):
    lo, la = window(win, stretch)
    gout = fg.GridConfig(win[4], win[5], lo, la)
    r = dump(fg, order, grids, gout, want_src=want_src)
    if (name, order) not in _generic:
        _generic[(name, order)] = dump(fg, order, grids, gout, rect=False)
    g = _generic[(name, order)]
    assert g["stats"]["bins"] > 0 and r["stats"]["bins"] == 0, "the two searches must really take different paths"
    assert_same_plan(r, g, order, name)
    return r, g, gout


def three_unaligned_tiles(fg):
    """20x10, 33x7 and 5x41 cells side by side: 636 cells = two full blocks and a partial one, a partial last wave, and tile
    offsets (200, 431) that are no multiples of 64"""
    tiles = []
    for win in ((0, 120, -60, 60, 20, 10), (120, 250, -40, 50, 33, 7), (250, 360, -85, 85, 5, 41)):
        lo, la = latlon_window(*win)
        tiles.append(fg.GridConfig(win[4], win[5], lo, la))
    return tiles


FIRST_TWO = [
    ("three unaligned lat-lon tiles -> 72x36", "tiles3", (0, 360, -90, 90, 72, 36)),
    ("C24 -> regional 230..310 x 15..65 (waves and runs of lanes without candidates)", "c24", (230, 310, 15, 65, 40, 25)),
]
WINDOWS = [
    ("C24 -> window -30..40 x -20..30 (two windows, +-2pi shifts)", "c24", (-30, 40, -20, 30, 35, 25)),
    ("C24 -> global -180..180 120x60 (up to three windows)", "c24", (-180, 180, -90, 90, 120, 60)),
]
NEAR_HEAVY = [
    ("C24 -> 144x72 (large per-lane counts beside heavy cells)", "c24", (0, 360, -90, 90, 144, 72)),
    ("C12 -> 180x90 (large per-lane counts beside heavy cells)", "c12", (0, 360, -90, 90, 180, 90)),
]


def sources(fg, kind):
    if kind == "tiles3":
        return three_unaligned_tiles(fg)
    if kind == "c12":
        lon, lat = fg.gnomonic_ed_corners(12)
        return [fg.GridConfig(12, 12, lon[t], lat[t]) for t in range(6)]
    return source_grids(fg, kind)


@pytest.mark.parametrize("case", FIRST_TWO + WINDOWS, ids=[c[0] for c in FIRST_TWO + WINDOWS])
@pytest.mark.parametrize("order", [1, 2])
def test_wave_candidates_equal_the_generic_path(fg, gpu_ok, case, order):
    name, kind, win = case
    both_paths(fg, name, order, sources(fg, kind), win)


@pytest.mark.parametrize("case", NEAR_HEAVY, ids=[c[0] for c in NEAR_HEAVY])
@pytest.mark.parametrize("order", [1, 2])
def test_large_lane_counts_beside_heavy_cells(fg, gpu_ok, case, order):
    name, kind, win = case
    r, g, _ = both_paths(fg, name, order, sources(fg, kind), win, want_src=True)
    assert r["stats"]["heavy"] > 0, name
    # ... and cells just below the estimate, which the lanes of the same waves handle: rows x columns above 30 by the kernel's own reckoning
    s = r["src"]
    nr = (s["lat_max"] - s["lat_min"]) * (win[5] / ((win[3] - win[2]) * D2R)) + 2.0
    nc = (s["lon_max"] - s["lon_min"]) * (win[4] / ((win[1] - win[0]) * D2R)) + 2.0
    est = np.where(s["lon_max"] - s["lon_min"] > np.pi, np.inf, nr * nc)
    assert np.count_nonzero((est > 30) & (est <= RECT_HEAVY)) > 50, name


def _window_columns(lon_ax, lo, hi):
    """columns of the axis whose raw interval, moved by a whole number of turns, meets (lo, hi): d_rect_query's windows"""
    n = np.zeros(lo.shape, dtype=np.int64)
    nx = lon_ax.size - 1
    for t in (2, 1, 0, -1, -2):
        l, h = lo - RECT_EPS - t * 2 * np.pi, hi + RECT_EPS - t * 2 * np.pi
        a = np.maximum(np.searchsorted(lon_ax, l, side="right") - 1, 0)
        b = np.minimum(np.searchsorted(lon_ax, h, side="left") - 1, nx - 1)
        ok = (lon_ax[-1] > l) & (lon_ax[0] < h)
        n += np.where(ok, np.maximum(b - a + 1, 0), 0)
    return n


@pytest.mark.parametrize("order", [1, 2])
def test_lane_with_more_than_64_window_columns(fg, gpu_ok, order):
    """Stretched axes (latlon_window(..., stretch=True)): the columns are (i / n)^1.7, so at the left edge they are far narrower
    than the mean spacing d_rect_heavy goes by.  The window starts at 45 deg, an edge of the cubed sphere's tiles, so that cells
    of ordinary width begin right there: their windows hold 66 columns while the estimate (rows x columns <= 48) leaves them to
    their lanes -- the lanes that must re-test and write their own pairs (nwc > 64).  That such cells exist is checked here from
    the plan's own source records; the 600x40 global window has none (52 columns at most)."""
    win = (45, 190, -88, 88, 600, 40)
    r, g, gout = both_paths(fg, "C24 -> stretched 600x40 from 45 deg", order, source_grids(fg, "c24"), win, stretch=True, want_src=True)
    lo, la = window(win, True)
    s = r["src"]
    lon_ax, lat_ax = lo[0], la[:, 0]
    live = s["nvert"] > 0
    nr = (s["lat_max"] - s["lat_min"]) * (win[5] / (lat_ax[-1] - lat_ax[0])) + 2.0
    nc = (s["lon_max"] - s["lon_min"]) * (win[4] / (lon_ax[-1] - lon_ax[0])) + 2.0
    heavy = np.where(s["lon_max"] - s["lon_min"] > np.pi, True, nr * nc > RECT_HEAVY)
    rows = (np.searchsorted(lat_ax, s["lat_max"], side="left") - 1) - np.maximum(np.searchsorted(lat_ax, s["lat_min"], side="right") - 1, 0) + 1
    wide = live & ~heavy & (rows > 0) & (_window_columns(lon_ax, s["lon_min"], s["lon_max"]) > 64)
    assert np.count_nonzero(wide) >= 2, np.count_nonzero(wide)
    assert r["stats"]["heavy"] > 0
    # the global stretched window of tests/test_gpu_rect.py at this shape, for the axis search under large per-lane counts
    both_paths(fg, "C24 -> stretched 600x40 global", order, source_grids(fg, "c24"), (0, 360, -88, 88, 600, 40), stretch=True)


def test_inactive_cells_and_blocks_that_leave_early(fg, gpu_ok):
    """seeded masks (one tile without), culling on, three bands of 90x45: masked lanes inside live waves, and source blocks that
    leave before their records and must still leave pair counts of zero behind"""
    grids = source_grids(fg, "c24")
    rng = np.random.default_rng(11)
    masks = [(rng.random((24, 24)) > 0.3).astype(np.float64) for _ in range(6)]
    masks[4] = None
    lo, la = latlon_window(0, 360, -90, 90, 90, 45)
    for j0, j1 in ((0, 10), (10, 31), (31, 45)):
        gout = fg.GridConfig(90, j1 - j0, np.ascontiguousarray(lo[j0:j1 + 1]), np.ascontiguousarray(la[j0:j1 + 1]))
        for order in (1, 2):
            r = dump(fg, order, grids, gout, masks=masks, cull=True)
            g = dump(fg, order, grids, gout, masks=masks, rect=False)
            assert r["stats"]["bins"] == 0 and g["stats"]["bins"] > 0
            assert r["n"] == g["n"] > 0
            for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
                assert np.array_equal(r[k], g[k]), (j0, order, k)
            for k in ["area", "a_out"] + (["c1", "c2", "sums"] if order == 2 else []):
                assert same_bits(r[k], g[k]), (j0, order, k)


@pytest.mark.parametrize("case", FIRST_TWO, ids=[c[0] for c in FIRST_TWO])
@pytest.mark.parametrize("order", [1, 2])
def test_region_clamps_and_the_repeated_search(fg, gpu_ok, case, order):
    """fg_set_search_mode(1) starts from empty buffers: the first attempt's regions hold nothing, every wave's slots fall
    beyond them (n_ok < cnt), and the search is repeated with the counted sizes -- same plan as mode 0 and as the generic path"""
    name, kind, win = case
    grids = sources(fg, kind)
    r0, g, gout = both_paths(fg, name, order, grids, win)
    r1 = dump(fg, order, grids, gout, exact=True)
    assert r1["stats"]["bins"] == 0 and r1["stats"]["exact_mode"] == 1          # (more than one attempt)
    assert_same_plan(r1, r0, order, name + " (exact)")
    assert_same_plan(r1, g, order, name + " (exact, generic)")


def _polygon_list(fg):
    """~500 quads and pentagons: clipped polygons of C8 x 30x16 (how coupler_xgrid gets its list, tests/test_gpu_coupler.py), a seeded draw"""
    lon, lat = fg.gnomonic_ed_corners(8)
    atm = [fg.GridConfig(8, 8, lon[t], lat[t]) for t in range(6)]
    lo, la = fg.latlon_corners(30, 16)
    p = fg.XgridPlan.create(1, atm, fg.GridConfig(30, 16, lo, la))
    x = p.get_xgrid(); poly = p.get_polygons(maxv=8)
    src = p.get_cell_struct(0, 6 * 64)
    p.destroy()
    cell = x["t_in"].astype(np.int64) * 64 + x["j_in"] * 8 + x["i_in"]
    pick = np.flatnonzero((poly["n"] == 4) | (poly["n"] == 5))
    pick = np.sort(np.random.default_rng(3).choice(pick, size=min(500, pick.size), replace=False))
    assert pick.size >= 400 and np.count_nonzero(poly["n"][pick] == 5) > 10
    return poly["n"][pick], poly["lon"][pick], poly["lat"][pick], src["lon_avg"][cell[pick]], x["area"][pick]


@pytest.mark.parametrize("order", [1, 2])
def test_polygon_list_source_uses_the_stand_alone_kernel(fg, gpu_ok, order):
    n, plon, plat, lon_avg, area = _polygon_list(fg)
    lo, la = latlon_window(0, 360, -90, 90, 72, 36)
    gout = fg.GridConfig(72, 36, lo, la)
    L = fg.lib()
    out = {}
    for rect in (1, 0):
        L.fg_set_search_rect(rect)
        try:
            p = fg.XgridPlan.create_polylist(order, n, plon, plat, lon_avg, area, gout)
            out[rect] = _take(p, order, gout)
        finally:
            L.fg_set_search_rect(1)
    r, g = out[1], out[0]
    assert g["stats"]["bins"] > 0 and r["stats"]["bins"] == 0
    assert_same_plan(r, g, order, "polygon list -> 72x36")


@pytest.mark.parametrize("tile", [0, 2])
def test_c24_against_the_cpu_oracle(fg, gpu_ok, tile):
    """C24 -> 72x36, order 2, against the CPU oracle (as tests/test_gpu_xgrid.py::test_create_xgrid_c48)"""
    lon, lat = fg.gnomonic_ed_corners(24)
    lo, la = fg.latlon_corners(72, 36)
    r = fg.create_xgrid_2dx2d_order2(24, 24, 72, 36, lon[tile], lat[tile], lo, la)
    o = orc.orc_create_xgrid(2, 24, 24, 72, 36, lon[tile], lat[tile], lo, la)
    assert r[0] == o["n"] > 0
    for a, k in zip(r[1:5], ("i_in", "j_in", "i_out", "j_out")):
        assert np.array_equal(a, o[k]), k
    scale = np.maximum(np.abs(o["area"]), 1e-10 * np.max(np.abs(o["area"])) + 1e-300)
    assert np.max(np.abs(r[5] - o["area"]) / scale) < 1e-10
    for a, k in ((r[6], "clon"), (r[7], "clat")):
        assert np.max(np.abs(a - o[k])) <= 1e-10 * np.max(np.abs(o[k])), k
    if orc.host_has_fma():
        bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
        assert np.array_equal(bits(r[5]), bits(o["area"]))
        assert np.array_equal(bits(r[6]), bits(o["clon"])) and np.array_equal(bits(r[7]), bits(o["clat"]))
