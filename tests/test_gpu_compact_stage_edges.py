"""The big-cell role of k_compact (csrc/xgrid_kernels.hip: d_compact_big) at the edges of its sizes: a source cell with more
than CP_SMALL = 128 pairs gets a block of its own, which ranks the cell's exchange cells -- by a bitmap over the span of their
destination indices where that is at most 65536, by comparison otherwise -- and, at order 2, adds their area and centroid
integrals up in exchange-cell order, a stage of ranks at a time through LDS.  The block's LDS is divided per cell
(d_big_stage): the bitmap, half as much for its prefix, the rest in three parts for the staged values, so that eight blocks
share a CU.  A cell of at most one stage takes the loads of a pair ahead of its rank, a cell of several stages passes over its
pairs once per stage.  The plans below have source cells on both sides of 128 exchange cells, of one stage (as this file
computes it from the constants of the kernel and the oracle's list) and of 512, the fixed stage the kernel had before, cells of
more than three stages, and cells whose span does not fit the bitmap; the classes are counted on the CPU oracle's list and
asserted, so that a change of the grids cannot empty one.

References, none of them the code under test:
  * the CPU oracle (orc.orc_create_xgrid, tile by tile): the per-cell counts and spans, and the indices of the exchange cells;
  * the exactly sized search (fg_set_search_mode(1): its first attempt has capacity 0, so every clamp of the role runs):
    every exchange array equal in bits;
  * numpy: copy_cell_sums against the left-to-right float64 sums (np.cumsum) of area, clon and clat over each source cell's
    exchange cells in exchange-cell order, equal in bits.

C24 is taken with an equatorial and a polar tile only (the other four repeat their counts and would triple the oracle's time),
and the polar tile of C6 over 720x360 instead of 1440x720: a pole cell of 28 000 exchange cells over 20 rows of 1440 columns is
ranked by comparison, a quarter of a minute on the GPU; the equatorial tile of C6 has such spans with 4 000 exchange cells a cell."""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
CP_SMALL, RANK_WORDS, CP_LDS_DOUBLES, OLD_STAGE = 128, 1024, 2552, 512          # csrc/xgrid_kernels.hip


def stage_of(span):
    """d_big_stage: ranks per stage of a cell whose exchange cells span `span` destination indices"""
    nw = np.where(span <= RANK_WORDS * 64, (span + 63) // 64, 0)
    w8 = (nw + 7) & ~7
    return ((CP_LDS_DOUBLES - w8 - w8 // 2) // 3) & ~7


# the classes of source cells a case must hold, from the exchange cells per cell (na) and the stage of the cell
CLASS = {
    "lane role": lambda na, st, bm: na <= CP_SMALL,
    "one stage": lambda na, st, bm: (na > CP_SMALL) & (na <= st),
    "one stage, two of the old": lambda na, st, bm: (na > OLD_STAGE) & (na <= st),
    "under 512": lambda na, st, bm: (na > CP_SMALL) & (na <= OLD_STAGE),
    "two or three stages": lambda na, st, bm: (na > st) & (na <= 3 * st),
    "more than three stages": lambda na, st, bm: na > 3 * st,
    "ranked by comparison": lambda na, st, bm: (na > CP_SMALL) & ~bm,
    "full-size bitmap": lambda na, st, bm: (na > CP_SMALL) & bm & (st < 512),
}
# source C<ni>, its tiles, target (nlon, nlat), and at least so many cells of a class
CASES = {
    "C24 tiles 1 and 3 -> 720x360": dict(ni=24, tiles=(0, 2), tgt=(720, 360),
                                         has={"lane role": 500, "one stage": 100, "under 512": 100, "one stage, two of the old": 1, "two or three stages": 2}),
    "C12 -> 720x360": dict(ni=12, tiles=range(6), tgt=(720, 360),
                           has={"one stage": 400, "under 512": 400, "one stage, two of the old": 8, "two or three stages": 8, "more than three stages": 4}),
    "C3 -> 360x180": dict(ni=3, tiles=range(6), tgt=(360, 180), has={"two or three stages": 20}),
    "tile 3 of C6 -> 720x360": dict(ni=6, tiles=(2,), tgt=(720, 360), has={"two or three stages": 8, "more than three stages": 4}),
    "tile 1 of C6 -> 1440x720": dict(ni=6, tiles=(0,), tgt=(1440, 720), has={"ranked by comparison": 36, "more than three stages": 30}),
    "tile 1 of C2 -> 1440x180": dict(ni=2, tiles=(0,), tgt=(1440, 180), has={"full-size bitmap": 1, "more than three stages": 1}),
}
NAMES = list(CASES)
_cases, _runs = {}, {}


def case(fg, name):
    """grids and the oracle's exchange-cell list of a case, made once; asserts the case's classes"""
    if name in _cases:
        return _cases[name]
    spec = CASES[name]
    ni, tiles = spec["ni"], list(spec["tiles"])
    nlon, nlat = spec["tgt"]
    lon, lat = fg.gnomonic_ed_corners(ni)
    lo, la = fg.latlon_corners(nlon, nlat, 0., 360., -90., 90.)
    parts = [orc.orc_create_xgrid(2, ni, ni, nlon, nlat, lon[t], lat[t], lo, la, None, capacity=64 * (ni * ni + nlon * nlat) + 1024)
             for t in tiles]
    o = {k: np.concatenate([p[k] for p in parts]) for k in ("i_in", "j_in", "i_out", "j_out")}
    o["t_in"] = np.concatenate([np.full(p["n"], k, dtype=np.int32) for k, p in enumerate(parts)])
    o["n"] = int(sum(p["n"] for p in parts))
    cell = o["t_in"].astype(np.int64) * ni * ni + o["j_in"] * ni + o["i_in"]
    first = np.flatnonzero(np.r_[True, cell[1:] != cell[:-1]])
    per = np.diff(np.r_[first, cell.size])
    dst = o["j_out"].astype(np.int64) * nlon + o["i_out"]
    span = np.maximum.reduceat(dst, first) - np.minimum.reduceat(dst, first) + 1
    st, bm = stage_of(span), span <= RANK_WORDS * 64
    for what, least in spec["has"].items():
        got = int(np.count_nonzero(CLASS[what](per, st, bm)))
        assert got >= least, (name, what, got, least)
    c = dict(ni=ni, nsrc=len(tiles) * ni * ni, nlon=nlon, oracle=o, grids=[fg.GridConfig(ni, ni, lon[t], lat[t]) for t in tiles],
             gout=fg.GridConfig(nlon, nlat, lo, la))
    _cases[name] = c
    return c


def run(fg, name, order, exact):
    """one search; the exchange cells as the compaction left them (c1 / c2 are the centroid integrals) and the per-cell sums"""
    if (name, order, exact) in _runs:
        return _runs[(name, order, exact)]
    import torch
    c = case(fg, name)
    L = fg.lib()
    L.fg_set_search_mode(1 if exact else 0)
    try:
        p = fg.XgridPlan.create(order, c["grids"], c["gout"])
    finally:
        L.fg_set_search_mode(0)
    r = dict(p.get_xgrid(), n=p.nxgrid, exact=p.stats()["exact_mode"])
    if order == 2:
        t = torch.empty(3 * p.ncells_in, dtype=torch.float64, device="cuda:0")
        p.copy_cell_sums(t)
        r["sums"] = t.cpu().numpy().reshape(3, p.ncells_in)
    p.destroy()
    _runs[(name, order, exact)] = r
    return r


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_exchange_cells_equal_the_exactly_sized_search_and_the_oracle(fg, gpu_ok, name, order):
    o = case(fg, name)["oracle"]
    a, b = run(fg, name, order, False), run(fg, name, order, True)
    assert a["exact"] == 0 and b["exact"] == 1
    assert a["n"] == b["n"] == o["n"] > 0
    for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(a[k], o[k]), k
        assert same_bits(a[k], b[k]), k
    for k in ("area",) + (("c1", "c2") if order == 2 else ()):
        assert same_bits(a[k], b[k]), k


@pytest.mark.parametrize("name", NAMES)
def test_cell_sums_are_the_left_to_right_sums(fg, gpu_ok, name):
    c = case(fg, name)
    ni = c["ni"]
    for exact in (False, True):
        x = run(fg, name, 2, exact)
        cell = x["t_in"].astype(np.int64) * ni * ni + x["j_in"].astype(np.int64) * ni + x["i_in"]
        start = np.flatnonzero(np.r_[True, cell[1:] != cell[:-1]])
        end = np.r_[start[1:], cell.size]
        want = np.zeros((3, c["nsrc"]))
        for m, k in enumerate(("area", "c1", "c2")):
            for a, b in zip(start, end):
                want[m, cell[a]] = np.cumsum(x[k][a:b])[-1]
        assert np.unique(cell[start]).size == start.size                    # (a cell's exchange cells are one run)
        assert same_bits(x["sums"], want), exact
