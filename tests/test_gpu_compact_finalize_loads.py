"""k_compact's pair loader (csrc/xgrid_kernels.hip: d_cp_load issues the loads of a lane's main and halo pair together, ahead of
their guards, from clamped indices) and the record loop of k_csr_sortgather (csrc/apply_kernels.hip: d_csr_records, G entries
per lane and pass with a predicated tail) on the smallest grid pairs at which those loops take each of their paths.

References, none of them the code under test:
  * the CPU oracle (orc.orc_create_xgrid, tile by tile) for the exchange-cell list: count and indices identical, areas and
    centroid integrals within the bar of tests/test_gpu_xgrid.py (RTOL of the value, integrals on the scale of their largest);
  * numpy on what get_xgrid() returns: the canonical order (source tile, j_in, i_in, destination index, strictly ascending);
    the per-source-cell sums of copy_cell_sums against a float64 sum taken one exchange cell after the other; and, after
    finalize, the sweep of 8 levels against sweep_cases._sweep, the plain float64 loop over every destination row's exchange
    cells in list order -- which pins the CSR records and their order inside a row, bit for bit;
  * the other searches: exactly sized (fg_set_search_mode(1): the first attempt has capacity 0, so every clamp runs), the
    generic bins path (fg_set_search_rect(0)) and the fused finalize (fg_set_search_finalize(1)), all equal in bits.

Every case asserts, from the oracle's list, the property it is there for (CASES[...]["has"]).  Pair order on the device is not
known to the host (pairs include the rejected candidates and are appended by region), so the properties are stated on the
exchange cells, of which the pairs are a superset: a cell with more than 128 exchange cells has more than 128 pairs."""
import numpy as np
import pytest

import orc
import sweep_cases as sc

pytestmark = pytest.mark.gpu
RTOL = 1e-10                                   # tests/test_gpu_xgrid.py
CP_SMALL, BLOCK_PAIRS = 128, 256               # csrc/xgrid_kernels.hip
SHORT, STAGE1 = 12, 2048                       # csrc/apply_kernels.hip: k_csr_sortgather's SHORT, and CAP of its block-per-row form
NLEV = 8


def _per_cell(o):
    """exchange cells per source cell that has any, in list order"""
    key = (o["t_in"].astype(np.int64) << 40) | (o["j_in"].astype(np.int64) << 20) | o["i_in"]
    return np.diff(np.flatnonzero(np.r_[True, key[1:] != key[:-1], True]))


def _has_similar(o, c):
    per = _per_cell(o)
    ends = np.cumsum(per)
    cut = np.count_nonzero((ends - per) // BLOCK_PAIRS != (ends - 1) // BLOCK_PAIRS)
    assert per.max() <= CP_SMALL and o["n"] > 4 * BLOCK_PAIRS and cut >= 4, (per.max(), o["n"], cut)


def _has_one_tile(o, c):
    lens = np.bincount(o["dst"], minlength=c["ndst"])
    empty = lens == 0
    runs = np.diff(np.flatnonzero(np.diff(np.r_[0, empty.view(np.int8), 0])))[::2]
    assert np.count_nonzero(empty) > c["ndst"] // 2 and runs.max() >= 64 and o["n"] % BLOCK_PAIRS != 0, (np.count_nonzero(empty), runs.max())


def _has_mask(o, c):
    cells = np.unique(o["t_in"].astype(np.int64) * c["tile_cells"] + o["j_in"] * c["ni"] + o["i_in"])
    dead = np.flatnonzero(np.concatenate([m.ravel() for m in c["masks"]]) == 0)
    assert dead.size >= 6 * c["tile_cells"] // 3 - 6 and np.intersect1d(cells, dead).size == 0 and cells.size > 0


def _has_small_role_halo(o, c):
    per = _per_cell(o)
    small = per[per <= CP_SMALL]                                             # (the cells round the poles are big: 286 exchange cells)
    lens = np.bincount(o["dst"], minlength=c["ndst"])
    nq = np.add.reduceat(lens, np.arange(0, c["ndst"], 64))                  # the run of a block of 64 short rows
    assert small.size > 0.9 * per.size and 25 <= np.median(small) <= 60 and small.max() > 64, (np.median(small), small.max())
    assert np.any(nq % (64 * 4) != 0) and np.any(nq % (64 * 2) != 0)


def _has_big(o, c):
    assert _per_cell(o).max() > CP_SMALL


def _rows(o, c):
    return np.bincount(o["dst"], minlength=c["ndst"])


def _has_rows16(o, c):
    lens = _rows(o, c)
    assert lens.max() > SHORT and 8 * c["ndst"] < o["n"] <= 256 * c["ndst"], (lens.max(), o["n"])


def _has_row_blocks(o, c):
    lens = _rows(o, c)
    assert o["n"] > 256 * c["ndst"] and lens.max() <= STAGE1, (o["n"], lens.max())


def _has_row_beyond_staging(o, c):
    lens = _rows(o, c)
    assert o["n"] > 256 * c["ndst"] and lens.max() > STAGE1, lens


def _has_every_tail(o, c):
    """rows beyond the staging whose last pass of 256 * G entries (G = 2, 4) is 1, 2, ... G groups of 256 long, the last partly filled"""
    lens = _rows(o, c)
    tails = {int(-(-(n % 1024) // 256)) for n in lens if n > STAGE1}
    assert o["n"] > 256 * c["ndst"] and tails >= {1, 2, 3, 4} and np.all(lens % 256 != 0), (lens, tails)


def _has_regional(o, c):
    assert 0 < len(_per_cell(o)) < 6 * c["tile_cells"] // 2                  # most source cells have no exchange cell


def _has_band(o, c):
    assert o["n"] > 0 and np.unique(o["t_in"]).size < 6                      # whole tiles cannot meet the band


# source C<ni>, its tiles, target (nlon, nlat, lon0, lon1, lat0, lat1), rows of it, mask (True: every third cell), culling
CASES = {
    "similar C12 -> 72x36": dict(ni=12, tiles=range(6), tgt=(72, 36, 0., 360., -90., 90.), has=_has_similar),
    "one tile of C12 -> 72x36": dict(ni=12, tiles=(0,), tgt=(72, 36, 0., 360., -90., 90.), has=_has_one_tile),
    "C12 with a third masked -> 72x36": dict(ni=12, tiles=range(6), tgt=(72, 36, 0., 360., -90., 90.), mask=True, has=_has_mask),
    "coarse to fine C8 -> 144x90": dict(ni=8, tiles=range(6), tgt=(144, 90, 0., 360., -90., 90.), has=_has_small_role_halo),
    "coarse to fine C4 -> 288x180 (big cells)": dict(ni=4, tiles=range(6), tgt=(288, 180, 0., 360., -90., 90.), has=_has_big),
    "fine to coarse C48 -> 18x9": dict(ni=48, tiles=range(6), tgt=(18, 9, 0., 360., -90., 90.), has=_has_rows16),
    "fine to coarse C48 -> 6x3": dict(ni=48, tiles=range(6), tgt=(6, 3, 0., 360., -90., 90.), has=_has_row_blocks),
    "fine to coarse C64 -> 4x2": dict(ni=64, tiles=range(6), tgt=(4, 2, 0., 360., -90., 90.), has=_has_row_beyond_staging),
    "fine to coarse C64 thinned row by row -> 4x2": dict(ni=64, tiles=range(6), tgt=(4, 2, 0., 360., -90., 90.), mask="by row", has=_has_every_tail),
    "C48 -> regional 80x50": dict(ni=48, tiles=range(6), tgt=(80, 50, 230., 310., 15., 65.), has=_has_regional),
    "C12 -> rows 0..8 of 72x36, culling": dict(ni=12, tiles=range(6), tgt=(72, 36, 0., 360., -90., 90.), rows=(0, 8), cull=True, has=_has_band),
}
NAMES = list(CASES)
MODES = ("default", "exact", "generic", "fused")
_cases, _runs = {}, {}


def case(fg, name):
    """grids, masks and the oracle's exchange-cell list of a case, made once"""
    if name in _cases:
        return _cases[name]
    spec = CASES[name]
    ni = spec["ni"]
    lon, lat = fg.gnomonic_ed_corners(ni)
    tiles = list(spec["tiles"])
    nlon, nlat = spec["tgt"][:2]
    lo, la = fg.latlon_corners(*spec["tgt"])
    if "rows" in spec:
        j0, j1 = spec["rows"]
        lo, la, nlat = np.ascontiguousarray(lo[j0:j1 + 1]), np.ascontiguousarray(la[j0:j1 + 1]), j1 - j0
    def oracle_list(masks):
        parts = [orc.orc_create_xgrid(2, ni, ni, nlon, nlat, lon[t], lat[t], lo, la, None if masks is None else masks[k],
                                      capacity=64 * (ni * ni + nlon * nlat) + 1024) for k, t in enumerate(tiles)]
        o = {k: np.concatenate([p[k] for p in parts]) for k in ("i_in", "j_in", "i_out", "j_out", "area", "clon", "clat")}
        o["t_in"] = np.concatenate([np.full(p["n"], k, dtype=np.int32) for k, p in enumerate(parts)])
        o["n"] = int(sum(p["n"] for p in parts))
        o["dst"] = o["j_out"].astype(np.int64) * nlon + o["i_out"]
        return o

    masks = None
    if spec.get("mask") == "by row":
        # destination row r loses about 8 r per cent of its source cells (a cell counts for the row of its first exchange cell):
        # eight rows of eight lengths from one symmetric grid pair, whose rows all have 3142 entries
        o = oracle_list(None)
        cell = o["t_in"].astype(np.int64) * ni * ni + o["j_in"] * ni + o["i_in"]
        first = np.flatnonzero(np.r_[True, cell[1:] != cell[:-1]])
        keep = np.ones(len(tiles) * ni * ni)
        keep[cell[first]] = np.random.default_rng(8).random(first.size) >= 0.08 * o["dst"][first]
        masks = [keep[k * ni * ni:(k + 1) * ni * ni].reshape(ni, ni) for k in range(len(tiles))]
    elif spec.get("mask"):
        masks = [((np.arange(ni * ni) + t) % 3 != 0).astype(np.float64).reshape(ni, ni) for t in tiles]
    c = dict(name=name, ni=ni, tile_cells=ni * ni, tiles=tiles, nlon=nlon, nlat=nlat, ndst=nlon * nlat, lo=lo, la=la, masks=masks,
             cull=bool(spec.get("cull")), grids=[fg.GridConfig(ni, ni, lon[t], lat[t]) for t in tiles],
             gout=fg.GridConfig(nlon, nlat, lo, la))
    o = oracle_list(masks)
    spec["has"](o, c)
    c["oracle"] = o
    rng = np.random.default_rng(5)
    nt = len(tiles)
    c["f1"] = rng.standard_normal((NLEV, nt * ni * ni))
    c["f2"] = rng.standard_normal((NLEV, nt * (ni + 2) ** 2))
    c["gx"], c["gy"] = rng.standard_normal((NLEV, nt * ni * ni)), rng.standard_normal((NLEV, nt * ni * ni))
    _cases[name] = c
    return c


def run(fg, name, order, mode):
    """one search in `mode`, its finalize and one sweep of NLEV levels; `default` also keeps the list and the sums as they are
    before finalize (c1 / c2 still the centroid integrals)"""
    if (name, order, mode) in _runs:
        return _runs[(name, order, mode)]
    import torch
    c = case(fg, name)
    L = fg.lib()
    L.fg_set_search_mode(1 if mode == "exact" else 0); L.fg_set_search_rect(0 if mode == "generic" else 1)
    L.fg_set_search_finalize(1 if mode == "fused" else 0); L.fg_set_search_cull(1 if c["cull"] else 0)
    try:
        p = fg.XgridPlan.create(order, c["grids"], c["gout"], masks=c["masks"])
    finally:
        L.fg_set_search_mode(0); L.fg_set_search_rect(1); L.fg_set_search_finalize(0); L.fg_set_search_cull(0)
    r = dict(n=p.nxgrid, stats=p.stats())
    if mode == "default":
        r["before"] = p.get_xgrid()
        if order == 2:
            t = torch.empty(3 * p.ncells_in, dtype=torch.float64, device="cuda:0")
            p.copy_cell_sums(t)
            r["sums"] = t.cpu().numpy().reshape(3, p.ncells_in)
    p.finalize(None)
    r.update(p.get_xgrid())                           # after finalize: c1 / c2 are di / dj
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    out = torch.full((NLEV, c["ndst"]), np.nan, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()                          # (the fill runs on torch's stream, the library on the plan's own)
    if order == 2:
        p.apply(dev(c["f2"]), out, nz=NLEV, grad_x_t=dev(c["gx"]), grad_y_t=dev(c["gy"]))
    else:
        p.apply(dev(c["f1"]), out, nz=NLEV)
    p.sync()
    r["out"] = out.cpu().numpy()
    p.destroy()
    _runs[(name, order, mode)] = r
    return r


def relerr(a, b):
    scale = np.maximum(np.abs(b), 1e-10 * np.max(np.abs(b)) + 1e-300)
    return float(np.max(np.abs(a - b) / scale)) if len(b) else 0.0


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_exchange_cells_equal_the_oracle_in_canonical_order(fg, gpu_ok, name, order):
    c = case(fg, name)
    o, x = c["oracle"], run(fg, name, order, "default")["before"]
    assert len(x["area"]) == o["n"] > 0
    for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(x[k], o[k]), k
    assert relerr(x["area"], o["area"]) < RTOL
    if order == 2:
        for a, k in ((x["c1"], "clon"), (x["c2"], "clat")):
            assert np.max(np.abs(a - o[k])) <= RTOL * np.max(np.abs(o[k])), k
    key = np.stack([x["t_in"], x["j_in"], x["i_in"], x["j_out"].astype(np.int64) * c["nlon"] + x["i_out"]]).astype(np.int64)
    d = np.diff(key, axis=1)
    first = np.argmax(d != 0, axis=0)                                        # the first key that differs from the predecessor's
    assert np.all(np.any(d != 0, axis=0)) and np.all(d[first, np.arange(d.shape[1])] > 0)


@pytest.mark.parametrize("name", NAMES)
def test_cell_sums_add_the_exchange_cells_one_by_one(fg, gpu_ok, name):
    c = case(fg, name)
    r = run(fg, name, 2, "default")
    x = r["before"]
    ni, nsrc = c["ni"], len(c["tiles"]) * c["tile_cells"]
    cell = x["t_in"].astype(np.int64) * c["tile_cells"] + x["j_in"] * ni + x["i_in"]
    start = np.flatnonzero(np.r_[True, cell[1:] != cell[:-1]])
    per = np.diff(np.r_[start, cell.size])
    want = np.zeros((3, nsrc))
    vals = np.stack([x["area"], x["c1"], x["c2"]])
    for k in range(int(per.max())):                                          # step k adds cell k of every source cell that has one
        live = per > k
        want[:, cell[start[live]]] = want[:, cell[start[live]]] + vals[:, start[live] + k]
    assert sc.same(r["sums"], want)
    assert np.count_nonzero(want[0]) == start.size


def _plain(c, x, order):
    """sweep_cases._sweep on the list x: every destination row's exchange cells in list order, float64"""
    ni = c["ni"]
    t, i, j = x["t_in"].astype(np.int64), x["i_in"].astype(np.int64), x["j_in"].astype(np.int64)
    dst = x["j_out"].astype(np.int64) * c["nlon"] + x["i_out"]
    lens = np.bincount(dst, minlength=c["ndst"])
    cc = dict(x=dict(area=x["area"], di=x.get("c1"), dj=x.get("c2")), src=t * ni * ni + j * ni + i,
              fidx=t * (ni + 2) ** 2 + (j + 1) * (ni + 2) + i + 1, dst=dst, ndst=c["ndst"], nx=len(dst), lens=lens,
              row_ptr=np.r_[0, np.cumsum(lens)])
    return sc._sweep(cc, order, c["f2"] if order == 2 else c["f1"], c["gx"], c["gy"], None, False, -1.0e20)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_sweep_equals_the_plain_loop_over_each_row(fg, gpu_ok, name, order):
    c = case(fg, name)
    r = run(fg, name, order, "default")
    assert sc.same(r["out"], _plain(c, r, order))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_the_other_searches_keep_the_bits(fg, gpu_ok, name, order):
    a = run(fg, name, order, "default")
    assert a["stats"]["bins"] == 0
    for mode in MODES[1:]:
        b = run(fg, name, order, mode)
        if mode == "exact":
            assert b["stats"]["exact_mode"] == 1
        if mode == "generic":
            assert b["stats"]["bins"] > 0
        assert a["n"] == b["n"] > 0, mode
        for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(a[k], b[k]), (mode, k)
        for k in ("area", "out") + (("c1", "c2") if order == 2 else ()):
            assert sc.same(a[k], b[k]), (mode, k)
