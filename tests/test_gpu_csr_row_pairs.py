"""The row lists of the finalize hold pairs {exchange cell, source cell} and the centroid pass writes one record per source cell
(csrc/xgrid_device.h: FgRowEnt, FgSrcRec).  tests/test_gpu_compact_finalize_loads.py pins the searched order-1/2 plans (default,
exact, generic, fused); this file covers the producers and consumers of the two layouts which that file does not reach:

  * k_csr_fill        lists that arrive from outside (create_empty + set_xgrid, which builds the CSR records itself: a plan made
                      that way is finalized when set_xgrid returns and fg_plan_finalize refuses it), order 1 and order 2 with
                      di / dj handed in -- the record loop without centroids;
  * k_csr_fill_pos    the great-circle search, whose row slots are taken in the compaction;
  * fg_plan_finalize  with totals handed in, against its own sums and against the fused finalize;
  * k_distances       di / dj of get_xgrid() after finalize, from the per-source-cell record.

References, never the code under test: sweep_cases._sweep (the plain float64 loop over each destination row's exchange cells in
list order) compared with sweep_cases.same, i.e. in bits; numpy for the centroids; the CPU oracles for the lists.

Four grid pairs, one per way k_csr_sortgather sorts a row (six tiles, global lat-lon target); every test asserts the class of
its pair from the oracle's list before it uses the device.  Exchange cells and longest row, legacy / great circle:
  C12 -> 72x36   6336, 4 / 6336, 4            64 rows per wave, rows <= 12: lane-serial insertion
  C48 -> 18x9    17232, 181 / 17232, 183      16 rows per block, rows > 12 ranked by the block, some runs of 16 rows beyond 2048
  C48 -> 6x3     15008, 1268 / 11686, 1074    a block per row, 256 < row <= 2048: several elements per lane
  C64 -> 4x2     25136, 3142 / 25109, 3139    a block per row, row > 2048: through the scratch"""
import numpy as np
import pytest

import orc
import sweep_cases as sc

pytestmark = pytest.mark.gpu
SHORT, STAGE0, STAGE1, BT = 12, 512, 2048, 256     # csrc/apply_kernels.hip: k_csr_sortgather's SHORT, CAP (64 rows / else), lanes
NLEV = 8


def _is_rows64(n, lens, ndst):
    nq = np.add.reduceat(lens, np.arange(0, ndst, 64))
    assert n <= 8 * ndst and lens.max() <= SHORT and nq.max() <= STAGE0, (n, lens.max(), nq.max())


def _is_rows16(n, lens, ndst):
    nq = np.add.reduceat(lens, np.arange(0, ndst, 16))
    assert 8 * ndst < n <= 256 * ndst and lens.max() > SHORT and nq.max() > STAGE1 > nq.min(), (n, lens.max(), nq)


def _is_row_blocks(n, lens, ndst):
    assert n > 256 * ndst and BT < lens.max() <= STAGE1, (n, lens.max())


def _is_row_scratch(n, lens, ndst):
    assert n > 256 * ndst and lens.max() > STAGE1, (n, lens.max())


# source C<ni> -> nlon x nlat; (exchange cells, longest row) of the legacy and of the great-circle oracle; the class
PAIRS = {
    "C12 -> 72x36": dict(ni=12, tgt=(72, 36), legacy=(6336, 4), gc=(6336, 4), cls=_is_rows64),
    "C48 -> 18x9": dict(ni=48, tgt=(18, 9), legacy=(17232, 181), gc=(17232, 183), cls=_is_rows16),
    "C48 -> 6x3": dict(ni=48, tgt=(6, 3), legacy=(15008, 1268), gc=(11686, 1074), cls=_is_row_blocks),
    "C64 -> 4x2": dict(ni=64, tgt=(4, 2), legacy=(25136, 3142), gc=(25109, 3139), cls=_is_row_scratch),
}
NAMES = list(PAIRS)
_pairs, _lists, _plans = {}, {}, {}


def pair(fg, name):
    """grids and fields of a pair, made once"""
    if name not in _pairs:
        spec = PAIRS[name]
        ni, (nlon, nlat) = spec["ni"], spec["tgt"]
        lon, lat = fg.gnomonic_ed_corners(ni)
        lo, la = fg.latlon_corners(nlon, nlat)
        rng = np.random.default_rng(11)
        _pairs[name] = dict(name=name, ni=ni, nlon=nlon, nlat=nlat, ndst=nlon * nlat, nsrc=6 * ni * ni, lon=lon, lat=lat, lo=lo, la=la,
                            grids=[fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)], gout=fg.GridConfig(nlon, nlat, lo, la),
                            f1=rng.standard_normal((NLEV, 6 * ni * ni)), f2=rng.standard_normal((NLEV, 6 * (ni + 2) ** 2)),
                            gx=rng.standard_normal((NLEV, 6 * ni * ni)), gy=rng.standard_normal((NLEV, 6 * ni * ni)))
    return _pairs[name]


def oracle_list(fg, name, method):
    """the CPU oracle's exchange cells of the six tiles, tile by tile; asserts the pair's row-length class on them"""
    if (name, method) not in _lists:
        c = pair(fg, name)
        ni, nlon, nlat = c["ni"], c["nlon"], c["nlat"]
        cap = 64 * (ni * ni + nlon * nlat) + 1024
        if method == "legacy":
            parts = [orc.orc_create_xgrid(2, ni, ni, nlon, nlat, c["lon"][t], c["lat"][t], c["lo"], c["la"], capacity=cap) for t in range(6)]
        else:
            parts = [orc.orc_create_xgrid_gc(ni, ni, nlon, nlat, c["lon"][t], c["lat"][t], c["lo"], c["la"], capacity=cap) for t in range(6)]
        o = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "n"}
        o["t_in"] = np.concatenate([np.full(p["n"], t, dtype=np.int32) for t, p in enumerate(parts)])
        o["n"] = int(sum(p["n"] for p in parts))
        lens = np.bincount(o["j_out"].astype(np.int64) * nlon + o["i_out"], minlength=c["ndst"])
        assert (o["n"], int(lens.max())) == PAIRS[name][method], (o["n"], int(lens.max()))
        PAIRS[name]["cls"](o["n"], lens, c["ndst"])
        _lists[(name, method)] = o
    return _lists[(name, method)]


def plain(c, x, order, di=None, dj=None):
    """sweep_cases._sweep on the list x: every destination row's exchange cells in list order, float64"""
    ni = c["ni"]
    t, i, j = x["t_in"].astype(np.int64), x["i_in"].astype(np.int64), x["j_in"].astype(np.int64)
    dst = x["j_out"].astype(np.int64) * c["nlon"] + x["i_out"]
    lens = np.bincount(dst, minlength=c["ndst"])
    cc = dict(x=dict(area=x["area"], di=di, dj=dj), src=t * ni * ni + j * ni + i, fidx=t * (ni + 2) ** 2 + (j + 1) * (ni + 2) + i + 1,
              dst=dst, ndst=c["ndst"], nx=len(dst), lens=lens, row_ptr=np.r_[0, np.cumsum(lens)])
    return sc._sweep(cc, order, c["f2"] if order == 2 else c["f1"], c["gx"], c["gy"], None, False, -1.0e20)


def sweep(c, p, order):
    """NLEV levels through the finalized plan p"""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    out = torch.full((NLEV, c["ndst"]), np.nan, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()                          # (the fill runs on torch's stream, the library on the plan's own)
    if order == 2:
        p.apply(dev(c["f2"]), out, nz=NLEV, grad_x_t=dev(c["gx"]), grad_y_t=dev(c["gy"]))
    else:
        p.apply(dev(c["f1"]), out, nz=NLEV)
    p.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_list_from_outside_sweeps_like_the_plain_loop(fg, gpu_ok, name, order):
    c, o = pair(fg, name), oracle_list(fg, name, "legacy")
    rng = np.random.default_rng(23)
    di, dj = (rng.uniform(-0.02, 0.02, o["n"]), rng.uniform(-0.02, 0.02, o["n"])) if order == 2 else (None, None)
    p = fg.XgridPlan.create_empty(order, [c["ni"]] * 6, [c["ni"]] * 6, c["nlon"], c["nlat"])
    try:
        p.set_xgrid(o["t_in"], o["i_in"], o["j_in"], o["i_out"], o["j_out"], o["area"], di, dj)    # (builds the rows and the records)
        out = sweep(c, p, order)
    finally:
        p.destroy()
    assert sc.same(out, plain(c, o, order, di, dj))


@pytest.mark.parametrize("name", NAMES)
def test_great_circle_search_sweeps_like_the_plain_loop(fg, gpu_ok, name):
    c, o = pair(fg, name), oracle_list(fg, name, "gc")
    p = fg.XgridPlan.create_great_circle(c["grids"], c["gout"])
    try:
        p.finalize(None)
        x = p.get_xgrid()
        out = sweep(c, p, 1)
    finally:
        p.destroy()
    assert len(x["area"]) == o["n"]
    for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(x[k], o[k]), k
    assert sc.same(out, plain(c, x, 1))


def searched(fg, name, how):
    """an order-2 legacy search finalized with its own sums (`own`), with a copy of them handed in (`handed`) or by the search
    itself (`fused`): the list before finalize, the sums, the list after, one sweep"""
    if (name, how) in _plans:
        return _plans[(name, how)]
    import torch
    c = pair(fg, name)
    L = fg.lib()
    L.fg_set_search_finalize(1 if how == "fused" else 0)
    try:
        p = fg.XgridPlan.create(2, c["grids"], c["gout"])
    finally:
        L.fg_set_search_finalize(0)
    try:
        r = {}
        if how != "fused":
            r["before"] = p.get_xgrid()
            t = torch.empty(3 * p.ncells_in, dtype=torch.float64, device="cuda:0")
            p.copy_cell_sums(t)
            r["sums"] = t.cpu().numpy().reshape(3, p.ncells_in)
            p.finalize(t.data_ptr() if how == "handed" else None)
        r.update(p.get_xgrid())
        r["out"] = sweep(c, p, 2)
    finally:
        p.destroy()
    _plans[(name, how)] = r
    return r


@pytest.mark.parametrize("name", NAMES[:2])
def test_handed_in_totals_keep_the_bits(fg, gpu_ok, name):
    oracle_list(fg, name, "legacy")                   # (the class of the pair)
    a = searched(fg, name, "handed")
    for how in ("own", "fused"):
        b = searched(fg, name, how)
        assert len(a["area"]) == len(b["area"]) > 0, how
        for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(a[k], b[k]), (how, k)
        for k in ("area", "c1", "c2", "out"):
            assert sc.same(a[k], b[k]), (how, k)


def test_distances_on_request_are_numpy_s(fg, gpu_ok):
    name = NAMES[0]
    c, o = pair(fg, name), oracle_list(fg, name, "legacy")
    ni, nsrc = c["ni"], c["nsrc"]
    # every source cell is fully covered (the centroid is then sum of integrals / sum of areas: conserve_interp.c:337-340)
    cell_area = np.concatenate([orc.orc_get_grid_area(ni, ni, c["lon"][t], c["lat"][t]) for t in range(6)])
    s_o = o["t_in"].astype(np.int64) * ni * ni + o["j_in"] * ni + o["i_in"]
    covered = np.bincount(s_o, weights=o["area"], minlength=nsrc)
    assert nsrc == 864 and np.max(np.abs(covered - cell_area) / cell_area) < 1e-12
    r = searched(fg, name, "own")
    x, S = r["before"], r["sums"]
    s = x["t_in"].astype(np.int64) * ni * ni + x["j_in"] * ni + x["i_in"]
    assert np.array_equal(s, s_o) and len(r["c1"]) == o["n"]
    assert sc.same(r["area"], x["area"])
    assert sc.same(r["c1"], x["c1"] / x["area"] - (S[1] / S[0])[s])
    assert sc.same(r["c2"], x["c2"] / x["area"] - (S[2] / S[0])[s])
    assert sc.same(r["out"], plain(c, r, 2, r["c1"], r["c2"]))
