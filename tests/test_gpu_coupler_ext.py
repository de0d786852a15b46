"""CouplerMosaic with a nested atmosphere tile (fg_coupler_set_nest), a wave grid (fg_coupler_add_wave) and --check
(fg_coupler_check) against the restatement of tests/coupler_ext_cases.py over the reference's compiled primitives.

Comparison rule, as tests/test_gpu_coupler_mosaic.py: every index list identical; area, clon, clat, the distances, the per-cell
sums, the masks and every number of check() bit-identical where orc.host_has_fma(), within 1e-10 relative otherwise; nbad and
the argmax of check() equal.  The great-circle case compares with the _cr oracle's primitives bit for bit, as
tests/test_gpu_coupler_gc.py.  The coverage each case relies on is asserted on the restatement in tests/test_coupler_ext_cpu.py."""
import os

import numpy as np
import pytest

import coupler_cases as cc
import coupler_ext_cases as ce
import coupler_gc_cases as cg
import orc
import polylist_gc_cases as pc

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not orc.ref_available(), reason="needs oracle/_ref (the reference compiled in place)")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what, exact=False):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if exact or orc.host_has_fma():
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
    else:
        scale = np.max(np.abs(want)) if want.size else 0.0
        assert np.all(np.abs(got - want) <= 1e-10 * scale), what


def _mosaic(fg, c, order, nest=False, wave=False, **kw):
    return fg.CouplerMosaic(c["atm"], c["lnd"], c["ocn"], c["omask"], interp_order=order, ocn_south_ext=c["ext"],
                            tile_nest=c["tile_nest"] if nest else None, wav=c["wav"] if wave else None,
                            wav_same_as_ocn=bool(wave and c.get("wav_same")), **kw)


def _compare_list(got, ref, keys, order, what):
    for k in keys:
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), ref[k]), (what, k)
    for k in ("area", "clon", "clat", "di1", "dj1", "di2", "dj2") if order == 2 else ("area",):
        _same(got[k], ref[k], (what, k))


def _compare_atm_side(m, c, r, order, ck):
    """lists, per-cell sums, masks, nbad: r from coupler_cases.reference_coupler or coupler_ext_cases.with_nest; ck: reference_check's"""
    nta, ntl = len(c["atm"]), len(r["land"])
    for na in range(nta):
        for nl in range(ntl):
            _compare_list(m.axl(na, nl), r["axl"][na][nl], ce.LIST_KEYS["axl"], order, ("axl", na, nl))
        _compare_list(m.axo(na), r["axo"][na], ce.LIST_KEYS["axo"], order, ("axo", na))
    for nl in range(len(r["lxo"])):
        _compare_list(m.lxo(nl), r["lxo"][nl], ce.LIST_KEYS["lxo"], order, ("lxo", nl))
    o = m.cells(m.OCN)
    _same(o["area"], r["ocean"]["area"], "area_ocn")
    _same(o["xarea"], r["ocean"]["o_area"], "o_area")
    _same(o["frac"][c["ext"]:], r["ocean"]["mask"], "ocean mask")
    for nl in range(ntl):
        l = m.cells(m.LND, nl)
        _same(l["area"], r["land"][nl]["area_lnd"], ("area_lnd", nl))
        _same(l["xarea"], r["land"][nl]["l_area"], ("l_area", nl))
        _same(l["frac"], r["land"][nl]["mask"], ("land mask", nl))
        if order == 2:
            _same(l["clon"], r["land"][nl]["l_clon"], ("l_clon", nl))
            _same(l["clat"], r["land"][nl]["l_clat"], ("l_clat", nl))
    if order == 2:
        _same(o["clon"], r["ocean"]["o_clon"], "o_clon")
        _same(o["clat"], r["ocean"]["o_clat"], "o_clat")
    for na in range(nta):
        a = m.cells(m.ATM, na)
        _same(a["area"], r["atmos"][na]["area"], ("area_atm", na))
        _same(a["xarea"], ck["atm_xarea"][na], ("atm_xarea", na))                   # :2210, :2333: every tile's, the nest's too
        if order == 2:
            _same(a["clon"], r["atmos"][na]["a_clon"], ("a_clon", na))              # the nest tile's: 0, as :1857 / :1903 leave them
            _same(a["clat"], r["atmos"][na]["a_clat"], ("a_clat", na))
    assert m.stats()["nbad"] == r["nbad"]


def _compare_check(got, ck):
    want = {k: v for k, v in ck.items() if k != "atm_xarea"}
    assert set(want) <= set(got) and set(got) - set(want) == {"max_area_atm", "max_atm_xarea"}, (sorted(got), sorted(want))
    for k in ("max_tile", "max_i", "max_j"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k, v in want.items():
        if k not in ("max_tile", "max_i", "max_j"):
            _same([got[k]], [v], ("check", k))


def _compare_wave(m, c, w, order):
    for tw in range(len(c["wav"])):
        _compare_list(m.wxo(tw), w["wxo"][tw], ce.LIST_KEYS["wxo"], order, ("wxo", tw))
        x = m.cells(m.WAV, tw)
        _same(x["area"], w["area_wav"][tw], ("area_wav", tw))
        _same(x["xarea"], w["w_area"][tw], ("w_area", tw))
        _same(x["frac"], w["mask"][tw], ("wave mask", tw))
        if order == 2:
            _same(x["clon"], w["w_clon"][tw], ("w_clon", tw))
            _same(x["clat"], w["w_clat"][tw], ("w_clat", tw))
    if order == 2:
        o = m.wave_ocean_cells()
        for got, want in (("xarea", "o_area"), ("clon", "o_clon"), ("clat", "o_clat")):
            _same(o[got], w[want], ("wave side", want))
    else:
        with pytest.raises(Exception, match="interp_order 2"):
            m.wave_ocean_cells()
    assert m.stats()["nwxo"] == sum(t["area"].size for t in w["wxo"])


@needs_ref
@pytest.mark.parametrize("order", [1, 2])
def test_case_n_nested_tile(fg, gpu_ok, order):
    c, r = ce.nest_reference(fg, order)
    ck = ce.check_of(c, r, tile_nest=6)
    with _mosaic(fg, c, order, nest=True) as m:
        m.run()
        _compare_atm_side(m, c, r, order, ck)
        _compare_check(m.check(), ck)
        m.run()                                                 # a second run on the same handle
        _compare_atm_side(m, c, r, order, ck)


@needs_ref
@pytest.mark.parametrize("name,order", [("w1", 1), ("w1", 2), ("w2", 2), ("w0", 2), ("wb", 2)])
def test_wave_cases(fg, gpu_ok, name, order, tmp_path):
    from scipy.io import netcdf_file
    c, r, w = ce.wave_reference(name, fg, order)
    ck = ce.check_of(c, r, w=w)
    with _mosaic(fg, c, order, wave=True) as m:
        m.run()
        _compare_wave(m, c, w, order)
        _compare_atm_side(m, c, r, order, ck)                   # the atmosphere side does not see the wave grid
        _compare_check(m.check(), ck)
        files = sorted(os.path.basename(f) for f in m.write_wave(str(tmp_path), wav_mosaic="ocean_mosaic" if name == "w2" else "wave_mosaic"))
    ntw = len(c["wav"])
    masks = ["wave_mask.nc"] if ntw == 1 else [f"wave_mask_tile{k + 1}.nc" for k in range(ntw)]
    xname = (lambda k: f"wav_ocean_mosaic_tile{k + 1}Xocn_ocean_mosaic_tile1.nc") if name == "w2" else (lambda k: f"wave_mosaic_tile{k + 1}Xocean_mosaic_tile1.nc")
    assert files == sorted(masks + [xname(k) for k in range(ntw) if w["wxo"][k]["area"].size]), files      # an empty list gets no file
    assert sorted(os.listdir(str(tmp_path))) == files
    for k in range(ntw):
        with netcdf_file(str(tmp_path / masks[k]), mmap=False) as f:
            assert set(f.variables) == {"mask"}
            _same(f.variables["mask"][:], w["mask"][k], "wave mask file")
        t = w["wxo"][k]
        if t["area"].size:
            with netcdf_file(str(tmp_path / xname(k)), mmap=False) as f:
                wm = "ocean_mosaic" if name == "w2" else "wave_mosaic"
                assert f.variables["contact"][:].tobytes().rstrip(b"\0").decode() == f"{wm}:tile{k + 1}::ocean_mosaic:tile1"
                assert np.array_equal(f.variables["tile1_cell"][:], np.stack([t["iw"] + 1, t["jw"] + 1], axis=1))
                assert np.array_equal(f.variables["tile2_cell"][:], np.stack([t["io"] + 1, t["jo"] + 1 - c["ext"]], axis=1))      # :3492
                _same(f.variables["xgrid_area"][:], t["area"], "xgrid_area")
                if order == 2:
                    _same(f.variables["tile1_distance"][:], np.stack([t["di1"], t["dj1"]], axis=1), "tile1_distance")
                    _same(f.variables["tile2_distance"][:], np.stack([t["di2"], t["dj2"]], axis=1), "tile2_distance")
                else:
                    assert "tile1_distance" not in f.variables


@needs_ref
def test_nest_and_wave_on_one_handle(fg, gpu_ok):
    c, r = ce.nest_reference(fg, 2)
    cw, _, w = ce.wave_reference("w1", fg, 2)
    c = dict(c, wav=cw["wav"])
    ck = ce.check_of(c, r, tile_nest=6, w=w)
    with _mosaic(fg, c, 2, nest=True, wave=True) as m:
        m.run()
        _compare_atm_side(m, c, r, 2, ck)
        _compare_wave(m, c, w, 2)
        got = m.check()
        _compare_check(got, ck)
        assert got["max_ratio"] >= 0 and got["max_tile"] >= 0 and "wxo_area_sum" in got and "axo_area_sum_nest" in got


def _gc_nest_case(fg):
    """coupler_gc_cases.own_c4 with a seventh atmosphere tile: a 3 x 3 block of the C4 tile 1 halved"""
    c = dict(cg.own_c4(fg))
    p = c["atm"][1]
    nlon, nlat = ce.nest_corners(p.lon, p.lat, 0, 1)
    c["atm"] = c["atm"] + [pc.Grid(6, 6, nlon, nlat)]
    c["tile_nest"] = 6
    return c


def test_case_n_on_the_great_circle_handle(fg, gpu_ok):
    P = pc.prims_oracle(True)

    def make():
        c = _gc_nest_case(fg)
        return c, cg.reference_coupler_gc(c["atm"], c["lnd"], c["ocn"], c["omask"], P, ocn_south_ext=c["ext"])
    c, r = pc.cached(("ext-gc-nest", P.name), make)
    area = lambda gs: [P.grid_area(g.nx, g.ny, g.lon, g.lat) for g in gs]
    a_atm, a_lnd, a_ocn = area(c["atm"]), area(c["lnd"]), area([c["ocn"]])[0]
    s = ce.sums_gc(c["atm"], c["lnd"], c["ocn"], c["omask"], a_atm, a_lnd, a_ocn, r["axl"], r["axo"], tile_nest=6, ocn_south_ext=c["ext"])
    s0 = ce.sums_gc(c["atm"], c["lnd"], c["ocn"], c["omask"], a_atm, a_lnd, a_ocn, r["axl"], r["axo"], tile_nest=-1, ocn_south_ext=c["ext"])
    assert r["axo"][6]["area"].size > 10 and r["axl"][6][0]["area"].size > 10
    assert np.count_nonzero(_bits(s["o_area"]) != _bits(s0["o_area"])) >= 3 and np.count_nonzero(_bits(s["l_area"][0]) != _bits(s0["l_area"][0])) >= 3
    ck = ce.reference_check(c["atm"], a_atm, r["axl"], r["axo"], tile_nest=6)
    cfg = lambda g: fg.GridConfig(g.nx, g.ny, g.lon, g.lat)
    with fg.CouplerMosaic([cfg(g) for g in c["atm"]], [cfg(g) for g in c["lnd"]], cfg(c["ocn"]), c["omask"], interp_order=1, ocn_south_ext=c["ext"],
                          clip_method="great_circle", tile_nest=6) as m:
        m.run()
        for na in range(7):
            got = m.axl(na, 0)
            for k in ce.LIST_KEYS["axl"]:
                assert np.array_equal(np.asarray(got[k], dtype=np.int64), r["axl"][na][0][k]), ("axl", na, k)
            _same(got["area"], r["axl"][na][0]["area"], ("axl", na), exact=True)
            got = m.axo(na)
            for k in ce.LIST_KEYS["axo"]:
                assert np.array_equal(np.asarray(got[k], dtype=np.int64), r["axo"][na][k]), ("axo", na, k)
            _same(got["area"], r["axo"][na]["area"], ("axo", na), exact=True)
            _same(m.cells(m.ATM, na)["xarea"], s["a_area"][na], ("a_area", na), exact=True)
        o, l = m.cells(m.OCN), m.cells(m.LND, 0)
        _same(o["xarea"], s["o_area"], "o_area", exact=True)
        _same(o["frac"], s["ocean_mask"], "ocean mask", exact=True)
        _same(l["xarea"], s["l_area"][0], "l_area", exact=True)
        _same(l["frac"], s["land_mask"][0], "land mask", exact=True)
        assert m.stats()["nbad"] == s["nbad"]
        got = m.check()
        assert (got["max_tile"], got["max_i"], got["max_j"]) == (ck["max_tile"], ck["max_i"], ck["max_j"])
        for k, v in ck.items():
            if k not in ("atm_xarea", "max_tile", "max_i", "max_j"):
                _same([got[k]], [v], ("check", k), exact=True)


@needs_ref
def test_a_handle_with_neither_keeps_its_results_and_its_d2h_bytes(fg, gpu_ok):
    """tile_nest = None, wav = None: byte for byte what the handle returned before these arguments existed (the restatement of
    tests/coupler_cases.py, bit for bit), and the bytes of a run are those of the recorded count"""
    c, r = cc.reference_of("b", fg, 2)
    ck = ce.check_of(c, r)
    with fg.CouplerMosaic(c["atm"], c["lnd"], c["ocn"], c["omask"], interp_order=2, ocn_south_ext=c["ext"]) as m:
        m.run()
        _compare_atm_side(m, c, r, 2, ck)
        s = m.stats()
        assert set(s) == {"d2h_bytes", "nbad", "searches", "naxo", "naxl", "nlxo", "npolygons", "ocn_south_ext"}
        assert set(m.phase_ms()) == {"create", "axl_candidates", "axo", "polygons_x_ocean", "lxo", "sums", "run"}
        plain = s["d2h_bytes"]
        _compare_check(m.check(), ck)
        assert m.stats()["d2h_bytes"] == plain                  # check() is not run()'s
        with pytest.raises(fg.FregridHipError, match="no wave grid"):
            m.wxo(0)
    # an explicit tile_nest = -1 through the C entry is the same handle
    with fg.CouplerMosaic(c["atm"], c["lnd"], c["ocn"], c["omask"], interp_order=2, ocn_south_ext=c["ext"]) as m:
        assert fg.lib().fg_coupler_set_nest(m.handle, -1) == 0
        m.run()
        assert m.stats()["d2h_bytes"] == plain
    # a nest copies nothing more either: the tile starts were read before
    cn, _ = ce.nest_reference(fg, 2)
    with _mosaic(fg, cn, 2) as m0, _mosaic(fg, cn, 2, nest=True) as m1:
        assert m0.run().stats()["d2h_bytes"] == m1.run().stats()["d2h_bytes"]


def test_d2h_bytes_with_a_wave_grid_do_not_grow_with_the_grids(fg, gpu_ok):
    def bytes_of(ni):
        b = cc.case_b(fg)
        lo, la = fg.latlon_corners(3 * ni, 2 * ni, 20.0, 200.0, -60.0, 70.0)
        wav = [fg.GridConfig(3 * ni, 2 * ni, lo, la)]
        with fg.CouplerMosaic(cc.cubed_sphere(fg, ni), b["lnd"], b["ocn"], b["omask"], interp_order=2, ocn_south_ext=b["ext"], wav=wav) as m:
            with_wave = m.run().stats()
        with fg.CouplerMosaic(cc.cubed_sphere(fg, ni), b["lnd"], b["ocn"], b["omask"], interp_order=2, ocn_south_ext=b["ext"]) as m:
            without = m.run().stats()
        assert with_wave["nwxo"] > 0
        return with_wave["d2h_bytes"], without["d2h_bytes"]
    c4, c8 = bytes_of(4), bytes_of(8)
    assert c4 == c8, (c4, c8)
    assert c4[0] > c4[1], c4                                     # the wave search's counter block and its list length


def test_refusals(fg, gpu_ok):
    a = cc.case_a(fg)                                            # land on the atmosphere grid
    with pytest.raises(fg.FregridHipError, match="land mosaic must be different from atmos mosaic"):
        fg.CouplerMosaic(a["atm"], None, a["ocn"], a["omask"], ocn_south_ext=a["ext"], tile_nest=2)
    b = cc.case_b(fg)
    for bad in (6, -2, 100):
        with pytest.raises(fg.FregridHipError, match="no atmosphere tile"):
            fg.CouplerMosaic(b["atm"], b["lnd"], b["ocn"], b["omask"], tile_nest=bad)
    with pytest.raises(fg.FregridHipError, match="great-circle handle takes no wave grid"):
        fg.CouplerMosaic(b["atm"], b["lnd"], b["ocn"], b["omask"], interp_order=1, clip_method="great_circle", wav=ce.wave_w1(fg))
    with fg.CouplerMosaic(b["atm"], b["lnd"], b["ocn"], b["omask"], wav=ce.wave_w1(fg)) as m:
        with pytest.raises(fg.FregridHipError, match="has not run"):
            m.wxo(0)
        with pytest.raises(fg.FregridHipError, match="has not run"):
            m.check()
        m.run()
        with pytest.raises(fg.FregridHipError, match="no wave tile"):
            m.wxo(1)
