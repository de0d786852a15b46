"""CouplerMosaic (fg_coupler_*: make_coupler_mosaic.c:1198-2127, :2466-2811 as a device pipeline) against the line-by-line
restatement of tests/coupler_cases.py over the reference's compiled primitives.

Comparison rule: every index list identical; area, clon, clat, the six distances, the per-cell sums, the masks and nbad
bit-identical where orc.host_has_fma(), within 1e-10 relative otherwise (the convention of the suite's header).  Each case first
asserts its coverage conditions on the REFERENCE's result, so that a pass means something."""
import os

import numpy as np
import pytest

import coupler_cases as cc
import orc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not orc.ref_available(), reason="needs oracle/_ref (the reference compiled in place)")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if orc.host_has_fma():
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
    else:
        scale = np.max(np.abs(want)) if want.size else 0.0
        assert np.all(np.abs(got - want) <= 1e-10 * scale), what


def _run(fg, c, order):
    m = fg.CouplerMosaic(c["atm"], c["lnd"], c["ocn"], c["omask"], interp_order=order, ocn_south_ext=c["ext"])
    return m.run()


def _compare_list(got, ref, keys, order, what):
    for k in keys:
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), ref[k]), (what, k)
    names = ("area", "clon", "clat", "di1", "dj1", "di2", "dj2") if order == 2 else ("area",)
    for k in names:
        _same(got[k], ref[k], (what, k))


def _compare(m, c, r, order):
    nta, ntl = len(c["atm"]), len(r["land"])
    for na in range(nta):
        for nl in range(ntl):
            _compare_list(m.axl(na, nl), r["axl"][na][nl], ("ia", "ja", "il", "jl"), order, ("axl", na, nl))
        _compare_list(m.axo(na), r["axo"][na], ("ia", "ja", "io", "jo"), order, ("axo", na))
    for nl in range(len(r["lxo"])):
        _compare_list(m.lxo(nl), r["lxo"][nl], ("il", "jl", "io", "jo"), order, ("lxo", nl))
    # per-cell sums and masks
    o = m.cells(m.OCN)
    _same(o["area"], r["ocean"]["area"], "area_ocn")
    _same(o["xarea"], r["ocean"]["o_area"], "o_area")
    e = c["ext"]
    _same(o["frac"][e:], r["ocean"]["mask"], "ocean mask")
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
            _same(a["xarea"], r["atmos"][na]["a_area"], ("a_area", na))
            _same(a["clon"], r["atmos"][na]["a_clon"], ("a_clon", na))
            _same(a["clat"], r["atmos"][na]["a_clat"], ("a_clat", na))
    assert m.stats()["nbad"] == r["nbad"]


def _count(r, which):
    return sum(t["area"].size for row in r[which] for t in (row if which == "axl" else [row]))


def test_case_a_land_on_the_atmosphere_grid(fg, gpu_ok):
    c, r = cc.reference_of("a", fg, 2)
    assert _count(r, "axo") > 1000 and _count(r, "axl") >= 100
    assert r["cover"]["atm_without_axl"] >= 10 and r["cover"]["poly5"] >= 1
    with _run(fg, c, 2) as m:
        _compare(m, c, r, 2)
        s = m.stats()
        print("case A stats", s, m.phase_ms())
        assert s["naxo"] == _count(r, "axo") and s["naxl"] == _count(r, "axl") and s["nlxo"] == 0 and s["npolygons"] == r["cover"]["ncand"]
        assert 0 < s["d2h_bytes"] <= 4096, s                   # counts, error words and the searches' counter blocks: no list, no polygon
        with pytest.raises(fg.FregridHipError):
            m.lxo(0)
        m.run()                                                 # a second run on the same handle
        _compare(m, c, r, 2)


@pytest.mark.parametrize("order", [1, 2])
def test_case_b_land_of_its_own(fg, gpu_ok, order):
    c, r = cc.reference_of("b", fg, order)
    assert _count(r, "axl") > 300 and _count(r, "lxo") > 300 and r["cover"]["dropped"] >= 20
    with _run(fg, c, order) as m:
        _compare(m, c, r, order)
        assert m.stats()["nlxo"] == _count(r, "lxo")
        if order == 1:                                          # an order-1 handle has no centroids to hand out
            buf = np.empty(max(1, m.stats()["naxo"]))
            rc = fg.lib().fg_coupler_get(m.handle, m.AXO, 0, 0, None, None, None, None, None, buf.ctypes.data_as(fg.coupler._dpt), None, None, None,
                                         None, None)
            assert rc == -1 and "interp_order 2" in fg._lib.last_error()


@pytest.mark.parametrize("name", ["c0", "c1"])
def test_case_c_empty_lists(fg, gpu_ok, name):
    c, r = cc.reference_of(name, fg, 2)
    if name == "c0":                                            # omask == 0: no sea anywhere, every atmosphere cell is land
        assert _count(r, "axo") == 0 and _count(r, "axl") == sum(g.nx * g.ny for g in c["atm"])
    else:                                                       # omask == 1: no land anywhere
        assert _count(r, "axl") == 0 and _count(r, "axo") > 0
    with _run(fg, c, 2) as m:
        _compare(m, c, r, 2)
        for na in range(6):
            empty = m.axo(na) if name == "c0" else m.axl(na, na)
            assert all(v.size == 0 for v in empty.values())


def test_case_d_write(fg, gpu_ok, tmp_path):
    from scipy.io import netcdf_file
    c, r = cc.reference_of("a", fg, 2)
    with _run(fg, c, 2) as m:
        files = m.write(str(tmp_path))
    names = sorted(os.path.basename(f) for f in files)
    assert "ocean_mask.nc" in names and "land_mask_tile1.nc" in names and "atmos_mosaic_tile3Xocean_mosaic_tile1.nc" in names
    assert "atmos_mosaic_tile1Xland_mosaic_tile2.nc" not in names          # an empty list gets no file (:2136)
    for na in range(6):
        t = r["axo"][na]
        with netcdf_file(str(tmp_path / f"atmos_mosaic_tile{na + 1}Xocean_mosaic_tile1.nc"), mmap=False) as f:
            assert f.variables["contact"][:].tobytes().rstrip(b"\0").decode() == f"atmos_mosaic:tile{na + 1}::ocean_mosaic:tile1"
            assert f.variables["contact"].distant_to_parent2_centroid == b"tile2_distance"
            assert np.array_equal(f.variables["tile1_cell"][:], np.stack([t["ia"] + 1, t["ja"] + 1], axis=1))          # 1-based
            assert np.array_equal(f.variables["tile2_cell"][:], np.stack([t["io"] + 1, t["jo"] + 1 - c["ext"]], axis=1))      # :2309
            _same(f.variables["xgrid_area"][:], t["area"], "xgrid_area")
            _same(f.variables["tile1_distance"][:], np.stack([t["di1"], t["dj1"]], axis=1), "tile1_distance")
            _same(f.variables["tile2_distance"][:], np.stack([t["di2"], t["dj2"]], axis=1), "tile2_distance")
        t = r["axl"][na][na]
        with netcdf_file(str(tmp_path / f"atmos_mosaic_tile{na + 1}Xland_mosaic_tile{na + 1}.nc"), mmap=False) as f:
            assert np.array_equal(f.variables["tile2_cell"][:], np.stack([t["il"] + 1, t["jl"] + 1], axis=1))
            _same(f.variables["tile2_distance"][:], np.stack([t["di2"], t["dj2"]], axis=1), "axl tile2_distance")
        with netcdf_file(str(tmp_path / f"land_mask_tile{na + 1}.nc"), mmap=False) as f:
            _same(f.variables["mask"][:], r["land"][na]["mask"], "land mask")
            _same(f.variables["area_atm"][:], r["atmos"][na]["area"], "area_atm")
    with netcdf_file(str(tmp_path / "ocean_mask.nc"), mmap=False) as f:
        assert f.variables["mask"].shape == (24, 40)                       # without the added southern row
        _same(f.variables["mask"][:], r["ocean"]["mask"], "ocean mask")
        _same(f.variables["areaX"][:], r["ocean"]["areaX"], "areaX")


def test_errors_keep_the_references_texts(fg, gpu_ok):
    c = cc.case_c(fg, 0.5)
    with pytest.raises(fg.FregridHipError, match="interp_order should be 1 or 2"):
        fg.CouplerMosaic(c["atm"], None, c["ocn"], c["omask"], interp_order=3)
    with pytest.raises(fg.FregridHipError, match="below 1e-6"):
        fg.CouplerMosaic(c["atm"], None, c["ocn"], c["omask"], area_ratio_thresh=1e-8)
    with pytest.raises(fg.FregridHipError, match="outside"):
        fg.CouplerMosaic(c["atm"], None, c["ocn"], c["omask"] + 1.0)
    with fg.CouplerMosaic(c["atm"], None, c["ocn"], c["omask"]) as m:
        with pytest.raises(fg.FregridHipError, match="has not run"):
            m.axo(0)


def test_run_leaves_the_process_wide_search_frame_alone(fg, gpu_ok):
    """a tripolar target has raw longitudes outside [0, 2 pi): its exchange-cell areas differ in the last bits between the two
    frames (fg_set_search_frame), so a plan made after a run shows which frame the process is in"""
    c = cc.case_c(fg, 0.5)
    to, ta = fg.tripolar_corners(20, 12)
    dst = fg.GridConfig(20, 12, to, ta)

    def areas():
        p = fg.XgridPlan.create(2, c["atm"], dst)
        try:
            return p.get_xgrid()["area"]
        finally:
            p.destroy()

    before = areas()
    with fg.CouplerMosaic(c["atm"], None, c["ocn"], c["omask"]) as m:
        m.run()
    assert np.array_equal(_bits(before), _bits(areas()))
