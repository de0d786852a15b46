"""CouplerMosaic(clip_method="great_circle") (fg_coupler_create_gc: make_coupler_mosaic's GREAT_CIRCLE_CLIP branch as a device pipeline)
against tests/coupler_gc_cases.py run over the _cr oracle's primitives: every list (atmosphere x land, atmosphere x ocean, land x
ocean) with identical indices in identical order, areas, per-cell a_area / l_area / o_area, model areas and masks BIT-IDENTICAL,
nbad equal, no tolerance.  The _cr restatement is tied to the compiled reference on the CPU (tests/test_coupler_gc_cpu.py)."""
import os

import numpy as np
import pytest

import coupler_cases as cc
import coupler_gc_cases as cg
import polylist_gc_cases as pc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _cfg(fg, g):
    return fg.GridConfig(g.nx, g.ny, g.lon, g.lat)


def _mosaic(fg, c, **kw):
    lnd = None if c["lnd"] is None else [_cfg(fg, g) for g in c["lnd"]]
    return fg.CouplerMosaic([_cfg(fg, g) for g in c["atm"]], lnd, _cfg(fg, c["ocn"]), c["omask"], interp_order=kw.pop("interp_order", 1),
                            ocn_south_ext=c["ext"], clip_method="great_circle", **kw)


def _compare_list(got, ref, keys, what):
    for k in keys:
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), ref[k]), (what, k)
    _same(got["area"], ref["area"], (what, "area"))


def _compare(m, c, r):
    nta, ntl = len(c["atm"]), len(r["land"])
    for na in range(nta):
        for nl in range(ntl):
            _compare_list(m.axl(na, nl), r["axl"][na][nl], ("ia", "ja", "il", "jl"), ("axl", na, nl))
        _compare_list(m.axo(na), r["axo"][na], ("ia", "ja", "io", "jo"), ("axo", na))
    for nl in range(len(r["lxo"])):
        _compare_list(m.lxo(nl), r["lxo"][nl], ("il", "jl", "io", "jo"), ("lxo", nl))
    o = m.cells(m.OCN)
    _same(o["area"], r["ocean"]["area"], "area_ocn")
    _same(o["xarea"], r["ocean"]["o_area"], "o_area")
    _same(o["frac"], r["ocean"]["mask"], "ocean mask")
    for nl in range(ntl):
        l = m.cells(m.LND, nl)
        _same(l["area"], r["land"][nl]["area"], ("area_lnd", nl))
        _same(l["xarea"], r["land"][nl]["l_area"], ("l_area", nl))
        _same(l["frac"], r["land"][nl]["mask"], ("land mask", nl))
    for na in range(nta):
        a = m.cells(m.ATM, na)
        _same(a["area"], r["atmos"][na]["area"], ("area_atm", na))
        _same(a["xarea"], r["atmos"][na]["a_area"], ("a_area", na))
    assert m.stats()["nbad"] == r["nbad"]


def _count(r, which):
    return sum(t["area"].size for row in r[which] for t in (row if which == "axl" else [row]))


@pytest.mark.parametrize("name", ["same_c5", "own_c4", "own_c4_two_land_tiles"])
def test_lists_sums_and_masks(fg, gpu_ok, name):
    c, r = cg.reference_of(name, fg, pc.prims_oracle(True))
    rem = r["cover"]["remembered"]
    if name == "same_c5":
        assert _count(r, "axo") > 900 and _count(r, "axl") == 150 and r["cover"]["pole_ocn_cells"] == 30
    else:
        assert rem.get(3, 0) >= 1 and sum(v for k, v in rem.items() if k >= 6) >= 1, rem      # both ends of the n-gon path
        assert max(r["cover"]["poly_x_ocn"]) >= 6 and r["cover"]["dropped"] >= 1 and _count(r, "lxo") > 500
    with _mosaic(fg, c) as m:
        m.run()
        _compare(m, c, r)
        s = m.stats()
        print(name, "stats", s, m.phase_ms())
        assert s["naxo"] == _count(r, "axo") and s["naxl"] == _count(r, "axl") and s["nlxo"] == _count(r, "lxo")
        assert s["npolygons"] == sum(rem.values())
        assert 0 < s["d2h_bytes"] <= 4096, s                    # counts, error words and the searches' counter blocks only
        m.run()                                                 # a second run on the same handle
        _compare(m, c, r)


@pytest.mark.parametrize("name", ["same_c5_omask0", "same_c5_omask1"])
def test_uniform_ocean_fractions_and_files(fg, gpu_ok, name, tmp_path):
    from scipy.io import netcdf_file
    c, r = cg.reference_of(name, fg, pc.prims_oracle(True))
    if name.endswith("0"):                                      # no sea anywhere: no atmosphere x ocean cell, every atmosphere cell is land
        assert _count(r, "axo") == 0 and _count(r, "axl") == 150
    else:                                                       # sea everywhere but the added southern row (omask 0 there)
        assert _count(r, "axo") > 1000 and 0 < _count(r, "axl") < 20
    with _mosaic(fg, c) as m:
        m.run()
        _compare(m, c, r)
        assert 0 < m.stats()["d2h_bytes"] <= 4096, m.stats()
        files = m.write(str(tmp_path))
    names = sorted(os.path.basename(f) for f in files)
    assert "ocean_mask.nc" in names and "land_mask_tile1.nc" in names
    for na in range(6):                                         # an empty list gets no file (:2136)
        for which, fname in (("axo", f"atmos_mosaic_tile{na + 1}Xocean_mosaic_tile1.nc"), ("axl", f"atmos_mosaic_tile{na + 1}Xland_mosaic_tile{na + 1}.nc")):
            t = r[which][na] if which == "axo" else r[which][na][na]
            assert (fname in names) == (t["area"].size > 0) == os.path.exists(tmp_path / fname), fname
            if t["area"].size == 0:
                continue
            with netcdf_file(str(tmp_path / fname), mmap=False) as f:
                second = ("io", "jo") if which == "axo" else ("il", "jl")
                shift = 1 - c["ext"] if which == "axo" else 1
                assert np.array_equal(f.variables["tile1_cell"][:], np.stack([t["ia"] + 1, t["ja"] + 1], axis=1))
                assert np.array_equal(f.variables["tile2_cell"][:], np.stack([t[second[0]] + 1, t[second[1]] + shift], axis=1))
                _same(f.variables["xgrid_area"][:], t["area"], "xgrid_area")
                assert "tile1_distance" not in f.variables and "tile2_distance" not in f.variables      # order 1
    with netcdf_file(str(tmp_path / "ocean_mask.nc"), mmap=False) as f:
        assert f.variables["mask"].shape == (20, 30)            # without the added southern row
        _same(f.variables["mask"][:], r["ocean"]["mask"][c["ext"]:], "ocean mask")
        _same(f.variables["areaX"][:], r["ocean"]["o_area"][c["ext"]:], "areaX")


def test_files_of_land_of_its_own(fg, gpu_ok, tmp_path):
    """own_c4_two_land_tiles written and read back: atmosphere tile x land tile files with the two tile numbers different, the land x
    ocean files, the land masks without area_atm"""
    from scipy.io import netcdf_file
    c, r = cg.reference_of("own_c4_two_land_tiles", fg, pc.prims_oracle(True))
    with _mosaic(fg, c) as m:
        m.run()
        files = m.write(str(tmp_path))
    names = sorted(os.path.basename(f) for f in files)

    def check(fname, t, first, second, shift):
        assert (fname in names) == (t["area"].size > 0) == os.path.exists(tmp_path / fname), fname
        if t["area"].size == 0:
            return 0
        with netcdf_file(str(tmp_path / fname), mmap=False) as f:
            assert np.array_equal(f.variables["tile1_cell"][:], np.stack([t[first[0]] + 1, t[first[1]] + 1], axis=1))
            assert np.array_equal(f.variables["tile2_cell"][:], np.stack([t[second[0]] + 1, t[second[1]] + shift], axis=1))
            _same(f.variables["xgrid_area"][:], t["area"], fname)
            assert "tile1_distance" not in f.variables and "tile2_distance" not in f.variables
        return 1

    nfiles = 0
    for na in range(6):
        for nl in range(2):
            nfiles += check(f"atmos_mosaic_tile{na + 1}Xland_mosaic_tile{nl + 1}.nc", r["axl"][na][nl], ("ia", "ja"), ("il", "jl"), 1)
        check(f"atmos_mosaic_tile{na + 1}Xocean_mosaic_tile1.nc", r["axo"][na], ("ia", "ja"), ("io", "jo"), 1 - c["ext"])
    assert nfiles >= 8                                          # most atmosphere tiles meet both land tiles
    for nl in range(2):
        assert check(f"land_mosaic_tile{nl + 1}Xocean_mosaic_tile1.nc", r["lxo"][nl], ("il", "jl"), ("io", "jo"), 1 - c["ext"]) == 1
        with netcdf_file(str(tmp_path / f"land_mask_tile{nl + 1}.nc"), mmap=False) as f:
            _same(f.variables["mask"][:], r["land"][nl]["mask"], "land mask")
            _same(f.variables["l_area"][:], r["land"][nl]["l_area"], "l_area")
            assert "area_atm" not in f.variables
    with netcdf_file(str(tmp_path / "ocean_mask.nc"), mmap=False) as f:
        _same(f.variables["mask"][:], r["ocean"]["mask"][c["ext"]:], "ocean mask")


def test_order_2_is_the_argument_error(fg, gpu_ok):
    c = cg.same_c5(fg)
    with pytest.raises(fg.FregridHipError, match="interp_order = 1") as e:
        _mosaic(fg, c, interp_order=2)
    assert e.value.code == -1                                   # FG_ERR_ARG, :593
    with pytest.raises(fg.FregridHipError, match="below 1e-6"):
        _mosaic(fg, c, area_ratio_thresh=1e-8)
    with pytest.raises(ValueError):
        fg.CouplerMosaic([_cfg(fg, g) for g in c["atm"]], None, _cfg(fg, c["ocn"]), c["omask"], interp_order=1, clip_method="planar")


def test_legacy_handle_before_and_after_a_great_circle_run(fg, gpu_ok):
    """a great-circle run sets no longitude frame and leaves none behind: the legacy pipeline on the same process gives the bits it
    gave before (the sibling of test_run_leaves_the_process_wide_search_frame_alone)"""
    lc = cc.case_c(fg, 0.5)

    def legacy():
        with fg.CouplerMosaic(lc["atm"], None, lc["ocn"], lc["omask"], interp_order=2) as m:
            m.run()
            return [m.axo(t)["area"] for t in range(6)] + [m.axl(t, t)["area"] for t in range(6)] + [m.cells(m.OCN)["xarea"]]

    before = legacy()
    c, r = cg.reference_of("same_c5", fg, pc.prims_oracle(True))
    with _mosaic(fg, c) as m:
        m.run()
    after = legacy()
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(before, after))
    to, ta = fg.tripolar_corners(20, 12)                         # ... and a plain plan on a grid whose areas depend on the frame
    p = fg.XgridPlan.create(2, lc["atm"], fg.GridConfig(20, 12, to, ta))
    q_area = p.get_xgrid()["area"]
    p.destroy()
    with _mosaic(fg, c) as m:
        m.run()
    p = fg.XgridPlan.create(2, lc["atm"], fg.GridConfig(20, 12, to, ta))
    assert np.array_equal(_bits(q_area), _bits(p.get_xgrid()["area"]))
    p.destroy()
