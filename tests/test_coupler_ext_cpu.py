"""The nest, wave and --check additions of the coupler pipeline without a GPU: the teeth of the restatement in
tests/coupler_ext_cases.py (the arbiter of tests/test_gpu_coupler_ext.py) and what the GPU cases rely on, a scipy round trip of the
wave files written from the restatement's arrays, and the new entries' exports and argument checks."""
import ctypes as C

import numpy as np
import pytest

import coupler_cases as cc
import coupler_ext_cases as ce
import orc

needs_ref = pytest.mark.skipif(not orc.ref_available(), reason="needs oracle/_ref (the reference compiled in place)")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _differ(a, b):
    return int(np.count_nonzero(_bits(a) != _bits(b)))


def test_new_symbols_are_exported_and_check_their_arguments_without_a_device(fg):
    L = fg.lib()
    for s in ("fg_coupler_set_nest", "fg_coupler_add_wave", "fg_coupler_get_wave_ocean", "fg_coupler_check", "fg_coupler_write_wave",
              "fg_coupler_write_wave_xgrid", "fg_coupler_write_wave_mask"):
        assert s in fg._lib.EXPORTS and hasattr(L, s), s
    assert fg.CouplerMosaic.WXO == 3 and fg.CouplerMosaic.WAV == 3
    buf = (C.c_double * 19)()
    one = (C.c_int * 1)(1)
    calls = (("fg_coupler_set_nest", lambda: L.fg_coupler_set_nest(None, 0)),
             ("fg_coupler_add_wave", lambda: L.fg_coupler_add_wave(None, 1, one, one, None, None, 0)),
             ("fg_coupler_get_wave_ocean", lambda: L.fg_coupler_get_wave_ocean(None, buf, None, None)),
             ("fg_coupler_check", lambda: L.fg_coupler_check(None, buf, 19)),
             ("fg_coupler_write_wave", lambda: L.fg_coupler_write_wave(None, b"/nowhere", None)),
             ("fg_coupler_write_wave_mask", lambda: L.fg_coupler_write_wave_mask(b"/nowhere/x.nc", 0, 1, buf)),
             ("fg_coupler_write_xgrid", lambda: L.fg_coupler_write_wave_xgrid(b"/nowhere/x.nc", b"w:tile1::o:tile1", 0, None, None, None, None, 1, None, None,
                                                                              None, None, None)))
    for who, call in calls:
        assert call() == -1, who                                  # FG_ERR_ARG
        assert who in fg._lib.last_error(), (who, fg._lib.last_error())


@needs_ref
def test_sums_without_a_nest_are_reference_couplers(fg):
    """coupler_sums over reference_coupler's lists with tile_nest = -1 gives that function's own numbers"""
    for order in (1, 2):
        c, r = cc.reference_of("b", fg, order)
        s = ce.with_nest(c, r, -1)
        assert s["nbad"] == r["nbad"]
        assert _differ(s["ocean"]["o_area"], r["ocean"]["o_area"]) == 0 and _differ(s["ocean"]["mask"], r["ocean"]["mask"]) == 0
        assert _differ(s["land"][0]["l_area"], r["land"][0]["l_area"]) == 0
        if order == 2:
            for na in range(6):
                for k in ("di1", "dj1", "di2", "dj2"):
                    assert _differ(s["axo"][na][k], r["axo"][na][k]) == 0 and _differ(s["axl"][na][0][k], r["axl"][na][0][k]) == 0
                assert _differ(s["atmos"][na]["a_clon"], r["atmos"][na]["a_clon"]) == 0


@needs_ref
@pytest.mark.parametrize("order", [1, 2])
def test_nest_restatement_has_teeth(fg, order):
    """case N without the exclusion changes bits of l_area, o_area and of a tile-2 distance"""
    c, r = ce.nest_reference(fg, order)
    _, w = ce.nest_reference(fg, order, no_exclusion=True)
    nest = r["axo"][6]["area"].size + r["axl"][6][0]["area"].size
    assert r["axo"][6]["area"].size > 20 and r["axl"][6][0]["area"].size > 20, nest          # the nest tile lies over land and over sea
    assert _differ(r["land"][0]["l_area"], w["land"][0]["l_area"]) >= 5
    assert _differ(r["ocean"]["o_area"], w["ocean"]["o_area"]) >= 5
    assert np.all(w["land"][0]["l_area"] >= r["land"][0]["l_area"])
    for na in range(7):                                          # the lists do not depend on the sums
        assert _differ(r["axo"][na]["area"], w["axo"][na]["area"]) == 0
    if order == 2:
        p = ce.NEST_PARENT
        assert _differ(r["axo"][p]["di2"], w["axo"][p]["di2"]) >= 1 and _differ(r["axl"][p][0]["dj2"], w["axl"][p][0]["dj2"]) >= 1
        assert _differ(r["axo"][p]["di1"], w["axo"][p]["di1"]) == 0          # tile-1 distances of another tile: untouched
        # :1857 / :1903 also keep the nest tile's own a_area at 0: its tile-1 distances are clon / area
        t = r["axo"][6]
        assert not r["atmos"][6]["a_area"].any() and _differ(t["di1"], t["clon"] / t["area"]) == 0
        assert _differ(t["di1"], w["axo"][6]["di1"]) >= 1
    # the parent's cells under the nest: with the exclusion the land and ocean cells are covered once, not twice
    assert r["nbad"] <= w["nbad"] and w["nbad"] >= 1
    ck = ce.check_of(c, r, tile_nest=6)
    assert ck["axo_area_sum_nest"] > 0 and ck["axl_area_sum_nest"] > 0 and abs(ck["tiling_area_nest"]) < 1.0 and abs(ck["tiling_area"]) < 1.0
    ck0 = ce.check_of(c, r, tile_nest=-1)                        # without a nest the seventh tile's areas count twice
    assert ck0["atm_area_sum"] > ck["atm_area_sum"] and "atm_area_sum_nest" not in ck0


@needs_ref
def test_nest_corners_keep_the_parents_bits(fg):
    c = ce.case_n(fg)
    p, n = c["atm"][ce.NEST_PARENT], c["atm"][6]
    plon, nlon = np.asarray(p.lonc).reshape(9, 9), np.asarray(n.lonc).reshape(7, 7)
    plat, nlat = np.asarray(p.latc).reshape(9, 9), np.asarray(n.latc).reshape(7, 7)
    sl = (slice(ce.NEST_J0, ce.NEST_J0 + 4), slice(ce.NEST_I0, ce.NEST_I0 + 4))
    assert _differ(nlon[::2, ::2], plon[sl]) == 0 and _differ(nlat[::2, ::2], plat[sl]) == 0
    assert np.all(np.diff(nlon, axis=1) > 0) and np.all(np.diff(nlat, axis=0) > 0)


@needs_ref
@pytest.mark.parametrize("order", [1, 2])
def test_wave_restatement_has_teeth(fg, order):
    c, _, w = ce.wave_reference("w1", fg, order)
    n = w["wxo"][0]["area"].size
    js, je = w["bands"][0]
    assert n > 300 and 0 < js and je < c["ocn"].ny - 1                        # the band is a proper subset of the ocean rows
    assert np.count_nonzero(w["mask"][0] == 0) >= 5 and np.count_nonzero(w["mask"][0] > 0.99) >= 5      # wave cells wholly over land / over sea
    t = w["wxo"][0]
    key = (t["jw"] * 24 + t["iw"]) * 10000 + t["jo"] * 36 + t["io"]
    assert np.all(np.diff(key) > 0)                                            # wave cell, then ocean cell, ascending
    # the band drops nothing on W1 (a search finds pairs outside it only in degenerate cases) ...
    _, _, nb = ce.wave_reference("w1", fg, order, skip_band=True)
    assert nb["wxo"][0]["area"].size == n
    # ... so the tile that shows it is WB's first: it lies over sea strictly inside one ocean row, and the band of :3107-3117 is empty
    cb, _, b = ce.wave_reference("wb", fg, order)
    _, _, bn = ce.wave_reference("wb", fg, order, skip_band=True)
    assert b["bands"][0] == (cb["ocn"].ny - 1, 0) and b["wxo"][0]["area"].size == 0 and bn["wxo"][0]["area"].size >= 10
    assert not b["mask"][0].any() and bn["mask"][0].any()
    assert b["wxo"][1]["area"].size == bn["wxo"][1]["area"].size > 20
    if order == 2:
        _, _, rv = ce.wave_reference("w1", fg, order, reverse_sums=True)
        assert _differ(w["wxo"][0]["area"], rv["wxo"][0]["area"]) == 0
        assert _differ(w["o_clon"], rv["o_clon"]) + _differ(w["w_clon"][0], rv["w_clon"][0]) + _differ(w["w_area"][0], rv["w_area"][0]) >= 1
        assert np.allclose(w["o_area"], rv["o_area"], rtol=1e-12, atol=0)            # sums of positive terms: the order moves the last bits only
        # the ocean cells' wave-side sums are their own: not the atmosphere side's o_area
        _, r = cc.reference_of("b", fg, 2)
        assert _differ(w["o_area"], r["ocean"]["o_area"]) > 100
    else:
        assert "o_area" not in w                                               # :3262-3267 cannot execute; w_area alone is formed
    assert ce.check_of(c, cc.reference_of("b", fg, order)[1], w=w)["wxo_area_sum"] > 0


@needs_ref
def test_wave_on_the_ocean_grid_and_without_sea(fg):
    c, _, w = ce.wave_reference("w2", fg, 2)
    t = w["wxo"][0]
    own = (t["iw"] == t["io"]) & (t["jw"] == t["jo"])
    sea = np.flatnonzero(c["omask"].reshape(-1) > cc.MIN_AREA_FRAC)
    assert np.count_nonzero(own) == sea.size                                   # every sea cell is clipped with itself
    assert np.array_equal((t["jw"] * 40 + t["iw"])[own], sea)
    c0, r0, w0 = ce.wave_reference("w0", fg, 2)
    assert w0["wxo"][0]["area"].size == 0 and not w0["mask"][0].any() and sum(x["area"].size for x in r0["axo"]) == 0


@needs_ref
def test_wave_files_round_trip_through_scipy(fg, tmp_path):
    from scipy.io import netcdf_file
    c, _, w = ce.wave_reference("w2", fg, 2)
    t = w["wxo"][0]
    p = str(tmp_path / "wav_ocean_mosaic_tile1Xocn_ocean_mosaic_tile1.nc")
    fg.coupler.write_wave_xgrid_file(p, "ocean_mosaic:tile1::ocean_mosaic:tile1", t["iw"], t["jw"], t["io"], t["jo"], t["area"], (t["di1"], t["dj1"]),
                                     (t["di2"], t["dj2"]), jo_shift=1 - c["ext"])
    with netcdf_file(p, mmap=False) as f:
        assert f.dimensions == {"string": 255, "ncells": t["area"].size, "two": 2}
        v = f.variables["contact"]
        assert v[:].tobytes().rstrip(b"\0") == b"ocean_mosaic:tile1::ocean_mosaic:tile1"
        assert (v.standard_name, v.contact_type, v.parent1_cell, v.parent2_cell, v.xgrid_area_field, v.distant_to_parent1_centroid,
                v.distant_to_parent2_centroid) == (b"grid_contact_spec", b"exchange", b"tile1_cell", b"tile2_cell", b"xgrid_area", b"tile1_distance",
                                                   b"tile2_distance")
        assert f.variables["tile1_cell"].standard_name == b"parent1_cell_indices" and f.variables["tile2_cell"].standard_name == b"parent2_cell_indices"
        assert np.array_equal(f.variables["tile1_cell"][:], np.stack([t["iw"] + 1, t["jw"] + 1], axis=1))          # 1-based
        assert np.array_equal(f.variables["tile2_cell"][:], np.stack([t["io"] + 1, t["jo"] + 1 - c["ext"]], axis=1))      # :3492
        assert f.variables["xgrid_area"].units == b"m2" and _differ(f.variables["xgrid_area"][:].astype(np.float64), t["area"]) == 0
        assert f.variables["tile1_distance"].standard_name == b"distance_from_parent1_cell_centroid"
        assert _differ(f.variables["tile1_distance"][:].astype(np.float64), np.stack([t["di1"], t["dj1"]], axis=1)) == 0
        assert _differ(f.variables["tile2_distance"][:].astype(np.float64), np.stack([t["di2"], t["dj2"]], axis=1)) == 0
    _, _, w1 = ce.wave_reference("w1", fg, 1)
    t = w1["wxo"][0]
    p1 = str(tmp_path / "wave_mosaic_tile1Xocean_mosaic_tile1.nc")
    fg.coupler.write_wave_xgrid_file(p1, "wave_mosaic:tile1::ocean_mosaic:tile1", t["iw"], t["jw"], t["io"], t["jo"], t["area"])
    with netcdf_file(p1, mmap=False) as f:                       # order 1: no distances, five attributes
        assert set(f.variables) == {"contact", "tile1_cell", "tile2_cell", "xgrid_area"} and not hasattr(f.variables["contact"], "distant_to_parent1_centroid")
        assert np.array_equal(f.variables["tile2_cell"][:, 1], t["jo"] + 1)
    pm = str(tmp_path / "wave_mask.nc")
    fg.coupler.write_wave_mask_file(pm, w1["mask"][0])
    with netcdf_file(pm, mmap=False) as f:
        assert f.dimensions == {"nx": 24, "ny": 14} and set(f.variables) == {"mask"}
        m = f.variables["mask"]
        assert m.standard_name == b"land/sea fraction at T-cell centers" and m.units == b"none" and _differ(m[:].astype(np.float64), w1["mask"][0]) == 0
    with pytest.raises(fg.FregridHipError, match="empty list"):
        fg.coupler.write_wave_xgrid_file(str(tmp_path / "e.nc"), "x", [], [], [], [], [])
