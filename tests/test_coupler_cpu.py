"""The host side of the coupler pipeline without a GPU: coupler_ocean_grid against a direct transcription of
make_coupler_mosaic.c:841-876, the teeth of the restatement in tests/coupler_cases.py (the arbiter of tests/test_gpu_coupler_mosaic.py),
and a scipy round trip of the three kinds of file written from the restatement's arrays."""
import numpy as np
import pytest

import os

import coupler_cases as cc
import orc

needs_ref = pytest.mark.skipif(not orc.ref_available(), reason="needs oracle/_ref (the reference compiled in place)")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _transcribed_ocean_grid(tmpx, tmpy, nxo, nyo):
    """:841-876 with the reference's loops and names; tmpx, tmpy flat [(nyo+1)*(nxo+1)] in degrees"""
    D2R, TINY_VALUE = np.pi / 180, 1.e-7
    ocn_south_ext = 0
    min_atm_lat = -90. * D2R
    if tmpy[0] * D2R > min_atm_lat + TINY_VALUE:
        ocn_south_ext = 1
    nyo_old = nyo
    nyo += ocn_south_ext
    xocn, yocn = np.full((nxo + 1) * (nyo + 1), np.nan), np.full((nxo + 1) * (nyo + 1), np.nan)
    for j in range(nyo_old + 1):
        for i in range(nxo + 1):
            xocn[(j + ocn_south_ext) * (nxo + 1) + i] = tmpx[j * (nxo + 1) + i] * D2R
            yocn[(j + ocn_south_ext) * (nxo + 1) + i] = tmpy[j * (nxo + 1) + i] * D2R
    if ocn_south_ext == 1:
        for i in range(nxo + 1):
            xocn[i] = xocn[nxo + 1 + i]
            yocn[i] = min_atm_lat
    return ocn_south_ext, nyo, xocn, yocn


@pytest.mark.parametrize("south", [-82.0, -90.0, -90.0 + 1e-5, -90.0 + 1e-9])
def test_coupler_ocean_grid_is_the_references_preparation(fg, south):
    nx, ny = 7, 5
    x = np.linspace(-280.0, 80.0, nx + 1)[None, :] + 0.3 * np.arange(ny + 1)[:, None]
    y = np.linspace(south, 65.0, ny + 1)[:, None] + np.zeros((1, nx + 1))
    om = np.random.default_rng(3).random((ny, nx))
    g = fg.coupler_ocean_grid(x, y, om)
    ext, nyo, xo, yo = _transcribed_ocean_grid(x.reshape(-1), y.reshape(-1), nx, ny)
    assert ext == (1 if south > -90.0 + 1e-6 else 0)
    assert (g["ocn_south_ext"], g["ny"], g["nx"], g["jo_shift"]) == (ext, nyo, nx, 1 - ext)
    assert g["x"].shape == g["y"].shape == (nyo + 1, nx + 1)
    assert np.array_equal(_bits(g["x"]).reshape(-1), _bits(xo)) and np.array_equal(_bits(g["y"]).reshape(-1), _bits(yo))
    assert g["omask"].shape == (nyo, nx) and np.array_equal(g["omask"][ext:], om) and not g["omask"][:ext].any()        # :940, :946
    assert g["uniform"]
    with pytest.raises(ValueError, match="grid size mismatch"):
        fg.coupler_ocean_grid(x, y, om[1:])


def test_package_exports_the_pipeline(fg):
    assert fg.CouplerMosaic is fg.coupler.CouplerMosaic and "CouplerMosaic" in fg.__all__ and "coupler_ocean_grid" in fg.__all__
    for s in ("fg_coupler_write", "fg_coupler_write_xgrid", "fg_coupler_write_mask", "fg_coupler_create", "fg_coupler_run", "fg_coupler_count", "fg_coupler_get", "fg_coupler_get_cells", "fg_coupler_stats",
              "fg_coupler_phase_ms", "fg_coupler_stream", "fg_coupler_destroy"):
        assert s in fg._lib.EXPORTS and hasattr(fg.lib(), s), s


@needs_ref
def test_restatement_has_teeth_summation_order(fg):
    """every cell's terms added in reversed order: at least one o_clon of case A changes bits"""
    _, r = cc.reference_of("a", fg, 2)
    _, w = cc.reference_of("a", fg, 2, reverse_sums=True)
    for na in range(6):                                          # the lists themselves do not depend on the sums
        assert np.array_equal(_bits(r["axo"][na]["area"]), _bits(w["axo"][na]["area"]))
    assert np.count_nonzero(_bits(r["ocean"]["o_clon"]) != _bits(w["ocean"]["o_clon"])) >= 1
    assert np.allclose(r["ocean"]["o_clon"], w["ocean"]["o_clon"], rtol=1e-12, atol=0)


@needs_ref
def test_restatement_has_teeth_same_grid_copy(fg):
    """without the vertex copy of :1463-1477 every atmosphere cell is clipped against every land (= atmosphere) cell: the list changes"""
    _, r = cc.reference_of("a", fg, 2)
    _, w = cc.reference_of("a", fg, 2, skip_same_copy=True)
    same = all(r["axl"][na][nl]["area"].size == w["axl"][na][nl]["area"].size and
               np.array_equal(_bits(r["axl"][na][nl]["area"]), _bits(w["axl"][na][nl]["area"])) and
               np.array_equal(r["axl"][na][nl]["il"], w["axl"][na][nl]["il"]) for na in range(6) for nl in range(6))
    assert not same


@needs_ref
def test_restatement_coverage(fg):
    """what the GPU cases rely on, checked where no GPU is needed"""
    _, a = cc.reference_of("a", fg, 2)
    assert sum(t["area"].size for t in a["axo"]) > 1000 and sum(t["area"].size for row in a["axl"] for t in row) >= 100
    assert a["cover"]["atm_without_axl"] >= 10 and a["cover"]["poly5"] >= 1 and a["nbad"] == 0
    # land on the atmosphere grid: sea and land shares of every atmosphere cell add up to the cell (rejections: ~1e-6 each)
    assert max(np.max(np.abs(t["a_area"] / t["area"] - 1)) for t in a["atmos"]) < 1e-3
    _, b = cc.reference_of("b", fg, 2)
    assert sum(t["area"].size for row in b["axl"] for t in row) > 300 and sum(t["area"].size for t in b["lxo"]) > 300
    assert b["cover"]["dropped"] >= 20
    _, b1 = cc.reference_of("b", fg, 1)
    for k in ("ia", "ja", "il", "jl"):
        assert np.array_equal(b["axl"][2][0][k], b1["axl"][2][0][k])


@needs_ref
def test_files_round_trip_through_scipy(fg, tmp_path):
    from scipy.io import netcdf_file
    c, r = cc.reference_of("a", fg, 2)
    shift = fg.coupler_ocean_grid(np.zeros((2, 2)), np.array([[-82.0, -82.0], [0.0, 0.0]]))["jo_shift"]
    assert shift == 0
    t = r["axo"][2]
    p = str(tmp_path / "axo.nc")
    fg.coupler.write_xgrid_file(p, "atmos_mosaic:tile3::ocean_mosaic:tile1", t["ia"], t["ja"], t["io"], t["jo"], t["area"], (t["di1"], t["dj1"]),
                                (t["di2"], t["dj2"]), j2_shift=shift)
    with netcdf_file(p, mmap=False) as f:
        assert f.dimensions == {"string": 255, "ncells": t["area"].size, "two": 2}
        v = f.variables["contact"]
        assert v[:].tobytes().rstrip(b"\0") == b"atmos_mosaic:tile3::ocean_mosaic:tile1"
        assert (v.standard_name, v.contact_type, v.parent1_cell, v.parent2_cell, v.xgrid_area_field, v.distant_to_parent1_centroid,
                v.distant_to_parent2_centroid) == (b"grid_contact_spec", b"exchange", b"tile1_cell", b"tile2_cell", b"xgrid_area", b"tile1_distance",
                                                   b"tile2_distance")
        assert f.variables["tile1_cell"].standard_name == b"parent_cell_indices_in_mosaic1"
        assert np.array_equal(f.variables["tile1_cell"][:], np.stack([t["ia"] + 1, t["ja"] + 1], axis=1))
        assert np.array_equal(f.variables["tile2_cell"][:], np.stack([t["io"] + 1, t["jo"]], axis=1))           # jo + 1 - ocn_south_ext
        assert f.variables["xgrid_area"].units == b"m2" and np.array_equal(_bits(f.variables["xgrid_area"][:].astype(np.float64)), _bits(t["area"]))
        assert np.array_equal(_bits(f.variables["tile1_distance"][:].astype(np.float64)), _bits(np.stack([t["di1"], t["dj1"]], axis=1)))
        assert np.array_equal(_bits(f.variables["tile2_distance"][:].astype(np.float64)), _bits(np.stack([t["di2"], t["dj2"]], axis=1)))
    p1 = str(tmp_path / "axo1.nc")                                # order 1: no distances, five attributes
    fg.coupler.write_xgrid_file(p1, "a:tile1::o:tile1", t["ia"], t["ja"], t["io"], t["jo"], t["area"])
    with netcdf_file(p1, mmap=False) as f:
        assert "tile1_distance" not in f.variables and not hasattr(f.variables["contact"], "distant_to_parent1_centroid")
        assert np.array_equal(f.variables["tile2_cell"][:, 1], t["jo"] + 1)
    po = str(tmp_path / "ocean_mask.nc")
    fg.coupler.write_mask_file(po, "ocean", {k: r["ocean"][k] for k in ("mask", "areaO", "areaX")})
    with netcdf_file(po, mmap=False) as f:
        assert f.dimensions == {"nx": 40, "ny": 24} and f.variables["mask"].standard_name == b"ocean fraction at T-cell centers"
        for k in ("mask", "areaO", "areaX"):
            assert np.array_equal(_bits(f.variables[k][:].astype(np.float64)), _bits(r["ocean"][k]))
    pl = str(tmp_path / "land_mask.nc")
    land = r["land"][4]
    fg.coupler.write_mask_file(pl, "land", dict(mask=land["mask"], area_lnd=land["area_lnd"], l_area=land["l_area"]))
    with netcdf_file(pl, mmap=False) as f:
        assert set(f.variables) == {"mask", "area_lnd", "l_area"} and f.variables["l_area"].standard_name == b"land x area"
        assert np.array_equal(_bits(f.variables["mask"][:].astype(np.float64)), _bits(land["mask"]))
    with pytest.raises(fg.FregridHipError, match="empty list"):
        fg.coupler.write_xgrid_file(str(tmp_path / "e.nc"), "x", [], [], [], [], [])


@needs_ref
@pytest.mark.parametrize("name", ["c0", "c1"])
def test_restatement_gives_the_recorded_case_c(fg, name):
    """tests/golden/coupler_c*.npz (make_golden_coupler.py): the restatement's lists, sums and masks of case C as recorded"""
    import importlib.util
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_golden_coupler", os.path.join(here, "make_golden_coupler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    _, r = cc.reference_of(name, fg, 2)
    got, want = mod.flatten(r), np.load(os.path.join(here, f"coupler_{name}.npz"))
    assert set(got) == set(want.files)
    for k in want.files:
        a, b = np.asarray(got[k]), want[k]
        assert a.shape == b.shape, k
        if b.dtype.kind == "f" and orc.host_has_fma():
            assert np.array_equal(_bits(a), _bits(b)), k
        elif b.dtype.kind == "f":
            assert np.all(np.abs(a - b) <= 1e-10 * (np.max(np.abs(b)) if b.size else 0.0)), k
        else:
            assert np.array_equal(a, b), k
