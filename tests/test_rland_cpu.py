"""remap_land's nearest-point search without a device: the survivor rule, the finish and the fallback scan of csrc/rland.h (a
host build, run as a stand-alone program, survivors by brute force) against the reference's idx_map / face_map / idx_map_sf in
every fixture; the fixtures against what they are for; and, where the reference's sources are present, the recipe again."""
import os
import tempfile

import numpy as np
import pytest

import rland_cases as rc


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rland_host")
    return {name: rc.hostcheck(tmp, rc.load(name)) for name in rc.CASES}


@pytest.mark.parametrize("name", rc.CASES)
def test_host_build_reproduces_reference_maps(name, host):
    fx = rc.load(name)
    for k in rc.OUTPUTS:
        assert np.array_equal(host[name][k], fx[k]), (name, k, np.flatnonzero(host[name][k] != fx[k]))


def test_host_build_takes_the_routes_the_cases_are_for(host):
    assert host["cube_small"]["fallback"] == 0
    assert host["latlon_ties"]["fallback"] == 1            # the south pole's same-face search: the northern half is 97.5 degrees away
    assert host["latlon_ties"]["several"] >= 5             # two poles, an edge, a corner, the equator; some again for the same face
    assert host["dup_points"]["several"] >= 4
    assert host["one_source_point"]["fallback"] > 0 and host["antipode_first"]["fallback"] > 0
    # a latitude beyond pi/2 in the source sends every query to the loop (25, and the 20 same-face searches); one in the query
    # sends that query (20 and their 20 same-face searches), and the five ordinary queries keep the survivor route
    assert host["beyond_pole_source"]["fallback"] == 45 and host["beyond_pole_query"]["fallback"] == 40


def _chord(c, q, l):
    """the true chord between query q and the source point with flat index l, from float64 trigonometry"""
    def xyz(lon, lat):
        return np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    return np.linalg.norm(xyz(c["lon_dst"][q], c["lat_dst"][q]) - xyz(c["lon_src"].ravel()[l], c["lat_src"].ravel()[l]))


def test_fixture_cases_hold_what_they_are_for():
    fx = rc.load("cube_small")
    on = fx["mask_dst"] != 0
    assert fx["lon_src"].shape == (6, 64) and on.sum() > 60 and 0 < (fx["face_map"][on] != fx["iface_dst"]).sum() < on.sum()
    assert 0.3 < fx["mask_src"].mean() < 0.5
    fx = rc.load("latlon_ties")
    n = fx["lon_src"].size
    for q, nties in ((0, 24), (1, 24), (2, 2), (4, 4), (5, 2)):          # poles, an edge, a corner at the equator, an edge across the faces
        ch = np.array([_chord(fx, q, l) for l in range(n)])
        ch[fx["mask_src"].ravel() == 0] = np.inf
        tied = np.flatnonzero(ch <= ch.min() + 2.0 ** -40)
        assert tied.size == nties, (q, tied)
        assert fx["face_map"][q] * 144 + fx["idx_map"][q] in tied
    assert fx["mask_dst"][7] == 0 and fx["idx_map"][7] == -1 and fx["face_map"][7] == -1 and fx["idx_map_sf"][7] == -1
    fx = rc.load("dup_points")
    ls, la = fx["lon_src"], fx["lat_src"]
    assert ls[1, 10] == ls[1, 40] and la[1, 10] == la[1, 40] and ls[4, 5] == ls[0, 20] and la[4, 5] == la[0, 20]
    assert (fx["face_map"][144], fx["idx_map"][144]) == (1, 10) and (fx["face_map"][145], fx["idx_map"][145]) == (0, 20)
    assert not ((fx["face_map"] == 1) & (fx["idx_map"] == 40)).any() and not ((fx["face_map"] == 4) & (fx["idx_map"] == 5)).any()
    fx = rc.load("frames")
    assert fx["lon_dst"].min() < -2.4263 and fx["lon_dst"].min() >= -300 * np.pi / 180 and fx["lon_src"].min() >= 0 and fx["lon_src"].max() > 2.4263
    small = rc.load("cube_small")
    assert np.array_equal(np.mod(fx["lon_dst"], 2 * np.pi).round(9), small["lon_dst"].round(9)) and np.array_equal(fx["mask_src"], small["mask_src"])
    fx = rc.load("one_source_point")
    assert fx["mask_src"].sum() == 1 and fx["mask_src"][1, 7] == 1 and np.all(fx["face_map"] == 1) and np.all(fx["idx_map"] == 7)
    far = np.array([_chord(fx, q, 57) for q in range(fx["lon_dst"].size)])
    assert (far > np.sqrt(2) + 1e-3).sum() > 10 and (far < np.sqrt(2) - 1e-3).sum() > 10 and far[61] > 2 - 1e-12 and far[62] == 0
    fx = rc.load("antipode_first")
    assert np.flatnonzero(fx["mask_src"].ravel())[0] == 3 and _chord(fx, 61, 3) > 2 - 1e-12 and fx["mask_src"].sum() == 41
    if int(fx["nan_first"]):
        assert (fx["face_map"][61], fx["idx_map"][61]) == (0, 3)
    else:                                                   # no NaN placement was found: the nearest point wins, the route is the flag's
        assert (fx["face_map"][61], fx["idx_map"][61]) != (0, 3)
    for name in ("beyond_pole_source", "beyond_pole_query"):
        fx = rc.load(name)
        half_pi = 1.5707963267948966                        # RL_LAT_MAX: the largest double whose cosine is still >= 0
        assert np.cos(half_pi) > 0 and np.cos(np.nextafter(half_pi, 2)) < 0
        assert fx["lat_dst"][:20].min() > half_pi and fx["lat_dst"][:20].max() < 1.6 and np.abs(fx["lat_dst"][20:]).max() < half_pi
        assert (np.abs(fx["lat_src"]).max() > half_pi) == (name == "beyond_pole_source")
        # the two candidates of query k are the flat indices 2k and 2k + 1, 1e-11 .. 1e-9.5 rad apart: further than the margin
        # of the survivor rule, so the chord alone would decide -- and the reference, whose h cancels there (negative, NaN, or
        # garbage of the size of the rounding), does not always agree
        assert np.all(fx["face_map"][:20] == 0)
        near = np.array([np.argmin([_chord(fx, q, l) for l in range(40)]) for q in range(20)])
        assert (fx["idx_map"][:20] != near).any(), "the case must hold a query where the nearest point by chord loses in the reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(rc.REF, "tools", "remap_land")), reason="the reference's sources are not present")
def test_recipe_regenerates_the_fixtures():
    with tempfile.TemporaryDirectory(prefix="rland_ref_") as tmp:
        exe = rc.build_driver(tmp)
        for name in rc.CASES:
            fx = rc.load(name)
            r = rc.run_ref(exe, tmp, fx)
            for k in rc.OUTPUTS:
                assert np.array_equal(r[k], fx[k]), (name, k)
