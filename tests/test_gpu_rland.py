"""remap_land's nearest-point search on the device against the reference's fixtures (tests/golden/rland_*.npz,
tests/rland_cases.py): idx_map, face_map and idx_map_sf bit for bit in both prune modes, the routes each case is for, the tile
edges against the host build, and the interface's corners."""
import numpy as np
import pytest

import rland_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixtures(fg, gpu_ok):
    return {name: rc.load(name) for name in rc.CASES}


@pytest.fixture(scope="module")
def host(fixtures, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rland_host")
    return {name: rc.hostcheck(tmp, fx) for name, fx in fixtures.items()}


@pytest.fixture(autouse=True)
def _default_prune(fg):
    yield
    fg.set_rland_prune(1)


def _both(h, fx):
    """(idx_map, face_map, idx_map_sf, stats of the search, stats of the same-face search)"""
    idx, fmap = h.search(fx["mask_src"], fx["lon_dst"], fx["lat_dst"], fx["mask_dst"])
    st = h.stats()
    sf = h.search_sface(fx["mask_src"], fx["lon_dst"], fx["lat_dst"], fx["mask_dst"], idx, fmap, int(fx["iface_dst"]))
    return idx, fmap, sf, st, h.stats()


@pytest.mark.parametrize("prune", [1, 0])
@pytest.mark.parametrize("name", rc.CASES)
def test_maps_equal_the_reference(fg, fixtures, host, name, prune):
    fx = fixtures[name]
    fg.set_rland_prune(prune)
    with fg.LandNearest(fx["lon_src"], fx["lat_src"]) as h:
        idx, fmap, sf, st, st_sf = _both(h, fx)
    assert np.array_equal(idx, fx["idx_map"]) and np.array_equal(fmap, fx["face_map"]) and np.array_equal(sf, fx["idx_map_sf"])
    on = fx["mask_dst"] != 0
    nsrc = int((fx["mask_src"] != 0).sum())
    assert st["queries"] == int(on.sum()) and st["tiles"] == -(-nsrc // fg.rland_tile())
    assert st_sf["queries"] == int((on & (fx["face_map"] != fx["iface_dst"])).sum())
    if not prune:
        assert st["tiles_visited"] == st["queries"] * st["tiles"] and st["tiles_visited_survivors"] == st["queries"] * st["tiles"]
        assert st_sf["tiles_visited"] == st_sf["queries"] * st_sf["tiles"]
    # the routes are the host build's, which finds the survivors by brute force
    assert st["fallback"] + st_sf["fallback"] == host[name]["fallback"]
    assert st["host_finished"] + st_sf["host_finished"] == host[name]["several"]
    assert st["survivors"] >= st["queries"] - st["fallback"] and st["overflow"] <= st["host_finished"]
    if name == "latlon_ties":
        assert st["overflow"] == 2 and st["survivors"] >= 48          # the two poles: a whole row of 24 each
    if name == "one_source_point":
        assert st["fallback"] > 10 and st["fallback"] < st["queries"]
    if name == "cube_small":
        assert st["fallback"] == 0 and st["overflow"] == 0


def test_tile_edges_pruned_equals_brute_force_equals_host_build(fg, gpu_ok, tmp_path):
    """unmasked source counts 1, T-1, T, T+1, 2T+1 and 64T+1 (one past a full ballot step) on 1200 points in three faces; 173
    queries over the whole sphere, no multiple of the four queries of a block.  Then (64 * 64 + 64) T + 1 of 66900 points: one
    tile past 65 groups, so the walk's group ballot runs a second time, over one full group and one group of a single one-point
    tile."""
    T = fg.rland_tile()
    big = (64 * 64 + 64) * T + 1
    assert 64 * T + 1 < 1200 and big < 66900
    qlon, qlat = rc.sphere_points(173, 0.7)
    for nsrc, n in [(k, 1200) for k in (1, T - 1, T, T + 1, 2 * T + 1, 64 * T + 1)] + [(big, 66900)]:
        lon, lat, mask = rc.thinned_source(nsrc, n=n)
        c = dict(lon_src=lon, lat_src=lat, mask_src=mask, lon_dst=qlon, lat_dst=qlat, mask_dst=np.ones(173, dtype=np.int32), iface_dst=-1)
        ref = rc.hostcheck(tmp_path, c)
        got = {}
        with fg.LandNearest(lon, lat) as h:
            for prune in (1, 0):
                fg.set_rland_prune(prune)
                got[prune] = h.search(mask, qlon, qlat, c["mask_dst"])
                st = h.stats()
                assert st["tiles"] == -(-nsrc // T) and st["fallback"] == ref["fallback"], (nsrc, prune, st)
                if prune:
                    assert st["tiles_visited_survivors"] <= st["queries"] * st["tiles"]
                if prune and nsrc == big:
                    assert st["tiles"] > 64 * 64 and st["tiles_visited"] < st["queries"] * st["tiles"], st
        for prune in (1, 0):
            assert np.array_equal(got[prune][0], ref["idx_map"]) and np.array_equal(got[prune][1], ref["face_map"]), (nsrc, prune)
        assert np.all(mask[got[1][1], got[1][0]] != 0)


@pytest.mark.parametrize("nq", [1, 2, 3, 5, 63])
def test_query_counts_off_the_block_size(fg, fixtures, nq):
    fx = fixtures["cube_small"]
    keep = np.flatnonzero(fx["mask_dst"])[:nq]
    mask_dst = np.zeros_like(fx["mask_dst"])
    mask_dst[keep] = 1
    for prune in (1, 0):
        fg.set_rland_prune(prune)
        with fg.LandNearest(fx["lon_src"], fx["lat_src"]) as h:
            idx, fmap = h.search(fx["mask_src"], fx["lon_dst"], fx["lat_dst"], mask_dst)
            assert h.stats()["queries"] == nq
        assert np.array_equal(idx[keep], fx["idx_map"][keep]) and np.array_equal(fmap[keep], fx["face_map"][keep])
        off = mask_dst == 0
        assert np.all(idx[off] == -1) and np.all(fmap[off] == -1)


def test_one_face_search_equals_all_faces_on_a_mask_zeroed_elsewhere(fg, fixtures):
    fx = fixtures["cube_small"]
    with fg.LandNearest(fx["lon_src"], fx["lat_src"]) as h:
        for face in range(6):
            only = np.zeros_like(fx["mask_src"])
            only[face] = fx["mask_src"][face]
            a = h.search(fx["mask_src"], fx["lon_dst"], fx["lat_dst"], fx["mask_dst"], face=face)
            b = h.search(only, fx["lon_dst"], fx["lat_dst"], fx["mask_dst"])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert np.all(a[1][fx["mask_dst"] != 0] == face)
        sf = h.search(fx["mask_src"], fx["lon_dst"], fx["lat_dst"], fx["mask_dst"], face=int(fx["iface_dst"]))[0]
    assert np.array_equal(sf, fx["idx_map_sf"])             # the same-face search is the one-face search where it does not copy


def test_empty_source_mask_is_the_reference_error(fg, fixtures):
    fx = fixtures["cube_small"]
    none = np.zeros_like(fx["mask_src"])
    with fg.LandNearest(fx["lon_src"], fx["lat_src"]) as h:
        with pytest.raises(fg.FregridHipError) as e:
            h.search(none, fx["lon_dst"], fx["lat_dst"], fx["mask_dst"])
        assert e.value.code == -1 and "no nearest point is found" in str(e.value)
        # no destination point unmasked: nothing to find, no error
        idx, fmap = h.search(none, fx["lon_dst"], fx["lat_dst"], np.zeros_like(fx["mask_dst"]))
        assert np.all(idx == -1) and np.all(fmap == -1)
        # the same-face search: the error only if a query needs the search
        only0 = np.zeros_like(fx["mask_src"])
        only0[0] = 1
        idx, fmap = h.search(only0, fx["lon_dst"], fx["lat_dst"], fx["mask_dst"])
        assert np.all(fmap[fx["mask_dst"] != 0] == 0)
        sf = h.search_sface(only0, fx["lon_dst"], fx["lat_dst"], fx["mask_dst"], idx, fmap, 0)
        assert np.array_equal(sf, idx) and h.stats()["queries"] == 0
        with pytest.raises(fg.FregridHipError) as e:
            h.search_sface(only0, fx["lon_dst"], fx["lat_dst"], fx["mask_dst"], idx, fmap, 1)
        assert e.value.code == -1 and "no nearest point is found" in str(e.value)
        with pytest.raises(fg.FregridHipError):
            h.search(fx["mask_src"], fx["lon_dst"], fx["lat_dst"], fx["mask_dst"], face=6)


def test_torch_device_tensors_equal_numpy(fg, fixtures):
    import torch
    fx = fixtures["frames"]
    lon, lat = torch.from_numpy(fx["lon_dst"].copy()).cuda(), torch.from_numpy(fx["lat_dst"].copy()).cuda()
    with fg.LandNearest(fx["lon_src"], fx["lat_src"]) as h:
        idx, fmap = h.search(fx["mask_src"], lon, lat, fx["mask_dst"])
        sf = h.search_sface(fx["mask_src"], lon, lat, fx["mask_dst"], idx, fmap, int(fx["iface_dst"]))
    assert np.array_equal(idx, fx["idx_map"]) and np.array_equal(fmap, fx["face_map"]) and np.array_equal(sf, fx["idx_map_sf"])
