"""river_regrid on the device against the reference's fixtures (tests/golden/river_*.npz, tests/river_cases.py): max subA with
its halo, then subA, cellarea, celllength bit for bit and tocell, travel, basin equal, with check_river_data's counts, in both
prune modes; the pruned replay against the literal loop on a larger generated case; the reference's errors; two handles."""
import numpy as np
import pytest

import river_cases as rv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixtures(fg, gpu_ok):
    return {name: rv.load(name) for name in rv.CASES}


@pytest.fixture(autouse=True)
def _default_prune(fg):
    yield
    fg.set_river_prune(1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run_case(fg, fx):
    """-> (max_suba [ntiles, ny+2, nx+2], dict of fields [ntiles, ny, nx], stats)"""
    source, tiles, opcode, cutoff = rv.tiles_of(fx)
    with fg.RiverRegrid(source, tiles, opcode, suba_cutoff=cutoff) as h:
        h.run()
        ms = np.stack([h.max_suba(n) for n in range(h.ntiles)])
        per = [h.fields(n) for n in range(h.ntiles)]
        return ms, {k: np.stack([p[k] for p in per]) for k in per[0]}, h.stats()


def assert_equals_fixture(fx, ms, f, st):
    assert np.array_equal(bits(ms), bits(fx["max_suba"])), "max subA with halo"
    for k in ("subA", "cellarea", "celllength"):
        print(k, "cells that differ:", int((bits(f[k]) != bits(fx[k])).sum()))
        assert np.array_equal(bits(f[k]), bits(fx[k])), k
    for k in ("tocell", "travel", "basin"):
        assert np.array_equal(f[k], fx[k]), k
    for k in rv.COUNTS:
        assert st[k] == int(fx[k]), k


@pytest.mark.parametrize("prune", [1, 0])
@pytest.mark.parametrize("name", rv.CASES)
def test_every_output_equals_the_reference(fg, fixtures, name, prune):
    fx = fixtures[name]
    fg.set_river_prune(prune)
    ms, f, st = run_case(fg, fx)
    assert_equals_fixture(fx, ms, f, st)
    full, nsrc = int((fx["landfrac"] == 1).sum()), fx["src_subA"].size
    assert st["land_cells"] == full
    if prune:
        assert 0 < st["source_cells_visited"] < full * nsrc // 50
    else:
        assert st["source_cells_visited"] == full * nsrc
    # the travel levels cost one launch each, the rounds that find them do not grow with them
    assert st["launches"] <= int(fx["maxtravel"]) + 1 + 5 + int(np.ceil(np.log2(int(fx["maxtravel"]) + 2))) + 1


def test_pruned_equals_literal_replay_on_a_generated_c48(fg, gpu_ok):
    c = rv.generated_case(48, (360, 180))
    got = {}
    for prune in (1, 0):
        fg.set_river_prune(prune)
        got[prune] = run_case(fg, c)
    (ms1, f1, st1), (ms0, f0, st0) = got[1], got[0]
    assert np.array_equal(bits(ms1), bits(ms0))
    for k in f1:
        assert np.array_equal(bits(f1[k]) if f1[k].dtype == np.float64 else f1[k], bits(f0[k]) if f0[k].dtype == np.float64 else f0[k]), k
    full, nsrc = int((c["landfrac"] == 1).sum()), c["src_subA"].size
    assert full > 1000 and st1["land_cells"] == st0["land_cells"] == full
    assert st0["source_cells_visited"] == full * nsrc
    assert 0 < st1["source_cells_visited"] < full * nsrc // 100
    for k in rv.COUNTS:
        assert st1[k] == st0[k]
    assert st1["maxtravel"] >= 4 and st1["maxbasin"] > 100
    # cells whose corners straddle the date line are among the searched ones: the shifts are live
    lon = c["xb_r"]
    span = np.maximum.reduce([lon[:, :-1, :-1], lon[:, :-1, 1:], lon[:, 1:, 1:], lon[:, 1:, :-1]]) - \
        np.minimum.reduce([lon[:, :-1, :-1], lon[:, :-1, 1:], lon[:, 1:, 1:], lon[:, 1:, :-1]])
    assert int(((span > np.pi) & (c["landfrac"] == 1)).sum()) > 0


def _small(fixtures):
    return fixtures["regional"]


def test_argument_errors_carry_the_reference_text_and_leave_the_library_usable(fg, fixtures):
    fx = _small(fixtures)
    source, tiles, opcode, cutoff = rv.tiles_of(fx)

    def raises(text, source=source, tiles=tiles, opcode=opcode):
        with pytest.raises(fg.FregridHipError) as e:
            fg.RiverRegrid(source, tiles, opcode, suba_cutoff=cutoff)
        assert e.value.code == -1 and text in str(e.value), str(e.value)

    for bad in (1.5, -0.25):
        t = [dict(tiles[0], landfrac=tiles[0]["landfrac"].copy())]
        t[0]["landfrac"][3, 4] = bad
        raises("river_regrid: land_frac should be between 0 or 1", tiles=t)
    cut = {k: (v[:-1, :-1] if k in ("area", "landfrac", "xt", "yt", "xb_r", "yb_r") else v) for k, v in tiles[0].items()}
    raises("river_regrid: all the tiles should have the same grid size", tiles=[tiles[0], cut])
    raises("river_regrid: the mosaic must be a 6-tile cubic grid for 12 contacts.", opcode=4)
    for k in (1, 2, 3):
        for v in (0.0, 7.0):
            m = fx["missing"].copy()
            m[k] = v
            raises("must be negative integers", source=dict(source, missing=m))
    m = fx["missing"].copy()
    m[0] = -1.e20
    raises("does not fit the int", source=dict(source, missing=m))
    ms, f, st = run_case(fg, fx)
    assert_equals_fixture(fx, ms, f, st)


def test_a_fatal_check_of_the_reference_comes_back_as_an_error(fg, fixtures):
    """rv.funnel_case: the reference stops in check_river_data (seen with its driver); here the run raises with its text, the
    handle stays usable for its max subA, and the library for the next case"""
    c = rv.funnel_case()
    c["area"] = np.stack([fg.get_grid_area(20, 12, c["xb_r"][0], c["yb_r"][0]).reshape(12, 20)])
    source, tiles, opcode, cutoff = rv.tiles_of(c)
    with fg.RiverRegrid(source, tiles, opcode, suba_cutoff=cutoff) as h:
        with pytest.raises(fg.FregridHipError) as e:
            h.run()
        assert e.value.code == -1 and "river_regrid, subA, tocell, travel, or basin is missing value for some river points" in str(e.value)
        with pytest.raises(fg.FregridHipError):
            h.fields(0)
        ms = h.max_suba(0)
        assert ms[7, 11] == 1e20 and np.all(ms[1:-1, 1:-1] > 0)
    fx = _small(fixtures)
    assert_equals_fixture(fx, *run_case(fg, fx))


def test_two_handles_alive_at_once(fg, fixtures):
    a, b = fixtures["cube_c8_continent"], fixtures["latlon_shift"]
    sa, sb = rv.tiles_of(a), rv.tiles_of(b)
    with fg.RiverRegrid(sa[0], sa[1], sa[2], suba_cutoff=sa[3]) as ha, fg.RiverRegrid(sb[0], sb[1], sb[2], suba_cutoff=sb[3]) as hb:
        ha.run()
        hb.run()
        ha.run()                                                   # a handle may be run again
        for h, fx in ((hb, b), (ha, a)):
            ms = np.stack([h.max_suba(n) for n in range(h.ntiles)])
            per = [h.fields(n) for n in range(h.ntiles)]
            assert_equals_fixture(fx, ms, {k: np.stack([p[k] for p in per]) for k in per[0]}, h.stats())
