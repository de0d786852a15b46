"""river_regrid's fixtures (tests/golden/river_*.npz, tests/river_cases.py) without a device: the reference's driver rebuilt
where its sources exist reproduces every file bit for bit, the numpy mirrors of the tool's grid preparation give the recorded
inputs, the host basin sort gives the recorded ids, and the host build of csrc/river.h gives the recorded max subA both as the
literal loop and as the pruned replay."""
import os

import numpy as np
import pytest

import river_cases as rv


@pytest.fixture(scope="module")
def fixtures():
    return {name: rv.load(name) for name in rv.CASES}


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    if not os.path.exists(os.path.join(rv.REF, "tools", "river_regrid", "river_regrid.c")):
        pytest.skip("the reference's sources are not on this machine")
    return rv.build_driver(str(tmp_path_factory.mktemp("river_ref")))


@pytest.mark.parametrize("name", rv.CASES)
def test_reference_driver_reproduces_the_fixture(fixtures, ref_exe, tmp_path, name):
    fx = fixtures[name]
    r = rv.run_ref(ref_exe, str(tmp_path), fx)
    for k in rv.OUTPUTS_D:
        assert np.array_equal(r[k].view(np.int64), fx[k].view(np.int64)), k
    for k in rv.OUTPUTS_I + rv.COUNTS:
        assert np.array_equal(r[k], fx[k]), k


@pytest.mark.parametrize("name", rv.CASES)
def test_generated_inputs_equal_the_recorded_ones(fg, fixtures, name):
    fx = fixtures[name]
    sg = fg.river_source_grid(fx["src_xt"], fx["src_yt"])
    assert np.array_equal(sg["xb_r"], fx["src_xb_r"]) and np.array_equal(sg["yb_r"], fx["src_yb_r"])
    assert sg["xb"][0] == 0 and sg["xb"][-1] == 360 and sg["yb"][0] == -90 and sg["yb"][-1] == 90
    assert np.array_equal(fg.river_land_frac(fx["landfrac_raw"], rv.LAND_THRESH, rv.MIN_FRAC), fx["landfrac"])
    # (land and subA come from numpy's trigonometry and the cube from the reference's generator: they are read, never rebuilt)
    xt, yt = rv.source_grid(fx["src_subA"].shape[1], fx["src_subA"].shape[0])
    assert np.array_equal(xt, fx["src_xt"]) and np.array_equal(yt, fx["src_yt"])


def test_source_grid_and_land_frac_errors(fg):
    xt, yt = rv.source_grid(72, 36)
    with pytest.raises(ValueError, match="starting longitude of grid bound is not 0"):
        fg.river_source_grid(xt + 1, yt)
    with pytest.raises(ValueError, match="ending latitude of grid bound is not 90"):
        fg.river_source_grid(xt, np.concatenate([yt[:-1], [yt[-1] - 1]]))
    with pytest.raises(ValueError, match=r"land_frac > 1 \+ 1.e-3"):
        fg.river_land_frac([0.5, 1.01])
    with pytest.raises(ValueError, match="land_frac should be between 0 or 1"):
        fg.river_land_frac([0.5, -0.2])
    f = fg.river_land_frac([0.99995, 0.05, 0.5, 1.0005], 1.e-4, 0.1)
    assert np.array_equal(f, [1, 0, 0.5, 1])


@pytest.mark.parametrize("name", rv.CASES)
def test_host_basin_sort_gives_the_recorded_ids(fg, fixtures, name):
    fx = fixtures[name]
    got = fg.river_sort_basin(fx["basin_presort"], fx["last_point"], fx["subA"], int(fx["missing"][3]))
    assert np.array_equal(got.reshape(fx["basin"].shape), fx["basin"])
    if name in ("latlon_shift", "latlon_aligned"):                      # the order among equal values is what is pinned here
        assert rv.features(fx, fx)["tie_outlets"] >= 10
        last, pre = fx["last_point"].reshape(-1) != 0, fx["basin_presort"].reshape(-1)
        maxsuba = np.empty(pre.max())
        maxsuba[pre[last] - 1] = fx["subA"].reshape(-1)[last]
        rank = np.empty(maxsuba.size, dtype=np.int64)
        rank[np.argsort(maxsuba, kind="stable")] = np.arange(maxsuba.size)
        stable = np.where(pre != int(fx["missing"][3]), maxsuba.size - rank[np.maximum(pre, 1) - 1], pre)
        assert not np.array_equal(stable, fx["basin"].reshape(-1)), "a stable sort gives the same ids: the ties do not bite"


def test_qsort_index_on_the_reference_example(fg):
    # the example in the reference's own test block (:247-251)
    a, idx = fg.river_qsort_index([12, 5, 18, 25, 14, 4, 11])
    assert np.array_equal(a, [4, 5, 11, 12, 14, 18, 25]) and np.array_equal(np.array([12, 5, 18, 25, 14, 4, 11])[idx], a)
    a, idx = fg.river_qsort_index(np.ones(20001))                       # all equal: the reference's deepest recursion
    assert sorted(idx.tolist()) == list(range(20001))
    assert fg.river_qsort_index([])[1].size == 0


@pytest.mark.parametrize("name", rv.CASES)
def test_host_build_literal_and_pruned_equal_the_reference(fixtures, tmp_path, name):
    fx = fixtures[name]
    h = rv.hostcheck(tmp_path, fx)
    ref = fx["max_suba"][:, 1:-1, 1:-1]
    assert np.array_equal(h["literal"].view(np.int64), ref.view(np.int64))
    assert np.array_equal(h["pruned"].view(np.int64), ref.view(np.int64))
    full = int((fx["landfrac"] == 1).sum())
    assert h["visited_literal"] == full * fx["src_subA"].size and h["visited_pruned"] < h["visited_literal"] // 50
    if name == "missing_rows":
        assert rv.features(fx, fx)["empty"] >= 1
