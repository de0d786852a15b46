"""runoff_regrid on the device against the reference's fixtures (tests/golden/runoff_*.npz, tests/runoff_cases.py): the
nearest-ocean maps bit for bit in both prune modes and at the tile edges, the converted points against the host build, and
process_data's arithmetic per time level."""
import numpy as np
import pytest

import runoff_cases as rc

pytestmark = pytest.mark.gpu
NX, NY = 40, 30


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fixtures(fg, gpu_ok):
    return {name: rc.load(name) for name in rc.CASES}


@pytest.fixture(autouse=True)
def _default_prune(fg):
    yield
    fg.set_runoff_prune(1)


def _xgrid(fx):
    return fx["i_in"], fx["j_in"], fx["i_out"], fx["j_out"], fx["xgrid_area"]


def _regular(mask):
    """a handle on the regular grid of the mask's shape with the given mask and an empty exchange list"""
    ny, nx = mask.shape
    x, y = np.meshgrid((np.arange(nx) + 0.5) * (2 * np.pi / nx), -np.pi / 2 + (np.arange(ny) + 0.5) * (np.pi / ny))
    gi = dict(nx=2, ny=2, mask=np.ones((2, 2)), area=np.ones((2, 2)))
    go = dict(nx=nx, ny=ny, xt=x, yt=y, mask=mask, area=np.ones((ny, nx)))
    e = np.zeros(0, dtype=np.int32)
    return gi, go, (e, e, e, e, np.zeros(0))


def _numpy_nearest(x, y, z, mask):
    """the lexicographic minimum of (r, index) over the ocean points with r < r0, in float64, the sums in the reference's order.
    r0 = distance(0, pi/2, 0, -pi/2) = sqrt((1 - -1)^2 + 0 + 0) = 2 whatever cos(pi/2) rounds to: both points have the same x, y."""
    x, y, z, m = x.ravel(), y.ravel(), z.ravel(), mask.ravel()
    oc = np.flatnonzero(m != 0)
    imap, jmap = np.full(m.size, -1, dtype=np.int32), np.full(m.size, -1, dtype=np.int32)
    for q in np.flatnonzero(m == 0):
        dz, dx, dy = z[q] - z[oc], x[q] - x[oc], y[q] - y[oc]
        r = np.sqrt((dz * dz + dx * dx) + dy * dy)
        k = int(np.argmin(r))                                   # the first occurrence of the minimum
        if r[k] < 2.0:
            imap[q], jmap[q] = oc[k] % mask.shape[1], oc[k] // mask.shape[1]
    return imap.reshape(mask.shape), jmap.reshape(mask.shape)


@pytest.mark.parametrize("prune", [1, 0])
@pytest.mark.parametrize("name", rc.CASES)
def test_maps_equal_the_reference(fg, fixtures, name, prune):
    fx, gi, go = fixtures[name]
    fg.set_runoff_prune(prune)
    with fg.RunoffRegrid(gi, go, xgrid=_xgrid(fx)) as h:
        imap, jmap = h.maps()
        st = h.search_stats()
    assert np.array_equal(imap, fx["imap"]) and np.array_equal(jmap, fx["jmap"])
    assert st["queries"] == int((go["mask"] == 0).sum())
    if not prune:
        assert st["tiles_visited"] == st["queries"] * st["tiles"]


def test_tile_edges_pruned_equals_brute_force_equals_numpy(fg, gpu_ok):
    """ocean counts 1, T-1, T, T+1, 2T+1 and 64T+1 (one past a full ballot step) on 1200 cells; the land counts 1199, 1185, 1183,
    1167 and 175 are no multiples of the four queries of a block, 1184 is.  Then (64 * 64 + 64) T + 1 ocean cells of 300 x 223:
    one tile past 65 groups, so the walk's group ballot runs a second time, over one full group and one group of a single
    one-point tile; 339 land queries at T = 16."""
    T = fg.runoff_tile()
    big = (64 * 64 + 64) * T + 1
    assert 64 * T + 1 < NX * NY and big < 300 * 223
    for nocean, nx, ny in [(k, NX, NY) for k in (1, T - 1, T, T + 1, 2 * T + 1, 64 * T + 1)] + [(big, 300, 223)]:
        mask = rc.thinned_mask(nocean, nx, ny)
        gi, go, xg = _regular(mask)
        got = {}
        for prune in (1, 0):
            fg.set_runoff_prune(prune)
            with fg.RunoffRegrid(gi, go, xgrid=xg) as h:
                got[prune] = h.maps()
                xyz = h.xyz()
                st = h.search_stats()
                assert st["tiles"] == -(-nocean // T)
                if prune and nocean == big:
                    assert st["tiles"] > 64 * 64 and st["tiles_visited"] < st["queries"] * st["tiles"], st
        assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][1], got[0][1]), nocean
        ref = _numpy_nearest(*xyz, mask)
        assert np.array_equal(got[1][0], ref[0]) and np.array_equal(got[1][1], ref[1]), nocean
        assert np.all(got[1][0][mask == 0] >= 0) and np.all(got[1][0][mask != 0] == -1)


def test_xyz_equals_the_host_build_bit_for_bit(fg, fixtures, tmp_path):
    fx, gi, go = fixtures["tripolar_small"]
    assert go["xt"].min() < -2.4263                         # the -300..60 frame: beyond the hand-over on the negative side ...
    host = rc.hostcheck_nearest(tmp_path, go["mask"], go["xt"], go["yt"])[2:]
    with fg.RunoffRegrid(gi, go, xgrid=_xgrid(fx)) as h:
        dev = h.xyz()
    for d, s in zip(dev, host):
        assert np.array_equal(_bits(d), _bits(s))
    # ... and the same points one turn on: longitudes beyond it on the positive side
    go2 = dict(go, xt=go["xt"] + 2 * np.pi)
    assert go2["xt"].max() > 2.4263
    host = rc.hostcheck_nearest(tmp_path, go["mask"], go2["xt"], go["yt"])[2:]
    with fg.RunoffRegrid(gi, go2, xgrid=_xgrid(fx)) as h:
        dev = h.xyz()
    for d, s in zip(dev, host):
        assert np.array_equal(_bits(d), _bits(s))


def test_dup_points_lower_index_wins(fg, fixtures):
    fx, gi, go = fixtures["dup_points"]
    for prune in (1, 0):
        fg.set_runoff_prune(prune)
        with fg.RunoffRegrid(gi, go, xgrid=_xgrid(fx)) as h:
            imap, jmap = h.maps()
        to_low, to_high = (jmap == 5) & (imap == 4), (jmap == 7) & (imap == 9)
        assert to_low.sum() > 10 and not to_high.any()


def test_all_ocean_is_a_pure_remap_and_all_land_is_an_error(fg, fixtures):
    fx, gi, go = fixtures["latlon_regular"]
    ocean = dict(go, mask=np.ones_like(go["mask"]))
    with fg.RunoffRegrid(gi, ocean, xgrid=_xgrid(fx)) as h:
        imap, jmap = h.maps()
        out = h.apply(fx["data_in"][2])[0]
    assert np.all(imap == -1) and np.all(jmap == -1)
    ref = np.zeros(go["nx"] * go["ny"])
    for l in range(fx["i_in"].size):
        ref[fx["j_out"][l] * go["nx"] + fx["i_out"][l]] += fx["data_in"][2][fx["j_in"][l], fx["i_in"][l]] * fx["xgrid_area"][l]
    assert np.array_equal(_bits(out), _bits((ref / go["area"].ravel()).reshape(out.shape)))
    with pytest.raises(fg.FregridHipError) as e:
        fg.RunoffRegrid(gi, dict(go, mask=np.zeros_like(go["mask"])), xgrid=_xgrid(fx))
    assert e.value.code == -1 and "no ocean point" in str(e.value)
    with pytest.raises(fg.FregridHipError) as e:
        fg.RunoffRegrid(gi, dict(go, mask=np.zeros_like(go["mask"])))
    assert e.value.code == -1 and "no ocean point" in str(e.value)


@pytest.mark.parametrize("name", rc.CASES)
def test_apply_with_the_reference_list_is_bit_identical(fg, fixtures, name):
    fx, gi, go = fixtures[name]
    with fg.RunoffRegrid(gi, go, xgrid=_xgrid(fx)) as h:
        for lev in range(3):
            out, tin, tout, rate = h.apply(fx["data_in"][lev])
            assert np.array_equal(_bits(out), _bits(fx["data_out"][lev])), (name, lev)
            rin, rout = fx["totals"][lev]
            assert abs(tin - rin) <= 1e-12 * abs(rin) and abs(tout - rout) <= 1e-12 * abs(rout), (tin, rin, tout, rout)
            assert rate == ((tout - tin) / tin if tin > 0 and tout > 0 else 0.0)


def test_apply_torch_tensor_equals_numpy(fg, fixtures):
    import torch
    fx, gi, go = fixtures["dup_points"]
    with fg.RunoffRegrid(gi, go, xgrid=_xgrid(fx)) as h:
        out = h.apply(torch.from_numpy(fx["data_in"][1].copy()).cuda())[0]
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(fx["data_out"][1]))


def test_one_ocean_cell_adds_in_the_reference_order(fg, fixtures):
    fx, gi, go = fixtures["one_ocean_cell"]
    seq = rc.process_data_numpy(fx, go, gi, fx["data_in"][0])
    land = np.flatnonzero(go["mask"].ravel() == 0)
    shuffled = rc.process_data_numpy(fx, go, gi, fx["data_in"][0], order=np.random.default_rng(5).permutation(land))
    assert seq[6, 7] != shuffled[6, 7], "the values must make the order of the additions visible"
    with fg.RunoffRegrid(gi, go, xgrid=_xgrid(fx)) as h:
        out = h.apply(fx["data_in"][0])[0]
    assert np.array_equal(_bits(out), _bits(seq))
    assert np.count_nonzero(out) == 1 and out[6, 7] > 0


@pytest.mark.parametrize("name", rc.CASES)
def test_own_search_reproduces_list_and_data(fg, fixtures, name):
    """The handle's own create_xgrid_1dx2d_order1 search: the list's indices exactly; data within 2e-10, which is the stated
    1e-10 bound of the box-variant areas carried over sums of products, with a factor two for the roundings:
    relative per cell where every term is non-negative, relative to the cell's sum of |term| on the level with negative values."""
    fx, gi, go = fixtures[name]
    with fg.RunoffRegrid(gi, go) as h:
        ii, ji, io, jo, xa = h.xgrid()
        imap, jmap = h.maps()
        outs = [h.apply(fx["data_in"][lev])[0] for lev in range(3)]
    for got, key in ((ii, "i_in"), (ji, "j_in"), (io, "i_out"), (jo, "j_out")):
        assert np.array_equal(got, fx[key]), key
    assert np.array_equal(imap, fx["imap"]) and np.array_equal(jmap, fx["jmap"])
    rel = np.abs(xa - fx["xgrid_area"]) / fx["xgrid_area"]
    print(name, "max relative area difference", rel.max())
    for lev in range(2):
        ref = fx["data_out"][lev]
        err = np.abs(outs[lev] - ref)
        print(name, lev, "max relative", (err[ref != 0] / ref[ref != 0]).max())
        assert np.all(err <= 2e-10 * np.abs(ref)), (name, lev)
    # level 2: the same move decisions, values against the cell's sum of |term|
    nx, n = go["nx"], go["nx"] * go["ny"]
    cell = fx["j_out"] * nx + fx["i_out"]
    term = fx["data_in"][2][fx["j_in"], fx["i_in"]] * fx["xgrid_area"]
    pre, mag = np.zeros(n), np.zeros(n)
    np.add.at(pre, cell, term)
    np.add.at(mag, cell, np.abs(term))
    land = go["mask"].ravel() == 0
    moved = np.flatnonzero(land & (pre > 0))
    np.add.at(mag, fx["jmap"].ravel()[moved] * nx + fx["imap"].ravel()[moved], mag[moved])
    ref, got = fx["data_out"][2].ravel(), outs[2].ravel()
    assert np.array_equal(np.sign(got[land]), np.sign(ref[land])), "a land cell was moved in one and not in the other"
    err = np.abs(got - ref) * go["area"].ravel()
    print(name, 2, "max error over sum of |term|", (err[mag > 0] / mag[mag > 0]).max())
    assert np.all(err <= 2e-10 * mag)


def test_nearest_unmasked_equals_the_handle_maps(fg, fixtures):
    fx, gi, go = fixtures["tripolar_small"]
    land = np.flatnonzero(go["mask"].ravel() == 0)
    q = land[::7]
    assert q.size % 4 != 0
    for prune in (1, 0):
        fg.set_runoff_prune(prune)
        iq, jq = fg.nearest_unmasked(go["mask"], go["xt"], go["yt"], q)
        assert np.array_equal(iq, fx["imap"].ravel()[q]) and np.array_equal(jq, fx["jmap"].ravel()[q])
