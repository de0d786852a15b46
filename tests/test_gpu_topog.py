"""make_topog's realistic topography on the device against the reference's fixtures (tests/golden/topog_*.npz,
tests/topog_cases.py): the source preparation, the depth after the remap, after filter_topo and after process_topo bit for bit,
num_levels and the reference's three counts equal, for the whole chain and for each stage fed the reference's intermediate, with
the isolated-cell step evaluated both as the in-place sweep and all cells at once; the great-circle remap to 1e-12 of the largest
depth against the reference's fixture (glibc's acosl rounds an angle differently now and then) and bit for bit against the remap
replayed on the exchange cells of the oracle that rounds like the device (gc_oracle.c's _cr build); the reference's errors; two handles; a second source on one handle."""
import ctypes as C

import numpy as np
import pytest

import orc
import topog_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixtures(fg, gpu_ok):
    return {name: tc.load(name) for name in tc.CASES}


@pytest.fixture(autouse=True)
def _default_sweep(fg):
    yield
    fg.set_topog_sweep(1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(name, got, ref):
    print(name, "cells that differ:", int((bits(got) != bits(ref)).sum()), "max |diff|", float(np.abs(got - ref).max()))
    assert np.array_equal(bits(got), bits(ref)), name


def check_counts(st, fx):
    for k in tc.COUNTS:
        assert st[k] == int(fx[k]), (k, st[k], int(fx[k]))


def with_first_row(fx, depth):
    d = depth.copy()
    if int(fx["fill_first_row"]):
        d[0] = 0.0
    return d


@pytest.mark.parametrize("name", [n for n in tc.CHAIN if n != "cube_c6_gca"])
def test_whole_chain_equals_the_reference(fg, fixtures, name):
    fx = fixtures[name]
    zw = fx["zw"]
    with fg.Topog(fx["x_dst"], fx["y_dst"], **tc.options(fx)) as h:
        h.source(fx["xt_src"], fx["yt_src"], fx["data"], float(fx["missing"]))
        st = h.stats()
        assert (st["jstart"], st["jend"]) == (int(fx["jstart"]), int(fx["jend"]))
        src = h.source_arrays()
        for k in ("x_src", "y_src", "depth_src", "mask_src"):
            same(k, src[k], fx[k])
        h.remap()
        same("depth after remap", h.depth(), fx["depth_remap"])
        assert (h.stats()["nxgrid"] > 0) != bool(int(fx["on_grid"]))
        if int(fx["filter_topog"]):
            same("depth after filter", h.filter().depth(), fx["depth_filter"])
        for fused in (0, 1):
            fg.set_topog_sweep(fused)
            h.run(zw if zw.size else None)
            same(f"depth after the whole chain (sweep {fused})", h.depth(), fx["depth_final"])
            st = h.stats()
            assert st["deepest"] == max(0.0, float(fx["depth_filter"].max()))
            if zw.size:
                assert np.array_equal(h.num_levels(), fx["num_levels"])
                check_counts(st, fx)
            else:
                assert st["verdict"] == -1
                with pytest.raises(fg.FregridHipError, match="no levels"):
                    h.num_levels()
    if name == "regional":
        depth, levels = fg.create_realistic_topog(fx["x_dst"], fx["y_dst"], fx["xt_src"], fx["yt_src"], fx["data"], float(fx["missing"]), zw=zw,
                                                  **tc.options(fx))
        same("create_realistic_topog", depth, fx["depth_final"])
        assert np.array_equal(levels, fx["num_levels"])


def test_great_circle_remap_then_the_stages_from_the_reference_intermediate(fg, fixtures):
    fx = fixtures["cube_c6_gca"]
    with fg.Topog(fx["x_dst"], fx["y_dst"], **tc.options(fx)) as h:
        h.source(fx["xt_src"], fx["yt_src"], fx["data"], float(fx["missing"]))
        src = h.source_arrays()
        h.remap()
        got, ref = h.depth(), fx["depth_remap"]
        print("great-circle remap: max |diff|", float(np.abs(got - ref).max()), "bar", 1e-12 * float(np.abs(ref).max()))
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        assert h.stats()["nxgrid"] > 0
        # conserve_interp_great_circle (interp.c:312-356) replayed on the exchange cells of the oracle that rounds like the device
        # (gc_oracle.c's _cr build): per destination cell the sum of its areas in list order, then data * (area / sum) added in
        # list order -- k_apply_frac's order -- so the depth after the remap in bits
        ny_now, nxs = src["depth_src"].shape
        ny, nx = got.shape
        o = orc.orc_create_xgrid_gc(nxs, ny_now, nx, ny, src["x_src"], src["y_src"], fx["x_dst"] * tc.D2R, fx["y_dst"] * tc.D2R,
                                    mask=src["mask_src"], cr=True)
        assert o["n"] == h.stats()["nxgrid"]
        d = o["j_out"].astype(np.int64) * nx + o["i_out"]
        s = o["j_in"].astype(np.int64) * nxs + o["i_in"]
        dst_area, replay = np.zeros(nx * ny), np.zeros(nx * ny)
        for k in range(o["n"]):
            dst_area[d[k]] += o["area"][k]
        data = src["depth_src"].ravel()
        for k in range(o["n"]):
            replay[d[k]] += data[s[k]] * (o["area"][k] / dst_area[d[k]])
        nd = int((bits(got).ravel() != bits(replay)).sum())
        assert nd == 0, f"{nd} of {nx * ny} depths differ from the replay on the _cr oracle's exchange cells"
        h.set_depth(fx["depth_remap"]).filter()
        same("depth after filter", h.depth(), fx["depth_filter"])
        h.set_depth(with_first_row(fx, fx["depth_filter"])).process(fx["zw"])
        same("depth after process", h.depth(), fx["depth_final"])
        assert np.array_equal(h.num_levels(), fx["num_levels"])


@pytest.mark.parametrize("name", tc.STAGE)
def test_each_stage_from_the_reference_intermediate(fg, fixtures, name):
    fx = fixtures[name]
    ny, nx = fx["depth_in"].shape
    x, y = tc.latlon_corners_deg(nx, ny, 0.0, 360.0, -80.0, 80.0)            # the stages never read the grid
    with fg.Topog(x, y, **tc.options(fx)) as h:
        h.set_depth(fx["depth_in"])
        if int(fx["filter_topog"]):
            h.filter()
            assert h.stats()["deepest"] == max(0.0, float(fx["depth_filter"].max()))
        same("depth after filter", h.depth(), fx["depth_filter"])
        if not fx["zw"].size:
            return
        for fused in (0, 1):
            fg.set_topog_sweep(fused)
            h.set_depth(fx["depth_filter"]).process(fx["zw"])
            same(f"depth after process (sweep {fused})", h.depth(), fx["depth_final"])
            assert np.array_equal(h.num_levels(), fx["num_levels"])
            st = h.stats()
            for k in tc.COUNTS[:3]:
                assert st[k] == int(fx[k]), (k, fused)
            swept = int(fx["adjust_topo"]) and int(fx["fill_isolated_cells"]) and not fused
            nj_max = ny - 1 if int(fx["tripolar_grid"]) else ny
            assert st["sweep_launches"] == (max(0, nx + 2 * nj_max - 2) if swept else 0)


def test_the_reference_errors_come_back_with_its_text_and_leave_the_library_usable(fg, fixtures):
    fx = fixtures["process_defaults"]
    ny, nx = fx["depth_in"].shape
    x, y = tc.latlon_corners_deg(nx, ny, 0.0, 360.0, -80.0, 80.0)

    def raises(text, zw=fx["zw"], **opts):
        with fg.Topog(x, y, **dict(tc.options(fx), **opts)) as h:
            h.set_depth(fx["depth_in"])
            for call in (h.process, h.run):
                with pytest.raises(fg.FregridHipError) as e:
                    call(zw)
                assert e.value.code == -1 and text in str(e.value), str(e.value)
                if call is h.process:
                    h.source(*_small_source(fixtures))

    raises("topog: number of vertical cells=3, is less than kmt_min=4", zw=fx["zw"][:3], kmt_min=4)
    raises("topog: at most one of round_shallow/deepen_shallow/fill_shallow can be set to true", round_shallow=1, fill_shallow=1)
    raises("topog: at most one of round_shallow/deepen_shallow/fill_shallow can be set to true", deepen_shallow=1, fill_shallow=1)
    zw = fx["zw"].copy()
    zw[5], zw[6] = zw[6], zw[5]
    raises("nearest_index: array must be monotonically increasing", zw=zw)
    with fg.Topog(x, y) as h:
        xt, yt, data, missing = _small_source(fixtures)
        with pytest.raises(fg.FregridHipError, match="nc_type should be NC_DOUBLE, NC_FLOAT or NC_INT") as e:
            h.source(xt, yt, np.zeros(data.shape, dtype=np.int16), missing)
        assert e.value.code == -1
        d64 = np.ascontiguousarray(data, dtype=np.float64)
        rc = fg.lib().fg_topog_set_source(h.handle, xt.size, yt.size, xt.ctypes.data_as(C.POINTER(C.c_double)), yt.ctypes.data_as(C.POINTER(C.c_double)),
                                          d64.ctypes.data_as(C.c_void_p), 3, missing)                     # NC_SHORT
        assert rc == -1 and "nc_type should be NC_DOUBLE, NC_FLOAT or NC_INT" in fg._lib.last_error()
        with pytest.raises(fg.FregridHipError, match="fg_topog_set_source has not been called"):
            h.remap()
        with pytest.raises(fg.FregridHipError, match="holds no depth"):
            h.depth()
    with fg.Topog(x, y, on_grid=1) as h:
        with pytest.raises(fg.FregridHipError, match="on_grid needs"):
            h.source(*_small_source(fixtures))
    with fg.Topog(x, y, **tc.options(fx)) as h:                                                        # the library goes on working
        h.set_depth(fx["depth_in"]).process(fx["zw"])
        same("depth after process", h.depth(), fx["depth_final"])


def _small_source(fixtures):
    fx = fixtures["torus"]
    return fx["xt_src"], fx["yt_src"], fx["data"], float(fx["missing"])


def test_two_handles_alive_at_once_and_a_second_source_on_one(fg, fixtures):
    a, b = fixtures["tripolar"], fixtures["cube_c6"]
    with fg.Topog(a["x_dst"], a["y_dst"], **tc.options(a)) as ha, fg.Topog(b["x_dst"], b["y_dst"], **tc.options(b)) as hb:
        ha.source(a["xt_src"], a["yt_src"], a["data"], float(a["missing"]))
        hb.source(*_small_source(fixtures)).run(b["zw"])                    # another file first: float64, 60 x 30
        other = hb.depth()
        hb.source(b["xt_src"], b["yt_src"], b["data"], float(b["missing"]))
        with pytest.raises(fg.FregridHipError, match="holds no depth"):
            hb.depth()                                                      # the old source's result is gone
        ha.run(a["zw"])
        hb.run(b["zw"])
        ha.run(a["zw"])                                                     # a handle may be run again
        for h, fx in ((hb, b), (ha, a)):
            same("depth", h.depth(), fx["depth_final"])
            assert np.array_equal(h.num_levels(), fx["num_levels"])
            check_counts(h.stats(), fx)
        assert not np.array_equal(other, b["depth_final"])
