"""Host-side checks of the --extrapolate / --dst_vgrid feature: the fixtures against a fresh run of the reference (where its
sources are present), the C ABI, the no-device behaviour, the grid factors and setup_vertical_interp.  No GPU needed."""
import ctypes as C
import math
import os
import re
import shutil
import tempfile

import numpy as np
import pytest

import extrap_cases as ec
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["fg_extrap_create", "fg_extrap_destroy", "fg_extrap_set_stream", "fg_extrap_stream", "fg_extrap_run_dev", "fg_extrap_run",
               "fg_extrap_last_syncs", "fg_extrap_get_coef", "fg_extrap_coef_host", "fg_set_extrap_batch", "fg_set_extrap_coef",
               "fg_setup_vertical_interp", "fg_dev_vertical_interp"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_fixtures_equal_a_fresh_run_of_the_reference():
    """every fixture, bit for bit: outputs (or hash and sample), iteration counts, printed residuals, kstart / kend / need_interp"""
    if not ec.reference_present():
        pytest.skip("the reference's sources are not on this machine")
    tmp = tempfile.mkdtemp(prefix="extrap_ref_")
    try:
        exe = ec.build_driver(tmp)
        for name in ec.SMALL_CASES + ec.LARGE_CASES:
            c = ec.extrap_case(name)
            out, iters, printed, sec = ec.run_ref_extrap(exe, tmp, c)
            fx, fresh = np.load(ec.golden_path(name)), ec.fixture_of(name, out, iters, printed, sec)
            assert sorted(fx.files) == sorted(fresh), name
            assert np.array_equal(fx["iters"], iters) and list(fx["maxres_printed"]) == printed and str(fx["sha256"]) == ec.sha256(out), name
            key = "sample" if name in ec.LARGE_CASES else "out"
            assert np.array_equal(bits(fx[key]), bits(fresh[key])), name
            if name == "cap":
                assert iters[0] == 3999
        for name in ec.VERTICAL_CASES:
            c = ec.vertical_case(name)
            out, ks, ke, need = ec.run_ref_vertical(exe, tmp, c)
            fx = np.load(ec.golden_path(name))
            assert np.array_equal(bits(fx["out"]), bits(out)) and list(fx["kinfo"]) == [ks, ke, need], name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_fixture_files_are_small():
    for name in ec.SMALL_CASES + ec.LARGE_CASES + ec.VERTICAL_CASES:
        assert os.path.getsize(ec.golden_path(name)) < 500 * 1000


def test_header_declares_and_library_exports_the_new_symbols(fg):
    hdr = open(os.path.join(ROOT, "include", "fregrid_hip.h")).read()
    L = fg.lib()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in fg._lib.EXPORTS and hasattr(L, s), s


def test_no_gpu_fails_loudly(fg):
    """no CPU fallback: without a device the handle cannot be made and every compute entry raises"""
    if fg.lib().fg_device_count() > 0:
        pytest.skip("a GPU is present")
    c = ec.extrap_case("warm")
    with pytest.raises(fg.FregridHipError) as e:
        fg.Extrapolator(c["lon"], c["lat"], 1)
    assert e.value.code == -2 and len(str(e.value)) > 30
    with pytest.raises(fg.FregridHipError):
        fg.do_extrapolate(c["ni"], c["nj"], c["nk"], c["lon"], c["lat"], c["data"], 1, c["missing"], c["stop_crit"])
    v = ec.vertical_case("vert_7to9")
    with pytest.raises(fg.FregridHipError):
        fg.do_vertical_interp(v["z1"], v["z2"], v["data"])
    dpt = C.POINTER(C.c_double)
    h = C.c_void_p()
    rc = fg.lib().fg_extrap_create(c["ni"], c["nj"], c["lon"].ctypes.data_as(dpt), c["lat"].ctypes.data_as(dpt), 1, 0, C.byref(h))
    assert rc == -2 and not h.value and fg._lib.last_error()


def test_bad_arguments_are_refused(fg):
    dpt = C.POINTER(C.c_double)
    h = C.c_void_p()
    lon, lat = np.array([0.1, 0.2]), np.array([10.0, 20.0])                   # degrees, not radians
    assert fg.lib().fg_extrap_create(2, 2, lon.ctypes.data_as(dpt), lat.ctypes.data_as(dpt), 1, 0, C.byref(h)) == -1
    assert "radians" in fg._lib.last_error()
    assert fg.lib().fg_extrap_create(1, 2, lon.ctypes.data_as(dpt), lat.ctypes.data_as(dpt), 1, 0, C.byref(h)) == -1


def numpy_coefficients(lon, lat):
    """fregrid_util.c:2676-2720 restated"""
    ni, nj = lon.size, lat.size
    dyu = np.append(lat[1:] - lat[:-1], 0.0); dyu[-1] = dyu[-2]
    dyt = 0.5 * (dyu + np.roll(dyu, 1)); dyt[0] = dyt[1]
    dxu = np.append(lon[1:] - lon[:-1], 0.0); dxu[-1] = dxu[-2]
    dxt = 0.5 * (dxu + np.roll(dxu, 1)); dxt[0] = dxt[1]
    latp = np.append(0.5 * (lat[:-1] + lat[1:]), lat[-1] + 0.5 * (lat[-1] - lat[-2]))
    latm = np.append(lat[0] - 0.5 * (lat[1] - lat[0]), 0.5 * (lat[1:] + lat[:-1]))
    csj, csm = np.array([math.cos(v) for v in latp]), np.array([math.cos(v) for v in latm])
    cstr = np.array([1.0 / math.cos(v) for v in lat])
    cfn = np.repeat((csj * cstr / (dyt * dyu))[:, None], ni, 1)
    cfs = np.repeat((csm * cstr / (dyt * np.append(dyu[0], dyu[:-1])))[:, None], ni, 1)
    cfe = (cstr * cstr)[:, None] / (dxu * dxt)[None, :]
    cfw = (cstr * cstr)[:, None] / (np.append(dxu[0], dxu[:-1]) * dxt)[None, :]
    cfc = 1.0 / (cfn + cfs + cfe + cfw)
    return cfw * cfc, cfe * cfc, cfs * cfc, cfn * cfc


@pytest.mark.parametrize("name", ["stretched", "regional", "real_360x180"])
def test_grid_factors_match_numpy_restatement(fg, name):
    """the host-built coefficients (cosines from csrc/sincos_glibc.h) against the same formulas with this host's libm: bitwise
    equal where libm runs its FMA sin/cos build (the reference's build host), 1e-15 relative elsewhere"""
    c = ec.extrap_case(name)
    got = fg.extrap_coef_host(c["lon"], c["lat"])
    want = numpy_coefficients(c["lon"], c["lat"])
    for g, w in zip(got, want):
        assert g.shape == w.shape == (c["nj"], c["ni"])
        if orc.host_has_fma():
            assert np.array_equal(bits(g), bits(w))
        else:
            assert np.max(np.abs(g - w) / np.abs(w)) < 1e-15
    assert np.allclose(sum(got), 1.0, rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", ec.VERTICAL_CASES)
def test_setup_vertical_interp_on_the_fixture_cases(fg, name):
    c = ec.vertical_case(name)
    fx = np.load(ec.golden_path(name))
    assert list(fg.setup_vertical_interp(c["z1"], c["z2"])) == list(fx["kinfo"])


def test_setup_vertical_interp_values(fg):
    z1 = [5.0, 15.0, 30.0, 50.0, 80.0, 120.0, 200.0]
    assert fg.setup_vertical_interp(z1, [2.0, 10.0, 15.0, 25.0, 40.0, 70.0, 110.0, 190.0, 250.0]) == (1, 7, 1)
    assert fg.setup_vertical_interp(z1, z1) == (0, 6, 0)
    assert fg.setup_vertical_interp(z1, [v + 5e-11 for v in z1]) == (0, 5, 0)       # within EPSLN10: no interpolation (:783)
    assert fg.setup_vertical_interp(z1, [v + 1e-9 for v in z1])[2] == 1
    assert fg.setup_vertical_interp(z1, [1.0, 2.0]) == (2, 1, 1)                      # all above the first source level
    assert fg.setup_vertical_interp(z1, [300.0, 400.0]) == (0, -1, 1)                 # all below the last


def test_field_io_replacement_serves_extrapolate():
    """integration/field_io_hip.c runs the handle for the conservative methods instead of handing --extrapolate back"""
    src = open(os.path.join(ROOT, "integration", "field_io_hip.c")).read()
    assert "fg_extrap_run_dev" in src and "fg_extrap_create" in src
    assert "has_missing = 0" in src
