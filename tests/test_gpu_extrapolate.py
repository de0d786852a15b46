"""--extrapolate fill and --dst_vgrid levels on the device against the REFERENCE's answers (tests/golden/extrapolate_*.npz, made
by tests/golden/make_golden_extrapolate.py from the reference's do_extrapolate / do_vertical_interp; inputs rebuilt by
tests/extrap_cases.py).  There is no tolerance: the arithmetic is the reference's, so outputs are compared on their bits,
iteration counts for equality and the largest residual against the six digits the reference printed."""
import ctypes as C
import threading

import numpy as np
import pytest

import extrap_cases as ec
import orc

pytestmark = pytest.mark.gpu
ALL_CASES = ec.SMALL_CASES + ec.LARGE_CASES
_dpt = C.POINTER(C.c_double)
_ipt = C.POINTER(C.c_int)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_against_fixture(name, c, out, iters, resmax):
    fx = np.load(ec.golden_path(name))
    print(name, "iters", list(iters), "reference", list(fx["iters"]), "resmax", list(resmax), "printed", list(fx["maxres_printed"]))
    assert np.array_equal(iters, fx["iters"])
    for k in range(c["nk"]):
        assert "%g" % resmax[k] == str(fx["maxres_printed"][k])
        if name != "cap":
            assert resmax[k] <= c["stop_crit"]
    assert out.shape == c["data"].shape
    if name in ec.LARGE_CASES:
        assert ec.sha256(out) == str(fx["sha256"])
        assert np.array_equal(bits(out.reshape(-1)[ec.sample_index(out.size)]), bits(fx["sample"]))
    else:
        assert np.array_equal(bits(out), bits(fx["out"]))
        assert ec.sha256(out) == str(fx["sha256"])


def make(fg, c):
    return fg.Extrapolator(c["lon"], c["lat"], c["is_cyclic"])


@pytest.mark.parametrize("name", ALL_CASES)
def test_extrapolate_bit_identical_to_reference(fg, gpu_ok, name):
    """the Python mirror on host arrays (fg_extrap_run)"""
    c = ec.extrap_case(name)
    with make(fg, c) as ex:
        out, iters, resmax = ex.run(c["data"], c["missing"], c["stop_crit"])
    check_against_fixture(name, c, out, iters, resmax)


@pytest.mark.parametrize("name", ALL_CASES)
def test_extrapolate_device_resident_entry(fg, gpu_ok, name):
    """torch device tensors through fg_extrap_run_dev, separate output and in place"""
    import torch
    c = ec.extrap_case(name)
    d = torch.from_numpy(c["data"]).cuda()
    with make(fg, c) as ex:
        out, iters, resmax = ex.run(d, c["missing"], c["stop_crit"])
        assert out.is_cuda and np.array_equal(bits(d.cpu().numpy()), bits(c["data"]))        # the input is left alone
        check_against_fixture(name, c, out.cpu().numpy(), iters, resmax)
        it2, rm2 = np.empty(c["nk"], dtype=np.int32), np.empty(c["nk"])
        torch.cuda.synchronize()
        fg._lib.check(fg.lib().fg_extrap_run_dev(ex.handle, d.data_ptr(), d.data_ptr(), c["nk"], 0, c["missing"], c["stop_crit"],
                                                 it2.ctypes.data_as(_ipt), rm2.ctypes.data_as(_dpt)))
        check_against_fixture(name, c, d.cpu().numpy(), it2, rm2)


@pytest.mark.parametrize("name", ["warm", "cap", "real_360x180"])
def test_extrapolate_mirror_function(fg, gpu_ok, name, capsys):
    """do_extrapolate with the reference's argument list, printing the reference's line"""
    c = ec.extrap_case(name)
    out = fg.do_extrapolate(c["ni"], c["nj"], c["nk"], c["lon"], c["lat"], c["data"].reshape(-1), c["is_cyclic"], c["missing"],
                            c["stop_crit"])
    fx = np.load(ec.golden_path(name))
    assert ec.sha256(out) == str(fx["sha256"])
    want = ["Stopped after %d iterations, maxres = %s" % (n, s) for n, s in zip(fx["iters"], fx["maxres_printed"])]
    assert capsys.readouterr().out.strip().splitlines() == want


@pytest.mark.parametrize("name", ALL_CASES)
def test_extrapolate_independent_of_batch_and_coefficient_mode(fg, gpu_ok, name):
    """the stop lands on the reference's iteration wherever a batch of launches ends; the stored coefficient table and the
    per-use evaluation give the same bits; the host synchronises once per batch, not once per iteration"""
    c = ec.extrap_case(name)
    fx = np.load(ec.golden_path(name))
    try:
        with make(fg, c) as ex:
            for batch, stored in ((1, 0), (7, 0), (0, 0), (0, 1), (7, 1)):
                fg.set_extrap_batch(batch)
                fg.set_extrap_coef(stored)
                out, iters, resmax = ex.run(c["data"], c["missing"], c["stop_crit"])
                check_against_fixture(name, c, out, iters, resmax)
                b = batch if batch else 64
                assert ex.last_syncs == sum(-(-(int(n) + 1) // b) for n in fx["iters"])
    finally:
        fg.set_extrap_batch(0)
        fg.set_extrap_coef(0)


def test_extrapolate_coefficients_match_host_table(fg, gpu_ok):
    c = ec.extrap_case("stretched")
    with make(fg, c) as ex:
        for a, b in zip(ex.coef(), fg.extrap_coef_host(c["lon"], c["lat"])):
            assert np.array_equal(bits(a), bits(b))


def test_two_handles_two_streams_and_no_state_between_runs(fg, gpu_ok):
    """two handles (each on its own stream) driven from two host threads give the single-handle results; a second run of the
    same handle, after a different field, gives the first run's bits"""
    names = ["warm", "whole_level"]
    cases = [ec.extrap_case(n) for n in names]
    handles = [make(fg, c) for c in cases]
    assert handles[0].stream != handles[1].stream
    res = [None, None]

    def work(q):
        res[q] = [handles[q].run(cases[q]["data"], cases[q]["missing"], cases[q]["stop_crit"]) for _ in range(2)]

    th = [threading.Thread(target=work, args=(q,)) for q in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for q in range(2):
        for out, iters, resmax in res[q]:
            check_against_fixture(names[q], cases[q], out, iters, resmax)
    # same grid (72 x 45 cyclic), other field in between: nothing of it is left in the handle
    handles[0].run(cases[1]["data"], cases[1]["missing"], cases[1]["stop_crit"])
    out, iters, resmax = handles[0].run(cases[0]["data"], cases[0]["missing"], cases[0]["stop_crit"])
    check_against_fixture(names[0], cases[0], out, iters, resmax)
    for h in handles:
        h.destroy()


def test_level_stride(fg, gpu_ok):
    """levels further apart than ni*nj (fregrid keeps the tiles of a level back to back)"""
    import torch
    c = ec.extrap_case("warm")
    ncell = c["ni"] * c["nj"]
    stride = ncell + 100
    buf = torch.full((c["nk"], stride), 7.0, dtype=torch.float64, device="cuda")
    buf[:, :ncell] = torch.from_numpy(c["data"].reshape(c["nk"], ncell)).cuda()
    iters, resmax = np.empty(c["nk"], dtype=np.int32), np.empty(c["nk"])
    with make(fg, c) as ex:
        torch.cuda.synchronize()
        fg._lib.check(fg.lib().fg_extrap_run_dev(ex.handle, buf.data_ptr(), buf.data_ptr(), c["nk"], stride, c["missing"], c["stop_crit"],
                                                 iters.ctypes.data_as(_ipt), resmax.ctypes.data_as(_dpt)))
    h = buf.cpu().numpy()
    assert np.all(h[:, ncell:] == 7.0)
    check_against_fixture("warm", c, h[:, :ncell].reshape(c["data"].shape).copy(), iters, resmax)


# ------------------------------------------------------------------------------------------------ vertical interpolation
@pytest.mark.parametrize("name", ec.VERTICAL_CASES)
def test_vertical_interp_bit_identical_to_reference(fg, gpu_ok, name):
    import torch
    c = ec.vertical_case(name)
    fx = np.load(ec.golden_path(name))
    out = fg.do_vertical_interp(c["z1"], c["z2"], c["data"])
    assert out.shape == fx["out"].shape and np.array_equal(bits(out), bits(fx["out"]))
    out_t = fg.do_vertical_interp(c["z1"], c["z2"], torch.from_numpy(c["data"]).cuda())
    assert np.array_equal(bits(out_t.cpu().numpy()), bits(fx["out"]))


def test_vertical_interp_fatal_checks(fg, gpu_ok):
    c = ec.vertical_case("vert_7to9")
    z1 = c["z1"].copy()
    z1[3] = z1[2]
    with pytest.raises(fg.FregridHipError, match="grid1 not monotonic") as e:
        fg.do_vertical_interp(z1, c["z2"], c["data"])
    assert e.value.code == -7
    z2 = c["z2"].copy()
    z2[4] = z2[3]
    with pytest.raises(fg.FregridHipError, match="grid2 not monotonic"):
        fg.do_vertical_interp(c["z1"], z2, c["data"])


def test_linear_vertical_interp_vs_compiled_reference(fg, gpu_ok):
    """linear_vertical_interp alone (interp.c:360) from oracle/_ref/libfrenc_ref.so on a random 64 x 48, 33 -> 50 level case; the
    destination levels lie inside the source range, so do_vertical_interp is that function"""
    R = orc.ref()
    if R is None:
        pytest.fail("oracle/_ref/libfrenc_ref.so has not been built")
    rng = np.random.default_rng(20261016)
    nx, ny, nk1, nk2 = 64, 48, 33, 50
    z1 = np.cumsum(rng.uniform(1.0, 40.0, nk1))
    z2 = np.sort(rng.uniform(z1[0], z1[-1], nk2))
    z2[0], z2[-1], z2[17] = z1[0], z1[-1], z1[9]
    z2 = np.sort(z2)
    data = rng.standard_normal((nk1, ny, nx)) * 30.0
    assert fg.setup_vertical_interp(z1, z2) == (0, nk2 - 1, 1)
    want = np.empty((nk2, ny, nx))
    R.linear_vertical_interp.argtypes = [C.c_int] * 4 + [_dpt] * 4
    R.linear_vertical_interp.restype = None
    d1 = data.copy()
    R.linear_vertical_interp(nx, ny, nk1, nk2, z1.ctypes.data_as(_dpt), z2.ctypes.data_as(_dpt), d1.ctypes.data_as(_dpt),
                             want.ctypes.data_as(_dpt))
    got = fg.do_vertical_interp(z1, z2, data)
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------ the pieces compose
def test_end_to_end_extrapolate_remap_vertical(fg, gpu_ok):
    """lat-lon 72 x 45 field with land -> extrapolate -> conserve_order1 onto 36 x 18 -> --dst_vgrid levels, all on the device,
    equals the same chain fed with the fixture's extrapolated field (the reference's)."""
    import torch
    c = ec.extrap_case("warm")
    fx = np.load(ec.golden_path("warm"))
    ni, nj, nk = c["ni"], c["nj"], c["nk"]
    lonc, latc = fg.latlon_corners(ni, nj)
    lo, la = fg.latlon_corners(36, 18)
    plan = fg.XgridPlan.create(1, [fg.GridConfig(ni, nj, lonc, latc)], fg.GridConfig(36, 18, lo, la))
    plan.finalize()
    z1, z2 = np.array([5.0, 15.0, 30.0]), np.array([2.0, 10.0, 15.0, 22.0, 40.0])

    def chain(filled_t):
        out_t = torch.empty(nk * 36 * 18, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        plan.apply(filled_t, out_t, nz=nk)
        plan.sync()
        return fg.do_vertical_interp(z1, z2, out_t.reshape(nk, 18, 36)).cpu().numpy()

    with make(fg, c) as ex:
        filled, _, _ = ex.run(torch.from_numpy(c["data"]).cuda(), c["missing"], c["stop_crit"])
    got = chain(filled)
    want = chain(torch.from_numpy(fx["out"]).cuda())
    assert got.shape == (5, 18, 36) and np.all(np.isfinite(got)) and np.all(np.abs(got) < 1e3)       # no missing value survives
    assert np.array_equal(bits(got), bits(want))
    plan.destroy()
