"""Bilinear cubed-sphere -> lat-lon (fregrid --interp_method bilinear) on the host: fixture inputs, the acos / asin header,
the remap file and argument checks.  The fixtures come from the reference's own bilinear_interp.c
(tests/golden/make_golden_bilinear.py)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = sorted(glob.glob(os.path.join(GOLD, "bilinear_c24_*.npz")))


@pytest.fixture(scope="module")
def fg():
    return __graft_entry__.load_package()


def contacts_and_centres(fg, N):
    lonc, latc, lont, latt = fg.gnomonic_ed_grid(N)
    return fg.find_contacts([N] * 6, [N] * 6, list(lonc), list(latc)), lont, latt


def test_fixture_cases_present():
    assert len(CASES) == 5
    for p in CASES + [os.path.join(GOLD, "bilinear_write_layout.npz")]:
        assert os.path.getsize(p) < 1 << 20


def test_generator_and_halo_reproduce_fixture_inputs(fg):
    """the repository's gnomonic generator + halo map give the halo'd centres the reference ran on, bit for bit; the xyz
    the device search uses are latlon2xyz of those"""
    d = np.load(CASES[0])
    N = int(d["config"][0])
    contacts, lont, latt = contacts_and_centres(fg, N)
    _, m = fg.halo_map([N] * 6, [N] * 6, contacts)
    for tiles, ref in ((lont, d["lont_halo"]), (latt, d["latt_halo"])):
        h = np.zeros((6, N + 2, N + 2))
        h[:, 1:-1, 1:-1] = np.asarray(tiles).reshape(6, N, N)
        h = h.reshape(-1)
        e = np.nonzero(m >= 0)[0]
        h[e] = h[m[e]]
        assert np.array_equal(h.view(np.int64), ref.reshape(-1).view(np.int64))
    # halo corners stay at init_halo's zero
    for t in range(6):
        for j, i in ((0, 0), (0, N + 1), (N + 1, 0), (N + 1, N + 1)):
            assert d["lont_halo"][t, j, i] == 0.0 and d["latt_halo"][t, j, i] == 0.0


def test_fine_grid_matches_get_output_grid_by_size(fg):
    from fre_nctools_amd import bilinear
    lo, la, l1 = bilinear.fine_grid(72, 37, 1)
    assert lo.shape == (73, 144) and l1.shape == (73,)
    assert l1[0] == -90.0 * (np.pi / 180) and l1[-1] == 90.0 * (np.pi / 180)
    lo, la, l1 = bilinear.fine_grid(72, 36, 0, center_y=True)
    assert np.allclose(l1, (-90 + (np.arange(36) + 0.5) * 5.0) * np.pi / 180, rtol=0, atol=1e-15)


def test_acos_asin_header_against_libm():
    """csrc/acos_dd.h (the device's acos / asin of the weights) against the host libm on 4 million arguments per function.
    glibc 2.35's acos / asin are not correctly rounded (errors up to ~0.505 ulp): the header rounds correctly, so it may
    differ from libm by one ulp where libm misrounds -- never more, never where libm is the nearer one, and rarely."""
    inc = os.path.join(ROOT, "fre-nctools_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostcheck", "acos_check.cpp")
    out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libacos_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", inc, src, "-o", out, "-lm"])
    L = C.CDLL(out)
    L.acos_check.argtypes = [C.c_long, C.POINTER(C.c_long)]
    L.acos_check.restype = C.c_long
    n = 4000000
    f = (C.c_long * 4)()
    bad = L.acos_check(n, f)
    assert f[2] <= 1, list(f)              # at most one ulp
    assert f[3] == 0, list(f)              # every difference is a libm misrounding
    assert bad <= 2 * n * 2e-3, list(f)


def test_remap_file_round_trip_and_reference_layout(fg, tmp_path):
    """our WRITE branch, parsed back with fg_nc_inq_*, has the layout the reference's WRITE branch requested, and its data
    are the buffers the reference handed to mpp_put_var_value, byte for byte; READ gives the arrays back"""
    from fre_nctools_amd import bilinear
    lay = np.load(os.path.join(GOLD, "bilinear_write_layout.npz"))
    d = np.load(os.path.join(GOLD, "bilinear_c24_72x37_fs0.npz"))
    index, weight = d["index"], d["weight"]
    path = str(tmp_path / "remap_bilinear.nc")
    bilinear.write_bilinear_remap_file(path, 72, 37, index, weight)
    rows = [r.split() for r in str(lay["layout"]).splitlines()]
    dims = [(r[1], int(r[2])) for r in rows if r[0] == "dim"]
    vars_ = [(r[1], int(r[2]), [int(x) for x in r[4:]]) for r in rows if r[0] == "var"]
    L = fg.lib()
    h = C.c_void_p()
    assert L.fg_nc_open(path.encode(), C.byref(h)) == 0
    try:
        assert L.fg_nc_inq_ndims(h) == len(dims)
        for k, (name, ln) in enumerate(dims):
            buf = C.create_string_buffer(64)
            n = C.c_long()
            assert L.fg_nc_inq_dim(h, k, buf, 64, C.byref(n)) == 0
            assert (buf.value.decode(), n.value) == (name, ln)
        assert L.fg_nc_inq_nvars(h) == len(vars_)
        for k, (name, typ, dimids) in enumerate(vars_):
            buf = C.create_string_buffer(64)
            t, nd = C.c_int(), C.c_int()
            ids = (C.c_int * 8)()
            shape = (C.c_long * 8)()
            assert L.fg_nc_inq_var(h, k, buf, 64, C.byref(t), C.byref(nd), ids, shape) == 0
            assert (buf.value.decode(), t.value, list(ids[:nd.value])) == (name, typ, dimids)
    finally:
        L.fg_nc_close(h)
    # the stored data, read raw, are the reference's buffers
    ri = np.empty(index.size, dtype=np.int32)
    rw = np.empty(weight.size)
    for name, arr in (("index", ri), ("weight", rw)):
        h = C.c_void_p()
        assert L.fg_nc_open(path.encode(), C.byref(h)) == 0
        vid = L.fg_nc_inq_varid(h, name.encode())
        shape = (C.c_long * 3)(3 if name == "index" else 4, 37, 72)
        start = (C.c_long * 3)(0, 0, 0)
        assert L.fg_nc_get_vara(h, vid, start, shape, arr.ctypes.data_as(C.c_void_p)) == 0
        L.fg_nc_close(h)
    assert ri.tobytes() == lay["put_index"].tobytes()
    assert rw.tobytes() == lay["put_weight"].tobytes()
    i2, w2 = bilinear.read_bilinear_remap_file(path, 72, 37)
    assert np.array_equal(i2, index) and np.array_equal(w2.view(np.int64), weight.view(np.int64))
    with pytest.raises(fg.FregridHipError):
        bilinear.read_bilinear_remap_file(path, 144, 73)          # the reference's size-mismatch check


def test_invalid_arguments_return_codes(fg):
    """the reference's fatal checks come back as FG_ERR_ARG (-1), before any device is touched"""
    from fre_nctools_amd import bilinear
    L = fg.lib()
    contacts, lont, latt = contacts_and_centres(fg, 8)
    lont = [np.ascontiguousarray(a, dtype=np.float64) for a in np.asarray(lont).reshape(6, 8, 8)]
    latt = [np.ascontiguousarray(a, dtype=np.float64) for a in np.asarray(latt).reshape(6, 8, 8)]
    dpt = C.POINTER(C.c_double)
    keys = bilinear._CONTACT_KEYS
    c = {k: np.ascontiguousarray(contacts[k], dtype=np.int32) for k in keys}

    def create(ntiles=6, ncont=12, nlat=19, fs=0):
        nt = 6
        h = C.c_void_p()
        return L.fg_bilin_create(ntiles, (C.c_int * nt)(*[8] * nt), (C.c_int * nt)(*[8] * nt),
                                 (dpt * nt)(*[a.ctypes.data_as(dpt) for a in lont]), (dpt * nt)(*[a.ctypes.data_as(dpt) for a in latt]),
                                 ncont, *[c[k].ctypes.data_as(C.POINTER(C.c_int)) for k in keys], 36, nlat, fs, 0.0, 360.0, -90.0,
                                 90.0, 0, 0, C.byref(h))
    assert len(c["tile1"]) == 12
    assert create(ntiles=5) == -1
    assert create(ncont=11) == -1
    assert create(fs=-1) == -1
    assert create(nlat=1) == -1
