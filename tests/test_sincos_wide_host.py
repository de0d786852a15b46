"""The wide-range part of csrc/sincos_glibc.h on the host: fgs_sin_wide / fgs_cos_wide / fgs_sincos_wide_f against the host
libm's sin() / cos() beyond 2.4262 (longitudes), and the per-vertex body of k_latlon2xyz against the compiled reference's
latlon2xyz.  The device builds its great-circle unit vectors with exactly this code, so equality here is what makes the
lon/lat plan entries carry the reference's bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "sincos_wide_check.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "libsincos_wide_check.so")
dp = C.POINTER(C.c_double)
lp = C.POINTER(C.c_long)


@pytest.fixture(scope="module")
def chk():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    inc = os.path.join(ROOT, "fre-nctools_amd", "csrc")
    srcs = [SRC, os.path.join(inc, "sincos_glibc.h"), os.path.join(inc, "sincos_table.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(s) > os.path.getmtime(OUT) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-fno-builtin", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", inc, SRC, "-o", OUT, "-lm"])
    L = C.CDLL(OUT)
    L.sincos_wide_check.argtypes = [C.c_long, C.c_long, lp, lp, lp, dp]
    L.sincos_wide_check.restype = C.c_long
    L.sincos_wide_fused_check.argtypes = [C.c_long, C.c_long, dp]
    L.sincos_wide_fused_check.restype = C.c_long
    L.sincos_wide_nan_check.argtypes = []
    L.sincos_wide_nan_check.restype = C.c_long
    L.latlon2xyz_vertex_loop.argtypes = [C.c_long] + [dp] * 5
    L.latlon2xyz_vertex_loop.restype = C.c_long
    return L


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_wide_sin_cos_bit_identical_to_host_libm(chk, seed):
    """7e6 arguments per seed (2.1e7 in all): uniform in [-4pi, 4pi] and [0, 2pi], k pi/2 +- 2^-e (k = -8..8, e <= 45), around the
    hand-over at 2.4262, reduced arguments around a*a = 0.01588 and |a| = 0.126, +-0, up to +-1000 and the bound itself."""
    if not orc.host_has_fma():
        pytest.skip("host CPU without FMA: libm runs its uncontracted sin/cos here")
    bs, bc, bf, fb = C.c_long(0), C.c_long(0), C.c_long(0), C.c_double(0)
    bad = chk.sincos_wide_check(7000000, seed, C.byref(bs), C.byref(bc), C.byref(bf), C.byref(fb))
    assert bad == 0, (bs.value, bc.value, bf.value, fb.value)


def test_fused_form_equals_the_two_single_calls(chk):
    fb = C.c_double(0)
    assert chk.sincos_wide_fused_check(4000000, 21, C.byref(fb)) == 0, fb.value


def test_beyond_the_bound_and_non_finite_is_nan(chk):
    assert chk.sincos_wide_nan_check() == 0


def _frames(fg):
    """(name, lon, lat) corner arrays: the six C24 tiles and 144x90 lat-lon grids in three longitude frames"""
    lon, lat = fg.gnomonic_ed_corners(24)
    out = [(f"c24_tile{t + 1}", lon[t], lat[t]) for t in range(6)]
    for name, b, e in (("0_2pi", 0.0, 360.0), ("-pi_pi", -180.0, 180.0), ("2pi_4pi", 360.0, 720.0)):
        lo, la = fg.latlon_corners(144, 90, b, e, -90.0, 90.0)
        out.append(("latlon_" + name, lo, la))
    return out


@pytest.mark.skipif(not orc.ref_available(), reason="oracle/_ref not built (needs the reference sources)")
def test_vertex_body_equals_reference_latlon2xyz(chk, fg):
    """The inline function k_latlon2xyz calls per vertex, looped on the host, against the compiled reference's latlon2xyz."""
    R = orc.ref()
    R.latlon2xyz.argtypes = [C.c_int] + [dp] * 5
    R.latlon2xyz.restype = None
    for name, lon, lat in _frames(fg):
        lon, lat = orc.f64(lon).ravel(), orc.f64(lat).ravel()
        n = lon.size
        got = [np.empty(n) for _ in range(3)]
        ref = [np.empty(n) for _ in range(3)]
        assert chk.latlon2xyz_vertex_loop(n, orc._dp(lon), orc._dp(lat), *[orc._dp(v) for v in got]) == 0, name
        R.latlon2xyz(n, orc._dp(lon), orc._dp(lat), *[orc._dp(v) for v in ref])
        for g, r, ax in zip(got, ref, "xyz"):
            if orc.host_has_fma():
                assert np.array_equal(_bits(g), _bits(r)), (name, ax)
            else:                                   # (the relaxed rule of test_device_sincos_equals_host_libm)
                assert np.mean(_bits(g) != _bits(r)) < 2e-3 and np.max(np.abs(g - r)) < 3e-16, (name, ax)


def test_vertex_body_outside_the_domain_is_nan(chk):
    lon = np.array([0.5, np.nan, 0.5, 1025.0, np.inf, 0.5, -1000.0])
    lat = np.array([0.25, 0.25, np.nan, 0.25, 0.25, 2.43, -0.25])
    out = [np.empty(lon.size) for _ in range(3)]
    assert chk.latlon2xyz_vertex_loop(lon.size, orc._dp(lon), orc._dp(lat), *[orc._dp(v) for v in out]) == 5
    for v in out:
        assert np.array_equal(np.isnan(v), [False, True, True, True, True, True, False])
