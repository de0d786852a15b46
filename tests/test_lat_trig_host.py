"""fgs_trig<M> of csrc/sincos_glibc.h on the host: one evaluation of an argument for any subset of libm's sin(), cos() and the
two results of sincos().  Required: for every subset the polygon integrals use, and the full one, each result has the 64-bit
pattern of fgs_sin / fgs_cos / fgs_sincos -- and of the host libm itself -- on millions of arguments over [-2.426, 2.426], the
zeros, every table node, every mid-point between two nodes (where the reduction changes its node) and every range threshold
with its +-4 ulp neighbours, and the last 1e-6 below pi/2."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "lat_trig_check.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "liblat_trig_check.so")


@pytest.fixture(scope="module")
def chk():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    inc = os.path.join(ROOT, "fre-nctools_amd", "csrc")
    srcs = [SRC, os.path.join(inc, "sincos_glibc.h"), os.path.join(inc, "sincos_table.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(s) > os.path.getmtime(OUT) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-fno-builtin", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", inc, SRC, "-o", OUT, "-lm"])
    L = C.CDLL(OUT)
    L.lat_trig_check.argtypes = [C.c_long, C.c_long, C.c_int, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.lat_trig_check.restype = C.c_long
    return L


def _host_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return True


def _run(chk, n, seed, libm, fma_host):
    bad = (C.c_long * 4)()
    fb, na = C.c_double(0), C.c_long(0)
    nb = chk.lat_trig_check(n, seed, libm, fma_host, bad, C.byref(fb), C.byref(na))
    assert na.value > n + 5000
    return nb, dict(sin_fma=bad[0], cos_fma=bad[1], sin_nofma=bad[2], cos_nofma=bad[3], first_bad=fb.value.hex())


def test_trig_subsets_equal_the_separate_functions(chk):
    """Every mask: the requested results are fgs_sin / fgs_cos / fgs_sincos bit for bit, the others are not written."""
    nb, info = _run(chk, 3000000, 11, 0, 1)
    assert nb == 0, info


def test_trig_uncontracted_results_equal_host_sincos(chk):
    """FGS_SIN_N / FGS_COS_N against libm's sincos() directly."""
    nb, info = _run(chk, 2000000, 12, 1, 0)
    assert nb == 0, info


def test_trig_fma_results_equal_host_sin_cos(chk):
    """FGS_SIN_F / FGS_COS_F against libm's sin() / cos() as an FMA-capable x86-64 host runs them."""
    if not _host_has_fma():
        pytest.skip("host CPU without FMA: libm runs its uncontracted sin/cos here")
    nb, info = _run(chk, 2000000, 13, 1, 1)
    assert nb == 0, info
