"""The C interface of the streamed bilinear field loop (fg_bilin_sweep_*, include/fregrid_hip.h) without a device: the header
with the new declarations compiles as C99 and C++, the library exports the four entries, and nothing runs without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["fg_bilin_sweep_create", "fg_bilin_sweep_run_scalar", "fg_bilin_sweep_run_vector", "fg_bilin_sweep_destroy"]
FG_ERR_ARG, FG_ERR_HIP = -1, -2

PROGRAM = """#include "fregrid_hip.h"
int main(void)
{
  fg_field_conv c = {0.01, 273.15, -1.0e20};
  fg_bilin_sweep *sw = 0;
  int (*create)(fg_bilin *, int, int, fg_bilin_sweep **) = fg_bilin_sweep_create;
  int (*scalar)(fg_bilin_sweep *, const void *, long, const fg_field_conv *, int, int, void *) = fg_bilin_sweep_run_scalar;
  int (*vector)(fg_bilin_sweep *, const void *, const void *, long, const fg_field_conv *, const fg_field_conv *, int, int,
                void *, void *) = fg_bilin_sweep_run_vector;
  void (*destroy)(fg_bilin_sweep *) = fg_bilin_sweep_destroy;
  return (create && scalar && vector && destroy && sw == 0 && c.scale > 0 && FG_NC_FLOAT == 5) ? 0 : 1;
}
"""


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr


def test_header_with_the_sweep_declarations_compiles_as_c99_and_cxx(tmp_path):
    """the prototypes as the header's users will write them: a mismatch is an incompatible-pointer error under -Werror"""
    src = tmp_path / "bls.c"
    src.write_text(PROGRAM)
    inc = os.path.join(ROOT, "include")
    _run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "bls.o")])
    _run(["g++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "bls2.o")])


def test_library_exports_the_four_entries(fg):
    L = fg.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in fg._lib.EXPORTS
    assert L.fg_bilin_sweep_run_scalar.argtypes is not None and L.fg_bilin_sweep_run_vector.argtypes is not None
    assert fg.BilinearSweep is fg.field_io.BilinearSweep and hasattr(fg.BilinearPlan, "sweep")


def test_bad_arguments_are_refused_without_touching_a_device(fg):
    """a null plan, a null output handle and a null sweep give FG_ERR_ARG with a message; destroying nothing is harmless"""
    L = fg.lib()
    h = C.c_void_p()
    assert L.fg_bilin_sweep_create(None, 5, 5, C.byref(h)) == FG_ERR_ARG and not h.value
    assert b"fg_bilin_sweep_create" in L.fg_last_error()
    a = np.zeros(4, dtype=np.float32)
    cv = fg._lib.FieldConv(0.0, 0.0, -1.0e20)
    p = a.ctypes.data_as(C.c_void_p)
    assert L.fg_bilin_sweep_run_scalar(None, p, 1, C.byref(cv), 0, 0, p) == FG_ERR_ARG
    assert L.fg_bilin_sweep_run_vector(None, p, p, 1, C.byref(cv), C.byref(cv), 0, 0, p, p) == FG_ERR_ARG
    assert np.all(a == 0)
    L.fg_bilin_sweep_destroy(None)


def test_no_gpu_fails_loudly(fg):
    """no CPU fallback: without a device neither the plan nor a sweep over it can be made"""
    if fg.lib().fg_device_count() > 0:
        pytest.skip("a GPU is present")
    N = 4
    lonc, latc, lont, latt = fg.gnomonic_ed_grid(N)
    contacts = fg.find_contacts([N] * 6, [N] * 6, list(lonc), list(latc))
    with pytest.raises(fg.FregridHipError) as e:
        fg.BilinearPlan([np.asarray(a).reshape(N, N) for a in lont], [np.asarray(a).reshape(N, N) for a in latt], contacts, 8, 5)
    assert e.value.code == FG_ERR_HIP and len(str(e.value)) > 30

    class NoPlan:                      # what a caller without a device could at most hold
        _h, ncells, nlat, nlon = None, 6 * N * N, 5, 8
    with pytest.raises(fg.FregridHipError) as e:
        fg.BilinearSweep(NoPlan(), np.float32, np.float32)
    assert e.value.code == FG_ERR_HIP and "no CPU fallback" in str(e.value)
