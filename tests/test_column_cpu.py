"""Host-side checks of the column loop (fg_extrap_run_batch_dev, fg_column_*): the fixtures tests/golden/column_*.npz against a
fresh run of the reference's chain (where its sources and oracle/_ref/ are present), the C ABI, and the no-device behaviour.
No GPU needed."""
import os
import re
import shutil
import tempfile

import numpy as np
import pytest

import column_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["fg_extrap_run_batch_dev", "fg_column_create", "fg_column_run", "fg_column_destroy", "fg_set_column_records"]
LARGEST_FIXTURE = os.path.join(ROOT, "tests", "golden", "c48_xgrid.npz")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_fixtures_equal_a_fresh_run_of_the_reference(fg):
    if not cc.reference_available():
        pytest.skip("the reference's sources (or oracle/_ref/libconserve_ref.so) are not on this machine")
    tmp = tempfile.mkdtemp(prefix="column_ref_")
    try:
        fresh = cc.reference_results(fg, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert sorted(fresh) == sorted(cc.CASES)
    for (dest, vgrid), want in fresh.items():
        fx = np.load(cc.golden_path(dest, vgrid))
        assert sorted(fx.files) == ["iters", "out"]
        assert fx["out"].shape == want["out"].shape and np.array_equal(bits(fx["out"]), bits(want["out"])), (dest, vgrid)
        assert np.array_equal(fx["iters"], want["iters"]), (dest, vgrid)


def test_fixtures_are_what_the_cases_say():
    for dest, vgrid in cc.CASES:
        path = cc.golden_path(dest, vgrid)
        assert os.path.getsize(path) < os.path.getsize(LARGEST_FIXTURE), path
        fx = np.load(path)
        nx, ny = cc.DESTS[dest]
        assert fx["out"].shape == (cc.NREC, cc.nk_out(vgrid), ny, nx) and fx["iters"].shape == (cc.NREC, cc.NK)
        assert np.all(np.isfinite(fx["out"])) and np.all(np.abs(fx["out"]) < 1e3)          # no missing value survives the fill
        assert np.all(fx["iters"] > 0) and np.all(fx["iters"] < 3999)
        assert len({tuple(r) for r in fx["iters"]}) == cc.NREC                             # the records stop apart
    a, b = (np.load(cc.golden_path("latlon", v)) for v in ("same", "none"))
    assert np.array_equal(bits(a["out"]), bits(b["out"]))                                 # need_interp = 0 leaves the field alone
    recs = cc.records()
    land = recs == cc.MISSING
    assert all(0 < land[r, k].sum() < land[r, k].size for r in range(cc.NREC) for k in range(cc.NK))
    assert any(not np.array_equal(land[r, 0], land[r, k]) for r in range(cc.NREC) for k in range(1, cc.NK))
    assert not np.array_equal(land[0], land[1]) and not np.array_equal(land[1], land[2])


def test_header_declares_and_library_exports_the_new_symbols(fg):
    hdr = open(os.path.join(ROOT, "include", "fregrid_hip.h")).read()
    L = fg.lib()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in fg._lib.EXPORTS and hasattr(L, s), s
    for name in ("ColumnSweep", "set_column_records", "Extrapolator"):
        assert hasattr(fg, name)
    assert hasattr(fg.Extrapolator, "run_batch")


def test_no_gpu_fails_loudly(fg):
    """no CPU fallback: without a device the extrapolator a ColumnSweep or run_batch needs cannot be made, and the C entries
    refuse null handles"""
    if fg.lib().fg_device_count() > 0:
        pytest.skip("a GPU is present")
    lon, lat = cc.source_axes()
    with pytest.raises(fg.FregridHipError) as e:
        fg.Extrapolator(lon, lat, 1).run_batch(cc.records(), cc.MISSING)
    assert e.value.code == -2
    with pytest.raises(fg.FregridHipError) as e:
        fg.ColumnSweep(fg.Extrapolator(lon, lat, 1), [], np.float64, np.float64, z_in=cc.Z1)
    assert e.value.code == -2
    assert fg.lib().fg_extrap_run_batch_dev(None, 1, None, None, 1, 0, 0, cc.MISSING, 0.005, None, None) == -1
    assert fg.lib().fg_column_run(None, None, 1, 0.0, 0.0, cc.MISSING, 0.005, None, None, None) == -1 and fg._lib.last_error()


def test_column_records_hook(fg):
    try:
        assert fg.set_column_records(2) == 2
        assert fg.set_column_records(0) == 0 and fg.set_column_records(-3) == 0
    finally:
        fg.set_column_records(0)
