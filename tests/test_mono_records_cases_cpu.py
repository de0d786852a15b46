"""tests/mono_records_cases.py checked without a device: its bounds records are the neighbourhood bounds mono_levels_cases' plain
loop limits with, partial chunks carry the start values, the real-pair fixture of tests/test_gpu_mono_records.py meets its
preconditions at the seed fixed there, and the library exports the entries those tests call."""
import ctypes

import numpy as np
import pytest

import mono_levels_cases as mc
import mono_records_cases as rc
import sweep_cases as sc

NEW_SYMBOLS = ("fg_c2l_records_levels_mono", "fg_plan_apply_records_levels_mono", "fg_plan_mono_records_reset", "fg_plan_mono_records_begin",
               "fg_plan_mono_records_copy_minmax", "fg_plan_mono_records_end", "fg_sweep_run_levels_mono")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _limited_bounds(c, kw):
    """f_bar_max / f_bar_min as mono_levels_cases.limited takes them (its first four lines)"""
    (nx, ny), = c["tiles"]
    f, missing = kw["data"], kw["missing"]
    L = f.shape[0]
    f3 = f.reshape(L, ny + 2, nx + 2)
    nb = np.stack([f3[:, 1 + dj:1 + dj + ny, 1 + di:1 + di + nx].reshape(L, -1) for dj in (-1, 0, 1) for di in (-1, 0, 1)])
    return np.max(np.where(nb != missing, nb, -1.0e20), axis=0), np.min(np.where(nb != missing, nb, 1.0e20), axis=0)


@pytest.mark.parametrize("name", mc.CASES)
def test_bounds_are_the_plain_loops(name):
    c = sc.make(name)
    for masked in (False, True):
        kw = mc.inputs(name, "none", masked)
        fbmax, fbmin = _limited_bounds(c, kw)
        if masked:                                                    # (the frame of a hand-made list is never missing)
            assert np.any(fbmax[mc.K_NONE] == -1.0e20) and np.any(fbmin[mc.K_NONE] == 1.0e20)
        for k0, nz in ((0, 8), (8, 8), (16, 1), (3, 5)):
            rec, mb, b8, missing = rc.chunk(name, masked, k0, nz)
            assert missing == kw["missing"] and rec.shape == (c["nsrc"], 3, 8) and b8.shape == (c["nsrc"], 4, 8)
            assert np.array_equal(_bits(b8[:, 0, :nz].T), _bits(fbmax[k0:k0 + nz])), (name, masked, k0)
            assert np.array_equal(_bits(b8[:, 1, :nz].T), _bits(fbmin[k0:k0 + nz])), (name, masked, k0)
            # the extremes' rows, and every row of a level >= nz, hold the start values
            assert np.all(b8[:, 2] == -1.0e20) and np.all(b8[:, 3] == 1.0e20)
            assert np.all(b8[:, 0, nz:] == -1.0e20) and np.all(b8[:, 1, nz:] == 1.0e20)
            assert np.all(rec[:, :, nz:] == 0.0)
            field = kw["data"][k0:k0 + nz][:, c["inner"]]
            assert np.array_equal(_bits(rec[:, 0, :nz].T), _bits(field))
            assert np.array_equal(_bits(rec[:, 1, :nz].T), _bits(kw["gx"][k0:k0 + nz])) and np.array_equal(_bits(rec[:, 2, :nz].T), _bits(kw["gy"][k0:k0 + nz]))
            if masked:
                want = np.zeros(c["nsrc"], dtype=np.uint8)
                for k in range(nz):
                    want |= (kw["gm"][k0 + k] != 0).astype(np.uint8) << k
                assert np.array_equal(mb, want) and np.any(mb != 0)
            else:
                assert mb is None
    rec, mb, b8, _ = rc.chunk(name, False, 0, 8, with_gm=True)        # a gradient mask without missing values
    assert mb is not None and np.any(mb != 0)


def test_library_exports_the_new_entries(fg):
    L = ctypes.CDLL(fg._lib.lib_path())
    missing = [s for s in NEW_SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert set(NEW_SYMBOLS) <= set(fg._lib.EXPORTS)


def test_real_pair_preconditions(fg):
    c = rc.check_real_preconditions(fg)
    assert c["ncell"] == 6 * 81 and c["ndst"] == 450 and np.all(c["lens"] > 0)
    assert int(c["gm"].sum()) > 0
    # the bounds records of a partial chunk of the pair
    b8 = rc.bounds8(c["halo"][16:17], c["tiles"], rc.MISSING, 1)
    assert np.all(b8[:, :, 1:] == np.array([-1.0e20, 1.0e20, -1.0e20, 1.0e20])[None, :, None])
    assert np.any(b8[:, 0, 0] != -1.0e20)
