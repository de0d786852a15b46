"""CPU side of the great-circle polygon-list plan: ties the _cr oracle the GPU test compares with (tests/test_gpu_polylist_gc.py) to
the compiled reference, on the very inputs of that test.

* The restatement of tests/polylist_gc_cases.py over the compiled reference's primitives and over the _cr oracle gives the same
  lists, vertex counts and vertices; every area that differs in bits is accounted for singly by gc_cases.account (an angle rounded
  the other way by one ulp, the area within the bound that follows).
* Every tenth pair the restatement skipped by the clip's range test is given to the reference's clip: it returns 0.
* The library exports the new entries and refuses a polygon of 9 vertices before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import gc_cases
import orc
import polylist_gc_cases as pc

needs_ref = pytest.mark.skipif(not orc.ref_available(), reason="the compiled reference has not been built")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_lists_areas_accounted(a, b):
    """a: the reference's list, b: the _cr oracle's.  Returns how many areas differ."""
    for key in ("poly", "cell", "nv"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(_bits(a["verts"]), _bits(b["verts"]))
    differ = np.nonzero(_bits(a["area"]) != _bits(b["area"]))[0]
    for k in differ:
        why = gc_cases.account(a["verts"][k, :a["nv"][k]], a["area"][k], b["area"][k])
        assert why is None, f"exchange cell {k}: {why}"
    return len(differ)


@needs_ref
def test_own_c4_reference_and_cr_oracle_agree(fg):
    c = pc.own_c4(fg)
    R, O = pc.prims_ref(), pc.prims_oracle(True)
    ra, rb = pc.remembered_polygons(c["atm"], c["lnd"], R), pc.remembered_polygons(c["atm"], c["lnd"], O)
    assert ra["cover"] == rb["cover"] and ra["cover"].get(3, 0) >= 1 and sum(v for k, v in ra["cover"].items() if k >= 6) >= 1
    assert np.array_equal(ra["n"], rb["n"]) and np.array_equal(ra["ia"], rb["ia"]) and np.array_equal(ra["il"], rb["il"])
    assert np.array_equal(_bits(ra["xyz"]), _bits(rb["xyz"]))
    # (area_ref = min(area_lnd, area_atm) of get_grid_great_circle_area: tests/test_gc_oracle_cr_cpu.py accounts for those)
    # the polygons of the _cr run against the ocean, under both primitive sets (the same polygons and reference areas for both)
    la = pc.polylist_reference(rb["n"], rb["xyz"], rb["area_ref"], c["ocn"], R, want_skipped=True)
    lb = pc.polylist_reference(rb["n"], rb["xyz"], rb["area_ref"], c["ocn"], O)
    assert not la["errors"] and not lb["errors"] and len(la["poly"]) > 1000
    _same_lists_areas_accounted(la, lb)
    assert max(la["cover"]) >= 6
    for k, d in la["skipped"][::10]:                                                # the range test is the clip's own first test
        assert R.clip(rb["xyz"][k, :rb["n"][k]], c["ocn"].cells[d])[0] == 0


@needs_ref
def test_crafted_batch_reference_and_cr_oracle_agree(fg):
    dst, kinds, n, xyz = pc.crafted(fg)
    plain = pc.prims_oracle(False)
    bad = pc.polylist_reference(n, xyz, np.ones(len(n)), dst, plain)["errors"]      # where the reference's clip would end the process
    assert len(bad) <= 1, [kinds[k] for k in bad]
    keep = [k for k in range(len(n)) if k not in bad]
    n, xyz = n[keep], xyz[keep]
    R, O = pc.prims_ref(), pc.prims_oracle(True)
    area_ref = np.array([pc.own_area(xyz[k, :n[k]], O) for k in range(len(n))])
    la, lb = pc.polylist_reference(n, xyz, area_ref, dst, R), pc.polylist_reference(n, xyz, area_ref, dst, O)
    assert not la["errors"] and not lb["errors"]
    _same_lists_areas_accounted(la, lb)
    assert not np.any(la["poly"] == [kinds[k] for k in keep].index("antipodal"))


def test_new_entries_exist_and_check_their_arguments(fg):
    L = fg.lib()
    assert hasattr(L, "fg_plan_create_polylist_gc") and hasattr(L, "fg_plan_create_polylist_gc_dev")
    assert "fg_plan_create_polylist_gc" in fg._lib.EXPORTS
    dst, kinds, n, xyz = pc.crafted(fg)
    n9 = n.copy()
    n9[2] = 9
    dp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_double))
    v = [np.ascontiguousarray(xyz[:, :, k]) for k in range(3)]
    h = C.c_void_p()
    rc = L.fg_plan_create_polylist_gc(len(n9), n9.ctypes.data_as(C.POINTER(C.c_int)), dp(v[0]), dp(v[1]), dp(v[2]), dp(np.ones(len(n9))), dst.nx, dst.ny,
                                      dp(dst.lon), dp(dst.lat), 0, C.byref(h))
    assert rc == -1 and "9 vertices" in fg._lib.last_error() and not h.value      # FG_ERR_ARG
