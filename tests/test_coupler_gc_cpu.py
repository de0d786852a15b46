"""CPU side of the great-circle coupler (CouplerMosaic(clip_method="great_circle"), fg_coupler_create_gc): ties the _cr restatement
the GPU test compares with (tests/test_gpu_coupler_gc.py) to the compiled reference.

* tests/coupler_gc_cases.py run over the compiled reference's primitives and over the _cr oracle's gives identical index lists on
  every case.  Every weighted single-clip term (a clipped polygon's area times a fraction) is compared: the same polygon bit for
  bit, and an unweighted area that differs in bits accounted for singly by gc_cases.account's three conditions, whatever the
  fraction.  An atmosphere x land entry, a per-cell sum (a_area, l_area, o_area) and a mask (sum / cell area) may then differ by no
  more than the differences of exactly the terms they add up (plus the roundings of those additions, and none at all where no term
  differs: bit equality); cell areas that differ are accounted for like terms.
* every tenth pair the restatement skipped by the range test -- atmosphere x land, atmosphere x ocean, remembered polygon x ocean,
  land x ocean -- is given to the reference's clip: 0.
* teeth: reversing the summation order of the cells changes o_area (and not l_area, whose cells collect one term each on same_c5).
  A MISSING TOOTH: clipping the lnd_same_as_atm cell instead of copying it was expected to change bits and changes nothing on
  same_c5 -- the clip of a cell with itself returns its corners bit for bit -- so no test here separates the copy from a clip;
  the test records that finding instead.
* the library exports the new entry and refuses interp_order 2 before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import coupler_gc_cases as cg
import gc_cases
import orc
import polylist_gc_cases as pc

needs_ref = pytest.mark.skipif(not orc.ref_available(), reason="the compiled reference has not been built")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _lists(r):
    return [t for row in r["axl"] for t in row] + r["axo"] + r["lxo"]


def _sum_bound(addend_bounds, largest):
    """Two sums of the same number of non-negative addends, added in the same order, whose addends differ by at most addend_bounds:
    if no addend differs the operations are the same and so are the bits (bound 0); otherwise the sums differ by at most the sum of
    the addends' differences plus, per addition, the two roundings (half an ulp of a partial sum each, and no partial sum exceeds
    the final one)."""
    tot = float(sum(addend_bounds))
    return 0.0 if tot == 0.0 else tot + len(addend_bounds) * float(np.spacing(largest))


def _account_terms(name, a, b):
    """every weighted single-clip term of the two restatements: the same clipped polygon; an unweighted area that differs in bits is
    accounted for by gc_cases.account's three conditions; returns |w_ref - w_cr| per term and how many differ"""
    assert len(a["terms"]) == len(b["terms"])
    d = np.zeros(len(a["terms"]))
    n = 0
    for k, (ta, tb) in enumerate(zip(a["terms"], b["terms"])):
        assert np.array_equal(_bits(ta["v"]), _bits(tb["v"])), (name, k)
        if _bits(ta["ua"]) != _bits(tb["ua"]):
            why = gc_cases.account(ta["v"], ta["ua"], tb["ua"])
            assert why is None, f"{name}: term {k}: {why}"
            n += 1
            d[k] = abs(ta["w"] - tb["w"])
            # the weight is one multiplication by the same fraction <= 1 on both sides
            assert d[k] <= abs(ta["ua"] - tb["ua"]) + np.spacing(max(ta["w"], tb["w"])), (name, k)
        else:
            assert _bits(ta["w"]) == _bits(tb["w"]), (name, k)
    return d, n


def _account_cell_areas(name, grid, area_a, area_b):
    """get_grid_great_circle_area of one grid under the two primitive sets: a cell whose area differs is accounted for like a term"""
    area_a, area_b = np.asarray(area_a).reshape(-1), np.asarray(area_b).reshape(-1)
    for c in np.nonzero(_bits(area_a) != _bits(area_b))[0]:
        why = gc_cases.account(gc_cases.dedup(grid.cells[c]), area_a[c], area_b[c])
        assert why is None, f"{name}: cell {c}: {why}"


def _check_cells(name, what, sum_a, sum_b, area_a, area_b, mask_a, mask_b, bounds):
    """per cell: the sum within the bound its entries give; the mask = sum / cell area within what follows for a quotient"""
    sum_a, sum_b, area_a, area_b, mask_a, mask_b = (np.asarray(v).reshape(-1) for v in (sum_a, sum_b, area_a, area_b, mask_a, mask_b))
    for c in range(sum_a.size):
        bs = _sum_bound(bounds.get(c, []), max(sum_a[c], sum_b[c]))
        assert abs(sum_a[c] - sum_b[c]) <= bs, (name, what, c, sum_a[c], sum_b[c], bs)
        if mask_a is None:
            continue
        if bs == 0.0 and _bits(area_a[c]) == _bits(area_b[c]):
            assert _bits(mask_a[c]) == _bits(mask_b[c]), (name, what, "mask", c)
        else:                                                   # |s/A - s'/A'| <= |s - s'| / A + s' |A - A'| / (A A'), and one rounding each
            bm = bs / min(area_a[c], area_b[c]) + max(sum_a[c], sum_b[c]) * abs(area_a[c] - area_b[c]) / (area_a[c] * area_b[c])
            bm = bm * (1 + 1e-15) + 2 * float(np.spacing(max(mask_a[c], mask_b[c], 1e-300)))
            assert abs(mask_a[c] - mask_b[c]) <= bm, (name, what, "mask", c, mask_a[c], mask_b[c], bm)


@needs_ref
@pytest.mark.parametrize("name", list(cg.CASES))
def test_reference_and_cr_restatements_agree(fg, name):
    R = pc.prims_ref()
    c, a = cg.reference_of(name, fg, R, want_skipped=True)
    _, b = cg.reference_of(name, fg, pc.prims_oracle(True))
    assert a["cover"] == b["cover"] and a["nbad"] == b["nbad"]
    for ta, tb in zip(_lists(a), _lists(b)):
        for key in ta:
            if key != "area":
                assert np.array_equal(ta[key], tb[key]), key
    assert len(a["skipped"]) > 1000
    for p, q in a["skipped"][::10]:                             # the range test is the clip's own first test: every tenth skipped pair
        assert R.clip(p, q)[0] == 0
    d, ndiff = _account_terms(name, a, b)
    print(name, "terms", len(d), "differing", ndiff, "skipped pairs", len(a["skipped"]))
    atm, lnd, ocn = c["atm"], c["lnd"] or c["atm"], c["ocn"]
    # the entries: an atmosphere x ocean or land x ocean entry is one term, an atmosphere x land entry the ordered sum of its terms
    entry = {}
    o_b, l_b, a_b = {}, [dict() for _ in lnd], [dict() for _ in atm]
    for na, (ta, tb) in enumerate(zip(a["axo"], b["axo"])):
        for i in range(len(ta["area"])):
            bound = float(d[ta["tid"][i]])
            assert abs(ta["area"][i] - tb["area"][i]) <= bound
            o_b.setdefault(int(ta["jo"][i] * ocn.nx + ta["io"][i]), []).append(bound)
            entry[("axo", na, i)] = bound
    for nl, (ta, tb) in enumerate(zip(a["lxo"], b["lxo"])):
        for i in range(len(ta["area"])):
            assert abs(ta["area"][i] - tb["area"][i]) <= float(d[ta["tid"][i]])
    for na in range(len(atm)):
        for nl in range(len(lnd)):
            ta, tb = a["axl"][na][nl], b["axl"][na][nl]
            assert a["axl_tids"][na][nl] == b["axl_tids"][na][nl]
            for i in range(len(ta["area"])):
                bound = _sum_bound([d[t] for t in a["axl_tids"][na][nl][i]], max(ta["area"][i], tb["area"][i]))
                assert abs(ta["area"][i] - tb["area"][i]) <= bound, (name, "axl", na, nl, i)
                l_b[nl].setdefault(int(ta["jl"][i] * lnd[nl].nx + ta["il"][i]), []).append(bound)
                a_b[na].setdefault(int(ta["ja"][i] * atm[na].nx + ta["ia"][i]), []).append(bound)
        ta = a["axo"][na]
        for i in range(len(ta["area"])):
            a_b[na].setdefault(int(ta["ja"][i] * atm[na].nx + ta["ia"][i]), []).append(entry[("axo", na, i)])
    # cell areas, per-cell sums and masks
    _account_cell_areas(name, ocn, a["ocean"]["area"], b["ocean"]["area"])
    _check_cells(name, "o_area", a["ocean"]["o_area"], b["ocean"]["o_area"], a["ocean"]["area"], b["ocean"]["area"], a["ocean"]["mask"], b["ocean"]["mask"], o_b)
    for nl, g in enumerate(lnd):
        _account_cell_areas(name, g, a["land"][nl]["area"], b["land"][nl]["area"])
        _check_cells(name, ("l_area", nl), a["land"][nl]["l_area"], b["land"][nl]["l_area"], a["land"][nl]["area"], b["land"][nl]["area"],
                     a["land"][nl]["mask"], b["land"][nl]["mask"], l_b[nl])
    for na, g in enumerate(atm):
        _account_cell_areas(name, g, a["atmos"][na]["area"], b["atmos"][na]["area"])
        x, y = a["atmos"][na], b["atmos"][na]
        _check_cells(name, ("a_area", na), x["a_area"], y["a_area"], x["area"], y["area"], x["a_area"] / x["area"], y["a_area"] / y["area"], a_b[na])


@needs_ref
def test_teeth_same_copy_and_summation_order(fg):
    P = pc.prims_oracle(True)
    c, good = cg.reference_of("same_c5", fg, P)
    _, clipped = cg.reference_of("same_c5", fg, P, skip_same_copy=True)
    _, reverse = cg.reference_of("same_c5", fg, P, reverse_sums=True)
    differ = lambda x, y: int(np.count_nonzero(_bits(x) != _bits(y))) if x.shape == y.shape else -1
    # Clipping the lnd_same_as_atm cell instead of copying it (:1426-1437) was expected to change bits.  On this case it does not:
    # clip_2dx2d_great_circle(cell, cell) returns the four corners of each of the 150 cells bit for bit and in the same order (every
    # corner is "inside", the walk starts at corner 0), so remembered polygons, areas and lists are the same.  Recorded as found.
    assert all(differ(x["area"], y["area"]) == 0 for rx, ry in zip(good["axl"], clipped["axl"]) for x, y in zip(rx, ry))
    assert all(differ(x["area"], y["area"]) == 0 for x, y in zip(good["axo"], clipped["axo"]))
    for g in c["atm"]:
        for cell in g.cells[::7]:
            n, v = P.clip(cell, cell)
            assert n == 4 and np.array_equal(_bits(v), _bits(cell))
    # the order of the sums: o_area collects several terms per cell, l_area (one atmosphere x land cell per land cell here) one
    assert differ(good["ocean"]["o_area"], reverse["ocean"]["o_area"]) > 0
    assert differ(good["land"][0]["l_area"], reverse["land"][0]["l_area"]) == 0


def test_new_entry_exists_and_wants_order_1(fg):
    L = fg.lib()
    assert hasattr(L, "fg_coupler_create_gc") and "fg_coupler_create_gc" in fg._lib.EXPORTS
    lo, la = fg.latlon_corners(4, 2)
    dp = C.POINTER(C.c_double)
    one = (C.c_int * 1)
    tab = lambda a: (dp * 1)(a.ctypes.data_as(dp))
    om = np.ones(8)
    h = C.c_void_p()
    rc = L.fg_coupler_create_gc(2, 1.0e-6, 1, one(4), one(2), tab(lo), tab(la), 0, None, None, None, None, 4, 2, lo.ctypes.data_as(dp),
                                la.ctypes.data_as(dp), om.ctypes.data_as(dp), 0, 0, C.byref(h))
    assert rc == -1 and "interp_order = 1" in fg._lib.last_error() and not h.value      # FG_ERR_ARG, :593
