"""The great-circle oracle that rounds like the device (gc_oracle.c's second build, orc_*_cr: the same text with csrc/fp80.h's
correctly rounded fg_acosl for libm's acosl) against the plain build, which is pinned bit for bit to the compiled reference
(tests/test_oracle_vs_ref.py).  On every grid pair the exchange-cell lists must be identical, and every exchange-cell or grid-cell
area that differs in bits is accounted for singly: its polygon is clipped again, its angles are taken with both arc cosines, and
(a) at least one angle differs, (b) each differing angle by exactly one double ulp, (c) the areas by no more than
n (ulp(pi) + ulp(S)) R^2 (gc_cases.account).  No cap on how many differ: an area that differs for any other reason fails.
The GPU tests then hold the device to the _cr build in all values (tests/test_gpu_great_circle.py and others).

Measured here (x86-64, glibc's acosl = x87 fpatan): see DESIGN.md section 6 for the table; -s prints the counts per case."""

import numpy as np
import pytest

import gc_cases
import orc
from gc_cases import bits


@pytest.fixture(scope="module")
def cases(fg):
    """name -> (args, mask)"""
    out = {k: (v, None) for k, v in gc_cases.grid_cases(fg).items()}
    out.update({k: (v, None) for k, v in zip(gc_cases.AWKWARD_NAMES, gc_cases.awkward_pairs(fg))})
    out.update(gc_cases.degenerate_cases(fg))
    return out


CASE_NAMES = ["c24_tile1_144x90", "c24_tile3_polar_144x90", "latlon_aligned_2x", "latlon_regional_offset", "latlon_to_cubed_polar",
              "tripolar_to_cubed"] + gc_cases.AWKWARD_NAMES + ["identical_latlon", "identical_cubed", "disjoint", "single_cells",
                                                               "fully_masked", "masked_cubed_to_latlon"]


def _xyz(lon, lat):
    lon, lat = orc.f64(lon).ravel(), orc.f64(lat).ravel()
    x, y, z = (np.empty(lon.size) for _ in range(3))
    orc.oracle().orc_latlon2xyz(lon.size, orc._dp(lon), orc._dp(lat), orc._dp(x), orc._dp(y), orc._dp(z))
    return np.stack([x, y, z], -1)


def _cell(v, nxp, i, j):
    """create_xgrid.c:1413-1420"""
    return np.array([v[j * nxp + i], v[(j + 1) * nxp + i], v[(j + 1) * nxp + i + 1], v[j * nxp + i + 1]])


_RESULTS = {}


def _run(name, args, mask):
    """both builds on one grid pair; every difference accounted for.  Returns (n exchange cells, differing exchange cells,
    grid cells, differing grid cells, largest |d area| in m^2)."""
    if name in _RESULTS:
        return _RESULTS[name]
    nx1, ny1, nx2, ny2, lo1, la1, lo2, la2 = args
    err = []
    outs = []
    for cr in (False, True):
        try:
            outs.append(orc.orc_create_xgrid_gc(*args, mask=mask, cr=cr))
        except RuntimeError as e:            # one of the reference's fatal checks on this input: the same one in both builds
            outs.append(None)
            err.append(str(e))
    if err:
        assert len(err) == 2 and err[0] == err[1], (name, err)
        _RESULTS[name] = None
        return None
    p, c = outs
    assert p["n"] == c["n"], (name, p["n"], c["n"])
    for k in ("i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(p[k], c[k]), (name, k)
    if orc.ref_available():
        r = orc.ref_create_xgrid_gc(*args, mask=mask)
        assert r["n"] == p["n"], (name, r["n"], p["n"])
        for k in ("i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(r[k], p[k]), (name, k)
        assert np.array_equal(bits(r["area"]), bits(p["area"])), name      # the plain build is the reference's, still
    v1, v2 = _xyz(lo1, la1), _xyz(lo2, la2)
    m = np.ones(nx1 * ny1) if mask is None else orc.f64(mask).ravel()
    if p["n"] and nx1 * ny1 * nx2 * ny2 <= 30 * 20 * 45 * 33:
        # orc_gc_pair_areas (the full-size GPU test's way to the _cr areas of a row) is the list's area before the mask
        for cr, x in ((False, p), (True, c)):
            pa = orc.orc_gc_pair_areas(nx1, lo1, la1, nx2, lo2, la2, x["i_in"], x["j_in"], x["i_out"], x["j_out"], cr=cr)
            assert np.array_equal(bits(pa * m[x["j_in"].astype(np.int64) * nx1 + x["i_in"]]), bits(x["area"])), (name, cr)
    worst = 0.0
    xd = np.flatnonzero(bits(p["area"]) != bits(c["area"]))
    for k in xd:
        i1, j1, i2, j2 = (int(p[q][k]) for q in ("i_in", "j_in", "i_out", "j_out"))
        n, poly = orc.orc_clip_gc(_cell(v1, nx1 + 1, i1, j1), _cell(v2, nx2 + 1, i2, j2))
        assert n >= 3, (name, k, n)
        scale = m[j1 * nx1 + i1]
        # the polygon is the one whose area the list holds
        assert orc.orc_great_circle_area(*poly.T) * scale == p["area"][k] and orc.orc_great_circle_area(*poly.T, cr=True) * scale == c["area"][k]
        why = gc_cases.account(poly, p["area"][k], c["area"][k], scale)
        assert why is None, (name, "exchange cell", int(k), (i1, j1, i2, j2), why, poly.tolist())
        worst = max(worst, abs(p["area"][k] - c["area"][k]))
    ngrid = gd = 0
    for nx, ny, lo, la, v in ((nx1, ny1, lo1, la1, v1), (nx2, ny2, lo2, la2, v2)):
        ap, ac = orc.orc_get_grid_gc_area(nx, ny, lo, la), orc.orc_get_grid_gc_area(nx, ny, lo, la, cr=True)
        if orc.ref_available():
            assert np.array_equal(bits(orc.ref_get_grid_gc_area(nx, ny, lo, la)), bits(ap)), name
        ngrid += nx * ny
        for k in np.flatnonzero(bits(ap) != bits(ac)):
            j, i = divmod(int(k), nx)
            poly = gc_cases.dedup(_cell(v, nx + 1, i, j))
            assert orc.orc_great_circle_area(*poly.T) == ap[k] and orc.orc_great_circle_area(*poly.T, cr=True) == ac[k]
            why = gc_cases.account(poly, ap[k], ac[k])
            assert why is None, (name, "grid cell", (i, j), why, poly.tolist())
            worst = max(worst, abs(ap[k] - ac[k]))
            gd += 1
    _RESULTS[name] = (p["n"], len(xd), ngrid, gd, worst)
    return _RESULTS[name]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cr_oracle_against_the_pinned_one(cases, name):
    args, mask = cases[name]
    r = _run(name, args, mask)
    if r is None:
        print(f"{name}: both builds stop at the same fatal check of the reference")
        return
    print(f"{name}: {r[1]} of {r[0]} exchange-cell areas and {r[3]} of {r[2]} grid-cell areas differ, at most {r[4]:.3g} m^2")
    if name in ("disjoint", "fully_masked"):
        assert r[0] == 0
    else:
        assert r[0] > 0


def test_the_two_builds_are_different_oracles(cases):
    """Over all cases at least one exchange-cell area differs (latlon_regional_offset has one): otherwise the tests above would
    not show that the second build takes another arc cosine."""
    tot = np.zeros(4, dtype=np.int64)
    worst = 0.0
    for name in CASE_NAMES:
        r = _run(name, *cases[name])
        if r is not None:
            tot += r[:4]
            worst = max(worst, r[4])
    print(f"total: {tot[1]} of {tot[0]} exchange-cell areas and {tot[3]} of {tot[2]} grid-cell areas differ, at most {worst:.3g} m^2")
    assert tot[1] > 0
    assert _RESULTS["latlon_regional_offset"][1] > 0


def test_crafted_batch_reaches_the_hard_arguments():
    """The crafted batch (gc_cases.crafted_batch; the GPU test puts it through fg_gc_clip_batch): no pair stops at a fatal check,
    the clipped polygons have interior angles within 1e-6 of 0 and of pi -- exactly 0 / pi (the argument snapped to +-1) and next
    to them (through the arc cosine) -- besides ordinary ones, the two builds clip the same polygons, and every area that differs
    is accounted for.  Measured: 3028 pairs, 2654 polygons, 11701 angles, 28 areas differ (all in the `rounding` family, which is made of
    such cells; the 3000 pairs of the other families hold none, one polygon in about ten thousand differs)."""
    a, b, fam = gc_cases.crafted_batch()
    assert 2000 < len(a) < 10000
    ang = []
    npoly = ndiff = 0
    per_family = {}
    for q in range(len(a)):
        n, v = orc.orc_clip_gc(a[q], b[q])
        n2, v2 = orc.orc_clip_gc(a[q], b[q], cr=True)
        assert n >= 0 and n != 1 and n != 2, (q, fam[q], n)
        assert n == n2 and np.array_equal(bits(v), bits(v2)), (q, fam[q])
        if n == 0:
            continue
        npoly += 1
        ang.append(gc_cases.polygon_angles(v, False))
        ap, ac = orc.orc_great_circle_area(*v.T), orc.orc_great_circle_area(*v.T, cr=True)
        if ap != ac:
            why = gc_cases.account(v, ap, ac)
            assert why is None, (q, fam[q], why, v.tolist())
            ndiff += 1
            per_family[str(fam[q])] = per_family.get(str(fam[q]), 0) + 1
    ang = np.concatenate(ang)
    print(f"crafted batch: {len(a)} pairs, {npoly} polygons, {len(ang)} angles, {ndiff} areas differ between the arc cosines {per_family}; "
          f"angles: {np.sum(ang < 1e-6)} within 1e-6 of 0 ({np.sum((ang > 0) & (ang < 1e-6))} not 0), "
          f"{np.sum(ang > np.pi - 1e-6)} within 1e-6 of pi ({np.sum((ang > np.pi - 1e-6) & (ang < np.pi))} not pi)")
    assert ndiff > 0
    assert np.sum((ang > 0) & (ang < 1e-6)) > 0 and np.sum((ang > np.pi - 1e-6) & (ang < np.pi)) > 0
    assert np.sum((ang > 0.1) & (ang < np.pi - 0.1)) > 1000
    assert set(fam) == {"shifted", "turned", "pole", "thin", "sliver", "ordinary", "rounding"}
