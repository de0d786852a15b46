"""d_poly_area_ctr (csrc/geom.hip.h), the one-pass area and centroid integrals of the order-2 clip kernels, which evaluates every
latitude's trig variants from one reduction (fgs_trig, csrc/sincos_glibc.h):
(a) through fg_poly_op_batch's probe ops 4, 5, 6 against the three separate routines (ops 0, 1, 2) on hand-made polygons that
    reach every branch of the loop -- equal in bits;
(b) the kernels that call it -- k_clip_quad<2, .> and k_clip_general<2, .> -- on the smallest grids that reach every latitude
    range: C12 -> 36x18, on the rectilinear and on the generic path, against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
STRIDE = 24                                    # FG_POLY_STRIDE: a polygon is a row of [npoly][24]
HPI = 0.5 * np.pi


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _convex(rng, n, lon0, lat0, r):
    """n vertices on an ellipse around (lon0, lat0), counter-clockwise, latitudes kept on the sphere"""
    t = np.sort(rng.uniform(0, 2 * np.pi, n))
    t += np.arange(n) * 1e-3                   # no two vertices coincide
    lat = np.clip(lat0 + r * np.sin(t), -HPI, HPI)
    lon = lon0 + r * np.cos(t) / max(np.cos(lat0), 0.05)
    return lon, lat


def _box(lon0, lon1, lat0, lat1):
    return np.array([lon0, lon1, lon1, lon0]), np.array([lat0, lat0, lat1, lat1])


def make_polygons():
    """-> n [N] int32, lon / lat [N, 24], clon [N], and the name of every polygon's family"""
    rng = np.random.default_rng(20)
    P, fam = [], []

    def add(name, lon, lat, clon=None):
        lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
        assert 3 <= lon.size <= 8 and lon.size == lat.size and np.all(np.abs(lat) <= HPI)
        P.append((lon, lat, float(np.mean(lon)) if clon is None else float(clon))); fam.append(name)

    for i in range(1200):                      # 3..8 vertices anywhere on the sphere
        lon, lat = _convex(rng, 3 + i % 6, rng.uniform(0, 2 * np.pi), rng.uniform(-1.5, 1.5), 10 ** rng.uniform(-3, -0.5))
        add("convex", lon, lat)
    for i in range(600):                       # flat edges: equal latitudes, and |dlat| around both 1e-10 thresholds
        la0 = rng.uniform(-1.5, 1.4); lo0 = rng.uniform(0, 6)
        lon, lat = _box(lo0, lo0 + rng.uniform(0.01, 0.3), la0, la0 + rng.uniform(0.005, 0.1))
        eps = (0.0, 3e-11, -7e-11, 1.5e-10, 1.9e-10, 2.5e-10)[i % 6]   # poly_area tests |dlat|, poly_ctrlat |dlat| / 2
        lat[1] += eps; lat[3] -= eps
        add("flat", lon, lat)                  # (its sides are meridian edges: dlon = 0 exactly)
    for i in range(200):                       # meridian edges on polygons that are no boxes
        lon, lat = _convex(rng, 5 + i % 4, rng.uniform(0, 6), rng.uniform(-1.3, 1.3), 0.05)
        lon[1] = lon[0]; lon[3] = lon[4]
        add("meridian", lon, lat)
    for i in range(200):                       # an edge with |dlon| = pi (poly_area adds pi for it)
        la = rng.uniform(-1.4, 1.4, 2); lo0 = (0.0, 0.5, 1.0, 3.0)[i % 4]
        mid = lo0 + rng.uniform(0.5, 2.5)
        lon = np.array([lo0, mid, lo0 + np.pi]) if i % 2 else np.array([lo0 + np.pi, mid, lo0])
        add("dlon_pi", lon, [la[0], rng.uniform(-1.4, 1.4), la[1]])
    for i in range(300):                       # a vertex at a pole
        s = 1.0 if i % 2 else -1.0
        lo0 = rng.uniform(0, 6); w = rng.uniform(0.02, 0.5); la = s * (HPI - 10 ** rng.uniform(-7, -0.5))
        if i % 3 == 0:
            add("pole", [lo0, lo0 + w, lo0 + 0.5 * w], [la, la, s * HPI])
        elif i % 3 == 1:                       # the pole as fix_lon leaves it: twice, at the neighbours' longitudes
            add("pole", [lo0, lo0 + w, lo0 + w, lo0], [la, la + s * 1e-3 * (HPI - abs(la)), s * HPI, s * HPI])
        else:
            lon, lat = _convex(rng, 6, lo0, s * 1.45, 0.2)
            lat[2] = s * HPI
            add("pole", lon, lat)
    for i in range(600):                       # latitudes on both sides of +-0.126 and +-0.855 (and of pi/2 - 0.126) in one polygon
        c = (0.126, -0.126, 0.85546875, -0.85546875, HPI - 0.126, 0.126 - HPI)[i % 6]
        lon, lat = _convex(rng, 3 + i % 6, rng.uniform(0, 6), c + rng.uniform(-1, 1) * 1e-3, 10 ** rng.uniform(-2.5, -1))
        add("threshold", lon, lat)
    for i in range(300):                       # within 1e-7 of the equator: latitudes around 2^-26 and 2^-27, and zero
        h = (1e-7, 2e-8, 1e-8, 5e-9, 1e-9)[i % 5]
        lon, lat = _convex(rng, 3 + i % 6, rng.uniform(0, 6), 0.0, 0.1)
        lat = rng.uniform(-h, h, lat.size)
        if i % 4 == 0: lat[0] = 0.0
        if i % 8 == 0: lat[1] = -0.0
        add("equator", lon, lat)
    for i in range(600):                       # clon more than pi from the vertices, and just about pi (the fint branch of ctrlon)
        lo0 = rng.uniform(0, 6); r = 10 ** rng.uniform(-2, -0.7)
        lon, lat = _convex(rng, 3 + i % 6, lo0, rng.uniform(-1.2, 1.2), r)
        clon = lo0 + (4.0, -4.5, np.pi + rng.uniform(-r, r), -np.pi + rng.uniform(-r, r))[i % 4]
        add("far_clon", lon, lat, clon)
    N = len(P)
    n = np.array([p[0].size for p in P], dtype=np.int32)
    lon, lat = np.zeros((N, STRIDE)), np.zeros((N, STRIDE))
    for k, p in enumerate(P):
        lon[k, :n[k]] = p[0]; lat[k, :n[k]] = p[1]
    return n, lon, lat, np.array([p[2] for p in P]), np.array(fam)


def _poly_op(fg, op, n, lon, lat, clon):
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    res = np.full(n.size, np.nan)
    a, b, m = lon.copy(), lat.copy(), n.copy()
    rc = fg.lib().fg_poly_op_batch(op, n.size, dp(a), dp(b), m.ctypes.data_as(C.POINTER(C.c_int)), dp(clon), dp(res))
    assert rc == 0, fg._lib.last_error()
    return res


def test_fused_integrals_equal_the_separate_routines(fg, gpu_ok):
    n, lon, lat, clon, fam = make_polygons()
    assert 3000 <= n.size <= 6000 and set(np.unique(n)) == set(range(3, 9))
    # the families hold what they are named for
    dlat = np.abs(lat - np.roll(lat, 1, axis=1))[:, 1:4]
    assert np.any(dlat[fam == "flat"] == 0.0) and np.any((dlat[fam == "flat"] > 1e-10) & (dlat[fam == "flat"] < 2e-10))
    assert np.any(np.abs(lat[fam == "pole"]) == HPI)
    for k in np.flatnonzero(fam == "threshold")[:6]:
        v = np.abs(lat[k, :n[k]])
        assert any(v.min() < c < v.max() for c in (0.126, 0.85546875, HPI - 0.126))
    assert np.max(np.abs(lat[fam == "equator"])) <= 1e-7
    for name, spec_op, fused_op in (("area", 0, 4), ("ctrlon", 1, 5), ("ctrlat", 2, 6)):
        want = _poly_op(fg, spec_op, n, lon, lat, clon)
        got = _poly_op(fg, fused_op, n, lon, lat, clon)
        assert np.all(np.isfinite(want)) and np.count_nonzero(want) > 0.9 * n.size, name
        bad = np.flatnonzero(_bits(want) != _bits(got))
        assert bad.size == 0, (name, bad.size, sorted(set(fam[bad])), int(bad[0]), want[bad[0]], got[bad[0]])


# ------------------------------------------------------------------------------------------------- (b) the clip kernels
NI, NLON, NLAT = 12, 36, 18
_oracle = {}


def _c12_oracle(fg):
    """the six tiles' exchange cells from the CPU oracle, computed once"""
    if not _oracle:
        lon, lat = fg.gnomonic_ed_corners(NI)
        lo, la = fg.latlon_corners(NLON, NLAT)
        tiles = [orc.orc_create_xgrid(2, NI, NI, NLON, NLAT, lon[t], lat[t], lo, la) for t in range(6)]
        _oracle.update(lon=lon, lat=lat, lo=lo, la=la, tiles=tiles)
    return _oracle


@pytest.mark.parametrize("rect", [1, 0], ids=["rectilinear", "generic"])
def test_c12_clip_kernels_against_the_cpu_oracle(fg, gpu_ok, rect):
    o = _c12_oracle(fg)
    grids = [fg.GridConfig(NI, NI, o["lon"][t], o["lat"][t]) for t in range(6)]
    L = fg.lib()
    L.fg_set_search_rect(rect)
    try:
        p = fg.XgridPlan.create(2, grids, fg.GridConfig(NLON, NLAT, o["lo"], o["la"]))
        x = p.get_xgrid()                          # before finalize: c1 / c2 are the centroid integrals
        st = p.stats()
        p.destroy()
    finally:
        L.fg_set_search_rect(1)
    print("C12 -> 36x18 order 2, rect", rect, "stats", st)
    assert (st["bins"] == 0) == bool(rect), "the two runs must take different search paths"
    if not rect:
        # the pole-fixed source cells (5 vertices) cannot go through the generic quad kernel: k_clip_general<2, .> has run.
        # (The rectilinear quad kernel takes source cells of up to 8 vertices itself; it defers nothing on these grids.)
        assert st["deferred"] >= 1
    assert len(x["area"]) == sum(t["n"] for t in o["tiles"])
    lats = np.abs(o["lat"])
    assert lats.min() < 0.126 and np.any((lats > 0.126) & (lats < 0.855)) and lats.max() > HPI - 0.126
    off = 0
    for t, r in enumerate(o["tiles"]):
        sel = slice(off, off + r["n"])
        assert np.all(x["t_in"][sel] == t)
        for k in ("i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(x[k][sel], r[k]), (t, k)
        for a, k in ((x["area"][sel], "area"), (x["c1"][sel], "clon"), (x["c2"][sel], "clat")):
            if orc.host_has_fma():
                assert np.array_equal(_bits(a), _bits(r[k])), (t, k)
            else:
                assert np.max(np.abs(a - r[k])) <= 1e-10 * np.max(np.abs(r[k])), (t, k)
        off += r["n"]
