"""The rectilinear quad clip (d_clip_quad_sh<RECT>, csrc/xgrid_kernels.hip) tests a vertex against an axis-aligned cutting edge with
one product instead of d_inside_edge's two (create_xgrid.c:2342-2350):

    horizontal edge (y1 == y0):  (x0 - x1) * (y - y0) <= 1e-12
    vertical edge   (x1 == x0):  (x - x0) * (y1 - y0) <= 1e-12

The other product has an exact zero for a factor, and adding +-0 cannot move a sum across the threshold.  Checked here in numpy, no
GPU: on the oracle's cell records of the grid cases of tests/test_gpu_clip_zero_terms.py (every vertex of every polygon a candidate
pair's Sutherland-Hodgman loop tests, against every cutting edge) and on 10^6 random operands.

The crossings must NOT be reduced the same way: there the sign of a zero numerator reaches the result.  The last test pins that."""
import numpy as np

import orc
from test_gpu_clip_edges import PI, TPI, _pimod, latlon_window

THRESH = 1.e-12


def full(x0, y0, x1, y1, x, y):
    return (x - x0) * (y1 - y0) + (x0 - x1) * (y - y0) <= THRESH


def horizontal(x0, y0, x1, y1, x, y):
    return (x0 - x1) * (y - y0) <= THRESH


def vertical(x0, y0, x1, y1, x, y):
    return (x - x0) * (y1 - y0) <= THRESH


# ------------------------------------------------------------------------------------------------ the grid cases
def _win(*w):
    lo, la = latlon_window(*w)
    return (w[4], w[5], lo, la)


def targets(fg):
    """(a) 36x18 global from 0: every column vertical.  (b) the same from -2.5 and (c) a 10x10 window from -0.5: the longitude axis
    changes sign inside one column, and fix_lon's raw0 + (raw1 - raw0) leaves its two sides a bit apart.  (d) a 12x6 window over the
    prime meridian from the equator to the pole: both signs of the +-2 pi shift and the `wrap` branch (the seam of the cells'
    longitudes after fix_lon is the prime meridian; the CPU walk finds no shift in a window across 180 degrees)."""
    def ll(a, b):
        lo, la = fg.latlon_corners(36, 18, a, b)
        return (36, 18, lo, la)
    return {"a": ll(0.0, 360.0), "b": ll(-2.5, 357.5), "c": _win(-0.5, 9.5, -5.0, 5.0, 10, 10), "d": _win(-30.0, 30.0, 0.0, 90.0, 12, 6)}


def sources(fg):
    lon, lat = fg.gnomonic_ed_corners(8)
    return [(8, 8, lon[t], lat[t]) for t in range(6)]


_memo = {}


def walk(fg, name):
    """The candidate pairs of C8 (six tiles) and target `name`, as create_xgrid_2dx2d finds them (create_xgrid.c:1058-1078), each
    clipped by a plain Sutherland-Hodgman loop (:1270-1340) over the oracle's records.  Per pair: whether the cutting quad is
    `flagged` (x2[3] != x2[0] or x2[1] != x2[2] in the cell's record, where the kernel's guard looks: the shift and pimod keep
    equal values equal, and can round unequal ones together), the shift, wrap, and every inside test on the values the edge loop
    sees as a row (x0, y0, x1, y1, x, y, e, flagged) of `tests`.  Made once per case."""
    if name in _memo:
        return _memo[name]
    nx2, ny2, lo, la = targets(fg)[name]
    D = orc.orc_cell_struct(nx2, ny2, lo, la)
    assert np.all(D["nvert"] == 4)
    pairs, rows = [], []
    for (nx, ny, lon, lat) in sources(fg):
        S = orc.orc_cell_struct(nx, ny, lon, lat)
        for s in range(nx * ny):
            n1 = int(S["nvert"][s])
            cand = np.flatnonzero((D["lat_min"] < S["lat_max"][s]) & (D["lat_max"] > S["lat_min"][s]))
            for d in cand:
                x2, y2 = D["vlon"][d, :4].copy(), D["vlat"][d, :4].copy()
                flagged = bool(x2[3] != x2[0] or x2[1] != x2[2])
                dx = D["lon_avg"][d] - S["lon_avg"][s]
                shift = TPI if dx < -PI else (-TPI if dx > PI else 0.0)
                lo_min, lo_max = D["lon_min"][d], D["lon_max"][d]
                if shift != 0.0:
                    lo_min += shift; lo_max += shift; x2 += shift
                if lo_min >= S["lon_max"][s] or lo_max <= S["lon_min"][s]:
                    continue
                x1, y1 = S["vlon"][s, :n1].copy(), S["vlat"][s, :n1].copy()
                wrap = bool(np.any((x1 > TPI) | (x1 < 0.0)))
                if wrap:
                    x1 = np.array([_pimod(v) for v in x1]); x2 = np.array([_pimod(v) for v in x2])
                poly = list(zip(x1, y1))
                maxn = maxcross = 0
                e0 = (x2[3], y2[3])
                for e in range(4):
                    e1 = (x2[e], y2[e])
                    new = []
                    px, py = poly[-1]
                    pin = full(e0[0], e0[1], e1[0], e1[1], px, py)
                    for (qx, qy) in poly:
                        rows.append((e0[0], e0[1], e1[0], e1[1], qx, qy, e, flagged))
                        qin = full(e0[0], e0[1], e1[0], e1[1], qx, qy)
                        if qin != pin:
                            dy1, dy2, dx1, dx2 = qy - py, e1[1] - e0[1], qx - px, e1[0] - e0[0]
                            ds1, ds2 = py * qx - qy * px, e0[1] * e1[0] - e1[1] * e0[0]
                            det = dy2 * dx1 - dy1 * dx2
                            new.append(((dx2 * ds1 - dx1 * ds2) / det, (dy2 * ds1 - dy1 * ds2) / det))
                        if qin:
                            new.append((qx, qy))
                        px, py, pin = qx, qy, qin
                    maxcross = max(maxcross, sum(1 for v in new if v not in poly))
                    poly = new
                    maxn = max(maxn, len(poly))
                    e0 = e1
                    if not poly:
                        break
                pairs.append(dict(d=int(d), col=int(d) % nx2, n1=n1, shift=shift, wrap=wrap, flagged=flagged, nout=len(poly), maxn=maxn,
                                  maxcross=maxcross))
    _memo[name] = dict(pairs=pairs, tests=np.array(rows, dtype=np.float64), D=D, nx2=nx2)
    return _memo[name]


def record_flagged_columns(w):
    v = w["D"]["vlon"]
    return sorted(set(np.flatnonzero((v[:, 3] != v[:, 0]) | (v[:, 1] != v[:, 2])) % w["nx2"]))


# ------------------------------------------------------------------------------------------------ the tests
def test_the_cases_hold_what_they_are_there_for(fg):
    a, b, c, d = (walk(fg, k) for k in "abcd")
    for w in (a, b, c, d):          # nothing the quad kernel defers for a reason of its own: polygons over 8 vertices, over 2 crossings
        assert max(p["maxn"] for p in w["pairs"]) <= 8 and max(p["maxcross"] for p in w["pairs"]) <= 2
    assert record_flagged_columns(a) == [] and not any(p["flagged"] for p in a["pairs"])
    for w in (b, c):
        cols = record_flagged_columns(w)
        assert 0 < len(cols) < w["nx2"], cols                       # a column fix_lon left not exactly vertical, and one it did
        assert any(p["flagged"] for p in w["pairs"]) and not all(p["flagged"] for p in w["pairs"])
    assert not any(p["flagged"] for p in d["pairs"])
    live = [p for p in d["pairs"] if p["nout"] > 0]
    assert {np.sign(p["shift"]) for p in live} == {-1.0, 0.0, 1.0}
    assert {np.sign(p["shift"]) for p in live if p["wrap"]} >= {-1.0, 1.0}


def test_reduced_predicates_on_the_cell_records(fg):
    ntests = 0
    for name in "abcd":
        t = walk(fg, name)["tests"]
        x0, y0, x1, y1, x, y, e, flagged = t.T
        ref = full(x0, y0, x1, y1, x, y)
        hor = (e == 1) | (e == 3)
        assert np.array_equal(y0[hor], y1[hor])                       # horizontal by construction
        assert np.array_equal(horizontal(x0, y0, x1, y1, x, y)[hor], ref[hor]), name
        ver = ~hor & (flagged == 0)                                    # the guard: such a pair is left to the general kernel
        assert np.array_equal(x0[ver], x1[ver])
        assert np.array_equal(vertical(x0, y0, x1, y1, x, y)[ver], ref[ver]), name
        assert np.count_nonzero(hor) > 0 and np.count_nonzero(ver) > 0
        assert 0 < np.count_nonzero(ref) < ref.size
        ntests += ref.size
    assert ntests > 20000


def _operands(rng, n):
    """n values: magnitudes from 1e-300 to 1e300 and O(1) coordinates, both signs, with +-0 and repeated values mixed in"""
    v = np.where(rng.random(n) < 0.5, rng.uniform(-7.0, 7.0, n), 10.0 ** rng.uniform(-300.0, 300.0, n) * rng.choice([-1.0, 1.0], n))
    z = rng.random(n)
    v = np.where(z < 0.05, 0.0, np.where(z < 0.10, -0.0, v))
    return v


def test_reduced_predicates_on_random_operands():
    rng = np.random.default_rng(20)
    n = 1000000
    x0, y0, x1, y1, x, y = (_operands(rng, n) for _ in range(6))
    # equal coordinates: the vertex on the edge's line or on its first end
    k = rng.random(n)
    x = np.where(k < 0.1, x0, x); y = np.where((k > 0.05) & (k < 0.15), y0, y)
    # products at the threshold and one ulp to either side of it: factor * t with t around 1e-12 / factor
    f = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    t = THRESH / f
    t = np.where(rng.random(n) < 0.5, np.nextafter(t, np.inf), np.where(rng.random(n) < 0.5, np.nextafter(t, -np.inf), t))
    near = rng.random(n) < 0.2
    with np.errstate(over="ignore", invalid="ignore"):
        # horizontal edge: y1 is y0; the kept product is (x0 - x1) * (y - y0)
        hx1 = np.where(near, x0 - f, x1); hy = np.where(near, y0 + t, y)
        ref = full(x0, y0, hx1, y0, x, hy)
        got = horizontal(x0, y0, hx1, y0, x, hy)
        assert np.array_equal(ref, got), np.flatnonzero(ref != got)[:5]
        assert 0 < np.count_nonzero(ref[near]) < np.count_nonzero(near)
        # vertical edge: x1 is x0; the kept product is (x - x0) * (y1 - y0)
        vy1 = np.where(near, y0 + f, y1); vx = np.where(near, x0 + t, x)
        ref = full(x0, y0, x0, vy1, vx, y)
        got = vertical(x0, y0, x0, vy1, vx, y)
        assert np.array_equal(ref, got), np.flatnonzero(ref != got)[:5]
        assert 0 < np.count_nonzero(ref[near]) < np.count_nonzero(near)
    assert not np.any(np.isnan((x - x0) * (y0 - y0)))                  # no inf * 0: coordinates stay below 1e300


def test_the_crossing_must_keep_both_products():
    """A crossing with a vertical cutting edge on the line x = 0 (dx2 = 0, ds2 = +0): the reference's x numerator is
    dx2 * ds1 - dx1 * ds2, the 'simplified' one -(dx1 * ds2).  Both are zero, with different signs for some signs of dx1 and ds1,
    and the quotient keeps the sign."""
    differ = []
    dx2, determ = np.float64(0.0), np.float64(0.125)
    for ds2 in (np.float64(0.0), np.float64(-0.0)):                  # (-0: the edge's two latitudes have different signs)
        for dx1 in (np.float64(-0.25), np.float64(0.25)):
            for ds1 in (np.float64(-0.5), np.float64(0.5)):
                ref = (dx2 * ds1 - dx1 * ds2) / determ
                simple = -(dx1 * ds2) / determ
                assert ref == simple == 0.0                          # equal as numbers ...
                if ref.view(np.uint64) != simple.view(np.uint64):    # ... not in bits
                    differ.append((float(ds2), float(dx1), float(ds1)))
    assert differ, "the simplified crossing equals the reference's in bits on every crafted operand set"
    assert any(dx1 < 0 for (_, dx1, _) in differ)
