"""Inputs and the brute-force reference of the great-circle polygon-list search (fg_plan_create_polylist_gc).

The reference side is make_coupler_mosaic.c's GREAT_CIRCLE_CLIP branch restated over a primitive set passed in (Prims): the
remembered atmosphere x land polygons of :1396-1551 (every atmosphere cell against every land cell, clip_2dx2d_great_circle,
great_circle_area, the :1507 test against min(area_lnd, area_atm)) and the clip of a list of polygons against every cell of a
grid in polygon-major, cell-ascending order (:1664-1678 without the land fraction; the plan's acceptance test is
area / min(area_ref, area_cell) > 1e-6).  A pair is skipped only by the clip's own first test (create_xgrid.c:1508-1528, the
0.05 range test on x, y, z), evaluated here in numpy with the same comparisons; `skipped` keeps those pairs for the CPU test.
Line numbers are the reference's.  The rest of the branch (ocean fractions, sums, masks) is not restated here."""
import ctypes as C
import math

import numpy as np

import gc_cases
import orc

RANGE_CHECK = 0.05              # mosaic_util.h:26
THRESH = 1.0e-6                 # create_xgrid.c:26


class Prims:
    """clip(a [n, 3], b [m, 3]) -> (n_out, v [n_out, 3]); area(v [n, 3]); grid_area(nx, ny, lon, lat) -> [ny * nx]"""

    def __init__(self, clip, area, grid_area, name):
        self.clip, self.area, self.grid_area, self.name = clip, area, grid_area, name


def prims_oracle(cr):
    """gc_oracle.c: the plain build (pinned to the compiled reference) or the _cr build (the device's arc cosine)"""
    return Prims(lambda a, b: orc.orc_clip_gc(a, b, cr=cr), lambda v: orc.orc_great_circle_area(v[:, 0], v[:, 1], v[:, 2], cr=cr),
                 lambda nx, ny, lon, lat: orc.orc_get_grid_gc_area(nx, ny, lon, lat, cr=cr), "oracle_cr" if cr else "oracle")


def prims_ref():
    """the compiled reference's own clip_2dx2d_great_circle / great_circle_area / get_grid_great_circle_area.  Its clip ends the
    process on a polygon it calls not convex: callers run the plain oracle first, which returns a negative code there."""
    R = orc.ref()

    def clip(a, b):
        a, b = orc.f64(a), orc.f64(b)
        aa = [np.ascontiguousarray(a[:, k]) for k in range(3)]
        bb = [np.ascontiguousarray(b[:, k]) for k in range(3)]
        oo = [np.zeros(50) for _ in range(3)]
        n = R.clip_2dx2d_great_circle(*[orc._dp(v) for v in aa], len(a), *[orc._dp(v) for v in bb], len(b), *[orc._dp(v) for v in oo])
        return n, np.stack([v[:max(n, 0)] for v in oo], axis=1)

    def area(v):
        x, y, z = (np.ascontiguousarray(v[:, k]) for k in range(3))
        return R.great_circle_area(len(x), orc._dp(x), orc._dp(y), orc._dp(z))

    return Prims(clip, area, orc.ref_get_grid_gc_area, "reference")


def corners_xyz(lon, lat):
    """latlon2xyz (mosaic_util.c:212-222) of a corner array -> [ny+1, nx+1, 3]"""
    lo, la = orc.f64(lon), orc.f64(lat)
    x, y, z = (np.empty(lo.size) for _ in range(3))
    orc.oracle().orc_latlon2xyz(lo.size, orc._dp(lo.ravel()), orc._dp(la.ravel()), orc._dp(x), orc._dp(y), orc._dp(z))
    return np.stack([x, y, z], axis=1).reshape(lo.shape + (3,))


def cells_xyz(c):
    """[ny * nx, 4, 3]: the cells of a corner array clockwise, (j, i) (j+1, i) (j+1, i+1) (j, i+1) (:1367-1375)"""
    ny, nx = c.shape[0] - 1, c.shape[1] - 1
    return np.stack([c[:-1, :-1], c[1:, :-1], c[1:, 1:], c[:-1, 1:]], axis=2).reshape(ny * nx, 4, 3)


def range_pass(p, cells):
    """create_xgrid.c:1508-1528 for the polygon p [n, 3] against cells [m, 4, 3]: True where the clip goes on"""
    mn1, mx1 = p.min(axis=0), p.max(axis=0)
    mn2, mx2 = cells.min(axis=1), cells.max(axis=1)
    out = (mn1[None, :] >= mx2 + RANGE_CHECK) | (mn2 >= mx1[None, :] + RANGE_CHECK)
    return ~out.any(axis=1)


class Grid:
    def __init__(self, nx, ny, lon, lat):
        self.nx, self.ny = nx, ny
        self.lon, self.lat = orc.f64(lon).reshape(ny + 1, nx + 1), orc.f64(lat).reshape(ny + 1, nx + 1)
        self.cells = cells_xyz(corners_xyz(self.lon, self.lat))


def remembered_polygons(atm, lnd, P):
    """:1396-1551 with land of its own: (n [np], xyz [np, 8, 3], area_ref [np], atm cell [np] flattened over the tiles, land cell
    [np], cover = polygons by vertex count).  atm: list of Grid, lnd: one Grid."""
    area_lnd = P.grid_area(lnd.nx, lnd.ny, lnd.lon, lnd.lat)
    n, xyz, ref, ia, il = [], [], [], [], []
    cover = {}
    off = 0
    for ga in atm:
        area_atm = P.grid_area(ga.nx, ga.ny, ga.lon, ga.lat)
        for la in range(ga.nx * ga.ny):
            a = ga.cells[la]
            for ll in np.nonzero(range_pass(a, lnd.cells))[0]:
                n_out, v = P.clip(a, lnd.cells[ll])                                 # :1439
                if n_out < 0:
                    raise RuntimeError(f"{P.name}: clip error {n_out} (atm cell {off + la}, land cell {ll})")
                if n_out > 0:
                    min_area = min(area_lnd[ll], area_atm[la])                      # :1488
                    if P.area(v) / min_area > THRESH:                               # :1507
                        if n_out > 8:
                            raise RuntimeError("a remembered polygon has more than 8 vertices")
                        p = np.zeros((8, 3))
                        p[:n_out] = v
                        n.append(n_out); xyz.append(p); ref.append(min_area); ia.append(off + la); il.append(int(ll))
                        cover[n_out] = cover.get(n_out, 0) + 1
        off += ga.nx * ga.ny
    return dict(n=np.array(n, dtype=np.int32), xyz=np.array(xyz).reshape(-1, 8, 3), area_ref=np.array(ref), ia=np.array(ia), il=np.array(il),
                cover=cover)


def polylist_reference(n, xyz, area_ref, dst, P, want_skipped=False):
    """every polygon against every cell of dst, polygon-major, cells ascending: dict poly, cell, nv, verts [k, 16, 3], area; cover =
    outputs by vertex count; errors = {polygon: code} of the polygons whose clip returned a negative code (they get no entry)"""
    area_dst = P.grid_area(dst.nx, dst.ny, dst.lon, dst.lat)
    poly, cell, nv, verts, area, skipped = [], [], [], [], [], []
    cover, errors = {}, {}
    for k in range(len(n)):
        if n[k] < 3:
            continue
        p = xyz[k, :n[k]]
        go = range_pass(p, dst.cells)
        if want_skipped:
            skipped += [(k, int(d)) for d in np.nonzero(~go)[0]]
        rows = []
        for d in np.nonzero(go)[0]:
            n_out, v = P.clip(p, dst.cells[d])
            if n_out < 0:
                errors[k] = n_out
                break
            if n_out > 0:
                a = P.area(v)
                if a / min(area_ref[k], area_dst[d]) > THRESH:
                    rows.append((int(d), n_out, v, a))
        if k in errors:
            continue
        for d, n_out, v, a in rows:
            w = np.zeros((16, 3))
            w[:n_out] = v
            poly.append(k); cell.append(d); nv.append(n_out); verts.append(w); area.append(a)
            cover[n_out] = cover.get(n_out, 0) + 1
    return dict(poly=np.array(poly, dtype=np.int64), cell=np.array(cell, dtype=np.int64), nv=np.array(nv, dtype=np.int32),
                verts=np.array(verts).reshape(-1, 16, 3), area=np.array(area), cover=cover, errors=errors, skipped=skipped, area_dst=area_dst)


# ------------------------------------------------------------------------------------------------------------------- the cases
def own_c4(fg):
    """C4 atmosphere, one 15 x 7 lat-lon land tile over -88 .. 88 degrees starting at 13 E, a 24 x 14 lat-lon ocean from -78 to 90
    degrees with the southern extension row of coupler_ocean_grid"""
    lon, lat = fg.gnomonic_ed_corners(4)
    atm = [Grid(4, 4, lon[t], lat[t]) for t in range(6)]
    ll, la = fg.latlon_corners(15, 7, 13.0, 373.0, -88.0, 88.0)
    oo, oa = fg.latlon_corners(24, 14, 0.0, 360.0, -78.0, 90.0)
    g = fg.coupler_ocean_grid(np.degrees(oo), np.degrees(oa), None)
    assert g["ocn_south_ext"] == 1 and g["ny"] == 15
    return dict(atm=atm, lnd=Grid(15, 7, ll, la), ocn=Grid(24, 15, g["x"], g["y"]))


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _ll(lon_deg, lat_deg):
    lo, la = math.radians(lon_deg), math.radians(lat_deg)
    return np.array([math.cos(la) * math.cos(lo), math.cos(la) * math.sin(lo), math.sin(la)])


def _ring(lon_deg, lat_deg, r, m, phase=0.0):
    """m points at angular distance ~r around a centre, clockwise seen from outside (east to the right, north up)"""
    c = _ll(lon_deg, lat_deg)
    e = _unit(np.cross([0.0, 0.0, 1.0], c))
    nrt = np.cross(c, e)
    th = phase - 2.0 * math.pi * np.arange(m) / m
    return _unit(c[None, :] + math.tan(r) * (np.cos(th)[:, None] * e[None, :] + np.sin(th)[:, None] * nrt[None, :]))


CRAFTED_KINDS = ("triangle", "octagon", "equals_cell", "snap_corner_and_edge", "holds_north_pole", "antipodal", "first_two_coincide")


def crafted(fg):
    """(dst Grid 12 x 8 over longitudes 0 .. 180 from pole to pole, kinds, n [7], xyz [7, 8, 3]); the antipodal polygon sits at
    270 E on the equator, opposite the grid's middle, and must meet no cell"""
    lo, la = fg.latlon_corners(12, 8, 0.0, 180.0, -90.0, 90.0)
    dst = Grid(12, 8, lo, la)
    c = corners_xyz(dst.lon, dst.lat)                       # [9, 13, 3]
    polys = {
        "triangle": _ring(40.0, 20.0, 0.12, 3, 0.3),
        "octagon": _ring(100.0, -35.0, 0.2, 8, 0.1),
        "equals_cell": dst.cells[3 * 12 + 5].copy(),
        # first vertex: the corner (i 8, j 5) of the grid, bit for bit; third: the middle of the meridian edge (i 9, j 4 .. 5)
        "snap_corner_and_edge": np.stack([c[5, 8], _ll(131.0, 30.0), _unit(c[4, 9] + c[5, 9]), _ll(125.0, 5.0)]),
        "holds_north_pole": _ring(60.0, 88.0, 0.15, 6, 0.2),
        "antipodal": _ring(270.0, 0.0, 0.1, 4, 0.4),
    }
    q = _ring(60.0, -50.0, 0.15, 4, 0.5)
    polys["first_two_coincide"] = np.concatenate([q[:1], q])
    n = np.array([len(polys[k]) for k in CRAFTED_KINDS], dtype=np.int32)
    xyz = np.zeros((len(CRAFTED_KINDS), 8, 3))
    for k, name in enumerate(CRAFTED_KINDS):
        xyz[k, :n[k]] = polys[name]
    return dst, CRAFTED_KINDS, n, xyz


def own_area(p, P):
    """great_circle_area of the de-duplicated polygon (gridArea, mosaic_util.c:1399-1419)"""
    return P.area(gc_cases.dedup(p))


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]
