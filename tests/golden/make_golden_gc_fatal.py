#!/usr/bin/env python3
"""Inputs on which clip_2dx2d_great_circle (create_xgrid.c:1479-1908) ends the process, for the polygon-list entry: a polygon of
3..8 unit vectors and a destination grid of 4 x 4 cells such that one (polygon, cell) pair makes the CPU oracle's clip return a
negative code (oracle/gc_oracle.c: -1/-2 not convex, -3 .. -8 the six fatals inside the clip, -9 its list capacity, -11 the pairs on
which the reference's insertIntersect does not end).

A seeded search: TRIALS polygons built from the destination grid's own corners (bit-exact corner copies, unit(c_a + c_b) edge
midpoints, shifts of 1e-16 .. 1e-9) and from the generators of tests/polylist_gc_cases.py (_ring, _ll, _unit), each against every
cell its range test lets through, under the plain oracle (pinned to the compiled reference) and the _cr one (the device's arc
cosine).  An input is kept only if
  * both builds return the same code on every pair, and
  * every pair of the polygon that is fatal at all has that one code (the device reports the largest clip code of a search, the
    reference the first in its loop order: with one code per input the two cannot differ),
at most three per code, from different recipes where the search offers them.  Code 2 needs a destination cell that is not
convex: those inputs use the second grid, whose interior corner (1, 1) is moved north past its neighbours.

A second search (search_grids) looks for the clip's own codes between two quadrilateral grids: the 2 x 2 source grid of
tests/gc_fatal_cases.py against random lat-lon grids of 2..4 x 2..4 cells with one corner snapped onto the middle of a source edge.

Run:  python tests/golden/make_golden_gc_fatal.py      (about four minutes; prints what it reached and what it did not)
Output: gc_fatal_polygons.npz -- grids lon / lat [2, 5, 5] (radians), per input n, xyz [8, 3], code, grid, recipe; per found grid
pair g_code, g_nx, g_ny, g_lon / g_lat [5, 5] (the leading [ny + 1, nx + 1] part), g_extent (w, e, s, n of the grid before the
snap, degrees), g_snap (j, i of the snapped corner).  The file
holds this project's own input data; tests/gc_fatal_cases.py re-derives every code from the oracle when it is imported, so no
test depends on this search running again bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc  # noqa: E402
import polylist_gc_cases as pc  # noqa: E402

SEED, TRIALS, PER_CODE = 20261021, 150000, 3
D2R = np.pi / 180.0
RECIPES = ("cell_copy_shifted", "ring_midpoint_and_corner", "corners_and_midpoints", "ring_one_vertex_pulled", "cell_midpoint_vertex",
           "ring_through_two_corners")


def latlon(nx, ny, w, e, s, n):
    lon, lat = np.meshgrid((w + np.arange(nx + 1) * ((e - w) / nx)) * D2R, (s + np.arange(ny + 1) * ((n - s) / ny)) * D2R)
    return np.ascontiguousarray(lon), np.ascontiguousarray(lat)


def grids():
    """[0] 4 x 4 over 20 .. 120 E, -60 .. 40 N; [1] the same with the corner (j 1, i 1) moved to 14 N, beyond (j 2, i 1) at -10 N:
    the cells (0, 0), (0, 1) grow a spike and the cells (1, 0), (1, 1) turn inside out there"""
    lo, la = latlon(4, 4, 20.0, 120.0, -60.0, 40.0)
    la2 = la.copy()
    la2[1, 1] = 14.0 * D2R
    return np.stack([lo, lo]), np.stack([la, la2])


def pair_codes(p, g, cr):
    """{cell: negative code} over every cell of the pc.Grid g that the range test lets through"""
    out = {}
    for d in np.nonzero(pc.range_pass(p, g.cells))[0]:
        c = orc.orc_clip_gc(p, g.cells[d], cr=cr)[0]
        if c < 0:
            out[int(d)] = int(c)
    return out


def candidate(rng, it, g, c):
    """one trial polygon of recipe it % 6 against the grid g (corners c [5, 5, 3])"""
    mode = it % len(RECIPES)
    cell = g.cells[int(rng.integers(0, 16))]
    lon0, lat0 = rng.uniform(25.0, 115.0), rng.uniform(-55.0, 35.0)
    if mode == 0:       # a cell's corners, one to four of them shifted by 1e-16 .. 1e-9, in either order
        p = cell.copy()
        for q in rng.choice(4, int(rng.integers(1, 5)), replace=False):
            p[q] = pc._unit(p[q] + rng.normal(size=3) * 10.0 ** rng.uniform(-16, -9))
        if rng.random() < 0.5:
            p = p[::-1]
    elif mode == 1:     # a ring with one vertex on the middle of a cell edge and another on a corner, bit for bit
        p = pc._ring(lon0, lat0, rng.uniform(0.05, 0.4), int(rng.integers(3, 9)), rng.uniform(0, 6))
        a = int(rng.integers(0, 4))
        p[0] = pc._unit(cell[a] + cell[(a + 1) % 4])
        p[int(rng.integers(1, len(p)))] = cell[int(rng.integers(0, 4))]
    elif mode == 2:     # the corners of a cell with edge midpoints between them, some shifted
        j, i = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        pts = [c[j, i], c[j + 1, i], c[j + 1, i + 1], c[j, i + 1]]
        m, out = int(rng.integers(3, 9)), []
        for q in range(4):
            out.append(pts[q])
            if len(out) < m and rng.random() < 0.6:
                out.append(pc._unit(pts[q] + pts[(q + 1) % 4]))
        p = np.array(out[:8])
        for q in range(len(p)):
            if rng.random() < 0.4:
                p[q] = pc._unit(p[q] + rng.normal(size=3) * 10.0 ** rng.uniform(-16, -9))
        if rng.random() < 0.3:
            p = p[::-1]
    elif mode == 3:     # a ring with one vertex pulled towards (or through) its centre: a chevron when pulled far enough
        m = int(rng.integers(4, 9))
        p = pc._ring(lon0, lat0, rng.uniform(0.05, 0.4), m, rng.uniform(0, 6))
        q = int(rng.integers(0, m))
        cen = pc._unit(p.sum(0))
        p[q] = pc._unit(cen + rng.uniform(-0.5, 0.3) * (p[q] - cen))
    elif mode == 4:     # a cell with one corner replaced by the middle of the edge that starts there, another shifted by 1e-12 .. 1e-7
        p = cell.copy()
        a, b = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        p[a] = pc._unit(cell[a] + cell[(a + 1) % 4])
        if b != a:
            p[b] = pc._unit(p[b] + rng.normal(size=3) * 10.0 ** rng.uniform(-12, -7))
        if rng.random() < 0.5:
            p = p[::-1]
    else:               # a ring whose first two vertices are two corners of a cell
        p = pc._ring(lon0, lat0, rng.uniform(0.05, 0.4), int(rng.integers(3, 9)), rng.uniform(0, 6))
        p[0], p[1] = cell[0], cell[int(rng.integers(1, 4))]
        if rng.random() < 0.5:
            p = p[::-1]
    return mode, np.ascontiguousarray(p)


def search():
    lon, lat = grids()
    G = [pc.Grid(4, 4, lon[k], lat[k]) for k in range(2)]
    C = [pc.corners_xyz(g.lon, g.lat) for g in G]
    rng = np.random.default_rng(SEED)
    hits, mixed, disagree = {}, 0, 0            # code -> [(recipe, grid, polygon)]
    count = {}
    for it in range(TRIALS):
        gi = 1 if it % 7 == 6 else 0            # every seventh trial against the grid with the cell that is not convex
        mode, p = candidate(rng, it, G[gi], C[gi])
        a = pair_codes(p, G[gi], False)
        if not a:
            continue
        b = pair_codes(p, G[gi], True)
        if a != b:
            disagree += 1
            continue
        for v in set(a.values()):
            count[-v] = count.get(-v, 0) + 1
        if len(set(a.values())) != 1:
            mixed += 1
            continue
        code = -next(iter(a.values()))
        if gi == 1 and code != 2:               # the second grid is there for code 2 alone
            continue
        have = hits.setdefault(code, [])
        if len(have) < PER_CODE and (mode not in [h[0] for h in have] or it > TRIALS // 2):
            have.append((mode, gi, p))
    print(f"{TRIALS} trials, seed {SEED}: polygons with a fatal pair, by code {dict(sorted(count.items()))}; "
          f"{mixed} with two codes, {disagree} on which the two builds differ (neither kept)")
    print("not reached:", [k for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11) if k not in count])
    return lon, lat, hits


# ------------------------------------------------------------------------------------------------- two quadrilateral grids
GRID_SEED, GRID_TRIALS = 20261022, 150000
SRC = (2, 2, 3.0, 27.0, -12.0, 12.0)          # the source grid of every quad x quad case (tests/gc_fatal_cases.py)


def grid_code(src, dst, cr):
    """orc_create_xgrid_great_circle_rows on (nx, ny, lon, lat) pairs: the count, or -(100 + code)"""
    try:
        return orc.orc_create_xgrid_gc(src[0], src[1], dst[0], dst[1], src[2], src[3], dst[2], dst[3], cr=cr)["n"]
    except RuntimeError as e:
        return int(str(e).rsplit(":", 1)[1])


def grid_pair_codes(S, T, cr):
    """{(source cell, destination cell): negative code} over every pair of two pc.Grid that the range test lets through"""
    out = {}
    for s in range(len(S.cells)):
        for d, c in pair_codes(S.cells[s], T, cr).items():
            out[(s, d)] = c
    return out


def search_grids():
    """Clip codes from two lat-lon grids: a random destination grid of 2..4 x 2..4 cells around the source grid; its interior corner
    nearest the middle of a source edge (no further than 4 degrees) is snapped onto that midpoint, and (recipes 0, 1) the neighbouring
    destination corner nearest an end of that edge onto the end (if within 4 degrees too), lon and lat copied; recipe 1 then moves the snapped corner by
    1e-16 .. 1e-9 rad.  Kept: the first grid pair per code whose fatal pairs all have that one clip code, under both builds."""
    lo1, la1 = latlon(*SRC)
    S = pc.Grid(2, 2, lo1, la1)
    c1 = pc.corners_xyz(S.lon, S.lat)
    edges = [((j, i), (j, i + 1)) for j in range(3) for i in range(2)] + [((j, i), (j + 1, i)) for j in range(2) for i in range(3)]
    mids = []
    for a, b in edges:
        m = pc._unit(c1[a] + c1[b])
        mids.append((np.arctan2(m[1], m[0]), np.arcsin(m[2])))
    rng = np.random.default_rng(GRID_SEED)
    hits, count, tried = {}, {}, 0
    for it in range(GRID_TRIALS):
        nx2, ny2 = int(rng.integers(2, 5)), int(rng.integers(2, 5))
        w, s = rng.uniform(-3.0, 9.0), rng.uniform(-18.0, -6.0)
        extent = (w, w + rng.uniform(14.0, 30.0), s, s + rng.uniform(14.0, 30.0))
        lo, la = latlon(nx2, ny2, *extent)
        shift = rng.normal(size=2) * 10.0 ** rng.uniform(-16, -9, size=2)
        which = int(rng.integers(0, 2))
        best = None
        for k, (mlon, mlat) in enumerate(mids):
            d2 = (lo[1:-1, 1:-1] - mlon) ** 2 + (la[1:-1, 1:-1] - mlat) ** 2
            q = np.unravel_index(np.argmin(d2), d2.shape)
            if best is None or d2[q] < best[0]:
                best = (d2[q], k, q[0] + 1, q[1] + 1)
        if best[0] > (4.0 * D2R) ** 2:
            continue
        tried += 1
        recipe, (_, k, j, i) = it % 3, best
        lo[j, i], la[j, i] = mids[k]
        if recipe != 2:
            end = edges[k][which]
            nb = min(((lo[j + dj, i + di] - lo1[end]) ** 2 + (la[j + dj, i + di] - la1[end]) ** 2, j + dj, i + di)
                     for dj, di in ((0, 1), (0, -1), (1, 0), (-1, 0)))
            if nb[0] <= (4.0 * D2R) ** 2:
                lo[nb[1], nb[2]], la[nb[1], nb[2]] = lo1[end], la1[end]
        if recipe == 1:
            lo[j, i] += shift[0]; la[j, i] += shift[1]
        r = grid_code((2, 2, lo1, la1), (nx2, ny2, lo, la), False)
        if r >= 0 or r != grid_code((2, 2, lo1, la1), (nx2, ny2, lo, la), True):
            continue
        T = pc.Grid(nx2, ny2, lo, la)
        a, b = grid_pair_codes(S, T, False), grid_pair_codes(S, T, True)
        codes = set(b.values())
        for v in codes:
            count[-v] = count.get(-v, 0) + 1
        if a != b or len(codes) != 1 or -next(iter(codes)) < 3:
            continue
        hits.setdefault(-next(iter(codes)), (nx2, ny2, lo, la, recipe, extent, (j, i)))
    print(f"grid pairs: {GRID_TRIALS} trials ({tried} with a corner to snap), seed {GRID_SEED}: grid pairs with a fatal pair, by code "
          f"{dict(sorted(count.items()))}; kept {sorted(hits)}")
    return hits


def main():
    ghits = search_grids()
    lon, lat, hits = search()
    n, xyz, code, grid, recipe = [], [], [], [], []
    for k in sorted(hits):
        for mode, gi, p in hits[k]:
            v = np.zeros((8, 3))
            v[:len(p)] = p
            n.append(len(p)); xyz.append(v); code.append(k); grid.append(gi); recipe.append(RECIPES[mode])
            print("code", k, "grid", gi, RECIPES[mode], len(p), "vertices")
    gk = sorted(ghits)
    g_lon, g_lat = np.zeros((len(gk), 5, 5)), np.zeros((len(gk), 5, 5))      # [ny + 1, nx + 1] in the leading corner
    for q, k in enumerate(gk):
        nx2, ny2, lo, la, rec = ghits[k][:5]
        g_lon[q, :ny2 + 1, :nx2 + 1], g_lat[q, :ny2 + 1, :nx2 + 1] = lo, la
        print("grid pair: code", k, f"destination {nx2} x {ny2}, recipe", rec)
    np.savez_compressed(os.path.join(HERE, "gc_fatal_polygons.npz"), lon=lon, lat=lat, n=np.array(n, dtype=np.int32), xyz=np.array(xyz),
                        code=np.array(code, dtype=np.int32), grid=np.array(grid, dtype=np.int32), recipe=np.array(recipe),
                        g_code=np.array(gk, dtype=np.int32), g_nx=np.array([ghits[k][0] for k in gk], dtype=np.int32),
                        g_ny=np.array([ghits[k][1] for k in gk], dtype=np.int32), g_lon=g_lon, g_lat=g_lat,
                        g_extent=np.array([ghits[k][5] for k in gk]).reshape(len(gk), 4), g_snap=np.array([ghits[k][6] for k in gk], dtype=np.int32).reshape(len(gk), 2))


if __name__ == "__main__":
    main()
