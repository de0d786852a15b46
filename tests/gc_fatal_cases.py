"""Inputs on which the reference's great-circle clip ends the process, and what the device must say about them.

clip_2dx2d_great_circle (create_xgrid.c:1479-1908) calls error_handler -- a line on stderr, exit(1) -- in eight places.  The CPU
oracle (oracle/gc_oracle.c, plain and _cr builds) returns them as negative codes, orc_create_xgrid_great_circle_rows as
-(100 + code); the device raises error words that plan_search_core turns into FG_ERR_GEOM with the reference's text (MESSAGES).
One more code, 11, is the oracle's and the device's own: the pairs on which the reference's insertIntersect never returns.

PAIR_CASES   for the polygon-list entries: a polygon of 3..8 unit vectors and a 4 x 4 destination grid, from the seeded search of
             tests/golden/make_golden_gc_fatal.py, stored in tests/golden/gc_fatal_polygons.npz.  Every fatal pair of a case has the
             case's one code under both builds of the oracle -- checked again here, at import.
ordinary()   the four polygons of polylist_gc_cases.crafted that need no particular grid, which surround the bad one in a list.
GRID_CASES   for the quad x quad entries: lat-lon grids of at most 4 x 4 cells with one displaced corner (codes 1 and 2; also with
             the bad cell beside the other grid, where no pair overlaps and the reference still ends), the
             grid pairs the same search found for the clip's own codes, the silent cases (a grid with descending latitudes gives
             no exchange cell and no error; a distorted cell that stays convex is no error either), the
             masked twins (the source cells of every fatal pair have mask 0: create_xgrid.c:1401 skips them before the clip),
             and the mixed ones.
A mixed case holds two codes in different pairs.  The reference reports the first in its loop order, the device in the fixed
order of plan_search_core: grid box 1, grid box 2, then the largest clip code (device_code).

Reached by the searches (make_golden_gc_fatal.py prints the counts): pair cases 1, 2, 5, 6 and 11; grid pairs 1, 2 and the codes
in the fixture's g_code (6).  NOT_REACHED names the rest with the size of the search that did not find them; nothing is asserted
about those."""
import os

import numpy as np

import orc
import polylist_gc_cases as pc

FG_ERR_GEOM = -8
D2R = np.pi / 180.0
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gc_fatal_polygons.npz")

# code -> the reference's text (create_xgrid.c:1577, :1579, :1720, :1795, :1822, :1825; mosaic_util.c:1331, :1526)
MESSAGES = {
    1: "create_xgrid.c(clip_2dx2d_great_circle): grid box 1 is not convex",
    2: "create_xgrid.c(clip_2dx2d_great_circle): grid box 2 is not convex",
    3: "firstIntersect is not in the grid1List",
    4: " not found the next intersection ",
    5: "not return back to the first intersection",
    6: "After clipping, nintersect should be 0",
    7: "inserAfter: point (x,y,z) is not found in the list",
    8: "Error from create_xgrid.c: temp is not in list1",
    # not the reference's: on such a pair its insertIntersect walks a circular list of intersections for ever (mosaic_util.c:1352);
    # the oracle and the device stop after a full turn.  tests/test_gc_fatal_cases_cpu.py starts no reference on these inputs.
    11: "clip_2dx2d_great_circle: insertIntersect finds no node that is not an intersection (the reference's loop over the list, "
        "mosaic_util.c:1352, does not end on this pair of cells)",
}
NO_REFERENCE_TEXT = {11}
# code -> (what the reference calls it, trials of the pair search, trials of the grid-pair search) that did not produce it
NOT_REACHED = {
    3: ("firstIntersect is not in the grid1List", 150000, 150000),
    4: ("not found the next intersection", 150000, 150000),
    7: ("insertIntersect's anchor point is not in the list", 150000, 150000),
    8: ("setInbound: temp is not in list1", 150000, 150000),
    9: ("the oracle's list capacity (GC_CAP 40 nodes; not a check of the reference)", 150000, 150000),
}


def device_code(codes):
    """the code plan_search_core reports for a search whose pairs returned `codes` (positive numbers)"""
    codes = set(codes)
    return 1 if 1 in codes else 2 if 2 in codes else max(codes)


def latlon(nx, ny, w, e, s, n):
    """corner arrays [ny + 1, nx + 1] of a regular lat-lon grid, radians"""
    lon, lat = np.meshgrid((w + np.arange(nx + 1) * ((e - w) / nx)) * D2R, (s + np.arange(ny + 1) * ((n - s) / ny)) * D2R)
    return np.ascontiguousarray(lon), np.ascontiguousarray(lat)


def pair_codes(p, g, cr):
    """{cell: negative code} of the polygon p against every cell of the pc.Grid g that the clip's range test lets through"""
    out = {}
    for d in np.nonzero(pc.range_pass(p, g.cells))[0]:
        c = orc.orc_clip_gc(p, g.cells[d], cr=cr)[0]
        if c < 0:
            out[int(d)] = int(c)
    return out


def list_codes(n, xyz, g, cr):
    """the positive codes over every pair of a polygon list"""
    return {-c for k in range(len(n)) for c in pair_codes(xyz[k, :n[k]], g, cr).values()}


# ------------------------------------------------------------------------------------------------------------------ pair cases
class _HostGrids:
    @staticmethod
    def latlon_corners(nx, ny, w=0.0, e=360.0, s=-90.0, n=90.0):
        return latlon(nx, ny, w, e, s, n)


ORDINARY_KINDS = ("triangle", "octagon", "antipodal", "first_two_coincide")


def ordinary():
    """(n [4], xyz [4, 8, 3]) of ORDINARY_KINDS from polylist_gc_cases.crafted: rings placed by longitude and latitude alone"""
    def make():
        _, kinds, n, xyz = pc.crafted(_HostGrids)
        sel = [kinds.index(k) for k in ORDINARY_KINDS]
        return n[sel].copy(), xyz[sel].copy()
    return pc.cached("gc_fatal_ordinary", make)


def _load():
    d = np.load(FIXTURE)
    grids = [pc.Grid(4, 4, d["lon"][k], d["lat"][k]) for k in range(len(d["lon"]))]
    cases = {}
    for k in range(len(d["n"])):
        n = int(d["n"][k])
        cases[f"code{int(d['code'][k])}_{str(d['recipe'][k])}_{k}"] = dict(code=int(d["code"][k]), poly=np.ascontiguousarray(d["xyz"][k, :n]),
                                                                         grid=int(d["grid"][k]))
    found = {}
    for q in range(len(d["g_code"])):
        nx, ny = int(d["g_nx"][q]), int(d["g_ny"][q])
        found[int(d["g_code"][q])] = dict(nx=nx, ny=ny, lon=np.ascontiguousarray(d["g_lon"][q, :ny + 1, :nx + 1]),
                                          lat=np.ascontiguousarray(d["g_lat"][q, :ny + 1, :nx + 1]), extent=[float(v) for v in d["g_extent"][q]])
    return grids, cases, found


PAIR_GRIDS, PAIR_CASES, _FOUND_GRIDS = _load()
CLEAN_GRID = 0                  # the grid without a displaced corner: where the list without the bad polygon is built


def polylist(case, position):
    """the bad polygon of a pair case among the four ordinary ones, at `position` of the list of five: (n, xyz [5, 8, 3])"""
    n4, v4 = ordinary()
    c = PAIR_CASES[case] if isinstance(case, str) else case
    v = np.zeros((1, 8, 3))
    v[0, :len(c["poly"])] = c["poly"]
    n = np.concatenate([n4[:position], [len(c["poly"])], n4[position:]]).astype(np.int32)
    return n, np.ascontiguousarray(np.concatenate([v4[:position], v, v4[position:]]))


def mixed_polylist(names):
    """the four ordinary polygons with the bad polygons of several pair cases between them: positions 1, 3, ..."""
    n, v = [int(k) for k in ordinary()[0]], [p for p in ordinary()[1]]
    for q, name in enumerate(names):
        p = np.zeros((8, 3))
        p[:len(PAIR_CASES[name]["poly"])] = PAIR_CASES[name]["poly"]
        n.insert(1 + 2 * q, len(PAIR_CASES[name]["poly"]))
        v.insert(1 + 2 * q, p)
    return np.array(n, dtype=np.int32), np.ascontiguousarray(np.array(v))


def area_ref(n, xyz):
    """great_circle_area of each polygon's de-duplicated corners under the _cr oracle: the list's reference areas"""
    P = pc.prims_oracle(True)
    return np.array([pc.own_area(xyz[k, :n[k]], P) for k in range(len(n))])


def clean_reference():
    """(n, xyz, area_ref, pc.Grid, polylist_reference under the _cr oracle) of the four ordinary polygons on the clean grid"""
    def make():
        n, xyz = ordinary()
        ar = area_ref(n, xyz)
        return n, xyz, ar, PAIR_GRIDS[CLEAN_GRID], pc.polylist_reference(n, xyz, ar, PAIR_GRIDS[CLEAN_GRID], pc.prims_oracle(True))
    return pc.cached("gc_fatal_clean_list", make)


def _first(code):
    return next(name for name, c in PAIR_CASES.items() if c["code"] == code)


# name -> the pair cases whose polygons the list holds; every one on the clean grid
MIXED_LISTS = {"grid_box_1_and_code_6": (_first(1), _first(6)), "codes_5_and_6": (_first(5), _first(6))}

# ------------------------------------------------------------------------------------------------------------------ grid cases
SRC = (2, 2) + latlon(2, 2, 3.0, 27.0, -12.0, 12.0)
DST = (3, 3) + latlon(3, 3, 0.0, 30.0, -15.0, 15.0)


def _moved(g, j, i, lat_deg):
    lat = g[3].copy()
    lat[j, i] = lat_deg * D2R
    return (g[0], g[1], g[2], lat)


def grid_result(src, dst, mask, cr):
    """the grid-level oracle: ("n", dict of the exchange grid) or ("code", positive code)"""
    try:
        return "n", orc.orc_create_xgrid_gc(src[0], src[1], dst[0], dst[1], src[2], src[3], dst[2], dst[3], mask=mask, cr=cr)
    except RuntimeError as e:
        r = int(str(e).rsplit(":", 1)[1])
        assert -111 <= r <= -101, r
        return "code", -r - 100


def grid_pair_codes(src, dst, mask, cr):
    """{(source cell, destination cell): positive code} over the pairs of unmasked source cells that the range test lets through"""
    S, T = pc.Grid(*src), pc.Grid(*dst)
    m = np.ones(src[0] * src[1]) if mask is None else np.asarray(mask, dtype=np.float64).ravel()
    return {(s, d): -c for s in range(len(S.cells)) if m[s] > 0.5 for d, c in pair_codes(S.cells[s], T, cr).items()}


def _grid_cases():
    cases = {}

    def add(name, src, dst, clean, mask=None):
        cases[name] = dict(src=src, dst=dst, mask=mask, clean=clean)

    clean = (SRC, DST)
    # the interior source corner moved from the equator to 14 S, past its southern neighbour at 12 S: the two southern source
    # cells turn inside out.  At 11 S the same corner leaves four distorted but convex cells: no error in the reference.
    add("src_cell_not_convex", _moved(SRC, 1, 1, -14.0), DST, clean)
    add("src_cell_distorted_but_convex", _moved(SRC, 1, 1, -11.0), DST, clean)
    # the same corner moved to (8 E, 7 S), across the diagonal of the south-western cell: that cell becomes a dart.  great_circle_area
    # takes every angle below pi, so the re-entrant corner makes its area negative
    dart = (SRC[0], SRC[1], SRC[2].copy(), SRC[3].copy())
    dart[2][1, 1], dart[3][1, 1] = 8.0 * D2R, -7.0 * D2R
    add("src_cell_is_a_dart", dart, DST, clean)
    # cells that are not convex BESIDE the other grid, two degrees from its edge: no pair overlaps, but the clip's range test
    # (create_xgrid.c:1508-1528, 0.05 on x, y, z) lets pairs through, and the reference checks convexity before anything else
    add("src_cell_not_convex_beside_the_grid", _moved((2, 2) + latlon(2, 2, 32.0, 44.0, -12.0, 12.0), 1, 1, -14.0), DST, clean)
    add("dst_cell_not_convex_beside_the_grid", SRC, _moved((3, 3) + latlon(3, 3, 29.0, 59.0, -15.0, 15.0), 1, 1, 14.0), clean)
    # the destination corner (1, 1) moved from 5 S to 14 N, past its northern neighbour at 5 N
    add("dst_cell_not_convex", SRC, _moved(DST, 1, 1, 14.0), clean)
    for code, g in sorted(_FOUND_GRIDS.items()):
        add(f"clip_code_{code}", SRC, (g["nx"], g["ny"], g["lon"], g["lat"]), (SRC, (g["nx"], g["ny"]) + latlon(g["nx"], g["ny"], *g["extent"])))
    add("src_lat_descending", (SRC[0], SRC[1], SRC[2], np.ascontiguousarray(SRC[3][::-1])), DST, clean)
    add("dst_lat_descending", SRC, (DST[0], DST[1], DST[2], np.ascontiguousarray(DST[3][::-1])), clean)
    add("mixed_grid_boxes_1_and_2", _moved(SRC, 1, 1, -14.0), _moved(DST, 1, 1, 14.0), clean)
    # a found destination grid with a second interior corner moved past its northern neighbour, none of whose four cells is in a
    # fatal pair of the found case: grid box 2 in some pairs, the clip code in others
    for code, g in sorted(_FOUND_GRIDS.items()):
        dst = (g["nx"], g["ny"], g["lon"], g["lat"])
        fatal = {d for _, d in grid_pair_codes(SRC, dst, None, True)}
        free = [(j, i) for j in range(1, g["ny"]) for i in range(1, g["nx"])
                if not fatal & {(j - a) * g["nx"] + i - b for a in (0, 1) for b in (0, 1)}]
        if free:
            j, i = free[0]
            north = np.degrees(g["lat"][j + 1, i])
            add(f"mixed_grid_box_2_and_code_{code}", SRC, _moved(dst, j, i, north + 0.9 * (north - np.degrees(g["lat"][j, i]))), cases[f"clip_code_{code}"]["clean"])
    # masked twins: the source cells of every fatal pair with mask 0
    for name in [k for k in cases if k == "src_cell_not_convex" or k.startswith("clip_code_")]:
        c = cases[name]
        mask = np.ones(c["src"][0] * c["src"][1])
        for s, _ in grid_pair_codes(c["src"], c["dst"], None, True):
            mask[s] = 0.0
        add(name + "_masked", c["src"], c["dst"], c["clean"], mask)
    return cases


GRID_CASES = _grid_cases()


def grid_facts(name):
    """per build (plain, _cr): the grid-level result and the codes over every pair; computed once"""
    def make():
        c = GRID_CASES[name]
        return [dict(result=grid_result(c["src"], c["dst"], c["mask"], cr), codes=set(grid_pair_codes(c["src"], c["dst"], c["mask"], cr).values()))
                for cr in (False, True)]
    return pc.cached(("gc_fatal_grid", name), make)


SILENT = [k for k in GRID_CASES if k.endswith("_descending") or k.endswith("_masked") or k == "src_cell_distorted_but_convex"]
FATAL_GRIDS = [k for k in GRID_CASES if k not in SILENT]
MIXED_GRIDS = [k for k in FATAL_GRIDS if k.startswith("mixed_")]


# ------------------------------------------------------------------------------------------------------------------ at import
def _check():
    for name, c in PAIR_CASES.items():
        a, b = pair_codes(c["poly"], PAIR_GRIDS[c["grid"]], False), pair_codes(c["poly"], PAIR_GRIDS[c["grid"]], True)
        assert a == b and set(a.values()) == {-c["code"]}, (name, a, b)
        assert 3 <= len(c["poly"]) <= 8
    per_code = {}
    for c in PAIR_CASES.values():
        per_code[c["code"]] = per_code.get(c["code"], 0) + 1
    assert set(per_code) >= {1, 2, 5, 6} and max(per_code.values()) <= 3, per_code
    assert not set(per_code) & set(NOT_REACHED)
    n4, v4 = ordinary()
    for g in PAIR_GRIDS[:1]:
        for cr in (False, True):
            assert not list_codes(n4, v4, g, cr)
    ref = clean_reference()[4]
    assert not ref["errors"] and len(set(ref["poly"].tolist())) == 3          # all but the antipodal one meet the grid
    for name, c in PAIR_CASES.items():
        n, xyz = polylist(name, 2)
        assert list_codes(n, xyz, PAIR_GRIDS[c["grid"]], True) == {c["code"]}, name
    for name, members in MIXED_LISTS.items():
        n, xyz = mixed_polylist(members)
        want = {PAIR_CASES[m]["code"] for m in members}
        assert len(want) == 2 and list_codes(n, xyz, PAIR_GRIDS[CLEAN_GRID], True) == want == list_codes(n, xyz, PAIR_GRIDS[CLEAN_GRID], False), name
    covered = set()
    for name in GRID_CASES:
        plain, cr = grid_facts(name)
        assert plain["result"][0] == cr["result"][0] and plain["codes"] == cr["codes"], name
        c = GRID_CASES[name]
        assert max(c["src"][0], c["src"][1], c["dst"][0], c["dst"][1]) <= 4
        if name in SILENT:
            assert cr["result"][0] == "n" and not cr["codes"], (name, cr)
        else:
            assert cr["result"][0] == "code" and plain["result"][1] == cr["result"][1] and cr["result"][1] in cr["codes"], (name, plain, cr)
            if name in MIXED_GRIDS:
                assert len(cr["codes"]) == 2, (name, cr)
            else:
                assert cr["codes"] == {cr["result"][1]}, (name, cr)
                covered.add(cr["result"][1])
        kind, clean = grid_result(c["clean"][0], c["clean"][1], None, True)
        assert kind == "n" and clean["n"] > 0, name
    assert covered >= {1, 2}, covered
    assert grid_facts("src_lat_descending")[1]["result"][1]["n"] == 0
    return per_code, covered


PAIR_CODES_COVERED, GRID_CODES_COVERED = _check()
