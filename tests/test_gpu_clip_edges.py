"""The Sutherland-Hodgman pass of the quad clip kernel (d_clip_quad_sh, csrc/xgrid_kernels.hip) at the smallest shapes that reach
each of its branches: clipped polygons of 3 to 8 vertices, candidate pairs that come out empty -- at each of the four cutting
edges --, pole-fixed source cells of more than four vertices, the `wrap` branch and both signs of the +-2 pi shift, a pair the
kernel hands to the general kernel, a pair count that is no multiple of the block and the exactly sized search.

Every case with a rectilinear target runs on the rectilinear path (k_clip_quad<., true>) and on the generic one
(fg_set_search_rect(0): <., false>); a curvilinear target (tripolar, a tilted window) has the generic path only.  Each run is
compared with the CPU oracle (tests/orc.py: orc_create_xgrid, and the compiled reference's create_xgrid where it was
built), which share no code with the kernels: index lists equal, areas and the two centroid integrals equal in bits (on a host
whose libm runs the FMA build of sin / cos, orc.host_has_fma -- the oracle calls the host's libm; elsewhere 1e-10), every
exchange cell compared.

That a case holds what it is there for is asserted on the CPU: `trace` below walks the pairs that pass create_xgrid's
bounding-box tests through a plain Sutherland-Hodgman loop (create_xgrid.c:1270-1340) over the oracle's cell records and notes the
vertex count after every cutting edge.  It only classifies pairs; no result is compared with it."""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
D2R = np.pi / 180
PI, TPI = np.pi, 2 * np.pi


def latlon_window(lon0, lon1, lat0, lat1, nlon, nlat):
    """corner arrays of a regular lat-lon window (as tests/test_gpu_rect.py builds them)"""
    i = np.arange(nlon + 1, dtype=np.float64); j = np.arange(nlat + 1, dtype=np.float64)
    lon = (lon0 + i * ((lon1 - lon0) / nlon)) * D2R
    lat = (lat0 + j * ((lat1 - lat0) / nlat)) * D2R
    return (np.ascontiguousarray(np.broadcast_to(lon[None, :], (nlat + 1, nlon + 1))),
            np.ascontiguousarray(np.broadcast_to(lat[:, None], (nlat + 1, nlon + 1))))


# ------------------------------------------------------------------------------------------------ classification on the CPU
def _inside(x0, y0, x1, y1, x, y):
    return (x - x0) * (y1 - y0) + (x0 - x1) * (y - y0) <= 1.e-12


def _pimod(v):
    return v + TPI if v < -PI else (v - TPI if v > PI else v)


def trace(S, D):
    """For every pair of a source cell of S and a destination cell of D (orc.orc_cell_struct records) that passes the
    bounding-box tests of create_xgrid_2dx2d (create_xgrid.c:1058-1078): n1, n2, the shift, whether the cells were wrapped, and
    the vertex count after each cutting edge (a list that ends at the first 0) and the crossings of each cutting line."""
    out = []
    for s in range(len(S["nvert"])):
        n1 = int(S["nvert"][s])
        for d in range(len(D["nvert"])):
            if D["lat_min"][d] >= S["lat_max"][s] or D["lat_max"][d] <= S["lat_min"][s]:
                continue
            n2 = int(D["nvert"][d])
            x2, y2 = D["vlon"][d, :n2].copy(), D["vlat"][d, :n2].copy()
            lo_min, lo_max = D["lon_min"][d], D["lon_max"][d]
            dx = D["lon_avg"][d] - S["lon_avg"][s]
            shift = TPI if dx < -PI else (-TPI if dx > PI else 0.0)
            if shift != 0.0:
                lo_min += shift; lo_max += shift; x2 += shift
            if lo_min >= S["lon_max"][s] or lo_max <= S["lon_min"][s]:
                continue
            x1, y1 = S["vlon"][s, :n1].copy(), S["vlat"][s, :n1].copy()
            wrap = bool(np.any((x1 > TPI) | (x1 < 0.0)))
            if wrap:
                x1 = np.array([_pimod(v) for v in x1]); x2 = np.array([_pimod(v) for v in x2])
            poly = list(zip(x1, y1))
            counts, cross = [], []
            e0 = (x2[n2 - 1], y2[n2 - 1])
            for e in range(n2):
                e1 = (x2[e], y2[e])
                new, nc = [], 0
                px, py = poly[-1]
                pin = _inside(e0[0], e0[1], e1[0], e1[1], px, py)
                for (qx, qy) in poly:
                    qin = _inside(e0[0], e0[1], e1[0], e1[1], qx, qy)
                    if qin != pin:
                        nc += 1
                        dy1, dy2, dx1, dx2 = qy - py, e1[1] - e0[1], qx - px, e1[0] - e0[0]
                        ds1, ds2 = py * qx - qy * px, e0[1] * e1[0] - e1[1] * e0[0]
                        det = dy2 * dx1 - dy1 * dx2
                        new.append(((dx2 * ds1 - dx1 * ds2) / det, (dy2 * ds1 - dy1 * ds2) / det))
                    if qin:
                        new.append((qx, qy))
                    px, py, pin = qx, qy, qin
                poly = new
                counts.append(len(poly)); cross.append(nc)
                e0 = e1
                if not poly:
                    break
            out.append(dict(s=s, d=d, n1=n1, n2=n2, shift=shift, wrap=wrap, counts=counts, cross=cross))
    return out


# ------------------------------------------------------------------------------------------------ the cases
def _c(fg, ni, tiles=range(6)):
    lon, lat = fg.gnomonic_ed_corners(ni)
    return [(ni, ni, lon[t], lat[t]) for t in tiles]


def _ll(fg, nlon, nlat):
    lo, la = fg.latlon_corners(nlon, nlat)
    return (nlon, nlat, lo, la)


def _win(*w):
    lo, la = latlon_window(*w)
    return (w[4], w[5], lo, la)


def _diamond():
    """one source cell standing on a corner over the middle cell of a 3x3 window of 10 degree cells: its bounding box reaches
    into all eight neighbours, the cell itself only into the four that share an edge with the middle one"""
    lon = np.array([[15.0, 23.0], [7.0, 15.0]]) * D2R          # corners (j, i): south, east / west, north
    lat = np.array([[-8.0, 0.5], [-0.5, 8.0]]) * D2R
    return (1, 1, lon, lat)


def _chevron():
    """one source cell that is not convex (an arrow head pointing north): the line of a southern cutting edge crosses it four
    times, which the quad kernel's two-crossings scheme hands to the general kernel"""
    lon = np.array([[10.0, 15.0], [15.0, 20.0]]) * D2R          # corners (j, i): west tip, notch / apex, east tip
    lat = np.array([[-8.0, -2.0], [7.0, -8.0]]) * D2R
    return (1, 1, lon, lat)


def _tilted(deg=30.0):
    """a 3x3 window of 10 degree cells turned about its centre (40 E, 10 N): curvilinear, so the search takes the generic path,
    and no cutting edge runs along an axis -- a cell can pass the bounding-box tests and lie wholly beyond the FIRST edge"""
    u = np.array([-15.0, -5.0, 5.0, 15.0])
    uu, vv = np.meshgrid(u, u)
    c, s = np.cos(deg * D2R), np.sin(deg * D2R)
    return (3, 3, np.ascontiguousarray((40.0 + c * uu - s * vv) * D2R), np.ascontiguousarray((10.0 + s * uu + c * vv) * D2R))


def _tri(fg):
    lon, lat = fg.tripolar_corners(24, 16)
    return (24, 16, lon, lat)


# name -> (source grids, target grid)
def _cases(fg):
    return {
        "C8 -> 45x23": (_c(fg, 8), _ll(fg, 45, 23)),
        "C12 -> 45x23": (_c(fg, 12), _ll(fg, 45, 23)),
        "lat-lon 12x8 -> lat-lon 20x11": ([_ll(fg, 12, 8)], _ll(fg, 20, 11)),
        "lat-lon 12x8 -> tripolar 24x16": ([_ll(fg, 12, 8)], _tri(fg)),
        "C6 -> lat-lon 20x11": (_c(fg, 6), _ll(fg, 20, 11)),
        "C6 -> tripolar 24x16": (_c(fg, 6), _tri(fg)),
        "window -30..40 -> window 330..390": ([_win(-30, 40, -20, 30, 7, 5)], _win(330, 390, -25, 35, 9, 8)),
        "window 330..390 -> window -30..40": ([_win(330, 390, -25, 35, 9, 8)], _win(-30, 40, -20, 30, 7, 5)),
        "one cell on its corner -> 3x3": ([_diamond()], _win(0, 30, -15, 15, 3, 3)),
        "6x6 window -> tilted 3x3": ([_win(19, 61, -11, 31, 6, 6)], _tilted()),
        "one cell that is not convex -> 3x3": ([_chevron()], _win(0, 30, -15, 15, 3, 3)),
    }


_memo = {}


def case(fg, name):
    """grids, the oracle's lists (orders 1 and 2, tile by tile) and the CPU classification of a case, made once"""
    if name in _memo:
        return _memo[name]
    srcs, tgt = _cases(fg)[name]
    nx2, ny2, lo, la = tgt
    D = orc.orc_cell_struct(nx2, ny2, lo, la)
    tr = []
    for (nx, ny, lon, lat) in srcs:
        tr += trace(orc.orc_cell_struct(nx, ny, lon, lat), D)
    c = dict(name=name, srcs=srcs, tgt=tgt, trace=tr, oracle={}, ref={})
    for order in (1, 2):
        c["oracle"][order] = [orc.orc_create_xgrid(order, nx, ny, nx2, ny2, lon, lat, lo, la) for (nx, ny, lon, lat) in srcs]
        if orc.ref_available():
            c["ref"][order] = [orc.ref_create_xgrid(order, nx, ny, nx2, ny2, lon, lat, lo, la) for (nx, ny, lon, lat) in srcs]
    _memo[name] = c
    return c


def search(fg, c, order, rect, exact=False):
    L = fg.lib()
    L.fg_set_search_rect(1 if rect else 0); L.fg_set_search_mode(1 if exact else 0)
    try:
        grids = [fg.GridConfig(nx, ny, lon, lat) for (nx, ny, lon, lat) in c["srcs"]]
        nx2, ny2, lo, la = c["tgt"]
        p = fg.XgridPlan.create(order, grids, fg.GridConfig(nx2, ny2, lo, la))
        x = p.get_xgrid()                              # before finalize: c1 / c2 are the two centroid integrals
        st = p.stats()
        p.destroy()
        return x, st
    finally:
        L.fg_set_search_rect(1); L.fg_set_search_mode(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_equals_the_oracle(x, lists, order, what):
    """every exchange cell of the plan against the per-tile lists of an oracle, in the reference's order"""
    n = sum(o["n"] for o in lists)
    assert len(x["area"]) == n > 0, (what, len(x["area"]), n)
    cat = lambda k: np.concatenate([o[k] for o in lists])
    assert np.array_equal(x["t_in"], np.concatenate([np.full(o["n"], t, dtype=np.int32) for t, o in enumerate(lists)])), what
    for k in ("i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(x[k], cat(k)), (what, k)
    pairs = [("area", "area")] + ([("c1", "clon"), ("c2", "clat")] if order == 2 else [])
    for kx, ko in pairs:
        a, b = x[kx], cat(ko)
        assert a.shape == b.shape
        assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b)), (what, kx)
        if orc.host_has_fma():
            nb = int(np.count_nonzero(bits(a) != bits(b)))
            assert nb == 0, (what, kx, nb, "of", a.size, "differ in bits")


def check(fg, name, order, rect, exact=False, rectilinear_target=True):
    c = case(fg, name)
    x, st = search(fg, c, order, rect, exact)
    what = f"{name}, order {order}, {'rectilinear' if rect else 'generic'} path" + (", exactly sized" if exact else "")
    assert (st["bins"] == 0) == (rect and rectilinear_target), (what, "took the other path", st)
    assert_equals_the_oracle(x, c["oracle"][order], order, what + " against the CPU oracle")
    if c["ref"]:
        assert_equals_the_oracle(x, c["ref"][order], order, what + " against the compiled reference")
    return c, st


def final_counts(c):
    """vertex counts of the polygons that are left after the last cutting edge"""
    return {t["counts"][-1] for t in c["trace"] if len(t["counts"]) == t["n2"] and t["counts"][-1] > 0}


def emptied_at(c):
    """the cutting edges (0..3) at which some candidate pair's polygon became empty"""
    return {len(t["counts"]) - 1 for t in c["trace"] if t["counts"][-1] == 0}


PATHS = [True, False]
PATH_IDS = ["rect", "generic"]


@pytest.mark.parametrize("rect", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", ["C8 -> 45x23", "C12 -> 45x23"])
def test_clipped_polygons_of_3_to_7_vertices_and_empty_pairs(fg, gpu_ok, name, order, rect):
    """Cubed sphere onto a coarse lat-lon grid: triangles to heptagons, pairs that come out empty, pole-fixed source cells
    (n1 = 5: the quad kernel takes them on the rectilinear path and defers them on the generic one), wrapped cells and both
    signs of the shift, a last block that is not full.  (Neither grid pair holds an octagon -- the CPU classification finds
    3..6 in C8 and 3..7 in C12; the case of one cell on its corner below has the 8.)"""
    c, st = check(fg, name, order, rect)
    assert final_counts(c) >= ({3, 4, 5, 6, 7} if name.startswith("C12") else {3, 4, 5, 6}), sorted(final_counts(c))
    assert st["pairs"] > st["nonempty"] > 0, st                        # candidate pairs that come out empty
    assert st["pairs"] % 256 != 0, st                                  # the last block of the clip is not full
    assert len(emptied_at(c)) >= 3
    assert any(t["n1"] > 4 and t["counts"][-1] > 0 for t in c["trace"])
    assert {np.sign(t["shift"]) for t in c["trace"] if t["wrap"] and t["counts"][-1] > 0} == {-1.0, 0.0, 1.0}
    if not rect:
        assert st["deferred"] > 0, st


def test_the_cases_hold_every_vertex_count_from_3_to_8(fg):
    have = set()
    for name in ("C8 -> 45x23", "C12 -> 45x23", "one cell on its corner -> 3x3"):
        have |= final_counts(case(fg, name))
    assert have >= {3, 4, 5, 6, 7, 8}, sorted(have)


@pytest.mark.parametrize("rect", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("order", [1, 2])
def test_pole_fixed_source_cells_of_more_than_four_vertices(fg, gpu_ok, order, rect):
    """C6 -> lat-lon 20x11: the cells at the cube's polar corners have five vertices after fix_lon.  (A global lat-lon SOURCE,
    12x8, has none -- its polar cells keep four vertices -- so it runs here as one more plain case and the cubed sphere brings
    the n1 > 4.)  On the rectilinear path the quad kernel clips them; on the generic path they are deferred."""
    c, st = check(fg, "C6 -> lat-lon 20x11", order, rect)
    assert any(t["n1"] > 4 and t["counts"][-1] > 0 for t in c["trace"])
    assert (st["deferred"] > 0) == (not rect), st
    c, _ = check(fg, "lat-lon 12x8 -> lat-lon 20x11", order, rect)
    assert all(t["n1"] == 4 for t in c["trace"])


@pytest.mark.parametrize("order", [1, 2])
def test_pole_fixed_cells_onto_a_curvilinear_target(fg, gpu_ok, order):
    """a tripolar target is not rectilinear (the call falls back to the generic path): source cells AND destination cells of five
    vertices, all deferred to the general kernel, next to the quads the changed pass clips"""
    c, st = check(fg, "C6 -> tripolar 24x16", order, True, rectilinear_target=False)
    assert any(t["n1"] > 4 for t in c["trace"]) and any(t["n2"] > 4 for t in c["trace"])
    assert st["deferred"] > 0 and emptied_at(c) == {0, 1, 2, 3}, (st, emptied_at(c))
    check(fg, "lat-lon 12x8 -> tripolar 24x16", order, True, rectilinear_target=False)


@pytest.mark.parametrize("rect", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("order", [1, 2])
def test_windows_across_the_zero_meridian_and_both_signs_of_the_shift(fg, gpu_ok, order, rect):
    """a window at -30..40 deg under one at 330..390 (shift -2 pi), and the two exchanged (cells beyond 2 pi: the `wrap`
    branch, shift +2 pi)"""
    c, _ = check(fg, "window -30..40 -> window 330..390", order, rect)
    assert any(t["shift"] < 0 and t["counts"][-1] > 0 for t in c["trace"])
    c, _ = check(fg, "window 330..390 -> window -30..40", order, rect)
    assert any(t["wrap"] and t["shift"] > 0 and t["counts"][-1] > 0 for t in c["trace"])


@pytest.mark.parametrize("rect", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("order", [1, 2])
def test_one_cell_on_its_corner_over_a_3x3_window(fg, gpu_ok, order, rect):
    """Nine candidate pairs: an octagon in the middle, four triangles, and four pairs that come out empty -- at the second,
    third and fourth cutting edge.  (Against a cell whose edges run along the axes no polygon can empty at the FIRST edge: a
    polygon wholly beyond that edge fails the bounding-box test and is no candidate.  The tilted window below has it.)"""
    c, st = check(fg, "one cell on its corner -> 3x3", order, rect)
    assert emptied_at(c) == {1, 2, 3} and final_counts(c) == {3, 8}, (emptied_at(c), final_counts(c))
    assert st["pairs"] > st["nonempty"] > 0, st


@pytest.mark.parametrize("order", [1, 2])
def test_a_polygon_empties_at_each_of_the_four_cutting_edges(fg, gpu_ok, order):
    c, st = check(fg, "6x6 window -> tilted 3x3", order, True, rectilinear_target=False)
    assert emptied_at(c) == {0, 1, 2, 3}, emptied_at(c)
    assert st["pairs"] > st["nonempty"] > 0, st


@pytest.mark.parametrize("rect", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("order", [1, 2])
def test_a_pair_the_quad_kernel_defers(fg, gpu_ok, order, rect):
    """The issue's shape for this case -- an intermediate polygon of more than eight vertices -- does not exist among convex grid
    cells, on either path.  A half-plane cut of a convex n-gon leaves at most n + 1 vertices, and it gains one only by cutting
    off exactly one vertex.  A quad cut by a quad's four lines therefore ends at 8 at the most (the cell on its corner above
    reaches it) -- and the generic path's quad kernel takes nothing but quads.  On the rectilinear path, 9 needs a source cell of
    five vertices that loses exactly one vertex to EACH of the four cuts.  The only five-vertex cells a grid has are the
    pole-fixed ones of fix_lon, whose two added vertices lie on the line lat = +-pi/2 with an edge of constant latitude between
    them, and two of the cutter's four lines are lines of constant latitude: such a line cuts off both pole vertices or
    neither, never exactly one, so at least one cut gains nothing and the count stays at 8 or below.  (The CPU classification
    agrees: no case here exceeds 8.)  `ncross + popc(inmask) > CLIP_SLOTS` is thus a guard no grid pair reaches; the kernel's other reason to
    hand a pair on, a cutting line that crosses the polygon more than twice, is reached by a source cell that is not convex, on
    both paths, and that is the case kept here."""
    c, st = check(fg, "one cell that is not convex -> 3x3", order, rect)
    assert max(max(t["cross"]) for t in c["trace"]) == 4
    assert st["deferred"] > 0, st


@pytest.mark.parametrize("rect", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("order", [1, 2])
def test_exactly_sized_search(fg, gpu_ok, order, rect):
    _, st = check(fg, "C8 -> 45x23", order, rect, exact=True)
    assert st["exact_mode"] == 1 and st["pairs"] % 256 != 0, st
