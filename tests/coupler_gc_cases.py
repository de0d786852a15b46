"""make_coupler_mosaic.c's GREAT_CIRCLE_CLIP branches (:1198-2127, :2466-2811 where clip_method == GREAT_CIRCLE_CLIP; one process,
no nest, one ocean tile, interp_order 1) restated line by line over a primitive set passed in (polylist_gc_cases.Prims:
clip_2dx2d_great_circle, great_circle_area, get_grid_great_circle_area; the unit vectors are latlon2xyz's), and the cases the
great-circle coupler tests share.  It is run once with the compiled reference's primitives and once with the _cr oracle's.

The reference prunes nothing in this branch (is = 0 .. nx-1, js = 0 .. ny-1, :1253-1267, :2549-2556); the restatement skips a pair
only by the clip's own first test (create_xgrid.c:1508-1528, polylist_gc_cases.range_pass) and keeps the skipped pairs for the CPU
test, which gives every tenth to the reference's clip.  It also keeps every weighted single-clip term (`terms`) and, per
atmosphere x land entry, the terms it adds up (`axl_tids`), so that the CPU test can account for every difference term by term.  Kept as written there: the lnd_same_as_atm copy of the cell's four corners (:1426-1437, no clip, no vertex-count check), the
order of every sum, the `> 0` / `> MIN_AREA_FRAC` guards, min()'s operand order, the masks.  Line numbers are the reference's."""
import numpy as np

import polylist_gc_cases as pc

MIN_AREA_FRAC = 1.0e-4          # :148
TOLORENCE = 1.0e-4              # :149


def _new(names):
    return {k: [] for k in names + ("area",)}


def reference_coupler_gc(atm, lnd, ocn, omask, P, thresh=1.0e-6, ocn_south_ext=0, reverse_sums=False, skip_same_copy=False, want_skipped=False):
    """atm: list of pc.Grid; lnd: None (lnd_same_as_atm) or a list; ocn: one pc.Grid; omask [nyo, nxo]; P: the primitives.
    reverse_sums / skip_same_copy: deliberately wrong variants (the tests of this restatement's teeth)."""
    same = lnd is None
    L = atm if same else lnd
    O = ocn
    om = np.ascontiguousarray(omask, dtype=np.float64).reshape(-1)
    oml = om.tolist()
    area_A = [P.grid_area(g.nx, g.ny, g.lon, g.lat) for g in atm]                   # :607
    area_L = area_A if same else [P.grid_area(g.nx, g.ny, g.lon, g.lat) for g in L]  # :731
    area_O = P.grid_area(O.nx, O.ny, O.lon, O.lat)                                  # :890
    nta, ntl = len(atm), len(L)
    axl = [[_new(("ia", "ja", "il", "jl")) for _ in range(ntl)] for _ in range(nta)]
    axo = [_new(("ia", "ja", "io", "jo", "tid")) for _ in range(nta)]
    cover = dict(remembered={}, poly_x_ocn={}, pole_ocn_cells=0, dropped=0)
    skipped = []                                                                    # want_skipped: EVERY pair the range test dropped
    terms = []                                                                      # every weighted single-clip term: polygon, area, area * fraction

    def term(v, ua, w):
        terms.append(dict(v=v, ua=ua, w=w))
        return len(terms) - 1

    axl_tids = [[[] for _ in range(ntl)] for _ in range(nta)]                       # per atmosphere x land entry: the terms it adds up, in order
    north = np.array([0.0, 0.0, 1.0])
    cover["pole_ocn_cells"] = int(np.count_nonzero((np.abs(O.cells - north).max(axis=2) <= 1e-10).any(axis=1)))

    for na, ga in enumerate(atm):                                                   # :1202
        for la in range(ga.nx * ga.ny):                                             # :1346
            ia, ja = la % ga.nx, la // ga.nx
            a = ga.cells[la]                                                        # :1367-1375
            found = []
            for nl, gl in enumerate(L):                                             # :1396
                if same:
                    cand = [la] if nl == na else []                                 # :1427: every other pair has n_out = 0
                else:
                    go = pc.range_pass(a, gl.cells)
                    cand = np.nonzero(go)[0]
                    if want_skipped:
                        skipped += [(a, gl.cells[d]) for d in np.nonzero(~go)[0]]
                for ll in cand:
                    ll = int(ll)
                    if same and not skip_same_copy:
                        n_out, v = 4, gl.cells[ll].copy()                           # :1428-1433
                    else:
                        n_out, v = P.clip(a, gl.cells[ll])                          # :1439
                        if n_out < 0:
                            raise RuntimeError(f"{P.name}: clip error {n_out}")
                    if n_out > 0:                                                   # :1483
                        xarea = P.area(v)                                           # :1485
                        min_area = min(area_L[nl][ll], area_A[na][la])              # :1488
                        if xarea / min_area > thresh:                               # :1507
                            found.append(dict(nl=nl, ll=ll, v=v, area=0.0, min_area=min_area, tids=[]))
                            cover["remembered"][n_out] = cover["remembered"].get(n_out, 0) + 1
            go_o = pc.range_pass(a, O.cells)
            go_f = [pc.range_pass(f["v"], O.cells) for f in found]
            if want_skipped:
                skipped += [(a, O.cells[d]) for d in np.nonzero(~go_o)[0]]
                for f, g in zip(found, go_f):                                       # the remembered polygons' pairs too (:1666)
                    skipped += [(f["v"], O.cells[d]) for d in np.nonzero(~g)[0]]
            touched = go_o.copy()
            for g in go_f:
                touched |= g
            for lo in np.nonzero(touched)[0]:                                       # :1555 (the other cells: every clip returns 0)
                lo = int(lo)
                ocn_frac = oml[lo]                                                  # :1601
                lnd_frac = 1 - ocn_frac
                if ocn_frac > MIN_AREA_FRAC and go_o[lo]:                           # :1604
                    n_out, v = P.clip(a, O.cells[lo])                               # :1610
                    if n_out < 0:
                        raise RuntimeError(f"{P.name}: clip error {n_out}")
                    if n_out > 0:
                        ua = P.area(v)
                        xarea = ua * ocn_frac                                       # :1638
                        min_area = min(area_O[lo], area_A[na][la])                  # :1643
                        if xarea / min_area > thresh:                               # :1646
                            t = axo[na]
                            t["tid"].append(term(v, ua, xarea))
                            t["area"].append(xarea); t["io"].append(lo % O.nx); t["jo"].append(lo // O.nx); t["ia"].append(ia); t["ja"].append(ja)
                if lnd_frac > MIN_AREA_FRAC:                                        # :1662
                    for f, g in zip(found, go_f):                                   # :1664
                        if not g[lo]:
                            continue
                        n_out, v = P.clip(f["v"], O.cells[lo])                      # :1666
                        if n_out < 0:
                            raise RuntimeError(f"{P.name}: clip error {n_out}")
                        if n_out > 0:
                            ua = P.area(v)
                            xarea = ua * lnd_frac                                   # :1674
                            if xarea / f["min_area"] > thresh:                      # :1677-1678
                                f["area"] += xarea                                  # :1689
                                f["tids"].append(term(v, ua, xarea))
                                cover["poly_x_ocn"][n_out] = cover["poly_x_ocn"].get(n_out, 0) + 1
            for f in found:                                                         # :1701
                if f["area"] / f["min_area"] > thresh:                              # :1703-1706
                    gl = L[f["nl"]]
                    t = axl[na][f["nl"]]
                    axl_tids[na][f["nl"]].append(f["tids"])
                    t["area"].append(f["area"]); t["ia"].append(ia); t["ja"].append(ja); t["il"].append(f["ll"] % gl.nx); t["jl"].append(f["ll"] // gl.nx)
                else:
                    cover["dropped"] += 1

    lxo = []                                                                        # :2470-2690
    if not same:
        for nl, gl in enumerate(L):
            t = _new(("il", "jl", "io", "jo", "tid"))
            for ll in range(gl.nx * gl.ny):                                         # :2598
                b = gl.cells[ll]
                go = pc.range_pass(b, O.cells)
                if want_skipped:
                    skipped += [(b, O.cells[d]) for d in np.nonzero(~go)[0]]
                for lo in np.nonzero(go & (om > MIN_AREA_FRAC))[0]:                 # :2628
                    lo = int(lo)
                    ocn_frac = oml[lo]                                              # :2660
                    n_out, v = P.clip(b, O.cells[lo])                               # :2662
                    if n_out < 0:
                        raise RuntimeError(f"{P.name}: clip error {n_out}")
                    if n_out > 0:
                        ua = P.area(v)
                        xarea = ua * ocn_frac                                       # :2670
                        min_area = min(area_O[lo], area_L[nl][ll])                  # :2673
                        if xarea / min_area > thresh:                               # :2674
                            t["tid"].append(term(v, ua, xarea))
                            t["area"].append(xarea); t["io"].append(lo % O.nx); t["jo"].append(lo // O.nx); t["il"].append(ll % gl.nx); t["jl"].append(ll // gl.nx)
            lxo.append(t)

    def arrays(t):
        return {k: np.array(v, dtype=np.float64 if k == "area" else np.int64) for k, v in t.items()}

    axl = [[arrays(t) for t in row] for row in axl]
    axo = [arrays(t) for t in axo]
    lxo = [arrays(t) for t in lxo]
    seq = (lambda n: range(n - 1, -1, -1)) if reverse_sums else range

    def add(dst, idx, t):                                                           # :1781-1784, :1807-1810
        for i in seq(len(idx)):
            dst[idx[i]] += t["area"][i]

    l_sum = [np.zeros(g.nx * g.ny) for g in L]
    o_sum = np.zeros(O.nx * O.ny)
    a_sums = []
    for na, ga in enumerate(atm):                                                   # :1763
        a_sum = np.zeros(ga.nx * ga.ny)                                             # (the device keeps a_area at order 1 too: the lists in this order)
        for nl, gl in enumerate(L):
            t = axl[na][nl]
            add(a_sum, t["ja"] * ga.nx + t["ia"], t)
            add(l_sum[nl], t["jl"] * gl.nx + t["il"], t)
        t = axo[na]
        add(a_sum, t["ja"] * ga.nx + t["ia"], t)
        add(o_sum, t["jo"] * O.nx + t["io"], t)
        a_sums.append(a_sum)
    e = ocn_south_ext
    ocn_frac = o_sum / area_O                                                       # :2037
    nbad = int(np.count_nonzero(np.abs(om - ocn_frac)[e * O.nx:] > TOLORENCE))      # :2038
    ocean = dict(mask=ocn_frac.reshape(O.ny, O.nx), o_area=o_sum.reshape(O.ny, O.nx), area=area_O.reshape(O.ny, O.nx))
    land = [dict(mask=(l_sum[nl] / area_L[nl]).reshape(gl.ny, gl.nx), l_area=l_sum[nl].reshape(gl.ny, gl.nx), area=area_L[nl].reshape(gl.ny, gl.nx))
            for nl, gl in enumerate(L)]                                             # :2087-2094
    atmos = [dict(a_area=a_sums[na].reshape(ga.ny, ga.nx), area=area_A[na].reshape(ga.ny, ga.nx)) for na, ga in enumerate(atm)]
    return dict(axl=axl, axo=axo, lxo=lxo, ocean=ocean, land=land, atmos=atmos, nbad=nbad, cover=cover, same=same, skipped=skipped,
                terms=terms, axl_tids=axl_tids)


# ------------------------------------------------------------------------------------------------------------------- the cases
def quarter_mask(nx, ny, seed):
    """ocean fractions in {0, 1/4, 1/2, 3/4, 1}, seeded"""
    return np.random.default_rng(seed).integers(0, 5, size=(ny, nx)) / 4.0


def _ocean(fg, nx, ny, seed, value=None):
    oo, oa = fg.latlon_corners(nx, ny, 0.0, 360.0, -78.0, 90.0)
    m = quarter_mask(nx, ny, seed) if value is None else np.full((ny, nx), float(value))
    g = fg.coupler_ocean_grid(np.degrees(oo), np.degrees(oa), m)
    assert g["ocn_south_ext"] == 1 and g["ny"] == ny + 1
    return pc.Grid(nx, ny + 1, g["x"], g["y"]), g["omask"]


def _cube(fg, ni):
    lon, lat = fg.gnomonic_ed_corners(ni)
    return [pc.Grid(ni, ni, lon[t], lat[t]) for t in range(6)]


def same_c5(fg, value=None):
    """land on the atmosphere grid: C5 (the pole strictly inside the centre cell of two tiles) over a 30 x 20 lat-lon ocean from -78 to
    90 degrees (its top row: degenerate pole cells) with the southern extension row"""
    ocn, om = _ocean(fg, 30, 20, 5, value)
    return dict(atm=_cube(fg, 5), lnd=None, ocn=ocn, omask=om, ext=1)


def own_c4(fg, split=False):
    """land of its own: C4, a 15 x 7 lat-lon land over -88 .. 88 degrees from 13 E (split: two tiles, cut at the 8th column), a
    24 x 14 lat-lon ocean from -78 to 90 degrees with the extension row"""
    ocn, om = _ocean(fg, 24, 14, 4)
    ll, la = fg.latlon_corners(15, 7, 13.0, 373.0, -88.0, 88.0)
    lnd = [pc.Grid(8, 7, ll[:, :9], la[:, :9]), pc.Grid(7, 7, ll[:, 8:], la[:, 8:])] if split else [pc.Grid(15, 7, ll, la)]
    return dict(atm=_cube(fg, 4), lnd=lnd, ocn=ocn, omask=om, ext=1)


CASES = {"same_c5": same_c5, "own_c4": own_c4, "own_c4_two_land_tiles": lambda fg: own_c4(fg, True),
         "same_c5_omask0": lambda fg: same_c5(fg, 0.0), "same_c5_omask1": lambda fg: same_c5(fg, 1.0)}


def reference_of(name, fg, P, **kw):
    """(case, restatement under the primitives P), computed once per session"""
    def make():
        c = CASES[name](fg)
        return c, reference_coupler_gc(c["atm"], c["lnd"], c["ocn"], c["omask"], P, ocn_south_ext=c["ext"], **kw)
    return pc.cached((name, P.name, tuple(sorted(kw.items()))), make)
