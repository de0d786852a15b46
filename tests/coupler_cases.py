"""make_coupler_mosaic.c:1198-2127 and :2466-2811 restated line by line over the reference's own compiled primitives (fix_lon,
clip_2dx2d, poly_area, poly_ctrlon, poly_ctrlat, get_grid_area from oracle/_ref/libfrenc_ref.so), and the cases the coupler tests
share.  make_coupler_mosaic.c is one main() bound to netCDF and mpp: the LOOPS below are a restatement (legacy clip, one process,
no nest, one ocean tile), every number in them comes out of the reference's object code.  Line numbers are the reference's.

Kept as written there: the lnd_same_as_atm copy of the land cell's vertices (:1463-1477), the tile-wide latitude bands
(:1269-1341, :2558-2595), the `continue` of :1614 that also skips the land branch, the latitude test of :1669 (it compares the
polygon with ya_max / ya_min, not with the ocean cell), the order of every sum, the `> 0` guards, the masks."""
import ctypes as C
import math

import numpy as np

import orc

MIN_AREA_FRAC = 1.0e-4          # :148
TOLORENCE = 1.0e-4              # :149
MV = 20
_Buf = C.c_double * 50


class Prim:
    """the reference's primitives on Python lists"""

    def __init__(self, R):
        self.R = R
        self.a, self.b, self.c, self.d, self.xo, self.yo = _Buf(), _Buf(), _Buf(), _Buf(), _Buf(), _Buf()

    def fix_lon(self, x, y, tlon):
        n = len(x)
        self.a[:n] = x
        self.b[:n] = y
        m = self.R.fix_lon(self.a, self.b, n, tlon)
        return self.a[:m], self.b[:m]

    def clip(self, x1, y1, x2, y2):
        n1, n2 = len(x1), len(x2)
        self.a[:n1] = x1; self.b[:n1] = y1; self.c[:n2] = x2; self.d[:n2] = y2
        m = self.R.clip_2dx2d(self.a, self.b, n1, self.c, self.d, n2, self.xo, self.yo)
        return self.xo[:m], self.yo[:m]

    def _put(self, x, y):
        n = len(x)
        self.a[:n] = x
        self.b[:n] = y
        return n

    def area(self, x, y):
        return self.R.poly_area(self.a, self.b, self._put(x, y))

    def ctrlon(self, x, y, clon):
        return self.R.poly_ctrlon(self.a, self.b, self._put(x, y), clon)

    def ctrlat(self, x, y):
        return self.R.poly_ctrlat(self.a, self.b, self._put(x, y))


def _avg(v):                                    # avgval_double, mosaic_util.c:194
    s = 0.0
    for t in v:
        s += t
    return s / len(v)


class _Grid:
    def __init__(self, g):
        self.nx, self.ny = g.nx, g.ny
        self.x = np.ascontiguousarray(g.lonc, dtype=np.float64).reshape(g.ny + 1, g.nx + 1)
        self.y = np.ascontiguousarray(g.latc, dtype=np.float64).reshape(g.ny + 1, g.nx + 1)
        self.area = orc.ref_get_grid_area(g.nx, g.ny, self.x, self.y).reshape(-1)          # get_grid_global_area, :254-285
        y = self.y
        self.ymin = np.minimum(np.minimum(y[:-1, :-1], y[:-1, 1:]), np.minimum(y[1:, 1:], y[1:, :-1]))
        self.ymax = np.maximum(np.maximum(y[:-1, :-1], y[:-1, 1:]), np.maximum(y[1:, 1:], y[1:, :-1]))
        self.xl, self.yl = self.x.tolist(), self.y.tolist()

    def cell(self, i, j):                       # n0, n1, n2, n3 of :1378-1385
        x, y = self.xl, self.yl
        return [x[j][i], x[j][i + 1], x[j + 1][i + 1], x[j + 1][i]], [y[j][i], y[j][i + 1], y[j + 1][i + 1], y[j + 1][i]]

    def band(self, lo, hi, both):
        """:1294-1306 (both = False) and :2583-2592 (both = True): the rows js .. je of this grid a tile with latitudes lo .. hi meets"""
        js, je = self.ny, -1
        for j in range(self.ny + 1):
            row = self.y[j]
            if both:
                if np.any((row > lo) & (row < hi)):
                    je = max(je, j); js = min(js, j)
            else:
                if np.any(row > lo):
                    js = min(js, j)
                if np.any(row < hi):
                    je = max(je, j)
        return max(0, js - 1), min(self.ny - 1, je + 1)


def _new_list(names):
    return {k: [] for k in names + ("area", "clon", "clat")}


def reference_coupler(atm, lnd, ocn, omask, order, thresh=1.0e-6, ocn_south_ext=0, reverse_sums=False, skip_same_copy=False):
    """atm: list of grids (nx, ny, lonc, latc in radians); lnd: None (lnd_same_as_atm) or a list; ocn: one grid; omask [nyo, nxo].
    reverse_sums / skip_same_copy: deliberately wrong variants for the tests of this restatement's teeth (every cell's terms added
    in reversed order; the atmosphere x land cells of lnd_same_as_atm clipped like any other pair).  Returns a dict."""
    P = Prim(orc.ref())
    same = lnd is None
    A = [_Grid(g) for g in atm]
    L = A if same else [_Grid(g) for g in lnd]
    O = _Grid(ocn)
    om = np.ascontiguousarray(omask, dtype=np.float64).reshape(-1)
    oml = om.tolist()
    nta, ntl = len(A), len(L)
    axl = [[_new_list(("ia", "ja", "il", "jl")) for _ in range(ntl)] for _ in range(nta)]
    axo = [_new_list(("ia", "ja", "io", "jo")) for _ in range(nta)]
    cover = dict(dropped=0, poly5=0, atm_without_axl=0, ncand=0)
    copy_same = same and not skip_same_copy

    for na, ga in enumerate(A):                                                     # :1202
        ya_lo, ya_hi = float(ga.y.min()), float(ga.y.max())                         # :1269-1292 (one process: the whole tile)
        lbands = [g.band(ya_lo, ya_hi, False) for g in L]                           # :1294-1316
        js_o, je_o = O.band(ya_lo, ya_hi, False)                                    # :1318-1341
        area_atm = ga.area
        for la in range(ga.nx * ga.ny):                                             # :1346
            ia, ja = la % ga.nx, la // ga.nx
            xa, ya = ga.cell(ia, ja)
            ya_min, ya_max = min(ya), max(ya)                                       # :1386-1387
            xa, ya = P.fix_lon(xa, ya, math.pi)                                     # :1389
            na_in = len(xa)
            xa_min, xa_max, xa_avg = min(xa), max(xa), _avg(xa)
            found = []                                                              # count = 0, :1395
            for nl, gl in enumerate(L):                                             # :1396
                if same and nl != na:                                               # :1311-1314: is_lnd > ie_lnd, an empty loop
                    continue
                js, je = lbands[nl]
                hit = ~((gl.ymin[js:je + 1] >= ya_max) | (gl.ymax[js:je + 1] <= ya_min))          # :1452-1454, in (jl, il) order
                for jl, il in zip(*np.nonzero(hit)):
                    jl, il = int(jl) + js, int(il)
                    xl, yl = gl.cell(il, jl)
                    xl, yl = P.fix_lon(xl, yl, xa_avg)                              # :1455
                    nl_in = len(xl)
                    if xa_min >= max(xl) or xa_max <= min(xl):                      # :1462
                        continue
                    if copy_same:                                                   # :1463-1477
                        if na == nl and ja == jl and ia == il:
                            if na_in != nl_in:
                                raise RuntimeError("make_coupler_mosaic: inconsistent number of grid box coreners")
                            x_out, y_out = list(xl), list(yl)
                        else:
                            x_out, y_out = [], []
                    else:
                        x_out, y_out = P.clip(xa, ya, xl, yl)                       # :1479
                    if len(x_out) > 0:                                              # :1483
                        xarea = P.area(x_out, y_out)
                        min_area = min(gl.area[jl * gl.nx + il], area_atm[la])      # :1488
                        if xarea / min_area > thresh:                               # :1507
                            found.append(dict(il=il, jl=jl, nl=nl, x=x_out, y=y_out, area=0.0, clon=0.0, clat=0.0, xmin=min(x_out),
                                              xmax=max(x_out), ymin=min(y_out), ymax=max(y_out)))
                            if len(x_out) >= 5:
                                cover["poly5"] += 1
            cover["ncand"] += len(found)
            for jo in range(js_o, je_o + 1):                                        # :1555
                for io in range(O.nx):
                    ocn_frac = oml[jo * O.nx + io]                                  # :1601
                    lnd_frac = 1 - ocn_frac
                    over_sea, over_land = ocn_frac > MIN_AREA_FRAC, lnd_frac > MIN_AREA_FRAC
                    yo_min, yo_max = O.ymin[jo, io], O.ymax[jo, io]
                    if over_sea and (yo_min >= ya_max or yo_max <= ya_min):         # :1614 (the latitude half, before the work of :1597)
                        continue
                    if not over_sea and not (over_land and found):
                        continue                                                    # (neither branch has anything to do with xo)
                    xo, yo = O.cell(io, jo)
                    xo, yo = P.fix_lon(xo, yo, xa_avg)                              # :1597
                    xo_min, xo_max = min(xo), max(xo)
                    if over_sea:                                                    # :1604
                        if xa_min >= xo_max or xa_max <= xo_min:                    # :1614: leaves the ocean cell, the land branch too
                            continue
                        x_out, y_out = P.clip(xa, ya, xo, yo)                       # :1615
                        if len(x_out) > 0:
                            xarea = P.area(x_out, y_out) * ocn_frac                 # :1640
                            min_area = min(O.area[jo * O.nx + io], area_atm[la])    # :1643
                            if xarea / min_area > thresh:                           # :1646
                                t = axo[na]
                                t["area"].append(xarea); t["io"].append(io); t["jo"].append(jo); t["ia"].append(ia); t["ja"].append(ja)
                                t["clon"].append(P.ctrlon(x_out, y_out, xa_avg) * ocn_frac if order == 2 else 0.0)      # :1654
                                t["clat"].append(P.ctrlat(x_out, y_out) * ocn_frac if order == 2 else 0.0)
                    if over_land:                                                   # :1662
                        for f in found:                                             # :1664
                            if f["xmin"] >= xo_max or f["xmax"] <= xo_min or f["ymin"] >= ya_max or f["ymax"] <= ya_min:      # :1669
                                continue
                            x_out, y_out = P.clip(f["x"], f["y"], xo, yo)           # :1670
                            if len(x_out) > 0:
                                xarea = P.area(x_out, y_out) * lnd_frac             # :1676
                                gl = L[f["nl"]]
                                min_area = min(gl.area[f["jl"] * gl.nx + f["il"]], area_atm[la])        # :1677
                                if xarea / min_area > thresh:                       # :1678
                                    f["area"] += xarea                              # :1689
                                    if order == 2:
                                        f["clon"] += P.ctrlon(x_out, y_out, xa_avg) * lnd_frac          # :1691
                                        f["clat"] += P.ctrlat(x_out, y_out) * lnd_frac
            kept = 0
            for f in found:                                                         # :1701
                gl = L[f["nl"]]
                min_area = min(gl.area[f["jl"] * gl.nx + f["il"]], area_atm[la])    # :1703
                if f["area"] / min_area > thresh:                                   # :1706
                    t = axl[na][f["nl"]]
                    t["area"].append(f["area"]); t["ia"].append(ia); t["ja"].append(ja); t["il"].append(f["il"]); t["jl"].append(f["jl"])
                    t["clon"].append(f["clon"]); t["clat"].append(f["clat"])
                    kept += 1
                else:
                    cover["dropped"] += 1
            if not kept:
                cover["atm_without_axl"] += 1

    # ---- land x ocean (:2470-2690)
    lxo = []
    if not same:
        for nl, gl in enumerate(L):                                                 # :2524
            t = _new_list(("il", "jl", "io", "jo"))
            js_o, je_o = O.band(float(gl.y.min()), float(gl.y.max()), True)         # :2558-2595
            for ll in range(gl.nx * gl.ny):                                         # :2598
                il, jl = ll % gl.nx, ll // gl.nx
                xl, yl = gl.cell(il, jl)
                yl_min, yl_max = min(yl), max(yl)
                xl, yl = P.fix_lon(xl, yl, math.pi)                                 # :2622
                xl_min, xl_max, xl_avg = min(xl), max(xl), _avg(xl)
                sl = slice(js_o, je_o + 1)
                hit = (om.reshape(O.ny, O.nx)[sl] > MIN_AREA_FRAC) & ~((O.ymin[sl] >= yl_max) | (O.ymax[sl] <= yl_min))      # :2628, :2651
                for jo, io in zip(*np.nonzero(hit)):
                    jo, io = int(jo) + js_o, int(io)
                    xo, yo = O.cell(io, jo)
                    xo, yo = P.fix_lon(xo, yo, xl_avg)                              # :2652
                    if xl_min >= max(xo) or xl_max <= min(xo):                      # :2658
                        continue
                    ocn_frac = oml[jo * O.nx + io]                                  # :2660
                    x_out, y_out = P.clip(xl, yl, xo, yo)                           # :2666
                    if len(x_out) > 0:
                        xarea = P.area(x_out, y_out) * ocn_frac                     # :2672
                        min_area = min(O.area[jo * O.nx + io], gl.area[ll])         # :2673
                        if xarea / min_area > thresh:                               # :2674
                            t["area"].append(xarea); t["io"].append(io); t["jo"].append(jo); t["il"].append(il); t["jl"].append(jl)
                            t["clon"].append(P.ctrlon(x_out, y_out, xl_avg) * ocn_frac if order == 2 else 0.0)          # :2681
                            t["clat"].append(P.ctrlat(x_out, y_out) * ocn_frac if order == 2 else 0.0)
            lxo.append(t)

    def arrays(t):
        return {k: np.array(v, dtype=np.float64 if k in ("area", "clon", "clat") else np.int64) for k, v in t.items()}

    axl = [[arrays(t) for t in row] for row in axl]
    axo = [arrays(t) for t in axo]
    lxo = [arrays(t) for t in lxo]
    seq = (lambda n: range(n - 1, -1, -1)) if reverse_sums else range

    def add(dst, idx, t):                                                           # the loops of :1781-1784, :1881-1890, :1926-1935, :2749-2758
        for i in seq(len(idx)):
            ii = idx[i]
            dst[0][ii] += t["area"][i]
            if order == 2:
                dst[1][ii] += t["clon"][i]
                dst[2][ii] += t["clat"][i]

    def centroid(s):                                                                # :1946-1951 and its siblings
        pos = s[0] > 0
        s[1][pos] /= s[0][pos]
        s[2][pos] /= s[0][pos]

    # ---- per-cell sums, centroid distances (:1744-2016)
    l_sum = [[np.zeros(g.nx * g.ny) for _ in range(3)] for g in L]
    o_sum = [np.zeros(O.nx * O.ny) for _ in range(3)]
    a_sums = []
    for na, ga in enumerate(A):                                                     # :1763 / :1845
        a_sum = [np.zeros(ga.nx * ga.ny) for _ in range(3)]
        for nl, gl in enumerate(L):
            t = axl[na][nl]
            if order == 2:
                # :1881-1890 adds one exchange cell to the atmosphere cell and to the land cell in one loop; the two targets are
                # independent, so two loops in the same order give the same bits
                add(a_sum, t["ja"] * ga.nx + t["ia"], t)
            add(l_sum[nl], t["jl"] * gl.nx + t["il"], t)
        t = axo[na]
        if order == 2:
            add(a_sum, t["ja"] * ga.nx + t["ia"], t)
        add(o_sum, t["jo"] * O.nx + t["io"], t)
        if order == 2:
            centroid(a_sum)                                                         # :1946-1951
            for nl in range(ntl):                                                   # :1954-1960
                t = axl[na][nl]
                la = t["ja"] * ga.nx + t["ia"]
                t["di1"] = t["clon"] / t["area"] - a_sum[1][la]
                t["dj1"] = t["clat"] / t["area"] - a_sum[2][la]
            t = axo[na]                                                             # :1961-1967
            la = t["ja"] * ga.nx + t["ia"]
            t["di1"] = t["clon"] / t["area"] - a_sum[1][la]
            t["dj1"] = t["clat"] / t["area"] - a_sum[2][la]
        a_sums.append(a_sum)
    if order == 2:
        for nl, gl in enumerate(L):                                                 # :1976-1989
            centroid(l_sum[nl])
            for na in range(nta):
                t = axl[na][nl]
                ll = t["jl"] * gl.nx + t["il"]
                t["di2"] = t["clon"] / t["area"] - l_sum[nl][1][ll]
                t["dj2"] = t["clat"] / t["area"] - l_sum[nl][2][ll]
        centroid(o_sum)                                                             # :1996-2001
        for na in range(nta):                                                       # :2002-2008
            t = axo[na]
            lo = t["jo"] * O.nx + t["io"]
            t["di2"] = t["clon"] / t["area"] - o_sum[1][lo]
            t["dj2"] = t["clat"] / t["area"] - o_sum[2][lo]
        if not same:                                                                # :2699-2811
            o2 = [np.zeros(O.nx * O.ny) for _ in range(3)]
            for nl, gl in enumerate(L):
                l2 = [np.zeros(gl.nx * gl.ny) for _ in range(3)]
                t = lxo[nl]
                add(l2, t["jl"] * gl.nx + t["il"], t)
                add(o2, t["jo"] * O.nx + t["io"], t)
                centroid(l2)                                                        # :2768-2773
                ll = t["jl"] * gl.nx + t["il"]
                t["di1"] = t["clon"] / t["area"] - l2[1][ll]                        # :2778
                t["dj1"] = t["clat"] / t["area"] - l2[2][ll]
            centroid(o2)                                                            # :2790-2795
            for nl in range(ntl):
                t = lxo[nl]
                lo = t["jo"] * O.nx + t["io"]
                t["di2"] = t["clon"] / t["area"] - o2[1][lo]                        # :2799
                t["dj2"] = t["clat"] / t["area"] - o2[2][lo]

    # ---- masks (:2018-2121)
    e = ocn_south_ext
    ocn_frac = o_sum[0] / O.area                                                    # :2037
    nbad = int(np.count_nonzero(np.abs(om - ocn_frac)[e * O.nx:] > TOLORENCE))      # :2038
    ocean = dict(mask=ocn_frac.reshape(O.ny, O.nx)[e:], areaO=O.area.reshape(O.ny, O.nx)[e:], areaX=o_sum[0].reshape(O.ny, O.nx)[e:],
                 o_area=o_sum[0], o_clon=o_sum[1], o_clat=o_sum[2], area=O.area)
    land = [dict(mask=(l_sum[nl][0] / gl.area).reshape(gl.ny, gl.nx), l_area=l_sum[nl][0].reshape(gl.ny, gl.nx), area_lnd=gl.area.reshape(gl.ny, gl.nx),
                 l_clon=l_sum[nl][1], l_clat=l_sum[nl][2]) for nl, gl in enumerate(L)]                                  # :2087-2094
    atmos = [dict(a_area=a_sums[na][0], a_clon=a_sums[na][1], a_clat=a_sums[na][2], area=ga.area) for na, ga in enumerate(A)]
    return dict(axl=axl, axo=axo, lxo=lxo, ocean=ocean, land=land, atmos=atmos, nbad=nbad, cover=cover, order=order, same=same)


# ------------------------------------------------------------------------------------------------------------------- the cases
def ocean_mask(nx, ny):
    """land blocks, sea, cells at 0.35 and cells at 0.99995 (a land fraction below MIN_AREA_FRAC), as tests/test_gpu_coupler.py"""
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    m = np.where((ii // 5 + jj // 4) % 3 == 0, 0.0, 1.0)
    m[(ii + 2 * jj) % 11 == 0] = 0.35
    m[(2 * ii + jj) % 13 == 0] = 0.99995
    return m


def cubed_sphere(fg, ni):
    lon, lat = fg.gnomonic_ed_corners(ni)
    return [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]


def case_a(fg):
    """land on the atmosphere grid: C8, tripolar 40 x 24 ocean from -82 degrees extended to 40 x 25"""
    to, ta = fg.tripolar_corners(40, 24)
    g = fg.coupler_ocean_grid(np.degrees(to), np.degrees(ta), ocean_mask(40, 24))
    assert g["ocn_south_ext"] == 1 and g["ny"] == 25
    return dict(atm=cubed_sphere(fg, 8), lnd=None, ocn=fg.GridConfig(40, 25, g["x"], g["y"]), omask=g["omask"], ext=1)


def case_b(fg):
    """land of its own: C8, 30 x 16 lat-lon land, 36 x 20 lat-lon ocean from -90 degrees (no extension)"""
    lo, la = fg.latlon_corners(30, 16)
    oo, oa = fg.latlon_corners(36, 20)
    g = fg.coupler_ocean_grid(np.degrees(oo), np.degrees(oa), ocean_mask(36, 20))
    assert g["ocn_south_ext"] == 0
    return dict(atm=cubed_sphere(fg, 8), lnd=[fg.GridConfig(30, 16, lo, la)], ocn=fg.GridConfig(36, 20, g["x"], g["y"]), omask=g["omask"], ext=0)


def case_c(fg, value):
    """C4 atmosphere = land over a 12 x 8 lat-lon ocean with omask == value everywhere"""
    oo, oa = fg.latlon_corners(12, 8)
    return dict(atm=cubed_sphere(fg, 4), lnd=None, ocn=fg.GridConfig(12, 8, oo, oa), omask=np.full((8, 12), float(value)), ext=0)


_CACHE = {}


def reference_of(name, fg, order=2, **kw):
    """the restatement's result for a case, computed once per session"""
    key = (name, order, tuple(sorted(kw.items())))
    if key not in _CACHE:
        c = {"a": case_a, "b": case_b, "c0": lambda f: case_c(f, 0.0), "c1": lambda f: case_c(f, 1.0)}[name](fg)
        _CACHE[key] = (c, reference_coupler(c["atm"], c["lnd"], c["ocn"], c["omask"], order, ocn_south_ext=c["ext"], **kw))
    return _CACHE[key]
