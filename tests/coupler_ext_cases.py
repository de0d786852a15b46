"""make_coupler_mosaic.c's nested atmosphere tile, wave grid and --check restated over the reference's own compiled primitives
(coupler_cases.Prim: fix_lon, clip_2dx2d, poly_area, poly_ctrlon, poly_ctrlat, get_grid_area from oracle/_ref), and the cases
the tests of fg_coupler_set_nest / fg_coupler_add_wave / fg_coupler_check share.  Line numbers are the reference's.

* coupler_sums: :1743-2011 and the masks of :2018-2121 with the `na != tile_nest` guards of :1765, :1792, :1857, :1903.  The three
  lists do not know of a nest (tile_nest appears nowhere in :1198-1740): they are coupler_cases.reference_coupler's for the
  seven-tile atmosphere, and with tile_nest = -1 coupler_sums gives that function's own sums bit for bit (tests/test_coupler_ext_cpu.py).
  At order 2 the guards of :1857 and :1903 enclose the WHOLE loop body, the `a_area / a_clon / a_clat +=` of :1882-1885 and
  :1927-1930 included: the nest tile's a_area stays 0, :1946-1951 divide nothing, and the nest lists' tile-1 distances (:1954-1967)
  are clon / area - 0.  That is kept as written.  atm_xarea (:2210, :2333) is a different array and has no guard: --check sees the
  nest tile's full sums.
* reference_wave: :3044-3424 (legacy clip, one process, one ocean tile).
* reference_check: :2199-2219, :2326-2342, :3504, :3591-3661.

Two places where the reference is not followed, because it cannot be: the order-1 wave sum (:3262-3267) gathers io / jo into
g_iw / g_jw and adds into w_area2, which is never allocated -- the statement cannot execute; at order 1 w_area is formed as the
order-2 branch forms it (:3325-3326) and nothing else.  And GREAT_CIRCLE_CLIP is first order only, so a wave grid under it has no
sums to pin: the library refuses it.

sums_gc is coupler_sums for tests/coupler_gc_cases.py's great-circle restatement (order 1: areas only)."""
import math

import numpy as np

import orc
from coupler_cases import MIN_AREA_FRAC, TOLORENCE, Prim, _Grid, _avg, _new_list, case_b, reference_coupler, reference_of

LIST_KEYS = {"axl": ("ia", "ja", "il", "jl"), "axo": ("ia", "ja", "io", "jo"), "lxo": ("il", "jl", "io", "jo"), "wxo": ("iw", "jw", "io", "jo")}


def _seq(reverse):
    return (lambda n: range(n - 1, -1, -1)) if reverse else range


def _strip(t):
    """a list without the distances a previous pass left in it"""
    return {k: np.array(v) for k, v in t.items() if k not in ("di1", "dj1", "di2", "dj2")}


def coupler_sums(atm, lnd, ocn, omask, area_atm, area_lnd, area_ocn, axl, axo, order, tile_nest=-1, ocn_south_ext=0, reverse_sums=False,
                 no_exclusion=False):
    """atm / lnd: lists of (nx, ny) grids; ocn: one; area_*: get_grid_area per tile (flat); axl [na][nl], axo [na]: the lists.
    no_exclusion: the deliberately wrong variant that adds the nest tile's terms like any tile's.  atmos[na]["a_area"] is the
    reference's temporary of :1848 (0 on the nest tile); what a caller sees as the cell's exchange area is reference_check's atm_xarea."""
    nta, ntl = len(atm), len(lnd)
    axl = [[_strip(t) for t in row] for row in axl]
    axo = [_strip(t) for t in axo]
    seq = _seq(reverse_sums)

    def add(dst, idx, t):
        for i in seq(len(idx)):
            ii = idx[i]
            dst[0][ii] += t["area"][i]
            if order == 2:
                dst[1][ii] += t["clon"][i]
                dst[2][ii] += t["clat"][i]

    def centroid(s):
        pos = s[0] > 0
        s[1][pos] /= s[0][pos]
        s[2][pos] /= s[0][pos]

    l_sum = [[np.zeros(g.nx * g.ny) for _ in range(3)] for g in lnd]
    o_sum = [np.zeros(ocn.nx * ocn.ny) for _ in range(3)]
    a_sums = []
    for na, ga in enumerate(atm):                                                   # :1763 / :1845
        a_sum = [np.zeros(ga.nx * ga.ny) for _ in range(3)]
        nest = na == tile_nest and not no_exclusion
        if not nest:                                                                # :1765 / :1857
            for nl, gl in enumerate(lnd):
                t = axl[na][nl]
                if order == 2:
                    add(a_sum, t["ja"] * ga.nx + t["ia"], t)                        # :1882-1885
                add(l_sum[nl], t["jl"] * gl.nx + t["il"], t)                        # :1783, :1886-1889
        if not nest:                                                                # :1792 / :1903
            t = axo[na]
            if order == 2:
                add(a_sum, t["ja"] * ga.nx + t["ia"], t)                            # :1927-1930
            add(o_sum, t["jo"] * ocn.nx + t["io"], t)                               # :1809, :1931-1934
        if order == 2:
            centroid(a_sum)                                                         # :1946-1951
            for t in axl[na] + [axo[na]]:                                           # :1954-1967
                la = t["ja"] * ga.nx + t["ia"]
                t["di1"] = t["clon"] / t["area"] - a_sum[1][la]
                t["dj1"] = t["clat"] / t["area"] - a_sum[2][la]
        a_sums.append(a_sum)
    if order == 2:
        for nl, gl in enumerate(lnd):                                               # :1976-1989
            centroid(l_sum[nl])
            for na in range(nta):
                t = axl[na][nl]
                ll = t["jl"] * gl.nx + t["il"]
                t["di2"] = t["clon"] / t["area"] - l_sum[nl][1][ll]
                t["dj2"] = t["clat"] / t["area"] - l_sum[nl][2][ll]
        centroid(o_sum)                                                             # :1996-2001
        for na in range(nta):                                                       # :2002-2008
            t = axo[na]
            lo = t["jo"] * ocn.nx + t["io"]
            t["di2"] = t["clon"] / t["area"] - o_sum[1][lo]
            t["dj2"] = t["clat"] / t["area"] - o_sum[2][lo]
    e = ocn_south_ext
    om = np.ascontiguousarray(omask, dtype=np.float64).reshape(-1)
    ocn_frac = o_sum[0] / area_ocn                                                  # :2037
    nbad = int(np.count_nonzero(np.abs(om - ocn_frac)[e * ocn.nx:] > TOLORENCE))    # :2038
    ocean = dict(mask=ocn_frac.reshape(ocn.ny, ocn.nx)[e:], o_area=o_sum[0], o_clon=o_sum[1], o_clat=o_sum[2], area=area_ocn)
    land = [dict(mask=(l_sum[nl][0] / area_lnd[nl]).reshape(gl.ny, gl.nx), l_area=l_sum[nl][0].reshape(gl.ny, gl.nx),
                 area_lnd=np.asarray(area_lnd[nl]).reshape(gl.ny, gl.nx), l_clon=l_sum[nl][1], l_clat=l_sum[nl][2]) for nl, gl in enumerate(lnd)]
    atmos = [dict(a_area=a_sums[na][0], a_clon=a_sums[na][1], a_clat=a_sums[na][2], area=area_atm[na]) for na in range(nta)]
    return dict(axl=axl, axo=axo, ocean=ocean, land=land, atmos=atmos, nbad=nbad, order=order)


def with_nest(c, r, tile_nest, **kw):
    """c: a case; r: reference_coupler's result for it (its lists are kept, its sums formed anew with the exclusions)"""
    lnd = c["atm"] if c["lnd"] is None else c["lnd"]
    out = coupler_sums(c["atm"], lnd, c["ocn"], c["omask"], [t["area"] for t in r["atmos"]], [t["area_lnd"].reshape(-1) for t in r["land"]],
                       r["ocean"]["area"], r["axl"], r["axo"], r["order"], tile_nest=tile_nest, ocn_south_ext=c["ext"], **kw)
    out["lxo"] = r["lxo"]                                                           # :2466-2811 never looks at the atmosphere
    return out


def sums_gc(atm, lnd, ocn, omask, area_atm, area_lnd, area_ocn, axl, axo, tile_nest=-1, ocn_south_ext=0):
    """:1762-1818 (interp_order 1) and the masks for coupler_gc_cases' lists: areas only; a_area as the device keeps it"""
    l_sum = [np.zeros(g.nx * g.ny) for g in lnd]
    o_sum = np.zeros(ocn.nx * ocn.ny)
    a_sums = []
    for na, ga in enumerate(atm):
        a_sum = np.zeros(ga.nx * ga.ny)
        for nl, gl in enumerate(lnd):
            t = axl[na][nl]
            for i in range(t["area"].size):
                a_sum[t["ja"][i] * ga.nx + t["ia"][i]] += t["area"][i]
                if na != tile_nest:                                                 # :1765
                    l_sum[nl][t["jl"][i] * gl.nx + t["il"][i]] += t["area"][i]
        t = axo[na]
        for i in range(t["area"].size):
            a_sum[t["ja"][i] * ga.nx + t["ia"][i]] += t["area"][i]
            if na != tile_nest:                                                     # :1792
                o_sum[t["jo"][i] * ocn.nx + t["io"][i]] += t["area"][i]
        a_sums.append(a_sum)
    om = np.ascontiguousarray(omask, dtype=np.float64).reshape(-1)
    ocn_frac = o_sum / area_ocn
    nbad = int(np.count_nonzero(np.abs(om - ocn_frac)[ocn_south_ext * ocn.nx:] > TOLORENCE))
    return dict(a_area=a_sums, l_area=l_sum, o_area=o_sum, land_mask=[l_sum[nl] / area_lnd[nl] for nl in range(len(lnd))], ocean_mask=ocn_frac, nbad=nbad)


# ------------------------------------------------------------------------------------------------------------------- the wave grid
def reference_wave(wav, ocn, omask, order, thresh=1.0e-6, skip_band=False, reverse_sums=False):
    """:3044-3424.  wav: list of grids (nx, ny, lonc, latc in radians); ocn: the ocean grid the tool works on; omask [nyo, nxo].
    skip_band / reverse_sums: deliberately wrong variants (every ocean row looked at; every cell's terms added in reversed order)."""
    P = Prim(orc.ref())
    W = [_Grid(g) for g in wav]
    O = _Grid(ocn)
    om = np.ascontiguousarray(omask, dtype=np.float64).reshape(O.ny, O.nx)
    oml = om.reshape(-1).tolist()
    wxo, bands = [], []
    for gw in W:                                                                    # :3044
        t = _new_list(LIST_KEYS["wxo"])
        yw_lo, yw_hi = float(gw.y.min()), float(gw.y.max())                         # :3071-3104 (one process: every cell of the tile)
        js, je = (0, O.ny - 1) if skip_band else O.band(yw_lo, yw_hi, True)         # :3107-3117 (the loop of :2583-2592, verbatim)
        bands.append((js, je))
        for lw in range(gw.nx * gw.ny):                                             # :3129
            iw, jw = lw % gw.nx, lw // gw.nx
            xw, yw = gw.cell(iw, jw)
            yw_min, yw_max = min(yw), max(yw)                                       # :3152-3153
            xw, yw = P.fix_lon(xw, yw, math.pi)                                     # :3154
            xw_min, xw_max, xw_avg = min(xw), max(xw), _avg(xw)
            sl = slice(js, je + 1)                                                  # :3162 (js > je: no row)
            # the tests of :3190 and the latitude half of :3199 need nothing of :3185: taken first, in (jo, io) order
            hit = (om[sl] > MIN_AREA_FRAC) & ~((O.ymax[sl] <= yw_min) | (O.ymin[sl] >= yw_max))
            for jo, io in zip(*np.nonzero(hit)):
                jo, io = int(jo) + js, int(io)
                xo, yo = O.cell(io, jo)
                xo, yo = P.fix_lon(xo, yo, xw_avg)                                  # :3185
                if xw_min >= max(xo) or xw_max <= min(xo):                          # :3199
                    continue
                ocn_frac = oml[jo * O.nx + io]                                      # :3189
                x_out, y_out = P.clip(xw, yw, xo, yo)                               # :3200
                if len(x_out) > 0:
                    xarea = P.area(x_out, y_out) * ocn_frac                         # :3203
                    min_area = min(O.area[jo * O.nx + io], gw.area[lw])             # :3204
                    if xarea / min_area > thresh:                                   # :3205
                        t["area"].append(xarea); t["io"].append(io); t["jo"].append(jo); t["iw"].append(iw); t["jw"].append(jw)
                        t["clon"].append(P.ctrlon(x_out, y_out, xw_avg) * ocn_frac if order == 2 else 0.0)      # :3213
                        t["clat"].append(P.ctrlat(x_out, y_out) * ocn_frac if order == 2 else 0.0)
        wxo.append({k: np.array(v, dtype=np.float64 if k in ("area", "clon", "clat") else np.int64) for k, v in t.items()})
    seq = _seq(reverse_sums)
    w_area = [np.zeros(g.nx * g.ny) for g in W]                                     # :3240-3246
    out = dict(wxo=wxo, bands=bands, order=order, area_wav=[g.area for g in W])
    if order == 2:                                                                  # :3276-3386
        o_sum = [np.zeros(O.nx * O.ny) for _ in range(3)]
        w_cen = []
        for nw, gw in enumerate(W):
            t = wxo[nw]
            w_clon, w_clat = np.zeros(gw.nx * gw.ny), np.zeros(gw.nx * gw.ny)
            for i in seq(t["area"].size):                                           # :3324-3333
                ii = t["jw"][i] * gw.nx + t["iw"][i]
                w_area[nw][ii] += t["area"][i]; w_clon[ii] += t["clon"][i]; w_clat[ii] += t["clat"][i]
                ii = t["jo"][i] * O.nx + t["io"][i]
                o_sum[0][ii] += t["area"][i]; o_sum[1][ii] += t["clon"][i]; o_sum[2][ii] += t["clat"][i]
            pos = w_area[nw] > 0                                                    # :3344-3349
            w_clon[pos] /= w_area[nw][pos]; w_clat[pos] /= w_area[nw][pos]
            lw = t["jw"] * gw.nx + t["iw"]                                          # :3351-3357
            t["di1"] = t["clon"] / t["area"] - w_clon[lw]
            t["dj1"] = t["clat"] / t["area"] - w_clat[lw]
            w_cen.append((w_clon, w_clat))
        pos = o_sum[0] > 0                                                          # :3366-3371
        o_sum[1][pos] /= o_sum[0][pos]; o_sum[2][pos] /= o_sum[0][pos]
        for t in wxo:                                                               # :3372-3378
            lo = t["jo"] * O.nx + t["io"]
            t["di2"] = t["clon"] / t["area"] - o_sum[1][lo]
            t["dj2"] = t["clat"] / t["area"] - o_sum[2][lo]
        out.update(o_area=o_sum[0], o_clon=o_sum[1], o_clat=o_sum[2], w_clon=[w[0] for w in w_cen], w_clat=[w[1] for w in w_cen])
    else:                                                                           # :3248-3275 cannot execute: w_area as :3325-3326, nothing else
        for nw, gw in enumerate(W):
            t = wxo[nw]
            for i in seq(t["area"].size):
                w_area[nw][t["jw"][i] * gw.nx + t["iw"][i]] += t["area"][i]
    out["w_area"] = w_area
    out["mask"] = [(w_area[nw] / gw.area).reshape(gw.ny, gw.nx) for nw, gw in enumerate(W)]       # :3397-3402
    return out


# ------------------------------------------------------------------------------------------------------------------------- --check
def _serial(values, s=0.0):
    for v in np.asarray(values, dtype=np.float64).tolist():
        s += v
    return s


def reference_check(atm, area_atm, axl, axo, tile_nest=-1, wxo=None):
    """:2199-2219, :2326-2342, :3504, :3591-3661.  atm: the tiles (nx, ny); area_atm [na] flat; axl [na][nl], axo [na]; wxo: None or [nw]"""
    s = dict(axl=0.0, axo=0.0, axl_nest=0.0, axo_nest=0.0)
    xareas = []
    for na, ga in enumerate(atm):
        xa = np.zeros(ga.nx * ga.ny)                                                # :575-576
        for t in axl[na]:                                                           # :2199-2219
            for ia, ja, a in zip(t["ia"].tolist(), t["ja"].tolist(), t["area"].tolist()):
                xa[ja * ga.nx + ia] += a                                            # :2210
            k = "axl_nest" if na == tile_nest else "axl"                            # :2215-2218
            s[k] = _serial(t["area"], s[k])
        xareas.append(xa)
    for na, ga in enumerate(atm):                                                   # :2326-2342: after every land list
        t = axo[na]
        for ia, ja, a in zip(t["ia"].tolist(), t["ja"].tolist(), t["area"].tolist()):
            xareas[na][ja * ga.nx + ia] += a                                        # :2333
        k = "axo_nest" if na == tile_nest else "axo"                                # :2338-2341
        s[k] = _serial(t["area"], s[k])
    max_ratio, max_ta, max_ia, max_ja = -1.0, -1, -1, -1                            # :3607-3610
    for n, ga in enumerate(atm):                                                    # :3612-3626
        ratio = np.abs(xareas[n] - area_atm[n]) / area_atm[n]
        assert not np.isnan(ratio).any()
        i = int(np.argmax(ratio))                                                   # the first cell with the tile's largest ratio
        if ratio[i] > max_ratio:                                                    # :3619: strictly larger than every earlier tile's
            max_ratio, max_ta, max_ja, max_ia = float(ratio[i]), n, i // ga.nx, i % ga.nx
    out = dict(max_ratio=max_ratio, max_tile=max_ta, max_i=max_ia, max_j=max_ja, atm_xarea=xareas)
    atm_sum = atm_nest = 0.0
    for n in range(len(atm)):                                                       # :3636-3641
        if n == tile_nest:
            atm_nest = _serial(area_atm[n], atm_nest)
        else:
            atm_sum = _serial(area_atm[n], atm_sum)
    out.update(atm_area_sum=atm_sum, axl_area_sum=s["axl"], axo_area_sum=s["axo"], axo_area_frac=s["axo"] / atm_sum * 100,
               axl_area_frac=s["axl"] / atm_sum * 100, tiling_area=(atm_sum - s["axo"] - s["axl"]) / atm_sum * 100)        # :3642-3644
    if tile_nest >= 0:                                                              # :3652-3655
        out.update(atm_area_sum_nest=atm_nest, axl_area_sum_nest=s["axl_nest"], axo_area_sum_nest=s["axo_nest"],
                   axo_area_frac_nest=s["axo_nest"] / atm_nest * 100, axl_area_frac_nest=s["axl_nest"] / atm_nest * 100,
                   tiling_area_nest=(atm_nest - s["axo_nest"] - s["axl_nest"]) / atm_nest * 100)
    if wxo is not None:
        w = 0.0
        for t in wxo:                                                               # :3504
            w = _serial(t["area"], w)
        out["wxo_area_sum"] = w
    return out


# ------------------------------------------------------------------------------------------------------------------- the cases
def nest_corners(lon, lat, i0, j0, nb=3):
    """the block of nb x nb parent cells from (i0, j0) halved: [2 nb + 1, 2 nb + 1] corners; the parent's corners bit for bit, the
    new ones midway in lon / lat (an edge's midpoint; a cell's centre midway between the midpoints of its west and east edges)"""
    out = []
    for p in (lon, lat):
        b = np.ascontiguousarray(p, dtype=np.float64)[j0:j0 + nb + 1, i0:i0 + nb + 1]
        f = np.empty((2 * nb + 1, 2 * nb + 1))
        f[::2, ::2] = b
        f[::2, 1::2] = 0.5 * (b[:, :-1] + b[:, 1:])
        f[1::2, ::2] = 0.5 * (b[:-1] + b[1:])
        f[1::2, 1::2] = 0.5 * (f[1::2, 0:-1:2] + f[1::2, 2::2])
        out.append(f)
    return out


NEST_PARENT, NEST_I0, NEST_J0 = 1, 2, 3                    # an equatorial tile of the cubed sphere; its block is away from the date line


def nest_tile(fg, parent):
    lon = np.asarray(parent.lonc, dtype=np.float64).reshape(parent.ny + 1, parent.nx + 1)
    lat = np.asarray(parent.latc, dtype=np.float64).reshape(parent.ny + 1, parent.nx + 1)
    nlon, nlat = nest_corners(lon, lat, NEST_I0, NEST_J0)
    # no date line (in either convention) inside the block, and the block lies on an equatorial tile
    assert 0.2 < nlon.min() and nlon.max() < np.pi - 0.2 and np.abs(nlat).max() < 0.8, (nlon.min(), nlon.max(), nlat.min(), nlat.max())
    return fg.GridConfig(6, 6, nlon, nlat)


def case_n(fg):
    """case B (C8, land 30 x 16, ocean 36 x 20) with a seventh atmosphere tile of 6 x 6 cells; tile_nest = 6"""
    c = dict(case_b(fg))
    c["atm"] = c["atm"] + [nest_tile(fg, c["atm"][NEST_PARENT])]
    c["tile_nest"] = 6
    return c


def wave_w1(fg):
    lo, la = fg.latlon_corners(24, 14, 20.0, 200.0, -60.0, 70.0)
    return [fg.GridConfig(24, 14, lo, la)]


def wave_wb(fg):
    """two wave tiles over case B's 9-degree ocean rows: the first lies strictly inside one row (1 .. 8 N), so that no corner row of
    the ocean lies inside (yw_min, yw_max) and the band of :3107-3117 is empty (js = nyo - 1 > je = 0) although the tile lies over
    sea; the second is an ordinary regional tile"""
    l1, a1 = fg.latlon_corners(6, 4, 30.0, 60.0, 1.0, 8.0)
    l2, a2 = fg.latlon_corners(8, 6, 100.0, 180.0, -30.0, 30.0)
    return [fg.GridConfig(6, 4, l1, a1), fg.GridConfig(8, 6, l2, a2)]


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def nest_reference(fg, order, **kw):
    """(case N, its restatement), computed once per session and variant"""
    def make():
        c = case_n(fg)
        r = _cached(("n-lists", order), lambda: reference_coupler(c["atm"], c["lnd"], c["ocn"], c["omask"], order, ocn_south_ext=c["ext"]))
        return c, with_nest(c, r, 6, **kw)
    return _cached(("n", order, tuple(sorted(kw.items()))), make)


def wave_reference(name, fg, order, **kw):
    """(case, the atmosphere side's restatement, the wave side's) of W1, W2, W0, WB"""
    def make():
        if name == "w2":
            c, r = reference_of("a", fg, order)
            c = dict(c, wav=[c["ocn"]], wav_same=True)
        else:
            c, r = reference_of("b", fg, order)
            c = dict(c, wav=wave_wb(fg) if name == "wb" else wave_w1(fg), wav_same=False)
            if name == "w0":
                c["omask"] = np.zeros_like(c["omask"])
                r = _cached(("b0", order), lambda: reference_coupler(c["atm"], c["lnd"], c["ocn"], c["omask"], order, ocn_south_ext=c["ext"]))
        return c, r, reference_wave(c["wav"], c["ocn"], c["omask"], order, **kw)
    return _cached((name, order, tuple(sorted(kw.items()))), make)


def check_of(c, r, tile_nest=-1, w=None):
    lists = r["axl"], r["axo"]
    return reference_check(c["atm"], [t["area"] for t in r["atmos"]], *lists, tile_nest=tile_nest, wxo=None if w is None else w["wxo"])
