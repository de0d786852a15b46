"""Atmosphere x land x ocean exchange grid of make_coupler_mosaic (tools/make_coupler_mosaic/make_coupler_mosaic.c:1360-1727,
legacy clip, one tile per component grid or several atmosphere tiles) as THREE searches on the device instead of three nested
brute-force loops:

  1. plan(atm -> lnd): the atmosphere x land cells and their clipped polygons (fg_plan_get_polygons) -- the reference keeps the
     vertices of each (atmxlnd_x / _y, :1560-1577);
  2. plan(atm -> ocn): the atmosphere x ocean cells, weighted by the ocean fraction (:1604-1657);
  3. plan(polygon list -> ocn) (fg_plan_create_polylist): every atmosphere x land polygon clipped against the ocean cells it
     overlaps, weighted by the land fraction and added up per polygon in ocean-cell order (:1659-1692), then the final area
     test of the atmosphere x land cell (:1700-1716).

The plans apply create_xgrid's acceptance (area / min(area_src, area_dst) > 1e-6, no weights); the coupler's own tests
(area x fraction against its own reference areas) can only reject more, so they are applied here, on the host, to the plans'
lists -- same products, same order, same bits as the reference loop (tests/test_gpu_coupler.py drives the reference's own
compiled clip_2dx2d / poly_area / poly_ctrlon / fix_lon through that loop and compares bit for bit).

coupler_xgrid is host logic over the plans' downloaded lists; it does not cover lnd_same_as_atm's vertex copy (pass distinct
grids), the land x ocean list or the bookkeeping after :1727.

CouplerMosaic (fg_coupler_*, csrc/coupler.hip) is the tool's compute core as one device-resident pipeline:
:1198-2127 and :2466-2811 -- land on the atmosphere grid or of its own, the three lists, the per-cell area and centroid sums, the
centroid distances, the land and ocean masks -- with the lists and polygons kept in device memory between the searches, and the
exchange-grid and mask files through the library's classic-netCDF writer.  coupler_ocean_grid is the numpy mirror of the ocean
grid preparation (:841-876, :940-955).  CouplerMosaic(clip_method="great_circle") is the tool's GREAT_CIRCLE_CLIP branch
(fg_coupler_create_gc, first order): unit vectors, clip_2dx2d_great_circle, and the remembered polygons searched by the great-circle
polygon-list plan (XgridPlan.create_polylist_gc).  CouplerMosaic(tile_nest=...) leaves a nested atmosphere tile's terms out of the
land and ocean cells' sums (:1765, :1792, :1857, :1903); CouplerMosaic(wav=...) adds the wave x ocean exchange grid (:2976-3535,
legacy clip); check() is --check (:3591-3661).  Not covered: several ocean tiles, the MPI split, the coupler mosaic file, the wave
grid on the great-circle handle; coupler_xgrid is legacy clip only and knows none of the three.
"""
import ctypes as C
import os

import numpy as np

from ._lib import check, lib, require_gpu
from .conserve_interp import GridConfig, XgridPlan

MIN_AREA_FRAC = 1.0e-4          # make_coupler_mosaic.c:148
AREA_RATIO_THRESH = 1.0e-6      # :362


def coupler_xgrid(atm, lnd, ocn, omask, interp_order=2, area_ratio_thresh=AREA_RATIO_THRESH, device=0):
    """atm: list of GridConfig (atmosphere tiles), lnd / ocn: one GridConfig each, omask [ny_ocn, nx_ocn] ocean fraction.
    Returns dict(axo=..., axl=...): axo = atmosphere x ocean cells (ta, ia, ja, io, jo, area[, clon, clat]) in the reference's
    order (atmosphere cell major, ocean cell ascending); axl = atmosphere x land cells (ta, ia, ja, il, jl, area[, clon, clat])."""
    from . import get_grid_area
    from ._lib import lib
    lib().fg_set_search_frame(1)            # the coupler's longitude convention for the second cell of a pair (fix_lon(cell, xa_avg))
    try:
        return _coupler_xgrid(atm, lnd, ocn, omask, interp_order, area_ratio_thresh, device, get_grid_area)
    finally:
        lib().fg_set_search_frame(0)


def _coupler_xgrid(atm, lnd, ocn, omask, interp_order, area_ratio_thresh, device, get_grid_area):
    order = 2 if interp_order == 2 else 1
    omask = np.ascontiguousarray(omask, dtype=np.float64).reshape(-1)
    area_atm = np.concatenate([get_grid_area(g.nx, g.ny, g.lonc, g.latc) for g in atm])
    area_lnd = get_grid_area(lnd.nx, lnd.ny, lnd.lonc, lnd.latc)
    area_ocn = get_grid_area(ocn.nx, ocn.ny, ocn.lonc, ocn.latc)
    off = np.concatenate([[0], np.cumsum([g.nx * g.ny for g in atm])])
    nxa = np.array([g.nx for g in atm])

    def atm_cell(x):
        return off[x["t_in"]] + x["j_in"].astype(np.int64) * nxa[x["t_in"]] + x["i_in"]

    # --- 1. atmosphere x land candidates and their polygons (:1398-1585)
    p = XgridPlan.create(order, atm, lnd, device=device)
    xl = p.get_xgrid()
    poly = p.get_polygons(maxv=8)
    src_struct = p.get_cell_struct(0, int(off[-1]))
    p.destroy()
    xa_avg = src_struct["lon_avg"]                          # avgval_double(na_in, xa) after fix_lon(xa, ya, 4, M_PI), :1389-1394
    a_of_l = atm_cell(xl)
    lcell = xl["j_out"].astype(np.int64) * lnd.nx + xl["i_out"]
    if np.any(poly["n"] > 8):
        raise ValueError("coupler_xgrid: an atmosphere x land polygon has more than 8 vertices")
    min_area_l = np.minimum(area_lnd[lcell], area_atm[a_of_l])          # :1701

    # --- 2. atmosphere x ocean over sea (:1604-1657)
    p = XgridPlan.create(order, atm, ocn, device=device)
    xo = p.get_xgrid()
    p.destroy()
    ocell = xo["j_out"].astype(np.int64) * ocn.nx + xo["i_out"]
    frac = omask[ocell]
    xarea = xo["area"] * frac                                           # poly_area(...) * ocn_frac, :1634
    keep = (frac > MIN_AREA_FRAC) & (xarea / np.minimum(area_ocn[ocell], area_atm[atm_cell(xo)]) > area_ratio_thresh)
    axo = {"ta": xo["t_in"][keep], "ia": xo["i_in"][keep], "ja": xo["j_in"][keep], "io": xo["i_out"][keep], "jo": xo["j_out"][keep],
           "area": xarea[keep]}
    if order == 2:
        axo["clon"], axo["clat"] = xo["c1"][keep] * frac[keep], xo["c2"][keep] * frac[keep]      # :1648-1649

    # --- 3. the remembered atmosphere x land polygons against the ocean cells over land (:1659-1692)
    axl_area = np.zeros(poly["n"].size)
    axl_clon, axl_clat = np.zeros_like(axl_area), np.zeros_like(axl_area)
    if poly["n"].size:
        p = XgridPlan.create_polylist(order, poly["n"], poly["lon"], poly["lat"], xa_avg[a_of_l], min_area_l, ocn, device=device)
        xp = p.get_xgrid()
        p.destroy()
        l = xp["i_in"].astype(np.int64)
        oc = xp["j_out"].astype(np.int64) * ocn.nx + xp["i_out"]
        lfrac = 1.0 - omask[oc]
        xa = xp["area"] * lfrac                                         # :1673
        ok = (lfrac > MIN_AREA_FRAC) & (xa / min_area_l[l] > area_ratio_thresh)
        # axl_area[l] += xarea in ocean-cell order: the plan's order for one polygon is ascending ocean cell, and np.add.at adds
        # the selected terms one by one in array order
        np.add.at(axl_area, l[ok], xa[ok])
        if order == 2:
            np.add.at(axl_clon, l[ok], xp["c1"][ok] * lfrac[ok])
            np.add.at(axl_clat, l[ok], xp["c2"][ok] * lfrac[ok])
    fin = axl_area / min_area_l > area_ratio_thresh                     # :1704
    axl = {"ta": xl["t_in"][fin], "ia": xl["i_in"][fin], "ja": xl["j_in"][fin], "il": xl["i_out"][fin], "jl": xl["j_out"][fin],
           "area": axl_area[fin]}
    if order == 2:
        axl["clon"], axl["clat"] = axl_clon[fin], axl_clat[fin]
    return {"axo": axo, "axl": axl, "n_axl_polygons": int(poly["n"].size)}


D2R = np.pi / 180               # constant.h
TINY_VALUE = 1.0e-7             # make_coupler_mosaic.c:146
STRING = 255                    # mpp.h
_dpt = C.POINTER(C.c_double)
_ipt = C.POINTER(C.c_int)


def coupler_ocean_grid(x_deg, y_deg, omask=None):
    """:841-876 and :940-955 in numpy.  x_deg, y_deg [ny+1, nx+1]: the ocean model grid's corners in degrees (one tile); omask
    [ny, nx]: the ocean fraction (area_frac, or 1 where depth > sea_level), None for none.  When the first row lies above
    -90 + 1e-7 degrees' worth of radians one row down to -90 is added (ocn_south_ext = 1) with the longitudes of the first row and
    omask = 0.  Returns a dict: nx, ny (with the extension), ocn_south_ext, x, y [ny+1, nx+1] in radians, omask [ny, nx],
    jo_shift = 1 - ocn_south_ext (what the exchange-grid files add to a 0-based jo, :2309, :2876), uniform (whether the first
    row has one latitude, :846-851)."""
    xd, yd = np.ascontiguousarray(x_deg, dtype=np.float64), np.ascontiguousarray(y_deg, dtype=np.float64)
    if xd.ndim != 2 or xd.shape != yd.shape or xd.shape[0] < 2 or xd.shape[1] < 2:
        raise ValueError("x_deg, y_deg must be [ny+1, nx+1]")
    ny0, nx = xd.shape[0] - 1, xd.shape[1] - 1
    uniform = bool(np.all(yd[0, 1:] == yd[0, :-1]))
    min_atm_lat = -90. * D2R
    ext = 1 if yd[0, 0] * D2R > min_atm_lat + TINY_VALUE else 0
    ny = ny0 + ext
    x, y = np.empty((ny + 1, nx + 1)), np.empty((ny + 1, nx + 1))
    x[ext:] = xd * D2R
    y[ext:] = yd * D2R
    if ext:
        x[0] = x[1]
        y[0] = min_atm_lat
    m = np.zeros((ny, nx))
    if omask is not None:
        om = np.ascontiguousarray(omask, dtype=np.float64)
        if om.shape != (ny0, nx):
            raise ValueError("make_coupler_mosaic: grid size mismatch between mosaic file and topog file")
        m[ext:] = om
    return dict(nx=nx, ny=ny, ocn_south_ext=ext, x=x, y=y, omask=m, jo_shift=1 - ext, uniform=uniform)


def write_xgrid_file(path, contact, i1, j1, i2, j2, area, dist1=None, dist2=None, j2_shift=1):
    """One exchange-grid file from host arrays (fg_coupler_write_xgrid; :2158-2244): contact, tile1_cell, tile2_cell [ncells, 2]
    (1-based: the 0-based indices + 1, the second grid's j + j2_shift), xgrid_area, and with dist1 / dist2 (each a pair (di, dj))
    tile1_distance / tile2_distance [ncells, 2] and the order-2 attributes of contact.  An empty list gets no file: an error here."""
    ints = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (i1, j1, i2, j2)]
    dbl = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (area,) + (tuple(dist1) + tuple(dist2) if dist1 is not None else ())]
    n = dbl[0].size
    if any(v.size != n for v in ints + dbl):
        raise ValueError("the arrays of an exchange-grid file must have one length")
    check(lib().fg_coupler_write_xgrid(str(path).encode(), contact.encode(), n, *[v.ctypes.data_as(_ipt) for v in ints], int(j2_shift),
                                       *[v.ctypes.data_as(_dpt) for v in dbl], *([None] * (5 - len(dbl)))))


def write_wave_xgrid_file(path, contact, iw, jw, io, jo, area, dist1=None, dist2=None, jo_shift=1):
    """A wave x ocean exchange-grid file from host arrays (fg_coupler_write_wave_xgrid; :3461-3527): write_xgrid_file's variables and
    attributes with :3476-3477's names on tile1_cell / tile2_cell; jo_shift = 1 - ocn_south_ext (:3492)."""
    ints = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (iw, jw, io, jo)]
    dbl = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (area,) + (tuple(dist1) + tuple(dist2) if dist1 is not None else ())]
    n = dbl[0].size
    if any(v.size != n for v in ints + dbl):
        raise ValueError("the arrays of an exchange-grid file must have one length")
    check(lib().fg_coupler_write_wave_xgrid(str(path).encode(), contact.encode(), n, *[v.ctypes.data_as(_ipt) for v in ints], int(jo_shift),
                                            *[v.ctypes.data_as(_dpt) for v in dbl], *([None] * (5 - len(dbl)))))


def write_wave_mask_file(path, mask):
    """wave_mask.nc / wave_mask_tileN.nc (:3405-3419) from a host array [ny, nx]: the single variable mask"""
    m = np.ascontiguousarray(mask, dtype=np.float64)
    if m.ndim != 2:
        raise ValueError("the wave mask must be [ny, nx]")
    check(lib().fg_coupler_write_wave_mask(str(path).encode(), m.shape[1], m.shape[0], m.ctypes.data_as(_dpt)))


def write_mask_file(path, kind, fields):
    """ocean_mask.nc (kind "ocean": fields mask, areaO, areaX, :2055-2066) or a land mask file (kind "land": mask, area_lnd, l_area and
    area_atm when given, :2103-2117) from host arrays [ny, nx] (fg_coupler_write_mask)."""
    keys = {"ocean": ("mask", "areaO", "areaX"), "land": ("mask", "area_lnd", "l_area")}[kind]
    a = [np.ascontiguousarray(fields[k], dtype=np.float64) for k in keys]
    ny, nx = a[0].shape
    atm = np.ascontiguousarray(fields["area_atm"], dtype=np.float64) if kind == "land" and "area_atm" in fields else None
    if any(v.shape != (ny, nx) for v in a) or (atm is not None and atm.shape != (ny, nx)):
        raise ValueError("the fields of a mask file must be [ny, nx]")
    check(lib().fg_coupler_write_mask(str(path).encode(), 1 if kind == "ocean" else 0, nx, ny, *[v.ctypes.data_as(_dpt) for v in a],
                                      atm.ctypes.data_as(_dpt) if atm is not None else None))


class CouplerMosaic:
    """RAII wrapper of fg_coupler.  atm: list of GridConfig (atmosphere tiles); lnd: None (land on the atmosphere grid,
    lnd_same_as_atm), one GridConfig or a list of them; ocn: one GridConfig, the grid the tool works on (coupler_ocean_grid's x, y);
    omask [ny_ocn, nx_ocn]: the ocean fraction; ocn_south_ext: coupler_ocean_grid's.  Corners in radians.
    clip_method "legacy" (clip_2dx2d on lon / lat) or "great_circle" (the tool's GREAT_CIRCLE_CLIP branch, fg_coupler_create_gc:
    clip_2dx2d_great_circle on unit vectors, what a grid with a pole inside a cell needs; interp_order must then be 1).
    tile_nest: None, or the index of the nested atmosphere tile (fg_coupler_set_nest; refused with land on the atmosphere grid).
    wav: None, one GridConfig or a list of them: the wave grid's tiles (fg_coupler_add_wave; legacy clip only); wav_same_as_ocn: the
    wave mosaic is the ocean mosaic (the names of write_wave's files)."""

    AXL, AXO, LXO, WXO = 0, 1, 2, 3
    ATM, LND, OCN, WAV = 0, 1, 2, 3

    def __init__(self, atm, lnd, ocn, omask, interp_order=2, area_ratio_thresh=AREA_RATIO_THRESH, ocn_south_ext=0, device=0, clip_method="legacy",
                 tile_nest=None, wav=None, wav_same_as_ocn=False):
        self._h = None
        if clip_method not in ("legacy", "great_circle"):
            raise ValueError("clip_method must be 'legacy' or 'great_circle'")
        self.clip_method = clip_method
        require_gpu()
        self.atm = list(atm)
        self.same = lnd is None
        self.lnd = self.atm if self.same else (list(lnd) if isinstance(lnd, (list, tuple)) else [lnd])
        self.ocn, self.order, self.ocn_south_ext, self.device = ocn, int(interp_order), int(ocn_south_ext), device
        om = np.ascontiguousarray(omask, dtype=np.float64)
        if om.size != ocn.nx * ocn.ny:
            raise ValueError(f"omask must be [{ocn.ny}, {ocn.nx}]")

        def table(grids):
            keep = [(np.ascontiguousarray(g.lonc, dtype=np.float64), np.ascontiguousarray(g.latc, dtype=np.float64)) for g in grids]
            for g, (lo, la) in zip(grids, keep):
                if lo.size != (g.nx + 1) * (g.ny + 1) or la.size != lo.size:
                    raise ValueError("a grid's corner arrays must be [ny+1, nx+1]")
            n = len(grids)
            return (keep, (C.c_int * n)(*[g.nx for g in grids]), (C.c_int * n)(*[g.ny for g in grids]),
                    (_dpt * n)(*[k[0].ctypes.data_as(_dpt) for k in keep]), (_dpt * n)(*[k[1].ctypes.data_as(_dpt) for k in keep]))

        ka, nxa, nya, loa, laa = table(self.atm)
        kl, nxl, nyl, lol, lal = table(self.lnd)
        ko, _, _, _, _ = table([ocn])
        h = C.c_void_p()
        create = lib().fg_coupler_create_gc if clip_method == "great_circle" else lib().fg_coupler_create
        check(create(self.order, float(area_ratio_thresh), len(self.atm), nxa, nya, loa, laa, 0 if self.same else len(self.lnd),
                     nxl, nyl, lol, lal, ocn.nx, ocn.ny, ko[0][0].ctypes.data_as(_dpt), ko[0][1].ctypes.data_as(_dpt),
                     om.ctypes.data_as(_dpt), self.ocn_south_ext, device, C.byref(h)))
        self._h = h
        self.tile_nest = None if tile_nest is None else int(tile_nest)
        self.wav = [] if wav is None else (list(wav) if isinstance(wav, (list, tuple)) else [wav])
        self.wav_same_as_ocn = bool(wav_same_as_ocn)
        try:
            if self.tile_nest is not None:
                check(lib().fg_coupler_set_nest(self._h, self.tile_nest))
            if self.wav:
                _, nxw, nyw, low, law = table(self.wav)
                check(lib().fg_coupler_add_wave(self._h, len(self.wav), nxw, nyw, low, law, int(self.wav_same_as_ocn)))
        except Exception:
            self.destroy()
            raise

    def destroy(self):
        if self._h is not None and self._h.value:
            lib().fg_coupler_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        """the hipStream_t (as an int) the handle queues its work on"""
        return lib().fg_coupler_stream(self._h)

    def run(self):
        check(lib().fg_coupler_run(self._h))
        return self

    def _list(self, which, t1, t2, names):
        n = check(lib().fg_coupler_count(self._h, which, t1, t2))
        out = {k: np.empty(n, dtype=np.int32) for k in names}
        out["area"] = np.empty(n)
        dbl = ("clon", "clat", "di1", "dj1", "di2", "dj2") if self.order == 2 else ()
        for k in dbl:
            out[k] = np.empty(n)
        ints = [out[k].ctypes.data_as(_ipt) for k in names]
        dbls = [out[k].ctypes.data_as(_dpt) for k in dbl] + [None] * (6 - len(dbl))
        check(lib().fg_coupler_get(self._h, which, t1, t2, *ints, out["area"].ctypes.data_as(_dpt), *dbls))
        return out

    def axl(self, ta, tl):
        """atmosphere tile ta x land tile tl in the reference's order: dict ia, ja, il, jl (0-based), area, and for order 2 clon, clat
        (the centroid integrals), di1, dj1 (tile1_distance), di2, dj2 (tile2_distance)"""
        return self._list(self.AXL, ta, tl, ("ia", "ja", "il", "jl"))

    def axo(self, ta):
        """atmosphere tile ta x ocean: dict ia, ja, io, jo (jo counts the added southern row), area, ..."""
        return self._list(self.AXO, ta, 0, ("ia", "ja", "io", "jo"))

    def lxo(self, tl):
        """land tile tl x ocean (land of its own only): dict il, jl, io, jo, area, ..."""
        return self._list(self.LXO, tl, 0, ("il", "jl", "io", "jo"))

    def wxo(self, tw):
        """wave tile tw x ocean (a handle with a wave grid): dict iw, jw, io, jo, area, and for order 2 clon, clat, di1 .. dj2"""
        return self._list(self.WXO, tw, 0, ("iw", "jw", "io", "jo"))

    def wave_ocean_cells(self):
        """the ocean cells' wave-side sums (:3329-3332, :3366-3371; order 2), [ny, nx] each: dict xarea, clon, clat.  Not the
        atmosphere-side o_area of cells(OCN)."""
        out = {k: np.empty((self.ocn.ny, self.ocn.nx)) for k in ("xarea", "clon", "clat")}
        check(lib().fg_coupler_get_wave_ocean(self._h, *[out[k].ctypes.data_as(_dpt) for k in ("xarea", "clon", "clat")]))
        return out

    def check(self):
        """--check (:3591-3661; fg_coupler_check): dict max_ratio, max_tile, max_i, max_j (0-based; the first cell with the largest
        |atm_xarea - area_atm| / area_atm), max_area_atm, max_atm_xarea, atm_area_sum, axl_area_sum, axo_area_sum, axo_area_frac,
        axl_area_frac, tiling_area (percent); with a nest their _nest counterparts; with a wave grid wxo_area_sum"""
        v = (C.c_double * 19)()
        check(lib().fg_coupler_check(self._h, v, 19))
        names = ("atm_area_sum", "axl_area_sum", "axo_area_sum", "axo_area_frac", "axl_area_frac", "tiling_area")
        out = dict(max_ratio=v[0], max_tile=int(v[1]), max_i=int(v[2]), max_j=int(v[3]), max_area_atm=v[4], max_atm_xarea=v[5])
        out.update(zip(names, v[6:12]))
        if self.tile_nest is not None and self.tile_nest >= 0:
            out.update(zip([k + "_nest" for k in names], v[12:18]))
        if self.wav:
            out["wxo_area_sum"] = v[18]
        return out

    def cells(self, grid, tile=0):
        """per cell of one tile (grid: ATM, LND, OCN, WAV), [ny, nx] each: dict area (get_grid_area), xarea (a_area / l_area / o_area /
        w_area), frac (their ratio: the land mask, the ocean fraction, the wave mask) and for order 2 clon, clat (the centroid)"""
        g = (self.atm, self.lnd, [self.ocn], self.wav)[grid][tile]
        names = ("area", "xarea", "frac") + (("clon", "clat") if self.order == 2 else ())
        out = {k: np.empty((g.ny, g.nx)) for k in names}
        ptr = [out[k].ctypes.data_as(_dpt) for k in names] + [None] * (5 - len(names))
        check(lib().fg_coupler_get_cells(self._h, grid, tile, *ptr))
        return out

    def stats(self):
        """dict: d2h_bytes (what run() copied to the host), nbad, searches, naxo, naxl, nlxo, npolygons, ocn_south_ext, and with a
        wave grid nwxo"""
        s = (C.c_long * 9)()
        check(lib().fg_coupler_stats(self._h, s, 9))
        return dict(zip(("d2h_bytes", "nbad", "searches", "naxo", "naxl", "nlxo", "npolygons", "ocn_south_ext") + (("nwxo",) if self.wav else ()), s))

    def phase_ms(self):
        """wall time in ms: dict create, axl_candidates, axo, polygons_x_ocean, lxo, sums, run, and with a wave grid wxo"""
        ms = (C.c_float * 8)()
        check(lib().fg_coupler_phase_ms(self._h, ms, 8))
        return dict(zip(("create", "axl_candidates", "axo", "polygons_x_ocean", "lxo", "sums", "run") + (("wxo",) if self.wav else ()), ms))

    def write(self, directory, atm_mosaic="atmos_mosaic", lnd_mosaic="land_mosaic", ocn_mosaic="ocean_mosaic", atm_tiles=None, lnd_tiles=None,
              ocn_tile="tile1"):
        """The exchange-grid files (:2130-2462, :2813-2920) and ocean_mask.nc / land_mask[_tileN].nc (:2030-2120) into directory
        (fg_coupler_write); names as the tool forms them from the mosaic and tile names.  Returns the files written; an empty list
        gets no file."""
        atm_tiles = list(atm_tiles or [f"tile{k + 1}" for k in range(len(self.atm))])
        lnd_tiles = list(lnd_tiles or [f"tile{k + 1}" for k in range(len(self.lnd))])
        if len(atm_tiles) != len(self.atm) or len(lnd_tiles) != len(self.lnd):
            raise ValueError("one name per atmosphere tile and per land tile")
        table = [atm_mosaic, lnd_mosaic, ocn_mosaic] + atm_tiles + lnd_tiles + [ocn_tile]
        names = (C.c_char_p * len(table))(*[t.encode() for t in table])
        check(lib().fg_coupler_write(self._h, str(directory).encode(), names))
        count = lambda which, t1, t2: check(lib().fg_coupler_count(self._h, which, t1, t2))
        files = []
        for ta, at in enumerate(atm_tiles):
            files += [f"{atm_mosaic}_{at}X{lnd_mosaic}_{lt}.nc" for tl, lt in enumerate(lnd_tiles) if count(self.AXL, ta, tl)]
            files += [f"{atm_mosaic}_{at}X{ocn_mosaic}_{ocn_tile}.nc"] if count(self.AXO, ta, 0) else []
        if not self.same:
            files += [f"{lnd_mosaic}_{lt}X{ocn_mosaic}_{ocn_tile}.nc" for tl, lt in enumerate(lnd_tiles) if count(self.LXO, tl, 0)]
        files.append("ocean_mask.nc")
        files += ["land_mask.nc"] if len(self.lnd) == 1 else [f"land_mask_tile{k + 1}.nc" for k in range(len(self.lnd))]
        return [os.path.join(str(directory), f) for f in files]

    def write_wave(self, directory, wav_mosaic="wave_mosaic", ocn_mosaic="ocean_mosaic", wav_tiles=None, ocn_tile="tile1"):
        """The wave grid's files (:3397-3421, :3430-3535; fg_coupler_write_wave) into directory: per non-empty list
        <wav_mosaic>_<tile>X<ocn_mosaic>_<ocn_tile>.nc (wav_<...>Xocn_<...>.nc with wav_same_as_ocn) and wave_mask.nc or
        wave_mask_tile<k>.nc.  Returns the files written."""
        wav_tiles = list(wav_tiles or [f"tile{k + 1}" for k in range(len(self.wav))])
        if len(wav_tiles) != len(self.wav):
            raise ValueError("one name per wave tile")
        table = [wav_mosaic, ocn_mosaic] + wav_tiles + [ocn_tile]
        names = (C.c_char_p * len(table))(*[t.encode() for t in table])
        check(lib().fg_coupler_write_wave(self._h, str(directory).encode(), names))
        files = []
        for tw, wt in enumerate(wav_tiles):
            if check(lib().fg_coupler_count(self._h, self.WXO, tw, 0)):
                files.append(f"wav_{wav_mosaic}_{wt}Xocn_{ocn_mosaic}_{ocn_tile}.nc" if self.wav_same_as_ocn else f"{wav_mosaic}_{wt}X{ocn_mosaic}_{ocn_tile}.nc")
            files.append("wave_mask.nc" if len(self.wav) == 1 else f"wave_mask_tile{tw + 1}.nc")
        return [os.path.join(str(directory), f) for f in files]


__all__ = ["coupler_xgrid", "CouplerMosaic", "coupler_ocean_grid", "write_xgrid_file", "write_mask_file", "write_wave_xgrid_file",
           "write_wave_mask_file", "MIN_AREA_FRAC", "AREA_RATIO_THRESH"]
