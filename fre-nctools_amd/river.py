"""river_regrid on the device (tools/river_regrid/river_regrid.c): a handle per source network and land mosaic (fg_river,
include/fregrid_hip.h) that runs calc_max_subA (:694), calc_tocell (:880), calc_river_data (:991), sort_basin (:1298) and
check_river_data (:1180) on the arrays get_source_data and get_mosaic_grid leave in river_type, and numpy mirrors of the
tool's grid preparation (the source bounds :352-369, the land fraction thresholds :544-551).  The tool's netCDF and mosaic
reading, the exchange-grid files behind the land fractions and write_river_data are the caller's.  There is no CPU fallback:
without a device every compute entry raises."""
import ctypes as C

import numpy as np

from ._lib import FregridHipError, check, lib, require_gpu

_dpt = C.POINTER(C.c_double)
_ipt = C.POINTER(C.c_int)
D2R = np.pi / 180                     # constant.h
EPSLN = 1.e-4                         # river_regrid.c:92
X_CYCLIC, Y_CYCLIC, CUBIC_GRID = 1, 2, 4          # :87-89
MISSING_NAMES = ("subA", "tocell", "travel", "basin", "cellarea", "celllength")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return a.ctypes.data_as(_dpt)


def _ip(a):
    return a.ctypes.data_as(_ipt)


def set_river_prune(on):
    """1 (default): the max-subA search replays only the adjust_lon calls that change the longitudes and visits the source cells
    between them that can overlap; 0: every land cell walks every source cell in the reference's order.  Same results (test hook)."""
    lib().fg_set_river_prune(1 if on else 0)


def river_source_grid(xt_deg, yt_deg):
    """get_source_data :352-369.  xt_deg [nx], yt_deg [ny]: the axes of the river network file in degrees.  Returns a dict: nx,
    ny, xb [nx+1], yb [ny+1] (degrees), xb_r, yb_r (radians).  The four range errors of the reference are ValueErrors with its text."""
    xt, yt = _f64(xt_deg).reshape(-1), _f64(yt_deg).reshape(-1)
    nx, ny = xt.size, yt.size
    xb, yb = np.empty(nx + 1), np.empty(ny + 1)
    xb[1:nx] = 0.5 * (xt[:-1] + xt[1:])
    yb[1:ny] = 0.5 * (yt[:-1] + yt[1:])
    xb[0] = 2 * xt[0] - xb[1]
    yb[0] = 2 * yt[0] - yb[1]
    xb[nx] = 2 * xt[nx - 1] - xb[nx - 1]
    yb[ny] = 2 * yt[ny - 1] - yb[ny - 1]
    if abs(xb[0]) > EPSLN:
        raise ValueError("river_regrid: The starting longitude of grid bound is not 0")
    if abs(xb[nx] - 360) > EPSLN:
        raise ValueError("river_regrid: The ending longitude of grid bound is not 360")
    if abs(yb[0] + 90) > EPSLN:
        raise ValueError("river_regrid: The starting latitude of grid bound is not -90")
    if abs(yb[ny] - 90) > EPSLN:
        raise ValueError("river_regrid: The ending latitude of grid bound is not 90")
    xb[0], xb[nx], yb[0], yb[ny] = 0., 360., -90., 90.
    return dict(nx=nx, ny=ny, xb=xb, yb=yb, xb_r=xb * D2R, yb_r=yb * D2R)


def river_land_frac(frac, land_thresh=0.0, min_frac=0.0):
    """get_mosaic_grid :544-551: a fraction above 1 - land_thresh becomes 1, one below min_frac in size becomes 0.  The two fatal
    errors of the reference are ValueErrors with its text."""
    f = _f64(frac).copy()
    if np.any(f > 1 + 1.e-3):
        raise ValueError("river_regrid: land_frac > 1 + 1.e-3")
    f[f > 1 - land_thresh] = 1
    f[np.abs(f) < min_frac] = 0
    if np.any((f > 1) | (f < 0)):
        raise ValueError("river_regrid: land_frac should be between 0 or 1")
    return f


class RiverRegrid:
    """RAII wrapper of fg_river.
    source: dict with xb_r [nx_in+1], yb_r [ny_in+1] (river_source_grid's), subA [ny_in, nx_in] and missing: the six missing
        values of the network file in the order of MISSING_NAMES (a sequence, or a dict by those names).  subA's must fit an
        int and those of tocell, travel and basin must be negative integers, else FregridHipError (include/fregrid_hip.h).
    tiles: one dict per tile with xb_r, yb_r [ny+1, nx+1] (radians), xt, yt (degrees; [ny, nx], or [ny+2, nx+2] with a halo
        whose corners are kept where the reference's halo update leaves them alone), area [ny, nx] (get_grid_area or
        get_grid_great_circle_area) and landfrac [ny, nx] (river_land_frac's).
    opcode: X_CYCLIC | Y_CYCLIC | CUBIC_GRID, as get_mosaic_grid derives it from the mosaic's contacts."""

    def __init__(self, source, tiles, opcode, suba_cutoff=1.e12, device=0):
        require_gpu()
        self._h = None
        xb_r, yb_r, sub = _f64(source["xb_r"]).reshape(-1), _f64(source["yb_r"]).reshape(-1), _f64(source["subA"])
        nx_in, ny_in = xb_r.size - 1, yb_r.size - 1
        if sub.shape != (ny_in, nx_in):
            raise ValueError(f"source subA must be [{ny_in}, {nx_in}], got {sub.shape}")
        m = source["missing"]
        missing = _f64([m[k] for k in MISSING_NAMES] if isinstance(m, dict) else m).reshape(-1)
        if missing.size != 6:
            raise ValueError("source missing: six values, in the order " + ", ".join(MISSING_NAMES))
        ntiles = len(tiles)
        if ntiles < 1:
            raise ValueError("no tile")
        nxs, nys, keep = np.empty(ntiles, dtype=np.int32), np.empty(ntiles, dtype=np.int32), []
        ptrs = {k: (_dpt * ntiles)() for k in ("xb_r", "yb_r", "xt", "yt", "area", "landfrac")}
        for n, t in enumerate(tiles):
            lf = _f64(t["landfrac"])
            if lf.ndim != 2:
                raise ValueError("landfrac must be [ny, nx]")
            ny, nx = lf.shape
            nxs[n], nys[n] = nx, ny
            arr = dict(landfrac=lf, area=_f64(t["area"]), xb_r=_f64(t["xb_r"]), yb_r=_f64(t["yb_r"]))
            if arr["area"].size != nx * ny or arr["xb_r"].size != (nx + 1) * (ny + 1) or arr["yb_r"].size != (nx + 1) * (ny + 1):
                raise ValueError(f"tile {n}: area must be [ny, nx] and xb_r, yb_r [ny+1, nx+1]")
            for k in ("xt", "yt"):
                a = _f64(t[k])
                if a.shape == (ny, nx):
                    full = np.zeros((ny + 2, nx + 2))
                    full[1:-1, 1:-1] = a
                    a = full
                if a.shape != (ny + 2, nx + 2):
                    raise ValueError(f"tile {n}: {k} must be [ny, nx] or [ny+2, nx+2]")
                arr[k] = a
            for k, a in arr.items():
                ptrs[k][n] = _dp(a)
            keep.append(arr)
        self.ntiles, self.nx, self.ny, self.opcode, self.device = ntiles, int(nxs[0]), int(nys[0]), int(opcode), device
        h = C.c_void_p()
        check(lib().fg_river_create(nx_in, ny_in, _dp(xb_r), _dp(yb_r), _dp(sub), _dp(missing), ntiles, _ip(nxs), _ip(nys), int(opcode),
                                    ptrs["xb_r"], ptrs["yb_r"], ptrs["xt"], ptrs["yt"], ptrs["area"], ptrs["landfrac"],
                                    float(suba_cutoff), device, C.byref(h)))
        self._h = h

    def destroy(self):
        if self._h is not None and self._h.value:
            lib().fg_river_destroy(self._h)
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
        return lib().fg_river_stream(self._h)

    def run(self):
        """all five stages; a fatal check of the reference raises FregridHipError with its text"""
        check(lib().fg_river_run(self._h))
        return self

    def fields(self, tile):
        """dict subA, cellarea, celllength (float64), tocell, travel, basin (int32), each [ny, nx]: what write_river_data writes"""
        d = {k: np.empty((self.ny, self.nx)) for k in ("subA", "cellarea", "celllength")}
        i = {k: np.empty((self.ny, self.nx), dtype=np.int32) for k in ("tocell", "travel", "basin")}
        check(lib().fg_river_get(self._h, tile, _dp(d["subA"]), _ip(i["tocell"]), _ip(i["travel"]), _ip(i["basin"]),
                                 _dp(d["cellarea"]), _dp(d["celllength"])))
        d.update(i)
        return d

    def max_suba(self, tile):
        """calc_max_subA's result with its halo [ny+2, nx+2], as calc_tocell reads it"""
        out = np.empty((self.ny + 2, self.nx + 2))
        check(lib().fg_river_get_max_suba(self._h, tile, _dp(out)))
        return out

    def stats(self):
        """dict: maxtravel, maxbasin, coast_full_land, sink (check_river_data's counts), land_cells (full-land cells, those the
        search runs for), source_cells_visited, launches"""
        s = (C.c_long * 7)()
        check(lib().fg_river_stats(self._h, s, 7))
        return dict(zip(("maxtravel", "maxbasin", "coast_full_land", "sink", "land_cells", "source_cells_visited", "launches"), s))

    def phase_ms(self):
        """wall time in ms: dict create, max_suba, tocell_travel_basin, accumulate, sort_check"""
        ms = (C.c_float * 5)()
        check(lib().fg_river_phase_ms(self._h, ms, 5))
        return dict(zip(("create", "max_suba", "tocell_travel_basin", "accumulate", "sort_check"), ms))


def river_qsort_index(values):
    """qsort_index (:1538) on the host: (sorted values, index) with the reference's order among equal values"""
    a = _f64(values).reshape(-1).copy()
    idx = np.arange(a.size, dtype=np.int32)
    check(lib().fg_river_qsort_index(_dp(a), a.size, _ip(idx)))
    return a, idx


def river_sort_basin(basin, last_point, subA, basin_missing):
    """sort_basin (:1298) on flat arrays of all tiles: the new ids, maxbasin - rank of the outlet's subA"""
    basin, last, sub = np.asarray(basin).reshape(-1), np.asarray(last_point).reshape(-1), _f64(subA).reshape(-1)
    maxbasin = int(basin.max())
    if maxbasin < 1:
        return basin.copy()
    maxsuba = np.empty(maxbasin)
    maxsuba[basin[last != 0] - 1] = sub[last != 0]
    _, idx = river_qsort_index(maxsuba)
    rank = np.empty(maxbasin, dtype=np.int64)
    rank[idx] = np.arange(maxbasin)
    out = basin.copy()
    on = basin != basin_missing
    out[on] = maxbasin - rank[basin[on] - 1]
    return out


__all__ = ["RiverRegrid", "river_source_grid", "river_land_frac", "set_river_prune", "river_qsort_index", "river_sort_basin",
           "X_CYCLIC", "Y_CYCLIC", "CUBIC_GRID", "FregridHipError"]
