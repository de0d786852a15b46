"""runoff_regrid on the device (tools/runoff_regrid/runoff_regrid.c): a handle per grid pair (fg_runoff, include/fregrid_hip.h)
with setup_remap's exchange list and nearest-ocean maps (:430) and process_data's arithmetic per time level (:626-675), the
nearest() search on its own (:708), and numpy mirrors of the tool's grid preparation (get_input_grid :279-314, get_output_grid
:347-423).  The tool's netCDF and mosaic handling is the caller's.  There is no CPU fallback: without a device every compute
entry raises."""
import ctypes as C

import numpy as np

from ._lib import check, lib, require_gpu

_dpt = C.POINTER(C.c_double)
_ipt = C.POINTER(C.c_int)
D2R = np.pi / 180                     # runoff_regrid.c:41
EPSLN10 = 1.e-10                      # :40


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _dp(a):
    return a.ctypes.data_as(_dpt)


def _ip(a):
    return a.ctypes.data_as(_ipt)


def set_runoff_prune(on):
    """1 (default): the nearest search skips tiles by their bounding balls; 0: it visits every tile.  Same results (test hook)."""
    lib().fg_set_runoff_prune(1 if on else 0)


def runoff_tile():
    """compacted ocean points per tile of the nearest search"""
    return int(lib().fg_runoff_tile())


def _grid_area(nx, ny, xc, yc):
    from . import get_grid_area
    return get_grid_area(nx, ny, xc, yc).reshape(ny, nx)


def runoff_input_grid(xt1d_deg, yt1d_deg, field, missing=-1.e+20, with_area=True):
    """get_input_grid :279-314.  xt1d_deg [nx], yt1d_deg [ny]: the field's axes in degrees; field [ny, nx]: its first time level.
    Returns a dict: nx, ny, xc1d [nx+1], yc1d [ny+1] (radians), mask [ny, nx] (0 where |field - missing| <= 1e-10), area [ny, nx] (get_grid_area on the device; left out with with_area=False)."""
    xt, yt = _f64(xt1d_deg).reshape(-1), _f64(yt1d_deg).reshape(-1)
    nx, ny = xt.size, yt.size
    xc, yc = np.empty(nx + 1), np.empty(ny + 1)
    xc[1:nx] = (xt[:-1] + xt[1:]) * 0.5
    xc[0] = 2 * xt[0] - xc[1]
    xc[nx] = 2 * xt[nx - 1] - xc[nx - 1]
    yc[1:ny] = (yt[:-1] + yt[1:]) * 0.5
    yc[0] = 2 * yt[0] - yc[1]
    yc[ny] = 2 * yt[ny - 1] - yc[ny - 1]
    xc *= D2R
    yc *= D2R
    xc2, yc2 = np.meshgrid(xc, yc)
    data = _f64(field).reshape(ny, nx)
    mask = np.where(np.abs(data - missing) <= EPSLN10, 0.0, 1.0)
    g = dict(nx=nx, ny=ny, xc1d=xc, yc1d=yc, mask=mask)
    if with_area:
        g["area"] = _grid_area(nx, ny, xc2, yc2)
    return g


def runoff_output_grid(x_super_deg, y_super_deg, depth, sea_level=0.0, with_area=True):
    """get_output_grid :347-423.  x_super_deg, y_super_deg [2*ny0+1, 2*nx+1]: the ocean supergrid in degrees; depth [ny0, nx]: the
    topography.  When the grid does not reach the south pole (y[0, 0] > -90 + 1e-10) one row of land cells is added below it
    (n_ext = 1), with corners at -90 and centres at 0.5 * (yc[0] + yc[1]), taken in degrees.  Returns a dict: nx, ny (with the
    extension), n_ext, xc, yc [ny+1, nx+1], xt, yt, mask, area [ny, nx] (radians; mask 1 where depth > sea_level; area as in runoff_input_grid)."""
    xs, ys = _f64(x_super_deg), _f64(y_super_deg)
    if xs.ndim != 2 or xs.shape != ys.shape or xs.shape[0] % 2 != 1 or xs.shape[1] % 2 != 1:
        raise ValueError("the supergrid arrays must be [2*ny+1, 2*nx+1]")
    ny0, nx = xs.shape[0] // 2, xs.shape[1] // 2
    n_ext = 1 if ys[0, 0] > -90 + EPSLN10 else 0
    ny = ny0 + n_ext
    xc, yc = np.empty((ny + 1, nx + 1)), np.empty((ny + 1, nx + 1))
    xt, yt = np.empty((ny, nx)), np.empty((ny, nx))
    yc[n_ext:] = ys[0::2, 0::2]
    yt[n_ext:] = ys[1::2, 1::2]
    xc[n_ext:] = xs[0::2, 0::2]
    xt[n_ext:] = xs[1::2, 1::2]
    if n_ext:
        yc[0] = -90
        yt[0] = 0.5 * (yc[0, :nx] + yc[1, :nx])
        xc[0] = xc[1]
        xt[0] = xt[1]
    xt *= D2R
    yt *= D2R
    xc *= D2R
    yc *= D2R
    d = _f64(depth)
    if d.shape != (ny0, nx):
        raise ValueError("runoff_regrid: grid size mismatch between mosaic file and topog file")
    mask = np.zeros((ny, nx))
    mask[n_ext:][d > sea_level] = 1.0
    g = dict(nx=nx, ny=ny, n_ext=n_ext, xc=xc, yc=yc, xt=xt, yt=yt, mask=mask)
    if with_area:
        g["area"] = _grid_area(nx, ny, xc, yc)
    return g


def nearest_unmasked(mask, lon, lat, qindex):
    """nearest() (:708) for the grid's own points qindex (row-major indices): mask, lon, lat [nlat, nlon] (radians).  Returns
    (iout, jout) [nq]; -1 where no point with mask != 0 lies within the reference's bound."""
    require_gpu()
    mask, lon, lat, q = _f64(mask), _f64(lon), _f64(lat), _i32(qindex).reshape(-1)
    if mask.ndim != 2 or lon.shape != mask.shape or lat.shape != mask.shape:
        raise ValueError("mask, lon and lat must be [nlat, nlon]")
    iout, jout = np.empty(q.size, dtype=np.int32), np.empty(q.size, dtype=np.int32)
    check(lib().fg_nearest_unmasked(mask.shape[1], mask.shape[0], _dp(mask), _dp(lon), _dp(lat), q.size, _ip(q), _ip(iout), _ip(jout)))
    return iout, jout


class RunoffRegrid:
    """RAII wrapper of fg_runoff.  grid_in: nx, ny, xc1d, yc1d, mask (runoff_input_grid's dict; area too when xgrid is given);
    grid_out: nx, ny, xc, yc, xt, yt, mask, area (runoff_output_grid's).  xgrid: (i_in, j_in, i_out, j_out, xgrid_area) to use
    instead of the handle's own create_xgrid_1dx2d_order1 search."""

    def __init__(self, grid_in, grid_out, xgrid=None, device=0):
        require_gpu()
        gi, go = grid_in, grid_out
        self.nx_in, self.ny_in, self.nx, self.ny, self.device = int(gi["nx"]), int(gi["ny"]), int(go["nx"]), int(go["ny"]), device
        mask_in = _f64(gi["mask"])
        xt, yt, mask_out, area_out = _f64(go["xt"]), _f64(go["yt"]), _f64(go["mask"]), _f64(go["area"])
        if mask_in.size != self.nx_in * self.ny_in or any(a.size != self.nx * self.ny for a in (xt, yt, mask_out, area_out)):
            raise ValueError("grid arrays do not match nx, ny")
        h = C.c_void_p()
        self._h = None
        if xgrid is None:
            xb, yb, xc, yc = _f64(gi["xc1d"]), _f64(gi["yc1d"]), _f64(go["xc"]), _f64(go["yc"])
            if xb.size != self.nx_in + 1 or yb.size != self.ny_in + 1 or xc.size != (self.nx + 1) * (self.ny + 1) or yc.size != xc.size:
                raise ValueError("corner arrays do not match nx, ny")
            check(lib().fg_runoff_create(self.nx_in, self.ny_in, _dp(xb), _dp(yb), _dp(mask_in), self.nx, self.ny, _dp(xc), _dp(yc),
                                         _dp(xt), _dp(yt), _dp(mask_out), _dp(area_out), device, C.byref(h)))
        else:
            area_in = _f64(gi["area"])
            ii, ji, io, jo = (_i32(a).reshape(-1) for a in xgrid[:4])
            xa = _f64(xgrid[4]).reshape(-1)
            if area_in.size != mask_in.size or any(a.size != xa.size for a in (ii, ji, io, jo)):
                raise ValueError("exchange list arrays differ in length, or area does not match the input grid")
            check(lib().fg_runoff_create_from_xgrid(self.nx_in, self.ny_in, _dp(mask_in), _dp(area_in), self.nx, self.ny, _dp(xt), _dp(yt),
                                                    _dp(mask_out), _dp(area_out), xa.size, _ip(ii), _ip(ji), _ip(io), _ip(jo), _dp(xa),
                                                    device, C.byref(h)))
        self._h = h

    def destroy(self):
        if self._h is not None and self._h.value:
            lib().fg_runoff_destroy(self._h)
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
        return lib().fg_runoff_stream(self._h)

    def maps(self):
        """(imap, jmap) [ny, nx]: the nearest ocean cell of every land cell, -1 on ocean cells"""
        imap, jmap = np.empty((self.ny, self.nx), dtype=np.int32), np.empty((self.ny, self.nx), dtype=np.int32)
        check(lib().fg_runoff_get_maps(self._h, _ip(imap), _ip(jmap)))
        return imap, jmap

    def xgrid(self):
        """(i_in, j_in, i_out, j_out, xgrid_area) in list order"""
        n = check(lib().fg_runoff_nxgrid(self._h))
        idx = [np.empty(n, dtype=np.int32) for _ in range(4)]
        area = np.empty(n)
        check(lib().fg_runoff_get_xgrid(self._h, *[_ip(a) for a in idx], _dp(area)))
        return (*idx, area)

    def xyz(self):
        """distance()'s point triples (x, y, z) [ny, nx] of the output grid's centres, as the search uses them"""
        out = [np.empty((self.ny, self.nx)) for _ in range(3)]
        check(lib().fg_runoff_get_xyz(self._h, *[_dp(a) for a in out]))
        return tuple(out)

    def search_stats(self):
        """dict: queries, tiles, tiles_visited (over all queries), tiles_visited_max (by one query)"""
        s = (C.c_long * 4)()
        check(lib().fg_runoff_search_stats(self._h, s))
        return dict(queries=s[0], tiles=s[1], tiles_visited=s[2], tiles_visited_max=s[3])

    def phase_ms(self):
        """setup wall time in ms: dict xgrid, convert, nearest, nearest_kernel, sort_upload"""
        ms = (C.c_float * 5)()
        check(lib().fg_runoff_phase_ms(self._h, ms, 5))
        return dict(zip(("xgrid", "convert", "nearest", "nearest_kernel", "sort_upload"), ms))

    def apply(self, data_in):
        """One time level data_in [ny_in, nx_in] -> (data_out [ny, nx], runoff_total_in, runoff_total_out, rate_change), the
        last three as process_data prints them (:666-675).  numpy in, numpy out; a contiguous float64 torch tensor on the
        handle's device in, a torch tensor out."""
        if tuple(data_in.shape) != (self.ny_in, self.nx_in):
            raise ValueError(f"data_in must be [{self.ny_in}, {self.nx_in}], got {tuple(data_in.shape)}")
        tot = (C.c_double * 2)()
        if type(data_in).__module__.split(".")[0] == "torch":
            import torch
            if data_in.dtype != torch.float64 or not data_in.is_cuda or not data_in.is_contiguous():
                raise ValueError("a torch input must be a contiguous float64 tensor on the device")
            out = torch.empty((self.ny, self.nx), dtype=torch.float64, device=data_in.device)
            torch.cuda.current_stream(data_in.device).synchronize()       # the handle's stream does not wait for torch's
            check(lib().fg_runoff_apply_dev(self._h, data_in.data_ptr(), out.data_ptr(), tot))
        else:
            a = _f64(data_in)
            out = np.empty((self.ny, self.nx))
            check(lib().fg_runoff_apply(self._h, _dp(a), _dp(out), tot))
        t_in, t_out = tot[0], tot[1]
        rate = (t_out - t_in) / t_in if (t_in > 0 and t_out > 0) else 0.0      # :672-675
        return out, t_in, t_out, rate
