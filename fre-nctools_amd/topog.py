"""make_topog --topog_type realistic on the device (tools/make_topog/topog.c): a handle per model grid (fg_topog,
include/fregrid_hip.h) that takes the topography file's axes and field in their file type and runs create_realistic_topog (:355)
with filter_topo (:687) and process_topo (:551) as stages whose results stay on the device, and numpy mirrors of the two
host-side preparations (the vertical grid :383-390, the row trim :416-449).  The tool's netCDF and mosaic reading, its domain
decomposition and the idealised topographies are the caller's.  There is no CPU fallback: without a device every compute entry
raises."""
import ctypes as C

import numpy as np

from ._lib import FregridHipError, TopogOpts, check, lib, require_gpu

_dpt = C.POINTER(C.c_double)
_ipt = C.POINTER(C.c_int)
D2R = np.pi / 180                     # constant.h
NC_TYPES = {np.dtype(np.int32): 4, np.dtype(np.float32): 5, np.dtype(np.float64): 6}          # NC_INT, NC_FLOAT, NC_DOUBLE
OPTIONS = tuple(k for k, _ in TopogOpts._fields_)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return a.ctypes.data_as(_dpt)


def zw_from_zeta(zeta):
    """:383-390: the vertical grid file's zeta [nzv = 2*nk+1] -> zw [nk], zw[k] = zeta[2*(k+1)]"""
    zeta = _f64(zeta).reshape(-1)
    if (zeta.size - 1) % 2:
        raise ValueError("topog: size of dimension nzv should be 2*nk+1, where nk is the number of model vertical level")
    return zeta[2::2].copy()


def topog_source_rows(yt_deg, y_dst_deg):
    """:420-427 and :437-449 in numpy: (jstart, jend) of the source rows kept for a model grid with corner latitudes y_dst_deg"""
    yt = _f64(yt_deg).reshape(-1)
    ny = yt.size
    yc = np.empty(ny + 1)
    yc[1:ny] = (yt[:-1] + yt[1:]) * 0.5
    yc[0] = 2 * yt[0] - yc[1]
    yc[ny] = 2 * yt[ny - 1] - yc[ny - 1]
    yc = yc * D2R
    y_out = _f64(y_dst_deg).reshape(-1) * D2R
    inside = np.nonzero((yc > y_out.min()) & (yc < y_out.max()))[0]
    jstart, jend = (int(inside[0]), int(inside[-1])) if inside.size else (ny, -1)
    return max(0, jstart - 1), min(ny - 1, jend + 1)


def set_topog_sweep(fused):
    """1 (default): remove_isolated_cells for every cell at once inside the last kernel; 0: as the reference's in-place sweep, one
    launch per anti-diagonal.  Same results (test hook)."""
    lib().fg_set_topog_sweep(1 if fused else 0)


def default_options():
    """make_topog.c:297-323 as a dict"""
    o = TopogOpts()
    lib().fg_topog_default_opts(C.byref(o))
    return {k: getattr(o, k) for k in OPTIONS}


class Topog:
    """RAII wrapper of fg_topog.  x_dst, y_dst [ny+1, nx+1]: the model grid's corners in degrees; opts: any of OPTIONS
    (create_realistic_topog's switches, defaults make_topog.c's)."""

    def __init__(self, x_dst, y_dst, device=0, **opts):
        self._h = None
        bad = [k for k in opts if k not in OPTIONS]
        if bad:
            raise TypeError("unknown option(s) " + ", ".join(bad))
        x, y = _f64(x_dst), _f64(y_dst)
        if x.ndim != 2 or x.shape != y.shape or x.shape[0] < 2 or x.shape[1] < 2:
            raise ValueError("x_dst, y_dst must be [ny+1, nx+1]")
        require_gpu()
        self.ny, self.nx, self.device = x.shape[0] - 1, x.shape[1] - 1, device
        o = TopogOpts()
        lib().fg_topog_default_opts(C.byref(o))
        for k, v in opts.items():
            setattr(o, k, v)
        self.options = {k: getattr(o, k) for k in OPTIONS}
        h = C.c_void_p()
        check(lib().fg_topog_create(self.nx, self.ny, _dp(x), _dp(y), C.byref(o), device, C.byref(h)))
        self._h = h

    def destroy(self):
        if self._h is not None and self._h.value:
            lib().fg_topog_destroy(self._h)
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
        return lib().fg_topog_stream(self._h)

    def source(self, xt, yt, data, missing):
        """xt [nx_src], yt [ny_src]: the file's cell-centre axes in degrees; data [ny_src, nx_src] float32, int32 or float64, sent in
        that type; missing: the file's missing_value.  May be called again."""
        xt, yt = _f64(xt).reshape(-1), _f64(yt).reshape(-1)
        data = np.asarray(data)
        if data.dtype not in NC_TYPES:
            raise FregridHipError(-1, "topog.c: nc_type should be NC_DOUBLE, NC_FLOAT or NC_INT")
        data = np.ascontiguousarray(data)
        if data.shape != (yt.size, xt.size):
            raise ValueError(f"data must be [{yt.size}, {xt.size}], got {data.shape}")
        check(lib().fg_topog_set_source(self._h, xt.size, yt.size, _dp(xt), _dp(yt), data.ctypes.data_as(C.c_void_p), NC_TYPES[data.dtype],
                                        float(missing)))
        self._nx_src = xt.size
        return self

    def source_arrays(self):
        """what source() left on the device (tests): dict x_src, y_src [ny_now+1, nx_src+1] radians, depth_src, mask_src [ny_now, nx_src]"""
        ny_now, nx = self.stats()["ny_now"], self._nx_src
        a = dict(x_src=np.empty((ny_now + 1, nx + 1)), y_src=np.empty((ny_now + 1, nx + 1)), depth_src=np.empty((ny_now, nx)),
                 mask_src=np.empty((ny_now, nx)))
        check(lib().fg_topog_get_source(self._h, _dp(a["x_src"]), _dp(a["y_src"]), _dp(a["depth_src"]), _dp(a["mask_src"])))
        return a

    def remap(self):
        """conserve_interp / conserve_interp_great_circle of the source onto the model grid, or the on_grid copy"""
        check(lib().fg_topog_remap(self._h))
        return self

    def filter(self):
        """filter_topo with num_filter_pass passes (whatever filter_topog says)"""
        check(lib().fg_topog_filter(self._h))
        return self

    def process(self, zw):
        """process_topo on the levels zw [nk]"""
        zw = _f64(zw).reshape(-1)
        check(lib().fg_topog_process(self._h, zw.size, _dp(zw)))
        return self

    def run(self, zw=None):
        """:512-536: remap, filter if filter_topog, fill_first_row, process_topo if zw is given"""
        zw = _f64([] if zw is None else zw).reshape(-1)
        check(lib().fg_topog_run(self._h, zw.size, _dp(zw) if zw.size else None))
        return self

    def set_depth(self, a):
        """test hook: overwrite the device depth [ny, nx], e.g. with the reference's intermediate"""
        a = _f64(a)
        if a.size != self.nx * self.ny:
            raise ValueError(f"depth must be [{self.ny}, {self.nx}]")
        check(lib().fg_topog_set_depth(self._h, _dp(a)))
        return self

    def depth(self):
        out = np.empty((self.ny, self.nx))
        check(lib().fg_topog_get(self._h, _dp(out), None))
        return out

    def num_levels(self):
        out = np.empty((self.ny, self.nx), dtype=np.int32)
        check(lib().fg_topog_get(self._h, None, out.ctypes.data_as(_ipt)))
        return out

    def stats(self):
        """dict: jstart, jend, nxgrid, isolated_filled, partial_restricted, shallow_modified (the counts the reference prints under
        debug), verdict (show_deepest's: 0 deeper than the grid, 1 fewer levels would do, 2 fits, -1 no vertical grid), sweep_launches,
        ny_now, deepest (the deepest non-zero depth after the filter stage)"""
        s = (C.c_long * 9)()
        d = C.c_double()
        check(lib().fg_topog_stats(self._h, s, C.byref(d), 9))
        r = dict(zip(("jstart", "jend", "nxgrid", "isolated_filled", "partial_restricted", "shallow_modified", "verdict", "sweep_launches",
                      "ny_now"), s))
        r["deepest"] = d.value
        return r

    def phase_ms(self):
        """wall time in ms: dict create, source, remap, filter, process"""
        ms = (C.c_float * 5)()
        check(lib().fg_topog_phase_ms(self._h, ms, 5))
        return dict(zip(("create", "source", "remap", "filter", "process"), ms))


def create_realistic_topog(x_dst, y_dst, xt_src, yt_src, data, missing, zw=None, device=0, **opts):
    """create_realistic_topog in one call: (depth [ny, nx], num_levels [ny, nx] or None without a vertical grid).  x_dst, y_dst:
    model grid corners in degrees; xt_src, yt_src, data, missing: the topography file's axes, field and missing_value; zw: the
    levels (zw_from_zeta), None for no vertical grid; opts: the tool's switches (OPTIONS)."""
    with Topog(x_dst, y_dst, device=device, **opts) as h:
        h.source(xt_src, yt_src, data, missing).run(zw)
        return h.depth(), (h.num_levels() if zw is not None and np.size(zw) else None)


__all__ = ["Topog", "create_realistic_topog", "zw_from_zeta", "topog_source_rows", "default_options", "set_topog_sweep", "OPTIONS", "FregridHipError"]
