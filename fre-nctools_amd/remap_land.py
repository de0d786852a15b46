"""remap_land's nearest-point search on the device (tools/remap_land/remap_land.c:2520-2607): full_search_nearest and
search_nearest_sface behind a handle per source grid (fg_rland, include/fregrid_hip.h).  The maps are the reference's, bit
for bit.  The tool's data move (tile and cohort matching, the compressed gathers, netCDF) is the caller's.
There is no CPU fallback: without a device every entry raises."""
import ctypes as C

import numpy as np

from ._lib import check, lib, require_gpu

_ipt = C.POINTER(C.c_int)
_STATS = ("queries", "tiles", "tiles_visited", "tiles_visited_survivors", "survivors", "host_finished", "fallback", "overflow")
_PHASES = ("convert", "order", "queries", "tiles_balls", "phase1", "phase2", "overflow", "host_finish")


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _ip(a):
    return a.ctypes.data_as(_ipt)


def set_rland_prune(on):
    """1 (default): the search skips tiles by their bounding balls; 0: it visits every tile.  Same results (test hook)."""
    lib().fg_set_rland_prune(1 if on else 0)


def rland_tile():
    """compacted source points per tile of the search"""
    return int(lib().fg_rland_tile())


def _points(lon, lat):
    """-> (keep-alive objects, lon pointer, lat pointer, n): numpy arrays, or contiguous float64 torch tensors on the device"""
    if type(lon).__module__.split(".")[0] == "torch":
        import torch
        if type(lat).__module__.split(".")[0] != "torch" or lon.shape != lat.shape:
            raise ValueError("lon_dst and lat_dst must be tensors of one shape")
        for t in (lon, lat):
            if t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError("a torch input must be a contiguous float64 tensor")
        if lon.is_cuda:
            torch.cuda.current_stream(lon.device).synchronize()       # the handle's stream does not wait for torch's
        return (lon, lat), C.c_void_p(lon.data_ptr()), C.c_void_p(lat.data_ptr()), lon.numel()
    lon, lat = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (lon, lat))
    if lon.size != lat.size:
        raise ValueError("lon_dst and lat_dst differ in size")
    return (lon, lat), C.c_void_p(lon.ctypes.data), C.c_void_p(lat.ctypes.data), lon.size


class LandNearest:
    """RAII wrapper of fg_rland.  lon_src, lat_src [nface, npts] in radians: converted and ordered once."""

    def __init__(self, lon_src, lat_src):
        require_gpu()
        lon, lat = (np.ascontiguousarray(a, dtype=np.float64) for a in (lon_src, lat_src))
        if lon.ndim != 2 or lon.shape != lat.shape:
            raise ValueError("lon_src and lat_src must be [nface, npts]")
        self.nface, self.npts = lon.shape
        h = C.c_void_p()
        self._h = None
        dp = C.POINTER(C.c_double)
        check(lib().fg_rland_create(self.nface, self.npts, lon.ctypes.data_as(dp), lat.ctypes.data_as(dp), C.byref(h)))
        self._h = h

    def destroy(self):
        if self._h is not None and self._h.value:
            lib().fg_rland_destroy(self._h)
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
    def stream(self):
        """the hipStream_t (as an int) the handle queues its work on"""
        return lib().fg_rland_stream(self._h)

    def _mask_src(self, mask_src):
        m = _i32(mask_src)
        if m.size != self.nface * self.npts:
            raise ValueError(f"mask_src must have {self.nface} x {self.npts} entries")
        return m

    def search(self, mask_src, lon_dst, lat_dst, mask_dst, face=-1):
        """full_search_nearest: (idx_map, face_map) [npts_dst] int32, -1 where mask_dst == 0.  face >= 0: that source face only.
        lon_dst, lat_dst: numpy arrays or contiguous float64 torch tensors (host or device)."""
        ms, md = self._mask_src(mask_src), _i32(mask_dst)
        keep, plon, plat, n = _points(lon_dst, lat_dst)
        if md.size != n:
            raise ValueError("mask_dst does not match the destination points")
        idx, fmap = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        check(lib().fg_rland_search(self._h, _ip(ms), int(face), n, plon, plat, _ip(md), _ip(idx), _ip(fmap)))
        return idx, fmap

    def search_sface(self, mask_src, lon_dst, lat_dst, mask_dst, idx_map, face_map, iface_dst):
        """search_nearest_sface: idx_map_sf [npts_dst] int32: idx_map where face_map == iface_dst, else the nearest unmasked
        point of source face iface_dst; -1 where mask_dst == 0."""
        ms, md, im, fm = self._mask_src(mask_src), _i32(mask_dst), _i32(idx_map), _i32(face_map)
        keep, plon, plat, n = _points(lon_dst, lat_dst)
        if md.size != n or im.size != n or fm.size != n:
            raise ValueError("mask_dst, idx_map and face_map must match the destination points")
        out = np.empty(n, dtype=np.int32)
        check(lib().fg_rland_search_sface(self._h, _ip(ms), n, plon, plat, _ip(md), _ip(im), _ip(fm), int(iface_dst), _ip(out)))
        return out

    def stats(self):
        """of the last search call, dict: queries, tiles, tiles_visited (phase 1, over all queries), tiles_visited_survivors
        (phase 2), survivors, host_finished, fallback, overflow"""
        s = (C.c_long * len(_STATS))()
        check(lib().fg_rland_stats(self._h, s, len(_STATS)))
        return dict(zip(_STATS, s))

    def phase_ms(self):
        """wall time in ms, dict: convert, order (create); queries, tiles_balls, phase1, phase2, overflow, host_finish (last search call)"""
        ms = (C.c_float * len(_PHASES))()
        check(lib().fg_rland_phase_ms(self._h, ms, len(_PHASES)))
        return dict(zip(_PHASES, ms))
