"""fregrid's --extrapolate fill and --dst_vgrid levels on the device (tools/fregrid/fregrid_util.c): a handle per source grid
(fg_extrap, include/fregrid_hip.h) and mirrors of do_extrapolate (:2662), setup_vertical_interp (:756) and do_vertical_interp
(:789).  There is no CPU fallback: without a device every compute entry raises."""
import ctypes as C

import numpy as np

from ._lib import check, lib

_dpt = C.POINTER(C.c_double)
_ipt = C.POINTER(C.c_int)
MAX_ITER = 4000                      # fregrid_util.c:39


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def set_extrap_batch(n):
    """Iterations queued per host synchronisation (test hook; < 1 restores the default).  Results never depend on it."""
    lib().fg_set_extrap_batch(int(n))


def set_extrap_coef(stored):
    """0: the kernel forms a cell's coefficients from row / column factors per use; 1: it reads a stored table.  Same results."""
    lib().fg_set_extrap_coef(1 if stored else 0)


def extrap_coef_host(lon1d, lat1d):
    """cfw, cfe, cfs, cfn [nj, ni] of do_extrapolate (:2676-2720) on the host (no device needed)."""
    lon, lat = _f64(lon1d).reshape(-1), _f64(lat1d).reshape(-1)
    out = [np.empty((lat.size, lon.size)) for _ in range(4)]
    check(lib().fg_extrap_coef_host(lon.size, lat.size, lon.ctypes.data_as(_dpt), lat.ctypes.data_as(_dpt),
                                    *[a.ctypes.data_as(_dpt) for a in out]))
    return tuple(out)


class Extrapolator:
    """RAII wrapper of fg_extrap: the grid factors of one lat-lon source grid.  lon1d [ni], lat1d [nj]: the T-cell axes in
    radians (grid_in[].lont1D / latt1D)."""

    def __init__(self, lon1d, lat1d, is_cyclic, device=0):
        lon, lat = _f64(lon1d).reshape(-1), _f64(lat1d).reshape(-1)
        h = C.c_void_p()
        self._h = None
        check(lib().fg_extrap_create(lon.size, lat.size, lon.ctypes.data_as(_dpt), lat.ctypes.data_as(_dpt),
                                     1 if is_cyclic else 0, device, C.byref(h)))
        self._h = h
        self.ni, self.nj, self.is_cyclic, self.device = lon.size, lat.size, bool(is_cyclic), device

    def destroy(self):
        if self._h is not None and self._h.value:
            lib().fg_extrap_destroy(self._h)
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
        return lib().fg_extrap_stream(self._h)

    @property
    def last_syncs(self):
        """host synchronisations of the last run's iteration loops: sum over levels of ceil((iters + 1) / batch)"""
        return int(lib().fg_extrap_last_syncs(self._h))

    def coef(self):
        """cfw, cfe, cfs, cfn [nj, ni] as the handle uses them"""
        out = [np.empty((self.nj, self.ni)) for _ in range(4)]
        check(lib().fg_extrap_get_coef(self._h, *[a.ctypes.data_as(_dpt) for a in out]))
        return tuple(out)

    def run(self, data, missing, stop_crit=0.005):
        """data [nk, nj, ni] (or [nj, ni]): a numpy array (uploaded, result downloaded) or a torch tensor on the handle's device
        (float64, contiguous; the result is a new tensor there).  Returns (out, iters [nk], resmax [nk]): iters[k] is the
        0-based iteration level k stopped after, the number the reference prints."""
        torch_in = _is_torch(data)
        shape = tuple(data.shape)
        if len(shape) not in (2, 3) or shape[-2:] != (self.nj, self.ni):
            raise ValueError(f"data must be [nk, {self.nj}, {self.ni}], got {shape}")
        nk = shape[0] if len(shape) == 3 else 1
        iters, resmax = np.empty(nk, dtype=np.int32), np.empty(nk)
        if torch_in:
            import torch
            if data.dtype != torch.float64 or not data.is_cuda or not data.is_contiguous():
                raise ValueError("a torch input must be a contiguous float64 tensor on the device")
            out = torch.empty_like(data)
            torch.cuda.current_stream(data.device).synchronize()       # the handle's stream does not wait for torch's
            check(lib().fg_extrap_run_dev(self._h, data.data_ptr(), out.data_ptr(), nk, 0, float(missing), float(stop_crit),
                                          iters.ctypes.data_as(_ipt), resmax.ctypes.data_as(_dpt)))
            return out, iters, resmax
        a = _f64(data)
        out = np.empty_like(a)
        check(lib().fg_extrap_run(self._h, a.ctypes.data_as(_dpt), out.ctypes.data_as(_dpt), nk, float(missing), float(stop_crit),
                                  iters.ctypes.data_as(_ipt), resmax.ctypes.data_as(_dpt)))
        return out, iters, resmax

    def run_batch(self, data, missing, stop_crit=0.005):
        """run() for several records in the same launches (fg_extrap_run_batch_dev): data [nrec, nk, nj, ni], a numpy array or a
        contiguous float64 torch tensor on the handle's device.  Returns (out, iters [nrec, nk], resmax [nrec, nk]); every record
        comes back as run() gives it alone."""
        shape = tuple(data.shape)
        if len(shape) != 4 or shape[-2:] != (self.nj, self.ni):
            raise ValueError(f"data must be [nrec, nk, {self.nj}, {self.ni}], got {shape}")
        nrec, nk = shape[:2]
        iters, resmax = np.empty((nrec, nk), dtype=np.int32), np.empty((nrec, nk))
        tail = (nk, 0, 0, float(missing), float(stop_crit), iters.ctypes.data_as(_ipt), resmax.ctypes.data_as(_dpt))
        if _is_torch(data):
            import torch
            if data.dtype != torch.float64 or not data.is_cuda or not data.is_contiguous():
                raise ValueError("a torch input must be a contiguous float64 tensor on the device")
            out = torch.empty_like(data)
            torch.cuda.current_stream(data.device).synchronize()       # the handle's stream does not wait for torch's
            check(lib().fg_extrap_run_batch_dev(self._h, nrec, data.data_ptr(), out.data_ptr(), *tail))
            return out, iters, resmax
        L = lib()
        a = _f64(data)
        out = np.empty_like(a)
        d = L.fg_dev_alloc(a.nbytes + 8, self.device)
        try:
            if not d:
                check(-2)
            check(L.fg_dev_upload(d, a.ctypes.data, a.nbytes))
            check(L.fg_extrap_run_batch_dev(self._h, nrec, d, d, *tail))   # in place: a level is read before it is written
            check(L.fg_dev_download(out.ctypes.data, d, out.nbytes))
        finally:
            L.fg_dev_free(d)
        return out, iters, resmax


def do_extrapolate(ni, nj, nk, lon, lat, data_in, is_cyclic, missing_value, stop_crit, verbose=True, device=0):
    """fregrid_util.c:2662 -- returns data_out [nk, nj, ni]; prints the reference's "Stopped after ..." line per level."""
    with Extrapolator(np.asarray(lon).reshape(-1)[:ni], np.asarray(lat).reshape(-1)[:nj], is_cyclic, device) as ex:
        out, iters, resmax = ex.run(_f64(data_in).reshape(nk, nj, ni), missing_value, stop_crit)
    if verbose:
        for n, r in zip(iters, resmax):
            print("Stopped after %d iterations, maxres = %g" % (n, r))
    return out


def setup_vertical_interp(z_in, z_out):
    """fregrid_util.c:756 -- (kstart, kend, need_interp) of VGrid_config; host only."""
    z1, z2 = _f64(z_in).reshape(-1), _f64(z_out).reshape(-1)
    ks, ke, need = C.c_int(), C.c_int(), C.c_int()
    check(lib().fg_setup_vertical_interp(z1.size, z1.ctypes.data_as(_dpt), z2.size, z2.ctypes.data_as(_dpt), C.byref(ks), C.byref(ke),
                                         C.byref(need)))
    return ks.value, ke.value, need.value


def do_vertical_interp(z_in, z_out, data, device=0):
    """fregrid_util.c:789 for a field with a z axis -- data [nk1, ...] -> [nk2, ...] (the input itself when need_interp is 0, as
    the reference leaves the field alone).  numpy in, numpy out; a torch device tensor in, a torch tensor out."""
    z1, z2 = _f64(z_in).reshape(-1), _f64(z_out).reshape(-1)
    shape = tuple(data.shape)
    if shape[0] != z1.size:
        raise ValueError("data's first axis must be the source levels")
    nxy = int(np.prod(shape[1:]))
    zargs = (z1.size, z1.ctypes.data_as(_dpt), z2.size, z2.ctypes.data_as(_dpt))
    if _is_torch(data):
        import torch
        if data.dtype != torch.float64 or not data.is_cuda or not data.is_contiguous():
            raise ValueError("a torch input must be a contiguous float64 tensor on the device")
        out = torch.empty((z2.size,) + shape[1:], dtype=torch.float64, device=data.device)
        torch.cuda.current_stream(data.device).synchronize()
        check(lib().fg_dev_vertical_interp(nxy, *zargs, data.data_ptr(), out.data_ptr()))
        return out
    L = lib()
    a = _f64(data)
    out = np.empty((z2.size,) + shape[1:])
    d_in = L.fg_dev_alloc(a.nbytes + 8, device)
    d_out = L.fg_dev_alloc(out.nbytes + 8, device)
    try:
        if not d_in or not d_out:
            check(-2)
        check(L.fg_dev_upload(d_in, a.ctypes.data, a.nbytes))
        check(L.fg_dev_vertical_interp(nxy, *zargs, d_in, d_out))
        check(L.fg_dev_download(out.ctypes.data, d_out, out.nbytes))
    finally:
        L.fg_dev_free(d_in)
        L.fg_dev_free(d_out)
    return out
