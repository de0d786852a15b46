"""Bilinear cubed-sphere -> lat-lon regridding (fregrid --interp_method bilinear; tools/fregrid/bilinear_interp.c):
a device-resident plan (fg_bilin, include/fregrid_hip.h) and mirrors of setup_bilinear_interp,
do_scalar_bilinear_interp and do_vector_bilinear_interp.  There is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import check, lib
from .conserve_interp import READ, WRITE

_dpt = C.POINTER(C.c_double)
_ipt = C.POINTER(C.c_int)
_CONTACT_KEYS = ["tile1", "tile2", "istart1", "iend1", "jstart1", "jend1", "istart2", "iend2", "jstart2", "jend2"]


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def fine_shape(nlon, nlat, finer_step):
    """(nlat_fine, nlon_fine) of get_output_grid_by_size (fregrid_util.c:575-576)"""
    return (2 ** finer_step) * (nlat - 1) + 1, (2 ** finer_step) * nlon


def fine_grid(nlon, nlat, finer_step=0, lonbegin=0.0, lonend=360.0, latbegin=-90.0, latend=90.0, center_y=False):
    """The fine target points (radians): lont, latt [nlat_fine, nlon_fine] and latt1D_fine [nlat_fine]."""
    ny, nx = fine_shape(nlon, nlat, finer_step)
    lo, la, l1 = np.empty(nx * ny), np.empty(nx * ny), np.empty(ny)
    lib().fg_bilin_fine_grid(nlon, nlat, finer_step, lonbegin, lonend, latbegin, latend, 1 if center_y else 0,
                             lo.ctypes.data_as(_dpt), la.ctypes.data_as(_dpt), l1.ctypes.data_as(_dpt))
    return lo.reshape(ny, nx), la.reshape(ny, nx), l1


def unit_vect_latlon(lon, lat):
    """unit_vect_latlon (mosaic_util.c:937) with the host libm: vlon, vlat [..., 3]"""
    lon, lat = _f64(lon).reshape(-1), _f64(lat).reshape(-1)
    vlo, vla = np.empty(3 * lon.size), np.empty(3 * lon.size)
    lib().fg_unit_vect_latlon(lon.size, lon.ctypes.data_as(_dpt), lat.ctypes.data_as(_dpt), vlo.ctypes.data_as(_dpt),
                              vla.ctypes.data_as(_dpt))
    return vlo.reshape(-1, 3), vla.reshape(-1, 3)


def write_bilinear_remap_file(path, nlon_fine, nlat_fine, index, weight):
    """setup_bilinear_interp's WRITE branch (bilinear_interp.c:408-426): index [n, 3] int32, weight [n, 4]"""
    index = np.ascontiguousarray(index, dtype=np.int32)
    weight = _f64(weight)
    n = nlon_fine * nlat_fine
    if index.size != 3 * n or weight.size != 4 * n:
        raise ValueError("index / weight do not match the fine grid")
    check(lib().fg_bilin_remap_write(os.fsencode(path), nlon_fine, nlat_fine, index.ctypes.data_as(_ipt), weight.ctypes.data_as(_dpt)))


def read_bilinear_remap_file(path, nlon_fine, nlat_fine):
    """The READ branch (bilinear_interp.c:110-125): (index [n, 3], weight [n, 4]); a size mismatch raises."""
    n = nlon_fine * nlat_fine
    index, weight = np.empty((n, 3), dtype=np.int32), np.empty((n, 4))
    check(lib().fg_bilin_remap_read(os.fsencode(path), nlon_fine, nlat_fine, index.ctypes.data_as(_ipt), weight.ctypes.data_as(_dpt)))
    return index, weight


class BilinearPlan:
    """RAII wrapper of fg_bilin.  lont / latt: six [N, N] arrays of T-cell centres (radians); contacts: the 12 contacts as
    c2l.find_contacts returns them.  The target is get_output_grid_by_size's (degrees).  index / weight given: the READ
    branch, no search."""

    def __init__(self, lont, latt, contacts, nlon, nlat, finer_step=0, lonbegin=0.0, lonend=360.0, latbegin=-90.0,
                 latend=90.0, center_y=False, index=None, weight=None, device=0):
        _lib.require_gpu()
        nt = len(lont)
        keep = [[_f64(a).reshape(-1) for a in arrs] for arrs in (lont, latt)]
        ptrs = [(_dpt * nt)(*[a.ctypes.data_as(_dpt) for a in arrs]) for arrs in keep]
        nx = [int(np.asarray(a).shape[-1]) for a in lont]
        ny = [int(np.asarray(a).shape[-2]) if np.asarray(a).ndim > 1 else nx[k] for k, a in enumerate(lont)]
        c = {k: np.ascontiguousarray(contacts[k], dtype=np.int32) for k in _CONTACT_KEYS}
        args = [nt, (C.c_int * nt)(*nx), (C.c_int * nt)(*ny), *ptrs, len(c["tile1"]), *[c[k].ctypes.data_as(_ipt) for k in _CONTACT_KEYS],
                nlon, nlat, finer_step, lonbegin, lonend, latbegin, latend, 1 if center_y else 0]
        h = C.c_void_p()
        if index is None:
            check(lib().fg_bilin_create(*args, device, C.byref(h)))
        else:
            index = np.ascontiguousarray(index, dtype=np.int32)
            weight = _f64(weight)
            check(lib().fg_bilin_create_from_weights(*args, index.ctypes.data_as(_ipt), weight.ctypes.data_as(_dpt), device,
                                                     C.byref(h)))
        self._h = h
        self._stream = None
        self.device = device
        self.nlon, self.nlat, self.finer_step = nlon, nlat, finer_step
        self.nlon_fine = int(lib().fg_bilin_nlon_fine(h))
        self.nlat_fine = int(lib().fg_bilin_nlat_fine(h))
        self.npoints_fine = int(lib().fg_bilin_npoints_fine(h))
        self.ncells = int(lib().fg_bilin_ncells(h))
        # search comparisons the host libm's rounding could have ordered otherwise (fg_bilin_ambiguous_ties)
        self.ambiguous_ties = int(lib().fg_bilin_ambiguous_ties(h))

    def destroy(self):
        if self._h is not None and self._h.value:
            lib().fg_bilin_destroy(self._h)
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

    def index_weight(self):
        """Interp_config.index [n, 3] (ic, jc, tile) and .weight [n, 4] on the fine grid, host copies"""
        index, weight = np.empty((self.npoints_fine, 3), dtype=np.int32), np.empty((self.npoints_fine, 4))
        check(lib().fg_bilin_get_index_weight(self._h, index.ctypes.data_as(_ipt), weight.ctypes.data_as(_dpt)))
        return index, weight

    def write_remap(self, path):
        index, weight = self.index_weight()
        write_bilinear_remap_file(path, self.nlon_fine, self.nlat_fine, index, weight)

    def set_stream(self, stream):
        check(lib().fg_bilin_set_stream(self._h, C.c_void_p(int(stream))))

    def sync(self):
        check(lib().fg_bilin_sync(self._h))

    def sweep(self, in_dtype=np.float64, out_dtype=np.float64):
        """field_io.BilinearSweep over this plan: levels streamed from host arrays in the file's type (fg_bilin_sweep)"""
        from .field_io import BilinearSweep
        return BilinearSweep(self, in_dtype, out_dtype)

    def _levels(self, t):
        import torch
        st = torch.cuda.current_stream(self.device).cuda_stream      # the applies run on the caller's current stream
        if st != self._stream:
            self.set_stream(st)
            self._stream = st
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t, dtype=np.float64))
        t = t.to(device=f"cuda:{self.device}", dtype=torch.float64).contiguous()
        if t.numel() % self.ncells:
            raise ValueError(f"field size {t.numel()} is not a multiple of 6*N*N = {self.ncells}")
        return t.reshape(-1, self.ncells)

    def apply_scalar(self, src, has_missing=False, missing=0.0, fill_missing=False, out=None):
        """src [nz, 6*N*N] (device tensor or host array) -> [nz, nlat, nlon] device tensor"""
        import torch
        src = self._levels(src)
        nz = src.shape[0]
        if out is None:
            out = torch.empty((nz, self.nlat, self.nlon), dtype=torch.float64, device=src.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != src.device
              or not out.is_contiguous() or out.numel() != nz * self.nlat * self.nlon):
            raise ValueError(f"out must be a contiguous float64 tensor of {nz * self.nlat * self.nlon} elements on {src.device}")
        check(lib().fg_bilin_apply_scalar(self._h, C.c_void_p(src.data_ptr()), nz, 1 if has_missing else 0, float(missing),
                                          1 if fill_missing else 0, C.c_void_p(out.data_ptr())))
        return out

    def apply_vector(self, u, v, has_missing=False, missing=0.0, fill_missing=False):
        """u, v [nz, 6*N*N] -> (u_out, v_out) [nz, nlat, nlon] device tensors"""
        import torch
        u, v = self._levels(u), self._levels(v)
        if u.shape != v.shape:
            raise ValueError("u and v differ in shape")
        nz = u.shape[0]
        uo = torch.empty((nz, self.nlat, self.nlon), dtype=torch.float64, device=u.device)
        vo = torch.empty_like(uo)
        check(lib().fg_bilin_apply_vector(self._h, C.c_void_p(u.data_ptr()), C.c_void_p(v.data_ptr()), nz, 1 if has_missing else 0,
                                          float(missing), 1 if fill_missing else 0, C.c_void_p(uo.data_ptr()),
                                          C.c_void_p(vo.data_ptr())))
        return uo, vo


def setup_bilinear_interp(lont, latt, contacts, nlon, nlat, opcode=0, remap_file=None, finer_step=0, lonbegin=0.0, lonend=360.0,
                          latbegin=-90.0, latend=90.0, center_y=False, device=0):
    """setup_bilinear_interp (bilinear_interp.c:72-434) with fregrid.c's span arguments (:944-963) derived inside.
    opcode & READ with an existing remap_file: index / weight from the file; opcode & WRITE: the file is written."""
    ny, nx = fine_shape(nlon, nlat, finer_step)
    kw = dict(finer_step=finer_step, lonbegin=lonbegin, lonend=lonend, latbegin=latbegin, latend=latend, center_y=center_y,
              device=device)
    if (opcode & READ) and remap_file and os.path.exists(remap_file):
        index, weight = read_bilinear_remap_file(remap_file, nx, ny)
        return BilinearPlan(lont, latt, contacts, nlon, nlat, index=index, weight=weight, **kw)
    plan = BilinearPlan(lont, latt, contacts, nlon, nlat, **kw)
    if opcode & WRITE:
        if not remap_file:
            raise ValueError("WRITE needs remap_file")
        plan.write_remap(remap_file)
    return plan


def do_scalar_bilinear_interp(plan, data, has_missing=False, missing=0.0, fill_missing=False):
    """do_scalar_bilinear_interp (:436-468) for nz levels at once: data [nz, 6*N*N] -> numpy [nz, nlat, nlon]"""
    return plan.apply_scalar(data, has_missing, missing, fill_missing).cpu().numpy()


def do_vector_bilinear_interp(plan, u, v, has_missing=False, missing=0.0, fill_missing=False):
    """do_vector_bilinear_interp (:476-560): (u_out, v_out) numpy [nz, nlat, nlon]"""
    uo, vo = plan.apply_vector(u, v, has_missing, missing, fill_missing)
    return uo.cpu().numpy(), vo.cpu().numpy()
