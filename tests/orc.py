"""ctypes access to the CPU checkers used by the tests (never by the product):

* ``oracle/liboracle.so``       our clean-room C restatement (oracle/xgrid_oracle.c); gc_oracle.c is in it twice, plain
  (libm's acosl, pinned to the reference) and as orc_*_cr (the device's correctly rounded arc cosine): ``cr=True`` below
* ``oracle/_ref/libfrenc_ref.so`` the reference's own sources compiled in place (oracle/Makefile);
  present in the build container and -- as a prebuilt .so -- on the GPU box.
* ``oracle/_ref/libconserve_ref.so`` the reference's own conserve_interp.c (setup_conserve_interp,
  do_scalar_conserve_interp) behind oracle/conserve_ref_adapter.c, built the same way.
* ``oracle/_ref/libbilinear_ref.so`` the reference's own bilinear_interp.c (setup_bilinear_interp,
  do_scalar_bilinear_interp, do_vector_bilinear_interp) behind oracle/bilinear_ref_adapter.c, built the same way.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
lp = C.POINTER(C.c_long)


def _dp(a):
    return a.ctypes.data_as(dp) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(ip) if a is not None else None


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


_ORACLE = None
_REF = None
_CREF = None
_BREF = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        path = os.path.join(ORACLE_DIR, "liboracle.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", ORACLE_DIR, "liboracle.so"], stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.orc_fix_lon.argtypes = [dp, dp, C.c_int, C.c_double]
        L.orc_fix_lon.restype = C.c_int
        L.orc_poly_area.argtypes = [dp, dp, C.c_int]
        L.orc_poly_area.restype = C.c_double
        L.orc_poly_ctrlon.argtypes = [dp, dp, C.c_int, C.c_double]
        L.orc_poly_ctrlon.restype = C.c_double
        L.orc_poly_ctrlat.argtypes = [dp, dp, C.c_int]
        L.orc_poly_ctrlat.restype = C.c_double
        L.orc_clip_2dx2d.argtypes = [dp, dp, C.c_int, dp, dp, C.c_int, dp, dp]
        L.orc_clip_2dx2d.restype = C.c_int
        L.orc_get_grid_area.argtypes = [C.c_int, C.c_int, dp, dp, dp]
        L.orc_get_grid_area.restype = None
        L.orc_create_xgrid_2dx2d_rows.argtypes = [C.c_int] * 5 + [dp] * 5 + [C.c_int, C.c_int, C.c_long] + [ip] * 4 + [dp] * 3
        L.orc_create_xgrid_2dx2d_rows.restype = C.c_long
        L.orc_get_grid_cell_struct.argtypes = [C.c_int, C.c_int, dp, dp] + [dp] * 5 + [ip] + [dp] * 3
        L.orc_get_grid_cell_struct.restype = C.c_int
        dpp = C.POINTER(dp)
        ipp = C.POINTER(ip)
        L.orc_setup_conserve_interp.argtypes = [C.c_int, C.c_int, ip, ip, dpp, dpp, dpp, C.c_int, ip, ip, dpp, dpp,
                                                C.c_long, lp] + [ip] * 5 + [dp] * 3
        L.orc_setup_conserve_interp.restype = C.c_long
        L.orc_do_scalar_conserve_interp.argtypes = [C.c_int, C.c_long] + [ip] * 5 + [dp] * 3 + [C.c_int, ip, ip,
                                                    dpp, dpp, dpp, ipp, C.c_int, C.c_double, C.c_int, C.c_int,
                                                    C.c_int, dp, dp]
        L.orc_do_scalar_conserve_interp.restype = C.c_int
        L.orc_do_scalar_conserve_interp_ex.argtypes = [C.c_int, C.c_long] + [ip] * 5 + [dp] * 3 + [C.c_int, ip, ip,
                                                       dpp, dpp, dpp, ipp, C.c_int, C.c_double, dpp, C.c_int, dpp,
                                                       C.c_double, dpp, C.c_int, dp, C.c_int, C.c_int, C.c_int,
                                                       C.c_int, dp, dp]
        L.orc_do_scalar_conserve_interp_ex.restype = C.c_int
        L.orc_gsum_in_ex.argtypes = [C.c_int, C.c_int, ip, ip, dpp, dpp, dpp, C.c_int, C.c_int, C.c_double, C.c_int]
        L.orc_gsum_in_ex.restype = C.c_double
        L.orc_gsum_in.argtypes = [C.c_int, C.c_int, ip, ip, dpp, dpp, C.c_int, C.c_double, C.c_int]
        L.orc_gsum_in.restype = C.c_double
        L.orc_clip_2dx2d_great_circle.argtypes = [dp, dp, dp, C.c_int, dp, dp, dp, C.c_int, dp, dp, dp]
        L.orc_clip_2dx2d_great_circle.restype = C.c_int
        L.orc_great_circle_area.argtypes = [C.c_int, dp, dp, dp]
        L.orc_great_circle_area.restype = C.c_double
        L.orc_get_grid_great_circle_area.argtypes = [C.c_int, C.c_int, dp, dp, dp]
        L.orc_get_grid_great_circle_area.restype = None
        L.orc_latlon2xyz.argtypes = [C.c_int, dp, dp, dp, dp, dp]
        L.orc_latlon2xyz.restype = None
        L.orc_create_xgrid_great_circle_rows.argtypes = [C.c_int] * 4 + [dp] * 5 + [C.c_int, C.c_int, C.c_long] + [ip] * 4 + [dp] * 3
        L.orc_create_xgrid_great_circle_rows.restype = C.c_long
        L.orc_spherical_angle.argtypes = [dp, dp, dp]
        L.orc_spherical_angle.restype = C.c_double
        # gc_oracle.c's second build: the same text with the device's arc cosine (csrc/fp80.h's fg_acosl)
        for nm in ("orc_clip_2dx2d_great_circle", "orc_great_circle_area", "orc_get_grid_great_circle_area",
                   "orc_create_xgrid_great_circle_rows", "orc_spherical_angle"):
            getattr(L, nm + "_cr").argtypes = getattr(L, nm).argtypes
            getattr(L, nm + "_cr").restype = getattr(L, nm).restype
        L.orc_clip.argtypes = [dp, dp, C.c_int] + [C.c_double] * 4 + [dp, dp]
        L.orc_clip.restype = C.c_int
        L.orc_box_ctrlat.argtypes = [C.c_double] * 4
        L.orc_box_ctrlat.restype = C.c_double
        L.orc_box_ctrlon.argtypes = [C.c_double] * 5
        L.orc_box_ctrlon.restype = C.c_double
        L.orc_get_grid_area_no_adjust.argtypes = [C.c_int, C.c_int, dp, dp, dp]
        L.orc_get_grid_area_no_adjust.restype = None
        L.orc_create_xgrid_box.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, dp, dp, dp, C.c_long] + [ip] * 4 + [dp] * 3
        L.orc_create_xgrid_box.restype = C.c_long
        _ORACLE = L
    return _ORACLE


def ref_available():
    return os.path.exists(os.path.join(ORACLE_DIR, "_ref", "libfrenc_ref.so"))


def ref():
    """The compiled reference (unmodified sources).  None if it has not been built."""
    global _REF
    if _REF is None:
        path = os.path.join(ORACLE_DIR, "_ref", "libfrenc_ref.so")
        if not os.path.exists(path):
            return None
        L = C.CDLL(path)
        cip = C.POINTER(C.c_int)
        L.fix_lon.argtypes = [dp, dp, C.c_int, C.c_double]
        L.fix_lon.restype = C.c_int
        L.poly_area.argtypes = [dp, dp, C.c_int]
        L.poly_area.restype = C.c_double
        L.poly_ctrlon.argtypes = [dp, dp, C.c_int, C.c_double]
        L.poly_ctrlon.restype = C.c_double
        L.poly_ctrlat.argtypes = [dp, dp, C.c_int]
        L.poly_ctrlat.restype = C.c_double
        L.clip_2dx2d.argtypes = [dp, dp, C.c_int, dp, dp, C.c_int, dp, dp]
        L.clip_2dx2d.restype = C.c_int
        L.get_grid_area.argtypes = [cip, cip, dp, dp, dp]
        L.get_grid_area.restype = None
        L.create_xgrid_2dx2d_order1.argtypes = [cip] * 4 + [dp] * 5 + [ip] * 4 + [dp]
        L.create_xgrid_2dx2d_order1.restype = C.c_int
        L.create_xgrid_2dx2d_order2.argtypes = [cip] * 4 + [dp] * 5 + [ip] * 4 + [dp] * 3
        L.create_xgrid_2dx2d_order2.restype = C.c_int
        L.conserve_interp.argtypes = [C.c_int] * 4 + [dp] * 7
        L.conserve_interp.restype = None
        L.conserve_interp_great_circle.argtypes = [C.c_int] * 4 + [dp] * 7
        L.conserve_interp_great_circle.restype = None
        L.clip_2dx2d_great_circle.argtypes = [dp, dp, dp, C.c_int, dp, dp, dp, C.c_int, dp, dp, dp]
        L.clip_2dx2d_great_circle.restype = C.c_int
        L.great_circle_area.argtypes = [C.c_int, dp, dp, dp]
        L.great_circle_area.restype = C.c_double
        L.get_grid_great_circle_area.argtypes = [cip, cip, dp, dp, dp]
        L.get_grid_great_circle_area.restype = None
        L.create_xgrid_great_circle.argtypes = [cip] * 4 + [dp] * 5 + [ip] * 4 + [dp] * 3
        L.create_xgrid_great_circle.restype = C.c_int
        L.clip.argtypes = [dp, dp, C.c_int] + [C.c_double] * 4 + [dp, dp]
        L.clip.restype = C.c_int
        L.box_ctrlat.argtypes = [C.c_double] * 4
        L.box_ctrlat.restype = C.c_double
        L.box_ctrlon.argtypes = [C.c_double] * 5
        L.box_ctrlon.restype = C.c_double
        L.get_grid_area_no_adjust.argtypes = [cip, cip, dp, dp, dp]
        L.get_grid_area_no_adjust.restype = None
        for nm in ("create_xgrid_1dx2d_order1", "create_xgrid_2dx1d_order1"):
            getattr(L, nm).argtypes = [cip] * 4 + [dp] * 5 + [ip] * 4 + [dp]
            getattr(L, nm).restype = C.c_int
        for nm in ("create_xgrid_1dx2d_order2", "create_xgrid_2dx1d_order2"):
            getattr(L, nm).argtypes = [cip] * 4 + [dp] * 5 + [ip] * 4 + [dp] * 3
            getattr(L, nm).restype = C.c_int
        _REF = L
    return _REF


# ------------------------------------------------------------------------------ wrappers
def orc_create_xgrid(order, nx1, ny1, nx2, ny2, lon_in, lat_in, lon_out, lat_out, mask=None,
                     j1_beg=0, j1_end=None, capacity=None):
    L = oracle()
    lon_in, lat_in, lon_out, lat_out = f64(lon_in).ravel(), f64(lat_in).ravel(), f64(lon_out).ravel(), f64(lat_out).ravel()
    mask = f64(np.ones(nx1 * ny1) if mask is None else mask).ravel()
    cap = capacity or 8 * (nx1 * ny1 + nx2 * ny2) + 1024
    ii, ji, io, jo = (np.empty(cap, dtype=np.int32) for _ in range(4))
    a = np.empty(cap)
    cl = np.empty(cap) if order == 2 else None
    ct = np.empty(cap) if order == 2 else None
    n = L.orc_create_xgrid_2dx2d_rows(order, nx1, ny1, nx2, ny2, _dp(lon_in), _dp(lat_in), _dp(lon_out), _dp(lat_out),
                                      _dp(mask), j1_beg, ny1 if j1_end is None else j1_end, cap,
                                      _ip(ii), _ip(ji), _ip(io), _ip(jo), _dp(a), _dp(cl), _dp(ct))
    if n < 0:
        raise RuntimeError(f"oracle create_xgrid failed: {n}")
    out = dict(n=int(n), i_in=ii[:n].copy(), j_in=ji[:n].copy(), i_out=io[:n].copy(), j_out=jo[:n].copy(), area=a[:n].copy())
    if order == 2:
        out["clon"], out["clat"] = cl[:n].copy(), ct[:n].copy()
    return out


def ref_create_xgrid(order, nx1, ny1, nx2, ny2, lon_in, lat_in, lon_out, lat_out, mask=None):
    L = ref()
    lon_in, lat_in, lon_out, lat_out = f64(lon_in).ravel(), f64(lat_in).ravel(), f64(lon_out).ravel(), f64(lat_out).ravel()
    mask = f64(np.ones(nx1 * ny1) if mask is None else mask).ravel()
    cap = 5000000        # MAXXGRID of the serial build: the reference aborts (exit) beyond it
    ii, ji, io, jo = (np.empty(cap, dtype=np.int32) for _ in range(4))
    a = np.empty(cap)
    args = [C.byref(C.c_int(nx1)), C.byref(C.c_int(ny1)), C.byref(C.c_int(nx2)), C.byref(C.c_int(ny2)),
            _dp(lon_in), _dp(lat_in), _dp(lon_out), _dp(lat_out), _dp(mask), _ip(ii), _ip(ji), _ip(io), _ip(jo), _dp(a)]
    if order == 1:
        n = L.create_xgrid_2dx2d_order1(*args)
        return dict(n=n, i_in=ii[:n].copy(), j_in=ji[:n].copy(), i_out=io[:n].copy(), j_out=jo[:n].copy(), area=a[:n].copy())
    cl, ct = np.empty(cap), np.empty(cap)
    n = L.create_xgrid_2dx2d_order2(*args, _dp(cl), _dp(ct))
    return dict(n=n, i_in=ii[:n].copy(), j_in=ji[:n].copy(), i_out=io[:n].copy(), j_out=jo[:n].copy(), area=a[:n].copy(),
                clon=cl[:n].copy(), clat=ct[:n].copy())


def orc_get_grid_area(nx, ny, lon, lat):
    lon, lat = f64(lon).ravel(), f64(lat).ravel()
    a = np.empty(nx * ny)
    oracle().orc_get_grid_area(nx, ny, _dp(lon), _dp(lat), _dp(a))
    return a


def ref_get_grid_area(nx, ny, lon, lat):
    lon, lat = f64(lon).ravel(), f64(lat).ravel()
    a = np.empty(nx * ny)
    ref().get_grid_area(C.byref(C.c_int(nx)), C.byref(C.c_int(ny)), _dp(lon), _dp(lat), _dp(a))
    return a


def orc_cell_struct(nx, ny, lon, lat):
    lon, lat = f64(lon).ravel(), f64(lat).ravel()
    n = nx * ny
    d = {k: np.empty(n) for k in ("lat_min", "lat_max", "lon_min", "lon_max", "lon_avg", "area")}
    nv = np.empty(n, dtype=np.int32)
    vlon, vlat = np.empty((n, 8)), np.empty((n, 8))
    rc = oracle().orc_get_grid_cell_struct(nx, ny, _dp(lon), _dp(lat), _dp(d["lat_min"]), _dp(d["lat_max"]),
                                           _dp(d["lon_min"]), _dp(d["lon_max"]), _dp(d["lon_avg"]), _ip(nv),
                                           _dp(vlon), _dp(vlat), _dp(d["area"]))
    assert rc == 0
    d.update(nvert=nv, vlon=vlon, vlat=vlat)
    return d


def _ptr_array(arrs, typ=dp):
    return (typ * len(arrs))(*[a.ctypes.data_as(typ) for a in arrs])


def orc_setup(order, grids_in, grids_out, capacity=None):
    """grids_*: lists of (nx, ny, lon, lat).  Returns dict of concatenated exchange cells + xoff."""
    L = oracle()
    nt, no = len(grids_in), len(grids_out)
    lon_in = [f64(g[2]).ravel() for g in grids_in]
    lat_in = [f64(g[3]).ravel() for g in grids_in]
    lon_out = [f64(g[2]).ravel() for g in grids_out]
    lat_out = [f64(g[3]).ravel() for g in grids_out]
    ca = [orc_get_grid_area(g[0], g[1], g[2], g[3]) for g in grids_in]
    nx_in = np.array([g[0] for g in grids_in], dtype=np.int32)
    ny_in = np.array([g[1] for g in grids_in], dtype=np.int32)
    nx_out = np.array([g[0] for g in grids_out], dtype=np.int32)
    ny_out = np.array([g[1] for g in grids_out], dtype=np.int32)
    cap = capacity or 4 * (int(np.sum(nx_in * ny_in)) + int(np.sum(nx_out * ny_out))) * no + 1024
    xoff = np.zeros(no + 1, dtype=np.int64)
    t, ii, ji, io, jo = (np.empty(cap, dtype=np.int32) for _ in range(5))
    a, di, dj = np.empty(cap), np.empty(cap), np.empty(cap)
    n = L.orc_setup_conserve_interp(order, nt, _ip(nx_in), _ip(ny_in), _ptr_array(lon_in), _ptr_array(lat_in),
                                    _ptr_array(ca), no, _ip(nx_out), _ip(ny_out), _ptr_array(lon_out),
                                    _ptr_array(lat_out), cap, xoff.ctypes.data_as(lp),
                                    _ip(t), _ip(ii), _ip(ji), _ip(io), _ip(jo), _dp(a), _dp(di), _dp(dj))
    if n < 0:
        raise RuntimeError(f"oracle setup failed: {n}")
    out = dict(n=int(n), xoff=xoff, t_in=t[:n].copy(), i_in=ii[:n].copy(), j_in=ji[:n].copy(), i_out=io[:n].copy(),
               j_out=jo[:n].copy(), area=a[:n].copy(), cell_area_in=ca)
    if order == 2:
        out["di"], out["dj"] = di[:n].copy(), dj[:n].copy()
    return out


def orc_apply(order, x, nx_in, ny_in, data, grad_x, grad_y, grad_mask, has_missing, missing, nx2, ny2, nz):
    """x: dict with t_in,i_in,j_in,i_out,j_out,area(,di,dj) for ONE destination tile; data etc.: per-tile lists."""
    L = oracle()
    n = len(x["area"])
    nxi = np.asarray(nx_in, dtype=np.int32)
    nyi = np.asarray(ny_in, dtype=np.int32)
    data = [f64(d).ravel() for d in data]
    gx = [f64(g).ravel() for g in grad_x] if grad_x is not None else None
    gy = [f64(g).ravel() for g in grad_y] if grad_y is not None else None
    gm = [np.ascontiguousarray(g, dtype=np.int32).ravel() for g in grad_mask] if grad_mask is not None else None
    out = np.empty(nz * nx2 * ny2)
    gs = C.c_double(0)
    ints = [np.ascontiguousarray(x[k], dtype=np.int32) for k in ("t_in", "i_in", "j_in", "i_out", "j_out")]
    area = f64(x["area"])
    di = f64(x["di"]) if order == 2 else None
    dj = f64(x["dj"]) if order == 2 else None
    rc = L.orc_do_scalar_conserve_interp(order, n, *[_ip(v) for v in ints], _dp(area), _dp(di), _dp(dj),
                                         len(data), _ip(nxi), _ip(nyi), _ptr_array(data),
                                         _ptr_array(gx) if gx else None, _ptr_array(gy) if gy else None,
                                         _ptr_array(gm, ip) if gm else None,
                                         1 if has_missing else 0, float(missing), nx2, ny2, nz, _dp(out), C.byref(gs))
    assert rc == 0
    return out, gs.value


def orc_apply_ex(order, x, nx_in, ny_in, data, grad_x, grad_y, grad_mask, has_missing, missing, nx2, ny2, nz,
                 weight=None, cell_methods_sum=False, field_area=None, area_missing=-1e20, cell_area_in=None,
                 target_grid=False, cell_area_out=None, monotonic=False):
    """All branches of do_scalar_conserve_interp (orc_do_scalar_conserve_interp_ex).  Returns (rc, out, gsum)."""
    L = oracle()
    n = len(x["area"])
    nxi = np.asarray(nx_in, dtype=np.int32)
    nyi = np.asarray(ny_in, dtype=np.int32)
    lst = lambda v: [f64(d).ravel() for d in v] if v is not None else None
    data, gx, gy, w, fa, ca = lst(data), lst(grad_x), lst(grad_y), lst(weight), lst(field_area), lst(cell_area_in)
    gm = [np.ascontiguousarray(g, dtype=np.int32).ravel() for g in grad_mask] if grad_mask is not None else None
    cao = f64(cell_area_out).ravel() if cell_area_out is not None else None
    out = np.empty(nz * nx2 * ny2)
    gs = C.c_double(0)
    ints = [np.ascontiguousarray(x[k], dtype=np.int32) for k in ("t_in", "i_in", "j_in", "i_out", "j_out")]
    area = f64(x["area"])
    di = f64(x["di"]) if order == 2 else None
    dj = f64(x["dj"]) if order == 2 else None
    pa = lambda v, t=dp: _ptr_array(v, t) if v else None
    rc = L.orc_do_scalar_conserve_interp_ex(order, n, *[_ip(v) for v in ints], _dp(area), _dp(di), _dp(dj),
                                            len(data), _ip(nxi), _ip(nyi), pa(data), pa(gx), pa(gy), pa(gm, ip),
                                            1 if has_missing else 0, float(missing), pa(w),
                                            1 if cell_methods_sum else 0, pa(fa), float(area_missing), pa(ca),
                                            1 if target_grid else 0, _dp(cao), 1 if monotonic else 0,
                                            nx2, ny2, nz, _dp(out), C.byref(gs))
    return rc, out, gs.value


# orc_do_scalar_conserve_interp_ex's error codes -> the message of the reference's fatal check (conserve_interp.c)
ORC_APPLY_ERRORS = {
    -1: "conserve_interp: has_missing should be false when nz > 1",
    -5: "conserve_interp: cell_measures should be false when nz > 1",
    -6: "conserve_interp: cell_methods should not be sum when nz > 1",
    -2: "conserve_interp: data is not missing but area is missing",
    -3: " xdata is greater than f_bar_max ",
    -4: " xdata is less than f_bar_min ",
}


def _gc(name, cr):
    """gc_oracle.c's function `name`: the plain build (libm's acosl, pinned to the reference) or, with cr, the build whose
    arc cosine is the device's correctly rounded fg_acosl"""
    return getattr(oracle(), name + ("_cr" if cr else ""))


def orc_spherical_angle(v1, v2, v3, cr=False):
    return _gc("orc_spherical_angle", cr)(_dp(f64(v1)), _dp(f64(v2)), _dp(f64(v3)))


def orc_great_circle_area(x, y, z, cr=False):
    x, y, z = f64(x), f64(y), f64(z)
    return _gc("orc_great_circle_area", cr)(len(x), _dp(x), _dp(y), _dp(z))


def orc_clip_gc(a, b, cr=False):
    """clip_2dx2d_great_circle of two polygons given as [n, 3] unit vectors: (n_out, vertices [n_out, 3])"""
    a, b = f64(a), f64(b)
    aa = [np.ascontiguousarray(a[:, ax]) for ax in range(3)]
    bb = [np.ascontiguousarray(b[:, ax]) for ax in range(3)]
    oo = [np.zeros(50) for _ in range(3)]
    n = _gc("orc_clip_2dx2d_great_circle", cr)(*[_dp(v) for v in aa], len(a), *[_dp(v) for v in bb], len(b), *[_dp(v) for v in oo])
    return n, np.stack([v[:max(n, 0)] for v in oo], axis=1)


def orc_create_xgrid_gc(nx1, ny1, nx2, ny2, lon_in, lat_in, lon_out, lat_out, mask=None, j1_beg=0, j1_end=None, capacity=None,
                        cr=False):
    """create_xgrid_great_circle (oracle restatement); source rows [j1_beg, j1_end).  cr: the build that rounds like the device."""
    L = oracle()
    lon_in, lat_in, lon_out, lat_out = f64(lon_in).ravel(), f64(lat_in).ravel(), f64(lon_out).ravel(), f64(lat_out).ravel()
    mask = f64(np.ones(nx1 * ny1) if mask is None else mask).ravel()
    cap = capacity or 8 * (nx1 * ny1 + nx2 * ny2) + 1024
    ii, ji, io, jo = (np.empty(cap, dtype=np.int32) for _ in range(4))
    a, cl, ct = np.empty(cap), np.empty(cap), np.empty(cap)
    n = _gc("orc_create_xgrid_great_circle_rows", cr)(nx1, ny1, nx2, ny2, _dp(lon_in), _dp(lat_in), _dp(lon_out), _dp(lat_out),
                                                      _dp(mask), j1_beg, ny1 if j1_end is None else j1_end, cap,
                                                      _ip(ii), _ip(ji), _ip(io), _ip(jo), _dp(a), _dp(cl), _dp(ct))
    if n < 0:
        raise RuntimeError(f"oracle create_xgrid_great_circle failed: {n}")
    return dict(n=int(n), i_in=ii[:n].copy(), j_in=ji[:n].copy(), i_out=io[:n].copy(), j_out=jo[:n].copy(), area=a[:n].copy())


def orc_gc_pair_areas(nx1, lon_in, lat_in, nx2, lon_out, lat_out, i_in, j_in, i_out, j_out, cr=False):
    """The areas create_xgrid_great_circle gives the listed (source cell, destination cell) pairs with a mask of ones:
    great_circle_area of clip_2dx2d_great_circle of the two cells (create_xgrid.c:1413-1447), pair by pair -- for lists whose
    brute-force search is too long to run a second time.  A pair that does not clip to a polygon comes back as NaN."""
    L = oracle()
    lon_in, lat_in, lon_out, lat_out = f64(lon_in).ravel(), f64(lat_in).ravel(), f64(lon_out).ravel(), f64(lat_out).ravel()

    def cells(lon, lat, nxp, i, j):
        i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
        idx = np.stack([j * nxp + i, (j + 1) * nxp + i, (j + 1) * nxp + i + 1, j * nxp + i + 1], axis=1).ravel()
        lo, la = np.ascontiguousarray(lon[idx]), np.ascontiguousarray(lat[idx])
        x, y, z = (np.empty(idx.size) for _ in range(3))
        L.orc_latlon2xyz(idx.size, _dp(lo), _dp(la), _dp(x), _dp(y), _dp(z))
        return np.stack([x, y, z], axis=1).reshape(-1, 4, 3)

    a, b = cells(lon_in, lat_in, nx1 + 1, i_in, j_in), cells(lon_out, lat_out, nx2 + 1, i_out, j_out)
    out = np.full(len(a), np.nan)
    for k in range(len(a)):
        n, v = orc_clip_gc(a[k], b[k], cr=cr)
        if n > 0:
            out[k] = orc_great_circle_area(v[:, 0], v[:, 1], v[:, 2], cr=cr)
    return out


def ref_create_xgrid_gc(nx1, ny1, nx2, ny2, lon_in, lat_in, lon_out, lat_out, mask=None):
    L = ref()
    lon_in, lat_in, lon_out, lat_out = f64(lon_in).ravel(), f64(lat_in).ravel(), f64(lon_out).ravel(), f64(lat_out).ravel()
    mask = f64(np.ones(nx1 * ny1) if mask is None else mask).ravel()
    cap = 5000000
    ii, ji, io, jo = (np.empty(cap, dtype=np.int32) for _ in range(4))
    a, cl, ct = np.empty(cap), np.empty(cap), np.empty(cap)
    n = L.create_xgrid_great_circle(C.byref(C.c_int(nx1)), C.byref(C.c_int(ny1)), C.byref(C.c_int(nx2)), C.byref(C.c_int(ny2)),
                                    _dp(lon_in), _dp(lat_in), _dp(lon_out), _dp(lat_out), _dp(mask),
                                    _ip(ii), _ip(ji), _ip(io), _ip(jo), _dp(a), _dp(cl), _dp(ct))
    return dict(n=n, i_in=ii[:n].copy(), j_in=ji[:n].copy(), i_out=io[:n].copy(), j_out=jo[:n].copy(), area=a[:n].copy())


def orc_get_grid_gc_area(nx, ny, lon, lat, cr=False):
    lon, lat = f64(lon).ravel(), f64(lat).ravel()
    a = np.empty(nx * ny)
    _gc("orc_get_grid_great_circle_area", cr)(nx, ny, _dp(lon), _dp(lat), _dp(a))
    return a


def ref_get_grid_gc_area(nx, ny, lon, lat):
    lon, lat = f64(lon).ravel(), f64(lat).ravel()
    a = np.empty(nx * ny)
    ref().get_grid_great_circle_area(C.byref(C.c_int(nx)), C.byref(C.c_int(ny)), _dp(lon), _dp(lat), _dp(a))
    return a


def orc_create_xgrid_box(box_is_src, order, lon_b, lat_b, nxq, nyq, lon_q, lat_q, mask=None):
    """create_xgrid_1dx2d (box_is_src) / create_xgrid_2dx1d, order 1 or 2; lon_b/lat_b are the 1-D bounds."""
    L = oracle()
    lon_b, lat_b, lon_q, lat_q = f64(lon_b).ravel(), f64(lat_b).ravel(), f64(lon_q).ravel(), f64(lat_q).ravel()
    nxb, nyb = lon_b.size - 1, lat_b.size - 1
    nm = nxb * nyb if box_is_src else nxq * nyq
    mask = f64(np.ones(nm) if mask is None else mask).ravel()
    cap = 16 * (nxb * nyb + nxq * nyq) + 1024
    ii, ji, io, jo = (np.empty(cap, dtype=np.int32) for _ in range(4))
    a, cl, ct = np.empty(cap), np.empty(cap), np.empty(cap)
    n = L.orc_create_xgrid_box(1 if box_is_src else 0, order, nxb, nyb, _dp(lon_b), _dp(lat_b), nxq, nyq, _dp(lon_q), _dp(lat_q),
                               _dp(mask), cap, _ip(ii), _ip(ji), _ip(io), _ip(jo), _dp(a), _dp(cl), _dp(ct))
    assert n >= 0
    out = dict(n=int(n), i_in=ii[:n].copy(), j_in=ji[:n].copy(), i_out=io[:n].copy(), j_out=jo[:n].copy(), area=a[:n].copy())
    if order == 2:
        out["clon"], out["clat"] = cl[:n].copy(), ct[:n].copy()
    return out


def ref_create_xgrid_box(box_is_src, order, lon_b, lat_b, nxq, nyq, lon_q, lat_q, mask=None):
    L = ref()
    lon_b, lat_b, lon_q, lat_q = f64(lon_b).ravel(), f64(lat_b).ravel(), f64(lon_q).ravel(), f64(lat_q).ravel()
    nxb, nyb = lon_b.size - 1, lat_b.size - 1
    nm = nxb * nyb if box_is_src else nxq * nyq
    mask = f64(np.ones(nm) if mask is None else mask).ravel()
    cap = 5000000
    ii, ji, io, jo = (np.empty(cap, dtype=np.int32) for _ in range(4))
    a, cl, ct = np.empty(cap), np.empty(cap), np.empty(cap)
    ci = lambda v: C.byref(C.c_int(v))
    if box_is_src:
        sizes = [ci(nxb), ci(nyb), ci(nxq), ci(nyq)]
        grids = [_dp(lon_b), _dp(lat_b), _dp(lon_q), _dp(lat_q)]
        fn = L.create_xgrid_1dx2d_order1 if order == 1 else L.create_xgrid_1dx2d_order2
    else:
        sizes = [ci(nxq), ci(nyq), ci(nxb), ci(nyb)]
        grids = [_dp(lon_q), _dp(lat_q), _dp(lon_b), _dp(lat_b)]
        fn = L.create_xgrid_2dx1d_order1 if order == 1 else L.create_xgrid_2dx1d_order2
    args = sizes + grids + [_dp(mask), _ip(ii), _ip(ji), _ip(io), _ip(jo), _dp(a)]
    if order == 2:
        args += [_dp(cl), _dp(ct)]
    n = fn(*args)
    out = dict(n=int(n), i_in=ii[:n].copy(), j_in=ji[:n].copy(), i_out=io[:n].copy(), j_out=jo[:n].copy(), area=a[:n].copy())
    if order == 2:
        out["clon"], out["clat"] = cl[:n].copy(), ct[:n].copy()
    return out


# ------------------------------------------------------------------------------ the reference's conserve_interp.c
# option bits (tools/libfrencutils/globals.h)
CONSERVE_ORDER1, CONSERVE_ORDER2, TARGET, CHECK_CONSERVE, GREAT_CIRCLE, MONOTONIC = 1, 2, 16, 1024, 4096, 16384
CONSERVE_REF_PATH = os.path.join(ORACLE_DIR, "_ref", "libconserve_ref.so")


def conserve_ref_available():
    return os.path.exists(CONSERVE_REF_PATH)


def cref():
    """oracle/_ref/libconserve_ref.so (None if it has not been built)."""
    global _CREF
    if _CREF is None:
        if not conserve_ref_available():
            return None
        L = C.CDLL(CONSERVE_REF_PATH)
        dpp, ipp = C.POINTER(dp), C.POINTER(ip)
        L.cref_init.argtypes = []
        L.cref_init.restype = None
        L.cref_setup.argtypes = [C.c_uint, C.c_int, ip, ip, dpp, dpp, C.c_int, ip, ip, dpp, dpp, C.c_long, lp] + \
                                [ip] * 5 + [dp] * 3 + [dpp, dpp]
        L.cref_setup.restype = C.c_long
        L.cref_apply.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, ip, ip, dpp, C.c_int, ip, ip, dpp, lp] + [ip] * 5 + \
                                [dp] * 3 + [dpp, dpp, dpp, ipp, C.c_int, C.c_double, dpp, C.c_int, C.c_int, dpp, C.c_double,
                                            C.c_int, dpp, C.c_char_p, C.c_int]
        L.cref_apply.restype = C.c_int
        L.cref_init()
        _CREF = L
    return _CREF


def cref_setup(order, grids_in, grids_out, great_circle=False, capacity=None):
    """The reference's setup_conserve_interp (compute branch).  grids_*: lists of (nx, ny, lon, lat) corners.  Returns the
    dict of orc_setup (exchange cells of every destination tile back to back, xoff) plus the reference caller's
    cell_area_in / cell_area_out (get_grid_area, or get_grid_great_circle_area with great_circle)."""
    L = cref()
    nt, no = len(grids_in), len(grids_out)
    lon_in = [f64(g[2]).ravel() for g in grids_in]
    lat_in = [f64(g[3]).ravel() for g in grids_in]
    lon_out = [f64(g[2]).ravel() for g in grids_out]
    lat_out = [f64(g[3]).ravel() for g in grids_out]
    nx_in = np.array([g[0] for g in grids_in], dtype=np.int32)
    ny_in = np.array([g[1] for g in grids_in], dtype=np.int32)
    nx_out = np.array([g[0] for g in grids_out], dtype=np.int32)
    ny_out = np.array([g[1] for g in grids_out], dtype=np.int32)
    ca_in = [np.empty(g[0] * g[1]) for g in grids_in]
    ca_out = [np.empty(g[0] * g[1]) for g in grids_out]
    cap = capacity or 4 * (int(np.sum(nx_in * ny_in)) + int(np.sum(nx_out * ny_out))) * no + 1024
    xoff = np.zeros(no + 1, dtype=np.int64)
    t, ii, ji, io, jo = (np.empty(cap, dtype=np.int32) for _ in range(5))
    a, di, dj = np.empty(cap), np.empty(cap), np.empty(cap)
    opcode = (CONSERVE_ORDER2 if order == 2 else CONSERVE_ORDER1) | (GREAT_CIRCLE if great_circle else 0)
    n = L.cref_setup(opcode, nt, _ip(nx_in), _ip(ny_in), _ptr_array(lon_in), _ptr_array(lat_in), no, _ip(nx_out),
                     _ip(ny_out), _ptr_array(lon_out), _ptr_array(lat_out), cap, xoff.ctypes.data_as(lp),
                     _ip(t), _ip(ii), _ip(ji), _ip(io), _ip(jo), _dp(a), _dp(di), _dp(dj), _ptr_array(ca_in), _ptr_array(ca_out))
    if n < 0:
        raise RuntimeError(f"reference setup: more than {cap} exchange cells")
    out = dict(n=int(n), xoff=xoff, t_in=t[:n].copy(), i_in=ii[:n].copy(), j_in=ji[:n].copy(), i_out=io[:n].copy(),
               j_out=jo[:n].copy(), area=a[:n].copy(), cell_area_in=ca_in, cell_area_out=ca_out)
    if order == 2:
        out["di"], out["dj"] = di[:n].copy(), dj[:n].copy()
    return out


def cref_apply(order, x, nx_in, ny_in, data, grad_x, grad_y, grad_mask, has_missing, missing, nx2, ny2, nz,
               weight=None, cell_methods_sum=False, field_area=None, area_missing=-1e20, cell_area_in=None,
               target_grid=False, cell_area_out=None, monotonic=False, use_volume=False, check_conserve=False):
    """The reference's do_scalar_conserve_interp, arguments as orc_apply_ex (field_area given = cell_measures).
    x holds the exchange cells of every destination tile with xoff (a dict without xoff is one tile); nx2 / ny2 /
    cell_area_out are per destination tile when lists.  Returns (out, printed): out is one array [nz*ny2*nx2] per
    destination tile (a list when nx2 is a list), printed what the reference wrote to stdout.  A fatal data check of the
    reference ends the calling process (mpp_error -> exit(1)): run such cases in a child process."""
    L = cref()
    multi = isinstance(nx2, (list, tuple, np.ndarray))
    nx_o = np.asarray(nx2 if multi else [nx2], dtype=np.int32)
    ny_o = np.asarray(ny2 if multi else [ny2], dtype=np.int32)
    no = len(nx_o)
    xoff = np.asarray(x["xoff"], dtype=np.int64) if "xoff" in x else np.array([0, len(x["area"])], dtype=np.int64)
    assert len(xoff) == no + 1
    nt = len(nx_in)
    nxi = np.asarray(nx_in, dtype=np.int32)
    nyi = np.asarray(ny_in, dtype=np.int32)
    lst = lambda v: [f64(d).ravel() for d in v] if v is not None else None
    data, gx, gy, w, fa = lst(data), lst(grad_x), lst(grad_y), lst(weight), lst(field_area)
    if cell_area_in is None:
        cell_area_in = [np.ones(int(nxi[t]) * int(nyi[t])) for t in range(nt)]
    ca = lst(cell_area_in)
    if cell_area_out is None:
        cao = [np.ones(int(nx_o[m]) * int(ny_o[m])) for m in range(no)]
    else:
        cao = lst(cell_area_out if multi else [cell_area_out])
    gm = None
    if order == 2:                     # the monotone branch reads grad_mask whether or not the field has one
        gm = grad_mask if grad_mask is not None else [np.zeros(int(nxi[t]) * int(nyi[t])) for t in range(nt)]
        gm = [np.ascontiguousarray(g, dtype=np.int32).ravel() for g in gm]
    outs = [np.empty(nz * int(nx_o[m]) * int(ny_o[m])) for m in range(no)]
    ints = [np.ascontiguousarray(x[k], dtype=np.int32) for k in ("t_in", "i_in", "j_in", "i_out", "j_out")]
    area = f64(x["area"])
    di = f64(x["di"]) if order == 2 else None
    dj = f64(x["dj"]) if order == 2 else None
    pa = lambda v, t=dp: _ptr_array(v, t) if v else None
    opcode = (TARGET if target_grid else 0) | (MONOTONIC if monotonic else 0) | (CHECK_CONSERVE if check_conserve else 0)
    msg = C.create_string_buffer(1 << 16)
    L.cref_apply(opcode, order, nz, nt, _ip(nxi), _ip(nyi), pa(ca), no, _ip(nx_o), _ip(ny_o), pa(cao),
                 xoff.ctypes.data_as(lp), *[_ip(v) for v in ints], _dp(area), _dp(di), _dp(dj),
                 pa(data), pa(gx), pa(gy), pa(gm, ip), 1 if has_missing else 0, float(missing), pa(w),
                 1 if cell_methods_sum else 0, 1 if fa is not None else 0, pa(fa), float(area_missing),
                 1 if use_volume else 0, pa(outs), msg, len(msg))
    printed = msg.value.decode(errors="replace")
    return (outs if multi else outs[0]), printed


# ------------------------------------------------------------------------------ the reference's bilinear_interp.c
BILINEAR_REF_PATH = os.path.join(ORACLE_DIR, "_ref", "libbilinear_ref.so")
_BREF_GRID = [C.c_int, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_double] * 4     # N, halo'd centres, target


def bilinear_ref_available():
    return os.path.exists(BILINEAR_REF_PATH)


def bref():
    """oracle/_ref/libbilinear_ref.so (None if it has not been built)."""
    global _BREF
    if _BREF is None:
        if not bilinear_ref_available():
            return None
        L = C.CDLL(BILINEAR_REF_PATH)
        L.bref_init.argtypes = [C.c_int]
        L.bref_init.restype = None
        L.bref_setup.argtypes = _BREF_GRID + [ip] + [dp] * 7
        L.bref_setup.restype = C.c_int
        target = [C.c_int] * 4 + [ip, dp, dp]
        L.bref_apply_scalar.argtypes = target + [dp, C.c_int, C.c_double, C.c_int, dp]
        L.bref_apply_scalar.restype = C.c_int
        L.bref_apply_vector.argtypes = target + [dp] * 6 + [C.c_int, C.c_double, C.c_int, dp, dp]
        L.bref_apply_vector.restype = C.c_int
        L.bref_unit_vect_latlon.argtypes = [C.c_int, dp, dp, dp, dp]
        L.bref_unit_vect_latlon.restype = None
        L.bref_cell_dist.argtypes = [C.c_int, dp, dp, dp]
        L.bref_cell_dist.restype = None
        L.bref_max_weight_index.argtypes = [C.c_long, dp, ip]
        L.bref_max_weight_index.restype = None
        L.normalize_great_circle_distance.argtypes = [dp, dp]
        L.normalize_great_circle_distance.restype = C.c_double
        L.max_weight_index.argtypes = [dp, C.c_int]
        L.max_weight_index.restype = C.c_int
        L.do_latlon_coarsening.argtypes = [dp, dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_double]
        L.do_latlon_coarsening.restype = None
        _BREF = L
    return _BREF


def _bref_grid(cfg, lont_h, latt_h):
    """cfg: dict(N, nlon, nlat, finer_step=0, center_y=False, lonbegin=0, lonend=360, latbegin=-90, latend=90)"""
    N = int(cfg["N"])
    lh, ah = f64(lont_h).reshape(-1), f64(latt_h).reshape(-1)
    assert lh.size == ah.size == 6 * (N + 2) ** 2
    args = [N, _dp(lh), _dp(ah), int(cfg["nlon"]), int(cfg["nlat"]), int(cfg.get("finer_step", 0)),
            1 if cfg.get("center_y", False) else 0, float(cfg.get("lonbegin", 0.0)), float(cfg.get("lonend", 360.0)),
            float(cfg.get("latbegin", -90.0)), float(cfg.get("latend", 90.0))]
    fs = int(cfg.get("finer_step", 0))
    nyf, nxf = (2 ** fs) * (int(cfg["nlat"]) - 1) + 1, (2 ** fs) * int(cfg["nlon"])
    return args, (lh, ah), nxf, nyf


def bref_setup(cfg, lont_h, latt_h):
    """The reference's setup_bilinear_interp (compute branch) in this process.  lont_h / latt_h: halo'd centres [6, N+2, N+2]
    (radians).  Returns index [n, 3], weight [n, 4] and the fine grid its caller built: lont, latt [n], latt1d [ny_fine],
    xyz [3, n], vlon, vlat [n, 3].  Only for targets whose ten sweeps are known to find every point: otherwise see
    bref_setup_child."""
    L = bref()
    args, keep, nxf, nyf = _bref_grid(cfg, lont_h, latt_h)
    n = nxf * nyf
    out = dict(index=np.empty((n, 3), dtype=np.int32), weight=np.empty((n, 4)), lont=np.empty(n), latt=np.empty(n),
               latt1d=np.empty(nyf), xyz=np.empty((3, n)), vlon=np.empty((n, 3)), vlat=np.empty((n, 3)))
    L.bref_setup(*args, _ip(out["index"]), *[_dp(out[k]) for k in ("weight", "lont", "latt", "latt1d", "xyz", "vlon", "vlat")])
    return out


def bref_setup_child(cfg, lont_h, latt_h, workdir, timeout=600):
    """bref_setup in a child process (its stdout line-buffered).  The reference starts its "global sweep" (bilinear_interp.c:
    213-259, which reads past its arrays) when the ten sweeps leave a point unfound; the child is stopped at its warning.
    Returns (result or None, printed text, fell_back).  The child loads only oracle/_ref and numpy."""
    inp, outp = os.path.join(workdir, "bref_in.npz"), os.path.join(workdir, "bref_out.npz")
    np.savez(inp, lont_h=f64(lont_h), latt_h=f64(latt_h), cfg=np.array(repr(dict(cfg))))
    if os.path.exists(outp):
        os.remove(outp)
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "bref_setup", inp, outp], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, cwd=workdir)
    lines, fell_back = [], False
    try:
        for line in p.stdout:
            lines.append(line)
            if "global sweep" in line:
                fell_back = True
                p.kill()
                break
        p.wait(timeout=timeout)
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
        p.stdout.close()
    printed = "".join(lines)
    if fell_back:
        return None, printed, True
    if p.returncode != 0:
        raise RuntimeError(f"reference setup child exited with {p.returncode}: {printed[-2000:]}")
    d = np.load(outp)
    return {k: d[k] for k in d.files}, printed, False


def _bref_setup_main(inp, outp):
    import ast
    d = np.load(inp)
    bref().bref_init(1)
    out = bref_setup(ast.literal_eval(str(d["cfg"])), d["lont_h"], d["latt_h"])
    np.savez(outp, **out)


def bref_unit_vect_latlon(lon, lat):
    """the reference's unit_vect_latlon: vlon, vlat [..., 3]"""
    lon, lat = f64(lon).reshape(-1), f64(lat).reshape(-1)
    vlo, vla = np.empty((lon.size, 3)), np.empty((lon.size, 3))
    bref().bref_unit_vect_latlon(lon.size, _dp(lon), _dp(lat), _dp(vlo), _dp(vla))
    return vlo, vla


def _bref_target(cfg, setup):
    fs = int(cfg.get("finer_step", 0))
    idx, w = np.ascontiguousarray(setup["index"], dtype=np.int32), f64(setup["weight"])
    nyf, nxf = (2 ** fs) * (int(cfg["nlat"]) - 1) + 1, (2 ** fs) * int(cfg["nlon"])
    assert idx.size == 3 * nxf * nyf and w.size == 4 * nxf * nyf and setup["latt1d"].size == nyf
    return [int(cfg["N"]), int(cfg["nlon"]), int(cfg["nlat"]), fs, _ip(idx), _dp(w), _dp(f64(setup["latt1d"]))], (idx, w)


def bref_apply_scalar(cfg, setup, data_h, has_missing=False, missing=0.0, fill_missing=False):
    """do_scalar_bilinear_interp, one level as fregrid calls it, with the plan of `setup` (bref_setup's dict or one with the
    same index / weight / latt1d): data_h [6, N+2, N+2] halo'd -> [nlat, nlon]"""
    args, keep = _bref_target(cfg, setup)
    d = f64(data_h)
    assert d.size == 6 * (int(cfg["N"]) + 2) ** 2
    out = np.empty((int(cfg["nlat"]), int(cfg["nlon"])))
    bref().bref_apply_scalar(*args, _dp(d), 1 if has_missing else 0, float(missing), 1 if fill_missing else 0, _dp(out))
    return out


def bref_apply_vector(cfg, setup, vlon_in, vlat_in, u_h, v_h, has_missing=False, missing=0.0, fill_missing=False):
    """do_vector_bilinear_interp, one level: u_h, v_h [6, N+2, N+2] halo'd -> (u_out, v_out) [nlat, nlon].  vlon_in / vlat_in:
    bref_unit_vect_latlon of the halo'd centres; the fine grid's vlon / vlat come from `setup`."""
    args, keep = _bref_target(cfg, setup)
    u, v, vi, wi = f64(u_h), f64(v_h), f64(vlon_in), f64(vlat_in)
    vo, wo = f64(setup["vlon"]), f64(setup["vlat"])
    F = 6 * (int(cfg["N"]) + 2) ** 2
    assert u.size == v.size == F and vi.size == wi.size == 3 * F and vo.size == 3 * len(keep[0])
    uo, vo_ = np.empty((int(cfg["nlat"]), int(cfg["nlon"]))), np.empty((int(cfg["nlat"]), int(cfg["nlon"])))
    bref().bref_apply_vector(*args, _dp(vi), _dp(wi), _dp(vo), _dp(wo), _dp(u), _dp(v), 1 if has_missing else 0, float(missing),
                             1 if fill_missing else 0, _dp(uo), _dp(vo_))
    return uo, vo_


def bref_cell_dist(N, lont_h, latt_h):
    """normalize_great_circle_distance of each cell's centres (jc, ic) -> (jc+1, ic+1), [6*N*N] in the device's cell order"""
    lh, ah = f64(lont_h).reshape(-1), f64(latt_h).reshape(-1)
    out = np.empty(6 * N * N)
    bref().bref_cell_dist(N, _dp(lh), _dp(ah), _dp(out))
    return out


def bref_max_weight_index(weight):
    w = f64(weight).reshape(-1, 4)
    out = np.empty(len(w), dtype=np.int32)
    bref().bref_max_weight_index(len(w), _dp(w), _ip(out))
    return out


def bref_latlon_coarsening(var, ylat, nlon, nlat, finer_step, has_missing=False, missing=0.0):
    """do_latlon_coarsening of one level: var [nlat, nlon] fine -> [(nlat-1)/2**fs+1, nlon/2**fs]"""
    v, y = f64(var).reshape(-1), f64(ylat)
    out = np.empty(((nlat - 1) // 2 ** finer_step + 1) * (nlon // 2 ** finer_step))
    bref().do_latlon_coarsening(_dp(v), _dp(y), nlon, nlat, 1, _dp(out), finer_step, 1 if has_missing else 0, float(missing))
    return out.reshape((nlat - 1) // 2 ** finer_step + 1, nlon // 2 ** finer_step)


def host_has_fma():
    """libm's sin()/cos() run their FMA build on an FMA-capable x86-64 host; the device trig emulates that build, so the
    bit-identity assertions of the legacy path hold where the oracle runs on such a host (every box of the GPU pool so far).
    On a host without FMA libm's results differ in the last place for ~0.07 % of arguments and the tests fall back to 1e-10."""
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return True


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "bref_setup":
        _bref_setup_main(sys.argv[2], sys.argv[3])
    else:
        sys.exit(f"usage: {sys.argv[0]} bref_setup IN.npz OUT.npz")
