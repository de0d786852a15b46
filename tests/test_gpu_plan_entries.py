"""The plan-creating entries side by side (fg_plan_create, _dev, _great_circle, _great_circle_dev, _great_circle_lonlat,
_great_circle_lonlat_dev, _polylist, _create_empty): what they share -- adoption of a caller's stream, given or derived
destination extents, the argument checks and the ownership of a plan that fails -- on grids small enough that every case is a
few milliseconds: one or two C8 tiles -> 36x18, and a list of 16 polygons."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FG_ERR_ARG = -1
DPT = C.POINTER(C.c_double)
DEV = ("create_dev", "create_great_circle_dev", "create_great_circle_lonlat_dev")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def _grids(fg, ntiles):
    c8 = fg.gnomonic_ed_corners(8)
    return [fg.GridConfig(8, 8, c8[0][t], c8[1][t]) for t in range(ntiles)], fg.GridConfig(36, 18, *fg.latlon_corners(36, 18))


def _same_plan(a, b, what):
    assert len(a["area"]) == len(b["area"]) > 0, what
    for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert np.array_equal(_bits(a["area"]), _bits(b["area"])), what


def _take(plan):
    x = plan.get_xgrid()
    plan.destroy()
    return x


# ------------------------------------------------------------------------------------------ the _dev entries
def _dev_plan(fg, entry, ntiles, **kw):
    """A plan from one of the three device-array entries; the tensors are uploaded and complete before the call"""
    import torch
    gin, gout = _grids(fg, ntiles)
    up = lambda a: torch.from_numpy(_f64(a).copy()).cuda()
    nx, ny = [g.nx for g in gin], [g.ny for g in gin]
    if entry == "create_great_circle_dev":
        xyz_in = [tuple(up(v) for v in fg.latlon2xyz(_f64(g.lonc), _f64(g.latc))) for g in gin]
        xyz_out = tuple(up(v) for v in fg.latlon2xyz(_f64(gout.lonc), _f64(gout.latc)))
        torch.cuda.synchronize()
        return fg.XgridPlan.create_great_circle_dev(nx, ny, xyz_in, gout.nx, gout.ny, xyz_out, **kw)
    t = [up(g.lonc) for g in gin], [up(g.latc) for g in gin], up(gout.lonc), up(gout.latc)
    torch.cuda.synchronize()
    args = (nx, ny, t[0], t[1], gout.nx, gout.ny, t[2], t[3])
    if entry == "create_dev":
        return fg.XgridPlan.create_dev(1, *args, **kw)
    return fg.XgridPlan.create_great_circle_lonlat_dev(*args, **kw)


@pytest.mark.parametrize("ntiles", [1, 2])
@pytest.mark.parametrize("entry", DEV)
def test_caller_stream(fg, gpu_ok, entry, ntiles):
    """stream=...: the plan runs on the caller's stream and leaves it alone when it goes; stream=None: on one of its own.  The
    same plan either way."""
    import torch
    s = torch.cuda.Stream()
    own = _dev_plan(fg, entry, ntiles, stream=None)
    mine = _dev_plan(fg, entry, ntiles, stream=s.cuda_stream)
    assert int(mine.stream() or 0) == int(s.cuda_stream)
    assert int(own.stream() or 0) not in (0, int(s.cuda_stream))
    a, b = _take(own), _take(mine)
    with torch.cuda.stream(s):
        y = torch.arange(1000, device="cuda", dtype=torch.float64) * 2
    s.synchronize()
    assert float(y.sum().item()) == 999000.0
    _same_plan(a, b, entry)


@pytest.mark.parametrize("ntiles", [1, 2])
@pytest.mark.parametrize("entry", DEV)
def test_given_and_derived_extents(fg, gpu_ok, entry, ntiles):
    """mean_dlat / mean_dlon only size the bins of the candidate search: extents sampled from the destination grid (0) and given
    ones (half a destination cell) make the same plan."""
    a = _take(_dev_plan(fg, entry, ntiles, mean_dlat=0.0, mean_dlon=0.0))
    b = _take(_dev_plan(fg, entry, ntiles, mean_dlat=np.pi / 36, mean_dlon=np.pi / 36))
    _same_plan(a, b, entry)


# ------------------------------------------------------------------------------------------ argument errors, raw calls
class _Entry:
    """One entry of the C interface with a good argument list, by name and in the entry's order (``h``, the plan_out word, is
    appended by call()); ptrs: the top-level pointers that must not be null; keep: whatever the pointers point into."""

    def __init__(self, fg, name, args, ptrs, great_circle, keep):
        self.fg, self.name, self.fn, self.args, self.ptrs, self.great_circle, self.keep = fg, name, getattr(fg.lib(), name), args, ptrs, great_circle, keep
        self.ntiles_key = "npoly" if "npoly" in args else "nt"

    def call(self, **over):
        h = C.c_void_p()
        rc = self.fn(*{**self.args, **over}.values(), C.byref(h))
        return rc, h

    def good(self):
        rc, h = self.call()
        assert rc >= 0 and h.value, (self.name, rc, self.fg._lib.last_error())
        return self.fg.XgridPlan(h.value, self.args.get("order", 1), 0, self.great_circle)

    def bad_calls(self):
        ndev = self.fg.lib().fg_device_count()
        bad = [(f"{p} = NULL", {p: None}) for p in self.ptrs]
        bad += [(f"{self.ntiles_key} = 0", {self.ntiles_key: 0}), ("nx_out = 0", {"nx_out": 0}), ("device = fg_device_count()", {"device": ndev})]
        if "nx" in self.args:
            bad.append(("nx_in[0] = 0", {"nx": (C.c_int * len(self.args["nx"]))(0, *list(self.args["nx"])[1:])}))
        if "order" in self.args:
            bad.append(("order = 3", {"order": 3}))
        return bad


def _entries(fg):
    """Every plan-creating entry on two C8 tiles -> 36x18 (the polygon list: 16 quadrilaterals -> 36x18)"""
    import torch
    gin, gout = _grids(fg, 2)
    nt = len(gin)
    nx, ny = (C.c_int * nt)(*[g.nx for g in gin]), (C.c_int * nt)(*[g.ny for g in gin])
    h_lon, h_lat, h_lo, h_la = [_f64(g.lonc) for g in gin], [_f64(g.latc) for g in gin], _f64(gout.lonc), _f64(gout.latc)
    dp = lambda a: a.ctypes.data_as(DPT)
    host = dict(nt=nt, nx=nx, ny=ny, lon=(DPT * nt)(*[dp(a) for a in h_lon]), lat=(DPT * nt)(*[dp(a) for a in h_lat]), mask=None,
                nx_out=gout.nx, ny_out=gout.ny, lo=dp(h_lo), la=dp(h_la), device=0)
    up = lambda a: torch.from_numpy(a.copy()).cuda()
    vps = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    vp = lambda t: C.c_void_p(t.data_ptr())
    d_lon, d_lat, d_lo, d_la = [up(a) for a in h_lon], [up(a) for a in h_lat], up(h_lo), up(h_la)
    tail = dict(mean_dlat=0.0, mean_dlon=0.0, device=0, stream=None, use=0)
    dev = dict(nt=nt, nx=nx, ny=ny, lon=vps(d_lon), lat=vps(d_lat), mask=None, nx_out=gout.nx, ny_out=gout.ny, lo=vp(d_lo), la=vp(d_la), **tail)
    xyz_in = [[up(v) for v in fg.latlon2xyz(a, b)] for a, b in zip(h_lon, h_lat)]
    xyz_out = [up(v) for v in fg.latlon2xyz(h_lo, h_la)]
    gcd = dict(nt=nt, nx=nx, ny=ny, x=vps([t[0] for t in xyz_in]), y=vps([t[1] for t in xyz_in]), z=vps([t[2] for t in xyz_in]), mask=None,
               nx_out=gout.nx, ny_out=gout.ny, xo=vp(xyz_out[0]), yo=vp(xyz_out[1]), zo=vp(xyz_out[2]), **tail)
    torch.cuda.synchronize()
    # 16 cells of 10 x 10 degrees, off the destination's grid lines by 3 degrees: SW, SE, NE, NW, padded to 8 vertices
    pn = np.full(16, 4, dtype=np.int32)
    plon, plat = np.zeros((16, 8)), np.zeros((16, 8))
    for k in range(16):
        x0, y0 = np.radians(13.0 + 10 * (k % 4)), np.radians(-17.0 + 10 * (k // 4))
        x1, y1 = x0 + np.radians(10.0), y0 + np.radians(10.0)
        plon[k, :4], plat[k, :4] = (x0, x1, x1, x0), (y0, y0, y1, y1)
    pavg = plon[:, :4].mean(axis=1)
    parea = (plon[:, 1] - plon[:, 0]) * (np.sin(plat[:, 2]) - np.sin(plat[:, 0]))
    poly = dict(order=1, npoly=16, n=pn.ctypes.data_as(C.POINTER(C.c_int)), lon=dp(plon), lat=dp(plat), lon_avg=dp(pavg), area_ref=dp(parea),
                nx_out=gout.nx, ny_out=gout.ny, lo=dp(h_lo), la=dp(h_la), device=0)
    empty = dict(order=1, nt=nt, nx=nx, ny=ny, nx_out=gout.nx, ny_out=gout.ny, device=0)
    keep = (h_lon, h_lat, h_lo, h_la, d_lon, d_lat, d_lo, d_la, xyz_in, xyz_out, pn, plon, plat, pavg, parea)
    grid, ll = ("nx", "ny", "lon", "lat", "lo", "la"), ("n", "lon", "lat", "lon_avg", "area_ref", "lo", "la")
    E = lambda name, args, ptrs, gc=False: _Entry(fg, name, args, ptrs, gc, keep)
    return [E("fg_plan_create", dict(order=1, **host), grid), E("fg_plan_create_dev", dict(order=1, **dev), grid),
            E("fg_plan_create_great_circle", host, grid, True), E("fg_plan_create_great_circle_dev", gcd, ("nx", "ny", "x", "y", "z", "xo", "yo", "zo"), True),
            E("fg_plan_create_great_circle_lonlat", host, grid, True), E("fg_plan_create_great_circle_lonlat_dev", dev, grid, True),
            E("fg_plan_create_polylist", poly, ll), E("fg_plan_create_empty", empty, ("nx", "ny"))]


ENTRY_NAMES = ["fg_plan_create", "fg_plan_create_dev", "fg_plan_create_great_circle", "fg_plan_create_great_circle_dev",
               "fg_plan_create_great_circle_lonlat", "fg_plan_create_great_circle_lonlat_dev", "fg_plan_create_polylist", "fg_plan_create_empty"]


@pytest.fixture(scope="module")
def entries(fg, gpu_ok):
    es = _entries(fg)
    assert [e.name for e in es] == ENTRY_NAMES
    return {e.name: e for e in es}


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_argument_errors(fg, entries, name):
    """Every bad argument is FG_ERR_ARG with a message, the plan_out word stays NULL, and the plan that follows the whole table
    is the plan made before it."""
    e = entries[name]
    searching = entries["fg_plan_create"] if name == "fg_plan_create_empty" else e      # (an empty plan has no lists to compare)
    before = _take(searching.good())
    for what, over in e.bad_calls():
        rc, h = e.call(**over)
        assert rc == FG_ERR_ARG, (name, what, rc)
        assert fg._lib.last_error(), (name, what)
        assert h.value is None, (name, what)
    if name == "fg_plan_create_empty":
        e.good().destroy()
    _same_plan(before, _take(searching.good()), name)


@pytest.mark.parametrize("name", ["fg_plan_create", "fg_plan_create_great_circle", "fg_plan_create_great_circle_lonlat"])
@pytest.mark.parametrize("which", ["lon", "lat"])
def test_null_per_tile_pointer(fg, entries, name, which):
    """A null corner array of one tile (the second of two) in a host pointer table: an argument error, not a crash"""
    e = entries[name]
    table = (DPT * 2)(e.args[which][0], DPT())
    rc, h = e.call(**{which: table})
    assert rc == FG_ERR_ARG, (name, rc)
    assert "null grid pointer" in fg._lib.last_error()
    assert h.value is None
    assert _take(e.good())["area"].size > 0
