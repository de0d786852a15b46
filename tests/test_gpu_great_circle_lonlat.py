"""latlon2xyz on the device and the great-circle plan entries that start from lon / lat (fg_dev_latlon2xyz,
fg_plan_create_great_circle_lonlat, fg_plan_create_great_circle_lonlat_dev): the unit vectors carry the bits of the compiled
reference's latlon2xyz, so the plans are the ones fg_plan_create_great_circle builds from host-made unit vectors -- bit for bit --
and agree with the reference's create_xgrid_great_circle to the bar test_gpu_great_circle.py sets: lists exact, areas to 1e-10
and 98 % in bits against the reference, all of them in bits against the oracle's _cr build (the device's arc cosine)."""
import ctypes as C

import numpy as np
import pytest

import orc
from test_gpu_great_circle import RTOL, _cases

pytestmark = pytest.mark.gpu
HPI = np.pi / 2
HANDOVER = float.fromhex("0x1.368fdp+1")       # where libm's sin() / cos() switch to the wide reduction (its "2.426265")
dp = C.POINTER(C.c_double)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _crafted_lons():
    """The arguments the host check walks: quadrant boundaries k pi/2 +- 2^-e, the hand-over at 2.4262, reduced arguments around
    a*a = 0.01588 and |a| = 0.126, +-0, +-1000 and the bound."""
    k = np.arange(-8, 9)[:, None, None] * HPI
    e = 2.0 ** -np.arange(0, 46)[None, :, None]
    s = np.array([-1.0, 1.0])[None, None, :]
    v = [(k + s * e).ravel()]
    v.append(np.array([sg * (2.426265 + d) for sg in (-1, 1) for d in (0.0, 4e-16, -4e-16, 1e-9, -1e-9, -2.372e-7, -2.38e-7, 1e-3, -1e-3)]))
    for a0 in (0.126, 0.12601587):
        v.append(np.array([kk * HPI + sg * (a0 + d) for kk in range(-8, 9) for sg in (-1, 1) for d in (0.0, 1e-12, -1e-12, 1e-7, -1e-7)]))
    v.append(np.array([0.0, -0.0, 1000.0, -1000.0, 1024.0, -1024.0, HANDOVER, -HANDOVER, np.nextafter(HANDOVER, 0), 2 * np.pi, 4 * np.pi]))
    return np.concatenate(v)


@pytest.fixture(scope="module")
def ll2x_pool():
    """4099 (lon, lat) pairs -- crafted longitudes first, random ones (frames up to +-4 pi, some up to +-1000) behind them -- and
    the compiled reference's latlon2xyz of them, once with these latitudes and once with lat = 0."""
    R = orc.ref()
    assert R is not None, "oracle/_ref/libfrenc_ref.so is missing: build() makes it from the reference sources"
    R.latlon2xyz.argtypes = [C.c_int] + [dp] * 5
    R.latlon2xyz.restype = None
    rng = np.random.default_rng(5)
    lon = _crafted_lons()
    nr = 4099 - lon.size
    assert nr > 1000
    lon = np.concatenate([lon, rng.uniform(-4 * np.pi, 4 * np.pi, nr - 200), rng.uniform(-1000, 1000, 200)])
    lat = rng.uniform(-HPI, HPI, lon.size)
    lat[:8] = [HPI, -HPI, 0.0, -0.0, 0.85546875, -0.85546875, 0.126, 1e-30]
    perm = rng.permutation(lon.size)                      # every n below gets crafted and random arguments
    lon, lat = np.ascontiguousarray(lon[perm]), np.ascontiguousarray(lat[perm])
    zero = np.zeros_like(lat)
    ref, ref0 = [np.empty(lon.size) for _ in range(3)], [np.empty(lon.size) for _ in range(3)]
    R.latlon2xyz(lon.size, orc._dp(lon), orc._dp(lat), *[orc._dp(v) for v in ref])
    R.latlon2xyz(lon.size, orc._dp(lon), orc._dp(zero), *[orc._dp(v) for v in ref0])
    return lon, lat, ref, ref0


def _same(got, ref, what):
    if orc.host_has_fma():
        assert np.array_equal(_bits(got), _bits(ref)), what
    else:                                                 # the relaxed rule of test_device_sincos_equals_host_libm
        assert np.mean(_bits(got) != _bits(ref)) < 2e-3 and np.max(np.abs(got - ref)) < 3e-16, what


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4099])
def test_dev_latlon2xyz_bits(fg, gpu_ok, ll2x_pool, n):
    import torch
    lon, lat, ref, ref0 = ll2x_pool
    lon_t, lat_t = torch.from_numpy(lon[:n].copy()).cuda(), torch.from_numpy(lat[:n].copy()).cuda()
    got = [v.cpu().numpy() for v in fg.latlon2xyz_dev(lon_t, lat_t)]
    got0 = [v.cpu().numpy() for v in fg.latlon2xyz_dev(lon_t, torch.zeros_like(lat_t))]
    for ax in range(3):
        _same(got[ax], ref[ax][:n], (n, "xyz"[ax]))
        _same(got0[ax], ref0[ax][:n], (n, "lat = 0", "xyz"[ax]))       # x = cos(lon), y = sin(lon): the wide branch alone
    assert not got0[2].any()


def test_dev_latlon2xyz_outside_the_domain_is_nan(fg, gpu_ok):
    import torch
    lon = np.array([0.5, np.nan, np.inf, 1025.0, 0.5, 0.5, -np.inf, -1000.0] + [0.25] * 70)
    lat = np.array([0.25, 0.0, 0.0, 0.0, np.nan, 2.43, 0.1, -0.25] + [0.5] * 70)
    bad = np.array([False, True, True, True, True, True, True, False] + [False] * 70)
    x, y, z = (v.cpu().numpy() for v in fg.latlon2xyz_dev(torch.from_numpy(lon).cuda(), torch.from_numpy(lat).cuda()))
    for v in (x, y, z):
        assert np.array_equal(np.isnan(v), bad)
    hx, hy, hz = fg.latlon2xyz(lon[~bad], lat[~bad])
    _same(x[~bad], hx, "x"); _same(y[~bad], hy, "y"); _same(z[~bad], hz, "z")


def _three_plans(fg, grids_in, grid_out, masks):
    """The plan from today's host entry, from the host lon / lat entry and from the device lon / lat entry"""
    import torch
    plans = [fg.XgridPlan.create_great_circle(grids_in, grid_out, masks=masks),
             fg.XgridPlan.create_great_circle_lonlat(grids_in, grid_out, masks=masks)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1).copy()).cuda()
    lon_t, lat_t = [up(g.lonc) for g in grids_in], [up(g.latc) for g in grids_in]
    lo_t, la_t = up(grid_out.lonc), up(grid_out.latc)
    masks_t = None if masks is None else [up(m) for m in masks]
    torch.cuda.synchronize()
    plans.append(fg.XgridPlan.create_great_circle_lonlat_dev([g.nx for g in grids_in], [g.ny for g in grids_in], lon_t, lat_t,
                                                             grid_out.nx, grid_out.ny, lo_t, la_t, masks_t=masks_t))
    return plans


def _lonlat_cases(fg):
    out = {}
    for name, (nxi, nyi, nxo, nyo, loi, lai, loo, lao) in _cases(fg).items():
        out[name] = ([fg.GridConfig(nxi, nyi, loi, lai)], fg.GridConfig(nxo, nyo, loo, lao))
    c12 = fg.gnomonic_ed_corners(12)
    six = [fg.GridConfig(12, 12, c12[0][t], c12[1][t]) for t in range(6)]
    out["c12_six_tiles_frame_-pi_pi"] = (six, fg.GridConfig(72, 36, *fg.latlon_corners(72, 36, -180.0, 180.0, -90.0, 90.0)))
    out["c12_six_tiles_frame_2pi_4pi"] = (six, fg.GridConfig(72, 36, *fg.latlon_corners(72, 36, 360.0, 720.0, -90.0, 90.0)))
    # ten grids in all: more than one launch's worth of descriptors (FG_TILESET_MAX = 8), so the conversion takes two launches
    c8 = fg.gnomonic_ed_corners(8)
    nine = [fg.GridConfig(8, 8, c8[0][t % 6], c8[1][t % 6]) for t in range(9)]
    out["nine_source_tiles"] = (nine, fg.GridConfig(36, 18, *fg.latlon_corners(36, 18)))
    return out


@pytest.mark.parametrize("name", ["c24_tile1_144x90", "c24_tile3_polar_144x90", "latlon_aligned_2x", "latlon_regional_offset",
                                  "latlon_to_cubed_polar", "tripolar_to_cubed", "c12_six_tiles_frame_-pi_pi", "c12_six_tiles_frame_2pi_4pi",
                                  "nine_source_tiles"])
@pytest.mark.parametrize("masked", [False, True])
def test_great_circle_lonlat_equals_xyz_entry(fg, gpu_ok, name, masked):
    """The same unit vectors, so the same plan: lists, areas and (with a mask) the sweep of one field, bit for bit among
    fg_plan_create_great_circle, the host lon / lat entry and the device lon / lat entry."""
    import torch
    grids_in, grid_out = _lonlat_cases(fg)[name]
    rng = np.random.default_rng(3)
    masks = [(rng.uniform(size=g.nx * g.ny) > 0.25).astype(np.float64) for g in grids_in] if masked else None
    plans = _three_plans(fg, grids_in, grid_out, masks)
    res = []
    data = np.concatenate([rng.standard_normal(g.nx * g.ny) + 3.0 for g in grids_in])
    for plan in plans:
        assert plan.nxgrid > 0
        plan.finalize()
        x = plan.get_xgrid()
        if masked:
            d_t = torch.from_numpy(data).cuda()
            out_t = torch.empty(grid_out.nx * grid_out.ny, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            plan.apply(d_t, out_t)
            plan.sync()
            x["swept"] = out_t.cpu().numpy()
        res.append(x)
        plan.destroy()
    a = res[0]
    for b, route in zip(res[1:], ("host lon/lat", "device lon/lat")):
        assert len(a["area"]) == len(b["area"]), route
        for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(a[k], b[k]), (route, k)
        assert np.array_equal(_bits(a["area"]), _bits(b["area"])), route
        if masked:
            assert np.array_equal(_bits(a["swept"]), _bits(b["swept"])), route


@pytest.mark.parametrize("name", ["c24_tile1_144x90", "latlon_aligned_2x"])
def test_great_circle_lonlat_vs_reference(fg, gpu_ok, name):
    """Against the reference's own entry from lon / lat (create_xgrid_great_circle of the compiled reference): lists exact,
    areas to the bar of test_create_xgrid_great_circle_vs_oracle, and every one in bits against the oracle's _cr build."""
    assert orc.ref_available(), "oracle/_ref/libfrenc_ref.so is missing: build() makes it from the reference sources"
    args = _cases(fg)[name]
    nxi, nyi, nxo, nyo, loi, lai, loo, lao = args
    o = orc.ref_create_xgrid_gc(*args)
    ocr = orc.orc_create_xgrid_gc(*args, cr=True)          # the oracle that rounds like the device: every area, in bits
    assert ocr["n"] == o["n"]
    for plan in _three_plans(fg, [fg.GridConfig(nxi, nyi, loi, lai)], fg.GridConfig(nxo, nyo, loo, lao), None)[1:]:
        x = plan.get_xgrid()
        plan.destroy()
        assert len(x["area"]) == o["n"] and o["n"] > 0
        for k in ("i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(x[k], o[k]), k
        rel = np.abs(x["area"] - o["area"]) / o["area"]
        assert rel.max() < RTOL
        same = np.mean(_bits(x["area"]) == _bits(o["area"]))
        assert same > 0.98, same
        nd = int(np.count_nonzero(_bits(x["area"]) != _bits(ocr["area"])))
        assert nd == 0, f"{nd} of {o['n']} exchange-cell areas differ from the _cr oracle"


def test_great_circle_lonlat_domain_error(fg, gpu_ok):
    """One NaN corner in the source grid: FG_ERR_ARG from the search's read-back; the next plan on the device is fine."""
    import torch
    c12 = fg.gnomonic_ed_corners(12)
    lo, la = fg.latlon_corners(36, 18)
    bad_lon = np.array(c12[0][2], dtype=np.float64).copy()
    bad_lon.reshape(-1)[40] = np.nan
    src_bad, src, dst = fg.GridConfig(12, 12, bad_lon, c12[1][2]), fg.GridConfig(12, 12, c12[0][2], c12[1][2]), fg.GridConfig(36, 18, lo, la)
    with pytest.raises(fg.FregridHipError, match="latlon2xyz") as ei:
        fg.XgridPlan.create_great_circle_lonlat([src_bad], dst)
    assert ei.value.code == -1                                  # FG_ERR_ARG
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1).copy()).cuda()
    t = [up(bad_lon), up(c12[1][2]), up(lo), up(la)]
    torch.cuda.synchronize()
    with pytest.raises(fg.FregridHipError, match="latlon2xyz") as ei:
        fg.XgridPlan.create_great_circle_lonlat_dev([12], [12], [t[0]], [t[1]], 36, 18, t[2], t[3])
    assert ei.value.code == -1
    good = fg.XgridPlan.create_great_circle_lonlat([src], dst)
    ref = fg.XgridPlan.create_great_circle([src], dst)
    a, b = good.get_xgrid(), ref.get_xgrid()
    good.destroy(); ref.destroy()
    assert len(a["area"]) == len(b["area"]) > 0 and np.array_equal(a["i_out"], b["i_out"]) and np.array_equal(_bits(a["area"]), _bits(b["area"]))
