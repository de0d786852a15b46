"""BASELINE.json configs 4 and 5 at full size on the device, checked through size-independent properties plus oracle
parity on sampled source rows (the brute-force oracle cannot finish these sizes; great-circle areas of those rows to 1e-10 and
98 % in bits against the plain oracle, all of them in bits against the oracle's _cr build, see test_gpu_great_circle.py):
  config 4a  C768 -> 2880x1440, great-circle clip, first order, write the remap file (order 2 + great circle is rejected
             by the reference itself, fregrid.c:763 -- SURVEY §8d)
  config 4b  C768 -> 2880x1440, legacy clip, second order (the order-2 half of config 4)
  config 5   tripolar 1440x1080 -> C384 mosaic (six destination tiles), first order, cached remap files read back,
             3-D field sweep through the READ-branch plans"""
import os

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
R = 6371000.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_config4_c768_great_circle_full_size(fg, gpu_ok, tmp_path):
    import torch
    ni, nlon, nlat = 768, 2880, 1440
    lon, lat = fg.gnomonic_ed_corners(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    grids = [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]
    plan = fg.XgridPlan.create_great_circle(grids, fg.GridConfig(nlon, nlat, lo, la))
    st = plan.stats()
    assert st["borderline"] == 0
    plan.finalize()
    x = plan.get_xgrid()
    n = plan.nxgrid
    assert 16_000_000 < n < 17_500_000                      # ~16.7 M (4.02 x the C384 count)
    s = x["t_in"].astype(np.int64) * ni * ni + x["j_in"].astype(np.int64) * ni + x["i_in"]
    d = x["j_out"].astype(np.int64) * nlon + x["i_out"]
    assert np.all(np.diff(s * (nlon * nlat) + d) > 0)       # canonical order, no duplicates
    assert abs(x["area"].sum() / (4 * np.pi * R * R) - 1) < 5e-9
    a_in, a_out = plan.get_cell_area(nlon * nlat)
    # great-circle cells tile the sphere, so exchange cells cover each source cell and each destination cell.  The
    # spherical-excess formula itself is only good to ~1e-16/cell-size^2 (1e-7 relative for 13 km cells), which is the
    # reference's own noise floor -- hence the loose bound; the sampled rows below are compared exactly.
    cov_s = np.bincount(s, weights=x["area"], minlength=6 * ni * ni)
    assert np.max(np.abs(cov_s / a_in - 1)) < 5e-5
    cov_d = np.bincount(d, weights=x["area"], minlength=nlon * nlat)
    assert np.max(np.abs(cov_d / a_out - 1)) < 5e-5
    # oracle parity on one equatorial and one polar source row (brute force against all 4.1 M destination cells)
    for t, j0 in ((0, ni // 2), (2, 0)):
        o = orc.orc_create_xgrid_gc(ni, ni, nlon, nlat, lon[t], lat[t], lo, la, j1_beg=j0, j1_end=j0 + 1, capacity=200000)
        sel = (x["t_in"] == t) & (x["j_in"] == j0)
        assert sel.sum() == o["n"] > 0
        for k in ("i_in", "i_out", "j_out"):
            assert np.array_equal(x[k][sel], o[k]), k
        assert np.max(np.abs(x["area"][sel] - o["area"]) / o["area"]) < 1e-10
        assert np.mean(_bits(x["area"][sel]) == _bits(o["area"])) > 0.98
        # every area of the row in bits against the oracle that rounds like the device (gc_oracle.c's _cr build).  The lists are
        # the plain build's (asserted above, and the two builds' lists are identical), so the _cr build clips the listed pairs
        # one by one: a second brute-force search of the row costs 50 s of CPU, these a fraction of a second
        acr = orc.orc_gc_pair_areas(ni, lon[t], lat[t], nlon, lo, la, o["i_in"], o["j_in"], o["i_out"], o["j_out"], cr=True)
        nd = int(np.count_nonzero(_bits(x["area"][sel]) != _bits(acr)))
        assert nd == 0, f"tile {t} row {j0}: {nd} of {o['n']} exchange-cell areas differ from the _cr oracle"
    # first-order sweep on the great-circle plan: constants preserved, conservation
    dev = "cuda:0"
    data = torch.full((2, 6 * ni * ni), 3.25, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()                   # (filled on torch's stream; the library works on the plan's own)
    data[1] = torch.from_numpy(np.random.default_rng(0).standard_normal(6 * ni * ni) + 4.0).to(dev)
    out = torch.empty(2, nlon * nlat, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    gs = plan.apply(data, out, nz=2, want_gsum=True)
    plan.sync()
    o2 = out.cpu().numpy()
    assert np.max(np.abs(o2[0] - 3.25)) < 1e-13
    ref_sum = 3.25 * x["area"].sum() + float(np.sum(data[1].cpu().numpy()[s] * x["area"]))
    assert abs(gs - ref_sum) < 1e-11 * abs(ref_sum)
    # write the remap file (fregrid --remap_file, conserve_interp.c:368-445) and read it back
    path = os.path.join(str(tmp_path), "remap_C768_2880x1440_gc.nc")
    fg.write_remap_file(path, 1, x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"])
    y = fg.read_remap_file(path, 1)
    for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(y[k], x[k]), k
    assert np.max(np.abs(y["area"] - x["area"]) / x["area"]) < 1e-15      # stored as area/(4 pi R^2)... and back
    plan.destroy()


def test_config5_tripolar_to_c384_cached_remap_and_3d_sweep(fg, gpu_ok, tmp_path):
    import torch
    nx, ny, ni, nz = 1440, 1080, 384, 50
    tlon, tlat = fg.tripolar_corners(nx, ny)
    lon, lat = fg.gnomonic_ed_corners(ni)
    grid_in = [fg.GridConfig(nx, ny, tlon, tlat)]
    grid_out = [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]
    interp = [fg.InterpConfig(remap_file=os.path.join(str(tmp_path), f"remap.tile{t + 1}.nc")) for t in range(6)]
    fg.setup_conserve_interp(1, grid_in, 6, grid_out, interp, fg.CONSERVE_ORDER1 | fg.WRITE)
    ntot = sum(ic.nxgrid for ic in interp)
    assert ntot > 6 * ni * ni
    # exchange cells cover every atmosphere cell south of the ocean grid's northern... the ocean grid spans -82..90:
    # atmosphere cells north of 80S are fully covered
    for t in (0, 2):
        ic = interp[t]
        cov = np.bincount(ic.j_out.astype(np.int64) * ni + ic.i_out, weights=ic.area, minlength=ni * ni)
        latc = 0.25 * (lat[t][:-1, :-1] + lat[t][1:, :-1] + lat[t][:-1, 1:] + lat[t][1:, 1:]).ravel()
        inside = latc > np.radians(-75.0)
        assert np.max(np.abs(cov[inside] / grid_out[t].cell_area[inside] - 1)) < 2e-3     # legacy area model, conserve_interp.c:479
    # oracle parity on one ocean row (a fold row of the bipolar cap and a mid-latitude row) against tile 3 (north polar)
    for j0 in (ny - 1, ny // 2):
        o = orc.orc_create_xgrid(1, nx, ny, ni, ni, tlon, tlat, lon[2], lat[2], j1_beg=j0, j1_end=j0 + 1, capacity=200000)
        ic = interp[2]
        sel = ic.j_in == j0
        assert sel.sum() == o["n"]
        if o["n"]:
            for k in ("i_in", "i_out", "j_out"):
                assert np.array_equal(getattr(ic, k)[sel], o[k]), k
            assert np.max(np.abs(ic.area[sel] - o["area"]) / o["area"]) < 2e-10
            if orc.host_has_fma():
                assert np.array_equal(_bits(ic.area[sel]), _bits(o["area"]))
    # cached remap files: READ branch (conserve_interp.c:62-126) gives plans whose sweep equals the computed plans'
    interp_r = [fg.InterpConfig(remap_file=ic.remap_file, file_exist=1) for ic in interp]
    fg.setup_conserve_interp(1, grid_in, 6, grid_out, interp_r, fg.CONSERVE_ORDER1 | fg.READ)
    dev = "cuda:0"
    rng = np.random.default_rng(4)
    field = torch.from_numpy(rng.standard_normal((nz, nx * ny)) + 10.0).to(dev)      # one 3-D field, 50 levels
    gsum_in = float((field.cpu().numpy() * grid_in[0].cell_area[None, :]).sum())
    gsum_out = 0.0
    for t in range(6):
        assert interp_r[t].nxgrid == interp[t].nxgrid
        o_c = torch.empty(nz, ni * ni, dtype=torch.float64, device=dev)
        o_r = torch.empty_like(o_c)
        torch.cuda.synchronize()
        g1 = interp[t].plan.apply(field, o_c, nz=nz, want_gsum=True)
        g2 = interp_r[t].plan.apply(field, o_r, nz=nz, want_gsum=True)
        interp[t].plan.sync(); interp_r[t].plan.sync()
        a, b = o_c.cpu().numpy(), o_r.cpu().numpy()
        assert np.max(np.abs(a - b)) < 1e-12 * np.max(np.abs(a))        # areas round-trip through area/(4 pi R^2)
        assert abs(g1 - g2) < 1e-12 * abs(g1)
        gsum_out += g1
    # ocean -> atmosphere conserves the part of the ocean field that lies on the atmosphere grid (= all of it)
    assert abs(gsum_out - gsum_in) < 2e-6 * abs(gsum_in)
    for ic in interp + interp_r:
        ic.plan.destroy()


def test_config4b_c768_legacy_order2_full_size(fg, gpu_ok):
    import torch
    ni, nlon, nlat = 768, 2880, 1440
    lon, lat = fg.gnomonic_ed_corners(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    grids = [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]
    plan = fg.XgridPlan.create(2, grids, fg.GridConfig(nlon, nlat, lo, la))
    st = plan.stats()
    assert st["borderline"] == 0 and st["exact_mode"] == 0
    plan.finalize()
    x = plan.get_xgrid()
    n = plan.nxgrid
    assert 16_000_000 < n < 17_500_000
    s = x["t_in"].astype(np.int64) * ni * ni + x["j_in"].astype(np.int64) * ni + x["i_in"]
    d = x["j_out"].astype(np.int64) * nlon + x["i_out"]
    assert np.all(np.diff(s * (nlon * nlat) + d) > 0)
    assert abs(x["area"].sum() / (4 * np.pi * R * R) - 1) < 5e-9
    a_in, a_out = plan.get_cell_area(nlon * nlat)
    cov = np.bincount(d, weights=x["area"], minlength=nlon * nlat)
    assert np.max(np.abs(cov - a_out) / a_out) < 1e-4                  # conserve_interp.c:479 bound
    for arr in (x["c1"], x["c2"]):                                     # centroid distances balance per source cell
        tot = np.bincount(s, weights=arr * x["area"], minlength=6 * ni * ni)
        assert np.max(np.abs(tot)) < 1e-9 * np.max(a_in)
    # oracle parity on one polar source row (brute force over the 4.1 M destination cells)
    o = orc.orc_create_xgrid(2, ni, ni, nlon, nlat, lon[2], lat[2], lo, la, j1_beg=0, j1_end=1, capacity=200000)
    sel = (x["t_in"] == 2) & (x["j_in"] == 0)
    assert sel.sum() == o["n"] > 0
    for k in ("i_in", "i_out", "j_out"):
        assert np.array_equal(x[k][sel], o[k]), k
    assert np.max(np.abs(x["area"][sel] - o["area"]) / o["area"]) < 2e-10
    if orc.host_has_fma():
        assert np.array_equal(_bits(x["area"][sel]), _bits(o["area"]))      # bit-identical, slivers included
    # sweep: constants preserved on 4 levels
    dev = "cuda:0"
    F, ncell = 6 * (ni + 2) ** 2, 6 * ni * ni
    data = torch.full((4, F), 2.5, dtype=torch.float64, device=dev)
    z = torch.zeros(4, ncell, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()                   # (filled on torch's stream; the library works on the plan's own)
    out = torch.empty(4, nlon * nlat, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    plan.apply(data, out, nz=4, grad_x_t=z, grad_y_t=z)
    plan.sync()
    assert float((out - 2.5).abs().max()) < 1e-13
    plan.destroy()


def test_mass_gap_equals_the_references(fg, gpu_ok):
    """north_star asks for mass conserved to 1e-10; by the reference's definition (conserve_interp.c:874-907) the bench reports
    ~1e-9.  tests/test_mass_gap_reference.py computes that gap with the reference's own compiled code at C96 -> 360x180 and pins
    it; here the device path must reproduce the SAME number -- the gap belongs to the reference's exchange grid, and the remap
    itself conserves to rounding (mass_rel_err_xgrid in bench.py)."""
    import json
    from test_mass_gap_reference import GOLD, NI, NLON, NLAT, field_on_cells, gap_from
    lon, lat, lont, latt = fg.gnomonic_ed_grid(NI)
    lo, la = fg.latlon_corners(NLON, NLAT)
    plan = fg.XgridPlan.create(2, [fg.GridConfig(NI, NI, lon[t], lat[t]) for t in range(6)], fg.GridConfig(NLON, NLAT, lo, la))
    x = plan.get_xgrid()
    assert plan.nxgrid == 256864
    a_in, _ = plan.get_cell_area(NLON * NLAT)
    s_idx = x["t_in"].astype(np.int64) * NI * NI + x["j_in"].astype(np.int64) * NI + x["i_in"]
    gap, closure = gap_from(x["area"], s_idx, a_in, field_on_cells(lont, latt).ravel())
    gold = json.load(open(GOLD))
    if orc.host_has_fma():                       # areas are the reference's bits, the sums are the same numpy reductions
        assert gap == gold["gap"] and closure == gold["closure"], (gap, closure, gold)
    else:
        assert abs(gap - gold["gap"]) < 1e-3 * abs(gold["gap"])
    plan.destroy()


@pytest.mark.parametrize("ni,nlon,nlat,nexp", [(384, 1440, 720, 4160160), (768, 2880, 1440, 16674181)])
def test_great_circle_three_passes_equal_one_kernel_at_full_size(fg, gpu_ok, ni, nlon, nlat, nexp):
    """The three-pass great-circle clip against the one-kernel clip (the version pinned to the oracle) at the BASELINE sizes:
    identical exchange cells, areas bit for bit; the counts are the ones every round has measured."""
    lon, lat = fg.gnomonic_ed_corners(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    grids = [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]
    res = []
    try:
        for split in (0, 1):
            fg.lib().fg_set_gc_split(split)
            plan = fg.XgridPlan.create_great_circle(grids, fg.GridConfig(nlon, nlat, lo, la))
            plan.finalize()
            x = plan.get_xgrid()
            res.append((x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], plan.stats()))
            plan.destroy()
    finally:
        fg.lib().fg_set_gc_split(1)
    a, b = res
    assert len(a[5]) == len(b[5]) == nexp
    for k in range(5):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(_bits(a[5]), _bits(b[5]))
    assert a[6]["below"] == b[6]["below"] and b[6]["deferred"] < 0.03 * b[6]["pairs"]
