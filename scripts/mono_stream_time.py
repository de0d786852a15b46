"""Times of the monotone limiter on the gradient object's records and in the streamed sweep against what they replace
(DESIGN.md sections 3.3 and 3.5).

  resident  C384 -> 1440 x 720, order 2, 8 levels of +-uniform(1, 10) under a land mask that grows with depth
            (scripts/masked_levels_time.py's), from the unpadded levels on the device, with and without cell_measures:
              loop      fg_c2l_fill_halo + fg_c2l_gradient + 8 x fg_plan_apply_ex(monotonic, nz = 1)
              levels    fg_c2l_fill_halo + fg_c2l_gradient + fg_plan_apply_levels_mono
              records   fg_c2l_records_levels_mono + fg_plan_apply_records_levels_mono
  streamed  tripolar 1440 x 1080 -> C384 (6 plans), order 2, NC_FLOAT in and out, 50 levels from page-locked memory, `none` and `meas`;
            the source grid is one tile without contacts, so every halo element holds init_halo's zero:
              loop      per level: upload, fg_dev_widen, fg_c2l_fill_halo, fg_c2l_gradient, then per plan fg_plan_apply_ex(monotonic),
                        fg_dev_narrow, download
              sweep     fg_sweep_run_levels_mono
The loop legs use only entry points older than the new ones, and the new legs are left out where the library lacks them, so the
same script times the loops on an older build.  Every figure is a host clock around `reps` repetitions that end in a synchronise,
after warm-up; the legs alternate over five rounds; best and worst round are printed (their ratio is the run-to-run spread).  The
timed outputs are asserted bit-identical first.  One JSON line per part.

  python scripts/mono_stream_time.py [--part resident|streamed|all] [--reps N]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from masked_levels_time import MISSING, land_mask      # noqa: E402
from levels_ex_time import alternate, report           # noqa: E402


def _same(torch, a, b):
    return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


def resident_part(fg, torch, reps):
    ni, nlon, nlat, nlev = 384, 1440, 720, 8
    dev = "cuda:0"
    lon, lat, lont, latt = fg.gnomonic_ed_grid(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    ncell, ndst = 6 * ni * ni, nlon * nlat
    prep = fg.C2lPrep([ni] * 6, [ni] * 6, lon, lat, lont, latt, fg.find_contacts([ni] * 6, [ni] * 6, lon, lat))
    plan = fg.XgridPlan.create(2, [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)], fg.GridConfig(nlon, nlat, lo, la))
    plan.finalize(); plan.sync()
    prep.set_stream(plan.stream())
    m8 = land_mask(np.asarray(lont).reshape(-1), np.asarray(latt).reshape(-1), 8)
    rng = np.random.default_rng(3)
    fa_t = torch.from_numpy(rng.uniform(0.5e-4, 2e-4, ncell)).to(dev)
    src = rng.choice([-1.0, 1.0], (nlev, ncell)) * rng.uniform(1.0, 10.0, (nlev, ncell))
    for k in range(nlev):
        src[k][m8[k]] = MISSING
    src_t = torch.from_numpy(src).to(dev)
    halo = torch.empty(nlev, prep.F, dtype=torch.float64, device=dev)
    gx = torch.empty(nlev, ncell, dtype=torch.float64, device=dev); gy = torch.empty_like(gx)
    gm = torch.empty(nlev, ncell, dtype=torch.int32, device=dev)
    rec = torch.empty(ncell, 3, 8, dtype=torch.float64, device=dev)
    bits = torch.empty(ncell, dtype=torch.uint8, device=dev)
    b8 = torch.empty(ncell, 4, 8, dtype=torch.float64, device=dev)
    outs = {k: torch.empty(nlev, ndst, dtype=torch.float64, device=dev) for k in ("loop", "levels", "records")}
    torch.cuda.synchronize()
    res = {"workload": f"C{ni} -> {nlon}x{nlat}, order 2, monotone limiter, {nlev} levels from the unpadded field, land fraction {m8.mean():.3f}",
           "unit": "ms per 8 levels, preparation included", "nxgrid": plan.nxgrid, "reps": reps}

    def prepare():
        prep.fill_halo(src_t, halo, nlev)
        prep.gradient(halo, nlev, gx, gy, gm, True, MISSING)

    for name, opts in (("none", {}), ("meas", dict(field_area_t=fa_t))):
        common = dict(has_missing=True, missing=MISSING, **opts)

        def loop():
            prepare()
            for k in range(nlev):
                plan.apply_ex(halo[k], outs["loop"][k], nz=1, grad_x_t=gx[k], grad_y_t=gy[k], grad_mask_t=gm[k], monotonic=True, **common)
        cands = {"prepare_loop_apply_ex": loop}
        same = {}
        loop(); plan.sync()
        if hasattr(plan, "apply_levels_mono"):
            def levels():
                prepare()
                plan.apply_levels_mono(halo, outs["levels"], nlev, gx, gy, gm, **common)
            cands["prepare_apply_levels_mono"] = levels
            levels(); plan.sync()
            same["levels"] = _same(torch, outs["loop"], outs["levels"])
        if hasattr(plan, "apply_records_levels_mono"):
            def records():
                prep.records_levels_mono(src_t, nlev, MISSING, rec, bits, b8)
                plan.apply_records_levels_mono(nlev, rec, bits, b8, outs["records"], **common)

            def records_sweep_only():                     # the bounds are spent after one call: reset the extremes, sweep again
                plan.mono_records_reset(b8)
                plan.apply_records_levels_mono(nlev, rec, bits, b8, outs["records"], **common)
            cands["records_levels_mono"] = records
            cands["reset_and_apply_records_levels_mono"] = records_sweep_only
            records(); plan.sync()
            same["records"] = _same(torch, outs["loop"], outs["records"])
            outs["records"].zero_(); torch.cuda.synchronize()
            records_sweep_only(); plan.sync()
            same["records_after_reset"] = _same(torch, outs["loop"], outs["records"])
        assert all(same.values()), same
        res[name] = dict(report(alternate(cands, plan.sync, reps)), bits_equal_to_loop=same)
    plan.destroy()
    prep.destroy()
    return res


def streamed_part(fg, torch, reps):
    nxs, nys, no, nlev = 1440, 1080, 384, 50
    L = fg.lib()
    lon_s, lat_s = fg.tripolar_corners(nxs, nys)
    lon_d, lat_d = fg.gnomonic_ed_corners(no)
    gin = [fg.GridConfig(nxs, nys, lon_s, lat_s)]
    plans = []
    for t in range(6):
        p = fg.XgridPlan.create(2, gin, fg.GridConfig(no, no, lon_d[t], lat_d[t])); p.finalize(); p.sync(); plans.append(p)
    ncin, ndst = nxs * nys, no * no
    lonc = 0.25 * (lon_s[:-1, :-1] + lon_s[1:, :-1] + lon_s[:-1, 1:] + lon_s[1:, 1:])
    latc = 0.25 * (lat_s[:-1, :-1] + lat_s[1:, :-1] + lat_s[:-1, 1:] + lat_s[1:, 1:])
    none = {k: np.zeros(0, dtype=np.int32) for k in ("tile1", "tile2", "istart1", "iend1", "jstart1", "jend1", "istart2", "iend2", "jstart2", "jend2")}
    prep = fg.C2lPrep([nxs], [nys], [lon_s], [lat_s], [lonc], [latc], none)
    m8 = land_mask(lonc.reshape(-1), latc.reshape(-1), 8)
    hin = fg.HostBuffer((nlev, ncin), np.float32)
    rng = np.random.default_rng(2)
    for k in range(nlev):
        hin.array[k] = (rng.choice([-1.0, 1.0], ncin) * rng.uniform(1.0, 10.0, ncin)).astype(np.float32)
        hin.array[k][m8[min(k * 8 // nlev, 7)]] = MISSING
    houts = [fg.HostBuffer((nlev, ndst), np.float32) for _ in range(6)]
    hloop = [fg.HostBuffer((nlev, ndst), np.float32) for _ in range(6)]
    sw = fg.Sweep(plans, prep, np.float32, np.float32)
    dev = "cuda:0"
    fa_t = torch.from_numpy(rng.uniform(0.5e-4, 2e-4, ncin)).to(dev)
    d_raw = torch.empty(ncin, dtype=torch.float32, device=dev); d_f64 = torch.empty(1, ncin, dtype=torch.float64, device=dev)
    halo = torch.empty(1, prep.F, dtype=torch.float64, device=dev)
    gx = torch.empty(1, ncin, dtype=torch.float64, device=dev); gy = torch.empty_like(gx)
    gm = torch.empty(1, ncin, dtype=torch.int32, device=dev)
    d_out = torch.empty(ndst, dtype=torch.float64, device=dev); d_fin = torch.empty(ndst, dtype=torch.float32, device=dev)
    nc_float = fg.field_io.nc_type_of(np.float32)
    vp, zero, miss = C.c_void_p, C.c_double(0.0), C.c_double(MISSING)
    res = {"workload": f"tripolar {nxs}x{nys} -> C{no} (6 tiles), order 2, monotone limiter, NC_FLOAT, {nlev} levels, land fraction "
                       f"{float(np.mean(hin.array == MISSING)):.3f}", "unit": "ms per 50 levels", "nxgrid": sum(p.nxgrid for p in plans)}
    for name, extra in (("none", {}), ("meas", dict(field_area_t=fa_t))):
        opts = dict(has_missing=True, missing=MISSING, **extra)

        def loop():
            for k in range(nlev):
                L.fg_dev_upload(vp(d_raw.data_ptr()), vp(hin.array[k].ctypes.data), ncin * 4)
                L.fg_dev_widen(C.c_int(nc_float), C.c_long(ncin), vp(d_raw.data_ptr()), zero, zero, miss, vp(d_f64.data_ptr()))
                prep.fill_halo(d_f64, halo, 1)
                prep.gradient(halo, 1, gx, gy, gm, True, MISSING)
                prep.sync()
                for p, h in zip(plans, hloop):
                    p.apply_ex(halo[0], d_out, nz=1, grad_x_t=gx[0], grad_y_t=gy[0], grad_mask_t=gm[0], monotonic=True, **opts); p.sync()
                    L.fg_dev_narrow(C.c_int(nc_float), C.c_long(ndst), vp(d_out.data_ptr()), zero, zero, miss, vp(d_fin.data_ptr()))
                    L.fg_dev_download(vp(h.array[k].ctypes.data), vp(d_fin.data_ptr()), ndst * 4)
        cands = {"per_level_loop": loop}
        same = None
        loop()
        if hasattr(sw, "run_levels_mono"):
            def sweep():
                sw.run_levels_mono(hin.array, [h.array for h in houts], **opts)
            cands["sweep_run_levels_mono"] = sweep
            sweep()
            same = all(np.array_equal(a.array.view(np.uint32), b.array.view(np.uint32)) for a, b in zip(houts, hloop))
            assert same, "the streamed sweep differs from the per-level chain"
        # (the gradient of a tripolar grid taken as one cubed-sphere tile is not finite everywhere: counted, not hidden)
        nonfinite = float(np.mean([np.mean(~np.isfinite(a.array)) for a in hloop]))
        res[name] = dict(report(alternate(cands, torch.cuda.synchronize, max(reps // 50, 2), rounds=5)), bits_equal_to_loop=same,
                         nonfinite_output_fraction=nonfinite)
    sw.destroy()
    for h in [hin] + houts + hloop:
        h.free()
    for p in plans:
        p.destroy()
    prep.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["resident", "streamed", "all"])
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    fg = g.load_package()
    fg._lib.require_gpu()
    if a.part in ("resident", "all"):
        print(json.dumps({"part": "resident", **resident_part(fg, torch, a.reps)}), flush=True)
    if a.part in ("streamed", "all"):
        print(json.dumps({"part": "streamed", **streamed_part(fg, torch, a.reps)}), flush=True)


if __name__ == "__main__":
    main()
