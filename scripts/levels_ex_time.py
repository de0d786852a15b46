"""Times of the many-level sweep with options against the per-level loop it replaces.

  kernel    C384 -> 1440 x 720, 8 levels, a land mask that grows with depth (scripts/masked_levels_time.py's):
              order 2, meas            cell_measures, one area for all levels
              order 2, meas_z_target   cell_measures with an area per level, --target_grid
              order 1, sum             cell_methods = sum
            loop      8 x fg_plan_apply_ex(has_missing, nz = 1) with the options
            levels    fg_plan_apply_levels_ex on level-major fields (order 2: gradients and masks as the loop takes them)
            records   fg_plan_apply_records_levels_ex on records made once outside the clock (order 2)
  streamed  tripolar 1440 x 1080 -> C384 (6 plans), order 1, NC_FLOAT in and out, 50 levels from page-locked memory, meas:
            loop      per level: upload, fg_dev_widen, fg_plan_apply_ex per plan, fg_dev_narrow, download
            levels    fg_sweep_run_levels_ex
The loop legs use only entry points older than the batched ones, and the batched legs are left out where the library lacks
them, so the same script times the loop on an older build.  Every figure is a host clock around `reps` repetitions that end
in a synchronise, after warm-up; the legs alternate; best and worst round are printed (their ratio is the run-to-run spread).
One JSON line per part.

  python scripts/levels_ex_time.py [--part kernel|streamed|all] [--reps N]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from masked_levels_time import MISSING, land_mask, timed      # noqa: E402

AREA_MISSING = -9.0e15


def alternate(cands, sync, reps, rounds=5):
    """{name: fn} -> {name: (best ms, worst ms) over the rounds}, the candidates taking turns"""
    for fn in cands.values():
        for _ in range(3):
            fn()
    seen = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            seen[k].append(timed(fn, sync, reps))
    return {k: (min(v), max(v)) for k, v in seen.items()}


def report(best):
    return {k: {"best_ms": round(b, 4), "worst_ms": round(w, 4)} for k, (b, w) in best.items()}


def kernel_part(fg, torch, reps):
    ni, nlon, nlat, nlev = 384, 1440, 720, 8
    dev = "cuda:0"
    lon, lat, lont, latt = fg.gnomonic_ed_grid(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    ncell, ndst = 6 * ni * ni, nlon * nlat
    prep = fg.C2lPrep([ni] * 6, [ni] * 6, lon, lat, lont, latt, fg.find_contacts([ni] * 6, [ni] * 6, lon, lat))
    mask = land_mask(np.asarray(lont).reshape(-1), np.asarray(latt).reshape(-1), nlev)
    rng = np.random.default_rng(1)
    src = 280.0 + 20.0 * rng.standard_normal((nlev, ncell))
    src[mask] = MISSING
    src_t = torch.from_numpy(src).to(dev)
    fa1 = rng.uniform(0.5e-4, 2e-4, ncell)
    faz = fa1[None, :] * rng.uniform(0.5, 1.5, (nlev, ncell))
    faz[mask & (rng.random((nlev, ncell)) < 0.3)] = AREA_MISSING                  # legal: only under missing data
    fa1_t, faz_t = torch.from_numpy(fa1).to(dev), torch.from_numpy(faz).to(dev)
    cao_t = torch.from_numpy(rng.uniform(0.5e-4, 2e-4, ndst)).to(dev)
    res = {"workload": f"C{ni} -> {nlon}x{nlat}, {nlev} levels, land fraction {mask.mean():.3f}", "unit": "ms per 8 levels"}
    work = (("order2_meas", 2, dict(field_area_t=fa1_t), False), ("order2_meas_z_target", 2, dict(field_area_t=faz_t, cell_area_out_t=cao_t), True),
            ("order1_sum", 1, dict(cell_methods_sum=True), False))
    plans = {}
    for name, order, opts, per_level in work:
        if order not in plans:
            p = fg.XgridPlan.create(order, [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)], fg.GridConfig(nlon, nlat, lo, la))
            p.finalize(); p.sync()
            plans[order] = p
        plan = plans[order]
        common = dict(has_missing=True, missing=MISSING, area_missing=AREA_MISSING)
        out = torch.empty(nlev, ndst, dtype=torch.float64, device=dev)
        out2 = torch.empty(nlev, ndst, dtype=torch.float64, device=dev)
        batched = hasattr(plan, "apply_levels_ex")
        if order == 2:
            prep.set_stream(plan.stream())
            halo = torch.empty(nlev, prep.F, dtype=torch.float64, device=dev)
            gx = torch.empty(nlev, ncell, dtype=torch.float64, device=dev); gy = torch.empty_like(gx)
            gm = torch.empty(nlev, ncell, dtype=torch.int32, device=dev)
            rec = torch.empty(ncell, 3, 8, dtype=torch.float64, device=dev)
            bits = torch.empty(ncell, dtype=torch.uint8, device=dev)
            prep.fill_halo(src_t, halo, nlev); prep.gradient(halo, nlev, gx, gy, gm, True, MISSING)
            prep.records_levels(src_t, nlev, MISSING, rec, bits); plan.sync()
            data, grads = halo, lambda k: dict(grad_x_t=gx[k], grad_y_t=gy[k], grad_mask_t=gm[k])
        else:
            data, grads = src_t, lambda k: {}

        def loop(plan=plan, data=data, grads=grads, opts=opts, per_level=per_level, out=out):
            for k in range(nlev):
                o = dict(opts, field_area_t=opts["field_area_t"][k]) if per_level else opts
                plan.apply_ex(data[k], out[k], nz=1, **grads(k), **common, **o)
        cands = {"loop_8x_apply_ex": loop}
        same = None
        if batched:
            def levels(plan=plan, data=data, opts=opts, per_level=per_level, out2=out2, order=order):
                g = (gx, gy, gm) if order == 2 else (None, None, None)
                plan.apply_levels_ex(data, out2, nlev, *g, field_area_per_level=per_level, **common, **opts)
            cands["apply_levels_ex"] = levels
            loop(); levels(); plan.sync()
            same = bool(torch.equal(out.view(torch.int64), out2.view(torch.int64)))
            if order == 2:
                def records(plan=plan, opts=opts, per_level=per_level, out2=out2):
                    plan.apply_records_levels_ex(nlev, rec, bits, out2, field_area_per_level=per_level, **common, **opts)
                cands["apply_records_levels_ex"] = records
                records(); plan.sync()
                same = same and bool(torch.equal(out.view(torch.int64), out2.view(torch.int64)))
        res[name] = dict(report(alternate(cands, plan.sync, reps)), bits_equal_to_loop=same, nxgrid=plan.nxgrid)
    for p in plans.values():
        p.destroy()
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
        p = fg.XgridPlan.create(1, gin, fg.GridConfig(no, no, lon_d[t], lat_d[t])); p.finalize(); p.sync(); plans.append(p)
    ncin, ndst = nxs * nys, no * no
    lonc = 0.25 * (lon_s[:-1, :-1] + lon_s[1:, :-1] + lon_s[:-1, 1:] + lon_s[1:, 1:]).reshape(-1)
    latc = 0.25 * (lat_s[:-1, :-1] + lat_s[1:, :-1] + lat_s[:-1, 1:] + lat_s[1:, 1:]).reshape(-1)
    m8 = land_mask(lonc, latc, 8)
    hin = fg.HostBuffer((nlev, ncin), np.float32)
    rng = np.random.default_rng(2)
    for k in range(nlev):
        hin.array[k] = (280.0 + 20.0 * rng.standard_normal(ncin)).astype(np.float32)
        hin.array[k][m8[min(k * 8 // nlev, 7)]] = MISSING
    houts = [fg.HostBuffer((nlev, ndst), np.float32) for _ in range(6)]
    hloop = [fg.HostBuffer((nlev, ndst), np.float32) for _ in range(6)]
    sw = fg.Sweep(plans, None, np.float32, np.float32)
    dev = "cuda:0"
    fa_t = torch.from_numpy(rng.uniform(0.5e-4, 2e-4, ncin)).to(dev)
    d_raw = torch.empty(ncin, dtype=torch.float32, device=dev); d_f64 = torch.empty(ncin, dtype=torch.float64, device=dev)
    d_out = torch.empty(ndst, dtype=torch.float64, device=dev); d_fin = torch.empty(ndst, dtype=torch.float32, device=dev)
    nc_float = fg.field_io.nc_type_of(np.float32)
    vp, zero, miss = C.c_void_p, C.c_double(0.0), C.c_double(MISSING)
    opts = dict(has_missing=True, missing=MISSING, field_area_t=fa_t, area_missing=AREA_MISSING)

    def loop():
        for k in range(nlev):
            L.fg_dev_upload(vp(d_raw.data_ptr()), vp(hin.array[k].ctypes.data), ncin * 4)
            L.fg_dev_widen(C.c_int(nc_float), C.c_long(ncin), vp(d_raw.data_ptr()), zero, zero, miss, vp(d_f64.data_ptr()))
            for p, h in zip(plans, hloop):
                p.apply_ex(d_f64, d_out, nz=1, **opts); p.sync()
                L.fg_dev_narrow(C.c_int(nc_float), C.c_long(ndst), vp(d_out.data_ptr()), zero, zero, miss, vp(d_fin.data_ptr()))
                L.fg_dev_download(vp(h.array[k].ctypes.data), vp(d_fin.data_ptr()), ndst * 4)
    cands = {"per_level_loop": loop}
    same = None
    if hasattr(sw, "run_levels_ex"):
        def levels():
            sw.run_levels_ex(hin.array, [h.array for h in houts], **opts)
        cands["sweep_run_levels_ex"] = levels
        loop(); levels()
        same = all(np.array_equal(a.array.view(np.uint32), b.array.view(np.uint32)) for a, b in zip(houts, hloop))
    best = alternate(cands, torch.cuda.synchronize, max(reps // 50, 2), rounds=3)
    res = {"workload": f"tripolar {nxs}x{nys} -> C{no} (6 tiles), order 1, NC_FLOAT, {nlev} levels, meas, land fraction "
                       f"{float(np.mean(hin.array == MISSING)):.3f}", "unit": "ms per 50 levels", **report(best), "bits_equal_to_loop": same}
    sw.destroy()
    for h in [hin] + houts + hloop:
        h.free()
    for p in plans:
        p.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["kernel", "streamed", "all"])
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    fg = g.load_package()
    fg._lib.require_gpu()
    if a.part in ("kernel", "all"):
        print(json.dumps({"part": "kernel", **kernel_part(fg, torch, a.reps)}), flush=True)
    if a.part in ("streamed", "all"):
        print(json.dumps({"part": "streamed", **streamed_part(fg, torch, a.reps)}), flush=True)


if __name__ == "__main__":
    main()
