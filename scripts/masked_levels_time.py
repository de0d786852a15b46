"""Times of the masked many-level sweep against the per-level loop it replaces (DESIGN.md sections 3.3 and 3.5).

  kernel    C384 -> 1440 x 720, orders 1 and 2, 8 levels, a land mask of ~25 % that grows with depth:
              loop      8 x fg_plan_apply_ex(has_missing, nz = 1)                      (+ 8 x fg_c2l_gradient, order 2)
              levels    fg_plan_apply_levels on level-major fields, gradients and masks
              records   fg_c2l_records_levels + fg_plan_apply_records_levels           (order 2)
              plain     fg_plan_apply_records on the same levels without a mask, for orientation (order 2)
  streamed  tripolar 1440 x 1080 -> C384 (6 plans), order 1, NC_FLOAT in and out, 50 levels from page-locked memory:
              loop      per level: upload, fg_dev_widen, fg_plan_apply_ex(has_missing) per plan, fg_dev_narrow, download
              levels    fg_sweep_run_levels
Every figure is a host clock around `reps` repetitions that end in a synchronise, after warm-up; the two sides of a comparison
alternate.  Prints one JSON line per part.

  python scripts/masked_levels_time.py [--part kernel|streamed|all] [--reps N]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MISSING = -1.0e10


def land_mask(lont, latt, nlev):
    """[nlev][cells] bool: 'continents' from the cell centres, a little wider on every level (about a quarter on average)"""
    s = np.sin(3.0 * lont) * np.cos(2.0 * latt) + 0.3 * np.sin(5.0 * latt)
    q = np.quantile(s, [1.0 - (0.15 + 0.20 * k / max(nlev - 1, 1)) for k in range(nlev)])
    return np.stack([s > q[k] for k in range(nlev)])


def timed(fn, sync, reps):
    sync(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps * 1e3


def alternate(cands, sync, reps, rounds=5):
    """{name: fn} -> {name: best ms over the rounds}, the candidates taking turns"""
    for fn in cands.values():
        for _ in range(3):
            fn()
    best = {k: float("inf") for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            best[k] = min(best[k], timed(fn, sync, reps))
    return best


def kernel_part(fg, torch, reps):
    ni, nlon, nlat, nlev = 384, 1440, 720, 8
    dev = "cuda:0"
    lon, lat, lont, latt = fg.gnomonic_ed_grid(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    ncell = 6 * ni * ni
    prep = fg.C2lPrep([ni] * 6, [ni] * 6, lon, lat, lont, latt, fg.find_contacts([ni] * 6, [ni] * 6, lon, lat))
    mask = land_mask(np.asarray(lont).reshape(-1), np.asarray(latt).reshape(-1), nlev)
    rng = np.random.default_rng(1)
    src = 280.0 + 20.0 * rng.standard_normal((nlev, ncell))
    plain_t = torch.from_numpy(src).to(dev)
    src[mask] = MISSING
    src_t = torch.from_numpy(src).to(dev)
    res = {"workload": f"C{ni} -> {nlon}x{nlat}, {nlev} levels, land fraction {mask.mean():.3f}", "unit": "ms per 8 levels"}
    for order in (1, 2):
        plan = fg.XgridPlan.create(order, [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)], fg.GridConfig(nlon, nlat, lo, la))
        plan.finalize(); plan.sync()
        prep.set_stream(plan.stream())
        ndst = nlon * nlat
        out = torch.empty(nlev, ndst, dtype=torch.float64, device=dev)
        out2 = torch.empty(nlev, ndst, dtype=torch.float64, device=dev)
        if order == 2:
            halo = torch.empty(nlev, prep.F, dtype=torch.float64, device=dev)
            gx = torch.empty(nlev, ncell, dtype=torch.float64, device=dev); gy = torch.empty_like(gx)
            gm = torch.empty(nlev, ncell, dtype=torch.int32, device=dev)
            rec = torch.empty(ncell, 3, 8, dtype=torch.float64, device=dev)
            bits = torch.empty(ncell, dtype=torch.uint8, device=dev)
            prep.fill_halo(src_t, halo, nlev); prep.gradient(halo, nlev, gx, gy, gm, True, MISSING); plan.sync()

            def loop_sweep():
                for k in range(nlev):
                    plan.apply_ex(halo[k], out[k], nz=1, grad_x_t=gx[k], grad_y_t=gy[k], grad_mask_t=gm[k], has_missing=True, missing=MISSING)

            def loop_all():
                prep.fill_halo(src_t, halo, nlev)
                for k in range(nlev):
                    prep.gradient(halo[k], 1, gx[k], gy[k], gm[k], True, MISSING)
                loop_sweep()

            def levels():
                plan.apply_levels(halo, out2, nlev, MISSING, gx, gy, gm)

            def records():
                prep.records_levels(src_t, nlev, MISSING, rec, bits)
                plan.apply_records_levels(nlev, rec, bits, out2, MISSING)

            def records_sweep():
                plan.apply_records_levels(nlev, rec, bits, out2, MISSING)

            def plain():
                prep.records(plain_t, nlev, rec)
                plan.apply_records(nlev, rec, out2)
            cands = {"loop_8x_apply_ex": loop_sweep, "loop_8x_gradient_and_apply_ex": loop_all, "apply_levels": levels,
                     "records_levels_and_apply": records, "apply_records_levels_alone": records_sweep, "plain_records_and_apply": plain}
            loop_sweep(); levels(); plan.sync()
            same = bool(torch.equal(out.view(torch.int64), out2.view(torch.int64)))
            records(); plan.sync()
            same = same and bool(torch.equal(out.view(torch.int64), out2.view(torch.int64)))
        else:
            def loop_sweep():
                for k in range(nlev):
                    plan.apply_ex(src_t[k], out[k], nz=1, has_missing=True, missing=MISSING)

            def levels():
                plan.apply_levels(src_t, out2, nlev, MISSING)

            def plain():
                plan.apply(plain_t, out2, nz=nlev)
            cands = {"loop_8x_apply_ex": loop_sweep, "apply_levels": levels, "plain_apply": plain}
            loop_sweep(); levels(); plan.sync()
            same = bool(torch.equal(out.view(torch.int64), out2.view(torch.int64)))
        best = alternate(cands, plan.sync, reps)
        res[f"order{order}"] = dict({k: round(v, 4) for k, v in best.items()}, bits_equal_to_loop=same, nxgrid=plan.nxgrid)
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
    d_raw = torch.empty(ncin, dtype=torch.float32, device=dev); d_f64 = torch.empty(ncin, dtype=torch.float64, device=dev)
    d_out = torch.empty(ndst, dtype=torch.float64, device=dev); d_fin = torch.empty(ndst, dtype=torch.float32, device=dev)
    nc_float = fg.field_io.nc_type_of(np.float32)
    vp, zero, miss = C.c_void_p, C.c_double(0.0), C.c_double(MISSING)

    def loop():
        for k in range(nlev):
            L.fg_dev_upload(vp(d_raw.data_ptr()), vp(hin.array[k].ctypes.data), ncin * 4)
            L.fg_dev_widen(C.c_int(nc_float), C.c_long(ncin), vp(d_raw.data_ptr()), zero, zero, miss, vp(d_f64.data_ptr()))
            for p, h in zip(plans, hloop):
                p.apply_ex(d_f64, d_out, nz=1, has_missing=True, missing=MISSING); p.sync()
                L.fg_dev_narrow(C.c_int(nc_float), C.c_long(ndst), vp(d_out.data_ptr()), zero, zero, miss, vp(d_fin.data_ptr()))
                L.fg_dev_download(vp(h.array[k].ctypes.data), vp(d_fin.data_ptr()), ndst * 4)

    def levels():
        sw.run_levels(hin.array, [h.array for h in houts], missing=MISSING)
    loop(); levels()
    same = all(np.array_equal(a.array.view(np.uint32), b.array.view(np.uint32)) for a, b in zip(houts, hloop))
    best = alternate({"per_level_loop": loop, "sweep_run_levels": levels}, torch.cuda.synchronize, max(reps // 50, 2), rounds=3)
    pts = 6.0 * ndst * nlev
    res = {"workload": f"tripolar {nxs}x{nys} -> C{no} (6 tiles), order 1, NC_FLOAT, {nlev} levels, land fraction {float(np.mean(hin.array == MISSING)):.3f}",
           "unit": "ms per 50 levels", **{k: round(v, 3) for k, v in best.items()},
           "points_per_s_levels": pts / (best["sweep_run_levels"] * 1e-3), "points_per_s_loop": pts / (best["per_level_loop"] * 1e-3),
           "bits_equal_to_loop": same}
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
