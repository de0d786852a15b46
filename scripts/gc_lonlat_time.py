"""Time the great-circle search from lon / lat by three routes, and k_latlon2xyz alone.
usage: python scripts/gc_lonlat_time.py [--runs 13] [--cases 384:1440:720,768:2880:1440] [--kernel-only] [--ab-lib LIB.so] [--out FILE.md]
The kernel reads its sin/cos table from global memory; for the variant that keeps a copy in LDS build
  scripts/exp_build.sh 1 latlon2xyz_kernels.hip -DFG_LL2X_TAB_LDS=1
and pass --ab-lib fre-nctools_amd/libfregrid_hip_exp1.so: the kernel of that library is then timed beside the product's, the two
alternating launch by launch in this process.

Routes to a finished search (plan created, stream drained), alternated run by run, median reported:
  (a) fg_plan_create_great_circle            host fg_latlon2xyz + upload of the unit vectors + search (the route before the device
                                             conversion existed; this entry point is unchanged)
  (b) fg_plan_create_great_circle_lonlat     upload of lon / lat + conversion on the device + search
  (c) fg_plan_create_great_circle_lonlat_dev lon / lat already on the device; wall time and HIP events on the plan's stream
The three plans of the last run are compared (lists and area bits) so that a timing of different work cannot pass unnoticed."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from conftest import load_package

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=13)
ap.add_argument("--cases", default="384:1440:720,768:2880:1440")
ap.add_argument("--out", default="")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--ab-lib", default="")
args = ap.parse_args()
assert args.runs >= 11
fg = load_package()
dev = "cuda:0"
med = lambda v: float(np.median(v))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def kernel_alone(lon_t, lat_t, libs):
    """libs: {label: library}.  Per library the median over runs of: one launch (events around it), and 10 launches back to back / 10;
    the libraries alternate run by run.  Returns {label: (one, ten, (x, y, z))}."""
    import ctypes as C
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    res = {k: ([], [], tuple(torch.empty_like(lon_t) for _ in range(3))) for k in libs}
    for L in libs.values():
        L.fg_dev_latlon2xyz.argtypes = [C.c_long, vp, vp, vp, vp, vp, C.c_int, vp]
        L.fg_dev_latlon2xyz.restype = C.c_int
    for _ in range(args.runs + 2):
        for k, L in libs.items():
            one, ten, out = res[k]
            conv = lambda: L.fg_dev_latlon2xyz(lon_t.numel(), vp(lon_t.data_ptr()), vp(lat_t.data_ptr()), *[vp(v.data_ptr()) for v in out], 0, st)
            e0.record(); rc = conv(); e1.record(); e1.synchronize()
            assert rc == 0
            one.append(e0.elapsed_time(e1))
            e0.record()
            for _ in range(10):
                conv()
            e1.record(); e1.synchronize()
            ten.append(e0.elapsed_time(e1) / 10)
    return {k: (med(v[0][2:]), med(v[1][2:]), v[2]) for k, v in res.items()}


for case in args.cases.split(","):
    ni, nlon, nlat = (int(v) for v in case.split(":"))
    lon, lat = fg.gnomonic_ed_corners(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    grids = [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]
    gout = fg.GridConfig(nlon, nlat, lo, la)
    nvert = 6 * (ni + 1) ** 2 + (nlon + 1) * (nlat + 1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(dev)
    lon_t, lat_t, lo_t, la_t = [up(lon[t]) for t in range(6)], [up(lat[t]) for t in range(6)], up(lo), up(la)
    all_lon, all_lat = torch.cat(lon_t + [lo_t]), torch.cat(lat_t + [la_t])
    stream = torch.cuda.Stream()                          # route (c) runs on it, so that events can bracket its device work
    torch.cuda.synchronize()
    libs = {"product library (table in global memory)": fg.lib()}
    if args.ab_lib:
        import ctypes
        libs["--ab-lib " + os.path.basename(args.ab_lib)] = ctypes.CDLL(os.path.abspath(args.ab_lib))
    hxyz = fg.latlon2xyz(np.concatenate([np.ravel(v) for v in list(lon) + [lo]]), np.concatenate([np.ravel(v) for v in list(lat) + [la]]))
    say(f"### C{ni} -> {nlon}x{nlat}: k_latlon2xyz alone, {nvert} corners (median of {args.runs} alternating runs)")
    say("")
    say("| library | one launch us | 10 back to back, per launch us | bits of the host fg_latlon2xyz |")
    say("|---|---|---|---|")
    for k, (k1, k10, out) in kernel_alone(all_lon, all_lat, libs).items():
        kernel_bits = all(np.array_equal(d.cpu().numpy().view(np.uint64), h.view(np.uint64)) for d, h in zip(out, hxyz))
        say(f"| {k} | {1e3 * k1:.1f} | {1e3 * k10:.1f} | {kernel_bits} |")
        assert kernel_bits
    say("")
    if args.kernel_only:
        continue
    wall = {"a": [], "b": [], "c": []}
    ev_c = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    last = {}
    for run in range(args.runs + 2):                      # the first two runs warm the pools and are dropped
        for route in ("a", "b", "c"):
            t0 = time.perf_counter()
            if route == "a":
                plan = fg.XgridPlan.create_great_circle(grids, gout)
            elif route == "b":
                plan = fg.XgridPlan.create_great_circle_lonlat(grids, gout)
            else:
                e0.record(stream)
                plan = fg.XgridPlan.create_great_circle_lonlat_dev([ni] * 6, [ni] * 6, lon_t, lat_t, nlon, nlat, lo_t, la_t,
                                                                   stream=stream.cuda_stream)
                e1.record(stream)
            plan.sync()
            t1 = time.perf_counter()
            if route == "c":
                e1.synchronize()
                ev = e0.elapsed_time(e1)
            if run >= 2:
                wall[route].append(1e3 * (t1 - t0))
                if route == "c":
                    ev_c.append(ev)
            if run == args.runs + 1:
                plan.finalize()
                last[route] = plan.get_xgrid()
            plan.destroy()
    same = all(len(last["a"]["area"]) == len(last[r]["area"]) and
               all(np.array_equal(last["a"][k], last[r][k]) for k in ("t_in", "i_in", "j_in", "i_out", "j_out")) and
               np.array_equal(last["a"]["area"].view(np.uint64), last[r]["area"].view(np.uint64)) for r in ("b", "c"))
    say(f"### C{ni} -> {nlon}x{nlat}  ({nvert} corners, nxgrid {len(last['a']['area'])}, median of {args.runs} alternating runs)")
    say("")
    say("| route to a finished search | wall ms | HIP events ms |")
    say("|---|---|---|")
    say(f"| (a) host fg_latlon2xyz + xyz upload + search (`fg_plan_create_great_circle`) | {med(wall['a']):.2f} | - |")
    say(f"| (b) lon/lat upload + device conversion + search (`..._lonlat`) | {med(wall['b']):.2f} | - |")
    say(f"| (c) device lon/lat, conversion + search (`..._lonlat_dev`) | {med(wall['c']):.2f} | {med(ev_c):.2f} |")
    say("")
    say(f"plans of the three routes identical: {same}; (b) below (a): {med(wall['b']) < med(wall['a'])}")
    say("")
    assert same

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
