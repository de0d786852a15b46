#!/usr/bin/env python3
"""Time runoff_regrid on the device at the size it is run at: a 1 degree lat-lon source (360 x 180) onto a 0.25 degree tripolar
target (1440 x 1080 plus the southern extension row) with a synthetic 30 % land mask that includes an Antarctic cap, whose
queries lie far from any ocean point -- the worst case of the nearest search.

    python scripts/runoff_time.py [--runs 5] [--out profiles/runoff_summary.md] [--nx 1440 --ny 1080]
    python scripts/runoff_time.py --ref       (no device: needs the reference's sources; writes tests/golden/runoff_ref_nearest.json)

Setup is reported by phase (fg_runoff_phase_ms: wall time around synchronised segments; the nearest kernel alone by events).
The two modes of the nearest search (pruned / brute force, fg_set_runoff_prune) are warmed up once and then run alternately
`runs` times in one process; medians and the largest deviation from the median are reported, and the maps of the two modes
are compared.  apply is timed by events on the handle's stream around fg_runoff_apply_dev, per time level.
--ref measures the reference's nearest() (tests/capi/runoff_ref_driver.c, one CPU core) on a 64-query sample of the same grid,
every 1/64th land point, and extrapolates to all land points."""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402
import runoff_cases as rc  # noqa: E402

REF_JSON = os.path.join(ROOT, "tests", "golden", "runoff_ref_nearest.json")


def build_case(fg, nx, ny):
    lon, lat = fg.tripolar_corners(2 * nx, 2 * ny, xbnd=(-300.0, 60.0), ybnd=(-82.0, 90.0), lat_join=65.0)
    rng = np.random.default_rng(2024)
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    land = j < ny // 12                                               # the Antarctic cap: -82 to about -68
    for _ in range(10):                                               # continents: seeded blobs, periodic in x
        cj, ci, a, b = rng.uniform(0.15, 0.95) * ny, rng.uniform(0, nx), rng.uniform(0.05, 0.11) * nx, rng.uniform(0.06, 0.14) * ny
        di = np.minimum(np.abs(i - ci), nx - np.abs(i - ci))
        land |= (di / a) ** 2 + ((j - cj) / b) ** 2 <= 1
    depth = np.where(land, 0.0, 1000.0)
    data = 10.0 ** rng.uniform(-6, 6, size=(180, 360))
    c = dict(x_super=lon * rc.R2D, y_super=lat * rc.R2D, depth=depth, xt1d_in=0.5 + np.arange(360.0), yt1d_in=-89.5 + np.arange(180.0),
             data_in=data[None])
    return c


def measure_ref(args):
    fg = __graft_entry__.load_package()
    c = build_case(fg, args.nx, args.ny)
    gi, go = rc.grids_of(c)
    land = np.flatnonzero(go["mask"].ravel() == 0)
    q = land[:: max(1, land.size // 64)][:64]
    tmp = tempfile.mkdtemp(prefix="runoff_ref_")
    try:
        iq, jq, sec = rc.run_ref_nearest(rc.build_driver(tmp), tmp, gi, go, q)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res = dict(nx=args.nx, ny=args.ny, queries=int(q.size), seconds=sec, seconds_per_query=sec / q.size, land_points=int(land.size),
               seconds_all_land_points=sec / q.size * land.size, qindex=[int(v) for v in q], iq=[int(v) for v in iq], jq=[int(v) for v in jq])
    with open(REF_JSON, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("queries", "seconds", "seconds_per_query", "land_points", "seconds_all_land_points")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--ref", action="store_true")
    args = ap.parse_args()
    if args.ref:
        return measure_ref(args)
    import torch
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    c = build_case(fg, args.nx, args.ny)
    gi = fg.runoff_input_grid(c["xt1d_in"], c["yt1d_in"], c["data_in"][0], rc.MISSING)
    go = fg.runoff_output_grid(c["x_super"], c["y_super"], c["depth"], 0.0)
    nland = int((go["mask"] == 0).sum())
    lines = [f"target {go['nx']} x {go['ny']} (n_ext = {go['n_ext']}), {nland} land points ({100.0 * nland / go['mask'].size:.1f} %), "
             f"{go['mask'].size - nland} ocean points; source 360 x 180; tile = {fg.runoff_tile()} points"]

    # the whole setup through the handle's own search, once warm-up and `runs` times
    full = []
    for r in range(args.runs + 1):
        with fg.RunoffRegrid(gi, go) as h:
            if r:
                full.append(h.phase_ms())
            xg = h.xgrid()
    med = {k: float(np.median([p[k] for p in full])) for k in full[0]}
    dev = {k: float(np.max(np.abs(np.array([p[k] for p in full]) - med[k]))) for k in full[0]}
    lines.append(f"setup, pruned search, median of {args.runs} (largest deviation): " +
                 ", ".join(f"{k} {med[k]:.2f} ms ({dev[k]:.2f})" for k in ("xgrid", "convert", "nearest", "nearest_kernel", "sort_upload")))
    lines.append(f"exchange list: {xg[4].size} entries")

    # the two prune modes, alternating, on the given list
    times, maps, stats = {1: [], 0: []}, {}, {}
    for r in range(args.runs + 1):
        for prune in (1, 0):
            fg.set_runoff_prune(prune)
            with fg.RunoffRegrid(gi, go, xgrid=xg) as h:
                if r:
                    times[prune].append(h.phase_ms())
                maps[prune], stats[prune] = h.maps(), h.search_stats()
    fg.set_runoff_prune(1)
    same = bool(np.array_equal(maps[1][0], maps[0][0]) and np.array_equal(maps[1][1], maps[0][1]))
    for prune, label in ((1, "pruned"), (0, "brute force")):
        for k in ("nearest_kernel", "nearest"):
            v = np.array([p[k] for p in times[prune]])
            lines.append(f"{label}: {k} median {np.median(v):.3f} ms, largest deviation {np.max(np.abs(v - np.median(v))):.3f} ms, runs {np.round(v, 3).tolist()}")
        s = stats[prune]
        lines.append(f"{label}: tiles {s['tiles']}, visited per query mean {s['tiles_visited'] / max(1, s['queries']):.1f}, max {s['tiles_visited_max']}")
    lines.append(f"maps of the two modes identical: {same}")
    if os.path.exists(REF_JSON):
        ref = json.load(open(REF_JSON))
        if (ref["nx"], ref["ny"]) == (args.nx, args.ny):
            q = np.array(ref["qindex"])
            ok = bool(np.array_equal(maps[1][0].ravel()[q], ref["iq"]) and np.array_equal(maps[1][1].ravel()[q], ref["jq"]))
            lines.append(f"reference nearest() on one CPU core: {ref['seconds_per_query'] * 1e3:.1f} ms per query ({ref['queries']} queries), "
                         f"extrapolated to {ref['land_points']} land points: {ref['seconds_all_land_points'] / 3600:.2f} h; "
                         f"its {ref['queries']} answers equal the device's: {ok}")

    # apply per time level
    with fg.RunoffRegrid(gi, go, xgrid=xg) as h:
        d = torch.from_numpy(np.ascontiguousarray(c["data_in"][0])).cuda()
        out = torch.empty((go["ny"], go["nx"]), dtype=torch.float64, device="cuda")
        st = torch.cuda.ExternalStream(h.stream)
        torch.cuda.synchronize()
        ts = []
        for r in range(args.runs * 4 + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record()
                fg._lib.check(fg.lib().fg_runoff_apply_dev(h.handle, d.data_ptr(), out.data_ptr(), None))
                e1.record()
            e1.synchronize()
            if r >= 3:
                ts.append(e0.elapsed_time(e1))
        ts = np.array(ts)
        o, tin, tout, rate = h.apply(c["data_in"][0])
        lines.append(f"apply per time level (3 launches, events): median {np.median(ts):.3f} ms, largest deviation {np.max(np.abs(ts - np.median(ts))):.3f} ms; "
                     f"total_in {tin:g}, total_out {tout:g}, change rate {rate:g}")
    text = "\n".join("- " + l for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
