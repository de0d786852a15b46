#!/usr/bin/env python3
"""Time remap_land's nearest-point search on the device at the size the reference's own comment worries about: the cell
centres of a C192 cubed sphere (six faces, a seeded land mask of about 40 %) as the source, every cell centre of one C384 face
as the destination.

    python scripts/rland_time.py [--runs 5] [--out profiles/rland_summary.md] [--nsrc 192 --ndst 384]
    python scripts/rland_time.py --ref       (no device: needs the reference's sources; writes tests/golden/rland_ref_nearest.json)

Create is reported by step (conversion, ordering: wall time).  `queries` is the copy and conversion of the destination
points; `wall` is the whole Python call, which adds the read-back and the host's lists to the steps.  The two modes of the
search (pruned / brute force, fg_set_rland_prune) are warmed up once and then run alternately `runs` times in one process on one handle; per step (compaction
with balls, phase 1, phase 2 by events, overflow pass, host finish) and for the whole call the median and the largest deviation
from the median are reported, and the maps of the two modes are compared.
--ref measures the reference's full_search_nearest (tests/capi/rland_ref_driver.c, one CPU core) on a 64-query sample of the
same case, every 1/64th destination point, and extrapolates to the face."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402
import rland_cases as rc  # noqa: E402

REF_JSON = os.path.join(ROOT, "tests", "golden", "rland_ref_nearest.json")


def build_case(nsrc, ndst):
    lon_src, lat_src = rc.cube_centres(nsrc)
    lon_dst, lat_dst = rc.cube_centres(ndst)
    rng = np.random.default_rng(2025)
    land = np.zeros(lon_src.shape, dtype=bool)
    x, y, z = np.cos(lat_src) * np.cos(lon_src), np.cos(lat_src) * np.sin(lon_src), np.sin(lat_src)
    for _ in range(14):                                               # continents: seeded caps of 10 to 30 degrees
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        land |= x * v[0] + y * v[1] + z * v[2] > np.cos(rng.uniform(10, 30) * np.pi / 180)
    return dict(lon_src=lon_src, lat_src=lat_src, mask_src=land.astype(np.int32), lon_dst=lon_dst[2], lat_dst=lat_dst[2],
                mask_dst=np.ones(ndst * ndst, dtype=np.int32), iface_dst=2)


def measure_ref(args):
    c = build_case(args.nsrc, args.ndst)
    n = c["lon_dst"].size
    q = np.arange(n)[:: max(1, n // 64)][:64]
    c["mask_dst"] = np.zeros(n, dtype=np.int32)
    c["mask_dst"][q] = 1
    tmp = tempfile.mkdtemp(prefix="rland_ref_")
    try:
        r = rc.run_ref(rc.build_driver(tmp), tmp, c, mode=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    sec = r["seconds"]
    res = dict(nsrc=args.nsrc, ndst=args.ndst, queries=int(q.size), seconds=sec, seconds_per_query=sec / q.size, face_points=int(n),
               seconds_whole_face=sec / q.size * n, unmasked_source_points=int(c["mask_src"].sum()), qindex=[int(v) for v in q],
               idx_map=[int(v) for v in r["idx_map"][q]], face_map=[int(v) for v in r["face_map"][q]])
    with open(REF_JSON, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("queries", "seconds", "seconds_per_query", "face_points", "seconds_whole_face")}))


def _med(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.median(v)), float(np.max(np.abs(v - np.median(v))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--nsrc", type=int, default=192)
    ap.add_argument("--ndst", type=int, default=384)
    ap.add_argument("--ref", action="store_true")
    args = ap.parse_args()
    if args.ref:
        return measure_ref(args)
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    c = build_case(args.nsrc, args.ndst)
    nun = int(c["mask_src"].sum())
    lines = [f"source C{args.nsrc} centres, 6 x {args.nsrc ** 2} points, {nun} unmasked ({100.0 * nun / c['mask_src'].size:.1f} %); "
             f"destination one C{args.ndst} face, {c['lon_dst'].size} queries; tile = {fg.rland_tile()} points, 64 tiles per group, 4 slots"]
    create = []
    for r in range(args.runs + 1):
        t0 = time.perf_counter()
        with fg.LandNearest(c["lon_src"], c["lat_src"]) as h:
            wall = (time.perf_counter() - t0) * 1e3
            if r:
                create.append(dict(h.phase_ms(), wall=wall))
    lines.append(f"create, median of {args.runs} (largest deviation): " +
                 ", ".join("{} {:.2f} ms ({:.2f})".format(k, *_med([p[k] for p in create])) for k in ("convert", "order", "wall")))
    steps = ("queries", "tiles_balls", "phase1", "phase2", "overflow", "host_finish", "wall")
    times, maps, stats = {1: [], 0: []}, {}, {}
    with fg.LandNearest(c["lon_src"], c["lat_src"]) as h:
        for r in range(args.runs + 1):
            for prune in (1, 0):
                fg.set_rland_prune(prune)
                t0 = time.perf_counter()
                maps[prune] = h.search(c["mask_src"], c["lon_dst"], c["lat_dst"], c["mask_dst"])
                wall = (time.perf_counter() - t0) * 1e3
                if r:
                    times[prune].append(dict(h.phase_ms(), wall=wall))
                stats[prune] = h.stats()
        fg.set_rland_prune(1)
        t0 = time.perf_counter()
        sf = h.search_sface(c["mask_src"], c["lon_dst"], c["lat_dst"], c["mask_dst"], maps[1][0], maps[1][1], c["iface_dst"])
        sf_wall, sf_stats = (time.perf_counter() - t0) * 1e3, h.stats()
    lines.append("| step | pruned median ms | deviation | brute force median ms | deviation |")
    lines.append("|---|---|---|---|---|")
    for k in steps:
        (m1, d1), (m0, d0) = _med([p[k] for p in times[1]]), _med([p[k] for p in times[0]])
        lines.append(f"| {k} | {m1:.3f} | {d1:.3f} | {m0:.3f} | {d0:.3f} |")
    for prune, label in ((1, "pruned"), (0, "brute force")):
        s = stats[prune]
        nq = max(1, s["queries"])
        lines.append(f"{label}: tiles {s['tiles']}, visited per query phase 1 {s['tiles_visited'] / nq:.1f}, phase 2 {s['tiles_visited_survivors'] / nq:.1f}; "
                     f"survivors per query {s['survivors'] / nq:.4f}, decided on the host {s['host_finished']}, fallback {s['fallback']}, overflow {s['overflow']}")
    (m1, d1), (m0, d0) = _med([p["wall"] for p in times[1]]), _med([p["wall"] for p in times[0]])
    lines.append(f"whole call: pruned {m1:.2f} ms, brute force {m0:.2f} ms: difference {m0 - m1:.2f} ms against twice the larger deviation {2 * max(d1, d0):.2f} ms")
    lines.append(f"maps of the two modes identical: {bool(np.array_equal(maps[1][0], maps[0][0]) and np.array_equal(maps[1][1], maps[0][1]))}")
    lines.append(f"same-face search for face {c['iface_dst']} after it (one run, pruned): {sf_stats['queries']} queries needed it, {sf_wall:.2f} ms; "
                 f"{int((sf >= 0).sum())} points mapped")
    if os.path.exists(REF_JSON):
        ref = json.load(open(REF_JSON))
        if (ref["nsrc"], ref["ndst"]) == (args.nsrc, args.ndst):
            q = np.array(ref["qindex"])
            ok = bool(np.array_equal(maps[1][0][q], ref["idx_map"]) and np.array_equal(maps[1][1][q], ref["face_map"]))
            lines.append(f"reference full_search_nearest on one CPU core: {ref['seconds_per_query'] * 1e3:.1f} ms per query ({ref['queries']} queries), "
                         f"extrapolated to the face's {ref['face_points']} points: {ref['seconds_whole_face'] / 60:.1f} min; "
                         f"its {ref['queries']} answers equal the device's: {ok}")
    text = "\n".join(l if l.startswith("|") else "- " + l for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
