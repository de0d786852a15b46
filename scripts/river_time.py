#!/usr/bin/env python3
"""Time river_regrid on the device: C96 and C384 cubed spheres (the package's gnomonic grid, seeded land of about 45 % full-land
cells) from a 720 x 360 river network with seeded subA.

    python scripts/river_time.py [--runs 5] [--out profiles/river_summary.md] [--sizes 96 384]
    python scripts/river_time.py --ref       (no device: needs the reference's sources; writes tests/golden/river_ref_seconds.json)

`all-in` is the wall time of one Python call sequence from host arrays to host arrays: the handle's creation (tables, uploads),
run() and the read-back of the six fields of every tile.  The phases are the handle's own wall times, each ended by a
synchronise.  The two modes of the search (pruned / literal replay, fg_set_river_prune) are warmed up once and then run
alternately `runs` times in one process; the median and the largest deviation from the median are reported, and the outputs of
the two modes are compared.
--ref runs the reference's five stages (tests/capi/river_ref_driver.c, gcc -O2, one CPU core) on the same inputs and records its
seconds per stage and check_river_data's counts."""
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
import river_cases as rv  # noqa: E402

REF_JSON = os.path.join(ROOT, "tests", "golden", "river_ref_seconds.json")
SRC = (720, 360)
STAGES = ("calc_max_subA", "calc_tocell", "calc_river_data", "sort_basin", "check_river_data")


def measure_ref(args):
    tmp = tempfile.mkdtemp(prefix="river_ref_")
    res = {}
    try:
        exe = rv.build_driver(tmp)
        for n in args.sizes:
            c = rv.generated_case(n, SRC, with_area=False)
            runs = [rv.run_ref(exe, tmp, c) for _ in range(3)]
            sec = np.median([r["seconds"] for r in runs], axis=0)
            res[str(n)] = dict(seconds=dict(zip(STAGES, [float(s) for s in sec])), total=float(sec.sum()),
                               full_land=int((c["landfrac"] == 1).sum()), **{k: int(runs[0][k]) for k in rv.COUNTS})
            print(n, json.dumps(res[str(n)]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(REF_JSON, "w") as f:
        json.dump(dict(source=list(SRC), runs=3, sizes=res), f, indent=1)


def _med(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.median(v)), float(np.max(np.abs(v - np.median(v))))


def one_call(fg, c):
    source, tiles, opcode, cutoff = rv.tiles_of(c)
    t0 = time.perf_counter()
    with fg.RiverRegrid(source, tiles, opcode, suba_cutoff=cutoff) as h:
        h.run()
        out = [h.fields(n) for n in range(h.ntiles)]
        wall = (time.perf_counter() - t0) * 1e3
        return dict(h.phase_ms(), all_in=wall), out, h.stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[96, 384])
    ap.add_argument("--ref", action="store_true")
    args = ap.parse_args()
    if args.ref:
        return measure_ref(args)
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    ref = json.load(open(REF_JSON))["sizes"] if os.path.exists(REF_JSON) else {}
    lines = []
    steps = ("create", "max_suba", "tocell_travel_basin", "accumulate", "sort_check", "all_in")
    for n in args.sizes:
        c = rv.generated_case(n, SRC)
        full = int((c["landfrac"] == 1).sum())
        times, outs, stats = {1: [], 0: []}, {}, {}
        for r in range(args.runs + 1):
            for prune in (1, 0):
                fg.set_river_prune(prune)
                t, outs[prune], stats[prune] = one_call(fg, c)
                if r:
                    times[prune].append(t)
        fg.set_river_prune(1)
        same = all(np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k], b[k].view(np.int64) if b[k].dtype == np.float64 else b[k])
                   for a, b in zip(outs[1], outs[0]) for k in a)
        s1, s0 = stats[1], stats[0]
        lines.append(f"C{n} (6 x {n}^2 cells, {full} full land) from {SRC[0]} x {SRC[1]}: maxtravel {s1['maxtravel']}, maxbasin {s1['maxbasin']}, "
                     f"launches {s1['launches']}; source cells visited per land cell: pruned {s1['source_cells_visited'] / max(1, full):.1f}, "
                     f"literal {s0['source_cells_visited'] / max(1, full):.0f}; outputs of the two modes identical: {same}")
        lines.append(f"| C{n} step | pruned median ms | deviation | literal median ms | deviation |")
        lines.append("|---|---|---|---|---|")
        for k in steps:
            (m1, d1), (m0, d0) = _med([p[k] for p in times[1]]), _med([p[k] for p in times[0]])
            lines.append(f"| {k} | {m1:.3f} | {d1:.3f} | {m0:.3f} | {d0:.3f} |")
        if str(n) in ref:
            rf = ref[str(n)]
            m1 = _med([p["all_in"] for p in times[1]])[0]
            counts = all(int(s1[k]) == int(rf[k]) for k in rv.COUNTS)
            lines.append(f"reference on one CPU core, same inputs (median of 3): " + ", ".join(f"{k} {rf['seconds'][k]:.4f} s" for k in STAGES) +
                         f"; five stages {rf['total']:.4f} s against the device's all-in {m1 / 1e3:.4f} s (pruned); check_river_data's counts equal: {counts}")
    text = "\n".join(l if l.startswith("|") else "- " + l for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
