#!/usr/bin/env python3
"""Time make_topog's realistic topography on the device: a global float32 elevation of NX x NY cells onto a tripolar model grid
(the package's generator) with cyclic_x, tripolar_grid, one filter pass and the tool's defaults, 50 levels.

    python scripts/topog_time.py [--runs 7] [--out profiles/topog_summary.md] [--size 1080 540 360 270]
    python scripts/topog_time.py --ref      (no device: needs the reference's sources; writes tests/golden/topog_ref_seconds.json)

`all-in` is the wall time of one Python call sequence from host arrays to host arrays: the handle's creation, source(), run() and
the read-back of depth and num_levels.  The phases are the handle's own wall times, each ended by a synchronise.  The two ways of
evaluating remove_isolated_cells (the in-place sweep as one launch per anti-diagonal / every cell at once in the last kernel,
fg_set_topog_sweep; the second is the default) are warmed up once and then run alternately `runs` times in one process; the
median and the largest deviation from the median are reported, and both results are compared with the reference's through the
digests --ref recorded.
`before` is what a caller had before fg_topog: the 2-D corner arrays, the widened field and the mask formed on the host,
conserve_interp (the drop-in entry, which builds a throw-away plan from host arrays), and filter_topo and process_topo on the
host, for which the reference's own seconds from --ref stand in.
--ref runs the reference's stages (tests/capi/topog_ref_driver.c, gcc -O2, one CPU core) on the same inputs and records its seconds
per stage, its counts and SHA-256 digests of its outputs."""
import argparse
import hashlib
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
import topog_cases as tc  # noqa: E402

REF_JSON = os.path.join(ROOT, "tests", "golden", "topog_ref_seconds.json")
STAGES = ("conserve_interp", "filter_topo", "process_topo")


def levels(nk=50, bottom=6000.0):
    """zw of a stretched vertical grid: 10 m at the surface, nk levels to `bottom`"""
    s = np.arange(1, nk + 1) / nk
    return np.round(bottom * (0.15 * s + 0.85 * s ** 3), 2)


def case(size):
    nxs, nys, nx, ny = size
    fg = tc.package()
    lon, lat = fg.tripolar_corners(nx, ny)
    c = tc._chain(lon * tc.R2D, lat * tc.R2D, (nxs, nys), 101, np.float32, zw=levels(), tripolar_grid=1, cyclic_x=1, filter_topog=1)
    return c


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def measure_ref(args):
    tmp = tempfile.mkdtemp(prefix="topog_ref_")
    try:
        exe = tc.build_driver(tmp)
        c = case(args.size)
        r = tc.run_ref(exe, tmp, c)
        res = dict(size=list(args.size), seconds=dict(zip(STAGES, [float(s) for s in r["seconds"]])), total=float(r["seconds"].sum()),
                   jstart=int(r["jstart"]), jend=int(r["jend"]), **{k: int(r[k]) for k in tc.COUNTS},
                   digests={k: digest(r[k]) for k in ("depth_remap", "depth_filter", "depth_final", "num_levels")})
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(REF_JSON, "w") as f:
        json.dump(res, f, indent=1)


def _med(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.median(v)), float(np.max(np.abs(v - np.median(v))))


def one_call(fg, c):
    t0 = time.perf_counter()
    with fg.Topog(c["x_dst"], c["y_dst"], **tc.options(c)) as h:
        h.source(c["xt_src"], c["yt_src"], c["data"], c["missing"]).run(c["zw"])
        depth, lev = h.depth(), h.num_levels()
        wall = (time.perf_counter() - t0) * 1e3
        return dict(h.phase_ms(), all_in=wall), depth, lev, h.stats()


def before(fg, c, nxgrid):
    """host preparation + conserve_interp through the drop-in entry, ms; None when the exchange grid would exceed MAXXGRID (the
    drop-in entry then stops the process, as the reference does)"""
    if nxgrid >= fg.get_maxxgrid():
        return None, None
    t0 = time.perf_counter()
    xt, yt = c["xt_src"], c["yt_src"]
    jstart, jend = fg.topog_source_rows(yt, c["y_dst"])

    def bounds(t):
        b = np.empty(t.size + 1)
        b[1:-1] = (t[:-1] + t[1:]) * 0.5
        b[0], b[-1] = 2 * t[0] - b[1], 2 * t[-1] - b[-2]
        return b * tc.D2R
    x2, y2 = np.meshgrid(bounds(xt), bounds(yt)[jstart:jend + 2])
    d = c["data"][jstart:jend + 1].astype(np.float64)
    miss = d == c["missing"]
    d = np.where(miss, d, d * float(c["scale_factor"]))
    mask = np.where(miss | (d <= 0), 0.0, 1.0)
    ny, nx = tc.shape_of(c)
    out = fg.conserve_interp(xt.size, jend - jstart + 1, nx, ny, x2, y2, c["x_dst"] * tc.D2R, c["y_dst"] * tc.D2R, mask, d)
    return (time.perf_counter() - t0) * 1e3, out.reshape(ny, nx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, nargs=4, default=[1080, 540, 360, 270], metavar=("NX_SRC", "NY_SRC", "NX", "NY"))
    ap.add_argument("--ref", action="store_true")
    args = ap.parse_args()
    if args.ref:
        return measure_ref(args)
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    ref = json.load(open(REF_JSON)) if os.path.exists(REF_JSON) else None
    if ref and ref["size"] != list(args.size):
        ref = None
    c = case(args.size)
    nx, ny = args.size[2], args.size[3]
    times, res = {0: [], 1: []}, {}
    for fused in (0, 1):                                   # warm-up: code objects, the pool, the first plan
        fg.set_topog_sweep(fused)
        one_call(fg, c)
    for _ in range(args.runs):
        for fused in (0, 1):
            fg.set_topog_sweep(fused)
            ms, depth, lev, st = one_call(fg, c)
            times[fused].append(ms)
            res[fused] = (depth, lev, st)
    fg.set_topog_sweep(1)
    same = bool(np.array_equal(res[0][0].view(np.int64), res[1][0].view(np.int64)) and np.array_equal(res[0][1], res[1][1]))
    st = res[0][2]
    before(fg, c, st["nxgrid"])
    b = [before(fg, c, st["nxgrid"]) for _ in range(args.runs)]
    lines = ["# make_topog realistic topography on the device: timing", "",
             f"Source {args.size[0]} x {args.size[1]} float32 (rows {st['jstart']} .. {st['jend']} kept) onto a tripolar {nx} x {ny} model grid, cyclic_x, "
             f"tripolar_grid, one filter pass, 50 levels; nxgrid {st['nxgrid']}.  {args.runs} alternating runs after a warm-up; median "
             "(largest deviation from it), ms.", "",
             "| remove_isolated_cells | launches of the step | create | source | remap | filter | process | all-in |", "|---|---|---|---|---|---|---|---|"]
    for fused, label in ((0, "in-place sweep, one launch per anti-diagonal"), (1, "every cell at once, in the last kernel")):
        row = [label, str(res[fused][2]["sweep_launches"])]
        for k in ("create", "source", "remap", "filter", "process", "all_in"):
            m, d = _med([t[k] for t in times[fused]])
            row.append(f"{m:.3f} ({d:.3f})")
        lines.append("| " + " | ".join(row) + " |")
    lines += ["", f"The two evaluations give the same depth and num_levels bit for bit: {same}.",
              f"Counts: isolated cells filled {st['isolated_filled']}, partial cells restricted {st['partial_restricted']}, shallow cells modified "
              f"{st['shallow_modified']}; deepest {st['deepest']:.3f} m, verdict {st['verdict']}."]
    if ref:
        ok = {f"{k}, sweep {m}": digest(res[m][q]) == ref["digests"][k] for m in (0, 1) for q, k in enumerate(("depth_final", "num_levels"))}
        lines += ["", "## Against the reference on one CPU core (gcc -O2, same inputs)", "",
                  "| stage | reference, s | device, ms (every cell at once, the default) |", "|---|---|---|"]
        for k, p in zip(STAGES, ("remap", "filter", "process")):
            lines.append(f"| {k} | {ref['seconds'][k]:.3f} | {_med([t[p] for t in times[1]])[0]:.3f} |")
        lines += ["", f"The device's depth and num_levels have the reference's SHA-256 digests: {ok}; the reference's counts: isolated "
                  f"{ref['isolated_filled']}, partial {ref['partial_restricted']}, shallow {ref['shallow_modified']}."]
        if b[0][0] is not None:
            m, d = _med([v[0] for v in b])
            host = (ref["seconds"]["filter_topo"] + ref["seconds"]["process_topo"]) * 1e3
            rem_ok = digest(b[0][1]) == ref["digests"]["depth_remap"]
            lines += ["", "## End to end, host arrays to host arrays", "",
                      f"Before: host preparation of the 2-D corners, the widened field and the mask + conserve_interp (drop-in entry): {m:.3f} ({d:.3f}) ms "
                      f"(its result has the reference's digest: {rem_ok}), + filter_topo and process_topo on the host (the reference's own "
                      f"{host:.3f} ms) = {m + host:.3f} ms.",
                      f"Now: {_med([t['all_in'] for t in times[1]])[0]:.3f} ms with every cell at once (the default), {_med([t['all_in'] for t in times[0]])[0]:.3f} ms with "
                      "the in-place sweep."]
        else:
            lines += ["", f"The drop-in conserve_interp was not run: nxgrid {st['nxgrid']} is not below MAXXGRID {fg.get_maxxgrid()}, where it stops the process."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
