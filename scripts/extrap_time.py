#!/usr/bin/env python3
"""Time the --extrapolate fill on the device (fg_extrap_run_dev) at 360 x 180 x 33 and 1440 x 720 x 8 (continents-like mask,
stop_crit = 0.005: tests/extrap_cases.py:timing_case) and compare with the reference's do_extrapolate on one CPU core
(tests/golden/extrapolate_cpu_baseline.json).

    python scripts/extrap_time.py [--runs 7] [--out profiles/extrapolate_timing.md] [--only 1440x720x8]

Every variant (coefficients evaluated per use / stored table, batch length) is warmed up once and then timed `runs` times,
variants alternating inside each round; the median is reported.  Times are HIP events on the handle's stream around the whole
call (prepare + iterations + the per-batch read-backs + the level copies), so they include the host synchronisations.
The bytes model: per iteration and cell 8 B state read (the four neighbours come from cache lines the block already fetched),
8 B state written, 1/8 B mask, plus 32 B of coefficients in the stored variant.  Both working sets (state x 2, mask, table:
2 / 6 MB at 1 degree, 17 / 50 MB at 0.25 degree) sit in the 256 MiB Infinity Cache and not in a 4 MiB L2, so the model is set
against the cache's measured 8.6 TB/s (MI355X gather figure), not against HBM."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402
import extrap_cases as ec  # noqa: E402

IC_BW = 8.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    L = fg.lib()
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "extrapolate_cpu_baseline.json")))
    variants = [("per-use coefficients, batch 64", 0, 64), ("stored table, batch 64", 1, 64), ("per-use coefficients, batch 256", 0, 256)]
    rows = []
    for ni, nj, nk in ((360, 180, 33), (1440, 720, 8)):
        key = f"{ni}x{nj}x{nk}"
        if args.only and args.only != key:
            continue
        c = ec.timing_case(ni, nj, nk)
        ref = base[f"timing_{key}"]
        d = torch.from_numpy(c["data"]).cuda()
        out = torch.empty_like(d)
        iters, resmax = np.empty(nk, dtype=np.int32), np.empty(nk)
        ex = fg.Extrapolator(c["lon"], c["lat"], 1)
        st = torch.cuda.Stream()
        fg._lib.check(L.fg_extrap_set_stream(ex.handle, C.c_void_p(st.cuda_stream)))
        times = {v[0]: [] for v in variants}
        syncs = {}

        def run(stored, batch):
            fg.set_extrap_coef(stored)
            fg.set_extrap_batch(batch)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record()
                fg._lib.check(L.fg_extrap_run_dev(ex.handle, d.data_ptr(), out.data_ptr(), nk, 0, c["missing"], c["stop_crit"],
                                                  iters.ctypes.data_as(C.POINTER(C.c_int)), resmax.ctypes.data_as(C.POINTER(C.c_double))))
                e1.record()
            e1.synchronize()
            assert list(iters) == ref["iters"], (list(iters), ref["iters"])
            return e0.elapsed_time(e1)

        torch.cuda.synchronize()
        for name, stored, batch in variants:
            run(stored, batch)                                        # warm-up of every variant
        for _ in range(args.runs):
            for name, stored, batch in variants:
                times[name].append(run(stored, batch))
                syncs[name] = ex.last_syncs
        total_iters = int(sum(n + 1 for n in ref["iters"]))
        for name, stored, batch in variants:
            ms = float(np.median(times[name]))
            us_it = 1e3 * ms / total_iters
            bytes_it = ni * nj * (16.125 + (32 if stored else 0))
            want_syncs = sum(-(-(n + 1) // batch) for n in ref["iters"])
            assert syncs[name] == want_syncs
            rows.append((key, name, ms, min(times[name]), max(times[name]), ms / nk, us_it, bytes_it / 1e6, 1e6 * bytes_it / IC_BW,
                         syncs[name] / nk, total_iters / nk, ref["seconds_cpu"], 1e3 * ref["seconds_cpu"] / ms))
        ex.destroy()
        fg.set_extrap_coef(0)
        fg.set_extrap_batch(0)
    hdr = ("| case | variant | ms (median of %d) | min .. max | ms / level | us / iteration | MB / iteration (model) | model at 8.6 TB/s, us |"
           " host syncs / level | iterations / level | reference, 1 CPU core, s | ratio |" % args.runs)
    lines = [hdr, "|" + "---|" * 12]
    for r in rows:
        lines.append("| %s | %s | %.2f | %.2f .. %.2f | %.3f | %.2f | %.2f | %.2f | %.1f | %.1f | %.3f | %.0fx |" % r)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
