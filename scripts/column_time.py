#!/usr/bin/env python3
"""Time the batched --extrapolate fill and the streamed column loop against the per-record calls they replace.

    python scripts/column_time.py [--runs 11] [--records 24] [--part fill|loop|all] [--only 360x180x33] [--out profiles/column_sweep_summary.md]

1. The fill alone (tests/extrap_cases.py:timing_case, record r shifted by 7 r cells in longitude): 360 x 180 x 33 and
   1440 x 720 x 8, with 1, 2, 4, 8 and 24 records -- fg_extrap_run_batch_dev on all of them against as many fg_extrap_run_dev
   calls.  Reported: ms, us per launch (iteration launches of the call), us per record-iteration, host synchronisations.
2. The whole loop: `records` records of 360 x 180 x 33 NC_FLOAT, remapped to a tripolar 1440 x 1080 tile and 50 levels --
   ColumnSweep against the chain upload, fg_dev_widen, fg_extrap_run_dev, fg_plan_apply(nz = 33), fg_dev_vertical_interp,
   fg_dev_narrow, download, record by record; from pageable and from page-locked (fg_host_alloc) arrays.

Both sides of a comparison are warmed up once and then alternate inside each of `runs` rounds.  Times are a host clock around
calls that end in a device synchronise.  Reported per pair: the medians, the mean of the paired differences and twice its
standard error -- a difference inside that margin is not a difference.  The outputs of both sides are compared on their bits."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402
import extrap_cases as ec  # noqa: E402

_ipt, _dpt = C.POINTER(C.c_int), C.POINTER(C.c_double)


def paired(a, b):
    """(median a, median b, mean of a - b, twice the standard error of that mean)"""
    a, b = np.asarray(a), np.asarray(b)
    d = a - b
    return float(np.median(a)), float(np.median(b)), float(d.mean()), 2.0 * float(d.std(ddof=1) / np.sqrt(d.size))


def fill_part(fg, runs, lines, only=None):
    import torch
    L = fg.lib()
    lines += ["## The fill alone", "",
              "| grid | records | batched, ms | per-record calls, ms | batched - calls, ms (mean +- 2 se) | launches (batched / calls) |"
              " us / launch (batched / calls) | us / record-iteration (batched / calls) | host syncs (batched / calls) |",
              "|" + "---|" * 9]
    for ni, nj, nk in ((360, 180, 33), (1440, 720, 8)):
        if only and only != f"{ni}x{nj}x{nk}":
            continue
        c = ec.timing_case(ni, nj, nk)
        all_recs = np.stack([np.roll(c["data"], 7 * r, axis=2) for r in range(24)])
        ex = fg.Extrapolator(c["lon"], c["lat"], 1)
        for nrec in (1, 2, 4, 8, 24):
            d = torch.from_numpy(all_recs[:nrec]).cuda()
            o_b, o_s = torch.empty_like(d), torch.empty_like(d)
            it_b, rm_b = np.empty((nrec, nk), dtype=np.int32), np.empty((nrec, nk))
            it_s, rm_s = np.empty((nrec, nk), dtype=np.int32), np.empty((nrec, nk))
            syncs = [0, 0]

            def batched():
                t0 = time.perf_counter()
                fg._lib.check(L.fg_extrap_run_batch_dev(ex.handle, nrec, d.data_ptr(), o_b.data_ptr(), nk, 0, 0, c["missing"], c["stop_crit"],
                                                        it_b.ctypes.data_as(_ipt), rm_b.ctypes.data_as(_dpt)))
                t = time.perf_counter() - t0
                syncs[0] = ex.last_syncs
                return 1e3 * t

            def calls():
                t0 = time.perf_counter()
                n = 0
                for r in range(nrec):
                    fg._lib.check(L.fg_extrap_run_dev(ex.handle, d[r].data_ptr(), o_s[r].data_ptr(), nk, 0, c["missing"], c["stop_crit"],
                                                      it_s[r].ctypes.data_as(_ipt), rm_s[r].ctypes.data_as(_dpt)))
                    n += ex.last_syncs
                t = time.perf_counter() - t0
                syncs[1] = n
                return 1e3 * t

            torch.cuda.synchronize()
            batched(), calls()
            assert np.array_equal(it_b, it_s) and torch.equal(o_b.view(torch.int64), o_s.view(torch.int64))
            tb, ts = [], []
            for _ in range(runs):
                tb.append(batched())
                ts.append(calls())
            mb, ms, diff, se2 = paired(tb, ts)
            rec_iters = int((it_s + 1).sum())
            # launches: a batch of 64 is queued whole, so a call launches 64 per synchronisation (the last batch of a level: the rest)
            launch_b, launch_s = 64 * syncs[0], 64 * syncs[1]
            lines.append("| %d x %d x %d | %d | %.2f | %.2f | %+.2f +- %.2f | %d / %d | %.2f / %.2f | %.3f / %.3f | %d / %d |" % (
                ni, nj, nk, nrec, mb, ms, diff, se2, launch_b, launch_s, 1e3 * mb / launch_b, 1e3 * ms / launch_s,
                1e3 * mb / rec_iters, 1e3 * ms / rec_iters, syncs[0], syncs[1]))
            print(lines[-1], flush=True)
        ex.destroy()
    lines.append("")


def loop_part(fg, runs, nrec, lines):
    L = fg.lib()
    ni, nj, nk1, nk2, nx, ny = 360, 180, 33, 50, 1440, 1080
    c = ec.timing_case(ni, nj, nk1)
    lonc, latc = fg.latlon_corners(ni, nj)
    lo, la = fg.tripolar_corners(nx, ny)
    plan = fg.XgridPlan.create(1, [fg.GridConfig(ni, nj, lonc, latc)], fg.GridConfig(nx, ny, lo, la))
    plan.finalize()
    ex = fg.Extrapolator(c["lon"], c["lat"], 1)
    z1 = np.cumsum(np.linspace(10.0, 300.0, nk1))
    z2 = np.linspace(z1[0] - 3.0, z1[-1] + 50.0, nk2)
    missing = float(np.float32(c["missing"]))
    dpz = lambda z: z.ctypes.data_as(_dpt)  # noqa: E731
    ncin, ndst = ni * nj, nx * ny
    conv = lambda name, ty, n, a, b: fg._lib.check(getattr(L, name)(C.c_int(ty), C.c_long(n), C.c_void_p(a), C.c_double(0.0),  # noqa: E731
                                                                    C.c_double(0.0), C.c_double(missing), C.c_void_p(b)))
    d_raw, d_f64 = L.fg_dev_alloc(nk1 * ncin * 4, 0), L.fg_dev_alloc(nk1 * ncin * 8, 0)
    d_mid, d_lev, d_fin = L.fg_dev_alloc(nk1 * ndst * 8, 0), L.fg_dev_alloc(nk2 * ndst * 8, 0), L.fg_dev_alloc(nk2 * ndst * 4, 0)
    assert d_raw and d_f64 and d_mid and d_lev and d_fin
    it_c = np.empty((nrec, nk1), dtype=np.int32)

    def chain(src, out):
        t0 = time.perf_counter()
        for r in range(nrec):
            fg._lib.check(L.fg_dev_upload(d_raw, src[r].ctypes.data, src[r].nbytes))
            conv("fg_dev_widen", fg.field_io.NC_FLOAT, nk1 * ncin, d_raw, d_f64)
            fg._lib.check(L.fg_extrap_run_dev(ex.handle, d_f64, d_f64, nk1, 0, missing, c["stop_crit"], it_c[r].ctypes.data_as(_ipt), None))
            fg._lib.check(L.fg_plan_apply(plan._h, C.c_void_p(d_f64), None, None, None, 0, 0.0, nk1, C.c_void_p(d_mid), None))
            plan.sync()
            fg._lib.check(L.fg_dev_vertical_interp(ndst, nk1, dpz(z1), nk2, dpz(z2), d_mid, d_lev))
            conv("fg_dev_narrow", fg.field_io.NC_FLOAT, nk2 * ndst, d_lev, d_fin)
            fg._lib.check(L.fg_dev_download(out[r].ctypes.data, d_fin, out[r].nbytes))
        return 1e3 * (time.perf_counter() - t0)

    sw = fg.ColumnSweep(ex, [plan], np.float32, np.float32, z_in=z1, z_out=z2)
    it_s = [None]

    def stream(src, out):
        t0 = time.perf_counter()
        it_s[0], _ = sw.run(src, [out], missing=missing, stop_crit=c["stop_crit"])
        return 1e3 * (time.perf_counter() - t0)

    recs = np.stack([np.roll(c["data"], 7 * r, axis=2) for r in range(nrec)]).astype(np.float32)
    lines += ["## The whole loop", "", "%d records of %d x %d x %d NC_FLOAT -> tripolar %d x %d x %d NC_FLOAT" % (nrec, ni, nj, nk1, nx, ny, nk2), "",
              "| host arrays | ColumnSweep, ms | chain of calls, ms | ColumnSweep - chain, ms (mean +- 2 se) | ratio |", "|" + "---|" * 5]
    for kind in ("pageable", "page-locked"):
        bufs = []
        if kind == "pageable":
            src, out_s, out_c = recs, np.empty((nrec, nk2, ny, nx), np.float32), np.empty((nrec, nk2, ny, nx), np.float32)
        else:
            bufs = [fg.HostBuffer(recs.shape, np.float32), fg.HostBuffer((nrec, nk2, ny, nx), np.float32), fg.HostBuffer((nrec, nk2, ny, nx), np.float32)]
            src, out_s, out_c = (b.array for b in bufs)
            src[:] = recs
        stream(src, out_s), chain(src, out_c)
        assert np.array_equal(it_s[0], it_c) and np.array_equal(out_s.view(np.uint32), out_c.view(np.uint32))
        ts, tc = [], []
        for _ in range(runs):
            ts.append(stream(src, out_s))
            tc.append(chain(src, out_c))
        m_s, m_c, diff, se2 = paired(ts, tc)
        lines.append("| %s | %.1f | %.1f | %+.1f +- %.1f | %.2fx |" % (kind, m_s, m_c, diff, se2, m_c / m_s))
        print(lines[-1], flush=True)
        del src, out_s, out_c
        for b in bufs:
            b.free()
    lines.append("")
    sw.destroy()
    for p in (d_raw, d_f64, d_mid, d_lev, d_fin):
        L.fg_dev_free(p)
    ex.destroy()
    plan.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--records", type=int, default=24)
    ap.add_argument("--part", default="all", choices=["fill", "loop", "all"])
    ap.add_argument("--only", default=None, help="fill part: 360x180x33 or 1440x720x8 alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    lines = ["# Batched fill and column loop: medians of %d alternating runs" % args.runs, ""]
    if args.part in ("fill", "all"):
        fill_part(fg, args.runs, lines, args.only)
    if args.part in ("loop", "all"):
        loop_part(fg, args.runs, args.records, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
