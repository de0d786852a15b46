#!/usr/bin/env python3
"""Time make_coupler_mosaic's exchange grids on the device (CouplerMosaic, fg_coupler_*).

    python scripts/coupler_time.py [--runs 7] [--out profiles/coupler_summary.md] [--large 384 1440 1080] [--shared 96 360 200 144 90]
    python scripts/coupler_time.py --large-only --runs 1        (the run a kernel trace wraps)
    python scripts/coupler_time.py --great-circle [--runs 7] [--out FILE] [--shared 96 360 200 144 90]
    python scripts/coupler_time.py --nest-wave [--runs 11] [--out FILE] [--large 384 1440 1080] [--own-land 720 360]

Two cases.
* large: a C<n> atmosphere with land on the atmosphere grid over a tripolar NX x NY ocean from -82 degrees (one row added by
  coupler_ocean_grid) with a 0 / 1 mask.  The handle is made once; run() is warmed up once and repeated `runs` times.  Reported: the
  handle's phase times (each ended by a synchronise), the bytes run() copied to the host, the list lengths and the largest
  |a_area / area_atm - 1| over the atmosphere cells -- a missed pair leaves a gap of the order of a cell, the area_ratio_thresh
  rejections about 1e-6 each.
* shared: a C<n> atmosphere, a lat-lon land grid of its own and a tripolar ocean: the configuration coupler.coupler_xgrid (three
  searches, the lists downloaded and finished in numpy) accepts.  Both paths go from host arrays to host arrays -- the pipeline's
  time is the handle's creation, run() and the download of its atmosphere x ocean and atmosphere x land lists; it also makes the
  land x ocean list, the sums, distances and masks, which coupler_xgrid does not.  The two alternate in one process after a warm-up
  of each; median and largest deviation from it.
* --nest-wave: the large case with no nest and no wave grid, and with a wave grid equal to the ocean grid (wav_same_as_ocn); then,
  because a nest is refused with land on the atmosphere grid (make_coupler_mosaic.c:742), the same atmosphere and ocean with a
  lat-lon land grid of its own: plain, with a nest (a block of a quarter of the edge of tile 2, halved: the seventh tile), and with
  the wave grid, whose step is reported beside the land x ocean step of the same handle.  One handle per leg, a warm-up, `runs`
  runs; check() is timed once per leg.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402


def _med(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.median(v)), float(np.max(np.abs(v - np.median(v))))


def _fmt(v):
    m, d = _med(v)
    return f"{m:.3f} ({d:.3f})"


def block_mask(nx, ny, fractions):
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    m = np.where((ii // max(nx // 12, 1) + jj // max(ny // 9, 1)) % 3 == 0, 0.0, 1.0)
    if fractions:
        m[(ii + 2 * jj) % 11 == 0] = 0.35
    return m


def ocean(fg, nx, ny, fractions):
    to, ta = fg.tripolar_corners(nx, ny)
    g = fg.coupler_ocean_grid(np.degrees(to), np.degrees(ta), block_mask(nx, ny, fractions))
    return fg.GridConfig(nx, g["ny"], g["x"], g["y"]), g["omask"], g["ocn_south_ext"]


def cubed_sphere(fg, ni):
    lon, lat = fg.gnomonic_ed_corners(ni)
    return [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]


def large(fg, size, runs):
    ni, nx, ny = size
    atm = cubed_sphere(fg, ni)
    ocn, omask, ext = ocean(fg, nx, ny, False)
    with fg.CouplerMosaic(atm, None, ocn, omask, ocn_south_ext=ext) as m:
        m.run()
        ph = []
        for _ in range(runs):
            m.run()
            ph.append(m.phase_ms())
        st = m.stats()
        gap = max(float(np.max(np.abs(m.cells(m.ATM, t)["frac"] - 1))) for t in range(6))
        create = m.phase_ms()["create"]
    lines = [f"## C{ni} atmosphere = land over a tripolar {nx} x {ny} ocean (+{ext} southern row), 0 / 1 mask, order 2", "",
             f"{runs} runs of one handle after a warm-up; median (largest deviation from it), ms.  Creation of the handle (uploads, the three "
             f"grids' areas): {create:.3f} ms.", "",
             "| atmosphere x land candidates | atmosphere x ocean | polygons x ocean | land x ocean | sums, distances, masks | run |", "|---|---|---|---|---|---|",
             "| " + " | ".join(_fmt([p[k] for p in ph]) for k in ("axl_candidates", "axo", "polygons_x_ocean", "lxo", "sums", "run")) + " |", "",
             f"Lists: {st['naxo']} atmosphere x ocean cells, {st['naxl']} atmosphere x land cells from {st['npolygons']} remembered polygons, "
             f"{st['searches']} searches; nbad {st['nbad']}.", f"Bytes run() copied to the host: {st['d2h_bytes']}.",
             f"Largest |a_area / area_atm - 1| over the atmosphere cells: {gap:.3e} (bound 1e-3: {'met' if gap < 1e-3 else 'MISSED'})."]
    return lines, gap


def shared(fg, size, runs):
    ni, nx, ny, nxl, nyl = size
    atm = cubed_sphere(fg, ni)
    ocn, omask, ext = ocean(fg, nx, ny, True)
    lo, la = fg.latlon_corners(nxl, nyl)
    lnd = fg.GridConfig(nxl, nyl, lo, la)

    def pipeline():
        t0 = time.perf_counter()
        with fg.CouplerMosaic(atm, [lnd], ocn, omask, ocn_south_ext=ext) as m:
            t1 = time.perf_counter()
            m.run()
            t2 = time.perf_counter()
            axo = [m.axo(t) for t in range(6)]
            axl = [m.axl(t, 0) for t in range(6)]
            t3 = time.perf_counter()
            return dict(create=(t1 - t0) * 1e3, run=(t2 - t1) * 1e3, download=(t3 - t2) * 1e3, all_in=(t3 - t0) * 1e3, d2h=m.stats()["d2h_bytes"]), axo, axl

    def parent():
        t0 = time.perf_counter()
        r = fg.coupler_xgrid(atm, lnd, ocn, omask, interp_order=2)
        return (time.perf_counter() - t0) * 1e3, r

    pipeline(); parent()
    tp, tq = [], []
    for _ in range(runs):
        p, axo, axl = pipeline()
        q, r = parent()
        tp.append(p); tq.append(q)
    same = True
    for name, mine, keys in (("axo", axo, ("ia", "ja", "io", "jo")), ("axl", axl, ("ia", "ja", "il", "jl"))):
        for i, k in enumerate(keys):
            same = same and np.array_equal(np.concatenate([t[k] for t in mine]), r[name][keys[i]])
        for k in ("area", "clon", "clat"):
            same = same and np.array_equal(np.concatenate([t[k] for t in mine]).view(np.uint64), r[name][k].view(np.uint64))
    ratio = _med(tq)[0] / _med([p["all_in"] for p in tp])[0]
    lines = [f"## C{ni} atmosphere, {nxl} x {nyl} lat-lon land, tripolar {nx} x {ny} ocean (+{ext} row), order 2: the case coupler_xgrid accepts", "",
             f"{runs} alternating runs after a warm-up of each; host arrays to host arrays; median (largest deviation from it), ms.", "",
             "| path | create | run | download of the two lists | all-in |", "|---|---|---|---|---|",
             "| CouplerMosaic | " + " | ".join(_fmt([p[k] for p in tp]) for k in ("create", "run", "download", "all_in")) + " |",
             f"| coupler_xgrid (three searches, lists finished in numpy) | | | | {_fmt(tq)} |", "",
             f"coupler_xgrid / CouplerMosaic, all-in: {ratio:.2f}.  The pipeline's run also makes the land x ocean list, the per-cell sums, the six "
             f"distances and the masks; it copied {tp[-1]['d2h']} bytes to the host.",
             f"Both give the same atmosphere x ocean and atmosphere x land lists, indices and bits of area, clon, clat: {same}."]
    return lines, ratio, same


def nest_wave(fg, size, own_land, runs):
    ni, nx, ny = size
    atm = cubed_sphere(fg, ni)
    ocn, omask, ext = ocean(fg, nx, ny, False)
    lo, la = fg.latlon_corners(*own_land)
    lnd = [fg.GridConfig(own_land[0], own_land[1], lo, la)]
    # the nest: ni / 4 x ni / 4 cells of tile 2 (equatorial, 35 .. 125 E) from (ni / 4, ni / 2) halved; new corners midway in lon / lat
    nb, i0, j0 = ni // 4, ni // 4, ni // 2
    corners = []
    for p in (atm[1].lonc, atm[1].latc):
        b = np.asarray(p, dtype=np.float64).reshape(ni + 1, ni + 1)[j0:j0 + nb + 1, i0:i0 + nb + 1]
        f = np.empty((2 * nb + 1, 2 * nb + 1))
        f[::2, ::2] = b
        f[::2, 1::2] = 0.5 * (b[:, :-1] + b[:, 1:])
        f[1::2, ::2] = 0.5 * (b[:-1] + b[1:])
        f[1::2, 1::2] = 0.5 * (f[1::2, 0:-1:2] + f[1::2, 2::2])
        corners.append(f)
    nest = fg.GridConfig(2 * nb, 2 * nb, corners[0], corners[1])
    keys = ("axl_candidates", "axo", "polygons_x_ocean", "lxo", "wxo", "sums", "run")
    legs = (("land on the atmosphere grid", atm, None, {}),
            ("land on the atmosphere grid, wave grid = ocean grid", atm, None, dict(wav=[ocn], wav_same_as_ocn=True)),
            (f"{own_land[0]} x {own_land[1]} land", atm, lnd, {}),
            (f"{own_land[0]} x {own_land[1]} land, nest of {2 * nb} x {2 * nb} cells", atm + [nest], lnd, dict(tile_nest=6)),
            (f"{own_land[0]} x {own_land[1]} land, wave grid = ocean grid", atm, lnd, dict(wav=[ocn], wav_same_as_ocn=True)))
    lines = [f"## Nest and wave legs: C{ni} atmosphere over a tripolar {nx} x {ny} ocean (+{ext} southern row), 0 / 1 mask, order 2", "",
             f"One handle per leg, a warm-up, {runs} runs; median (largest deviation from it), ms; check() once after the last run.", "",
             "| leg | " + " | ".join(keys) + " | check() | bytes to the host | lists (axo / axl / lxo / wxo) |", "|---|" + "---|" * (len(keys) + 3)]
    notes = []
    for title, a, l, kw in legs:
        with fg.CouplerMosaic(a, l, ocn, omask, ocn_south_ext=ext, **kw) as m:
            m.run()
            ph = []
            for _ in range(runs):
                m.run()
                ph.append(m.phase_ms())
            st = m.stats()
            t0 = time.perf_counter()
            ck = m.check()
            t_ck = (time.perf_counter() - t0) * 1e3
        cols = [_fmt([p[k] for p in ph]) if k in ph[0] else "-" for k in keys]
        lines.append(f"| {title} | " + " | ".join(cols) + f" | {t_ck:.1f} | {st['d2h_bytes']} | {st['naxo']} / {st['naxl']} / {st['nlxo']} / {st.get('nwxo', '-')} |")
        note = f"* {title}: largest area mismatch {ck['max_ratio']:.3e} at tile {ck['max_tile'] + 1}, tiling error {ck['tiling_area']:.3e} %"
        if "tiling_area_nest" in ck:
            note += f", nest region {ck['tiling_area_nest']:.3e} %"
        if "wxo_area_sum" in ck:
            note += f", wxo_area_sum / axo_area_sum = {ck['wxo_area_sum'] / ck['axo_area_sum']:.9f}"
        notes.append(note + ".")
    return lines + [""] + notes


def great_circle(fg, size, runs):
    """--great-circle: CouplerMosaic(clip_method="great_circle") against the legacy order-1 handle on the same grids, runs alternating
    after a warm-up of each; then the polygon-list search per candidate pair against the quad x quad great-circle search per pair
    with fg_set_gc_split(0) (the same general clip, so the ratio is what the wider lists cost)."""
    ni, nx, ny, nxl, nyl = size
    atm = cubed_sphere(fg, ni)
    ocn, omask, ext = ocean(fg, nx, ny, True)
    lo, la = fg.latlon_corners(nxl, nyl)
    lnd = fg.GridConfig(nxl, nyl, lo, la)
    keys = ("axl_candidates", "axo", "polygons_x_ocean", "lxo", "sums", "run")
    lines = []
    na, no, nl = 6 * ni * ni, ocn.nx * ocn.ny, nxl * nyl
    for title, land in ((f"C{ni} atmosphere = land", None), (f"C{ni} atmosphere, {nxl} x {nyl} lat-lon land", [lnd])):
        with fg.CouplerMosaic(atm, land, ocn, omask, interp_order=1, ocn_south_ext=ext) as ml, \
                fg.CouplerMosaic(atm, land, ocn, omask, interp_order=1, ocn_south_ext=ext, clip_method="great_circle") as mg:
            ml.run(); mg.run()
            pl, pg = [], []
            for _ in range(runs):
                ml.run(); pl.append(ml.phase_ms())
                mg.run(); pg.append(mg.phase_ms())
            sl, sg = ml.stats(), mg.stats()
            cl, cg = ml.phase_ms()["create"], mg.phase_ms()["create"]
        # what the reference's GREAT_CIRCLE_CLIP branch clips: every pair (:1253-1267, :2549-2556)
        brute = na * no + sg["npolygons"] * no + (0 if land is None else na * nl + nl * no)
        lines += [f"## {title}, tripolar {nx} x {ny} ocean (+{ext} row), order 1", "",
                  f"{runs} alternating runs of the two handles after a warm-up of each; median (largest deviation from it), ms.", "",
                  "| clip | create | " + " | ".join(keys) + " |", "|---|---|" + "---|" * len(keys),
                  f"| legacy | {cl:.3f} | " + " | ".join(_fmt([p[k] for p in pl]) for k in keys) + " |",
                  f"| great circle | {cg:.3f} | " + " | ".join(_fmt([p[k] for p in pg]) for k in keys) + " |", "",
                  f"great circle: {sg['naxo']} atmosphere x ocean, {sg['naxl']} atmosphere x land, {sg['nlxo']} land x ocean cells, {sg['npolygons']} remembered "
                  f"polygons, {sg['searches']} searches, {sg['d2h_bytes']} bytes to the host, nbad {sg['nbad']}; legacy: {sl['naxo']} / {sl['naxl']} / {sl['nlxo']}.",
                  f"Pairs the reference's branch clips for this job (no pruning there): {brute}.", ""]
    # the n-gon clip against the quad clip, per candidate pair
    L = fg.lib()
    L.fg_set_profiling(1)
    L.fg_set_gc_split(0)
    try:
        p = fg.XgridPlan.create_great_circle(atm, lnd)
        pg = p.get_polygons(8)
        x = p.get_xgrid()
        a_atm, a_lnd = p.get_cell_area(nl)
        p.destroy()
        ok = pg["n"] <= 8
        off = np.concatenate([[0], np.cumsum([g.nx * g.ny for g in atm])])
        ref = np.minimum(a_lnd[x["j_out"] * nxl + x["i_out"]], a_atm[off[x["t_in"]] + x["j_in"] * ni + x["i_in"]])[ok]
        tq, tp = [], []
        for _ in range(runs + 1):
            q = fg.XgridPlan.create_great_circle(atm, ocn)
            tq.append((q.phase_ms()["clip_general"], q.stats()["pairs"])); q.destroy()
            r = fg.XgridPlan.create_polylist_gc(pg["n"][ok], pg["x"][ok], pg["y"][ok], pg["z"][ok], ref, ocn)
            tp.append((r.phase_ms()["clip_general"], r.stats()["pairs"])); r.destroy()
    finally:
        L.fg_set_gc_split(1)
        L.fg_set_profiling(0)
    mq, mp = _med([t[0] for t in tq[1:]])[0], _med([t[0] for t in tp[1:]])[0]
    lines += ["## The general clip per candidate pair: polygons (k_gc_clip_poly) against quads (fg_set_gc_split(0))", "",
              "| search | candidate pairs | clip phase, ms | ns per pair |", "|---|---|---|---|",
              f"| C{ni} -> ocean, quad x quad, one-kernel clip | {tq[-1][1]} | {_fmt([t[0] for t in tq[1:]])} | {1e6 * mq / max(tq[-1][1], 1):.1f} |",
              f"| {int(ok.sum())} remembered polygons -> ocean | {tp[-1][1]} | {_fmt([t[0] for t in tp[1:]])} | {1e6 * mp / max(tp[-1][1], 1):.1f} |", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--large", type=int, nargs=3, default=[384, 1440, 1080], metavar=("NI", "NX", "NY"))
    ap.add_argument("--shared", type=int, nargs=5, default=[96, 360, 200, 144, 90], metavar=("NI", "NX", "NY", "NX_LND", "NY_LND"))
    ap.add_argument("--large-only", action="store_true")
    ap.add_argument("--great-circle", action="store_true", help="the great-circle handle against the legacy one on the --shared grids")
    ap.add_argument("--nest-wave", action="store_true", help="the large case with a wave grid, and with a land grid of its own plain / nest / wave")
    ap.add_argument("--own-land", type=int, nargs=2, default=[720, 360], metavar=("NX_LND", "NY_LND"))
    args = ap.parse_args()
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    if args.great_circle:
        text = "\n".join(["# make_coupler_mosaic's GREAT_CIRCLE_CLIP branch on the device: timing", ""] + great_circle(fg, args.shared, args.runs)) + "\n"
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return
    if args.nest_wave:
        text = "\n".join(nest_wave(fg, args.large, args.own_land, args.runs)) + "\n"
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return
    lines = ["# make_coupler_mosaic's exchange grids on the device: timing", ""]
    a, gap = large(fg, args.large, args.runs)
    lines += a
    if not args.large_only:
        b, ratio, same = shared(fg, args.shared, args.runs)
        lines += [""] + b
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if not gap < 1e-3:
        sys.exit("the atmosphere cells are not covered: gap %g" % gap)


if __name__ == "__main__":
    main()
