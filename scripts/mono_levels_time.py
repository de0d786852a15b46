"""Times of the monotone sweep on many levels against the per-level loop it replaces.

  C384 -> 1440 x 720, order 2, 8 and 50 levels of +-uniform(1, 10) under a land mask that grows with depth
  (scripts/masked_levels_time.py's), halo fill and gradients from the device's own preparation, made once outside the clock;
  with and without cell_measures (one area for all levels):
    loop     nlev x fg_plan_apply_ex(monotonic, nz = 1): four launches, an xdata array and the error word per level
    levels   fg_plan_apply_levels_mono: three launches beside the two transpositions per chunk of eight levels
    split    the same as fg_plan_mono_levels_begin / a hook that does nothing / fg_plan_mono_levels_end per chunk
The loop uses only entry points older than the batched ones, and the batched legs are left out where the library lacks them,
so the same script times the loop on an older build.  Every figure is a host clock around `reps` repetitions that end in a
synchronise, after warm-up; the legs alternate over five rounds; best and worst round are printed (their ratio is the
run-to-run spread).  One JSON line.

  python scripts/mono_levels_time.py [--reps N] [--levels 8,50]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from masked_levels_time import MISSING, land_mask      # noqa: E402
from levels_ex_time import alternate, report           # noqa: E402


def run(fg, torch, reps, level_counts):
    ni, nlon, nlat = 384, 1440, 720
    dev = "cuda:0"
    lon, lat, lont, latt = fg.gnomonic_ed_grid(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    ncell, ndst = 6 * ni * ni, nlon * nlat
    prep = fg.C2lPrep([ni] * 6, [ni] * 6, lon, lat, lont, latt, fg.find_contacts([ni] * 6, [ni] * 6, lon, lat))
    plan = fg.XgridPlan.create(2, [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)], fg.GridConfig(nlon, nlat, lo, la))
    plan.finalize(); plan.sync()
    prep.set_stream(plan.stream())
    m8 = land_mask(np.asarray(lont).reshape(-1), np.asarray(latt).reshape(-1), 8)
    rng = np.random.default_rng(3)
    fa_t = torch.from_numpy(rng.uniform(0.5e-4, 2e-4, ncell)).to(dev)
    batched = hasattr(plan, "apply_levels_mono")
    res = {"workload": f"C{ni} -> {nlon}x{nlat}, order 2, monotone limiter, land fraction {m8.mean():.3f}", "unit": "ms per call of all levels",
           "nxgrid": plan.nxgrid, "reps": reps}
    for nlev in level_counts:
        src = rng.choice([-1.0, 1.0], (nlev, ncell)) * rng.uniform(1.0, 10.0, (nlev, ncell))
        for k in range(nlev):
            src[k][m8[min(k * 8 // nlev, 7)]] = MISSING
        src_t = torch.from_numpy(src).to(dev)
        halo = torch.empty(nlev, prep.F, dtype=torch.float64, device=dev)
        gx = torch.empty(nlev, ncell, dtype=torch.float64, device=dev); gy = torch.empty_like(gx)
        gm = torch.empty(nlev, ncell, dtype=torch.int32, device=dev)
        out = torch.empty(nlev, ndst, dtype=torch.float64, device=dev); out2 = torch.empty_like(out)
        torch.cuda.synchronize()
        for k0 in range(0, nlev, 8):                       # (the preparation takes up to eight levels of missing values per call)
            n = min(8, nlev - k0)
            prep.fill_halo(src_t[k0:k0 + n], halo[k0:k0 + n], n)
            prep.gradient(halo[k0:k0 + n], n, gx[k0:k0 + n], gy[k0:k0 + n], gm[k0:k0 + n], True, MISSING)
        plan.sync()
        for name, opts in (("plain", {}), ("meas", dict(field_area_t=fa_t))):
            common = dict(has_missing=True, missing=MISSING, **opts)

            def loop():
                for k in range(nlev):
                    plan.apply_ex(halo[k], out[k], nz=1, grad_x_t=gx[k], grad_y_t=gy[k], grad_mask_t=gm[k], monotonic=True, **common)
            cands = {"loop_apply_ex": loop}
            same = None
            if batched:
                def levels():
                    plan.apply_levels_mono(halo, out2, nlev, gx, gy, gm, **common)

                def split():
                    plan.apply_levels_mono(halo, out2, nlev, gx, gy, gm, minmax_hook=lambda p, nz: None, **common)
                cands["apply_levels_mono"] = levels
                cands["begin_hook_end"] = split
                loop(); levels(); plan.sync()
                same = bool(torch.equal(out.view(torch.int64), out2.view(torch.int64)))
                out2.zero_(); torch.cuda.synchronize()
                split(); plan.sync()
                same = same and bool(torch.equal(out.view(torch.int64), out2.view(torch.int64)))
            res[f"{nlev}_levels_{name}"] = dict(report(alternate(cands, plan.sync, reps)), bits_equal_to_loop=same)
    plan.destroy()
    prep.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--levels", default="8,50")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    fg = g.load_package()
    fg._lib.require_gpu()
    print(json.dumps(run(fg, torch, a.reps, [int(v) for v in a.levels.split(",")])), flush=True)


if __name__ == "__main__":
    main()
