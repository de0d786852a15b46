#!/usr/bin/env python3
"""Timing of the bilinear path (fg_bilin) on one GPU; prints one JSON line.
  setup_ms        fg_bilin_create (host geometry + device search + weights), median of --reps after one warm-up
  scalar_ms_per_level / vector_ms_per_level   apply of --nz levels per call, device events after warm-up, divided by nz
  points_per_s    fine-grid points remapped per second (scalar)
Cases: C384 -> 1440x721 (finer_step 0) and C384 -> 720x361 (finer_step 1)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=384)
    ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import torch
    fg = __graft_entry__.load_package()
    N = a.n
    lonc, latc, lont, latt = fg.gnomonic_ed_grid(N)
    contacts = fg.find_contacts([N] * 6, [N] * 6, list(lonc), list(latc))
    lont = [np.asarray(x).reshape(N, N) for x in lont]
    latt = [np.asarray(x).reshape(N, N) for x in latt]
    res = {"metric": "bilinear", "source": f"C{N}", "nz": a.nz}
    for fs, nlon, nlat in ((0, 1440, 721), (1, 720, 361)):
        fg.BilinearPlan(lont, latt, contacts, nlon, nlat, finer_step=fs).destroy()          # warm-up
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            p = fg.BilinearPlan(lont, latt, contacts, nlon, nlat, finer_step=fs)
            ts.append((time.perf_counter() - t0) * 1e3)
            p.destroy()
        p = fg.BilinearPlan(lont, latt, contacts, nlon, nlat, finer_step=fs)
        stream = torch.cuda.current_stream()
        p.set_stream(stream.cuda_stream)
        src = torch.randn(a.nz, 6 * N * N, dtype=torch.float64, device="cuda")
        v = torch.randn_like(src)
        out = torch.empty(a.nz, nlat, nlon, dtype=torch.float64, device="cuda")

        def timed(fn):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.iters / a.nz
        sc = timed(lambda: p.apply_scalar(src, out=out))
        ve = timed(lambda: p.apply_vector(src, v))
        key = f"{nlon}x{nlat}_fs{fs}"
        res[key] = {"setup_ms": round(float(np.median(ts)), 3), "setup_ms_min": round(min(ts), 3),
                    "scalar_ms_per_level": round(sc, 5), "vector_ms_per_level": round(ve, 5),
                    "points_fine": p.npoints_fine, "points_per_s_scalar": p.npoints_fine / (sc * 1e-3)}
        p.destroy()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
