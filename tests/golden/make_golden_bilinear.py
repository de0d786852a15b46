#!/usr/bin/env python3
"""Generate tests/golden/bilinear_*.npz from the REFERENCE's bilinear code (tools/fregrid/bilinear_interp.c).

Run in the build container (needs /root/reference, oracle/_ref from `make -C oracle` and the built library):
    python tests/golden/make_golden_bilinear.py
tests/capi/bilinear_ref_driver.c is compiled with the reference's bilinear_interp.c, mosaic_util.c and mpp.c in a temporary
directory outside the repository; nothing compiled is kept.  Inputs: C24 centres from the reference's generator
(create_gnomonic_cubic_grid.c, oracle/_ref), halo'd with this repository's halo map (fg_halo_map).
Each case file holds (data only):
  config          N, nlon, nlat, finer_step, center_y, lonbegin, lonend, latbegin, latend, missing
  lont_halo, latt_halo [6, N+2, N+2]   the halo'd centres the reference ran on
  s, s_miss, u, v [6, N, N]            the source fields (s_miss: s with every 37th cell set to `missing`)
  index [n, 3], weight [n, 4]          Interp_config after setup_bilinear_interp (fine grid)
  s_plain, s_missing, s_fill, u_out, v_out [nlat, nlon]   do_scalar (plain / has_missing / fill_missing), do_vector
bilinear_write_layout.npz: what the WRITE branch requested for case c24_72x37_fs0 (dimensions, variables, raw buffers).
bilinear_cpu_baseline.json: the reference's single-core setup time at C96 -> 1 degree (and C384 -> 0.25 degree when it
finishes within the time limit)."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import gridutil  # noqa: E402
import __graft_entry__  # noqa: E402

REF = os.environ.get("FRE_REFERENCE", "/root/reference")
MISSING = -1.0e20
CASES = [
    # name, N, nlon, nlat, finer_step, lonbegin, lonend, latbegin, latend, center_y
    ("c24_72x37_fs0", 24, 72, 37, 0, 0.0, 360.0, -90.0, 90.0, 0),
    ("c24_72x37_fs1", 24, 72, 37, 1, 0.0, 360.0, -90.0, 90.0, 0),
    ("c24_36x19_fs2", 24, 36, 19, 2, 0.0, 360.0, -90.0, 90.0, 0),
    ("c24_72x36_centery", 24, 72, 36, 0, 0.0, 360.0, -90.0, 90.0, 1),
    ("c24_regional", 24, 80, 51, 0, 230.0, 310.0, 15.0, 65.0, 0),
]


def build_driver(tmp):
    fr, lib = os.path.join(REF, "tools", "fregrid"), os.path.join(REF, "tools", "libfrencutils")
    exe = os.path.join(tmp, "bilinear_ref_driver")
    subprocess.check_call(["gcc", "-O2", "-w", "-I", os.path.join(ROOT, "tests", "capi", "typecheck_shim"), "-I", fr, "-I", lib,
                           os.path.join(ROOT, "tests", "capi", "bilinear_ref_driver.c"), os.path.join(fr, "bilinear_interp.c"),
                           os.path.join(lib, "mosaic_util.c"), os.path.join(lib, "mpp.c"), "-lm", "-o", exe])
    return exe


def halo_inputs(fg, N):
    """reference-generator centres, halo'd with fg_halo_map (init_halo zeros at the corners); contacts from the corners"""
    lonc, latc, lont, latt = gridutil.ref_gnomonic_corners(N, centres=True)
    nx = [N] * 6
    contacts = fg.find_contacts(nx, nx, list(lonc), list(latc))
    _, m = fg.halo_map(nx, nx, contacts)
    F = (N + 2) ** 2

    def halo(tiles):
        h = np.zeros(6 * F)
        v = h.reshape(6, N + 2, N + 2)
        v[:, 1:-1, 1:-1] = tiles
        e = np.nonzero(m >= 0)[0]
        h[e] = h[m[e]]                               # sources are interior elements
        return h.reshape(6, N + 2, N + 2)
    return lont, latt, halo


def fields(lont, latt):
    s = 10.0 * np.sin(lont + latt) + 3.0 * np.cos(2.0 * latt)
    s_miss = s.copy().reshape(-1)
    s_miss[::37] = MISSING
    u = 20.0 * np.cos(latt) + 5.0 * np.sin(2.0 * lont)
    v = 8.0 * np.sin(lont) * np.cos(latt)
    return s, s_miss.reshape(s.shape), u, v


def run_case(exe, tmp, N, nlon, nlat, fs, lb, le, ab, ae, cy, lh, ah, flds, setup_only=False, timeout=None):
    inp = os.path.join(tmp, "in.bin")
    out = os.path.join(tmp, "out")
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    with open(inp, "wb") as f:
        np.array([N, nlon, nlat, fs, cy, 1 if setup_only else 0], dtype=np.int32).tofile(f)
        np.array([lb, le, ab, ae, MISSING]).tofile(f)
        lh.astype(np.float64).tofile(f)
        ah.astype(np.float64).tofile(f)
        if not setup_only:
            for a in flds:
                a.astype(np.float64).tofile(f)
    res = subprocess.run([exe, inp, out], cwd=out, capture_output=True, text=True, timeout=timeout)
    if res.returncode:
        raise RuntimeError(res.stdout[-2000:] + res.stderr[-2000:])
    assert "global sweep" not in res.stdout, "the reference took its fallback sweep"
    return out, float(open(os.path.join(out, "setup_s.txt")).read())


def main():
    fg = __graft_entry__.load_package()
    tmp = tempfile.mkdtemp(prefix="bilinear_ref_")
    try:
        exe = build_driver(tmp)
        lont, latt, halo = halo_inputs(fg, 24)
        lh, ah = halo(lont), halo(latt)
        s, s_miss, u, v = fields(lont, latt)
        hal = [halo(a) for a in (s, s_miss, u, v)]
        for name, N, nlon, nlat, fs, lb, le, ab, ae, cy in CASES:
            out, _ = run_case(exe, tmp, N, nlon, nlat, fs, lb, le, ab, ae, cy, lh, ah, hal)
            nyf, nxf = (2 ** fs) * (nlat - 1) + 1, (2 ** fs) * nlon
            rd = lambda f, dt=np.float64: np.fromfile(os.path.join(out, f), dtype=dt)
            np.savez_compressed(
                os.path.join(HERE, f"bilinear_{name}.npz"),
                config=np.array([N, nlon, nlat, fs, cy, lb, le, ab, ae, MISSING]),
                lont_halo=lh, latt_halo=ah, s=s, s_miss=s_miss, u=u, v=v,
                index=rd("index.bin", np.int32).reshape(nxf * nyf, 3), weight=rd("weight.bin").reshape(nxf * nyf, 4),
                s_plain=rd("s_plain.bin").reshape(nlat, nlon), s_missing=rd("s_miss.bin").reshape(nlat, nlon),
                s_fill=rd("s_fill.bin").reshape(nlat, nlon), u_out=rd("u.bin").reshape(nlat, nlon), v_out=rd("v.bin").reshape(nlat, nlon))
            if name == "c24_72x37_fs0":
                lay = open(os.path.join(out, "layout.txt")).read()
                np.savez_compressed(os.path.join(HERE, "bilinear_write_layout.npz"), layout=np.array(lay),
                                    put_index=rd("put_index.bin", np.uint8), put_weight=rd("put_weight.bin", np.uint8))
            print(name, "ok")
        base = {}
        for N, nlon, nlat, limit in ((96, 360, 181, 600), (384, 1440, 721, 300)):
            lo, la, hl = halo_inputs(fg, N)
            try:
                t0 = time.time()
                _, sec = run_case(exe, tmp, N, nlon, nlat, 0, 0.0, 360.0, -90.0, 90.0, 0, hl(lo), hl(la), [], setup_only=True,
                                  timeout=limit)
                base[f"C{N}->{nlon}x{nlat}"] = {"setup_s_cpu": sec, "wall_s": time.time() - t0}
            except subprocess.TimeoutExpired:
                base[f"C{N}->{nlon}x{nlat}"] = {"setup_s_cpu": None, "note": f"not finished within {limit} s"}
            print(base)
        with open(os.path.join(HERE, "bilinear_cpu_baseline.json"), "w") as f:
            json.dump(base, f, indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
