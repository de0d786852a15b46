"""Inputs of the --extrapolate / --dst_vgrid fixtures (tests/golden/extrapolate_*.npz), rebuilt from exact arithmetic so that no
input array is stored, and the recipe that runs the REFERENCE's do_extrapolate / do_vertical_interp on them
(tests/capi/extrapolate_ref_driver.c, compiled against the reference's sources in a temporary directory outside the repository).
Shared by tests/golden/make_golden_extrapolate.py, tests/test_extrapolate_cpu.py and tests/test_gpu_extrapolate.py."""
import hashlib
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
REF = os.environ.get("FRE_REFERENCE", "/root/reference")
D2R = np.pi / 180.0
NSAMPLE = 4096


def _field(ni, nj, nk):
    k, j, i = np.meshgrid(np.arange(nk), np.arange(nj), np.arange(ni), indexing="ij")
    return ((7 * i + 13 * j + 5 * k) % 97) / 8.0, i, j, k


def _uniform(n, begin, step):
    return (begin + (np.arange(n) + 0.5) * step) * D2R


def _ellipse(x, y, cx, cy, a, b):
    return (x - cx) ** 2 * (b * b) + (y - cy) ** 2 * (a * a) <= a * a * b * b


def _continents(ni, nj, i, j, k):
    """continents-like land in whole degrees (integer arithmetic); the coasts move a little with the level"""
    x, y = i * 360 // ni, j * 180 // nj
    land = y < 14 - k
    for cx, cy, a, b in ((20, 95, 22 - k, 38), (60, 140, 55, 22 - k), (100, 110, 12, 8), (135, 65, 20 - 2 * k, 16), (260, 135, 36, 28 - k),
                         (298, 75, 16, 34), (320, 165, 20, 9), (355, 95, 9, 30), (5, 95, 9, 30)):
        land = land | _ellipse(x, y, cx, cy, a, b)
    return land


def extrap_case(name):
    """-> dict(ni, nj, nk, is_cyclic, missing, stop_crit, lon, lat, data [nk, nj, ni])"""
    missing, stop_crit, cyc = -1.0e20, 0.005, 1
    if name == "warm":                       # the land mask changes with the level: warm start, both directions
        ni, nj, nk = 72, 45, 3
        data, i, j, k = _field(ni, nj, nk)
        land = ((i >= 10 + 4 * k) & (i < 30 + 4 * k) & (j >= 12) & (j < 30)) | ((i >= 50) & (i < 60) & (j >= 5 + 3 * k) & (j < 20 + 3 * k)) \
            | (((i >= 68) | (i < 3)) & (j >= 30) & (j < 40))
        lon, lat = _uniform(ni, 0.0, 5.0), _uniform(nj, -90.0, 4.0)
    elif name == "regional":                 # non-cyclic: zero boundary on all four sides
        ni, nj, nk, cyc = 60, 40, 2, 0
        data, i, j, k = _field(ni, nj, nk)
        land = ((i < 4) & (j >= 10) & (j < 25)) | ((i >= 55) & (j >= 5) & (j < 30)) | ((j < 3) & (i >= 20) & (i < 40)) \
            | ((j >= 37) & (i >= 10) & (i < 30)) | ((i >= 25 + k) & (i < 35) & (j >= 15) & (j < 24 + k))
        lon, lat = _uniform(ni, 230.0, 1.0), _uniform(nj, 10.0, 1.0)
    elif name == "stretched":                # non-uniform dyu / dyt and dxu / dxt
        ni, nj, nk = 72, 46, 2
        data, i, j, k = _field(ni, nj, nk)
        land = ((i >= 20) & (i < 41 - 3 * k) & (j >= 8) & (j < 33)) | ((i >= 66) | (i < 2)) & (j >= 20) & (j < 40) | (j < 2 + k)
        a, b = np.arange(ni), np.arange(nj)
        lon = (2.5 + 5.0 * a + 0.02 * a * (71 - a)) * D2R
        lat = (-88.0 + 176.0 * (b + 0.004 * b * (45 - b)) / 45.0) * D2R
    elif name == "cap":                      # stop_crit = 0: runs to the cap, the reference prints 3999
        ni, nj, nk, stop_crit = 72, 45, 1, 0.0
        data, i, j, k = _field(ni, nj, nk)
        land = ((i >= 15) & (i < 40) & (j >= 14) & (j < 32)) | (j < 4)
        lon, lat = _uniform(ni, 0.0, 5.0), _uniform(nj, -90.0, 4.0)
    elif name == "none_missing":
        ni, nj, nk = 72, 45, 2
        data, i, j, k = _field(ni, nj, nk)
        land = np.zeros_like(i, dtype=bool)
        lon, lat = _uniform(ni, 0.0, 5.0), _uniform(nj, -90.0, 4.0)
    elif name == "eps":                      # fabs(v - missing) <= 1e-10, not ==
        ni, nj, nk, missing = 48, 30, 2, -999.0
        data, i, j, k = _field(ni, nj, nk)
        land = ((i >= 8) & (i < 20) & (j >= 6 + k) & (j < 18))
        near = (i >= 28) & (i < 36) & (j >= 10) & (j < 20 - 2 * k)          # counted as missing
        far = (i >= 40) & (i < 44) & (j >= 4) & (j < 8)                       # 3e-10 away: valid data
        data = np.where(near, missing + 5e-11, np.where(far, missing + 3e-10, data))
        lon, lat = _uniform(ni, 0.0, 7.5), _uniform(nj, -90.0, 6.0)
    elif name == "whole_level":              # level 1 is all missing: the solution of level 0 is carried
        ni, nj, nk = 72, 45, 2
        data, i, j, k = _field(ni, nj, nk)
        land = ((i >= 30) & (i < 48) & (j >= 10) & (j < 28)) | (k == 1)
        lon, lat = _uniform(ni, 0.0, 5.0), _uniform(nj, -90.0, 4.0)
    elif name in ("real_360x180", "real_1440x720"):
        ni, nj, nk = (360, 180, 3) if name == "real_360x180" else (1440, 720, 1)
        data, i, j, k = _field(ni, nj, nk)
        land = _continents(ni, nj, i, j, k)
        lon, lat = _uniform(ni, 0.0, 360.0 / ni), _uniform(nj, -90.0, 180.0 / nj)
    else:
        raise KeyError(name)
    data = np.where(land, missing, data).astype(np.float64)
    return dict(ni=ni, nj=nj, nk=nk, is_cyclic=cyc, missing=missing, stop_crit=stop_crit, lon=lon, lat=lat, data=data)


SMALL_CASES = ["warm", "regional", "stretched", "cap", "none_missing", "eps", "whole_level"]
LARGE_CASES = ["real_360x180", "real_1440x720"]


def timing_case(ni, nj, nk):
    """scripts/extrap_time.py's inputs: the continents-like mask on nk levels"""
    data, i, j, k = _field(ni, nj, nk)
    land = _continents(ni, nj, i, j, k % 3)
    return dict(ni=ni, nj=nj, nk=nk, is_cyclic=1, missing=-1.0e20, stop_crit=0.005, lon=_uniform(ni, 0.0, 360.0 / ni),
                lat=_uniform(nj, -90.0, 180.0 / nj), data=np.where(land, -1.0e20, data).astype(np.float64))


def vertical_case(name):
    """-> dict(nxy, z1, z2, data [nk1, nxy])"""
    nxy = 40 * 30
    z1 = np.array([5.0, 15.0, 30.0, 50.0, 80.0, 120.0, 200.0])
    if name == "vert_7to9":                  # kstart = 1, kend = 7 < nk2 - 1, z2[2] == z1[1]
        z2 = np.array([2.0, 10.0, 15.0, 25.0, 40.0, 70.0, 110.0, 190.0, 250.0])
    elif name == "vert_same":                # need_interp = 0
        z2 = z1.copy()
    else:
        raise KeyError(name)
    k, l = np.meshgrid(np.arange(z1.size), np.arange(nxy), indexing="ij")
    return dict(nxy=nxy, z1=z1, z2=z2, data=(((7 * l + 13 * k) % 97) / 8.0).astype(np.float64))


VERTICAL_CASES = ["vert_7to9", "vert_same"]


def sample_index(n):
    return (np.arange(NSAMPLE, dtype=np.int64) * n) // NSAMPLE


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def golden_path(name):
    return os.path.join(GOLDEN, f"extrapolate_{name}.npz")


# ------------------------------------------------------------------------------------------------ the reference, compiled
def reference_present():
    return os.path.exists(os.path.join(REF, "tools", "fregrid", "fregrid_util.c"))


def build_driver(tmp):
    """gcc -O2 without -march: the reference's default build, no contraction.  Nothing is kept outside `tmp`."""
    fr, lib = os.path.join(REF, "tools", "fregrid"), os.path.join(REF, "tools", "libfrencutils")
    inc = ["-I", os.path.join(HERE, "capi", "typecheck_shim"), "-I", fr, "-I", lib]
    obj, exe = os.path.join(tmp, "fu.o"), os.path.join(tmp, "extrapolate_ref_driver")
    subprocess.check_call(["gcc", "-O2", "-w", "-DNC_UNLIMITED=0L", "-ffunction-sections", "-fdata-sections", "-c"] + inc +
                          [os.path.join(fr, "fregrid_util.c"), "-o", obj])
    subprocess.check_call(["gcc", "-O2", "-w", "-DNC_UNLIMITED=0L", "-ffunction-sections", "-fdata-sections"] + inc +
                          [os.path.join(HERE, "capi", "extrapolate_ref_driver.c"), obj, os.path.join(lib, "mpp.c"),
                           os.path.join(lib, "interp.c"), os.path.join(lib, "mosaic_util.c"), os.path.join(lib, "create_xgrid.c"),
                           "-Wl,--gc-sections", "-lm", "-o", exe])
    return exe


def _run(exe, tmp, header, params, arrays):
    inp, out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out")
    os.makedirs(out, exist_ok=True)
    with open(inp, "wb") as f:
        np.array(header, dtype=np.int32).tofile(f)
        np.array(params, dtype=np.float64).tofile(f)
        for a in arrays:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    res = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=900)
    if res.returncode:
        raise RuntimeError(res.stdout[-2000:] + res.stderr[-2000:])
    return out, res.stdout


def run_ref_extrap(exe, tmp, c):
    """-> (out [nk, nj, ni], iters [nk], printed maxres strings [nk], seconds)"""
    out, txt = _run(exe, tmp, [0, c["ni"], c["nj"], c["nk"], c["is_cyclic"]], [c["missing"], c["stop_crit"]],
                    [c["lon"], c["lat"], c["data"]])
    lines = re.findall(r"Stopped after (\d+) iterations, maxres = (\S+)", txt)
    assert len(lines) == c["nk"], txt
    data = np.fromfile(os.path.join(out, "out.bin")).reshape(c["nk"], c["nj"], c["ni"])
    return data, np.array([int(a) for a, _ in lines], dtype=np.int32), [b for _, b in lines], \
        float(open(os.path.join(out, "seconds.txt")).read())


def run_ref_vertical(exe, tmp, c):
    """-> (out [nk2 or nk1, nxy], kstart, kend, need_interp)"""
    out, _ = _run(exe, tmp, [1, c["nxy"], c["z1"].size, c["z2"].size, 0], [0.0, 0.0], [c["z1"], c["z2"], c["data"]])
    ks, ke, need = (int(v) for v in open(os.path.join(out, "kinfo.txt")).read().split())
    return np.fromfile(os.path.join(out, "out.bin")).reshape(-1, c["nxy"]), ks, ke, need


def fixture_of(name, out, iters, printed, seconds):
    """what a fixture file stores for an extrapolation case"""
    d = dict(iters=iters, maxres_printed=np.array(printed), sha256=np.array(sha256(out)))
    if name in LARGE_CASES:
        d["sample"] = out.reshape(-1)[sample_index(out.size)]
    else:
        d["out"] = out
    return d
