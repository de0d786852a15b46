"""Inputs of the make_topog fixtures (tests/golden/topog_*.npz) and the recipe that runs the REFERENCE's conserve_interp,
filter_topo, show_deepest and process_topo on them (tests/capi/topog_ref_driver.c, compiled with the reference's topog.c, interp.c,
create_xgrid.c, mosaic_util.c, mpp.c and mpp_domain.c in a temporary directory outside the repository).  Two kinds of case:
CHAIN cases run create_realistic_topog's whole chain from a topography file's axes and field; STAGE cases feed filter_topo and
process_topo a hand-made depth.  The fixtures hold their inputs, so a test loads one with `load()` and never rebuilds a grid.
Shared by tests/golden/make_golden_topog.py, tests/test_topog_cpu.py, tests/test_gpu_topog.py and scripts/topog_time.py."""
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
REF = os.environ.get("FRE_REFERENCE", "/root/reference")
D2R = np.pi / 180
R2D = 180 / np.pi
MISSING = -1.e34
NC = {np.dtype(np.int32): 4, np.dtype(np.float32): 5, np.dtype(np.float64): 6}
# fg_topog_opts' switches in the order of the driver's header, with make_topog.c's defaults (:297-323)
INT_OPTS = ("tripolar_grid", "cyclic_x", "cyclic_y", "fill_first_row", "filter_topog", "num_filter_pass", "smooth_topo_allow_deepening",
            "round_shallow", "fill_shallow", "deepen_shallow", "full_cell", "flat_bottom", "adjust_topo", "fill_isolated_cells",
            "dont_change_landmask", "kmt_min", "open_very_this_cell", "use_great_circle_algorithm", "on_grid")
DBL_OPTS = ("scale_factor", "min_thickness", "fraction_full_cell")
DEFAULTS = dict(tripolar_grid=0, cyclic_x=0, cyclic_y=0, fill_first_row=0, filter_topog=0, num_filter_pass=1, smooth_topo_allow_deepening=0,
                round_shallow=0, fill_shallow=0, deepen_shallow=0, full_cell=0, flat_bottom=0, adjust_topo=1, fill_isolated_cells=1,
                dont_change_landmask=0, kmt_min=2, open_very_this_cell=1, use_great_circle_algorithm=0, on_grid=0,
                scale_factor=1.0, min_thickness=0.1, fraction_full_cell=0.2)
ZW = np.array([10., 25., 45., 75., 120., 200., 350., 600., 1000., 1600., 2400., 3400., 4600., 5800.])

CHAIN = ["tripolar", "regional", "torus", "cube_c6", "fill_first_row", "on_grid", "no_vgrid", "cube_c6_gca"]
PROCESS_OPTS = dict(defaults={}, full_cell=dict(full_cell=1), flat_bottom=dict(flat_bottom=1), no_adjust=dict(adjust_topo=0),
                    no_fill_isolated=dict(fill_isolated_cells=0), keep_landmask=dict(dont_change_landmask=1),
                    dont_open_very_this_cell=dict(open_very_this_cell=0), fraction0=dict(fraction_full_cell=0.0),
                    fraction0_closed=dict(fraction_full_cell=0.0, open_very_this_cell=0),
                    round_shallow=dict(round_shallow=1, kmt_min=4), deepen_shallow=dict(deepen_shallow=1, kmt_min=4),
                    fill_shallow=dict(fill_shallow=1, kmt_min=4), kmt_min4=dict(kmt_min=4), min_thickness0=dict(min_thickness=0.0),
                    tripolar_cyclic=dict(tripolar_grid=1, cyclic_x=1), torus=dict(cyclic_x=1, cyclic_y=1))
STAIRS = [f"stairs_{w}x{h}" for w in (67, 130) for h in (1, 2, 9)]
FILTER = ["filter_2x5", "filter_5x2", "filter_3x3", "filter_65x4", "filter_65x4_p0", "filter_65x4_p3", "filter_65x4_deepen", "filter_9x8_p3_deepen"]
STAGE = ["process_" + k for k in PROCESS_OPTS] + STAIRS + ["stale_halo", "stale_halo_keep_landmask"] + FILTER
CASES = CHAIN + STAGE

CHAIN_OUT_D = ("x_src", "y_src", "depth_src", "mask_src", "depth_remap")
OUT_D = ("depth_filter", "depth_final")
COUNTS = ("isolated_filled", "partial_restricted", "shallow_modified", "verdict")


def package():
    """the package under the name the tests load it by (tests/conftest.py)"""
    if "fre_nctools_amd" not in sys.modules:
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.load_package()
    return sys.modules["fre_nctools_amd"]


def golden_path(name):
    return os.path.join(GOLDEN, f"topog_{name}.npz")


def load(name):
    with np.load(golden_path(name)) as z:
        return {k: z[k] for k in z.files}


def options(fx):
    """the switches of a case or fixture as keyword arguments of fg.Topog"""
    return {k: (float(fx[k]) if k in DBL_OPTS else int(fx[k])) for k in INT_OPTS + DBL_OPTS}


def _wave(lon_deg, lat_deg, seed, nterms=6):
    """a smooth seeded function of position in about [-1, 1]"""
    rng = np.random.default_rng(seed)
    lon, lat = np.asarray(lon_deg) * D2R, np.asarray(lat_deg) * D2R
    x, y, z = np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)
    f = np.zeros(np.broadcast(lon, lat).shape)
    for _ in range(nterms):
        k = rng.normal(size=3) * 3.0
        f += np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 2 * np.pi))
    return f / np.sqrt(nterms)


def axes(nx, ny, west=0.0, east=360.0, south=-90.0, north=90.0):
    """cell-centre axes of a topography file, degrees"""
    return west + (np.arange(nx) + 0.5) * ((east - west) / nx), south + (np.arange(ny) + 0.5) * ((north - south) / ny)


def elevation(xt, yt, seed, dtype, sign=-1.0, nmissing=40):
    """a field in the file's type: sign * depth, depth about 2500 +- 3500 m (a quarter of it land), a few missing cells"""
    lon, lat = np.meshgrid(xt, yt)
    depth = 2500.0 + 3500.0 * _wave(lon, lat, seed) + 300.0 * _wave(3 * lon, 2 * lat, seed + 1)
    v = (sign * depth).astype(dtype)
    rng = np.random.default_rng(seed + 2)
    for _ in range(nmissing):
        v[rng.integers(0, v.shape[0]), rng.integers(0, v.shape[1])] = dtype(MISSING) if dtype != np.int32 else np.int32(-2147483647)
    return v


def latlon_corners_deg(nx, ny, west, east, south, north):
    x, y = np.meshgrid(west + np.arange(nx + 1) * ((east - west) / nx), south + np.arange(ny + 1) * ((north - south) / ny))
    return x, y


def _chain(x_dst, y_dst, src, seed, dtype, sign=-1.0, zw=ZW, **opts):
    xt, yt = axes(*src)
    data = elevation(xt, yt, seed, dtype, sign)
    missing = float(dtype(MISSING)) if dtype != np.int32 else -2147483647.0           # the attribute has the variable's type
    c = dict(DEFAULTS, scale_factor=sign, **opts)
    c.update(mode=0, x_dst=np.ascontiguousarray(x_dst), y_dst=np.ascontiguousarray(y_dst), xt_src=xt, yt_src=yt, data=data, missing=missing,
             zw=np.asarray(zw, dtype=np.float64))
    return c


def special_depth(nx, ny, seed, zw=ZW):
    """a depth field for process_topo: smooth ocean with land, and cells exactly on a level, midway between two, a hair above a
    level (thinner than min_thickness), deeper than zw[nk-1] and shallower than zw[0]"""
    x, y = np.meshgrid(np.arange(nx) * (360.0 / nx), -60 + np.arange(ny) * (120.0 / ny))
    d = np.maximum(0.0, 1800.0 + 3800.0 * _wave(x, y, seed, 8))
    rng = np.random.default_rng(seed + 5)
    nk = zw.size
    special = [zw[k] for k in range(nk)] + [0.5 * (zw[k] + zw[k + 1]) for k in range(nk - 1)] + [zw[k] + 0.05 for k in range(nk)] + \
              [zw[k] + 0.1 for k in range(nk)] + [zw[k] - 0.05 for k in range(nk)] + [zw[-1] + 0.5, zw[-1] + 1.5, zw[-1] + 700.0, zw[0] * 0.5, 1.e-3,
               zw[0] + 0.2 * zw[0], zw[1] - 1.0, zw[3] + 2.0, zw[5] + 10.0, zw[8] + 79.0, zw[8] + 81.0]
    flat = d.reshape(-1)
    flat[rng.choice(flat.size, len(special), replace=False)] = special
    return d


def stairs_depth(w, h, zw=ZW):
    """hand-made staircases: levels that fall from west to east and from north to south in steps of unequal length, with one-cell
    potholes and one-cell-wide trenches cut into them, so that remove_isolated_cells' fill runs along the rows and down them"""
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    lev = np.clip(zw.size - 1 - ((i * 5) // 13 + (j * 7) // 4) % zw.size, 0, zw.size - 1)
    lev = np.where((i + 2 * j) % 5 == 0, np.minimum(lev + 3, zw.size - 1), lev)           # potholes on a lattice
    lev = np.where((i % 11 == 3) & (j % 3 != 1), np.minimum(lev + 2, zw.size - 1), lev)   # short trenches
    d = zw[lev] - 0.25 * (zw[lev] - np.where(lev > 0, zw[np.maximum(lev - 1, 0)], 0.0)) * ((i * 7 + j * 3) % 4) / 4.0
    d = np.where((i * 3 + j * 5) % 17 == 0, 0.0, d)                                      # scattered land
    return np.ascontiguousarray(d)


def halo_depth(nx=12, ny=6, zw=ZW):
    """a cyclic_x field whose first column is deep and is reset by the sweep while the last column's fill reads it through the halo"""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    lev = 3 + (i + j) % 4
    lev = np.where(i == 0, 10 + j % 3, lev)
    lev = np.where(i == nx - 1, 9 + (j + 1) % 3, lev)
    lev = np.where(i == 1, 2, lev)
    d = zw[lev] - 1.0 - ((i + 2 * j) % 3)
    d[0, 5] = 0.0
    d[3, nx - 1] = 0.0
    return np.ascontiguousarray(d)


def _stage(depth, zw=ZW, **opts):
    c = dict(DEFAULTS, **opts)
    c.update(mode=1, depth_in=np.ascontiguousarray(depth, dtype=np.float64), zw=np.asarray(zw, dtype=np.float64))
    return c


def filter_depth(nx, ny, seed):
    """depths with land inside the stencils and along the border"""
    x, y = np.meshgrid(np.arange(nx) * (360.0 / max(nx, 8)), -40 + np.arange(ny) * (80.0 / max(ny, 8)))
    d = np.maximum(0.0, 900.0 + 2500.0 * _wave(x, y, seed, 9))
    rng = np.random.default_rng(seed)
    d.reshape(-1)[rng.choice(d.size, max(1, d.size // 9), replace=False)] = 0.0
    if (nx, ny) == (3, 3):                                  # the one filtered cell is ocean, with land and ocean round it
        d = np.array([[700.0, 0.0, 1310.5], [2250.25, 2234.5, 0.0], [310.0, 1800.75, 90.5]])
    return d


def case_inputs(name):
    """-> dict: the switches (INT_OPTS, DBL_OPTS), mode, zw and, for a chain case, x_dst, y_dst (degrees), xt_src, yt_src, data,
    missing; for a stage case depth_in [ny, nx]"""
    fg = package()
    if name in ("tripolar", "no_vgrid"):
        lon, lat = fg.tripolar_corners(24, 18)
        return _chain(lon * R2D, lat * R2D, (72, 36), 11, np.float32, tripolar_grid=1, cyclic_x=1, zw=ZW if name == "tripolar" else ZW[:0])
    if name in ("regional", "fill_first_row"):
        x, y = latlon_corners_deg(17, 11, 20.0, 105.0, -33.0, 44.0)
        return _chain(x, y, (90, 45), 21, np.int32, filter_topog=1, num_filter_pass=2, fill_first_row=int(name == "fill_first_row"))
    if name == "torus":
        x, y = latlon_corners_deg(13, 7, 0.0, 360.0, -70.0, 70.0)
        return _chain(x, y, (60, 30), 31, np.float64, sign=1.0, cyclic_x=1, cyclic_y=1, filter_topog=1)
    if name in ("cube_c6", "cube_c6_gca"):
        lon, lat = fg.gnomonic_ed_corners(6)
        return _chain(lon[2] * R2D, lat[2] * R2D, (72, 36), 41, np.float32, use_great_circle_algorithm=int(name == "cube_c6_gca"), filter_topog=1)
    if name == "on_grid":
        x, y = latlon_corners_deg(20, 10, 0.0, 360.0, -90.0, 90.0)
        return _chain(x, y, (20, 10), 51, np.float64, on_grid=1)
    if name.startswith("process_"):
        return _stage(special_depth(21, 13, 61), **PROCESS_OPTS[name[len("process_"):]])
    if name.startswith("stairs_"):
        w, h = (int(v) for v in name[len("stairs_"):].split("x"))
        return _stage(stairs_depth(w, h), cyclic_x=int(h != 2), cyclic_y=int(h == 1))
    if name == "stale_halo":
        return _stage(halo_depth(), cyclic_x=1)
    if name == "stale_halo_keep_landmask":
        return _stage(halo_depth(), cyclic_x=1, dont_change_landmask=1)
    if name.startswith("filter_"):
        p = name.split("_")
        nx, ny = (int(v) for v in p[1].split("x"))
        passes = [int(q[1:]) for q in p[2:] if q[0] == "p" and q[1:].isdigit()]
        return _stage(filter_depth(nx, ny, 71 + nx), zw=ZW[:0], filter_topog=1, num_filter_pass=passes[0] if passes else 1,
                      smooth_topo_allow_deepening=int("deepen" in p))
    raise KeyError(name)


def shape_of(c):
    """(ny, nx) of the model grid"""
    return tuple(np.asarray(c["depth_in"]).shape) if int(c["mode"]) == 1 else (c["x_dst"].shape[0] - 1, c["x_dst"].shape[1] - 1)


def write_driver_input(path, c):
    ny, nx = shape_of(c)
    chain = int(c["mode"]) == 0
    nx_src, ny_src = (c["xt_src"].size, c["yt_src"].size) if chain else (0, 0)
    dtype = NC[np.asarray(c["data"]).dtype] if chain else 6
    hdr = [int(c["mode"]), nx, ny, nx_src, ny_src, dtype, np.asarray(c["zw"]).size] + [int(c[k]) for k in INT_OPTS] + [0, 0]
    assert len(hdr) == 28
    with open(path, "wb") as f:
        np.array(hdr, dtype=np.int32).tofile(f)
        np.array([float(c["scale_factor"]), float(c["min_thickness"]), float(c["fraction_full_cell"]), float(c["missing"]) if chain else 0.0]).tofile(f)
        np.asarray(c["zw"], dtype=np.float64).tofile(f)
        if chain:
            for k in ("x_dst", "y_dst", "xt_src", "yt_src"):
                np.ascontiguousarray(c[k], dtype=np.float64).tofile(f)
            np.ascontiguousarray(c["data"]).tofile(f)
        else:
            np.ascontiguousarray(c["depth_in"], dtype=np.float64).tofile(f)


def build_driver(tmp):
    """gcc -O2 without -march: the reference's default build, no contraction.  Nothing is kept outside `tmp`."""
    lib = os.path.join(REF, "tools", "libfrencutils")
    topog = os.path.join(REF, "tools", "make_topog")
    inc = ["-I", os.path.join(HERE, "capi", "typecheck_shim"), "-I", lib, "-I", topog]
    flags = ["gcc", "-O2", "-w", "-DNC_UNLIMITED=0L", "-ffunction-sections", "-fdata-sections"]
    exe = os.path.join(tmp, "topog_ref_driver")
    srcs = [os.path.join(HERE, "capi", "topog_ref_driver.c"), os.path.join(topog, "topog.c")] + \
           [os.path.join(lib, s) for s in ("interp.c", "create_xgrid.c", "mosaic_util.c", "mpp.c", "mpp_domain.c")]
    subprocess.check_call(flags + inc + srcs + ["-Wl,--gc-sections", "-lm", "-o", exe])
    return exe


def run_ref(exe, tmp, c):
    """-> dict of the driver's dumps, the counts parsed from the reference's debug notes, and seconds [3].  A fatal error of the
    reference raises CalledProcessError."""
    inp, out = os.path.join(tmp, "tp_in.bin"), os.path.join(tmp, "tp_out")
    os.makedirs(out, exist_ok=True)
    write_driver_input(inp, c)
    p = subprocess.run([exe, inp, out], check=True, capture_output=True, text=True, timeout=3000)
    ny, nx = shape_of(c)
    nk = np.asarray(c["zw"]).size
    r = {}
    if int(c["mode"]) == 0:
        jstart, jend = (int(v) for v in open(os.path.join(out, "trim.txt")).read().split())
        ny_now, nxs = jend - jstart + 1, c["xt_src"].size
        r["jstart"], r["jend"] = np.array(jstart), np.array(jend)
        shapes = dict(x_src=(ny_now + 1, nxs + 1), y_src=(ny_now + 1, nxs + 1), depth_src=(ny_now, nxs), mask_src=(ny_now, nxs), depth_remap=(ny, nx))
        for k in CHAIN_OUT_D:
            r[k] = np.fromfile(os.path.join(out, k + ".bin"), dtype=np.float64).reshape(shapes[k])
    for k in OUT_D:
        r[k] = np.fromfile(os.path.join(out, k + ".bin"), dtype=np.float64).reshape(ny, nx)
    if nk:
        r["num_levels"] = np.fromfile(os.path.join(out, "num_levels.bin"), dtype=np.int32).reshape(ny, nx)

    def count(pattern):
        m = re.search(pattern, p.stdout)
        return np.array(int(m.group(1)) if m else 0)
    r["isolated_filled"] = count(r"remove_isolated_cells: found (\d+) and filled them in")
    r["partial_restricted"] = count(r"restrict_partial_cells: Found (\d+) cells")
    r["shallow_modified"] = count(r"enforce_min_depth: Modified (\d+) shallow cells")
    r["verdict"] = np.array(-1 if not nk else 0 if "Re-think the vertical grid" in p.stdout else 1 if "is wasteful" in p.stdout else 2)
    r["seconds"] = np.array([float(v) for v in open(os.path.join(out, "seconds.txt")).read().split()])
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatements used by the CPU tests to show that a case has teeth (never as a reference)

def kmt_ht(depth, zw, c):
    """process_topo :574-645 in numpy: the haloed kmt and ht before remove_isolated_cells"""
    ny, nx = depth.shape
    nk = zw.size
    ht = np.zeros((ny + 2, nx + 2))
    kmt = -np.ones((ny + 2, nx + 2), dtype=np.int64)
    for j in range(ny):
        for i in range(nx):
            h, k = depth[j, i], -1
            if h > 0:
                if h < zw[0]:
                    k = 0
                elif h > zw[-1]:
                    k = nk - 1
                else:
                    k = next(q for q in range(1, nk) if h <= zw[q])
                    if zw[k] - h > h - zw[k - 1]:
                        k -= 1
                if zw[k] < h:
                    if h - zw[k] < float(c["min_thickness"]) or k == nk - 1:
                        h = zw[k]
                    else:
                        k += 1
            if int(c["full_cell"]) and h > 0:
                h = zw[k]
            if int(c["flat_bottom"]) and h > 0:
                h, k = zw[-1], nk - 1
            ht[j + 1, i + 1], kmt[j + 1, i + 1] = h, k
    halo_fill(ht, kmt, c)
    return ht, kmt


def halo_fill(ht, kmt, c):
    for a in (ht, kmt):
        if int(c["tripolar_grid"]):
            a[-1, 1:-1] = a[-2, 1:-1][::-1]
        elif int(c["cyclic_y"]):
            a[0, 1:-1] = a[-2, 1:-1]
            a[-1, 1:-1] = a[1, 1:-1]
        if int(c["cyclic_x"]):
            a[:, 0] = a[:, -2]
            a[:, -1] = a[:, 1]


def _quadmin(a):
    return np.minimum(np.minimum(a[:-1, :-1], a[:-1, 1:]), np.minimum(a[1:, :-1], a[1:, 1:]))


def isolated_jacobi(ht, kmt, c):
    """remove_isolated_cells with every cell evaluated on the arrays as they were before the sweep -> interior (ht, kmt)"""
    ny, nx = ht.shape[0] - 2, ht.shape[1] - 2
    nj_max = ny - 1 if int(c["tripolar_grid"]) else ny
    qk, qh = _quadmin(kmt), _quadmin(ht)
    k = np.maximum(np.maximum(qk[1:, 1:], qk[1:, :-1]), np.maximum(qk[:-1, 1:], qk[:-1, :-1]))
    t = np.maximum(np.maximum(qh[1:, 1:], qh[1:, :-1]), np.maximum(qh[:-1, 1:], qh[:-1, :-1]))
    hi, ki = ht[1:-1, 1:-1].copy(), kmt[1:-1, 1:-1].copy()
    change = ((k >= 0) | (not int(c["dont_change_landmask"]))) & (ki != k)
    change[nj_max:] = False
    hi[change], ki[change] = t[change], k[change]
    return hi, ki


def isolated_sequential(ht, kmt, c, refresh_halo=False):
    """the sweep in place, j then i; refresh_halo: the boundary condition re-applied after every cell (what the reference does NOT do)"""
    ht, kmt = ht.copy(), kmt.copy()
    ny, nx = ht.shape[0] - 2, ht.shape[1] - 2
    nj_max = ny - 1 if int(c["tripolar_grid"]) else ny
    dcl = int(c["dont_change_landmask"])
    for j in range(1, nj_max + 1):
        for i in range(1, nx + 1):
            k = max(kmt[j:j + 2, i:i + 2].min(), kmt[j:j + 2, i - 1:i + 1].min(), kmt[j - 1:j + 1, i:i + 2].min(), kmt[j - 1:j + 1, i - 1:i + 1].min())
            if (k >= 0 or not dcl) and kmt[j, i] != k:
                ht[j, i] = max(ht[j:j + 2, i:i + 2].min(), ht[j:j + 2, i - 1:i + 1].min(), ht[j - 1:j + 1, i:i + 2].min(), ht[j - 1:j + 1, i - 1:i + 1].min())
                kmt[j, i] = k
                if refresh_halo:
                    halo_fill(ht, kmt, c)
    return ht[1:-1, 1:-1], kmt[1:-1, 1:-1]
