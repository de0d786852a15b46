"""Inputs of the river_regrid fixtures (tests/golden/river_*.npz) and the recipe that runs the REFERENCE's calc_max_subA,
calc_tocell, calc_river_data, sort_basin and check_river_data on them (tests/capi/river_ref_driver.c, compiled around the
reference's river_regrid.c in a temporary directory outside the repository).  Land and subA are seeded analytic functions; the
cube tiles come from the reference's own generator, so the fixtures hold their inputs and a test loads a fixture with `load()`
and never rebuilds a grid.
Shared by tests/golden/make_golden_river.py, tests/test_river_cpu.py, tests/test_gpu_river.py and scripts/river_time.py."""
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
CASES = ["latlon_shift", "latlon_aligned", "regional", "torus_rect", "cube_c12", "cube_c12_gca", "cube_c10_odd", "cube_c8_continent",
         "latlon_continent", "cutoff_low", "missing_rows", "cube_c24"]
MISSING = np.array([-9999., -9999., -9999., -9999., -9999., -9999.])      # subA, tocell, travel, basin, cellarea, celllength
SCALARS = ("opcode", "gca", "suba_cutoff")
INPUTS = ("src_xt", "src_yt", "src_xb_r", "src_yb_r", "src_subA", "missing", "xb_r", "yb_r", "xt", "yt", "landfrac_raw", "landfrac") + SCALARS
OUTPUTS_D = ("area", "xt_halo", "yt_halo", "max_suba", "subA", "cellarea", "celllength")
OUTPUTS_I = ("tocell", "travel", "basin", "basin_presort", "last_point")
COUNTS = ("maxtravel", "maxbasin", "coast_full_land", "sink")
LAND_THRESH, MIN_FRAC = 1.e-4, 0.1
DI = np.array([1, 1, 0, -1, -1, -1, 0, 1])        # calc_river_data :1003
DJ = np.array([0, -1, -1, -1, 0, 1, 1, 1])


def package():
    """the package under the name the tests load it by (tests/conftest.py)"""
    if "fre_nctools_amd" not in sys.modules:
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.load_package()
    return sys.modules["fre_nctools_amd"]


def golden_path(name):
    return os.path.join(GOLDEN, f"river_{name}.npz")


def load(name):
    with np.load(golden_path(name)) as z:
        return {k: z[k] for k in z.files}


def source_grid(nx, ny):
    """the axes of a global nx x ny river network file, in degrees"""
    return (np.arange(nx) + 0.5) * (360.0 / nx), -90 + (np.arange(ny) + 0.5) * (180.0 / ny)


def _wave(lon_deg, lat_deg, seed, nterms=5):
    """a smooth seeded function of position in about [-1, 1]"""
    rng = np.random.default_rng(seed)
    lon, lat = np.asarray(lon_deg) * D2R, np.asarray(lat_deg) * D2R
    x, y, z = np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)
    f = np.zeros(np.broadcast(lon, lat).shape)
    for _ in range(nterms):
        k = rng.normal(size=3) * 2.5
        f += np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 2 * np.pi))
    return f / np.sqrt(nterms)


def source_suba(xt, yt, seed, scale):
    """subA of the network: positive, around `scale`, missing over the network's own ocean"""
    lon, lat = np.meshgrid(xt, yt)
    rng = np.random.default_rng(seed + 1000)
    v = scale * (1.2 + _wave(lon, lat, seed + 1) + 0.3 * rng.uniform(size=lon.shape))
    v = np.maximum(v, scale * 0.01)
    v[_wave(lon, lat, seed + 2) < -0.55] = MISSING[0]
    return v


def blob_land(lon_deg, lat_deg, seed, bias=0.1):
    """land fractions in quarters (equal values make equal cell areas along a latitude: ties among the outlets)"""
    f = np.clip((_wave(lon_deg, lat_deg, seed) + bias) / 0.5, 0.0, 1.0)
    return np.round(f * 4) / 4


def continent_land(lon_deg, lat_deg, cap_lon=200.0, cap_lat=-20.0, cap=25.0):
    """land everywhere outside a cap of `cap` degrees"""
    lon, lat = np.asarray(lon_deg) * D2R, np.asarray(lat_deg) * D2R
    c = np.sin(lat) * np.sin(cap_lat * D2R) + np.cos(lat) * np.cos(cap_lat * D2R) * np.cos(lon - cap_lon * D2R)
    return np.where(c > np.cos(cap * D2R), 0.0, 1.0)


def latlon_tile(nx, ny, west=0.0, east=None, south=-90.0, north=90.0):
    """one tile: corners and centres in degrees, [1, ny+1, nx+1] and [1, ny, nx]"""
    east = west + 360.0 if east is None else east
    xb1, yb1 = west + np.arange(nx + 1) * ((east - west) / nx), south + np.arange(ny + 1) * ((north - south) / ny)
    xb, yb = np.meshgrid(xb1, yb1)
    xt, yt = np.meshgrid(0.5 * (xb1[:-1] + xb1[1:]), 0.5 * (yb1[:-1] + yb1[1:]))
    return xb[None], yb[None], xt[None], yt[None]


def cube_tiles(n):
    """the reference generator's C<n> supergrid as get_mosaic_grid reads it (:473-478): corners and centres in degrees"""
    import gridutil
    x, y = gridutil.ref_gnomonic_corners(n, supergrid=True)
    return (np.ascontiguousarray(x[:, ::2, ::2]), np.ascontiguousarray(y[:, ::2, ::2]),
            np.ascontiguousarray(x[:, 1::2, 1::2]), np.ascontiguousarray(y[:, 1::2, 1::2]))


def _assemble(src, seed, scale, grid, opcode, land, gca=0, suba_cutoff=1.e12, fg=None):
    fg = fg or package()
    xt_s, yt_s = source_grid(*src)
    sg = fg.river_source_grid(xt_s, yt_s)
    xb, yb, xt, yt = grid
    raw = land(xt, yt)
    return dict(src_xt=xt_s, src_yt=yt_s, src_xb_r=sg["xb_r"], src_yb_r=sg["yb_r"], src_subA=source_suba(xt_s, yt_s, seed, scale), missing=MISSING.copy(),
                xb_r=xb * D2R, yb_r=yb * D2R, xt=xt, yt=yt, landfrac_raw=raw, landfrac=fg.river_land_frac(raw, LAND_THRESH, MIN_FRAC),
                opcode=np.array(opcode), gca=np.array(gca), suba_cutoff=np.array(float(suba_cutoff)))


def case_inputs(name):
    """-> dict of INPUTS.  Tile arrays are [ntiles, ...]; xt, yt are the interior [ntiles, ny, nx] in degrees."""
    blob = lambda seed, bias=0.1: (lambda lon, lat: blob_land(lon, lat, seed, bias))
    if name == "latlon_shift":
        return _assemble((72, 36), 11, 4e11, latlon_tile(48, 24, west=-177.5), 1, blob(12))
    if name == "latlon_aligned":
        return _assemble((40, 20), 21, 4e11, latlon_tile(40, 20, west=0.0), 1, blob(22))
    if name == "regional":
        return _assemble((72, 36), 31, 4e11, latlon_tile(20, 12, west=10.0, east=130.0, south=-40.0, north=50.0), 0, blob(32))
    if name == "torus_rect":
        return _assemble((72, 36), 41, 4e11, latlon_tile(48, 24, west=0.0), 3, blob(42))
    if name in ("cube_c12", "cube_c12_gca", "cutoff_low"):
        return _assemble((72, 36), 51, 4e12, cube_tiles(12), 4, blob(52), gca=int(name == "cube_c12_gca"),
                         suba_cutoff=0.0 if name == "cutoff_low" else 1.e12)
    if name == "cube_c10_odd":
        return _assemble((97, 45), 61, 4e12, cube_tiles(10), 4, blob(62, 0.6))
    if name == "cube_c8_continent":
        return _assemble((72, 36), 71, 4e11, cube_tiles(8), 4, continent_land)
    if name == "latlon_continent":
        return _assemble((72, 36), 81, 4e11, latlon_tile(48, 24, west=0.0), 1, continent_land)
    if name == "missing_rows":
        c = _assemble((72, 36), 11, 4e11, latlon_tile(48, 24, west=-177.5), 1, blob(12))
        c["src_subA"][::3, :] = MISSING[0]
        c["src_subA"][:, 30:48] = MISSING[0]              # 150 .. 240 degrees east
        return c
    if name == "cube_c24":
        return _assemble((144, 72), 91, 4e12, cube_tiles(24), 4, blob(92))
    raise KeyError(name)


def generated_case(n=48, src=(360, 180), seed=101, with_area=True):
    """a cube case with no fixture (pruned against literal replay; scripts/river_time.py), on the package's own gnomonic grid;
    the areas come from get_grid_area on the device"""
    fg = package()
    lonc, latc, lont, latt = fg.gnomonic_ed_grid(n)
    r2d = 180 / np.pi
    c = _assemble(src, seed, 4e12, (lonc * r2d, latc * r2d, lont * r2d, latt * r2d), 4, lambda lon, lat: blob_land(lon, lat, seed + 1, 0.3))
    c["xb_r"], c["yb_r"] = lonc, latc
    if with_area:
        c["area"] = np.stack([fg.get_grid_area(n, n, lonc[t], latc[t]).reshape(n, n) for t in range(6)])
    return c


def funnel_case():
    """A regional grid, all land but one ocean cell, with subA rising towards that cell from everywhere: every river ends in a
    cell next to the ocean (travel 1) and none in a travel-0 cell, so the first sweep of calc_river_data assigns nothing, the
    loop stops, and check_river_data finds river points without travel: one of the reference's fatal errors."""
    c = _assemble((72, 36), 31, 1.0, latlon_tile(20, 12, west=10.0, east=130.0, south=-40.0, north=50.0), 0, lambda lon, lat: np.ones_like(lon))
    lon, lat = np.meshgrid(c["src_xt"], c["src_yt"])
    c["src_subA"] = 1.e6 - 1.e3 * np.maximum(np.abs(lon - 73.0), np.abs(lat - 8.75))
    c["landfrac_raw"][0, 6, 10] = 0.0                     # the cell around 73 E, 8.75 N
    c["landfrac"] = c["landfrac_raw"].copy()
    return c


def write_driver_input(path, c):
    ntiles, ny, nx = c["xt"].shape
    ny_in, nx_in = c["src_subA"].shape
    with open(path, "wb") as f:
        np.array([nx_in, ny_in, ntiles, nx, ny, int(c["opcode"]), int(c["gca"])], dtype=np.int32).tofile(f)
        np.concatenate([[float(c["suba_cutoff"])], c["missing"]]).astype(np.float64).tofile(f)
        for k in ("src_xb_r", "src_yb_r", "src_subA"):
            np.ascontiguousarray(c[k], dtype=np.float64).tofile(f)
        for n in range(ntiles):
            for k in ("xb_r", "yb_r"):
                np.ascontiguousarray(c[k][n], dtype=np.float64).tofile(f)
            for k in ("xt", "yt"):
                full = np.zeros((ny + 2, nx + 2))
                full[1:-1, 1:-1] = c[k][n]
                full.tofile(f)
            np.ascontiguousarray(c["landfrac"][n], dtype=np.float64).tofile(f)


def build_driver(tmp):
    """gcc -O2 without -march: the reference's default build, no contraction.  Nothing is kept outside `tmp`."""
    lib = os.path.join(REF, "tools", "libfrencutils")
    river_c = os.path.join(REF, "tools", "river_regrid", "river_regrid.c")
    inc = ["-I", os.path.join(HERE, "capi", "typecheck_shim"), "-I", lib]
    flags = ["gcc", "-O2", "-w", "-DNC_UNLIMITED=0L", "-ffunction-sections", "-fdata-sections"]
    obj, exe = os.path.join(tmp, "rv.o"), os.path.join(tmp, "river_ref_driver")
    subprocess.check_call(flags + inc + [f'-DRIVER_C="{river_c}"', "-c", os.path.join(HERE, "capi", "river_ref_driver.c"), "-o", obj])
    subprocess.check_call(flags + inc + [obj] + [os.path.join(lib, s) for s in ("create_xgrid.c", "mosaic_util.c", "mpp.c", "mpp_domain.c")] +
                          ["-Wl,--gc-sections", "-lm", "-o", exe])
    return exe


def run_ref(exe, tmp, c):
    """-> dict of OUTPUTS_D, OUTPUTS_I, COUNTS and seconds [5].  A fatal error of the reference raises CalledProcessError."""
    inp, out = os.path.join(tmp, "rv_in.bin"), os.path.join(tmp, "rv_out")
    os.makedirs(out, exist_ok=True)
    write_driver_input(inp, c)
    p = subprocess.run([exe, inp, out], check=True, capture_output=True, text=True, timeout=3000)
    ntiles, ny, nx = c["xt"].shape
    shapes = dict(area=(ntiles, ny, nx), xt_halo=(ntiles, ny + 2, nx + 2), yt_halo=(ntiles, ny + 2, nx + 2), max_suba=(ntiles, ny + 2, nx + 2))
    files = dict(xt_halo="xt", yt_halo="yt")
    r = {}
    for k in OUTPUTS_D:
        r[k] = np.fromfile(os.path.join(out, files.get(k, k) + ".bin"), dtype=np.float64).reshape(shapes.get(k, (ntiles, ny, nx)))
    for k in OUTPUTS_I:
        r[k] = np.fromfile(os.path.join(out, k + ".bin"), dtype=np.int32).reshape(ntiles, ny, nx)
    m = re.search(r"maximum travel is (-?\d+) and maximum basin is (-?\d+)", p.stdout)
    r["maxtravel"], r["maxbasin"] = np.array(int(m.group(1))), np.array(int(m.group(2)))
    m = re.search(r"there are (\d+) coast points", p.stdout)
    r["coast_full_land"] = np.array(int(m.group(1)) if m else 0)
    m = re.search(r"there are (\d+) sink points", p.stdout)
    r["sink"] = np.array(int(m.group(1)) if m else 0)
    r["seconds"] = np.array([float(v) for v in open(os.path.join(out, "seconds.txt")).read().split()])
    return r


def features(c, r):
    """what a case is there for, from the reference's outputs: flows into halo cells, outlets in ties, full-land cells above
    and at or below the cutoff, full-land cells whose accepted set is empty"""
    ntiles, ny, nx = c["xt"].shape
    toc = r["tocell"]
    flows = toc > 0
    d = np.zeros_like(toc)
    d[flows] = np.round(np.log2(toc[flows])).astype(int)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    jd, idst = jj[None] + DJ[d], ii[None] + DI[d]
    halo = flows & ((jd < 0) | (jd >= ny) | (idst < 0) | (idst >= nx))
    out_sub = r["subA"][r["last_point"] != 0]
    vals, cnt = np.unique(out_sub, return_counts=True)
    full = c["landfrac"] == 1
    ms = r["max_suba"][:, 1:-1, 1:-1]
    return dict(halo_flows=int(halo.sum()), tie_outlets=int(cnt[cnt > 1].sum()), above=int((full & (ms > float(c["suba_cutoff"]))).sum()),
                below=int((full & (ms <= float(c["suba_cutoff"]))).sum()), empty=int((full & (ms == c["missing"][0])).sum()), full=int(full.sum()))


def tiles_of(fx):
    """RiverRegrid's arguments from a fixture (or case_inputs with area added): (source, tiles, opcode, suba_cutoff)"""
    source = dict(xb_r=fx["src_xb_r"], yb_r=fx["src_yb_r"], subA=fx["src_subA"], missing=fx["missing"])
    tiles = [dict(xb_r=fx["xb_r"][n], yb_r=fx["yb_r"][n], xt=fx["xt"][n], yt=fx["yt"][n], area=fx["area"][n], landfrac=fx["landfrac"][n])
             for n in range(fx["xt"].shape[0])]
    return source, tiles, int(fx["opcode"]), float(fx["suba_cutoff"])


def hostcheck_exe():
    """tests/hostcheck/river_check.cpp built for the host (rebuilt when a source is newer)"""
    src = os.path.join(HERE, "hostcheck", "river_check.cpp")
    exe = os.path.join(HERE, "hostcheck", "_build", "river_check")
    inc = os.path.join(ROOT, "fre-nctools_amd", "csrc")
    srcs = [src] + [os.path.join(inc, h) for h in ("river.h", "sincos_glibc.h", "sincos_table.h")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-fno-builtin", "-std=c++17", "-ffp-contract=off", "-I", inc, src, "-o", exe, "-lm"])
    return exe


def hostcheck(tmpdir, fx):
    """the host build of csrc/river.h on a fixture's inputs: dict literal, pruned (the interior of max subA [ntiles, ny, nx]) and
    visited_literal, visited_pruned (source cells)"""
    inp, out = os.path.join(str(tmpdir), "rvhc_in.bin"), os.path.join(str(tmpdir), "rvhc_out.bin")
    write_driver_input(inp, fx)
    with open(inp, "ab") as f:
        np.ascontiguousarray(fx["area"], dtype=np.float64).tofile(f)
    subprocess.run([hostcheck_exe(), inp, out], check=True, timeout=600)
    shape = fx["xt"].shape
    n = int(np.prod(shape))
    with open(out, "rb") as f:
        lit = np.fromfile(f, dtype=np.float64, count=n).reshape(shape)
        pru = np.fromfile(f, dtype=np.float64, count=n).reshape(shape)
        visited = np.fromfile(f, dtype=np.int64, count=2)
    return dict(literal=lit, pruned=pru, visited_literal=int(visited[0]), visited_pruned=int(visited[1]))
