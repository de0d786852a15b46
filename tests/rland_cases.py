"""Inputs of the remap_land nearest-search fixtures (tests/golden/rland_*.npz) and the recipe that runs the REFERENCE's
full_search_nearest and search_nearest_sface on them (tests/capi/rland_ref_driver.c, compiled against the reference's sources
in a temporary directory outside the repository).  The fixtures hold their inputs, because the points come from host
trigonometry; a test loads a fixture with `load()` and never rebuilds a point.
Shared by tests/golden/make_golden_rland.py, tests/test_rland_cpu.py, tests/test_gpu_rland.py and scripts/rland_time.py."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
REF = os.environ.get("FRE_REFERENCE", "/root/reference")
CASES = ["cube_small", "latlon_ties", "dup_points", "frames", "one_source_point", "antipode_first", "beyond_pole_source", "beyond_pole_query"]
INPUTS = ("lon_src", "lat_src", "mask_src", "lon_dst", "lat_dst", "mask_dst", "iface_dst")
OUTPUTS = ("idx_map", "face_map", "idx_map_sf")


def golden_path(name):
    return os.path.join(GOLDEN, f"rland_{name}.npz")


def load(name):
    with np.load(golden_path(name)) as z:
        return {k: z[k] for k in z.files}


def cube_centres(n):
    """cell centres of an equiangular gnomonic cubed sphere, (lon, lat) [6, n * n] in radians, lon in [0, 2 pi)"""
    a = (-0.25 + (np.arange(n) + 0.5) / (2 * n)) * np.pi
    u, v = np.meshgrid(np.tan(a), np.tan(a))
    one = np.ones_like(u)
    faces = [(one, u, v), (-u, one, v), (-one, -u, v), (u, -one, v), (-v, u, one), (v, u, -one)]
    lon, lat = np.empty((6, n * n)), np.empty((6, n * n))
    for f, (x, y, z) in enumerate(faces):
        lon[f] = np.mod(np.arctan2(y, x), 2 * np.pi).ravel()
        lat[f] = np.arctan2(z, np.hypot(x, y)).ravel()
    return lon, lat


def sphere_points(n, seed=0):
    """n points spread over the whole sphere (a golden-angle spiral), lon in [0, 2 pi)"""
    k = np.arange(n) + 0.5
    return np.mod(k * 2.399963229728653 + seed, 2 * np.pi), np.arcsin(1 - 2 * k / n)


def _cube_small():
    rng = np.random.default_rng(201)
    lon_src, lat_src = cube_centres(8)
    lon12, lat12 = cube_centres(12)
    mask_src = (rng.uniform(size=lon_src.shape) < 0.4).astype(np.int32)
    mask_dst = (rng.uniform(size=144) < 0.64).astype(np.int32)
    return dict(lon_src=lon_src, lat_src=lat_src, mask_src=mask_src, lon_dst=lon12[2], lat_dst=lat12[2], mask_dst=mask_dst, iface_dst=2)


def case_inputs(name, antipodes=None):
    """-> dict of INPUTS.  antipodes: for the last two cases, (lon, lat) of a point and (lon, lat) of a query at its computed
    antipode for which the reference's d is NaN, or None if the search found none (make_golden_rland.py)."""
    if name == "cube_small":
        return _cube_small()
    if name == "frames":                                   # the same points, the destination in a -300 .. 60 degree frame
        c = _cube_small()
        c["lon_dst"] = np.where(c["lon_dst"] > np.pi / 3, c["lon_dst"] - 2 * np.pi, c["lon_dst"])
        return c
    if name == "latlon_ties":                              # 24 x 12 centres, the southern six rows face 0, the northern face 1
        d = np.pi / 180
        lon, lat = np.meshgrid((np.arange(24) + 0.5) * 15 * d, (-82.5 + 15 * np.arange(12)) * d)
        mask = np.ones((12, 24), dtype=np.int32)
        mask[3, 5:9] = 0
        mask[8, 10:13] = 0
        qlon = np.array([0.3, 1.0, 30 * d, 45 * d, 45 * d, 200 * d, 97.5 * d, 3.0, 5.0, 180 * d])
        qlat = np.array([np.pi / 2, -np.pi / 2, 37.5 * d, 30 * d, 0.0, 0.0, 7.5 * d, 0.4, -1.2, 67.5 * d])
        return dict(lon_src=lon.reshape(2, 144), lat_src=lat.reshape(2, 144), mask_src=mask.reshape(2, 144), lon_dst=qlon, lat_dst=qlat,
                    mask_dst=np.array([1, 1, 1, 1, 1, 1, 1, 0, 1, 1], dtype=np.int32), iface_dst=1)
    if name == "dup_points":                               # two flat indices on one point: within face 1, and across faces 0 and 4
        c = _cube_small()
        for (fa, ia), (fb, ib) in (((1, 10), (1, 40)), ((4, 5), (0, 20))):
            c["lon_src"][fa, ia], c["lat_src"][fa, ia] = c["lon_src"][fb, ib], c["lat_src"][fb, ib]
            c["mask_src"][fa, ia] = c["mask_src"][fb, ib] = 1
        extra_lon = np.array([c["lon_src"][1, 40], c["lon_src"][0, 20], c["lon_src"][1, 40] + 1e-3, c["lon_src"][0, 20] - 1e-3])
        extra_lat = np.array([c["lat_src"][1, 40], c["lat_src"][0, 20], c["lat_src"][1, 40] + 1e-3, c["lat_src"][0, 20] + 1e-3])
        c["lon_dst"], c["lat_dst"] = np.concatenate([c["lon_dst"], extra_lon]), np.concatenate([c["lat_dst"], extra_lat])
        c["mask_dst"] = np.concatenate([c["mask_dst"], np.ones(4, dtype=np.int32)])
        c["iface_dst"] = 1
        return c
    if name in ("one_source_point", "antipode_first"):
        (plon, plat), (alon, alat) = antipodes if antipodes is not None else ((1.1, 0.35), (1.1 + np.pi, -0.35))
        lon_src, lat_src = sphere_points(100, 0.5)
        lon_src, lat_src = lon_src.reshape(2, 50), lat_src.reshape(2, 50)
        mask_src = np.zeros((2, 50), dtype=np.int32)
        if name == "one_source_point":                     # one unmasked point, queries over the whole sphere and at its antipode
            lon_src[1, 7], lat_src[1, 7], mask_src[1, 7] = plon, plat, 1
        else:                                              # the first unmasked point at the query's antipode, 30 more points behind it
            lon_src[0, 3], lat_src[0, 3], mask_src[0, 3] = plon, plat, 1
            mask_src[0, 20:], mask_src[1, :10] = 1, 1
        qlon, qlat = sphere_points(61, 0.1)
        qlon, qlat = np.concatenate([qlon, [alon, plon]]), np.concatenate([qlat, [alat, plat]])
        return dict(lon_src=lon_src, lat_src=lat_src, mask_src=mask_src, lon_dst=qlon, lat_dst=qlat,
                    mask_dst=np.ones(qlon.size, dtype=np.int32), iface_dst=1 if name == "one_source_point" else 0)
    if name in ("beyond_pole_source", "beyond_pole_query"):
        # Latitudes just beyond pi/2, where cos(lat) < 0 and the two terms of the haversine cancel: the reference's h can come out
        # negative and its d NaN for a point that is nowhere near the antipode.  Query k at (lon, phi), phi in (1.575, 1.6).
        # _source: flat index 2k at (lon, phi - delta), also beyond the pole, and 2k + 1 at (lon + pi, pi - phi): the query's own
        # point on the sphere, within range.  _query: every source point within range, 2k and 2k + 1 at (lon + pi, pi - phi -+ delta).
        rng = np.random.default_rng(203)
        nq = 20
        phi, lon = rng.uniform(1.575, 1.6, nq), rng.uniform(0.0, 2.5, nq)
        delta = 10.0 ** rng.uniform(-11, -9.5, nq)
        lon_src, lat_src = np.empty(2 * nq), np.empty(2 * nq)
        if name == "beyond_pole_source":
            lon_src[0::2], lat_src[0::2] = lon, phi - delta
            lon_src[1::2], lat_src[1::2] = lon + np.pi, np.pi - phi
        else:
            lon_src[0::2], lat_src[0::2] = lon + np.pi, np.pi - phi - delta
            lon_src[1::2], lat_src[1::2] = lon + np.pi, np.pi - phi + delta
        glon, glat = sphere_points(2 * nq, 0.3)                              # a second face of ordinary points
        qlon, qlat = sphere_points(5, 0.9)                                   # and five ordinary queries
        return dict(lon_src=np.stack([lon_src, glon]), lat_src=np.stack([lat_src, glat]), mask_src=np.ones((2, 2 * nq), dtype=np.int32),
                    lon_dst=np.concatenate([lon, qlon]), lat_dst=np.concatenate([phi, qlat]), mask_dst=np.ones(nq + 5, dtype=np.int32), iface_dst=1)
    raise KeyError(name)


def write_driver_input(path, mode, c):
    lon_src = np.ascontiguousarray(c["lon_src"], dtype=np.float64)
    nface, npts = lon_src.shape if lon_src.ndim == 2 else (1, lon_src.size)
    with open(path, "wb") as f:
        np.array([mode, nface, npts, np.asarray(c["lon_dst"]).size, int(c["iface_dst"]), 0], dtype=np.int32).tofile(f)
        for k, dt in (("lon_src", np.float64), ("lat_src", np.float64), ("mask_src", np.int32), ("lon_dst", np.float64),
                      ("lat_dst", np.float64), ("mask_dst", np.int32)):
            np.ascontiguousarray(c[k], dtype=dt).tofile(f)


def build_driver(tmp):
    """gcc -O2 without -march: the reference's default build, no contraction.  Nothing is kept outside `tmp`."""
    tool, lib = os.path.join(REF, "tools", "remap_land"), os.path.join(REF, "tools", "libfrencutils")
    inc = ["-I", os.path.join(HERE, "capi", "typecheck_shim"), "-I", lib]
    flags = ["gcc", "-O2", "-w", "-DNC_UNLIMITED=0L", "-DNC_FILL_INT=(-2147483647)", "-DNC_FILL_DOUBLE=(9.9692099683868690e+36)",
             "-ffunction-sections", "-fdata-sections"]
    obj, exe = os.path.join(tmp, "rl.o"), os.path.join(tmp, "rland_ref_driver")
    subprocess.check_call(flags + ["-Dmain=remap_land_main", "-c"] + inc + [os.path.join(tool, "remap_land.c"), "-o", obj])
    subprocess.check_call(flags + inc + [os.path.join(HERE, "capi", "rland_ref_driver.c"), obj] +
                          [os.path.join(lib, s) for s in ("mosaic_util.c", "mpp.c", "mpp_domain.c")] + ["-Wl,--gc-sections", "-lm", "-o", exe])
    return exe


def run_ref(exe, tmp, c, mode=0):
    """-> dict of OUTPUTS (mode 0), or idx_map, face_map, seconds (mode 1)"""
    inp, out = os.path.join(tmp, "rl_in.bin"), os.path.join(tmp, "rl_out")
    os.makedirs(out, exist_ok=True)
    write_driver_input(inp, mode, c)
    subprocess.run([exe, inp, out], check=True, capture_output=True, timeout=3000)
    r = {k: np.fromfile(os.path.join(out, k + ".bin"), dtype=np.int32) for k in (OUTPUTS if mode == 0 else OUTPUTS[:2])}
    if mode == 1:
        r["seconds"] = float(open(os.path.join(out, "seconds.txt")).read())
    return r


def run_ref_distance(exe, tmp, lon1, lat1, lon2, lat2):
    """the reference's great_circle_distance of the pairs (point 1, point 2)"""
    n = np.asarray(lon1).size
    c = dict(lon_src=np.asarray(lon2).reshape(1, n), lat_src=np.asarray(lat2).reshape(1, n), mask_src=np.ones(n), lon_dst=lon1, lat_dst=lat1,
             mask_dst=np.ones(n), iface_dst=0)
    inp, out = os.path.join(tmp, "rl_d_in.bin"), os.path.join(tmp, "rl_d_out")
    os.makedirs(out, exist_ok=True)
    write_driver_input(inp, 2, c)
    subprocess.run([exe, inp, out], check=True, capture_output=True, timeout=600)
    return np.fromfile(os.path.join(out, "d.bin"), dtype=np.float64)


def hostcheck_exe():
    """tests/hostcheck/rland_check.cpp built for the host (rebuilt when a source is newer)"""
    src = os.path.join(HERE, "hostcheck", "rland_check.cpp")
    exe = os.path.join(HERE, "hostcheck", "_build", "rland_check")
    inc = os.path.join(ROOT, "fre-nctools_amd", "csrc")
    srcs = [src] + [os.path.join(inc, h) for h in ("rland.h", "runoff.h", "sincos_glibc.h", "sincos_table.h")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-fno-builtin", "-std=c++17", "-ffp-contract=off", "-I", inc, src, "-o", exe, "-lm"])
    return exe


def hostcheck(tmpdir, c):
    """the host build on a case's inputs: dict of OUTPUTS, and fallback, several (the queries that took the reference's loop,
    and those decided among several survivors)"""
    inp, out = os.path.join(str(tmpdir), "rlhc_in.bin"), os.path.join(str(tmpdir), "rlhc_out.bin")
    write_driver_input(inp, 0, c)
    subprocess.run([hostcheck_exe(), inp, out], check=True, timeout=600)
    nd = np.asarray(c["lon_dst"]).size
    with open(out, "rb") as f:
        maps = np.fromfile(f, dtype=np.int32, count=3 * nd).reshape(3, nd)
        counts = np.fromfile(f, dtype=np.int64, count=2)
    return dict(idx_map=maps[0], face_map=maps[1], idx_map_sf=maps[2], fallback=int(counts[0]), several=int(counts[1]))


def thinned_source(nsrc, n=1200, seed=11):
    """`n` points (1200) over the sphere in 3 faces of n / 3 with exactly `nsrc` unmasked, chosen by a seeded permutation"""
    lon, lat = sphere_points(n, 0.25)
    mask = np.zeros(n, dtype=np.int32)
    mask[np.random.default_rng(seed).permutation(n)[:nsrc]] = 1
    return lon.reshape(3, n // 3), lat.reshape(3, n // 3), mask.reshape(3, n // 3)
