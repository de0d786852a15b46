"""Inputs of the runoff_regrid fixtures (tests/golden/runoff_*.npz) and the recipe that runs the REFERENCE's nearest(),
create_xgrid_1dx2d_order1 and get_grid_area on them (tests/capi/runoff_ref_driver.c, compiled against the reference's sources
in a temporary directory outside the repository).  The fixtures hold their inputs, because the grids come from host
trigonometry: a test loads a fixture with `load()`, which rebuilds the grids the tool would derive (fre_nctools_amd.runoff's
numpy mirrors: element-wise IEEE arithmetic only) from the stored supergrid, depth and source axes.
Shared by tests/golden/make_golden_runoff.py, tests/test_runoff_cpu.py, tests/test_gpu_runoff.py and scripts/runoff_time.py."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
REF = os.environ.get("FRE_REFERENCE", "/root/reference")
CASES = ["tripolar_small", "latlon_regular", "one_ocean_cell", "dup_points"]
MISSING = -1.e+20
R2D = 180 / np.pi


def _pkg():
    import conftest
    return conftest.load_package()


def golden_path(name):
    return os.path.join(GOLDEN, f"runoff_{name}.npz")


def _regular_super(nx, ny, x0=0.0, x1=360.0, y0=-90.0, y1=90.0):
    x, y = np.meshgrid(x0 + (x1 - x0) * np.arange(2 * nx + 1) / (2 * nx), y0 + (y1 - y0) * np.arange(2 * ny + 1) / (2 * ny))
    return x, y


def _blobs(rng, ny, nx, nblob, size):
    """land = union of seeded elliptic blobs on the index plane (periodic in x); returns depth: 0 on land, > 0 on ocean"""
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    land = np.zeros((ny, nx), dtype=bool)
    for _ in range(nblob):
        cj, ci, a, b = rng.uniform(0, ny), rng.uniform(0, nx), rng.uniform(0.5, 1.0) * size, rng.uniform(0.3, 0.8) * size
        di = np.minimum(np.abs(i - ci), nx - np.abs(i - ci))
        land |= (di / a) ** 2 + ((j - cj) / b) ** 2 <= 1
    return np.where(land, 0.0, 100.0 + 10.0 * ((3 * i + 7 * j) % 11))


def _source(rng, masked):
    """36 x 18 lat-lon source; three time levels: two of non-negative values over 12 decades with zeros, one with negative
    values and a band of zeros; the cells in `masked` hold the missing value on every level"""
    nx, ny = 36, 18
    xt, yt = 5.0 + 10.0 * np.arange(nx), -85.0 + 10.0 * np.arange(ny)
    data = 10.0 ** rng.uniform(-6, 6, size=(3, ny, nx))
    data[rng.uniform(size=data.shape) < 0.15] = 0.0
    neg = rng.uniform(size=(ny, nx)) < 0.3
    data[2][neg] = -data[2][neg]
    data[2][:, 10:16] = 0.0
    for j, i in masked:
        data[:, j, i] = MISSING
    return xt, yt, data


def case_inputs(name):
    """-> dict: x_super, y_super [2*ny0+1, 2*nx+1] (degrees), depth [ny0, nx], xt1d_in, yt1d_in (degrees), data_in [3, 18, 36]"""
    rng = np.random.default_rng({"tripolar_small": 101, "latlon_regular": 102, "one_ocean_cell": 103, "dup_points": 104}[name])
    masked = [(3, 4), (3, 5), (9, 20), (15, 30)]
    if name == "tripolar_small":
        nx, ny = 48, 40
        lon, lat = _pkg().tripolar_corners(2 * nx, 2 * ny, xbnd=(-300.0, 60.0), ybnd=(-82.0, 90.0), lat_join=65.0)
        xs, ys = lon * R2D, lat * R2D
        depth = _blobs(rng, ny, nx, 7, 9.0)
        depth[:3, 8:30] = 0.0                       # an Antarctic shelf above the extension row
    elif name == "latlon_regular":
        nx, ny = 40, 30
        xs, ys = _regular_super(nx, ny)
        depth = _blobs(rng, ny, nx, 5, 8.0)
        depth[10:19, 5:16] = 0.0                    # a continent ...
        depth[14, 10] = 50.0                        # ... with one ocean cell inside it
    elif name == "one_ocean_cell":
        nx, ny = 11, 10                             # odd: no cell centre lies opposite the ocean cell, where r would equal r0
        xs, ys = _regular_super(nx, ny)
        depth = np.zeros((ny, nx))
        depth[6, 7] = 10.0
    elif name == "dup_points":
        nx, ny = 16, 12
        xs, ys = _regular_super(nx, ny)
        depth = np.zeros((ny, nx))
        depth[5, 4] = depth[7, 9] = depth[1, 14] = 10.0
        xs[2 * 5 + 1, 2 * 4 + 1] = xs[2 * 7 + 1, 2 * 9 + 1]      # cell (5, 4) takes the centre of cell (7, 9): two ocean indices,
        ys[2 * 5 + 1, 2 * 4 + 1] = ys[2 * 7 + 1, 2 * 9 + 1]      # one point; every query is equidistant from them
    else:
        raise KeyError(name)
    xt, yt, data = _source(rng, masked)
    return dict(x_super=xs, y_super=ys, depth=depth, xt1d_in=xt, yt1d_in=yt, data_in=data)


def grids_of(c):
    """(grid_in, grid_out) as the tool derives them (no areas): fre_nctools_amd.runoff's mirrors on a case's or fixture's inputs"""
    fg = _pkg()
    gi = fg.runoff_input_grid(c["xt1d_in"], c["yt1d_in"], c["data_in"][0], MISSING, with_area=False)
    go = fg.runoff_output_grid(c["x_super"], c["y_super"], c["depth"], 0.0, with_area=False)
    return gi, go


def load(name):
    """a fixture with its grids: (fixture dict, grid_in, grid_out), the reference's areas filled in"""
    with np.load(golden_path(name)) as z:
        fx = {k: z[k] for k in z.files}
    gi, go = grids_of(fx)
    gi["area"], go["area"] = fx["area_in"], fx["area_out"]
    return fx, gi, go


def write_driver_input(path, mode, gi, go, data_in, qindex=()):
    data_in = np.ascontiguousarray(data_in, dtype=np.float64).reshape(-1, gi["ny"], gi["nx"])
    with open(path, "wb") as f:
        np.array([mode, gi["nx"], gi["ny"], go["nx"], go["ny"], data_in.shape[0], len(qindex)], dtype=np.int32).tofile(f)
        for a in (gi["xc1d"], gi["yc1d"], gi["mask"], go["xc"], go["yc"], go["xt"], go["yt"], go["mask"], data_in):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        np.asarray(qindex, dtype=np.int32).tofile(f)


def build_driver(tmp):
    """gcc -O2 without -march: the reference's default build, no contraction.  Nothing is kept outside `tmp`."""
    tool, lib = os.path.join(REF, "tools", "runoff_regrid"), os.path.join(REF, "tools", "libfrencutils")
    inc = ["-I", os.path.join(HERE, "capi", "typecheck_shim"), "-I", lib]
    flags = ["gcc", "-O2", "-w", "-DNC_UNLIMITED=0L", "-ffunction-sections", "-fdata-sections"]
    obj, exe = os.path.join(tmp, "rr.o"), os.path.join(tmp, "runoff_ref_driver")
    subprocess.check_call(flags + ["-Dmain=runoff_regrid_main", "-c"] + inc + [os.path.join(tool, "runoff_regrid.c"), "-o", obj])
    subprocess.check_call(flags + inc + [os.path.join(HERE, "capi", "runoff_ref_driver.c"), obj] +
                          [os.path.join(lib, s) for s in ("create_xgrid.c", "mosaic_util.c", "mpp.c", "mpp_domain.c")] +
                          ["-Wl,--gc-sections", "-lm", "-o", exe])
    return exe


def run_ref(exe, tmp, gi, go, data_in):
    """mode 0 -> dict of the reference's outputs"""
    inp, out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out")
    os.makedirs(out, exist_ok=True)
    write_driver_input(inp, 0, gi, go, data_in)
    subprocess.run([exe, inp, out], check=True, capture_output=True, timeout=900)
    rd = lambda n, dt: np.fromfile(os.path.join(out, n + ".bin"), dtype=dt)
    ny, nx, nt = go["ny"], go["nx"], np.asarray(data_in).reshape(-1, gi["ny"], gi["nx"]).shape[0]
    r = {k: rd(k, np.int32) for k in ("i_in", "j_in", "i_out", "j_out")}
    r.update(imap=rd("imap", np.int32).reshape(ny, nx), jmap=rd("jmap", np.int32).reshape(ny, nx), xgrid_area=rd("xgrid_area", np.float64),
             area_in=rd("area_in", np.float64).reshape(gi["ny"], gi["nx"]), area_out=rd("area_out", np.float64).reshape(ny, nx),
             data_out=rd("data_out", np.float64).reshape(nt, ny, nx), totals=rd("totals", np.float64).reshape(nt, 2))
    assert r["i_in"].size == int(open(os.path.join(out, "nxgrid.txt")).read())
    return r


def run_ref_nearest(exe, tmp, gi, go, qindex):
    """mode 1 -> (iq, jq, seconds for the len(qindex) calls of nearest())"""
    inp, out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out")
    os.makedirs(out, exist_ok=True)
    write_driver_input(inp, 1, gi, go, np.zeros((0, gi["ny"], gi["nx"])), qindex)
    subprocess.run([exe, inp, out], check=True, capture_output=True, timeout=3000)
    return (np.fromfile(os.path.join(out, "iq.bin"), dtype=np.int32), np.fromfile(os.path.join(out, "jq.bin"), dtype=np.int32),
            float(open(os.path.join(out, "seconds.txt")).read()))


def process_data_numpy(fx, go, gi, data_in, order=None):
    """process_data's three loops (:626-653) restated sequentially in numpy scalars, on a fixture's list and maps.
    order: a permutation of the land cells to move in, instead of the reference's ascending one."""
    nx = go["nx"]
    out = np.zeros(go["nx"] * go["ny"])
    din = np.asarray(data_in, dtype=np.float64).reshape(-1)
    for l in range(fx["i_in"].size):
        out[fx["j_out"][l] * nx + fx["i_out"][l]] += din[fx["j_in"][l] * gi["nx"] + fx["i_in"][l]] * fx["xgrid_area"][l]
    mask, imap, jmap = go["mask"].reshape(-1), fx["imap"].reshape(-1), fx["jmap"].reshape(-1)
    for l in (range(out.size) if order is None else order):
        if out[l] > 0 and mask[l] == 0:
            out[jmap[l] * nx + imap[l]] += out[l]
            out[l] = 0
    return (out / np.asarray(go["area"]).reshape(-1)).reshape(go["ny"], nx)


def thinned_mask(nocean, nx=40, ny=30, seed=7):
    """a 40 x 30 mask with exactly `nocean` ocean cells, chosen by a seeded permutation"""
    m = np.zeros(nx * ny)
    m[np.random.default_rng(seed).permutation(nx * ny)[:nocean]] = 1.0
    return m.reshape(ny, nx)


def hostcheck_exe():
    """tests/hostcheck/runoff_check.cpp built for the host (rebuilt when a source is newer)"""
    src = os.path.join(HERE, "hostcheck", "runoff_check.cpp")
    exe = os.path.join(HERE, "hostcheck", "_build", "runoff_check")
    inc = os.path.join(ROOT, "fre-nctools_amd", "csrc")
    srcs = [src] + [os.path.join(inc, h) for h in ("runoff.h", "sincos_glibc.h", "sincos_table.h")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-fno-builtin", "-std=c++17", "-ffp-contract=off", "-I", inc, src, "-o", exe, "-lm"])
    return exe


def hostcheck_nearest(tmpdir, mask, lon, lat):
    """the host build's brute-force nearest() and conversion: (imap, jmap [nlat, nlon], x, y, z [nlat, nlon])"""
    mask = np.ascontiguousarray(mask, dtype=np.float64)
    nlat, nlon = mask.shape
    inp, out = os.path.join(str(tmpdir), "hc_in.bin"), os.path.join(str(tmpdir), "hc_out.bin")
    with open(inp, "wb") as f:
        np.array([nlon, nlat], dtype=np.int32).tofile(f)
        for a in (mask, lon, lat):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    subprocess.run([hostcheck_exe(), "nearest", inp, out], check=True, timeout=600)
    n = nlon * nlat
    with open(out, "rb") as f:
        ij = np.fromfile(f, dtype=np.int32, count=2 * n)
        xyz = np.fromfile(f, dtype=np.float64, count=3 * n)
    return (ij[:n].reshape(nlat, nlon), ij[n:].reshape(nlat, nlon)) + tuple(xyz.reshape(3, nlat, nlon))
