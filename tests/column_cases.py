"""Inputs of the column-loop fixtures (tests/golden/column_*.npz: --extrapolate fill -> conservative remap of all levels ->
--dst_vgrid levels), rebuilt from exact arithmetic so that nothing but results is stored, and the recipe that chains the
REFERENCE's own functions on them: do_extrapolate and do_vertical_interp through tests/capi/extrapolate_ref_driver.c
(extrap_cases.build_driver, compiled in a temporary directory), do_scalar_conserve_interp with nz = 7 through
oracle/_ref/libconserve_ref.so (orc.cref_setup / orc.cref_apply).  Shared by tests/golden/make_golden_column.py,
tests/test_column_cpu.py and tests/test_gpu_column_sweep.py."""
import os

import numpy as np

import extrap_cases as ec
import orc

NI, NJ, NK, NREC = 72, 45, 7, 3
MISSING, STOP_CRIT = -1.0e20, 0.005
Z1 = ec.vertical_case("vert_7to9")["z1"]
DESTS = {"latlon": (40, 30), "tripolar": (36, 24)}      # (nx, ny): regular lat-lon (rectilinear search) / tripolar tile (generic)
VGRIDS = ["7to9", "same", "none"]                       # kstart = 1, kend = 7, z2[2] == z1[1] / z2 = z1: left alone / no --dst_vgrid
CASES = [(d, v) for d in DESTS for v in VGRIDS]


def z_out(vgrid):
    return None if vgrid == "none" else ec.vertical_case("vert_7to9" if vgrid == "7to9" else "vert_same")["z2"]


def nk_out(vgrid):
    return 9 if vgrid == "7to9" else NK


def source_axes():
    return ec._uniform(NI, 0.0, 5.0), ec._uniform(NJ, -90.0, 4.0)


def record(r):
    """[NK, NJ, NI]: multiples of 1/8 below 13; the land moves with the level and differs between the records"""
    k, j, i = np.meshgrid(np.arange(NK), np.arange(NJ), np.arange(NI), indexing="ij")
    data = ((7 * i + 13 * j + 5 * k + 11 * r) % 97) / 8.0
    land = ((i >= 8 + 2 * k + 5 * r) & (i < 26 + 2 * k + 5 * r) & (j >= 10 + r) & (j < 28 - k)) \
        | ((i >= 48 - 3 * r) & (i < 60) & (j >= 6 + 2 * k) & (j < 18 + 2 * k + r)) \
        | (((i >= 69 - r) | (i < 2 + k)) & (j >= 30) & (j < 41 - 2 * r)) | (j < (k + r) % 3)
    return np.where(land, MISSING, data).astype(np.float64)


def records(n=NREC):
    """n records; beyond NREC the first ones again (records four and five of the chunking tests)"""
    return np.stack([record(r % NREC) for r in range(n)])


def grids(fg, dest):
    """(source, destination) as (nx, ny, lon corners, lat corners)"""
    lo, la = fg.latlon_corners(NI, NJ)
    nx, ny = DESTS[dest]
    lo2, la2 = fg.latlon_corners(nx, ny) if dest == "latlon" else fg.tripolar_corners(nx, ny)
    return (NI, NJ, lo, la), (nx, ny, lo2, la2)


def golden_path(dest, vgrid):
    return os.path.join(ec.GOLDEN, f"column_{dest}_{vgrid}.npz")


def reference_available():
    return ec.reference_present() and orc.conserve_ref_available()


def reference_results(fg, tmp):
    """{(dest, vgrid): dict(out [NREC, nk2, ny, nx], iters [NREC, NK])} from the reference's functions alone"""
    exe = ec.build_driver(tmp)
    lon, lat = source_axes()
    filled, iters = [], []
    for r in range(NREC):
        c = dict(ni=NI, nj=NJ, nk=NK, is_cyclic=1, missing=MISSING, stop_crit=STOP_CRIT, lon=lon, lat=lat, data=record(r))
        out, it, _, _ = ec.run_ref_extrap(exe, tmp, c)
        filled.append(out)
        iters.append(it)
    res = {}
    for dest, (nx, ny) in DESTS.items():
        gin, gout = grids(fg, dest)
        x = orc.cref_setup(1, [gin], [gout])
        remapped = [orc.cref_apply(1, x, [NI], [NJ], [f.reshape(NK, -1)], None, None, None, False, MISSING, [nx], [ny], NK)[0][0]
                    .reshape(NK, ny * nx) for f in filled]
        for vgrid in VGRIDS:
            outs = remapped
            if vgrid != "none":
                outs = [ec.run_ref_vertical(exe, tmp, dict(nxy=nx * ny, z1=Z1, z2=z_out(vgrid), data=m))[0] for m in remapped]
            res[(dest, vgrid)] = dict(out=np.stack(outs).reshape(NREC, nk_out(vgrid), ny, nx), iters=np.array(iters, dtype=np.int32))
    return res
