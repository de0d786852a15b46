#!/usr/bin/env python3
"""Generate tests/golden/rland_*.npz from the REFERENCE's full_search_nearest and search_nearest_sface
(tools/remap_land/remap_land.c:2520, :2569) with its great_circle_distance (tools/libfrencutils/mosaic_util.c:747).

Run where the reference's sources are present (FRE_REFERENCE, default /root/reference):
    python tests/golden/make_golden_rland.py
tests/capi/rland_ref_driver.c is compiled with the reference's remap_land.c (-Dmain=..., function sections, --gc-sections: none
of its netCDF-bound functions is kept), mosaic_util.c, mpp.c and mpp_domain.c in a temporary directory outside the repository;
nothing compiled is kept.  Each file holds (data only):
  inputs    lon_src, lat_src [nface, npts] (radians), mask_src, lon_dst, lat_dst, mask_dst [npts_dst], iface_dst
  outputs   idx_map, face_map (the all-faces search), idx_map_sf (the same-face search for iface_dst with the same mask)
  libc      the C library of the host that made the file: the distances carry its sin/cos/asin bits
  nan_first 1 if the antipodal query's d to the first unmasked point is NaN in the reference (one_source_point, antipode_first)
The last two cases need a point and a query at its computed antipode for which the reference's d is NaN: up to 10^4 seeded
placements are tried through the reference's own function."""
import os
import platform
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rland_cases as rc  # noqa: E402


def find_nan_antipode(exe, tmp):
    rng = np.random.default_rng(202)
    plon, plat = rng.uniform(0, np.pi, 10000), rng.uniform(-1.4, 1.4, 10000)
    alon, alat = plon + np.pi, -plat
    alat[1::2] += rng.uniform(-1e-9, 1e-9, 5000)           # half of them beside the computed antipode, within the NaN zone's reach
    d = rc.run_ref_distance(exe, tmp, alon, alat, plon, plat)
    k = np.flatnonzero(np.isnan(d))
    print("antipodal placements with a NaN distance:", k.size, "of", d.size)
    return None if k.size == 0 else ((plon[k[0]], plat[k[0]]), (alon[k[0]], alat[k[0]]))


def main():
    tmp = tempfile.mkdtemp(prefix="rland_ref_")
    try:
        exe = rc.build_driver(tmp)
        anti = find_nan_antipode(exe, tmp)
        for name in rc.CASES:
            c = rc.case_inputs(name, anti)
            r = rc.run_ref(exe, tmp, c)
            on, off = c["mask_dst"] != 0, c["mask_dst"] == 0
            assert np.all(r["idx_map"][off] == -1) and np.all(r["face_map"][off] == -1) and np.all(r["idx_map_sf"][off] == -1)
            assert np.all(c["mask_src"][r["face_map"][on], r["idx_map"][on]] != 0) and np.all(c["mask_src"][c["iface_dst"], r["idx_map_sf"][on]] != 0)
            needs_sf = int((r["face_map"][on] != c["iface_dst"]).sum())
            if name in ("cube_small", "frames", "dup_points", "latlon_ties", "beyond_pole_source", "beyond_pole_query"):
                assert needs_sf > 0 and needs_sf < on.sum()
            if name == "frames":
                assert c["lon_dst"].min() < -2.4263 and c["lon_src"].max() > 2.4263
                small = rc.run_ref(exe, tmp, rc.case_inputs("cube_small"))
                print("frames: answers that differ from cube_small's (ties of the symmetric grid, decided by the last bits of d):",
                      [int((small[k] != r[k]).sum()) for k in rc.OUTPUTS])
            if name == "dup_points":
                n0 = 144
                assert r["face_map"][n0] == 1 and r["idx_map"][n0] == 10 and r["face_map"][n0 + 1] == 0 and r["idx_map"][n0 + 1] == 20
            if name.startswith("beyond_pole"):
                assert np.abs(c["lat_dst"][:20]).min() > np.pi / 2 and np.abs(c["lat_dst"][20:]).max() < np.pi / 2
                assert (np.abs(c["lat_src"]).max() > np.pi / 2) == (name == "beyond_pole_source")
                d = rc.run_ref_distance(exe, tmp, np.repeat(c["lon_dst"][:20], 2), np.repeat(c["lat_dst"][:20], 2), c["lon_src"][0], c["lat_src"][0])
                print(name, "the reference's d of the 40 close pairs: NaN", int(np.isnan(d).sum()), "largest finite", np.nanmax(d), "m")
            if name == "antipode_first" and anti is not None:
                assert r["face_map"][61] == 0 and r["idx_map"][61] == 3, "the NaN distance of the first point must be accepted"
            np.savez_compressed(rc.golden_path(name), libc=np.array(" ".join(platform.libc_ver())), nan_first=np.array(int(anti is not None)),
                                **{k: np.asarray(c[k]) for k in rc.INPUTS}, **r)
            print(name, "queries", int(on.sum()), "same-face searches", needs_sf, os.path.getsize(rc.golden_path(name)), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
