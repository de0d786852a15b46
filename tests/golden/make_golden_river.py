#!/usr/bin/env python3
"""Generate tests/golden/river_*.npz from the REFERENCE's init_river_data, calc_max_subA, calc_tocell, calc_river_data,
sort_basin and check_river_data (tools/river_regrid/river_regrid.c:642-1376).

Run where the reference's sources are present (FRE_REFERENCE, default /root/reference) and oracle/_ref has been built (the
cube tiles come from the reference's generator):
    python tests/golden/make_golden_river.py
tests/capi/river_ref_driver.c is compiled around the reference's river_regrid.c (function sections, --gc-sections: none of its
netCDF-bound functions is kept) with create_xgrid.c, mosaic_util.c, mpp.c and mpp_domain.c in a temporary directory outside the
repository; nothing compiled is kept.  Each file holds (data only):
  inputs    river_cases.INPUTS: the network's axes, bounds and subA, the six missing values, per tile the corners (radians), the
            centres (degrees), the land fraction before and after the thresholds, opcode, gca (great-circle areas), suba_cutoff
  outputs   area, xt_halo, yt_halo (after the halo update), max_suba (with halo, before calc_tocell), subA, cellarea,
            celllength, tocell, travel, basin, basin_presort, last_point (interior), and check_river_data's four counts
  libc      the C library of the host that made the file: areas and lengths carry its sin/cos bits
Every case asserts the feature it is there for on the reference's outputs; a case that fails gets other parameters."""
import os
import platform
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import river_cases as rv  # noqa: E402


def check_features(name, c, r):
    f = rv.features(c, r)
    print(name, "maxtravel", int(r["maxtravel"]), "maxbasin", int(r["maxbasin"]), f)
    if name in ("cube_c8_continent", "latlon_continent"):
        assert int(r["maxtravel"]) >= 8
    if int(c["opcode"]) in (3, 4):
        assert f["halo_flows"] >= 10
    if name in ("latlon_shift", "latlon_aligned"):
        assert f["tie_outlets"] >= 10
    if name == "cube_c12":
        assert f["above"] > 0 and f["below"] > 0
    if name == "missing_rows":
        assert f["empty"] >= 1
    if name == "latlon_aligned":                     # every cell edge is a source edge
        assert np.array_equal(c["xb_r"][0, 0], c["src_xb_r"]) and np.array_equal(c["yb_r"][0, :, 0], c["src_yb_r"])
    if name == "latlon_shift":
        assert c["xb_r"].min() < 0 and c["xb_r"].max() > np.pi
    if name == "torus_rect":
        assert c["xt"].shape[1] != c["xt"].shape[2]


def main():
    tmp = tempfile.mkdtemp(prefix="river_ref_")
    try:
        exe = rv.build_driver(tmp)
        for name in rv.CASES:
            c = rv.case_inputs(name)
            r = rv.run_ref(exe, tmp, c)                  # a fatal error of the reference stops here
            check_features(name, c, r)
            r.pop("seconds")
            np.savez_compressed(rv.golden_path(name), libc=np.array(" ".join(platform.libc_ver())),
                                **{k: np.asarray(c[k]) for k in rv.INPUTS}, **r)
            print(name, os.path.getsize(rv.golden_path(name)), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
