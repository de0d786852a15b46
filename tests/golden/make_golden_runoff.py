#!/usr/bin/env python3
"""Generate tests/golden/runoff_*.npz from the REFERENCE's nearest(), create_xgrid_1dx2d_order1 and get_grid_area
(tools/runoff_regrid/runoff_regrid.c, tools/libfrencutils/create_xgrid.c).

Run where the reference's sources are present (FRE_REFERENCE, default /root/reference):
    python tests/golden/make_golden_runoff.py
tests/capi/runoff_ref_driver.c is compiled with the reference's runoff_regrid.c (-Dmain=..., function sections, --gc-sections:
none of its netCDF-bound functions is kept), create_xgrid.c, mosaic_util.c, mpp.c and mpp_domain.c in a temporary directory
outside the repository; nothing compiled is kept.  Each file holds (data only):
  inputs    x_super, y_super (degrees), depth, xt1d_in, yt1d_in, data_in [3, ny_in, nx_in]   (tests/runoff_cases.py:case_inputs;
            the grids the tool derives from them are rebuilt on load by element-wise arithmetic)
  outputs   imap, jmap [ny, nx]; i_in, j_in, i_out, j_out, xgrid_area [nxgrid]; area_in, area_out (get_grid_area);
            data_out [3, ny, nx], totals [3, 2] (the driver's restatement of process_data's loops on the reference's list and maps)
  libc      the C library of the host that made the file: the grids, areas and distances carry its sin/cos bits
The assertions below hold on any host, with or without FMA."""
import os
import platform
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import runoff_cases as rc  # noqa: E402


def main():
    tmp = tempfile.mkdtemp(prefix="runoff_ref_")
    try:
        exe = rc.build_driver(tmp)
        for name in rc.CASES:
            c = rc.case_inputs(name)
            gi, go = rc.grids_of(c)
            r = rc.run_ref(exe, tmp, gi, go, c["data_in"])
            land, ocean = go["mask"] == 0, go["mask"] != 0
            assert ocean.any() and land.any()
            assert np.all(r["imap"][ocean] == -1) and np.all(r["imap"][land] >= 0), "a land cell without an ocean cell in range"
            assert np.all(go["mask"][r["jmap"][land], r["imap"][land]] != 0), "a land cell mapped to land"
            assert r["i_in"].size > 0 and np.all(gi["mask"][r["j_in"], r["i_in"]] != 0)
            assert np.all(np.isfinite(r["data_out"])) and np.all(r["data_out"][:2] >= 0) and np.all(r["data_out"][:2][:, land] == 0)
            assert (r["data_out"][2][land] < 0).any() and (r["data_out"][2][land] == 0).any(), "level 2 must exercise the > 0 test"
            if name == "tripolar_small":
                assert go["n_ext"] == 1 and go["xt"].min() < -2.43 and go["xt"].max() > 0.9
            if name == "latlon_regular":
                assert go["n_ext"] == 0 and ocean[14, 10] and (r["jmap"][land] == 14).any()
            if name == "one_ocean_cell":
                assert np.all(r["imap"][land] == 7) and np.all(r["jmap"][land] == 6)
            if name == "dup_points":
                assert go["xt"][5, 4] == go["xt"][7, 9] and go["yt"][5, 4] == go["yt"][7, 9]
                assert ((r["jmap"] == 5) & (r["imap"] == 4)).any() and not ((r["jmap"] == 7) & (r["imap"] == 9)).any()
            np.savez_compressed(rc.golden_path(name), libc=np.array(" ".join(platform.libc_ver())), **c, **r)
            print(name, go["ny"], go["nx"], "nxgrid", r["i_in"].size, "land", int(land.sum()), os.path.getsize(rc.golden_path(name)), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
