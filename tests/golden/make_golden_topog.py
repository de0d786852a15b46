#!/usr/bin/env python3
"""Generate tests/golden/topog_*.npz from the REFERENCE's conserve_interp / conserve_interp_great_circle (tools/libfrencutils/
interp.c:262-356), filter_topo, show_deepest and process_topo (tools/make_topog/topog.c:551-1048).

Run where the reference's sources are present (FRE_REFERENCE, default /root/reference) and the library has been built (the model
grids come from its host-side generators):
    python tests/golden/make_golden_topog.py
tests/capi/topog_ref_driver.c is compiled with the reference's topog.c, interp.c, create_xgrid.c, mosaic_util.c, mpp.c and
mpp_domain.c (function sections, --gc-sections: nothing bound to netCDF is kept) in a temporary directory outside the repository;
nothing compiled is kept.  Each file holds (data only):
  inputs    the switches of create_realistic_topog, zw, and for a chain case the model grid's corners (degrees), the file's axes,
            field (in its type) and missing value; for a stage case the depth handed to filter_topo / process_topo
  outputs   chain: jstart, jend, x_src, y_src, depth_src, mask_src, depth_remap; all: depth_filter, depth_final, num_levels (with a
            vertical grid), the three counts of the reference's debug notes and show_deepest's verdict
  libc      the C library of the host that made the file: the remap carries its sin/cos bits
Every case asserts the feature it is there for on the reference's outputs; a case that fails gets other parameters."""
import os
import platform
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import topog_cases as tc  # noqa: E402


def check_features(name, c, r):
    counts = {k: int(r[k]) for k in tc.COUNTS}
    print(name, tc.shape_of(c), counts, "land", int((r["depth_final"] == 0).sum()), "of", r["depth_final"].size)
    if int(c["mode"]) == 0:
        ny_src = c["yt_src"].size
        print("   rows", int(r["jstart"]), int(r["jend"]), "of", ny_src, "masked", int((r["mask_src"] == 0).sum()))
        assert (r["mask_src"] == 0).any() and (r["mask_src"] == 1).any()
        if name in ("regional", "fill_first_row"):
            assert int(r["jstart"]) > 0 and int(r["jend"]) < ny_src - 1
        if name == "on_grid":
            assert (r["depth_remap"] < 0).any() and (r["depth_remap"] == 0).any()
        elif not int(c["use_great_circle_algorithm"]):
            assert (r["depth_remap"] > 0).sum() > r["depth_remap"].size // 2
        if name == "fill_first_row":
            assert (r["depth_filter"][0] != 0).any() and not r["depth_final"][0].any()
        if int(c["filter_topog"]):
            assert not np.array_equal(r["depth_filter"], r["depth_remap"])
    if name == "process_defaults":
        assert all(counts[k] > 0 for k in ("isolated_filled", "partial_restricted", "shallow_modified"))
    if name in ("process_round_shallow", "process_deepen_shallow", "process_fill_shallow", "process_kmt_min4"):
        assert counts["shallow_modified"] >= 5
    if name in ("process_dont_open_very_this_cell", "process_fraction0_closed"):
        assert counts["partial_restricted"] >= 3
    if name.startswith("stairs_") or name.startswith("stale_halo"):
        assert counts["isolated_filled"] >= (10 if not name.endswith("keep_landmask") else 1)
    if name.startswith("filter_") and min(tc.shape_of(c)) >= 3 and int(c["num_filter_pass"]) > 0:
        assert not np.array_equal(r["depth_filter"], c["depth_in"])
    if name in ("filter_2x5", "filter_5x2", "filter_65x4_p0"):
        assert np.array_equal(r["depth_filter"], c["depth_in"])


def main():
    tmp = tempfile.mkdtemp(prefix="topog_ref_")
    try:
        exe = tc.build_driver(tmp)
        for name in tc.CASES:
            c = tc.case_inputs(name)
            r = tc.run_ref(exe, tmp, c)                  # a fatal error of the reference stops here
            check_features(name, c, r)
            r.pop("seconds")
            np.savez_compressed(tc.golden_path(name), libc=np.array(" ".join(platform.libc_ver())), **{k: np.asarray(v) for k, v in c.items()}, **r)
            print("  ", os.path.getsize(tc.golden_path(name)), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
