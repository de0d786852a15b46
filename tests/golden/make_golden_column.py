#!/usr/bin/env python3
"""Generate tests/golden/column_<dest>_<vgrid>.npz: the REFERENCE's whole ocean column loop -- do_extrapolate, then
do_scalar_conserve_interp on all seven levels at once, then do_vertical_interp -- on the inputs of tests/column_cases.py.

Run where the reference's sources are present and oracle/_ref/ has been built (make -C oracle):
    python tests/golden/make_golden_column.py
The fill and the levels come from tests/capi/extrapolate_ref_driver.c compiled in a temporary directory (nothing compiled is
kept), the remap from oracle/_ref/libconserve_ref.so.  The inputs are not stored.  Each file holds (data only):
  out   [3, nk2, ny, nx]  the double-precision result of the three records
  iters [3, 7]            the iteration counts the reference printed for the fill"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import column_cases as cc  # noqa: E402
from conftest import load_package  # noqa: E402


def main():
    fg = load_package()
    tmp = tempfile.mkdtemp(prefix="column_ref_")
    try:
        for (dest, vgrid), fx in cc.reference_results(fg, tmp).items():
            np.savez_compressed(cc.golden_path(dest, vgrid), **fx)
            print(dest, vgrid, fx["out"].shape, fx["iters"].tolist(), os.path.getsize(cc.golden_path(dest, vgrid)), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
