#!/usr/bin/env python3
"""Writes tests/golden/coupler_c0.npz and coupler_c1.npz: what the restatement of make_coupler_mosaic.c in tests/coupler_cases.py
gives for case C (a C4 atmosphere = land over a 12 x 8 lat-lon ocean with omask == 0 and omask == 1) on a host whose libm runs its
FMA build (tests/orc.py:host_has_fma).  Needs oracle/_ref (the reference compiled in place); no GPU.

    python tests/golden/make_golden_coupler.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import __graft_entry__  # noqa: E402
import coupler_cases as cc  # noqa: E402


def flatten(r):
    """the restatement's result as a flat dict of arrays"""
    out = {"nbad": np.array(r["nbad"])}
    for na, t in enumerate(r["axo"]):
        for k, v in t.items():
            out[f"axo{na}_{k}"] = v
    for na, row in enumerate(r["axl"]):
        for k, v in row[na].items():
            out[f"axl{na}_{k}"] = v
    for k in ("o_area", "o_clon", "o_clat"):
        out[k] = r["ocean"][k]
    for na, a in enumerate(r["atmos"]):
        for k in ("a_area", "a_clon", "a_clat"):
            out[f"{k}{na}"] = a[k]
    for nl, l in enumerate(r["land"]):
        out[f"l_mask{nl}"] = l["mask"]
    return out


if __name__ == "__main__":
    fg = __graft_entry__.load_package()
    for name in ("c0", "c1"):
        _, r = cc.reference_of(name, fg, 2)
        np.savez_compressed(os.path.join(HERE, f"coupler_{name}.npz"), **flatten(r))
        print(name, "written")
