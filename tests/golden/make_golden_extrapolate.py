#!/usr/bin/env python3
"""Generate tests/golden/extrapolate_*.npz and extrapolate_cpu_baseline.json from the REFERENCE's do_extrapolate,
setup_vertical_interp and do_vertical_interp (tools/fregrid/fregrid_util.c, tools/libfrencutils/interp.c).

Run where the reference's sources are present (FRE_REFERENCE, default /root/reference):
    python tests/golden/make_golden_extrapolate.py
tests/capi/extrapolate_ref_driver.c is compiled with the reference's fregrid_util.c (function sections, --gc-sections: none of
its netCDF-bound functions is kept), mpp.c, interp.c and mosaic_util.c in a temporary directory outside the repository; nothing
compiled is kept.  The inputs are not stored: tests/extrap_cases.py rebuilds them from exact arithmetic.  Each file holds (data only):
  iters [nk]            the iteration count the reference printed per level
  maxres_printed [nk]   the maxres it printed (%g)
  sha256                of the output bytes
  out [nk, nj, ni]      the output (small cases) / sample [4096] a strided sample of it (the two real-size cases)
vertical cases: out [nk2, nxy], kinfo = kstart, kend, need_interp.
extrapolate_cpu_baseline.json: the reference's wall time of do_extrapolate per case on one core of the machine that made the fixtures."""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import extrap_cases as ec  # noqa: E402


def main():
    tmp = tempfile.mkdtemp(prefix="extrap_ref_")
    base = {}
    try:
        exe = ec.build_driver(tmp)
        for name in ec.SMALL_CASES + ec.LARGE_CASES:
            c = ec.extrap_case(name)
            out, iters, printed, sec = ec.run_ref_extrap(exe, tmp, c)
            if name == "cap":
                assert iters[0] == 3999, f"the cap case stopped after {iters[0]} iterations: pick another mask"
            if name == "none_missing":
                assert np.all(iters == 0) and np.array_equal(out, c["data"])
            np.savez_compressed(ec.golden_path(name), **ec.fixture_of(name, out, iters, printed, sec))
            base[name] = {"ni": c["ni"], "nj": c["nj"], "nk": c["nk"], "stop_crit": c["stop_crit"], "iters": [int(v) for v in iters],
                          "seconds_cpu": sec}
            print(name, iters, printed, f"{sec:.3f} s")
        for ni, nj, nk in ((360, 180, 33), (1440, 720, 8)):                # scripts/extrap_time.py's two cases
            c = ec.timing_case(ni, nj, nk)
            _, iters, _, sec = ec.run_ref_extrap(exe, tmp, c)
            base[f"timing_{ni}x{nj}x{nk}"] = {"ni": ni, "nj": nj, "nk": nk, "stop_crit": c["stop_crit"],
                                               "iters": [int(v) for v in iters], "seconds_cpu": sec}
            print("timing", ni, nj, nk, iters, f"{sec:.3f} s")
        for name in ec.VERTICAL_CASES:
            c = ec.vertical_case(name)
            out, ks, ke, need = ec.run_ref_vertical(exe, tmp, c)
            np.savez_compressed(ec.golden_path(name), out=out, kinfo=np.array([ks, ke, need], dtype=np.int32))
            print(name, out.shape, ks, ke, need)
        with open(os.path.join(HERE, "extrapolate_cpu_baseline.json"), "w") as f:
            json.dump(base, f, indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
