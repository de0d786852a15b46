"""tests/gc_fatal_cases.py on the CPU: ties the oracle's negative codes, which the GPU test (tests/test_gpu_gc_fatal.py) compares the
device with, to the compiled reference, whose clip ends the process instead.

* Every pair case: a fresh child process gives the polygon to the reference's own clip_2dx2d_great_circle (oracle/_ref) against the
  cells of its grid in ascending order, as the polygon-list loop would.  It survives the cells before the first fatal one, then
  exits non-zero with the reference's message for the oracle's code on stderr.  (Code 11 is the exception: the reference's
  insertIntersect does not return on those pairs, so no child is started for them; the two builds of the oracle agree.)
* Every grid case: the plain and the _cr grid-level oracle return the same -(100 + code) or the same exchange grid; the fatal ones
  end the reference's create_xgrid_great_circle in a child with the text of that code, the silent ones return the oracle's count.
* The module's own conditions (which codes the cases cover) hold; they are asserted when it is imported.

No tolerance: codes, texts and index lists are compared for equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gc_fatal_cases as gf
import orc
import polylist_gc_cases as pc

TESTS = os.path.dirname(os.path.abspath(__file__))

CHILD_PAIR = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import polylist_gc_cases as pc
d = np.load(sys.argv[2])
clip = pc.prims_ref().clip
for k, cell in enumerate(d["cells"]):
    n = clip(d["poly"], cell)[0]
    print("cell", k, "returned", n, flush=True)
print("survived", flush=True)
"""

CHILD_GRID = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import orc
d = np.load(sys.argv[2])
r = orc.ref_create_xgrid_gc(int(d["nx1"]), int(d["ny1"]), int(d["nx2"]), int(d["ny2"]), d["lon1"], d["lat1"], d["lon2"], d["lat2"], mask=d["mask"])
print("nxgrid", r["n"], flush=True)
"""


@pytest.fixture(scope="module")
def ref_built():
    if not orc.ref_available():
        pytest.fail("oracle/_ref/libfrenc_ref.so has not been built (build() compiles it from the reference's sources)")


def _child(code, tmp_path, **arrays):
    inp = str(tmp_path / "in.npz")
    np.savez(inp, **arrays)
    return subprocess.run([sys.executable, "-c", code, TESTS, inp], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("name", list(gf.PAIR_CASES))
def test_the_reference_dies_on_the_pair_case_with_the_text_of_the_code(ref_built, tmp_path, name):
    c = gf.PAIR_CASES[name]
    g = gf.PAIR_GRIDS[c["grid"]]
    codes = gf.pair_codes(c["poly"], g, False)
    assert codes and set(codes.values()) == {-c["code"]}
    cells = np.nonzero(pc.range_pass(c["poly"], g.cells))[0]
    first = int(np.nonzero(cells == min(codes))[0][0])              # cells before it: the oracle returns a count
    if c["code"] in gf.NO_REFERENCE_TEXT:                           # the reference does not end on this pair: nothing to start
        assert gf.pair_codes(c["poly"], g, True) == codes
        return
    r = _child(CHILD_PAIR, tmp_path, poly=c["poly"], cells=g.cells[cells])
    print(name, "first fatal cell", min(codes), "child", r.returncode, r.stdout.strip().splitlines()[-1:], r.stderr.strip())
    assert r.returncode != 0 and r.returncode > 0, (r.returncode, r.stderr)       # exit(1), not a signal
    assert "survived" not in r.stdout
    assert r.stdout.count("returned") == first
    assert "FATAL Error: " + gf.MESSAGES[c["code"]] in r.stderr.split("\n"), r.stderr


def test_the_reference_survives_the_ordinary_polygons(ref_built, tmp_path):
    """the child's own teeth: on the four ordinary polygons and the clean grid it runs to its end"""
    n, xyz = gf.ordinary()
    g = gf.PAIR_GRIDS[gf.CLEAN_GRID]
    for k in range(len(n)):
        p = xyz[k, :n[k]]
        cells = np.nonzero(pc.range_pass(p, g.cells))[0]
        r = _child(CHILD_PAIR, tmp_path, poly=p, cells=g.cells[cells])
        assert r.returncode == 0 and r.stdout.count("returned") == len(cells) and "survived" in r.stdout, (k, r.stderr)


@pytest.mark.parametrize("name", list(gf.GRID_CASES))
def test_grid_case_under_both_builds_and_the_reference(ref_built, tmp_path, name):
    c = gf.GRID_CASES[name]
    plain, cr = (gf.grid_result(c["src"], c["dst"], c["mask"], b) for b in (False, True))
    assert plain[0] == cr[0]
    mask = np.ones(c["src"][0] * c["src"][1]) if c["mask"] is None else c["mask"]
    r = _child(CHILD_GRID, tmp_path, nx1=c["src"][0], ny1=c["src"][1], nx2=c["dst"][0], ny2=c["dst"][1], lon1=c["src"][2], lat1=c["src"][3],
               lon2=c["dst"][2], lat2=c["dst"][3], mask=mask)
    print(name, plain[0], plain[1] if plain[0] == "code" else plain[1]["n"], "child", r.returncode, r.stdout.strip(), r.stderr.strip())
    if name in gf.SILENT:
        assert plain[0] == "n" and plain[1]["n"] == cr[1]["n"]
        for k in ("i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(plain[1][k], cr[1][k]), k
        assert r.returncode == 0 and r.stdout.split() == ["nxgrid", str(plain[1]["n"])], (r.stdout, r.stderr)
    else:
        assert plain[0] == "code" and plain[1] == cr[1]
        assert r.returncode > 0 and "nxgrid" not in r.stdout
        assert "FATAL Error: " + gf.MESSAGES[plain[1]] in r.stderr.split("\n"), r.stderr


def test_what_the_cases_cover():
    print("pair cases per code", gf.PAIR_CODES_COVERED, "grid cases", sorted(gf.GRID_CODES_COVERED), "not reached", sorted(gf.NOT_REACHED))
    assert set(gf.PAIR_CODES_COVERED) >= {1, 2, 5, 6} and gf.GRID_CODES_COVERED >= {1, 2}
    assert all(v <= 3 for v in gf.PAIR_CODES_COVERED.values())
    assert not (set(gf.PAIR_CODES_COVERED) | gf.GRID_CODES_COVERED) & set(gf.NOT_REACHED)
    assert set(gf.MESSAGES) | {9} == set(range(1, 10)) | gf.NO_REFERENCE_TEXT
    for name in gf.MIXED_GRIDS:                                       # two codes, and the device's order picks one of them
        codes = gf.grid_facts(name)[1]["codes"]
        assert len(codes) == 2 and gf.device_code(codes) in codes
    assert gf.device_code({5, 6}) == 6 and gf.device_code({6, 2}) == 2 and gf.device_code({7, 2, 1}) == 1
