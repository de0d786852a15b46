"""The rectilinear quad clip with its axis-aligned inside tests: one product where d_inside_edge has two (d_clip_quad_sh,
csrc/xgrid_kernels.hip).

Grid cases (tests/test_clip_axis_predicate_host.py: targets): C8, six tiles, orders 1 and 2, onto (a) 36x18 global from 0, every
column vertical; (b) 36x18 global from -2.5 and (c) a 10x10 window from -0.5, each with one column that fix_lon leaves not exactly
vertical -- the quad kernel hands that column's pairs to the general kernel; (d) a 12x6 window over the prime meridian with both
signs of the +-2 pi shift and the `wrap` branch.  Every case runs on the rectilinear path and with fg_set_search_rect(0) and is
compared with the CPU oracle and, where it was built, the compiled reference, as tests/test_gpu_clip_edges.py states it: index
lists equal, areas and centroid integrals equal in bits under orc.host_has_fma(), else 1e-10.  That the cases hold their columns
is asserted on the CPU (test_clip_axis_predicate_host.py::test_the_cases_hold_what_they_are_there_for).

All plans are made in one child process."""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _plan(fg, order, srcs, tgt, rect):
    L = fg.lib()
    L.fg_set_search_rect(1 if rect else 0)
    try:
        nx2, ny2, lo, la = tgt
        p = fg.XgridPlan.create(order, [fg.GridConfig(nx, ny, lon, lat) for (nx, ny, lon, lat) in srcs], fg.GridConfig(nx2, ny2, lo, la))
        x = p.get_xgrid()                              # before finalize: c1 / c2 are the two centroid integrals
        st = p.stats()
        p.destroy()
        return dict(x={k: np.array(v) for k, v in x.items()}, stats=dict(st))
    finally:
        L.fg_set_search_rect(1)


def _child(path):
    sys.path.insert(0, HERE)
    import conftest
    import test_clip_axis_predicate_host as host
    fg = conftest.load_package()
    assert fg.lib().fg_device_count() >= 1
    out = {}
    srcs = host.sources(fg)
    for name, tgt in host.targets(fg).items():
        for order in (1, 2):
            for rect in (True, False):
                out[(name, order, rect)] = _plan(fg, order, srcs, tgt, rect)
    with open(path, "wb") as f:
        pickle.dump(out, f)


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


@pytest.fixture(scope="module")
def runs(gpu_ok):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "runs.pkl")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with open(path, "rb") as f:
            return pickle.load(f)


_oracle = {}


def oracle(fg, name, order):
    """the CPU oracle's lists, and the compiled reference's where it is built, tile by tile; made once"""
    import test_clip_axis_predicate_host as host
    if (name, order) not in _oracle:
        nx2, ny2, lo, la = host.targets(fg)[name]
        o = [orc.orc_create_xgrid(order, nx, ny, nx2, ny2, lon, lat, lo, la) for (nx, ny, lon, lat) in host.sources(fg)]
        r = [orc.ref_create_xgrid(order, nx, ny, nx2, ny2, lon, lat, lo, la) for (nx, ny, lon, lat) in host.sources(fg)] \
            if orc.ref_available() else None
        _oracle[(name, order)] = (o, r)
    return _oracle[(name, order)]


@pytest.mark.parametrize("rect", [True, False], ids=["rect", "generic"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_grid_case_equals_the_oracle(fg, runs, name, order, rect):
    from test_gpu_clip_edges import assert_equals_the_oracle
    r = runs[(name, order, rect)]
    what = f"case ({name}), order {order}, {'rectilinear' if rect else 'generic'} path"
    assert (r["stats"]["bins"] == 0) == rect, (what, "took the other path", r["stats"])
    o, ref = oracle(fg, name, order)
    assert_equals_the_oracle(r["x"], o, order, what + " against the CPU oracle")
    if ref is not None:
        assert_equals_the_oracle(r["x"], ref, order, what + " against the compiled reference")


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_rectilinear_and_generic_paths_agree_in_bits(runs, name, order):
    r, g = runs[(name, order, True)]["x"], runs[(name, order, False)]["x"]
    assert sorted(r) == sorted(g)
    for k in r:
        a, b = np.ascontiguousarray(r[k]), np.ascontiguousarray(g[k])
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, order, k)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_pairs_the_quad_kernel_defers(fg, runs, name, order):
    """On the rectilinear path the quad kernel takes every source cell (up to 8 vertices) and defers a pair for three reasons only:
    its column is not exactly vertical, an intermediate polygon of more than 8 vertices, more than two crossings of one cutting
    line.  The CPU walk finds neither of the last two in these cases, so (a) and (d), without such a column, defer nothing; (b)
    and (c) defer at least the candidate pairs of their flagged columns (at least: the device's candidate list may hold pairs
    that the reference's longitude test drops)."""
    import test_clip_axis_predicate_host as host
    st = runs[(name, order, True)]["stats"]
    flagged = sum(1 for p in host.walk(fg, name)["pairs"] if p["flagged"])
    print(f"case ({name}) order {order}: deferred {st['deferred']}, pairs {st['pairs']}, CPU candidate pairs "
          f"{len(host.walk(fg, name)['pairs'])}, of flagged columns {flagged}")
    if name in "ad":
        assert flagged == 0 and st["deferred"] == 0, st
    else:
        assert flagged > 0 and st["deferred"] >= flagged, (st, flagged)
        assert st["deferred"] < st["pairs"], st
