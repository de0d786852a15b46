"""Stream-ordered plans (fg_set_search_async): a fused search returns at its counter readback with its
centroid pass and CSR records still queued, fg_plan_destroy does not drain the stream, and the pool hands blocks from one plan to
the next in stream order.  Every plan made that way is compared bit for bit with the same plan made under fg_set_search_async(0):
exchange cells, areas, c1 / c2 and an 8-level order-2 apply.  Shapes: C24 -> 72x36 and C48 -> 144x90 (tests/test_gpu_fused.py).

The poisoned variant runs in a child process that sets FREGRID_HIP_POISON=1 before the library loads (the pool then fills every
block it hands out with 0x7f bytes behind a device-wide synchronise), as tests/test_gpu_src_records_compact.py does."""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {"C24": (24, 72, 36), "C48": (48, 144, 90)}
DEV = "cuda:0"


class Grids:
    """device corner arrays of one shape, and the fields of the 8-level apply"""

    def __init__(self, fg, name):
        import torch
        self.ni, self.nlon, self.nlat = SHAPES[name]
        lon, lat = fg.gnomonic_ed_corners(self.ni)
        lo, la = fg.latlon_corners(self.nlon, self.nlat)
        self.host = (lon, lat, lo, la)
        self.lon = [torch.from_numpy(lon[t]).to(DEV) for t in range(6)]
        self.lat = [torch.from_numpy(lat[t]).to(DEV) for t in range(6)]
        self.lo, self.la = torch.from_numpy(lo).to(DEV), torch.from_numpy(la).to(DEV)
        self.nsrc = 6 * self.ni * self.ni
        self.ndst = self.nlon * self.nlat
        rng = np.random.default_rng(7)
        self.src = {2: torch.from_numpy(rng.standard_normal((8, 6 * (self.ni + 2) ** 2))).to(DEV),
                    1: torch.from_numpy(rng.standard_normal((8, self.nsrc))).to(DEV)}
        self.gx = torch.from_numpy(rng.standard_normal((8, self.nsrc))).to(DEV)
        self.gy = torch.from_numpy(rng.standard_normal((8, self.nsrc))).to(DEV)
        torch.cuda.synchronize()


def make(fg, g, stream, async_on, order=2, fused=True, exact=False, target=None):
    """a plan on `stream` (a torch stream, or None = a stream of the plan's own); target: another destination (nx, ny, lon_t, lat_t)"""
    L = fg.lib()
    L.fg_set_search_async(1 if async_on else 0); L.fg_set_search_finalize(1 if fused else 0); L.fg_set_search_mode(1 if exact else 0)
    try:
        nx, ny, lo, la = target if target else (g.nlon, g.nlat, g.lo, g.la)
        return fg.XgridPlan.create_dev(order, [g.ni] * 6, [g.ni] * 6, g.lon, g.lat, nx, ny, lo, la,
                                       stream=None if stream is None else stream.cuda_stream)
    finally:
        L.fg_set_search_async(1); L.fg_set_search_finalize(0); L.fg_set_search_mode(0)


def apply8(g, p, stream, ndst=None):
    """the 8-level apply queued on the plan's stream; the output after that stream has drained"""
    import torch
    with torch.cuda.stream(stream):                   # (the fill is ordered ahead of the apply on the same stream)
        out = torch.full((8, ndst or g.ndst), np.nan, dtype=torch.float64, device=DEV)
    if p.order == 2:
        p.apply(g.src[2], out, nz=8, grad_x_t=g.gx, grad_y_t=g.gy)
    else:
        p.apply(g.src[1], out, nz=8)
    p.sync()
    return out.cpu().numpy()


def results(g, p, stream, ndst=None):
    """apply FIRST (queued behind whatever the search left in flight), then the exchange cells"""
    out = apply8(g, p, stream, ndst)
    return dict(p.get_xgrid(), out=out, n=p.nxgrid)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def assert_same(a, b, what=""):
    assert a["n"] == b["n"] > 0, what
    for k in ("t_in", "i_in", "j_in", "i_out", "j_out", "area", "c1", "c2", "out"):
        if k in b:
            assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


_cache = {}


def shape(fg, name):
    if ("g", name) not in _cache:
        _cache["g", name] = Grids(fg, name)
    return _cache["g", name]


def reference(fg, name, order=2):
    """the plan of fg_set_search_async(0), two-call finalize, made once per shape and order"""
    import torch
    if ("ref", name, order) not in _cache:
        g = shape(fg, name)
        p = make(fg, g, torch.cuda.current_stream(), False, order=order, fused=False)
        p.finalize(None)
        _cache["ref", name, order] = results(g, p, torch.cuda.current_stream())
        p.destroy()
    return _cache["ref", name, order]


def alternating(fg, n, stream, keep_every=1):
    """n fused plans alternating between the two shapes on one stream, each destroyed straight after create with no synchronisation
    in between; every keep_every-th is made once more and kept for its results"""
    res = []
    for k in range(n):
        name = ("C24", "C48")[k % 2]
        g = shape(fg, name)
        make(fg, g, stream, True).destroy()
        if k % keep_every == 0:
            p = make(fg, g, stream, True)
            res.append((name, results(g, p, stream)))
            p.destroy()
    return res


# --------------------------------------------------------------------------------------------------------------------------------
def test_plans_back_to_back_on_one_stream(fg, gpu_ok):
    import torch
    for name, r in alternating(fg, 20, torch.cuda.current_stream(), keep_every=5):
        assert_same(r, reference(fg, name), name)
    torch.cuda.synchronize()


def _child(path):
    sys.path.insert(0, HERE)
    import conftest
    import torch
    fg = conftest.load_package()
    out = {"res": alternating(fg, 20, torch.cuda.current_stream(), keep_every=5)}
    out["ref"] = {name: reference(fg, name) for name in SHAPES}
    torch.cuda.synchronize()
    with open(path, "wb") as f:
        pickle.dump(out, f)


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


def test_plans_back_to_back_with_a_poisoned_pool(fg, gpu_ok):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "plans.pkl")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, FREGRID_HIP_POISON="1"),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with open(path, "rb") as f:
            out = pickle.load(f)
    assert len(out["res"]) == 4
    for name, r in out["res"]:
        assert_same(r, out["ref"][name], "child " + name)
        assert_same(r, reference(fg, name), "parent " + name)


@pytest.mark.parametrize("second", ["same stream", "another stream"])
def test_predecessor_still_in_flight(fg, gpu_ok, second):
    """a large float64 product queued ahead of plan A keeps the stream busy (about 0.1 s) while A is created and destroyed and B
    created: B's blocks are A's, still in use; on another stream B takes them behind the event of A's batch"""
    import torch
    s1 = torch.cuda.Stream()
    s2 = s1 if second == "same stream" else torch.cuda.Stream()
    ga, gb = shape(fg, "C48"), shape(fg, "C24")
    ref_a, ref_b = reference(fg, "C48"), reference(fg, "C24")
    a = torch.ones((6144, 6144), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    fg.lib().fg_pool_release()                         # B can only get blocks that A gave back
    with torch.cuda.stream(s1):
        c = torch.mm(a, a)
    pa = make(fg, ga, s1, True)                        # (returns when ITS counters are back: behind the product)
    with torch.cuda.stream(s1):
        c2 = torch.mm(a, a)                            # legitimate long work between A's search and its destroy: A's blocks go
    pa.destroy()                                       # back behind it, and B below asks for them while it runs
    pb = make(fg, gb, s2, True)
    rb = results(gb, pb, s2)
    pb.destroy()
    pa2 = make(fg, ga, s1, True)
    ra = results(ga, pa2, s1)
    pa2.destroy()
    torch.cuda.synchronize()
    assert float(c[0, 0]) == 6144.0 == float(c2[-1, -1])
    assert_same(rb, ref_b, "B")
    assert_same(ra, ref_a, "A")


@pytest.mark.parametrize("consumer", ["sweep", "get_xgrid", "get_cell_struct", "set_stream + apply"])
def test_consumers_off_the_plans_stream(fg, gpu_ok, consumer):
    """straight after a fused create, with the centroid pass and the CSR records possibly still queued"""
    import torch
    g = shape(fg, "C48")
    s1 = torch.cuda.Stream()
    if consumer == "sweep":                            # fg.Sweep runs the plan on its own compute stream (order 1: no gradient object)
        hin = g.src[1].cpu().numpy()
        outs = {}
        for async_on in (False, True):
            if async_on:
                make(fg, g, s1, True, order=1).destroy()
            p = make(fg, g, s1, async_on, order=1)
            sw = fg.Sweep([p], None, np.float64, np.float64)
            outs[async_on] = np.full((8, g.ndst), np.nan)
            sw.run(hin, [outs[async_on]])
            sw.destroy()
            if not async_on:
                p.destroy()
        assert np.isfinite(outs[False]).all() and np.array_equal(bits(outs[True]), bits(outs[False]))
        assert_same(results(g, p, s1), reference(fg, "C48", order=1))
    elif consumer == "get_xgrid":
        ref = reference(fg, "C48")
        p = make(fg, g, s1, True)
        x = dict(p.get_xgrid(), n=p.nxgrid)            # c1 / c2 need the centroids of every source cell
        assert_same(x, {k: v for k, v in ref.items() if k != "out"})
    elif consumer == "get_cell_struct":
        p0 = make(fg, g, s1, False, fused=False)
        want = p0.get_cell_struct(0, g.nsrc)
        p0.destroy()
        p = make(fg, g, s1, True)
        got = p.get_cell_struct(0, g.nsrc)
        for k in want:
            assert np.array_equal(bits(got[k]), bits(want[k])), k
        assert_same(results(g, p, s1), reference(fg, "C48"))
    else:
        s2 = torch.cuda.Stream()
        p = make(fg, g, s1, True)
        p.set_stream(s2.cuda_stream)
        assert_same(results(g, p, s2), reference(fg, "C48"))
    p.destroy()
    torch.cuda.synchronize()


def test_repeated_attempts_behind_an_undrained_predecessor(fg, gpu_ok):
    """exact mode sizes by counting and a cubed-sphere tile fails the rectilinear check: several attempts, the first of them
    behind a plan that was destroyed without a drain"""
    import torch
    g = shape(fg, "C48")
    l2, a2 = fg.gnomonic_ed_corners(32)
    tgt = (32, 32, torch.from_numpy(l2[2]).to(DEV), torch.from_numpy(a2[2]).to(DEV))
    s1 = torch.cuda.Stream()
    torch.cuda.synchronize()
    p0 = make(fg, g, s1, False, fused=False, exact=True, target=tgt)
    p0.finalize(None)
    ref = results(g, p0, s1, ndst=32 * 32)
    p0.destroy()
    make(fg, g, s1, True).destroy()                    # the predecessor, not drained
    p = make(fg, g, s1, True, exact=True, target=tgt)
    assert p.stats()["exact_mode"] == 1 and p.stats()["bins"] > 0
    assert_same(results(g, p, s1, ndst=32 * 32), ref)
    p.destroy()
    torch.cuda.synchronize()


def test_profiling_keeps_the_full_synchronise(fg, gpu_ok):
    import torch
    g = shape(fg, "C24")
    fg.lib().fg_set_profiling(1)
    try:
        p = make(fg, g, torch.cuda.current_stream(), True)
        ms = p.phase_ms()
    finally:
        fg.lib().fg_set_profiling(0)
    assert ms["finalize"] > 0 and ms["search_total"] > 0
    assert_same(results(g, p, torch.cuda.current_stream()), reference(fg, "C24"))
    p.destroy()


def test_pool_release_after_an_undrained_destroy(fg, gpu_ok):
    import torch
    g = shape(fg, "C48")
    s1 = torch.cuda.Stream()
    make(fg, g, s1, True).destroy()
    fg.lib().fg_pool_release()                         # waits for the batch's event before it frees the blocks
    p = make(fg, g, s1, True)
    r = results(g, p, s1)
    p.destroy()
    torch.cuda.synchronize()                           # (a freed block still in use would surface here as a fault)
    assert_same(r, reference(fg, "C48"))


def test_two_call_finalize_on_a_caller_stream(fg, gpu_ok):
    """fg_plan_finalize with totals on a stream the caller supplied returns without a host wait; the totals are the plan's own
    sums, copied on that stream"""
    import torch
    g = shape(fg, "C48")
    s1 = torch.cuda.Stream()
    res = {}
    for async_on in (False, True):
        p = make(fg, g, s1, async_on, fused=False)
        with torch.cuda.stream(s1):
            tot = torch.empty(3 * g.nsrc, dtype=torch.float64, device=DEV)
        p.copy_cell_sums(tot)
        p.finalize(tot.data_ptr())
        res[async_on] = results(g, p, s1)
        p.destroy()
        s1.synchronize()
        del tot
    assert_same(res[True], res[False])
    assert_same(res[True], reference(fg, "C48"))


def test_footprint_does_not_grow(fg, gpu_ok):
    """Device memory in use after 3 warm-up cycles and after 40 cycles of the alternating test.  Allowance: the blocks of ONE plan
    of the larger shape, from the plan's own block list (fg_plan_device_bytes: the pool's class size of every block a searched,
    finalized C48 -> 144x90 plan holds; printed below).  Stream order needs none of it -- a plan's blocks are back before the next
    plan asks -- so the expected growth is 0 either way.  With the switch at 0 nothing may grow."""
    import ctypes as C
    import torch
    cur = torch.cuda.current_stream()
    free = lambda: torch.cuda.mem_get_info()[0]
    reference(fg, "C24"); reference(fg, "C48")
    L = fg.lib()
    L.fg_plan_device_bytes.restype = C.c_long
    L.fg_plan_device_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.c_int]
    p = make(fg, shape(fg, "C48"), cur, True)
    sizes = (C.c_long * 128)()
    one_plan = int(L.fg_plan_device_bytes(p._h, sizes, 128))
    blocks = [int(b) for b in sizes if b]
    p.destroy()
    print(f"blocks of one C48 -> 144x90 plan: {len(blocks)} blocks, {one_plan} B: {sorted(blocks, reverse=True)}")
    assert 0 < one_plan == sum(blocks)
    for async_on, allowance in ((False, 0), (True, one_plan)):
        torch.cuda.synchronize(); L.fg_pool_release()
        f0 = free()
        cycle = lambda n: [make(fg, shape(fg, ("C24", "C48")[k % 2]), cur, async_on).destroy() for k in range(n)]
        cycle(3)
        torch.cuda.synchronize(); f3 = free()
        cycle(40)
        torch.cuda.synchronize(); f40 = free()
        print(f"async={async_on}: in use after 3 cycles {f0 - f3} B, growth over 40 more {f3 - f40} B, allowance {allowance} B")
        assert f3 - f40 <= allowance, (async_on, f3 - f40, allowance)
