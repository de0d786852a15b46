"""ColumnSweep (fg_column_*): the streamed ocean column loop -- typed upload, widen, batched --extrapolate fill, conservative remap
of all levels, --dst_vgrid levels with narrowing, typed download -- against the REFERENCE's whole chain (tests/golden/column_*.npz,
made by tests/golden/make_golden_column.py; inputs rebuilt by tests/column_cases.py) and, for the typed paths, against the chain of
pinned calls on the same inputs.  No tolerance: bits and iteration counts."""
import ctypes as C

import numpy as np
import pytest

import column_cases as cc

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def rig(fg, gpu_ok):
    """the extrapolator and one finalized plan per destination, made once"""
    lon, lat = cc.source_axes()
    ex = fg.Extrapolator(lon, lat, 1)
    plans = {}
    for dest in cc.DESTS:
        (ni, nj, lo, la), (nx, ny, lo2, la2) = cc.grids(fg, dest)
        plans[dest] = fg.XgridPlan.create(1, [fg.GridConfig(ni, nj, lo, la)], fg.GridConfig(nx, ny, lo2, la2))
        plans[dest].finalize()
    recs = cc.records(5)
    recs.setflags(write=False)
    yield dict(ex=ex, plans=plans, recs=recs)
    for p in plans.values():
        p.destroy()
    ex.destroy()


def fixture(dest, vgrid, nrec=cc.NREC):
    fx = np.load(cc.golden_path(dest, vgrid))
    idx = [r % cc.NREC for r in range(nrec)]
    return fx["out"][idx], fx["iters"][idx]


def out_array(dest, vgrid, nrec, dtype=np.float64):
    nx, ny = cc.DESTS[dest]
    return np.full((nrec, cc.nk_out(vgrid), ny, nx), 77, dtype=dtype)


@pytest.mark.parametrize("dest,vgrid", cc.CASES)
def test_double_in_double_out_equals_the_reference_chain(fg, rig, dest, vgrid):
    sw = fg.ColumnSweep(rig["ex"], [rig["plans"][dest]], np.float64, np.float64, z_in=cc.Z1, z_out=cc.z_out(vgrid))
    try:
        assert sw.nk1 == cc.NK and sw.nk2 == cc.nk_out(vgrid)
        out = out_array(dest, vgrid, cc.NREC)
        iters, resmax = sw.run(rig["recs"][:cc.NREC], [out], missing=cc.MISSING, stop_crit=cc.STOP_CRIT)
        want, want_iters = fixture(dest, vgrid)
        print(dest, vgrid, "iters", iters.tolist(), "differing values", int(np.count_nonzero(out != want)))
        assert np.array_equal(iters, want_iters) and np.all(resmax <= cc.STOP_CRIT)
        assert same(out, want)
    finally:
        sw.destroy()


def dev_convert(fg, name, dtype, n, p_in, scale, offset, missing, p_out):
    fg._lib.check(getattr(fg.lib(), name)(C.c_int(fg.field_io.nc_type_of(dtype)), C.c_long(n), C.c_void_p(p_in), C.c_double(scale),
                                          C.c_double(offset), C.c_double(missing), C.c_void_p(p_out)))


def chain(fg, rig, dest, vgrid, raw, scale, offset, missing, out_dtype):
    """widen, Extrapolator.run per record, fg_plan_apply per level, do_vertical_interp, fg_dev_narrow -- the pinned calls"""
    import torch
    nx, ny = cc.DESTS[dest]
    plan, z2 = rig["plans"][dest], cc.z_out(vgrid)
    outs, its = [], []
    for rec in raw:
        t_raw = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
        wide = torch.empty(rec.shape, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dev_convert(fg, "fg_dev_widen", rec.dtype, rec.size, t_raw.data_ptr(), scale, offset, missing, wide.data_ptr())
        filled, it, _ = rig["ex"].run(wide, missing, cc.STOP_CRIT)
        mid = torch.empty((cc.NK, ny, nx), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for k in range(cc.NK):
            plan.apply(filled[k], mid[k], nz=1)
        plan.sync()
        lev = mid if z2 is None else fg.do_vertical_interp(cc.Z1, z2, mid)
        fin = torch.empty(lev.shape, dtype=getattr(torch, np.dtype(out_dtype).name), device="cuda")
        torch.cuda.synchronize()
        dev_convert(fg, "fg_dev_narrow", out_dtype, lev.numel(), lev.data_ptr(), scale, offset, missing, fin.data_ptr())
        outs.append(fin.cpu().numpy())
        its.append(it)
    return np.stack(outs), np.array(its)


def short_records(recs):
    """NC_SHORT with scale 2 and offset 100: the missing value -30000 is representable; in every record the valid cell (k, 40, 40)
    holds -15000, which lands exactly on `missing` after scaling -- the rule is `!= missing` BEFORE scaling, so it is scaled,
    then skips the offset (it equals missing by then) and is filled like a missing point"""
    raw = np.where(recs == cc.MISSING, -30000, np.rint(recs * 8.0)).astype(np.int16)
    assert np.all(raw[:, :, 40, 40] != -30000)
    raw[:, :, 40, 40] = -15000
    return raw


TYPED = {"float_float": (np.float32, np.float32, 0.0, 0.0, cc.MISSING), "short_float": (np.int16, np.float32, 2.0, 100.0, -30000.0),
         "double_float": (np.float64, np.float32, 0.0, 0.0, cc.MISSING)}


@pytest.mark.parametrize("path", list(TYPED))
@pytest.mark.parametrize("dest", list(cc.DESTS))
def test_typed_paths_equal_the_chain_of_pinned_calls(fg, rig, dest, path):
    in_dt, out_dt, scale, offset, missing = TYPED[path]
    recs = rig["recs"][:cc.NREC]
    raw = short_records(recs) if in_dt == np.int16 else recs.astype(in_dt)       # (-1e20 is a float: -1.00000002e20, not `missing`)
    if in_dt == np.float32:
        missing = float(np.float32(cc.MISSING))                                   # what the file's float attribute reads as
    want, want_iters = chain(fg, rig, dest, "7to9", raw, scale, offset, missing, out_dt)
    sw = fg.ColumnSweep(rig["ex"], [rig["plans"][dest]], in_dt, out_dt, z_in=cc.Z1, z_out=cc.z_out("7to9"))
    try:
        out = out_array(dest, "7to9", cc.NREC, out_dt)
        iters, _ = sw.run(raw, [out], scale=scale, offset=offset, missing=missing, stop_crit=cc.STOP_CRIT)
        print(dest, path, "iters", iters.tolist(), "differing values", int(np.count_nonzero(out != want)))
        assert np.array_equal(iters, want_iters)
        assert same(out, want) and np.all(np.isfinite(out)) and np.all(np.abs(out) < 1e4)
    finally:
        sw.destroy()


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page_locked"])
@pytest.mark.parametrize("nrec", [3, 5])
@pytest.mark.parametrize("per_chunk", [1, 2, 3])
def test_chunking_never_shows(fg, rig, per_chunk, nrec, pinned):
    """the last chunk is partial at (2, 3), (2, 5), (3, 5); records four and five are records one and two again, so a chunk's
    results do not depend on its neighbours"""
    dest, vgrid = "tripolar", "7to9"
    want, want_iters = fixture(dest, vgrid, nrec)
    bufs = []
    try:
        fg.set_column_records(per_chunk)
        sw = fg.ColumnSweep(rig["ex"], [rig["plans"][dest]], np.float64, np.float64, z_in=cc.Z1, z_out=cc.z_out(vgrid))
        if pinned:
            bufs = [fg.HostBuffer((nrec, cc.NK, cc.NJ, cc.NI), np.float64), fg.HostBuffer(want.shape, np.float64)]
            src, out = bufs[0].array, bufs[1].array
            src[:] = rig["recs"][:nrec]
            out[:] = 77
        else:
            src, out = rig["recs"][:nrec], out_array(dest, vgrid, nrec)
        iters, _ = sw.run(src, [out], missing=cc.MISSING, stop_crit=cc.STOP_CRIT)
        assert np.array_equal(iters, want_iters) and same(out, want)
        sw.destroy()
    finally:
        fg.set_column_records(0)
        for b in bufs:
            b.free()


def test_second_run_with_fewer_records_leaves_no_stale_state(fg, rig):
    dest, vgrid = "latlon", "7to9"
    sw = fg.ColumnSweep(rig["ex"], [rig["plans"][dest]], np.float64, np.float64, z_in=cc.Z1, z_out=cc.z_out(vgrid))
    try:
        for nrec, first in ((5, 0), (2, 1)):                                  # the second run: records two and three only
            out = out_array(dest, vgrid, nrec)
            iters, _ = sw.run(np.ascontiguousarray(rig["recs"][first:first + nrec]), [out], missing=cc.MISSING, stop_crit=cc.STOP_CRIT)
            want, want_iters = fixture(dest, vgrid, first + nrec)
            assert np.array_equal(iters, want_iters[first:]) and same(out, want[first:])
        # the extrapolator and the plan are their own again: the single-record entry still gives the reference's counts
        _, it, _ = rig["ex"].run(rig["recs"][0], cc.MISSING, cc.STOP_CRIT)
        assert np.array_equal(it, want_iters[0])
    finally:
        sw.destroy()


def test_two_plans_in_one_sweep(fg, rig):
    vgrid = "7to9"
    sw = fg.ColumnSweep(rig["ex"], [rig["plans"]["latlon"], rig["plans"]["tripolar"]], np.float64, np.float64, z_in=cc.Z1,
                        z_out=cc.z_out(vgrid))
    try:
        fg.set_column_records(2)
        outs = [out_array(d, vgrid, cc.NREC) for d in ("latlon", "tripolar")]
        iters, _ = sw.run(rig["recs"][:cc.NREC], outs, missing=cc.MISSING, stop_crit=cc.STOP_CRIT)
        for d, out in zip(("latlon", "tripolar"), outs):
            want, want_iters = fixture(d, vgrid)
            assert np.array_equal(iters, want_iters) and same(out, want), d
    finally:
        fg.set_column_records(0)
        sw.destroy()


def test_bad_arguments_and_fatal_levels(fg, rig):
    plan = rig["plans"]["latlon"]
    z1 = cc.Z1.copy()
    z1[3] = z1[2]
    with pytest.raises(fg.FregridHipError, match="grid1 not monotonic") as e:
        fg.ColumnSweep(rig["ex"], [plan], np.float64, np.float64, z_in=z1, z_out=cc.z_out("7to9"))
    assert e.value.code == -7
    z2 = cc.z_out("7to9").copy()
    z2[4] = z2[3]
    with pytest.raises(fg.FregridHipError, match="grid2 not monotonic"):
        fg.ColumnSweep(rig["ex"], [plan], np.float64, np.float64, z_in=cc.Z1, z_out=z2)
    lon, lat = cc.source_axes()
    with fg.Extrapolator(lon[:60], lat[:40], 0) as other:                     # not the plans' source grid
        with pytest.raises(fg.FregridHipError) as e:
            fg.ColumnSweep(other, [plan], np.float64, np.float64, z_in=cc.Z1)
        assert e.value.code == -1
