"""fg_sweep (csrc/sweep.hip): levels streamed from host memory, in the file's type, through the plans and back must equal the
resident sweep bit for bit -- get_input_data's widening / scale / offset (fregrid_util.c:2097-2123) and write_field_data's
inverse (:2376-2406) included -- for page-locked and pageable host arrays, several chunks, order 1 and order 2.
Further down the same pipeline is held against an all-CPU reference (numpy conversions, CPU oracle) at unaligned sizes, level
counts that reuse the buffer slots and every file type, and fg_dev_widen / fg_dev_narrow against numpy alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import gridutil
import orc
from test_gpu_c2l import oracle_prepare

pytestmark = pytest.mark.gpu


def _widen(a, scale, offset, missing):
    v = a.astype(np.float64)
    if scale != 0:
        v = np.where(v != missing, v * scale, v)
    if offset != 0:
        v = np.where(v != missing, v + offset, v)
    return v


def _narrow(v, scale, offset, missing, dtype):
    v = v.copy()
    if offset != 0:
        v = np.where(v != missing, v - offset, v)
    if scale != 0:
        v = np.where(v != missing, v / scale, v)
    return v.astype(dtype)


@pytest.mark.parametrize("pinned", [True, False])
def test_streamed_order2_equals_resident(fg, gpu_ok, pinned):
    ni, nlon, nlat, nlev = 32, 96, 48, 19                        # 19 levels: chunks of 8 + 8 + 3
    lon, lat, lont, latt = fg.gnomonic_ed_grid(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    plan = fg.XgridPlan.create(2, [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)], fg.GridConfig(nlon, nlat, lo, la))
    plan.finalize()
    prep = fg.C2lPrep([ni] * 6, [ni] * 6, lon, lat, lont, latt, fg.find_contacts([ni] * 6, [ni] * 6, lon, lat))
    ncell = 6 * ni * ni
    rng = np.random.default_rng(7)
    src = (280.0 + 20.0 * rng.standard_normal((nlev, ncell))).astype(np.float32)
    scale, offset, missing = 0.5, 3.25, -1.0e10
    # resident reference: widen on the host exactly as get_input_data, records + sweep per chunk, narrow as write_field_data
    f64 = _widen(src, scale, offset, missing)
    ref = np.empty((nlev, nlon * nlat), dtype=np.float32)
    dev = "cuda:0"
    for l0 in range(0, nlev, 8):
        nl = min(8, nlev - l0)
        s_t = torch.from_numpy(np.ascontiguousarray(f64[l0:l0 + nl])).to(dev)
        rec = torch.empty(ncell, 3, fg.C2lPrep.records_nb(nl), dtype=torch.float64, device=dev)
        out = torch.empty(nl, nlon * nlat, dtype=torch.float64, device=dev)
        prep.records(s_t, nl, rec); prep.sync()
        plan.apply_records(nl, rec, out); plan.sync()
        ref[l0:l0 + nl] = _narrow(out.cpu().numpy(), scale, offset, missing, np.float32)
    # streamed
    sw = fg.Sweep([plan], prep, np.float32, np.float32)
    if pinned:
        hin = fg.HostBuffer((nlev, ncell), np.float32); hout = fg.HostBuffer((nlev, nlon * nlat), np.float32)
        hin.array[:] = src
        a_in, a_out = hin.array, hout.array
    else:
        a_in, a_out = src.copy(), np.empty((nlev, nlon * nlat), dtype=np.float32)
    a_out[:] = np.nan
    sw.run(a_in, [a_out], scale=scale, offset=offset, missing=missing)
    assert np.array_equal(a_out.view(np.uint32), ref.view(np.uint32))
    sw.run(a_in, [a_out], scale=scale, offset=offset, missing=missing)       # the object is reusable
    assert np.array_equal(a_out.view(np.uint32), ref.view(np.uint32))
    sw.destroy()
    if pinned:
        hin.free(); hout.free()
    plan.destroy()


def test_streamed_order1_two_output_tiles_short_input(fg, gpu_ok):
    """conserve_order1, NC_SHORT input (packed field), two output tiles sharing one upload, double output, 11 levels."""
    ni, nlev = 24, 11
    lon, lat = fg.gnomonic_ed_corners(ni)
    gin = [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]
    outs_g = []
    for (x0, x1, y0, y1, nx, ny) in ((0.0, 180.0, -90.0, 90.0, 40, 36), (180.0, 360.0, -90.0, 90.0, 30, 20)):
        lo, la = fg.latlon_corners(nx, ny, x0, x1, y0, y1)
        outs_g.append((nx, ny, lo, la))
    plans = []
    for (nx, ny, lo, la) in outs_g:
        p = fg.XgridPlan.create(1, gin, fg.GridConfig(nx, ny, lo, la)); p.finalize(); plans.append(p)
    ncell = 6 * ni * ni
    rng = np.random.default_rng(3)
    src = rng.integers(-20000, 20000, size=(nlev, ncell)).astype(np.int16)
    scale, offset, missing = 0.01, 273.15, -32768.0
    f64 = _widen(src, scale, offset, missing)
    dev = "cuda:0"
    refs = []
    for p, (nx, ny, _, _) in zip(plans, outs_g):
        r = np.empty((nlev, nx * ny))
        for l0 in range(0, nlev, 8):
            nl = min(8, nlev - l0)
            s_t = torch.from_numpy(np.ascontiguousarray(f64[l0:l0 + nl])).to(dev)
            out = torch.empty(nl, nx * ny, dtype=torch.float64, device=dev)
            p.apply(s_t, out, nz=nl); p.sync()
            r[l0:l0 + nl] = out.cpu().numpy()
        refs.append(r)
    sw = fg.Sweep(plans, None, np.int16, np.float64)
    got = [np.empty_like(r) for r in refs]
    sw.run(src, got, scale=scale, offset=offset, missing=missing)
    for g, r in zip(got, refs):
        rr = _narrow(r, scale, offset, missing, np.float64)                  # out type double still undoes offset and scale
        assert np.array_equal(g.view(np.uint64), rr.view(np.uint64))
    sw.destroy()
    for p in plans:
        p.destroy()


def test_two_sweeps_share_plans_and_any_destruction_order(fg, gpu_ok):
    """fregrid needs one fg_sweep per pair of file types.  Two live sweeps over the same plan and gradient object,
    runs interleaved with a direct use of the plan, the plan destroyed BEFORE the sweeps: each run borrows the compute stream
    for its own duration only, results stay bit-identical and nothing touches a freed plan."""
    ni, nlon, nlat, nlev = 24, 72, 36, 10
    lon, lat, lont, latt = fg.gnomonic_ed_grid(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    plan = fg.XgridPlan.create(2, [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)], fg.GridConfig(nlon, nlat, lo, la))
    plan.finalize()
    prep = fg.C2lPrep([ni] * 6, [ni] * 6, lon, lat, lont, latt, fg.find_contacts([ni] * 6, [ni] * 6, lon, lat))
    ncell = 6 * ni * ni
    rng = np.random.default_rng(3)
    src32 = (280.0 + 20.0 * rng.standard_normal((nlev, ncell))).astype(np.float32)
    src64 = src32.astype(np.float64)
    sw_f = fg.Sweep([plan], prep, np.float32, np.float32)
    sw_d = fg.Sweep([plan], prep, np.float64, np.float64)
    out_f = [np.empty((nlev, nlon * nlat), dtype=np.float32) for _ in range(2)]
    out_d = [np.empty((nlev, nlon * nlat), dtype=np.float64) for _ in range(2)]
    sw_f.run(src32, [out_f[0]])
    sw_d.run(src64, [out_d[0]])
    # the plan used directly in between (its own stream again)
    dev = "cuda:0"
    rec = torch.empty(ncell, 3, fg.C2lPrep.records_nb(8), dtype=torch.float64, device=dev)
    o8 = torch.empty(8, nlon * nlat, dtype=torch.float64, device=dev)
    prep.records(torch.from_numpy(src64[:8].copy()).to(dev), 8, rec); prep.sync()
    plan.apply_records(8, rec, o8); plan.sync()
    assert np.array_equal(o8.cpu().numpy().view(np.uint64), out_d[0][:8].view(np.uint64))
    sw_d.run(src64, [out_d[1]])
    sw_f.run(src32, [out_f[1]])
    assert np.array_equal(out_d[0].view(np.uint64), out_d[1].view(np.uint64))
    assert np.array_equal(out_f[0].view(np.uint32), out_f[1].view(np.uint32))
    assert np.array_equal(out_d[0].astype(np.float32).view(np.uint32), out_f[0].view(np.uint32))     # float levels are exact in double
    plan.destroy()                                              # before its sweeps
    sw_f.destroy(); sw_d.destroy()


# ------------------------------------------------------------------------------------------------------------------------
# The pipeline against an all-CPU reference: numpy _widen -> (oracle_prepare, order 2) -> orc.orc_apply per chunk of <= 8
# levels -> numpy _narrow, on small unaligned mosaics (C10: 600 cells, C9: 486) and a 30 x 15 target.  The plans hold the
# ORACLE's exchange cells (XgridPlan.create_empty + set_xgrid from orc.orc_setup; fg_sweep_create takes such a plan), so the
# streamed result must equal the reference bit for bit.
NLON, NLAT = 30, 15
FG_ERR_ARG = -1


@pytest.fixture(scope="module")
def cases(fg, gpu_ok):
    """(mosaic name, order) -> dict(m, o, plan, prep), built on first use, destroyed with the module"""
    made = {}

    def get(name, order):
        if (name, order) not in made:
            m = gridutil.c2l_mosaic(fg, name)
            nx, ny = m["nx"], m["ny"]
            lo, la = fg.latlon_corners(NLON, NLAT)
            o = orc.orc_setup(order, [(nx[t], ny[t], m["lon"][t], m["lat"][t]) for t in range(len(nx))], [(NLON, NLAT, lo, la)])
            plan = fg.XgridPlan.create_empty(order, nx, ny, NLON, NLAT)
            plan.set_xgrid(o["t_in"], o["i_in"], o["j_in"], o["i_out"], o["j_out"], o["area"], o.get("di"), o.get("dj"))
            prep = fg.C2lPrep(nx, ny, m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"]) if order == 2 else None
            made[(name, order)] = dict(m=m, o=o, plan=plan, prep=prep, order=order, ncell=sum(a * b for a, b in zip(nx, ny)))
        return made[(name, order)]
    yield get
    for c in made.values():
        if c["prep"] is not None:
            c["prep"].destroy()
        c["plan"].destroy()


def _cpu_remap(fg, c, f64):
    """widened levels [nlev][ncell] -> remapped levels [nlev][NLON * NLAT], the way the device chunks them"""
    m, o, order = c["m"], c["o"], c["order"]
    nx, ny = m["nx"], m["ny"]
    offs = np.concatenate([[0], np.cumsum([a * b for a, b in zip(nx, ny)])])
    nlev = f64.shape[0]
    res = np.empty((nlev, NLON * NLAT))
    for l0 in range(0, nlev, 8):
        nl = min(8, nlev - l0)
        tiles = [np.ascontiguousarray(f64[l0:l0 + nl, offs[t]:offs[t + 1]]).reshape(nl, ny[t], nx[t]) for t in range(len(nx))]
        if order == 2:
            d, gx, gy, _, _, _ = oracle_prepare(fg, (nx, ny), m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"], tiles, nl)
            r, _ = orc.orc_apply(2, o, nx, ny, [a.reshape(nl, -1) for a in d], gx, gy, None, False, 0.0, NLON, NLAT, nl)
        else:
            r, _ = orc.orc_apply(1, o, nx, ny, [a.reshape(nl, -1) for a in tiles], None, None, None, False, 0.0, NLON, NLAT, nl)
        res[l0:l0 + nl] = r.reshape(nl, -1)
    return res


def _narrow_in_range(v, scale, offset, missing, dtype):
    """_narrow, after asserting that every value lies inside the output type's range (beyond it the cast is unpinned)"""
    w = _narrow(v, scale, offset, missing, np.float64)
    assert np.all(np.isfinite(w))
    if w.size == 0:
        return w.astype(dtype)
    if np.issubdtype(np.dtype(dtype), np.integer):
        info = np.iinfo(dtype)
        assert w.min() > info.min and w.max() < info.max, (w.min(), w.max())
    else:
        assert np.abs(w).max() < np.finfo(dtype).max
    return _narrow(v, scale, offset, missing, dtype)


def _view(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _fill(a):
    """pre-fill an output array with something no run writes: NaN, or a bit pattern for the integer types"""
    a[...] = np.nan if a.dtype.kind == "f" else -21555


def _run_and_compare(fg, sw, src, ref, scale, offset, missing, pin_in=False, pin_out=False, runs=2):
    bufs = []
    if pin_in:
        hb = fg.HostBuffer(src.shape, src.dtype); hb.array[:] = src; a_in = hb.array; bufs.append(hb)
    else:
        a_in = src.copy()
    if pin_out:
        hb = fg.HostBuffer(ref.shape, ref.dtype); a_out = hb.array; bufs.append(hb)
    else:
        a_out = np.empty(ref.shape, dtype=ref.dtype)
    for _ in range(runs):                                             # the object is reusable
        _fill(a_out)
        sw.run(a_in, [a_out], scale=scale, offset=offset, missing=missing)
        bad = np.nonzero(np.any(_view(a_out) != _view(ref), axis=1))[0]
        assert bad.size == 0, f"levels that differ: {bad.tolist()}"
    a_out = a_in = None
    for hb in bufs:
        hb.free()


def _levels(rng, nlev, ncell):
    """every level carries its own offset: a chunk that lands on another chunk's levels shows up"""
    return (280.0 + 20.0 * rng.standard_normal((nlev, ncell)) + 100.0 * np.arange(nlev)[:, None]).astype(np.float32)


@pytest.mark.parametrize("nlev,pin_in,pin_out", [(1, False, False), (7, False, False), (8, False, False), (9, False, False),
                                                 (24, False, False), (25, False, False), (41, False, False), (41, True, False),
                                                 (41, False, True), (41, True, True)])
def test_streamed_order1_level_counts_and_slot_reuse(fg, cases, nlev, pin_in, pin_out):
    """Less than a chunk, exactly one, exactly NSLOT = 3 chunks (24), the first reuse of a slot (25) and the second (41: six
    chunks and a level), page-locked and pageable host arrays mixed: the in-loop slot_retire hands an older chunk's staged
    outputs to its own levels while the compute stream already overwrites the shared buffers."""
    c = cases("c10", 1)
    src = _levels(np.random.default_rng(nlev), nlev, c["ncell"])
    scale, offset, missing = 0.5, 3.25, -1.0e10
    ref = _narrow_in_range(_cpu_remap(fg, c, _widen(src, scale, offset, missing)), scale, offset, missing, np.float32)
    sw = fg.Sweep([c["plan"]], None, np.float32, np.float32)
    _run_and_compare(fg, sw, src, ref, scale, offset, missing, pin_in, pin_out)
    sw.destroy()


def test_streamed_order2_slot_reuse_c9(fg, cases):
    """conserve_order2 on C9 (486 cells: both passes of the record store are short), 27 levels = four chunks: d_rec is
    rewritten while the first chunk's download may still be in flight."""
    c = cases("c9", 2)
    nlev = 27
    src = _levels(np.random.default_rng(27), nlev, c["ncell"])
    ref = _narrow_in_range(_cpu_remap(fg, c, _widen(src, 0.0, 0.0, -1.0e10)), 0.0, 0.0, -1.0e10, np.float32)
    sw = fg.Sweep([c["plan"]], c["prep"], np.float32, np.float32)
    _run_and_compare(fg, sw, src, ref, 0.0, 0.0, -1.0e10)
    sw.destroy()


def _typed_source(rng, dtype, nlev, ncell):
    lev = 37 * np.arange(nlev)[:, None]
    if np.dtype(dtype).kind == "i":
        return (rng.integers(-20000, 20000, size=(nlev, ncell)) + lev).astype(dtype)
    return (1000.0 * rng.standard_normal((nlev, ncell)).clip(-3, 3) + lev).astype(dtype)


@pytest.mark.parametrize("in_dtype,out_dtype,scale,offset,nlev", [
    (np.int32, np.int32, 0.01, 273.15, 9),            # k_widen<int32_t>, k_narrow<int32_t>
    (np.float64, np.int16, 0.01, 280.0, 9),           # a packed NC_SHORT output: k_narrow<int16_t>
    (np.int16, np.float32, 0.01, 273.15, 9),
    (np.float64, np.float64, 0.0, 0.0, 25),           # neither kernel runs: the sweep reads d_raw and writes d_fin, slots reused
])
def test_streamed_types(fg, cases, in_dtype, out_dtype, scale, offset, nlev):
    c = cases("c10", 1)
    missing = -1.0e10
    src = _typed_source(np.random.default_rng(nlev + np.dtype(in_dtype).itemsize), in_dtype, nlev, c["ncell"])
    ref = _narrow_in_range(_cpu_remap(fg, c, _widen(src, scale, offset, missing)), scale, offset, missing, out_dtype)
    sw = fg.Sweep([c["plan"]], None, in_dtype, out_dtype)
    _run_and_compare(fg, sw, src, ref, scale, offset, missing)
    sw.destroy()


@pytest.mark.parametrize("in_dtype,out_dtype,scale,offset,missing,quirk", [
    (np.float32, np.float32, 0.5, 3.25, 50.0, 100),          # raw 100 * 0.5 == missing: stays 50.0, gets no offset
    (np.int32, np.float64, 0.5, 3.25, 50.0, 100),
    (np.int16, np.float64, 0.01, 273.15, -32768.0, None),    # a packed variable's usual marker
])
def test_streamed_inputs_that_contain_the_missing_value(fg, cases, in_dtype, out_dtype, scale, offset, missing, quirk):
    """The `!= missing` guards of the conversions, including the reference's quirk that the offset guard looks at the already
    scaled value (fregrid_util.c:2117-2124).  The remap treats every value as data, as documented for the streamed sweep,
    and so does the reference pipeline here."""
    c = cases("c10", 1)
    nlev = 9
    rng = np.random.default_rng(99)
    src = _typed_source(rng, in_dtype, nlev, c["ncell"])
    src[:, ::7] = missing
    src[1::2, 3::11] = missing
    if quirk is not None:
        src[:, 5::13] = quirk
    f64 = _widen(src, scale, offset, missing)
    assert np.any(src == missing) and np.all(f64[src == missing] == missing)
    if quirk is not None:
        assert np.all(f64[src == quirk] == missing)
    ref = _narrow_in_range(_cpu_remap(fg, c, f64), scale, offset, missing, out_dtype)
    sw = fg.Sweep([c["plan"]], None, in_dtype, out_dtype)
    _run_and_compare(fg, sw, src, ref, scale, offset, missing)
    sw.destroy()


def test_argument_error_leaves_the_sweep_usable(fg, cases):
    """include/fregrid_hip.h: "After an error return the object is clean and may be run again".  nlev = 0 and a null output
    array are refused with FG_ERR_ARG; the next valid run gives the bits of the first."""
    c = cases("c9", 2)
    nlev = 11
    src = _levels(np.random.default_rng(11), nlev, c["ncell"])
    ref = _narrow_in_range(_cpu_remap(fg, c, _widen(src, 0.5, 3.25, -1.0e10)), 0.5, 3.25, -1.0e10, np.float32)
    sw = fg.Sweep([c["plan"]], c["prep"], np.float32, np.float32)
    _run_and_compare(fg, sw, src, ref, 0.5, 3.25, -1.0e10, runs=1)
    out = np.full(ref.shape, np.nan, dtype=np.float32)
    run = fg.lib().fg_sweep_run
    p_in = src.ctypes.data_as(C.c_void_p)
    assert run(sw._h, p_in, 0, 0.5, 3.25, -1.0e10, (C.c_void_p * 1)(out.ctypes.data)) == FG_ERR_ARG
    assert run(sw._h, p_in, nlev, 0.5, 3.25, -1.0e10, (C.c_void_p * 1)(None)) == FG_ERR_ARG
    assert np.all(np.isnan(out))
    _run_and_compare(fg, sw, src, ref, 0.5, 3.25, -1.0e10, runs=1)
    sw.destroy()


# ------------------------------------------------------------------------------------------------------------------------
# fg_dev_widen / fg_dev_narrow alone, on device tensors, against the numpy restatement above
_TORCH = {np.int16: torch.int16, np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}
_SIZES = (0, 1, 255, 256, 257, 100003)
_SCALE_OFFSET = ((0.0, 0.0), (0.5, 0.0), (0.0, 3.25), (0.5, 3.25))
_MISSING = 50.0


def _dev_convert(fg, name, dtype, n, p_in, scale, offset, p_out):
    f = getattr(fg.lib(), name)
    return f(C.c_int(fg.field_io.nc_type_of(dtype)), C.c_long(n), C.c_void_p(p_in), C.c_double(scale), C.c_double(offset),
             C.c_double(_MISSING), C.c_void_p(p_out))


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32, np.float64])
def test_dev_widen_against_numpy(fg, gpu_ok, dtype):
    dev = "cuda:0"
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    for n in _SIZES:
        raw = rng.integers(-2000, 2000, size=n).astype(dtype) if np.dtype(dtype).kind == "i" else (100.0 * rng.standard_normal(n)).astype(dtype)
        raw[:1] = 100                               # 100 * 0.5 == missing: no offset
        raw[n // 2:n // 2 + 1] = 50 if n > 1 else 100
        raw[7::31] = 50                             # the missing value itself
        raw[11::37] = 100
        for scale, offset in _SCALE_OFFSET:
            ref = _widen(raw, scale, offset, _MISSING)
            if n > 0 and scale == 0.5 and offset != 0:
                assert ref[0] == _MISSING
            t_in = torch.from_numpy(raw.copy()).to(dev)
            t_out = torch.full((n + 1,), -12345.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            assert _dev_convert(fg, "fg_dev_widen", dtype, n, t_in.data_ptr(), scale, offset, t_out.data_ptr()) == 0
            got = t_out.cpu().numpy()
            assert got[n] == -12345.0, (n, scale, offset)                      # nothing written past n
            assert np.array_equal(got[:n].view(np.uint64), ref.view(np.uint64)), (n, scale, offset)


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32, np.float64])
def test_dev_narrow_against_numpy(fg, gpu_ok, dtype):
    dev = "cuda:0"
    rng = np.random.default_rng(10 + np.dtype(dtype).itemsize)
    for n in _SIZES:
        for scale, offset in _SCALE_OFFSET:
            # values a widened field would hold: raw * scale + offset for raw within +-2000, so the narrowed ones are in range
            v = _widen(2000.0 * rng.uniform(-1, 1, size=n), scale, offset, _MISSING)
            v[:1] = _MISSING + offset               # equals missing once the offset is gone: not divided by scale
            v[n // 2:n // 2 + 1] = _MISSING if n > 1 else _MISSING + offset
            v[7::31] = _MISSING
            v[11::37] = _MISSING + offset
            ref = _narrow_in_range(v, scale, offset, _MISSING, dtype)
            if n > 0 and scale != 0:
                assert ref[0] == 50
            t_in = torch.from_numpy(v.copy()).to(dev)
            t_out = torch.full((n + 1,), -123, dtype=_TORCH[dtype], device=dev)
            torch.cuda.synchronize()
            assert _dev_convert(fg, "fg_dev_narrow", dtype, n, t_in.data_ptr(), scale, offset, t_out.data_ptr()) == 0
            got = t_out.cpu().numpy()
            assert got[n] == -123, (n, scale, offset)
            assert np.array_equal(_view(got[:n]), _view(ref)), (n, scale, offset)


def test_dev_convert_refuses_bad_arguments(fg, gpu_ok):
    t = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    for name in ("fg_dev_widen", "fg_dev_narrow"):
        f = getattr(fg.lib(), name)
        args = lambda nc, n, a, b: (C.c_int(nc), C.c_long(n), C.c_void_p(a), C.c_double(0.0), C.c_double(0.0), C.c_double(0.0), C.c_void_p(b))
        assert f(*args(fg.field_io.nc_type_of(np.float64), -1, t.data_ptr(), t.data_ptr())) == FG_ERR_ARG
        assert f(*args(fg.field_io.nc_type_of(np.float64), 4, 0, t.data_ptr())) == FG_ERR_ARG
        assert f(*args(0, 4, t.data_ptr(), t.data_ptr())) == FG_ERR_ARG
    assert np.all(t.cpu().numpy() == 0.0)
