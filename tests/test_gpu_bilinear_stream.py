"""fg_bilin_sweep (csrc/bilinear.hip, field_io.BilinearSweep): levels of a cubed-sphere variable streamed from host memory in
the file's type through a bilinear plan and back, scalar and vector.

1. Against the reference's own bilinear_interp.c (oracle/_ref/libbilinear_ref.so) with the plan built from the reference's
   index / weight: streamed == narrow(bref_apply_*(halo(widen(level)))) as raw bits, widen / narrow restated in numpy.
2. Against the resident path with the device's own search: streamed == fg_dev_widen -> apply(nz = 1) -> fg_dev_narrow per
   level, for level counts around the chunk and slot sizes and for page-locked / pageable host arrays.
3. Halo corners: the zero of a halo corner is not offset.
4. Object hygiene: shared plans, destruction order, argument errors, the plan's stream.

Integer outputs: the values and the missing value are chosen so that every narrowed value lies inside the output type's range
(_narrow_in_range asserts it); beyond it the cast is parity-unpinned, as documented for fg_sweep."""
import ctypes as C
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import orc
from test_gpu_bilinear_vs_ref import COMBOS, VARIANTS, _case, _corner_window, cfg_of, device_plan, grid, levels
from test_gpu_sweep_stream import _fill, _narrow_in_range, _view, _widen

pytestmark = pytest.mark.gpu
FG_ERR_ARG = -1

CASES = [
    _case("c24_72x37_fs0", 24, 72, 37),
    _case("c24_72x37_fs1", 24, 72, 37, 1),              # fine 144 x 73
    _case("c24_36x19_fs2", 24, 36, 19, 2),
    _case("c25_72x37_fs0", 25, 72, 37),                 # 3750 cells: int16 / float levels start unaligned, npts % 64 != 0
]
CORNER = [_case("c24_corner_window", 24, 48, 49, corner=True), _case("c48_corner_window", 48, 48, 49, corner=True)]
IDS = [c["name"] for c in CASES]
BYNAME = {c["name"]: c for c in CASES + CORNER}

# in / out file types; (scale, offset) of u (and of a scalar) and of v; the missing value as the file type holds it; the factor
# that turns levels()'s fields (|s|, |u|, |v| < 30) into raw values of the input type
PAIRS = {
    "f32_f32": dict(i=np.float32, o=np.float32, cu=(0.0, 0.0), cv=(0.0, 0.0), miss=float(np.float32(-1.0e20)), k=1.0),
    "i16_f32": dict(i=np.int16, o=np.float32, cu=(0.01, 273.15), cv=(0.02, -10.0), miss=-32768.0, k=100.0),
    "f64_f64": dict(i=np.float64, o=np.float64, cu=(0.0, 0.0), cv=(0.0, 0.0), miss=-1.0e20, k=1.0),
    # int16 output: |raw| < 1200, missing -20000; without has_missing a vector level of missing u and v rotates to at most
    # sqrt(2) * 20000 = 28285, and the narrowing divides by 2 and 4: inside +-32767
    "i32_i16": dict(i=np.int32, o=np.int16, cu=(2.0, -5.0), cv=(4.0, 3.0), miss=-20000.0, k=40.0),
}


@pytest.fixture(scope="module")
def fg():
    import __graft_entry__
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    return fg


@pytest.fixture(scope="module")
def refs(fg):
    """the reference's setup of every case, in child processes, all at once: name -> (setup or None, fell_back, printed)"""
    if not orc.bilinear_ref_available():
        pytest.fail("oracle/_ref/libbilinear_ref.so is missing: build() makes it where the reference exists")
    for N in sorted({c["N"] for c in CASES + CORNER}):
        grid(fg, N)
    tmp = tempfile.mkdtemp(prefix="bls_")

    def run(case):
        wd = os.path.join(tmp, case["name"])
        os.makedirs(wd)
        g = grid(fg, case["N"])
        r, printed, fell_back = orc.bref_setup_child(cfg_of(case), g[3], g[4], wd, timeout=300)
        return case["name"], (r, fell_back, printed)
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        return dict(ex.map(run, CASES + CORNER))


def raw_levels(fg, case, pair, nlev=4):
    """nlev levels of s, u, v in the input type [nlev, 6*N*N] and their missing masks, levels()'s four patterns repeating: none;
    every 37th cell; 3 x 3 blocks; all but one tile.  Every level carries its own shift, so a level that lands on another
    level's place shows up."""
    N = case["N"]
    _, lont, latt = grid(fg, N)[:3]
    s, u, v, mask = levels(case, lont, latt)
    rep = [k % 4 for k in range(nlev)]
    shift = (0.25 * (np.arange(nlev) // 4))[:, None]
    out = []
    for f in (s, u, v):
        x = (f[rep].reshape(nlev, -1) + shift) * pair["k"]
        out.append((np.rint(x) if np.dtype(pair["i"]).kind == "i" else x).astype(pair["i"]))
    return out[0], out[1], out[2], mask[rep].reshape(nlev, -1)


def masked(raw, mask, pair):
    a = raw.copy()
    a[mask] = pair["miss"]
    return a


def ref_scalar(fg, case, r, pair, raw, hm, fm):
    cfg, halo = cfg_of(case), grid(fg, case["N"])[5]
    sc, of = pair["cu"]
    w = _widen(raw, sc, of, pair["miss"])
    res = np.stack([orc.bref_apply_scalar(cfg, r, halo(w[k]), hm, pair["miss"], fm) for k in range(len(w))])
    return _narrow_in_range(res, sc, of, pair["miss"], pair["o"])


def ref_vector(fg, case, r, pair, ru, rv, hm, fm):
    g = grid(fg, case["N"])
    cfg, halo, vi, wi = cfg_of(case), g[5], g[6], g[7]
    uw, vw = _widen(ru, *pair["cu"], pair["miss"]), _widen(rv, *pair["cv"], pair["miss"])
    res = [orc.bref_apply_vector(cfg, r, vi, wi, halo(uw[k]), halo(vw[k]), hm, pair["miss"], fm) for k in range(len(uw))]
    return (_narrow_in_range(np.stack([a for a, _ in res]), *pair["cu"], pair["miss"], pair["o"]),
            _narrow_in_range(np.stack([b for _, b in res]), *pair["cv"], pair["miss"], pair["o"]))


def same_bits(got, ref, what):
    bad = np.nonzero(np.any(_view(got).reshape(len(ref), -1) != _view(ref).reshape(len(ref), -1), axis=1))[0]
    assert bad.size == 0, (what, f"levels that differ: {bad.tolist()}",
                           int(np.sum(_view(got).reshape(-1) != _view(ref).reshape(-1))))


def host(fg, shape, dtype, pinned, keep, fill_from=None):
    """a page-locked (HostBuffer) or pageable array; the buffers made are appended to keep for the caller to free"""
    if pinned:
        hb = fg.HostBuffer(shape, dtype); keep.append(hb); a = hb.array
    else:
        a = np.empty(shape, dtype=dtype)
    if fill_from is not None:
        a[...] = fill_from
    else:
        _fill(a)
    return a


def stream_scalar(fg, sw, case, pair, raw, hm, fm, pin_in=False, pin_out=False):
    keep = []
    a = host(fg, raw.shape, pair["i"], pin_in, keep, raw)
    o = host(fg, (len(raw), case["nlat"], case["nlon"]), pair["o"], pin_out, keep)
    sw.run_scalar(a, o, scale=pair["cu"][0], offset=pair["cu"][1], missing=pair["miss"], has_missing=hm, fill_missing=fm)
    got = o.copy()
    a = o = None
    for hb in keep:
        hb.free()
    return got


def stream_vector(fg, sw, case, pair, ru, rv, hm, fm, pin_in=False, pin_out=False):
    keep = []
    a, b = host(fg, ru.shape, pair["i"], pin_in, keep, ru), host(fg, rv.shape, pair["i"], pin_in, keep, rv)
    shape = (len(ru), case["nlat"], case["nlon"])
    o, p = host(fg, shape, pair["o"], pin_out, keep), host(fg, shape, pair["o"], pin_out, keep)
    sw.run_vector(a, b, o, p, conv_u=(*pair["cu"], pair["miss"]), conv_v=(*pair["cv"], pair["miss"]), has_missing=hm, fill_missing=fm)
    got = o.copy(), p.copy()
    a = b = o = p = None
    for hb in keep:
        hb.free()
    return got


# ------------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("pname", list(PAIRS))
@pytest.mark.parametrize("name", IDS)
def test_streamed_equals_reference(fg, refs, name, pname):
    """the plan read from the reference's index / weight (that configuration is bit for bit): every
    (has_missing, fill_missing), the four missing patterns, in u, in v and in both"""
    case, pair = BYNAME[name], PAIRS[pname]
    r, fell_back, printed = refs[name]
    assert not fell_back and r is not None and "global sweep" not in printed, printed[-300:]
    rs, ru, rv, mask = raw_levels(fg, case, pair)
    sm, um, vm = masked(rs, mask, pair), masked(ru, mask, pair), masked(rv, mask, pair)
    with device_plan(fg, case, index=r["index"], weight=r["weight"]) as p:
        sw = p.sweep(pair["i"], pair["o"])
        for hm, fm in COMBOS:
            same_bits(stream_scalar(fg, sw, case, pair, sm, hm, fm), ref_scalar(fg, case, r, pair, sm, hm, fm), ("s", hm, fm))
            for var in VARIANTS:
                a, b = (um if "u" in var else ru), (vm if "v" in var else rv)
                gu, gv = stream_vector(fg, sw, case, pair, a, b, hm, fm)
                wu, wv = ref_vector(fg, case, r, pair, a, b, hm, fm)
                same_bits(gu, wu, ("u", var, hm, fm))
                same_bits(gv, wv, ("v", var, hm, fm))
        sw.destroy()


# ------------------------------------------------------------------------------------------------------------------------ 2
def _dev_convert(fg, name, dtype, n, p_in, conv, missing, p_out):
    rc = getattr(fg.lib(), name)(C.c_int(fg.field_io.nc_type_of(dtype)), C.c_long(n), C.c_void_p(p_in), C.c_double(conv[0]),
                                 C.c_double(conv[1]), C.c_double(missing), C.c_void_p(p_out))
    assert rc == 0, fg._lib.last_error()


_NP2T = {np.int16: torch.int16, np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}


def chain(fg, plan, pair, raws, convs, hm, fm):
    """the per-level chain on one level: fg_dev_widen -> apply_scalar / apply_vector(nz = 1) -> fg_dev_narrow"""
    dev, n, miss = "cuda:0", raws[0].size, pair["miss"]
    wide = []
    for raw, cv in zip(raws, convs):
        t_raw = torch.from_numpy(np.ascontiguousarray(raw)).to(dev)
        t = torch.empty(1, n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        _dev_convert(fg, "fg_dev_widen", pair["i"], n, t_raw.data_ptr(), cv, miss, t.data_ptr())
        wide.append(t)
    res = [plan.apply_scalar(wide[0], hm, miss, fm)] if len(raws) == 1 else list(plan.apply_vector(wide[0], wide[1], hm, miss, fm))
    plan.sync()
    out = []
    for t, cv in zip(res, convs):
        o = torch.empty(t.numel(), dtype=_NP2T[pair["o"]], device=dev)
        torch.cuda.synchronize()
        _dev_convert(fg, "fg_dev_narrow", pair["o"], t.numel(), t.data_ptr(), cv, miss, o.data_ptr())
        out.append(o.cpu().numpy())
    return out


_OWN = {}


def own_plan(fg, name):
    """the device's own search (fg_bilin_create), one plan per case for the module"""
    if name not in _OWN:
        _OWN[name] = device_plan(fg, BYNAME[name])
    return _OWN[name]


@pytest.fixture(scope="module", autouse=True)
def _own_plans_go():
    yield
    for p in _OWN.values():
        p.destroy()
    _OWN.clear()


# every case with another pair of types; every level count on every case
CASE_PAIR = dict(zip(IDS, ["f32_f32", "i16_f32", "f64_f64", "i32_i16"]))
SCALE_F = {"f32_f32": dict(cu=(0.5, 3.25), cv=(0.25, -1.5)), "f64_f64": dict(cu=(0.5, 3.25), cv=(0.25, -1.5))}


@pytest.mark.parametrize("nlev", [1, 7, 8, 9, 25])
@pytest.mark.parametrize("name", IDS)
def test_streamed_equals_per_level_chain(fg, name, nlev):
    """below a chunk, a full chunk, a partial last chunk, more chunks than slots (25: every slot reused); page-locked input with
    pageable output and the reverse; each sweep run twice"""
    case = BYNAME[name]
    pair = dict(PAIRS[CASE_PAIR[name]], **SCALE_F.get(CASE_PAIR[name], {}))     # the float pairs with a scale and an offset too
    plan = own_plan(fg, name)
    rs, ru, rv, mask = raw_levels(fg, case, pair, nlev)
    sm, um, vm = masked(rs, mask, pair), masked(ru, mask, pair), masked(rv, mask, pair)
    sw = plan.sweep(pair["i"], pair["o"])
    for hm, fm in ((True, False), (True, True)):
        ws = np.stack([chain(fg, plan, pair, [sm[k]], [pair["cu"]], hm, fm)[0] for k in range(nlev)])
        wuv = [chain(fg, plan, pair, [um[k], rv[k]], [pair["cu"], pair["cv"]], hm, fm) for k in range(nlev)]
        wu, wv = np.stack([a for a, _ in wuv]), np.stack([b for _, b in wuv])
        for pin_in, pin_out in ((True, False), (False, True)):
            for rep in range(2):
                same_bits(stream_scalar(fg, sw, case, pair, sm, hm, fm, pin_in, pin_out), ws, ("s", hm, fm, pin_in, rep))
                gu, gv = stream_vector(fg, sw, case, pair, um, rv, hm, fm, pin_in, pin_out)
                same_bits(gu, wu, ("u", hm, fm, pin_in, rep))
                same_bits(gv, wv, ("v", hm, fm, pin_in, rep))
    sw.destroy()


# ------------------------------------------------------------------------------------------------------------------------ 3
def test_halo_corner_is_not_offset(fg, refs):
    """The +-12 degree window around a cube corner: points whose four corners include a halo corner, init_halo's 0.0.  The
    reference converts the unpadded block only, so that zero gets neither scale nor offset.  Its weight is zero, so the sum
    cannot tell; the missing test can: with missing == offset a halo corner that had been offset would equal the missing
    value and take its point out.  C24 where the reference completes its search there, else C48 (as the resident file)."""
    name = "c24_corner_window"
    if refs[name][1]:
        print("the reference fell back to its global sweep on the C24 corner window: C48 instead")
        name = "c48_corner_window"
    case = BYNAME[name]
    r, fell_back, printed = refs[name]
    assert not fell_back and r is not None, printed[-300:]
    N, idx = case["N"], np.asarray(r["index"])
    at_corner = ((idx[:, 0] == 0) | (idx[:, 0] == N)) & ((idx[:, 1] == 0) | (idx[:, 1] == N))
    assert at_corner.any(), "no point of the window reads a halo corner"
    pair = dict(PAIRS["i16_f32"])
    rs, ru, rv, mask = raw_levels(fg, case, pair)
    for a in (rs, ru, rv):
        a[a == 0] = 1                                    # no raw value widens to the offset itself
    with device_plan(fg, case, index=r["index"], weight=r["weight"]) as p:
        sw = p.sweep(pair["i"], pair["o"])
        sm = masked(rs, mask, pair)
        for hm, fm in COMBOS:                            # the packed field with its usual marker
            same_bits(stream_scalar(fg, sw, case, pair, sm, hm, fm), ref_scalar(fg, case, r, pair, sm, hm, fm), ("s", hm, fm))
            gu, gv = stream_vector(fg, sw, case, pair, masked(ru, mask, pair), rv, hm, fm)
            wu, wv = ref_vector(fg, case, r, pair, masked(ru, mask, pair), rv, hm, fm)
            same_bits(gu, wu, ("u", hm, fm)); same_bits(gv, wv, ("v", hm, fm))
        pair["miss"] = pair["cu"][1]                     # missing == offset: nothing in the data equals it ...
        want = ref_scalar(fg, case, r, pair, rs, True, False)
        assert not np.any(want.reshape(4, -1)[:, at_corner] == np.float32(pair["miss"]))    # ... and no halo corner does
        same_bits(stream_scalar(fg, sw, case, pair, rs, True, False), want, "missing == offset")
        sw.destroy()
    print(f"{name}: {int(at_corner.sum())} points read a halo corner")


# ------------------------------------------------------------------------------------------------------------------------ 4
def test_two_sweeps_share_a_plan_and_any_destruction_order(fg):
    case = BYNAME["c25_72x37_fs0"]
    pf, pi = PAIRS["f32_f32"], PAIRS["i16_f32"]
    plan = device_plan(fg, case)
    sw_f, sw_i = plan.sweep(pf["i"], pf["o"]), plan.sweep(pi["i"], pi["o"])
    sf = masked(*[raw_levels(fg, case, pf, 10)[k] for k in (0, 3)], pf)
    si = masked(*[raw_levels(fg, case, pi, 10)[k] for k in (0, 3)], pi)
    f0 = stream_scalar(fg, sw_f, case, pf, sf, True, False)
    i0 = stream_scalar(fg, sw_i, case, pi, si, True, True)
    f1 = stream_scalar(fg, sw_f, case, pf, sf, True, False)
    i1 = stream_scalar(fg, sw_i, case, pi, si, True, True)
    same_bits(f1, f0, "float sweep, runs interleaved"); same_bits(i1, i0, "short sweep, runs interleaved")
    ws = np.stack([chain(fg, plan, pf, [sf[k]], [pf["cu"]], True, False)[0] for k in range(10)])
    same_bits(f0, ws.reshape(f0.shape), "float sweep against the chain")
    sw_f.destroy()                                       # one before the plan ...
    plan.destroy()
    sw_i.destroy()                                       # ... one after it


def test_argument_error_leaves_the_sweep_usable(fg):
    case, pair = BYNAME["c24_72x37_fs1"], PAIRS["f32_f32"]
    plan = own_plan(fg, case["name"])
    L = fg.lib()
    h = C.c_void_p()
    for bad in ((0, 5), (5, 2), (7, 5)):                 # NC_CHAR / NC_BYTE and numbers outside the list are no field types
        assert L.fg_bilin_sweep_create(plan._h, bad[0], bad[1], C.byref(h)) == FG_ERR_ARG and not h.value
    rs, ru, rv, mask = raw_levels(fg, case, pair, 11)
    sm, um = masked(rs, mask, pair), masked(ru, mask, pair)
    sw = plan.sweep(pair["i"], pair["o"])
    s0 = stream_scalar(fg, sw, case, pair, sm, True, False)
    u0, v0 = stream_vector(fg, sw, case, pair, um, rv, True, True)
    out = np.full((11, case["nlat"], case["nlon"]), np.nan, dtype=np.float32)
    cv = fg._lib.FieldConv(0.0, 0.0, pair["miss"])
    p_in, p_out = sm.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.fg_bilin_sweep_run_scalar(sw._h, p_in, 11, C.byref(cv), 1, 0, None) == FG_ERR_ARG
    assert L.fg_bilin_sweep_run_scalar(sw._h, None, 11, C.byref(cv), 1, 0, p_out) == FG_ERR_ARG
    assert L.fg_bilin_sweep_run_scalar(sw._h, p_in, 11, None, 1, 0, p_out) == FG_ERR_ARG
    assert L.fg_bilin_sweep_run_scalar(sw._h, p_in, 0, C.byref(cv), 1, 0, p_out) == FG_ERR_ARG
    assert L.fg_bilin_sweep_run_scalar(sw._h, p_in, -3, C.byref(cv), 1, 0, p_out) == FG_ERR_ARG
    assert L.fg_bilin_sweep_run_vector(sw._h, p_in, p_in, 11, C.byref(cv), C.byref(cv), 1, 0, p_out, None) == FG_ERR_ARG
    assert np.all(np.isnan(out))                         # nothing was copied
    same_bits(stream_scalar(fg, sw, case, pair, sm, True, False), s0, "scalar after the refused calls")
    u1, v1 = stream_vector(fg, sw, case, pair, um, rv, True, True)
    same_bits(u1, u0, "u after the refused calls"); same_bits(v1, v0, "v after the refused calls")
    fresh = plan.sweep(pair["i"], pair["o"])
    same_bits(stream_scalar(fg, fresh, case, pair, sm, True, False), s0, "a fresh sweep")
    fresh.destroy(); sw.destroy()


def test_plan_stream_is_its_own_after_a_run(fg):
    case, pair = BYNAME["c24_36x19_fs2"], PAIRS["f64_f64"]
    plan = own_plan(fg, case["name"])
    rs, _, _, mask = raw_levels(fg, case, pair, 9)
    sm = masked(rs, mask, pair)
    before = plan.apply_scalar(sm, True, pair["miss"], False).cpu().numpy()
    sw = plan.sweep(pair["i"], pair["o"])
    got = stream_scalar(fg, sw, case, pair, sm, True, False)
    after = plan.apply_scalar(sm, True, pair["miss"], False).cpu().numpy()
    sw.destroy()
    again = plan.apply_scalar(sm, True, pair["miss"], False).cpu().numpy()
    same_bits(after, before, "resident apply after the run"); same_bits(again, before, "resident apply after the sweep is gone")
    same_bits(got, before, "no conversion, double in and out: the streamed levels are the resident ones")
