"""The monotone limiter on the gradient object's records and in the streamed sweep (fg_c2l_records_levels_mono,
fg_plan_apply_records_levels_mono, fg_plan_mono_records_begin / _copy_minmax / _end / _reset, fg_sweep_run_levels_mono; k_c2l_records_mb,
k_mono_reset8): every result must carry the bits of fg_plan_apply_levels_mono on the same levels -- that is, of
fg_plan_apply_ex(monotonic = 1, nz = 1) on each level alone (conserve_interp.c:617-742, :815-866) -- of the plain float64 loop, and of
the reference where oracle/_ref is built (the only leg that may be missing).

Hand-made one-tile lists (tests/mono_records_cases.py on tests/mono_levels_cases.py) reach all four row-length bins of the sweep; the
real pair is C9 -> 30 x 15, six tiles of nine cells a side (odd, no multiple of a block), tame values under the depth-dependent mask
of tests/test_gpu_masked_levels.py.  Every comparison is bit for bit and over every cell."""
import ctypes as C

import numpy as np
import pytest
import torch

import mono_levels_cases as mc
import mono_records_cases as rc
import orc
import sweep_cases as sc
import test_gpu_masked_levels as ml
import test_gpu_mono_levels as tm

pytestmark = pytest.mark.gpu
DEV = tm.DEV
FG_ERR_ARG, FG_ERR_STATE, FG_ERR_DATA = -1, -6, -7
MISSING, NLEV, K_NONE, K_FULL = rc.MISSING, rc.NLEV, rc.K_NONE, rc.K_FULL
SLACK = 64
_dev, _out, _get, _assert_bits = tm._dev, tm._out, tm._get, tm._assert_bits
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _chunk_buffers(ncell):
    """rec, maskbits, b8 of one chunk with SLACK elements behind each: NaN / 0xAA until written"""
    rec = torch.full((ncell * 24 + SLACK,), float("nan"), dtype=torch.float64, device=DEV)
    mb = torch.full((ncell + SLACK,), 0xAA, dtype=torch.uint8, device=DEV)
    b8 = torch.full((ncell * 32 + SLACK,), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    return rec, mb, b8


def _read_chunk(ncell, rec, mb, b8):
    """host copies of the three buffers; the slack behind them must be untouched"""
    r, m, b = rec.cpu().numpy(), mb.cpu().numpy(), b8.cpu().numpy()
    assert np.all(np.isnan(r[ncell * 24:])) and np.all(m[ncell:] == 0xAA) and np.all(np.isnan(b[ncell * 32:])), "a store past the last cell"
    return r[:ncell * 24].reshape(ncell, 3, 8), m[:ncell], b[:ncell * 32].reshape(ncell, 4, 8)


def _start_values(b8, nz):
    assert np.all(b8[:, 2] == -1.0e20) and np.all(b8[:, 3] == 1.0e20)
    assert np.all(b8[:, 0, nz:] == -1.0e20) and np.all(b8[:, 1, nz:] == 1.0e20)


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def real(fg, gpu_ok):
    """the real pair on the device: the plan, a second plan over the same source grid that holds the exchange cells of the lower
    destination rows only, the gradient object, and the device's own halo fill and gradients of all 17 levels"""
    c = dict(rc.check_real_preconditions(fg))                                         # (runs the plain loop: no fatal level)
    x, m, ncell = c["x"], c["m"], c["ncell"]
    plan = fg.XgridPlan.create_empty(2, c["tnx"], c["tny"], c["nlon"], c["nlat"])
    plan.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], x["di"], x["dj"])
    low = np.nonzero(c["dst"] < c["ndst"] // 2)[0]
    part = fg.XgridPlan.create_empty(2, c["tnx"], c["tny"], c["nlon"], c["nlat"])
    part.set_xgrid(*[x[k][low] for k in ("t_in", "i_in", "j_in", "i_out", "j_out", "area", "di", "dj")])
    prep = fg.C2lPrep(m["nx"], m["ny"], m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"])
    assert prep.ncells == ncell and plan.ncells_in == ncell and part.ncells_in == ncell
    src = _dev(c["field"])
    halo = torch.empty(NLEV, prep.F, dtype=torch.float64, device=DEV)
    gx, gy = (torch.empty(NLEV, ncell, dtype=torch.float64, device=DEV) for _ in range(2))
    gm = torch.empty(NLEV, ncell, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    prep.fill_halo(src, halo, NLEV)
    prep.gradient(halo, NLEV, gx, gy, gm, has_missing=True, missing=MISSING)
    prep.sync()
    # the plain loop ran on the CPU preparation: the device's is the same, bit for bit
    for name, t in (("halo", halo), ("gx", gx), ("gy", gy)):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(c[name])), name
    assert np.array_equal(gm.cpu().numpy(), c["gm"])
    c.update(plan=plan, part=part, prep=prep, src=src, f=dict(data=halo, gx=gx, gy=gy, gm=gm), low=low)
    yield c
    prep.destroy()
    part.destroy()
    plan.destroy()


def _real_opts(c, opt):
    kw = rc.real_options(c, opt)
    return dict(has_missing=True, missing=MISSING, weight_t=None, cell_methods_sum=False, field_area_t=_dev(kw["field_area"]),
                cell_area_in_t=_dev(kw["cell_area_in"]), cell_area_out_t=_dev(kw["cell_area_out"]))


def _records_chain(c, plan, o, nlev, src=None, want_gsum=True):
    """records_levels_mono -> apply_records_levels_mono per chunk of eight: (out [nlev][ndst], sums [nlev])"""
    src = c["src"] if src is None else src
    rec, mb, b8 = _chunk_buffers(c["ncell"])
    buf, out = _out(nlev, c["ndst"])
    sums = []
    for k0 in range(0, nlev, 8):
        nl = min(8, nlev - k0)
        c["prep"].records_levels_mono(src[k0:k0 + nl], nl, MISSING, rec, mb, b8)
        c["prep"].sync()
        g = plan.apply_records_levels_mono(nl, rec, mb, b8, out[k0:k0 + nl], want_gsum=want_gsum, **o)
        plan.sync()
        sums.append(g)
    _read_chunk(c["ncell"], rec, mb, b8)
    return _get(plan, buf, out), (np.concatenate(sums) if want_gsum else None)


@pytest.fixture(scope="module")
def cases(fg, gpu_ok):
    made = {}

    def get(name):
        if name not in made:
            mc.check_preconditions(name)
            c = dict(sc.make(name))
            c["plan"] = tm._make_plan(fg, c)
            made[name] = c
        return made[name]
    yield get
    for c in made.values():
        c["plan"].destroy()


def _list_chunk(plan, ndst, name, masked, k0, nz, o, hook=None, with_gm=None):
    """one chunk of a hand-made list through the records entry: (out [nz][ndst], sums [nz])"""
    rec, mb, b8, missing = rc.chunk(name, masked, k0, nz, with_gm)
    assert missing == o["missing"]
    buf, out = _out(nz, ndst)
    g = plan.apply_records_levels_mono(nz, _dev(rec), _dev(mb), _dev(b8), out, want_gsum=True, minmax_hook=hook, **o)
    return _get(plan, buf, out), g


# ------------------------------------------------------------------------------------------------------- 1. the records kernel
@pytest.mark.parametrize("nz", (1, 7, 8))
def test_records_kernel(fg, real, nz):
    c, prep, n = real, real["prep"], real["ncell"]
    for k0 in ((0, 16) if nz == 1 else (0,)):
        src = c["src"][k0:k0 + nz]
        rec0 = torch.full((n, 3, 8), float("nan"), dtype=torch.float64, device=DEV)
        mb0 = torch.zeros(n, dtype=torch.uint8, device=DEV)
        rec, mb, b8 = _chunk_buffers(n)
        prep.records_levels(src, nz, MISSING, rec0, mb0)
        prep.records_levels_mono(src, nz, MISSING, rec, mb, b8)
        prep.sync()
        r, m, b = _read_chunk(n, rec, mb, b8)
        assert np.array_equal(_bits(r), _bits(rec0.cpu().numpy())), "rec differs from fg_c2l_records_levels"
        assert np.array_equal(m, mb0.cpu().numpy()) and (np.any(m != 0) or nz == 1), "maskbits differ from fg_c2l_records_levels"
        want = rc.bounds8(c["f"]["data"][k0:k0 + nz].cpu().numpy(), c["tiles"], MISSING, nz)       # over the fg_c2l_fill_halo copy
        assert np.array_equal(_bits(b), _bits(want)), f"b8 differs from the bounds over the halo'd copy (levels from {k0})"
        _start_values(b, nz)
        assert np.any(b[:, 0, 0] != -1.0e20)
        if nz > K_NONE:
            # a level that is missing everywhere keeps the start values -- but for the cells in the cube's corners, whose
            # neighbourhood holds the halo element no contact fills: 0.0, compared like any value
            ni = c["ni"]
            j, i = np.meshgrid(np.arange(ni), np.arange(ni), indexing="ij")
            corner = np.tile((((i == 0) | (i == ni - 1)) & ((j == 0) | (j == ni - 1))).ravel(), 6)
            assert np.all(b[~corner, 0, K_NONE] == -1.0e20) and np.all(b[~corner, 1, K_NONE] == 1.0e20)
            assert np.all(b[corner, 0, K_NONE] == 0.0) and np.all(b[corner, 1, K_NONE] == 0.0)


def test_records_kernel_on_a_regional_tile(fg, gpu_ok):
    """one tile of 5 x 3 cells without a contact: the halo elements nothing fills enter the bounds as 0.0"""
    nx, ny, nz = 5, 3, 3
    lon, lat, lont, latt = fg.gnomonic_ed_grid(16)
    A = np.ascontiguousarray
    tile = [[A(a[0][:ny + 1, :nx + 1])] for a in (lon, lat)] + [[A(a[0][:ny, :nx])] for a in (lont, latt)]
    contacts = fg.find_contacts([nx], [ny], tile[0], tile[1])
    assert len(contacts["tile1"]) == 0
    prep = fg.C2lPrep([nx], [ny], *tile, contacts)
    try:
        n = nx * ny
        rng = np.random.default_rng(7)
        f = np.stack([rng.uniform(1.0, 10.0, n), -rng.uniform(1.0, 10.0, n), rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 10.0, n)])
        f[2, [0, 7, 14]] = MISSING
        src = _dev(f)
        halo = torch.full((nz, prep.F), float("nan"), dtype=torch.float64, device=DEV)
        rec0 = torch.full((n, 3, 8), float("nan"), dtype=torch.float64, device=DEV)
        mb0 = torch.zeros(n, dtype=torch.uint8, device=DEV)
        rec, mb, b8 = _chunk_buffers(n)
        prep.fill_halo(src, halo, nz)
        prep.records_levels(src, nz, MISSING, rec0, mb0)
        prep.records_levels_mono(src, nz, MISSING, rec, mb, b8)
        prep.sync()
        h = halo.cpu().numpy()
        frame = np.ones((ny + 2, nx + 2), dtype=bool)
        frame[1:-1, 1:-1] = False
        assert np.all(h.reshape(nz, ny + 2, nx + 2)[:, frame] == 0.0)
        r, m, b = _read_chunk(n, rec, mb, b8)
        assert np.array_equal(_bits(r), _bits(rec0.cpu().numpy())) and np.array_equal(m, mb0.cpu().numpy())
        assert np.array_equal(_bits(b), _bits(rc.bounds8(h, ((nx, ny),), MISSING, nz)))
        _start_values(b, nz)
        j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        border = ((i == 0) | (i == nx - 1) | (j == 0) | (j == ny - 1)).ravel()
        assert np.all(b[border, 1, 0] == 0.0) and np.all(b[~border, 1, 0] >= 1.0)     # all values positive: the minimum is the frame's 0.0
        assert np.all(b[border, 0, 1] == 0.0) and np.all(b[~border, 0, 1] <= -1.0)    # all negative: the maximum is
    finally:
        prep.destroy()


# ------------------------------------------------------------------------------------- 2. the records entry on hand-made lists
@pytest.mark.parametrize("name", mc.CASES)
def test_records_entry_on_lists(fg, cases, name):
    c = cases(name)
    plan, ndst = c["plan"], c["ndst"]
    for opt, masked in mc.SETS:
        what = mc.set_id(opt, masked)
        f, o = tm._tensors(mc.inputs(name, opt, masked))
        plain = mc.plain(name, opt, masked)[0]                                        # first: the reference would end the process
        levels, lsum = tm._mono(plan, ndst, f, o, NLEV)
        _assert_bits(levels, plain, f"{what}: fg_plan_apply_levels_mono against the plain loop")
        ref = mc.reference(name, opt, masked) if orc.conserve_ref_available() else None
        for k0, nz in ((0, 8), (8, 8), (16, 1)):
            assert any(k0 <= k < k0 + nz for k in mc.STEEP_LEVELS)
            got, gsum = _list_chunk(plan, ndst, name, masked, k0, nz, o)
            _assert_bits(got, levels[k0:k0 + nz], f"{what}: levels from {k0} against fg_plan_apply_levels_mono")
            _assert_bits(got, plain[k0:k0 + nz], f"{what}: levels from {k0} against the plain loop")
            if ref is not None:
                _assert_bits(got, ref[k0:k0 + nz], f"{what}: levels from {k0} against the reference")
            assert np.array_equal(sc.bits(gsum), sc.bits(lsum[k0:k0 + nz])), (what, k0)
            for k in range(k0, k0 + nz):                                              # the sums are fg_plan_apply_ex(monotonic, nz = 1)'s
                one, g1 = tm._one_level(plan, ndst, f, o, k)
                _assert_bits(one, got[k - k0], f"{what}: level {k} against apply_ex")
                assert sc.bits(np.array([g1]))[0] == sc.bits(gsum[k - k0:k - k0 + 1])[0], (what, k, g1, gsum[k - k0])
    # a gradient mask without missing values, and no mask bits at all
    f, o = tm._tensors(mc.inputs(name, "none", False, True))
    got, _ = _list_chunk(plan, ndst, name, False, 0, 8, o, with_gm=True)
    _assert_bits(got, mc.plain(name, "none", False, True)[0][:8], "a gradient mask without missing values")


# ------------------------------------------------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize("nlev", (1, 7, 8, 9, 17))
def test_end_to_end_on_the_real_pair(fg, real, nlev):
    c = real
    plan, ndst = c["plan"], c["ndst"]
    x, ni = c["x"], c["ni"]
    for opt in ("none", "meas_target"):
        o = _real_opts(c, opt)
        plain = rc.real_plain(fg, opt)[0]
        got, gsum = _records_chain(c, plan, o, nlev)
        levels, lsum = tm._mono(plan, ndst, c["f"], o, nlev)
        _assert_bits(got, levels, f"{opt}: against fg_plan_apply_levels_mono on fill_halo + gradient")
        assert np.array_equal(sc.bits(gsum), sc.bits(lsum)), opt
        _assert_bits(got, plain[:nlev], f"{opt}: against the plain loop")
        assert np.any(got != MISSING) and (nlev <= K_NONE or (np.all(got[K_NONE] == MISSING) and np.any(got == MISSING)))
        for k in range(nlev):
            one, g1 = tm._one_level(plan, ndst, c["f"], o, k)
            _assert_bits(one, got[k], f"{opt}: level {k} against apply_ex")
            assert sc.bits(np.array([g1]))[0] == sc.bits(gsum[k:k + 1])[0], (opt, k)
        if not orc.conserve_ref_available():
            print("oracle/_ref is not built: no reference leg")
            continue
        kw = rc.real_options(c, opt)
        w = (ni + 2) * (ni + 2)
        tl = lambda a, n: [np.ascontiguousarray(a[q * n:(q + 1) * n]) for q in range(6)] if a is not None else None
        for k in range(nlev):
            ref, _ = orc.cref_apply(2, x, c["tnx"], c["tny"], tl(c["halo"][k], w), tl(c["gx"][k], ni * ni), tl(c["gy"][k], ni * ni),
                                    tl(c["gm"][k], ni * ni), True, MISSING, c["nlon"], c["nlat"], 1, field_area=tl(kw["field_area"], ni * ni),
                                    cell_area_in=tl(kw["cell_area_in"], ni * ni), target_grid=kw["cell_area_out"] is not None,
                                    cell_area_out=kw["cell_area_out"], monotonic=True)
            _assert_bits(got[k], ref, f"{opt}: level {k} against the reference")


# ------------------------------------------------------------------------------------------ 4. two plans sharing the source
def test_two_plans_share_the_bounds(fg, real):
    c, prep, n, ndst = real, real["prep"], real["ncell"], real["ndst"]
    plan, part = c["plan"], c["part"]
    o = _real_opts(c, "meas")
    nz = 8
    rec, mb, b8 = _chunk_buffers(n)
    prep.records_levels_mono(c["src"][:nz], nz, MISSING, rec, mb, b8)
    prep.sync()
    _, _, fresh_b8 = _read_chunk(n, rec, mb, b8)
    buf_f, out_f = _out(nz, ndst)
    part.apply_records_levels_mono(nz, rec, mb, b8, out_f, **o)                       # the second plan from a fresh bounds pass
    fresh = _get(part, buf_f, out_f)
    prep.records_levels_mono(c["src"][:nz], nz, MISSING, rec, mb, b8)
    prep.sync()
    buf_a, out_a = _out(nz, ndst)
    plan.apply_records_levels_mono(nz, rec, mb, b8, out_a, **o)
    whole = _get(plan, buf_a, out_a)
    _, _, used = _read_chunk(n, rec, mb, b8)
    assert np.array_equal(_bits(used[:, :2]), _bits(fresh_b8[:, :2])) and np.any(used[:, 2, :nz] != -1.0e20)   # consumed: the extremes are in
    stale = b8.clone()
    torch.cuda.synchronize()
    part.mono_records_reset(b8)
    part.sync()
    _, _, again = _read_chunk(n, rec, mb, b8)
    assert np.array_equal(_bits(again), _bits(fresh_b8)), "the reset does not give the bounds pass's records back"
    buf_r, out_r = _out(nz, ndst)
    part.apply_records_levels_mono(nz, rec, mb, b8, out_r, **o)
    _assert_bits(_get(part, buf_r, out_r), fresh, "the second plan after the extremes reset against a fresh bounds pass")
    buf_s, out_s = _out(nz, ndst)
    part.apply_records_levels_mono(nz, rec, mb, stale, out_s, **o)                    # the control: the first plan's extremes left in
    assert np.any(sc.bits(_get(part, buf_s, out_s)) != sc.bits(fresh)), "the control without the reset does not differ"
    half = ndst // 2
    assert np.all(fresh[:, half:] == MISSING) and np.any(whole[:, half:] != MISSING)


# ------------------------------------------------------------------------------------------------------------- 5. the split
@pytest.mark.parametrize("nz", (3, 8))
def test_split_for_ranks_on_records(fg, cases, nz):
    name = "mid-201-1t"
    c = cases(name)
    L = fg.lib()
    ndst, nsrc, half = c["ndst"], c["nsrc"], c["ndst"] // 2
    lower = c["dst"] < half
    parts = [tm._make_plan(fg, c, np.nonzero(sel)[0]) for sel in (lower, ~lower)]
    try:
        for opt, masked in (("none", True), ("weight", False), ("meas_target", True)):
            f, o = tm._tensors(mc.inputs(name, opt, masked))
            whole, wsum = _list_chunk(c["plan"], ndst, name, masked, 0, nz, o)
            hooked, hsum = _list_chunk(c["plan"], ndst, name, masked, 0, nz, o, hook=lambda plan, n: None)
            _assert_bits(hooked, whole, f"{opt}: begin / end against the one call")
            assert np.array_equal(sc.bits(hsum), sc.bits(wsum))
            opts = fg.XgridPlan._levels_opts(o["has_missing"], o["missing"], o["weight_t"], o["cell_methods_sum"], o["field_area_t"], -1.0e20,
                                             o["cell_area_in_t"], o["cell_area_out_t"], True)
            args = [P(f["data"]), P(f["gx"]), P(f["gy"]), P(f["gm"])]
            rec, mb, b8, _ = rc.chunk(name, masked, 0, nz)
            rec_t, mb_t = _dev(rec), _dev(mb)
            ends = dict(weight_t=o["weight_t"], cell_methods_sum=o["cell_methods_sum"], field_area_t=o["field_area_t"],
                        cell_area_in_t=o["cell_area_in_t"], cell_area_out_t=o["cell_area_out_t"])
            for exchange in (True, False):
                joined = {}
                for form in ("levels", "records"):
                    bufs = [_out(nz, ndst) for _ in parts]
                    b8s = [_dev(b8) for _ in parts]                                   # the extremes are a plan's own until exchanged
                    torch.cuda.synchronize()
                    for pl, b in zip(parts, b8s):
                        if form == "levels":
                            assert L.fg_plan_mono_levels_begin(pl._h, C.byref(opts), *args, nz) == 0
                        else:
                            pl.mono_records_begin(nz, rec_t, mb_t, b, o["has_missing"], o["missing"])
                    if exchange:
                        mn = [torch.empty(nz, nsrc, dtype=torch.float64, device=DEV) for _ in parts]
                        mx = [torch.empty(nz, nsrc, dtype=torch.float64, device=DEV) for _ in parts]
                        torch.cuda.synchronize()
                        copy = (lambda pl: pl.mono_levels_copy_minmax) if form == "levels" else (lambda pl: pl.mono_records_copy_minmax)
                        for pl, a, b in zip(parts, mn, mx):
                            copy(pl)(False, a, b)
                        gmn, gmx = torch.minimum(mn[0], mn[1]), torch.maximum(mx[0], mx[1])
                        assert not torch.equal(gmx, mx[0]) and not torch.equal(gmx, mx[1])
                        torch.cuda.synchronize()
                        for pl in parts:
                            copy(pl)(True, gmn, gmx)
                    for pl, (buf, out) in zip(parts, bufs):
                        if form == "levels":
                            assert L.fg_plan_mono_levels_end(pl._h, C.byref(opts), *args, P(out), None) == 0
                        else:
                            pl.mono_records_end(rec_t, mb_t, out, o["has_missing"], o["missing"], **ends)
                    lo, hi = (_get(pl, buf, out) for pl, (buf, out) in zip(parts, bufs))
                    joined[form] = np.concatenate([lo[:, :half], hi[:, half:]], axis=1)
                _assert_bits(joined["records"], joined["levels"], f"{opt}: the records split against the levels split, exchange = {exchange}")
                if exchange:
                    _assert_bits(joined["records"], whole, f"{opt}: two plans, extremes exchanged")
                else:
                    assert np.any(sc.bits(joined["records"]) != sc.bits(whole)), f"{opt}: the control without the exchange does not differ"
        # no begin is open on either part now
        mn, mx = (torch.full((8, nsrc), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
        buf, out = _out(nz, ndst)
        for to_plan in (0, 1):
            assert L.fg_plan_mono_records_copy_minmax(parts[0]._h, to_plan, P(mn), P(mx)) == FG_ERR_STATE
        assert L.fg_plan_mono_records_end(parts[0]._h, C.byref(opts), P(rec_t), P(mb_t), P(out), None) == FG_ERR_STATE
        assert np.all(np.isnan(_get(parts[0], buf, out))) and np.all(np.isnan(mn.cpu().numpy())) and np.all(np.isnan(mx.cpu().numpy()))
    finally:
        for pl in parts:
            pl.destroy()


# ------------------------------------------------------------------------------------------------------------- 6. streamed
def _per_level_chain(c, plan, f64, o):
    """fill_halo, gradient(has_missing) and apply_ex(monotonic, nz = 1) per level on widened values f64 [L][ncell]"""
    L, ncell, prep = f64.shape[0], c["ncell"], c["prep"]
    src = _dev(f64)
    halo = torch.empty(L, prep.F, dtype=torch.float64, device=DEV)
    gx, gy = (torch.empty(L, ncell, dtype=torch.float64, device=DEV) for _ in range(2))
    gm = torch.empty(L, ncell, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    res = np.empty((L, c["ndst"]))
    for k in range(L):                                                                # one level at a time, as the issue's chain
        prep.fill_halo(src[k:k + 1], halo[k:k + 1], 1)
        prep.gradient(halo[k:k + 1], 1, gx[k:k + 1], gy[k:k + 1], gm[k:k + 1], has_missing=True, missing=MISSING)
        prep.sync()
        res[k], _ = tm._one_level(plan, c["ndst"], dict(data=halo, gx=gx, gy=gy, gm=gm), o, k)
    return res


@pytest.mark.parametrize("kind", ("float32", "float64"))
def test_streamed(fg, real, kind):
    c = real
    dt = np.dtype(kind)
    scale, offset = 0.5, 3.25
    raw_buf = fg.HostBuffer((NLEV, c["ncell"]), dt)
    raw = raw_buf.array
    raw[...] = c["field"].astype(dt)
    assert np.any(raw == MISSING) and np.all(raw[K_NONE] == MISSING)
    f64 = ml._widen(raw, scale, offset, MISSING)
    sweeps = {1: fg.FieldSweep([c["plan"]], c["prep"], dt, dt), 2: fg.FieldSweep([c["plan"], c["part"]], c["prep"], dt, dt)}
    pinned = [fg.HostBuffer((NLEV, c["ndst"]), dt) for _ in range(2)]
    chains = {}
    try:
        for nplans, opt in ((1, "none"), (1, "meas"), (1, "meas_target"), (2, "none"), (2, "meas")):
            o = _real_opts(c, opt)
            plans = [c["plan"], c["part"]][:nplans]
            want = []
            for p, plan in enumerate(plans):
                if (opt, p) not in chains:
                    chains[(opt, p)] = ml._narrow(_per_level_chain(c, plan, f64, o), scale, offset, MISSING, dt)
                want.append(chains[(opt, p)])
            assert np.any(want[0] == dt.type(MISSING)) and np.any(want[0] != dt.type(MISSING))
            runs = [("pinned", raw, [b.array for b in pinned[:nplans]]), ("pinned, second run", raw, [b.array for b in pinned[:nplans]]),
                    ("pageable", np.array(raw), [np.empty((NLEV, c["ndst"]), dtype=dt) for _ in plans])]
            for how, src, outs in runs:
                for a in outs:
                    a[...] = 77
                sweeps[nplans].run_levels_mono(src, outs, scale=scale, offset=offset, **o)
                for p, (got, w) in enumerate(zip(outs, want)):
                    bad = np.nonzero(np.any(ml._view(got) != ml._view(w), axis=1))[0]
                    assert bad.size == 0, f"{opt}, {nplans} plans, plan {p}, {how}: levels that differ from the per-level chain: {bad.tolist()}"
    finally:
        for s in sweeps.values():
            s.destroy()
        for b in pinned + [raw_buf]:
            b.free()


# ------------------------------------------------------------------------------------------------------------ 7. fatal level
def test_fatal_level_is_a_data_error(fg, cases):
    name = mc.FATAL_CASE
    c = cases(name)
    plan, ndst = c["plan"], c["ndst"]
    _, _, fatal = mc.fatal_level()                                                    # the plain loop first: it raised, the device only returns
    kw = mc.with_fatal_level(name, 4, 9)
    f, o = tm._tensors(kw)
    with pytest.raises(fg.FregridHipError) as one:
        tm._one_level(plan, ndst, f, o, 4)
    field = kw["data"][:8][:, c["inner"]]
    rec, mb = rc.records8(field, kw["gx"][:8], kw["gy"][:8], None, 8)
    b8 = rc.bounds8(kw["data"][:8], c["tiles"], -1.0e20, 8)
    for hook in (None, lambda plan, n: None):
        buf, out = _out(8, ndst)
        with pytest.raises(fg.FregridHipError) as many:
            plan.apply_records_levels_mono(8, _dev(rec), None, _dev(b8), out, minmax_hook=hook, **o)
        assert many.value.code == FG_ERR_DATA == one.value.code
        assert str(many.value) == str(one.value) and fatal.message in str(many.value)
        plan.sync()
    # the plan then sweeps the tame levels correctly
    got, _ = _list_chunk(plan, ndst, name, False, 0, 8, o)
    _assert_bits(got, mc.plain(name, "none", False)[0][:8], "the tame levels after the data error")


# -------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_leave_outputs_and_plans_alone(fg, cases):
    L = fg.lib()
    name = "mid-201-1t"
    c = cases(name)
    plan, ndst, h = c["plan"], c["ndst"], c["plan"]._h
    f, o = tm._tensors(mc.inputs(name, "meas_target", True))
    first, _ = _list_chunk(plan, ndst, name, True, 0, 8, o)
    rec, mb, b8, _ = rc.chunk(name, True, 0, 8)
    rec_t, mb_t = _dev(rec), _dev(mb)
    sentinel = np.full_like(b8, 77.0)
    b8_t = _dev(sentinel)
    buf, out = _out(8, ndst)
    gs = np.full(8, np.nan)
    gp = gs.ctypes.data_as(C.POINTER(C.c_double))
    mk = fg.XgridPlan._levels_opts
    good = mk(True, MISSING, None, False, o["field_area_t"], -1.0e20, o["cell_area_in_t"], o["cell_area_out_t"], True)
    no_area = mk(True, MISSING, None, False, o["field_area_t"], -1.0e20, None, None, True)           # cell_measures, a plan without geometry
    sum_no_area = mk(True, MISSING, None, True, None, -1.0e20, None, None, True)
    raw = fg.XgridPlan.create_empty(2, c["tnx"], c["tny"], c["nxo"], c["nyo"])                       # not finalized
    first_order = fg.XgridPlan.create_empty(1, c["tnx"], c["tny"], c["nxo"], c["nyo"])
    x = c["x"]
    first_order.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], None, None)

    def call(**over):
        a = dict(h=h, o=C.byref(good), nz=8, rec=P(rec_t), mb=P(mb_t), b8=P(b8_t), out=P(out), g=gp)
        a.update(over)
        return L.fg_plan_apply_records_levels_mono(a["h"], a["o"], a["nz"], a["rec"], a["mb"], a["b8"], a["out"], a["g"])

    def begin(**over):
        a = dict(h=h, o=C.byref(good), nz=8, rec=P(rec_t), mb=P(mb_t), b8=P(b8_t))
        a.update(over)
        return L.fg_plan_mono_records_begin(a["h"], a["o"], a["nz"], a["rec"], a["mb"], a["b8"])

    try:
        for fn in (call, begin):
            assert fn(h=first_order._h) == FG_ERR_ARG and fn(h=raw._h) == FG_ERR_ARG and fn(h=None) == FG_ERR_ARG
            assert fn(o=None) == FG_ERR_ARG and fn(rec=P(None)) == FG_ERR_ARG and fn(b8=P(None)) == FG_ERR_ARG
            assert fn(nz=0) == FG_ERR_ARG and fn(nz=9) == FG_ERR_ARG and fn(nz=-1) == FG_ERR_ARG
            assert fn(o=C.byref(no_area)) == FG_ERR_ARG and fn(o=C.byref(sum_no_area)) == FG_ERR_ARG
        assert call(out=P(None)) == FG_ERR_ARG
        assert L.fg_plan_mono_records_reset(h, P(None)) == FG_ERR_ARG and L.fg_plan_mono_records_reset(None, P(b8_t)) == FG_ERR_ARG
        assert L.fg_plan_mono_records_end(h, C.byref(good), P(rec_t), P(mb_t), P(out), gp) == FG_ERR_STATE     # every begin was refused
        assert np.all(np.isnan(_get(plan, buf, out))) and np.all(np.isnan(gs))
        assert np.array_equal(_bits(b8_t.cpu().numpy()), _bits(sentinel)), "a refused call wrote into b8"
    finally:
        raw.destroy()
        first_order.destroy()
    again, _ = _list_chunk(plan, ndst, name, True, 0, 8, o)
    _assert_bits(again, first, "the next valid call")


def test_streamed_refusals(fg, real):
    c = real
    x = c["x"]
    dt = np.dtype("float32")
    raw = np.ascontiguousarray(c["field"].astype(dt))
    o = _real_opts(c, "meas_target")
    first_order = fg.XgridPlan.create_empty(1, c["tnx"], c["tny"], c["nlon"], c["nlat"])
    first_order.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], None, None)
    sw0 = fg.FieldSweep([first_order], None, dt, dt)                                  # first order: created without a gradient object
    sw1 = fg.FieldSweep([c["plan"]], c["prep"], dt, dt)
    sw2 = fg.FieldSweep([c["plan"], c["part"]], c["prep"], dt, dt)
    outs = [np.full((NLEV, c["ndst"]), 77, dtype=dt) for _ in range(2)]
    try:
        with pytest.raises(fg.FregridHipError) as e:
            sw0.run_levels_mono(raw, outs[:1], **_real_opts(c, "none"))
        assert e.value.code == FG_ERR_ARG
        with pytest.raises(fg.FregridHipError) as e:
            sw2.run_levels_mono(raw, outs, **o)                                       # cell_area_out with two plans
        assert e.value.code == FG_ERR_ARG and all(np.all(a == 77) for a in outs)
        # the objects work afterwards: the first plan's output does not depend on the sweep it runs in
        one = np.full((NLEV, c["ndst"]), 77, dtype=dt)
        sw1.run_levels_mono(raw, [one], **_real_opts(c, "meas"))
        sw2.run_levels_mono(raw, outs, **_real_opts(c, "meas"))
        assert np.array_equal(ml._view(outs[0]), ml._view(one)) and not np.any(one == 77)
        sw0.run_levels(raw, [one], missing=MISSING)                                   # the first-order sweep still runs what it can
    finally:
        for s in (sw0, sw1, sw2):
            s.destroy()
        first_order.destroy()
