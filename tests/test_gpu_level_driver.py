"""The chunk driver behind the sweep entries that take eight levels per launch (run_levels in csrc/plan.hip), where the tests of the
families -- test_gpu_masked_levels, test_gpu_levels_ex, test_gpu_mono_levels, test_gpu_mono_records -- do not reach:

  * more than 256 levels with per-level sums: the 256 result slots fill and the sums go to the host in the middle of a call;
  * every call an entry refuses, with the code and the fg_last_error() text include/fregrid_hip.h documents, written out here;
  * the three families one after another on one plan, between the two halves of the limiter: they share the plan's scratch.

C4 -> 12 x 6 (96 source cells, 72 destination cells), order 2 and order 1.  No yardstick beyond the entries themselves is needed:
the family tests pin them to the reference at 1 .. 17 levels, and here a call of 270 levels must equal the same entry on slices of eight
levels, a crowded plan the same entry on a fresh one, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FG_ERR_ARG, FG_ERR_STATE = -1, -6
NI, NLON, NLAT = 4, 12, 6
NCELL, NDST, W = 6 * NI * NI, NLON * NLAT, NI + 2
MISSING = -1.0e10
NLEV = 270                    # 32 chunks of eight fill the 256 result slots and are handed over; a chunk of eight and one of six follow


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _make_plan(fg, order):
    lon, lat = fg.gnomonic_ed_corners(NI)
    lo, la = fg.latlon_corners(NLON, NLAT)
    plan = fg.XgridPlan.create(order, [fg.GridConfig(NI, NI, lon[t], lat[t]) for t in range(6)], fg.GridConfig(NLON, NLAT, lo, la))
    plan.finalize()
    assert plan.ncells_in == NCELL
    return plan


def _inputs(order, nlev, seed):
    """smooth values of one decade with small gradients, as tests/mono_levels_cases.py builds them (the limiter's excess is then an
    ulp, far below the 1e-10 of its fatal check), a seventh of the cells missing, the gradient mask set where a cell of the 3 x 3
    neighbourhood is missing"""
    rng = np.random.default_rng(seed)
    F = 6 * W * W if order == 2 else NCELL
    vals = 5.0 + 2.0 * np.sin(0.05 * np.arange(F)[None, :] + 0.3 * np.arange(nlev)[:, None]) + rng.uniform(-0.01, 0.01, (nlev, F))
    miss = rng.random((nlev, F)) < 1.0 / 7.0
    f = dict(data=_dev(np.where(miss, MISSING, vals)), gx=None, gy=None, gm=None)
    if order == 2:
        m = miss.reshape(nlev, 6, W, W)
        near = np.zeros((nlev, 6, NI, NI), dtype=bool)
        for dj in range(3):
            for di in range(3):
                near |= m[:, :, dj:dj + NI, di:di + NI]
        gm = near.reshape(nlev, NCELL).astype(np.int32)
        assert 0 < gm.sum() < gm.size
        f.update(gx=_dev(rng.uniform(-0.05, 0.05, (nlev, NCELL))), gy=_dev(rng.uniform(-0.05, 0.05, (nlev, NCELL))), gm=_dev(gm))
    f["weight"] = _dev(0.25 + ((5 * np.arange(NCELL)) % 8) / 8.0)
    return f


def _sl(f, k0, n):
    return {k: (v[k0:k0 + n] if v is not None and k != "weight" else v) for k, v in f.items()}


def _run(plan, family, f, nlev):
    """(out [nlev][NDST], sums [nlev]) of one call"""
    out = torch.full((nlev, NDST), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()                                                          # the plan sweeps on a stream of its own
    if family == "masked":
        g = plan.apply_levels(f["data"], out, nlev, MISSING, f["gx"], f["gy"], f["gm"], want_gsum=True)
    elif family == "ex":
        g = plan.apply_levels_ex(f["data"], out, nlev, f["gx"], f["gy"], f["gm"], has_missing=True, missing=MISSING, weight_t=f["weight"],
                                 want_gsum=True)
    else:
        g = plan.apply_levels_mono(f["data"], out, nlev, f["gx"], f["gy"], f["gm"], has_missing=True, missing=MISSING, want_gsum=True)
    plan.sync()
    return out.cpu().numpy(), g


@pytest.fixture(scope="module")
def plans(fg, gpu_ok):
    made = {o: _make_plan(fg, o) for o in (1, 2)}
    yield made
    for p in made.values():
        p.destroy()


# ------------------------------------------------------------------------------------------------------ the 256-slot hand-over
@pytest.mark.parametrize("family,order", [("masked", 1), ("masked", 2), ("ex", 1), ("ex", 2), ("mono", 2)])
def test_sums_handed_over_in_mid_call(fg, plans, family, order):
    plan = plans[order]
    f = _inputs(order, NLEV, 20251021 + order)
    got, gsum = _run(plan, family, f, NLEV)
    assert NLEV > 256 + 8                                                             # the hand-over: nred + 8 > 256 with chunks to come
    assert np.any(got == MISSING) and np.any(got != MISSING) and not np.any(np.isnan(got)) and np.all(gsum[256:] != 0.0)
    for k0 in range(0, NLEV, 8):                                                      # no hand-over in a call of eight levels
        n = min(8, NLEV - k0)
        part, psum = _run(plan, family, _sl(f, k0, n), n)
        assert _same(part, got[k0:k0 + n]), (family, order, k0)
        assert _same(psum, gsum[k0:k0 + n]), (family, order, k0, psum, gsum[k0:k0 + n])


# -------------------------------------------------------------------------------------------------- shared scratch across families
def test_families_share_a_plan_between_begin_and_end(fg, plans):
    """fg_plan_mono_levels_begin on field A, fg_plan_apply_levels on B, fg_plan_apply_levels_ex on C, fg_plan_mono_levels_end on A:
    each result is what the entry gives alone on a fresh plan"""
    L = fg.lib()
    nz, nb, nc = 5, 9, 9
    A, B, Cf = _inputs(2, nz, 1), _inputs(2, nb, 2), _inputs(2, nc, 3)
    opts = fg.XgridPlan._levels_opts(True, MISSING, None, False, None, -1.0e20, None, None, True)
    args = [_p(A[k]) for k in ("data", "gx", "gy", "gm")]

    def limiter(plan, between):
        out = torch.full((nz, NDST), float("nan"), dtype=torch.float64, device=DEV)
        g = np.full(nz, np.nan)
        torch.cuda.synchronize()
        assert L.fg_plan_mono_levels_begin(plan._h, C.byref(opts), *args, nz) == 0
        mid = between(plan)
        assert L.fg_plan_mono_levels_end(plan._h, C.byref(opts), *args, _p(out), g.ctypes.data_as(C.POINTER(C.c_double))) == 0
        plan.sync()
        return out.cpu().numpy(), g, mid

    fresh = [_make_plan(fg, 2) for _ in range(3)]
    try:
        a_out, a_sum, (b, c) = limiter(plans[2], lambda p: (_run(p, "masked", B, nb), _run(p, "ex", Cf, nc)))
        a_ref, a_rsum, _ = limiter(fresh[0], lambda p: None)
        b_ref, c_ref = _run(fresh[1], "masked", B, nb), _run(fresh[2], "ex", Cf, nc)
        assert np.any(a_out == MISSING) and np.any(a_out != MISSING)
        for what, got, ref in (("mono", (a_out, a_sum), (a_ref, a_rsum)), ("masked", b, b_ref), ("ex", c, c_ref)):
            assert _same(got[0], ref[0]) and _same(got[1], ref[1]), what
    finally:
        for p in fresh:
            p.destroy()


# ---------------------------------------------------------------------------------------------------------------- rejected calls
NULL = "null argument"
RAW = "the plan is not finalized (fg_plan_finalize)"
NO_LIMITER = "the monotone limiter works on one level per call (fg_plan_apply_ex)"
LD_VALUE = "field_area_ld must be 0 (one area for all levels) or ncells_in (an area per level)"
LD_NO_AREA = "field_area_ld is set but opts->field_area is NULL"
CELL_AREA = "cell_area_in is required (this plan was loaded from a remap file and holds no cell areas)"
RECORDS_ORDER = "records carry gradients, the plan is first order"
LIMITER_ORDER = "the monotone limiter belongs to conserve_order2 (conserve_interp.c:527-531)"
NLEV_1 = "nlev must be >= 1"
NZ_CALL = "1 to 8 levels per call"
NZ_PAIR = "1 to 8 levels per begin / end pair"
GRADS = "order 2 needs grad_x and grad_y [nlev][ncells_in]"
GRADS_MASK = "order 2 needs grad_x, grad_y and grad_mask [nlev][ncells_in]"
BITS = "order 2 needs the gradient-mask bits"
BITS_MISSING = "a field with missing values needs the gradient-mask bits"


def test_rejected_calls(fg, plans):
    """every refusal of the twelve entries' argument rules: return code and message; none reaches a kernel, so the outputs stay NaN"""
    L = fg.lib()
    good, first = plans[2], plans[1]
    x = good.get_xgrid()
    nogeo = fg.XgridPlan.create_empty(2, [NI] * 6, [NI] * 6, NLON, NLAT)                # exchange cells given: no cell areas
    nogeo.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], x["c1"], x["c2"])
    raw = fg.XgridPlan.create_empty(2, [NI] * 6, [NI] * 6, NLON, NLAT)                  # not finalized
    f = _inputs(2, 9, 7)
    rec = torch.zeros(NCELL, 3, 8, dtype=torch.float64, device=DEV)
    mb = torch.zeros(NCELL, dtype=torch.uint8, device=DEV)
    b8 = torch.zeros(NCELL, 4, 8, dtype=torch.float64, device=DEV)
    fa = torch.ones(9, NCELL, dtype=torch.float64, device=DEV)
    mn, mx = (torch.full((8, NCELL), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
    out = torch.full((9, NDST), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    g = np.full(9, np.nan)
    gp = g.ctypes.data_as(C.POINTER(C.c_double))
    mk = fg.XgridPlan._levels_opts
    plain = mk(True, MISSING, f["weight"], False, None, -1.0e20, None, None, False)
    limit = mk(True, MISSING, f["weight"], False, None, -1.0e20, None, None, True)
    summed = mk(True, MISSING, None, True, None, -1.0e20, None, None, False)               # cell_methods = sum, no cell_area_in
    summed_limit = mk(True, MISSING, None, True, None, -1.0e20, None, None, True)
    measured = mk(True, MISSING, None, False, fa, -1.0e20, None, None, False)             # cell_measures, no cell_area_in
    h, o, ol = good._h, C.byref(plain), C.byref(limit)
    arrays = dict(data=_p(f["data"]), gx=_p(f["gx"]), gy=_p(f["gy"]), gm=_p(f["gm"]))
    null = C.c_void_p(0)

    def entry(fn, order, **defaults):
        def call(**over):
            a = dict(defaults)
            a.update(over)
            return fn(*[a[k] for k in order])
        return call

    def refused(who, call, code, text, **over):
        rc = call(**over)
        assert rc == code, (who, sorted(over), rc, fg._lib.last_error())
        assert fg._lib.last_error() == f"{who}: {text}", (who, sorted(over))

    def common(who, call, nulls, order2=None, area=None):
        """the refusals every entry has: a null in each mandatory position, an unfinalized plan; a first-order plan and a plan
        without cell areas where the entry minds them"""
        for k in nulls:
            refused(who, call, FG_ERR_ARG, NULL, **{k: None if k in ("h", "o") else null})
        refused(who, call, FG_ERR_ARG, RAW, h=raw._h)
        if order2:
            refused(who, call, FG_ERR_ARG, order2, h=first._h)
        for opts in area or ():
            refused(who, call, FG_ERR_ARG, CELL_AREA, h=nogeo._h, o=C.byref(opts))

    try:
        who = "fg_plan_apply_levels"
        call = entry(L.fg_plan_apply_levels, ("h", "data", "gx", "gy", "gm", "missing", "nlev", "out", "g"), h=h, **arrays, missing=MISSING,
                     nlev=9, out=_p(out), g=gp)
        common(who, call, ("h", "data", "out"))
        for n in (0, -3):
            refused(who, call, FG_ERR_ARG, NLEV_1, nlev=n)
        for k in ("gx", "gy", "gm"):
            refused(who, call, FG_ERR_ARG, GRADS_MASK, **{k: null})

        who = "fg_plan_apply_records_levels"
        call = entry(L.fg_plan_apply_records_levels, ("h", "nz", "rec", "mb", "missing", "out", "g"), h=h, nz=8, rec=_p(rec), mb=_p(mb),
                     missing=MISSING, out=_p(out), g=gp)
        common(who, call, ("h", "rec", "out"), order2=RECORDS_ORDER)
        refused(who, call, FG_ERR_ARG, BITS, mb=null)
        for n in (0, 9):
            refused(who, call, FG_ERR_ARG, NZ_CALL, nz=n)

        who = "fg_plan_apply_levels_ex"
        call = entry(L.fg_plan_apply_levels_ex, ("h", "o", "data", "gx", "gy", "gm", "nlev", "ld", "out", "g"), h=h, o=o, **arrays, nlev=9, ld=0,
                     out=_p(out), g=gp)
        common(who, call, ("h", "o", "data", "out"), area=(summed, measured))
        refused(who, call, FG_ERR_ARG, NO_LIMITER, o=ol)
        refused(who, call, FG_ERR_ARG, LD_VALUE, ld=5, o=C.byref(measured))
        refused(who, call, FG_ERR_ARG, LD_NO_AREA, ld=NCELL)
        refused(who, call, FG_ERR_ARG, CELL_AREA, h=nogeo._h, ld=NCELL, o=C.byref(measured))
        refused(who, call, FG_ERR_ARG, NLEV_1, nlev=0)
        for k in ("gx", "gy"):
            refused(who, call, FG_ERR_ARG, GRADS, **{k: null})

        who = "fg_plan_apply_records_levels_ex"
        call = entry(L.fg_plan_apply_records_levels_ex, ("h", "o", "nz", "rec", "mb", "ld", "out", "g"), h=h, o=o, nz=8, rec=_p(rec), mb=_p(mb),
                     ld=0, out=_p(out), g=gp)
        common(who, call, ("h", "o", "rec", "out"), order2=RECORDS_ORDER, area=(summed, measured))
        refused(who, call, FG_ERR_ARG, NO_LIMITER, o=ol)
        refused(who, call, FG_ERR_ARG, LD_VALUE, ld=5, o=C.byref(measured))
        refused(who, call, FG_ERR_ARG, LD_NO_AREA, ld=NCELL)
        refused(who, call, FG_ERR_ARG, CELL_AREA, h=nogeo._h, ld=NCELL, o=C.byref(measured))
        for n in (0, 9):
            refused(who, call, FG_ERR_ARG, NZ_CALL, nz=n)
        refused(who, call, FG_ERR_ARG, BITS_MISSING, mb=null)

        who = "fg_plan_apply_levels_mono"
        call = entry(L.fg_plan_apply_levels_mono, ("h", "o", "data", "gx", "gy", "gm", "nlev", "out", "g"), h=h, o=ol, **arrays, nlev=9,
                     out=_p(out), g=gp)
        common(who, call, ("h", "o", "data", "gx", "gy", "out"), order2=LIMITER_ORDER, area=(summed_limit,))
        refused(who, call, FG_ERR_ARG, NLEV_1, nlev=0)

        who = "fg_plan_mono_levels_begin"
        call = entry(L.fg_plan_mono_levels_begin, ("h", "o", "data", "gx", "gy", "gm", "nz"), h=h, o=ol, **arrays, nz=8)
        common(who, call, ("h", "o", "data", "gx", "gy"), order2=LIMITER_ORDER, area=(summed_limit,))
        for n in (0, 9):
            refused(who, call, FG_ERR_ARG, NZ_PAIR, nz=n)

        who = "fg_plan_mono_levels_end"
        call = entry(L.fg_plan_mono_levels_end, ("h", "o", "data", "gx", "gy", "gm", "out", "g"), h=h, o=ol, **arrays, out=_p(out), g=gp)
        common(who, call, ("h", "o", "data", "gx", "gy", "out"), order2=LIMITER_ORDER, area=(summed_limit,))
        refused(who, call, FG_ERR_STATE, "call fg_plan_mono_levels_begin first")          # every begin above was refused
        who = "fg_plan_mono_levels_copy_minmax"
        for to_plan in (0, 1):
            refused(who, lambda: L.fg_plan_mono_levels_copy_minmax(h, to_plan, _p(mn), _p(mx)), FG_ERR_STATE,
                    "call fg_plan_mono_levels_begin first")

        who = "fg_plan_apply_records_levels_mono"
        call = entry(L.fg_plan_apply_records_levels_mono, ("h", "o", "nz", "rec", "mb", "b8", "out", "g"), h=h, o=ol, nz=8, rec=_p(rec),
                     mb=_p(mb), b8=_p(b8), out=_p(out), g=gp)
        common(who, call, ("h", "o", "rec", "b8", "out"), order2=LIMITER_ORDER, area=(summed_limit,))
        for n in (0, 9):
            refused(who, call, FG_ERR_ARG, NZ_CALL, nz=n)

        who = "fg_plan_mono_records_begin"
        call = entry(L.fg_plan_mono_records_begin, ("h", "o", "nz", "rec", "mb", "b8"), h=h, o=ol, nz=8, rec=_p(rec), mb=_p(mb), b8=_p(b8))
        common(who, call, ("h", "o", "rec", "b8"), order2=LIMITER_ORDER, area=(summed_limit,))
        for n in (0, 9):
            refused(who, call, FG_ERR_ARG, NZ_PAIR, nz=n)

        who = "fg_plan_mono_records_end"
        call = entry(L.fg_plan_mono_records_end, ("h", "o", "rec", "mb", "out", "g"), h=h, o=ol, rec=_p(rec), mb=_p(mb), out=_p(out), g=gp)
        common(who, call, ("h", "o", "rec", "out"), order2=LIMITER_ORDER, area=(summed_limit,))
        refused(who, call, FG_ERR_STATE, "call fg_plan_mono_records_begin first")
        who = "fg_plan_mono_records_copy_minmax"
        for to_plan in (0, 1):
            refused(who, lambda: L.fg_plan_mono_records_copy_minmax(h, to_plan, _p(mn), _p(mx)), FG_ERR_STATE,
                    "call fg_plan_mono_records_begin first")

        # the one difference the header documents: the one-level entries call an unfinalized plan a state error
        assert L.fg_plan_apply_ex(raw._h, o, arrays["data"], arrays["gx"], arrays["gy"], arrays["gm"], 1, _p(out), gp) == FG_ERR_STATE
        assert fg._lib.last_error() == "fg_plan_apply_ex: call fg_plan_finalize first"
        assert L.fg_plan_apply_ex(nogeo._h, C.byref(summed), arrays["data"], arrays["gx"], arrays["gy"], arrays["gm"], 1, _p(out), gp) == FG_ERR_ARG
        assert fg._lib.last_error() == "fg_plan_apply_ex: " + CELL_AREA

        torch.cuda.synchronize()
        for t in (out, mn, mx):
            assert torch.all(torch.isnan(t)).item()
        assert np.all(np.isnan(g)) and torch.all(b8 == 0).item()
    finally:
        nogeo.destroy()
        raw.destroy()
