"""The level loop of the monotone sweep, many levels per call (fg_plan_apply_levels_mono, fg_plan_mono_levels_begin / _copy_minmax /
_end; k_mono_bounds8, k_mono_extremes8, k_apply_ep8m): level k of the output must carry the bits of the reference's
do_scalar_conserve_interp(nz = 1) with MONOTONIC set -- and of fg_plan_apply_ex(monotonic = 1, nz = 1) -- on level k alone
(conserve_interp.c:617-742, :815-866); gsum_out[k] the bits fg_plan_apply_ex returns for that level (the device reduces its row sums
as a tree, so no host yardstick has those bits).

Hand-made one-tile lists (tests/mono_levels_cases.py on tests/sweep_cases.py; plans from create_empty + set_xgrid) reach all four
row-length bins of the sweep; one real pair, C9 -> 30 x 15 with six equal tiles, the depth-dependent land mask of
tests/test_gpu_masked_levels.py and the device's own halo fill and gradients.  Every comparison is bit for bit and over every
destination cell."""
import ctypes as C

import numpy as np
import pytest
import torch

import mono_levels_cases as mc
import orc
import sweep_cases as sc
import test_gpu_masked_levels as ml

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FG_ERR_ARG, FG_ERR_STATE, FG_ERR_DATA = -1, -6, -7
MISSING, NLEV, K_NONE = mc.MISSING, mc.NLEV, mc.K_NONE
LEVEL_COUNTS = (1, 7, 8, 9, 17)
SLACK = 64


def _dev(a, dt=None):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).to(DEV)


def _out(*shape):
    """an output of that shape with SLACK doubles behind it, all NaN"""
    n = int(np.prod(shape))
    buf = torch.full((n + SLACK,), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()                                                          # the plan sweeps on a stream of its own
    return buf, buf[:n].view(*shape)


def _get(plan, buf, view):
    plan.sync()
    host = buf.cpu().numpy()
    assert np.all(np.isnan(host[view.numel():])), "the slack behind the output was written"
    return host[:view.numel()].reshape(tuple(view.shape))


def _assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(sc.bits(got) != sc.bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:4].tolist()}: " \
                          f"{got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}"


def _tensors(kw):
    """device tensors of one input set: (fields, options)"""
    f = dict(data=_dev(kw["data"]), gx=_dev(kw["gx"]), gy=_dev(kw["gy"]), gm=_dev(kw["gm"], np.int32))
    o = dict(has_missing=kw["has_missing"], missing=kw["missing"], weight_t=_dev(kw["weight"]), cell_methods_sum=kw["sum"],
             field_area_t=_dev(kw["field_area"]), cell_area_in_t=_dev(kw["cell_area_in"]), cell_area_out_t=_dev(kw["cell_area_out"]))
    return f, o


def _mono(plan, ndst, f, o, nlev, want_gsum=True, hook=None, k0=0):
    buf, out = _out(nlev, ndst)
    sl = lambda t: t[k0:k0 + nlev] if t is not None else None
    gs = plan.apply_levels_mono(sl(f["data"]), out, nlev, sl(f["gx"]), sl(f["gy"]), sl(f["gm"]), want_gsum=want_gsum, minmax_hook=hook, **o)
    return _get(plan, buf, out), gs


def _one_level(plan, ndst, f, o, k):
    """fg_plan_apply_ex(monotonic = 1, nz = 1) on level k: (out [ndst], gsum)"""
    buf, one = _out(ndst)
    g1 = plan.apply_ex(f["data"][k], one, nz=1, grad_x_t=f["gx"][k], grad_y_t=f["gy"][k], grad_mask_t=f["gm"][k] if f["gm"] is not None else None,
                       monotonic=True, want_gsum=True, **o)
    return _get(plan, buf, one), g1


def _make_plan(fg, c, keep=None):
    x = c["x"]
    k = slice(None) if keep is None else keep
    plan = fg.XgridPlan.create_empty(2, c["tnx"], c["tny"], c["nxo"], c["nyo"])
    plan.set_xgrid(x["t_in"][k], x["i_in"][k], x["j_in"][k], x["i_out"][k], x["j_out"][k], x["area"][k], x["di"][k], x["dj"][k])
    return plan


@pytest.fixture(scope="module")
def cases(fg, gpu_ok):
    made = {}
    print("yardstick:", "the reference library" if orc.conserve_ref_available() else "the plain float64 loop (oracle/_ref not built)")

    def get(name):
        if name not in made:
            mc.check_preconditions(name)
            c = dict(sc.make(name))
            c["plan"] = _make_plan(fg, c)
            assert c["plan"].nxgrid == c["nx"] and c["plan"].ncells_in == c["nsrc"]
            made[name] = c
        return made[name]
    yield get
    for c in made.values():
        c["plan"].destroy()


# ---------------------------------------------------------------------------------------------------------- hand-made lists
@pytest.mark.parametrize("name", mc.CASES)
def test_mono_levels_on_lists(fg, cases, name):
    c = cases(name)
    plan, ndst = c["plan"], c["ndst"]
    variants = [(o, m, None) for o, m in mc.SETS] + [("none", False, True)]           # the last: a gradient mask without missing values
    for opt, masked, with_gm in variants:
        what = mc.set_id(opt, masked) + ("-gm" if with_gm else "")
        kw = mc.inputs(name, opt, masked, with_gm)
        which, ref = mc.yardstick(name, opt, masked, with_gm)
        f, o = _tensors(kw)
        got, gsum = _mono(plan, ndst, f, o, NLEV)
        _assert_bits(got, ref, f"{what}: 17 levels against {which}")
        if masked:
            assert np.all(got[K_NONE] == MISSING)
        for k in range(NLEV):                                                         # == one fg_plan_apply_ex(monotonic, nz = 1) per level
            one, g1 = _one_level(plan, ndst, f, o, k)
            _assert_bits(one, got[k], f"{what}: level {k} against apply_ex")
            assert sc.bits(np.array([g1]))[0] == sc.bits(gsum[k:k + 1])[0], (what, k, g1, gsum[k])
        for nlev in LEVEL_COUNTS[:-1]:                                                # fewer levels, a partial last chunk
            part, psum = _mono(plan, ndst, f, o, nlev)
            _assert_bits(part, ref[:nlev], f"{what}: {nlev} levels")
            assert np.array_equal(sc.bits(psum), sc.bits(gsum[:nlev])), (what, nlev)
        part, none = _mono(plan, ndst, f, o, 9, want_gsum=False)
        assert none is None
        _assert_bits(part, ref[:9], f"{what}: 9 levels, no sums")


def test_partial_chunks(fg, cases):
    """level 8 of a nine-level call, alone in its chunk, and a one-level call are the one-level entry's"""
    c = cases("long-201-1t")
    plan, ndst = c["plan"], c["ndst"]
    for masked in (False, True):
        f, o = _tensors(mc.inputs("long-201-1t", "meas_target", masked))
        nine, g9 = _mono(plan, ndst, f, o, 9)
        one8, g8 = _one_level(plan, ndst, f, o, 8)
        _assert_bits(nine[8], one8, "level 8 of 9")
        assert sc.bits(np.array([g8]))[0] == sc.bits(g9[8:9])[0]
        for k in (0, 8, 16):
            single, gs = _mono(plan, ndst, f, o, 1, k0=k)
            onek, gk = _one_level(plan, ndst, f, o, k)
            _assert_bits(single[0], onek, f"nlev = 1 on level {k}")
            assert sc.bits(np.array([gk]))[0] == sc.bits(gs)[0]


# ---------------------------------------------------------------------------------------------------------------- real pair
def test_mono_levels_on_a_real_pair(fg, gpu_ok):
    """C9 -> 30 x 15, six equal tiles (the reference's nx quirk, :653, tolerates them); tame values under the depth-dependent mask,
    halo fill and gradients from the device's own preparation; 9 levels.  Values stay below 10, so an excess of the limiter is a
    few ulps, far below 1e-10, and the reference's fatal check cannot end the process; the device runs first all the same."""
    if not orc.conserve_ref_available():
        pytest.skip("oracle/_ref/libconserve_ref.so not built (the exchange cells of the pair come from it)")
    nlev = 9
    c = ml.build_host(fg, "short", 2)
    ni, ncell, ndst, m, x = c["ni"], c["ncell"], c["ndst"], c["m"], c["x"]
    rng = np.random.default_rng(20240917)
    vals = rng.choice([-1.0, 1.0], (nlev, 6, ni, ni)) * rng.uniform(1.0, 10.0, (nlev, 6, ni, ni))
    src = np.stack([np.where(ml._missing_at(c["depth"], k), MISSING, vals[k]) for k in range(nlev)]).reshape(nlev, ncell)
    assert np.any(src == MISSING) and np.all(src[ml.K_NONE] == MISSING) and not np.any(src[ml.K_FULL] == MISSING)
    plan = fg.XgridPlan.create_empty(2, c["nx"], c["ny"], c["nlon"], c["nlat"])
    plan.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], x["di"], x["dj"])
    prep = fg.C2lPrep(m["nx"], m["ny"], m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"])
    try:
        assert prep.ncells == ncell
        halo = torch.empty(nlev, prep.F, dtype=torch.float64, device=DEV)
        gx, gy = (torch.empty(nlev, ncell, dtype=torch.float64, device=DEV) for _ in range(2))
        gm = torch.empty(nlev, ncell, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        prep.fill_halo(_dev(src), halo, nlev)
        prep.gradient(halo, nlev, gx, gy, gm, has_missing=True, missing=MISSING)
        prep.sync()
        assert int(gm.sum()) > 0
        f = dict(data=halo, gx=gx, gy=gy, gm=gm)
        ca_in = np.concatenate([np.asarray(a).ravel() for a in x["cell_area_in"]])
        fa = ca_in * (0.5 + ((3 * np.arange(ncell)) % 8) / 8.0)
        for opt in ("none", "meas_target"):
            meas = opt == "meas_target"
            cao = np.asarray(x["cell_area_out"][0]).ravel() if meas else None
            o = dict(has_missing=True, missing=MISSING, field_area_t=_dev(fa) if meas else None, cell_area_in_t=_dev(ca_in) if meas else None,
                     cell_area_out_t=_dev(cao))
            got, gsum = _mono(plan, ndst, f, o, nlev)
            assert np.any(got == MISSING) and np.any(got != MISSING) and np.all(got[ml.K_NONE] == MISSING)
            for k in range(nlev):
                one, g1 = _one_level(plan, ndst, f, o, k)
                _assert_bits(one, got[k], f"{opt}: level {k} against apply_ex")
                assert sc.bits(np.array([g1]))[0] == sc.bits(gsum[k:k + 1])[0], (opt, k)
            h, hx, hy, hm = (t.cpu().numpy() for t in (halo, gx, gy, gm))
            w = (ni + 2) * (ni + 2)
            tl = lambda a, n: [np.ascontiguousarray(a[q * n:(q + 1) * n]) for q in range(6)]
            for k in range(nlev):
                ref, _ = orc.cref_apply(2, x, c["nx"], c["ny"], tl(h[k], w), tl(hx[k], ni * ni), tl(hy[k], ni * ni), tl(hm[k], ni * ni), True, MISSING,
                                        c["nlon"], c["nlat"], 1, field_area=tl(fa, ni * ni) if meas else None,
                                        cell_area_in=tl(ca_in, ni * ni) if meas else None, target_grid=meas, cell_area_out=cao, monotonic=True)
                _assert_bits(got[k], ref, f"{opt}: level {k} against the reference")
    finally:
        prep.destroy()
        plan.destroy()


# ---------------------------------------------------------------------------------------------------------------- the split
@pytest.mark.parametrize("nz", (3, 8))
def test_split_for_ranks(fg, cases, nz):
    """one list, and the same list divided by destination rows into two plans on one device: with the extremes exchanged between
    begin and end (elementwise minimum / maximum, as mpp_min_double / mpp_max_double do across ranks, :672-677) the two outputs
    put together are the single plan's; without the exchange they are not"""
    name = "mid-201-1t"
    c = cases(name)
    ndst, nsrc, half = c["ndst"], c["nsrc"], c["ndst"] // 2
    lower = c["dst"] < half
    in_both = np.intersect1d(c["src"][lower], c["src"][~lower])
    assert in_both.size > 0                                                           # source cells whose exchange cells the division separates
    parts = [_make_plan(fg, c, np.nonzero(sel)[0]) for sel in (lower, ~lower)]
    try:
        for opt, masked in (("none", True), ("weight", False), ("meas_target", True)):
            f, o = _tensors(mc.inputs(name, opt, masked))
            whole, wsum = _mono(c["plan"], ndst, f, o, nz)
            hooked, hsum = _mono(c["plan"], ndst, f, o, nz, hook=lambda plan, n: None)     # the split form of one rank
            _assert_bits(hooked, whole, f"{opt}: begin / end against the one call")
            assert np.array_equal(sc.bits(hsum), sc.bits(wsum))
            L = fg.lib()
            opts = fg.XgridPlan._levels_opts(o["has_missing"], o["missing"], o["weight_t"], o["cell_methods_sum"], o["field_area_t"], -1.0e20,
                                             o["cell_area_in_t"], o["cell_area_out_t"], True)
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
            args = [p(f["data"]), p(f["gx"]), p(f["gy"]), p(f["gm"])]
            for exchange in (True, False):
                bufs = [_out(nz, ndst) for _ in parts]
                for pl in parts:
                    assert L.fg_plan_mono_levels_begin(pl._h, C.byref(opts), *args, nz) == 0
                if exchange:
                    mn = [torch.empty(nz, nsrc, dtype=torch.float64, device=DEV) for _ in parts]
                    mx = [torch.empty(nz, nsrc, dtype=torch.float64, device=DEV) for _ in parts]
                    torch.cuda.synchronize()
                    for pl, a, b in zip(parts, mn, mx):
                        pl.mono_levels_copy_minmax(False, a, b)
                    gmn, gmx = torch.minimum(mn[0], mn[1]), torch.maximum(mx[0], mx[1])
                    assert not torch.equal(gmx, mx[0]) and not torch.equal(gmx, mx[1])
                    torch.cuda.synchronize()
                    for pl in parts:
                        pl.mono_levels_copy_minmax(True, gmn, gmx)
                for pl, (buf, out) in zip(parts, bufs):
                    assert L.fg_plan_mono_levels_end(pl._h, C.byref(opts), *args, p(out), None) == 0
                lo, hi = (_get(pl, buf, out) for pl, (buf, out) in zip(parts, bufs))
                joined = np.concatenate([lo[:, :half], hi[:, half:]], axis=1)
                if exchange:
                    _assert_bits(joined, whole, f"{opt}: two plans, extremes exchanged")
                    # a destination cell outside a plan's part has no exchange cell there
                    assert np.all(lo[:, half:] == o["missing"]) and np.all(hi[:, :half] == o["missing"])
                else:
                    assert np.any(sc.bits(joined) != sc.bits(whole)), f"{opt}: the control without the exchange does not differ"
    finally:
        for pl in parts:
            pl.destroy()


# ------------------------------------------------------------------------------------------------------------------- errors
def test_fatal_level_is_a_data_error(fg, cases):
    name = mc.FATAL_CASE
    c = cases(name)
    plan, ndst = c["plan"], c["ndst"]
    _, _, fatal = mc.fatal_level()
    f, o = _tensors(mc.with_fatal_level(name, 4, 9))
    with pytest.raises(fg.FregridHipError) as one:
        _one_level(plan, ndst, f, o, 4)
    with pytest.raises(fg.FregridHipError) as many:
        _mono(plan, ndst, f, o, 9)
    assert many.value.code == FG_ERR_DATA == one.value.code
    assert str(many.value) == str(one.value) and fatal.message in str(many.value)
    with pytest.raises(fg.FregridHipError) as split:
        _mono(plan, ndst, f, o, 9, hook=lambda plan, n: None)
    assert split.value.code == FG_ERR_DATA and str(split.value) == str(one.value)
    # the plan then sweeps the tame levels correctly
    tame, _ = _tensors(mc.inputs(name, "none", False))
    got, _ = _mono(plan, ndst, tame, o, 9)
    _assert_bits(got, mc.yardstick(name, "none", False)[1][:9], "the tame levels after the data error")


def test_refusals_leave_outputs_and_plans_alone(fg, cases):
    L = fg.lib()
    name = "mid-201-1t"
    c = cases(name)
    plan, ndst, h = c["plan"], c["ndst"], c["plan"]._h
    f, o = _tensors(mc.inputs(name, "meas_target", True))
    first, _ = _mono(plan, ndst, f, o, 9)
    buf, out = _out(9, ndst)
    gs = np.full(9, np.nan)
    gp = gs.ctypes.data_as(C.POINTER(C.c_double))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    mk = fg.XgridPlan._levels_opts
    good = mk(True, MISSING, None, False, o["field_area_t"], -1.0e20, o["cell_area_in_t"], o["cell_area_out_t"], True)
    no_area = mk(True, MISSING, None, False, o["field_area_t"], -1.0e20, None, None, True)          # cell_measures, a plan without geometry
    sum_no_area = mk(True, MISSING, None, True, None, -1.0e20, None, None, True)
    raw = fg.XgridPlan.create_empty(2, c["tnx"], c["tny"], c["nxo"], c["nyo"])                       # not finalized
    first_order = fg.XgridPlan.create_empty(1, c["tnx"], c["tny"], c["nxo"], c["nyo"])
    x = c["x"]
    first_order.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], None, None)
    mn, mx = (torch.full((8, c["nsrc"]), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
    torch.cuda.synchronize()

    def call(**over):
        a = dict(h=h, o=C.byref(good), data=p(f["data"]), gx=p(f["gx"]), gy=p(f["gy"]), gm=p(f["gm"]), nlev=9, out=p(out), g=gp)
        a.update(over)
        return L.fg_plan_apply_levels_mono(a["h"], a["o"], a["data"], a["gx"], a["gy"], a["gm"], a["nlev"], a["out"], a["g"])

    def begin(**over):
        a = dict(h=h, o=C.byref(good), data=p(f["data"]), gx=p(f["gx"]), gy=p(f["gy"]), gm=p(f["gm"]), nz=8)
        a.update(over)
        return L.fg_plan_mono_levels_begin(a["h"], a["o"], a["data"], a["gx"], a["gy"], a["gm"], a["nz"])

    def end(**over):
        a = dict(h=h, o=C.byref(good), data=p(f["data"]), gx=p(f["gx"]), gy=p(f["gy"]), gm=p(f["gm"]), out=p(out), g=gp)
        a.update(over)
        return L.fg_plan_mono_levels_end(a["h"], a["o"], a["data"], a["gx"], a["gy"], a["gm"], a["out"], a["g"])

    try:
        for fn in (call, begin):
            assert fn(h=first_order._h) == FG_ERR_ARG and fn(h=raw._h) == FG_ERR_ARG and fn(h=None) == FG_ERR_ARG
            assert fn(o=None) == FG_ERR_ARG and fn(data=p(None)) == FG_ERR_ARG
            assert fn(gx=p(None)) == FG_ERR_ARG and fn(gy=p(None)) == FG_ERR_ARG
            assert fn(o=C.byref(no_area)) == FG_ERR_ARG and fn(o=C.byref(sum_no_area)) == FG_ERR_ARG
        assert call(out=p(None)) == FG_ERR_ARG
        assert call(nlev=0) == FG_ERR_ARG and call(nlev=-3) == FG_ERR_ARG
        assert begin(nz=0) == FG_ERR_ARG and begin(nz=9) == FG_ERR_ARG and begin(nz=-1) == FG_ERR_ARG
        # no begin is open (every begin above was refused)
        assert L.fg_plan_mono_levels_copy_minmax(h, 0, p(mn), p(mx)) == FG_ERR_STATE
        assert L.fg_plan_mono_levels_copy_minmax(h, 1, p(mn), p(mx)) == FG_ERR_STATE
        assert end() == FG_ERR_STATE
        # an open begin: a refused end writes nothing and leaves it open; the one-level split has its own state
        assert begin(nz=8) == 0
        assert end(out=p(None)) == FG_ERR_ARG and end(o=None) == FG_ERR_ARG and end(gx=p(None)) == FG_ERR_ARG
        assert L.fg_plan_mono_end(h, C.byref(good), p(f["data"]), p(out), gp) == FG_ERR_STATE
        assert np.all(np.isnan(_get(plan, buf, out))) and np.all(np.isnan(gs))
        assert np.all(np.isnan(mn.cpu().numpy())) and np.all(np.isnan(mx.cpu().numpy()))
        assert end() == 0                                                             # ... and the open chunk still ends
        _assert_bits(_get(plan, buf, out)[:8], first[:8], "the chunk that stayed open")
        assert end() == FG_ERR_STATE
    finally:
        raw.destroy()
        first_order.destroy()
    again, _ = _mono(plan, ndst, f, o, 9)
    _assert_bits(again, first, "the next valid run")
