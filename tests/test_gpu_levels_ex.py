"""The level loop with options, many levels per call (fg_plan_apply_levels_ex, fg_plan_apply_records_levels_ex,
fg_sweep_run_levels_ex; k_apply_ep8x): level k of the output and gsum_out[k] must be what the reference's
do_scalar_conserve_interp(nz = 1) -- and fg_plan_apply_ex(nz = 1) -- give on level k alone with the same options
(conserve_interp.c:561-616, :743-813, :815-866; the reference refuses nz > 1 for them, :544-546).

Hand-made lists (tests/levels_ex_cases.py on tests/sweep_cases.py; plans from create_empty + set_xgrid): the smallest cases
that reach every (rows per tile, chunk) pair of the kernel, both area layouts, and the chunk walk in each; row lengths far from
the mean, zero areas, zero weights, AREA_MISSING under missing data.  One real pair: C9 -> 30 x 15 with the depth-dependent
land mask of tests/test_gpu_masked_levels.py, real cell areas, and the gradients of the device's own preparation for the
records entry.

Against the reference: bit-identical where orc.host_has_fma(), 1e-10 relative otherwise, the missing pattern identical either
way.  Between device paths: bit for bit everywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
import levels_ex_cases as lx
import sweep_cases as sc
import test_gpu_masked_levels as ml

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FG_ERR_ARG, FG_ERR_DATA = -1, -7
MISSING, NLEV, K_FULL, K_NONE, AREA_MISSING = lx.MISSING, lx.NLEV, lx.K_FULL, lx.K_NONE, lx.AREA_MISSING
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


def _assert_ref(got, ref, missing, what):
    """the suite's parity rule against the reference"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(got == missing, ref == missing), f"{what}: the missing pattern differs"
    if orc.host_has_fma():
        _assert_bits(got, ref, what)
    else:
        assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref)), what


def _opt_tensors(kw):
    """the device tensors of one option set -> keyword arguments shared by apply_levels_ex and apply_ex"""
    return dict(has_missing=kw["has_missing"], missing=kw["missing"], weight_t=_dev(kw["weight"]), cell_methods_sum=kw["sum"],
                area_missing=AREA_MISSING, cell_area_in_t=_dev(kw["cell_area_in"]), cell_area_out_t=_dev(kw["cell_area_out"]))


def test_capacity_is_what_the_cases_assume(fg, gpu_ok):
    cap = (fg.XgridPlan.levels_ex_capacity(False), fg.XgridPlan.levels_ex_capacity(True))
    assert cap == lx.CAPACITY
    for name in lx.CASES:
        lx.check_crossings(sc.make(name), cap)


# ---------------------------------------------------------------------------------------------------------- hand-made lists
@pytest.fixture(scope="module")
def cases(fg, gpu_ok):
    made = {}
    print("yardstick:", "the reference library" if orc.conserve_ref_available() else "the plain float64 loop (oracle/_ref not built)")

    def get(name, order):
        if (name, order) not in made:
            c = dict(sc.make(name))
            sc.check_preconditions(sc.make(name))
            lx.check_preconditions(sc.make(name))
            x = c["x"]
            plan = fg.XgridPlan.create_empty(order, c["tnx"], c["tny"], c["nxo"], c["nyo"])
            plan.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], x["di"] if order == 2 else None,
                           x["dj"] if order == 2 else None)
            assert plan.nxgrid == c["nx"] and plan.ncells_in == c["nsrc"]
            c["plan"], c["order"] = plan, order
            c["f"] = {m: _dev(sc.field(c, order, m)) for m in (False, True)}
            c["g"] = dict(gx=_dev(c["gx"]), gy=_dev(c["gy"]), gm=_dev(c["gm"])) if order == 2 else dict(gx=None, gy=None, gm=None)
            made[(name, order)] = c
        return made[(name, order)]
    yield get
    for c in made.values():
        c["plan"].destroy()


def _levels_ex(c, kw, ot, fa_t, nlev, want_gsum=True):
    buf, out = _out(nlev, c["ndst"])
    g = c["g"]
    gs = c["plan"].apply_levels_ex(c["f"][kw["has_missing"]], out, nlev, g["gx"], g["gy"], g["gm"] if kw["has_missing"] else None,
                                   field_area_t=fa_t, field_area_per_level=kw["per_level"], want_gsum=want_gsum, **ot)
    return _get(c["plan"], buf, out), gs


def _records(c, k0, nz, masked):
    """[source cell][3][8]: field, grad_x, grad_y of levels [k0, k0 + nz), zero beyond; and the gradient-mask bits"""
    rec = np.zeros((c["nsrc"], 3, 8))
    f = np.where(c["miss"], MISSING, c["vals"]) if masked else c["vals"]
    for w, a in enumerate((f, c["gx"], c["gy"])):
        rec[:, w, :nz] = a[k0:k0 + nz].T
    mb = np.zeros(c["nsrc"], dtype=np.uint8)
    for k in range(nz):
        mb |= (c["gm"][k0 + k] != 0).astype(np.uint8) << k
    return rec, mb


ALL = [(n, o) for n in lx.CASES for o in (1, 2)]


@pytest.mark.parametrize("name,order", ALL, ids=[f"{n}-order{o}" for n, o in ALL])
def test_levels_ex_on_lists(fg, cases, name, order):
    c = cases(name, order)
    plan, g = c["plan"], c["g"]
    for opt, masked in lx.SETS:
        what = f"{lx.set_id(opt, masked)}"
        kw = lx.inputs(c, order, opt, masked)
        which, ref = lx.yardstick(name, order, opt, masked)
        ot, fa_t = _opt_tensors(kw), _dev(kw["field_area"])
        got, gsum = _levels_ex(c, kw, ot, fa_t, NLEV)
        _assert_ref(got, ref, kw["missing"], f"{what}: 17 levels against {which}")
        if masked:
            assert np.all(got[K_NONE] == MISSING)
        # == one fg_plan_apply_ex(nz = 1) per level, values and sums
        buf, one = _out(c["ndst"])
        for k in range(NLEV):
            kg = dict(grad_x_t=g["gx"][k], grad_y_t=g["gy"][k], grad_mask_t=g["gm"][k] if masked else None) if order == 2 else {}
            fa_k = fa_t[k] if (fa_t is not None and kw["per_level"]) else fa_t
            g1 = plan.apply_ex(c["f"][masked][k], one, nz=1, field_area_t=fa_k, want_gsum=True, **kg, **ot)
            _assert_bits(_get(plan, buf, one), got[k], f"{what}: level {k} against apply_ex")
            assert sc.bits(np.array([g1]))[0] == sc.bits(gsum[k:k + 1])[0], (what, k, g1, gsum[k])
        # fewer levels: the same bits, a partial last chunk, no sums
        for nlev in LEVEL_COUNTS[:-1]:
            part, psum = _levels_ex(c, kw, ot, fa_t, nlev)
            _assert_bits(part, got[:nlev], f"{what}: {nlev} levels")
            assert np.array_equal(sc.bits(psum), sc.bits(gsum[:nlev])), (what, nlev)
        part, none = _levels_ex(c, kw, ot, fa_t, 9, want_gsum=False)
        assert none is None
        _assert_bits(part, got[:9], f"{what}: 9 levels, no sums")
        # == the records entry
        if order == 2:
            for k0, nz in ((0, 8), (8, 8), (16, 1), (2, 5)):
                rec, mb = _records(c, k0, nz, masked)
                fa_r = fa_t[k0:k0 + nz].contiguous() if (fa_t is not None and kw["per_level"]) else fa_t
                buf2, o2 = _out(nz, c["ndst"])
                gr = plan.apply_records_levels_ex(nz, _dev(rec), _dev(mb) if masked else None, o2, field_area_t=fa_r,
                                                  field_area_per_level=kw["per_level"], want_gsum=True, **ot)
                _assert_bits(_get(plan, buf2, o2), got[k0:k0 + nz], f"{what}: records, levels {k0}..{k0 + nz}")
                assert np.array_equal(sc.bits(gr), sc.bits(gsum[k0:k0 + nz])), (what, k0, nz)


@pytest.mark.parametrize("name,order", ALL, ids=[f"{n}-order{o}" for n, o in ALL])
def test_every_option_off_is_apply_levels(fg, cases, name, order):
    c = cases(name, order)
    g = c["g"]
    for nlev in LEVEL_COUNTS:
        buf, out = _out(nlev, c["ndst"])
        gs = c["plan"].apply_levels_ex(c["f"][True], out, nlev, g["gx"], g["gy"], g["gm"], has_missing=True, missing=MISSING, want_gsum=True)
        got = _get(c["plan"], buf, out)
        buf2, out2 = _out(nlev, c["ndst"])
        gs2 = c["plan"].apply_levels(c["f"][True], out2, nlev, MISSING, g["gx"], g["gy"], g["gm"], want_gsum=True)
        _assert_bits(got, _get(c["plan"], buf2, out2), f"{nlev} levels against apply_levels")
        assert np.array_equal(sc.bits(gs), sc.bits(gs2)), nlev


# ---------------------------------------------------------------------------------------------------------------- real pair
def _real_options(c, opt):
    """option arrays of the real pair: the reference's own cell areas, weights with zeros, an area variable that is a positive
    function of (cell, level) with AREA_MISSING under a third of the missing (cell, level) pairs when it has a z axis"""
    o = lx.OPTS[opt]
    n, x = c["ncell"], c["x"]
    s, k = np.arange(n)[None, :], np.arange(NLEV)[:, None]
    ca_in = np.concatenate([np.asarray(a).ravel() for a in x["cell_area_in"]])
    w = 0.25 + ((5 * np.arange(n)) % 16) / 4.0
    w[np.arange(n) % 7 == 3] = 0.0
    fa = ca_in * (0.5 + ((3 * np.arange(n)) % 8) / 8.0)
    if o.get("z"):
        fa = fa[None, :] * (0.75 + ((7 * s + 3 * k) % 13) / 17.0)
        fa[(c["src"] == MISSING) & ((s + 2 * k) % 3 == 0)] = AREA_MISSING
        assert np.any(fa == AREA_MISSING)
    return dict(has_missing=True, missing=MISSING, weight=w if o.get("weight") else None, sum=bool(o.get("sum")),
                field_area=np.ascontiguousarray(fa) if o.get("meas") else None, per_level=bool(o.get("z")),
                cell_area_in=ca_in if (o.get("sum") or o.get("meas")) else None,
                cell_area_out=np.asarray(x["cell_area_out"][0]).ravel() if o.get("target") else None)


@pytest.fixture(scope="module")
def real(fg, gpu_ok):
    if not orc.conserve_ref_available():
        pytest.skip("oracle/_ref/libconserve_ref.so not built")
    made = {}

    def get(order):
        if order not in made:
            c = ml.build_host(fg, "short", order)
            plan = fg.XgridPlan.create_empty(order, c["nx"], c["ny"], c["nlon"], c["nlat"])
            x = c["x"]
            plan.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], x.get("di"), x.get("dj"))
            c["plan"] = plan
            m = c["m"]
            c["prep"] = fg.C2lPrep(m["nx"], m["ny"], m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"]) if order == 2 else None
            c["dev"] = {k: _dev(c[k]) for k in ("data", "grad_x", "grad_y", "grad_mask", "src") if k in c}
            made[order] = c
        return made[order]
    yield get
    for c in made.values():
        if c["prep"] is not None:
            c["prep"].destroy()
        c["plan"].destroy()


def _real_reference(c, kw):
    ni, nt, order = c["ni"], len(c["tiles"]), c["order"]
    tl = lambda a: [a[q * ni * ni:(q + 1) * ni * ni] for q in range(nt)] if a is not None else None
    ref = np.empty((NLEV, c["ndst"]))
    for k in range(NLEV):
        fa = kw["field_area"][k] if kw["per_level"] else kw["field_area"]
        common = dict(weight=tl(kw["weight"]), cell_methods_sum=kw["sum"], field_area=tl(fa), area_missing=AREA_MISSING,
                      cell_area_in=tl(kw["cell_area_in"]), target_grid=kw["cell_area_out"] is not None, cell_area_out=kw["cell_area_out"])
        if order == 2:
            ref[k], _ = orc.cref_apply(2, c["x"], c["nx"], c["ny"], [a[k] for a in c["halo"]], [a[k] for a in c["gx"]], [a[k] for a in c["gy"]],
                                       [a[k] for a in c["gm"]], True, MISSING, c["nlon"], c["nlat"], 1, **common)
        else:
            ref[k], _ = orc.cref_apply(1, c["x"], c["nx"], c["ny"], tl(c["src"][k]), None, None, None, True, MISSING, c["nlon"], c["nlat"], 1,
                                       **common)
    return ref


@pytest.mark.parametrize("order", (1, 2))
def test_levels_ex_on_a_real_pair(fg, real, order):
    c = real(order)
    plan, d = c["plan"], c["dev"]
    for opt in lx.OPTS:
        kw = _real_options(c, opt)
        ref = _real_reference(c, kw)
        assert np.any(ref == MISSING) and np.any(ref != MISSING)
        ot, fa_t = _opt_tensors(kw), _dev(kw["field_area"])
        buf, out = _out(NLEV, c["ndst"])
        gsum = plan.apply_levels_ex(d["data"], out, NLEV, d.get("grad_x"), d.get("grad_y"), d.get("grad_mask"), field_area_t=fa_t,
                                    field_area_per_level=kw["per_level"], want_gsum=True, **ot)
        got = _get(plan, buf, out)
        _assert_ref(got, ref, MISSING, f"{opt}: against the reference")
        buf1, one = _out(c["ndst"])
        for k in range(NLEV):
            kg = dict(grad_x_t=d["grad_x"][k], grad_y_t=d["grad_y"][k], grad_mask_t=d["grad_mask"][k]) if order == 2 else {}
            fa_k = fa_t[k] if kw["per_level"] else fa_t
            g1 = plan.apply_ex(d["data"][k], one, nz=1, field_area_t=fa_k, want_gsum=True, **kg, **ot)
            _assert_bits(_get(plan, buf1, one), got[k], f"{opt}: level {k} against apply_ex")
            assert sc.bits(np.array([g1]))[0] == sc.bits(gsum[k:k + 1])[0], (opt, k)
        if order == 2:                                                                # records of the device's own preparation
            rec = torch.empty(c["ncell"], 3, 8, dtype=torch.float64, device=DEV)
            mb = torch.empty(c["ncell"], dtype=torch.uint8, device=DEV)
            for k0 in range(0, NLEV, 8):
                nl = min(8, NLEV - k0)
                c["prep"].records_levels(d["src"][k0:k0 + nl].contiguous(), nl, MISSING, rec, mb); c["prep"].sync()
                fa_r = fa_t[k0:k0 + nl].contiguous() if kw["per_level"] else fa_t
                buf2, o2 = _out(nl, c["ndst"])
                gr = plan.apply_records_levels_ex(nl, rec, mb, o2, field_area_t=fa_r, field_area_per_level=kw["per_level"], want_gsum=True, **ot)
                _assert_bits(_get(plan, buf2, o2), got[k0:k0 + nl], f"{opt}: records, levels from {k0}")
                assert np.array_equal(sc.bits(gr), sc.bits(gsum[k0:k0 + nl])), (opt, k0)


# ----------------------------------------------------------------------------------------------------------------- streamed
@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("opt", ("meas", "sum"))
def test_streamed_levels_ex(fg, real, order, opt):
    """NC_FLOAT levels from the host, 17 of them (a partial last chunk), against the resident call on the widened values"""
    c = real(order)
    plan = c["plan"]
    kw = _real_options(c, opt)
    ot, fa_t = _opt_tensors(kw), _dev(kw["field_area"])
    scale, offset = 0.5, 3.25
    raw = np.ascontiguousarray(c["src"].astype(np.float32))
    assert np.array_equal(raw.astype(np.float64), c["src"]) and np.any(raw == MISSING)
    f64 = ml._widen(raw, scale, offset, MISSING)
    buf, out = _out(NLEV, c["ndst"])
    if order == 2:
        rec = torch.empty(c["ncell"], 3, 8, dtype=torch.float64, device=DEV)
        mb = torch.empty(c["ncell"], dtype=torch.uint8, device=DEV)
        src = _dev(f64)
        for k0 in range(0, NLEV, 8):
            nl = min(8, NLEV - k0)
            c["prep"].records_levels(src[k0:k0 + nl].contiguous(), nl, MISSING, rec, mb); c["prep"].sync()
            plan.apply_records_levels_ex(nl, rec, mb, out[k0:k0 + nl], field_area_t=fa_t, **ot)
            plan.sync()
    else:
        plan.apply_levels_ex(_dev(f64), out, NLEV, field_area_t=fa_t, **ot)
    res = _get(plan, buf, out)
    assert np.any(res == MISSING) and np.any(res != MISSING)
    want = ml._narrow(res, scale, offset, MISSING, np.float32)
    sw = fg.Sweep([plan], c["prep"], np.float32, np.float32)
    got = np.full(want.shape, 77, dtype=np.float32)
    for _ in range(2):                                                                # the second run reuses every slot
        got[...] = 77
        sw.run_levels_ex(raw, [got], scale=scale, offset=offset, field_area_t=fa_t, **ot)
        bad = np.nonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))[0]
        assert bad.size == 0, f"levels that differ from the resident result: {bad.tolist()}"
    if opt == "meas":                                                                 # area_missing under valid data, seen after the last chunk
        fa = kw["field_area"].copy()
        fa[int(np.nonzero(c["src"][16] != MISSING)[0][0])] = AREA_MISSING
        with pytest.raises(fg.FregridHipError, match="data is not missing but area is missing") as e:
            sw.run_levels_ex(raw, [got], scale=scale, offset=offset, field_area_t=_dev(fa), **ot)
        assert e.value.code == FG_ERR_DATA
        sw.run_levels_ex(raw, [got], scale=scale, offset=offset, field_area_t=fa_t, **ot)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # cell_area_out belongs to one destination grid: a sweep of two plans refuses it, and writes nothing
    sw2 = fg.Sweep([plan, plan], c["prep"], np.float32, np.float32)
    outs = [np.full(want.shape, 77, dtype=np.float32) for _ in range(2)]
    cao = _dev(np.asarray(c["x"]["cell_area_out"][0]).ravel())
    with pytest.raises(fg.FregridHipError) as e:
        sw2.run_levels_ex(raw, outs, scale=scale, offset=offset, field_area_t=fa_t, **dict(ot, cell_area_out_t=cao))
    assert e.value.code == FG_ERR_ARG and all(np.all(o == 77) for o in outs)
    sw2.destroy()
    sw.destroy()


# ------------------------------------------------------------------------------------------------------------------- errors
def test_refusals_leave_outputs_and_plans_alone(fg, cases):
    L = fg.lib()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    for order in (1, 2):
        c = cases("mid-201", order)
        plan, g, h = c["plan"], c["g"], c["plan"]._h
        kw = lx.inputs(c, order, "meas_z_target", True)
        ot, fa_t = _opt_tensors(kw), _dev(kw["field_area"])
        first, _ = _levels_ex(c, kw, ot, fa_t, 9)
        buf, out = _out(9, c["ndst"])
        gs = np.full(9, np.nan)
        gp = gs.ctypes.data_as(C.POINTER(C.c_double))
        nsrc = c["nsrc"]

        def opts(**over):
            v = dict(has_missing=1, missing=MISSING, weight=None, sum=0, field_area=fa_t.data_ptr(), area_missing=AREA_MISSING,
                     cell_area_in=ot["cell_area_in_t"].data_ptr(), cell_area_out=ot["cell_area_out_t"].data_ptr(), monotonic=0)
            v.update(over)
            return fg._lib.ApplyOpts(v["has_missing"], v["missing"], v["weight"], v["sum"], v["field_area"], v["area_missing"],
                                     v["cell_area_in"], v["cell_area_out"], v["monotonic"])

        def call(o=None, **over):
            a = dict(h=h, o=C.byref(o if o is not None else opts()), data=p(c["f"][True]), gx=p(g["gx"]), gy=p(g["gy"]), gm=p(g["gm"]),
                     nlev=9, ld=nsrc, out=p(out), g=gp)
            a.update(over)
            if a.pop("no_opts", False):
                a["o"] = None
            return L.fg_plan_apply_levels_ex(a["h"], a["o"], a["data"], a["gx"], a["gy"], a["gm"], a["nlev"], a["ld"], a["out"], a["g"])

        assert call(o=opts(monotonic=1)) == FG_ERR_ARG
        assert call(ld=nsrc - 1) == FG_ERR_ARG and call(ld=1) == FG_ERR_ARG and call(ld=-nsrc) == FG_ERR_ARG
        assert call(o=opts(field_area=None, cell_area_in=None)) == FG_ERR_ARG        # field_area_ld without field_area
        assert call(o=opts(cell_area_in=None)) == FG_ERR_ARG                        # cell_measures, no cell area, a plan without geometry
        assert call(o=opts(sum=1, field_area=None, cell_area_in=None), ld=0) == FG_ERR_ARG
        assert call(nlev=0) == FG_ERR_ARG and call(nlev=-2) == FG_ERR_ARG
        assert call(data=p(None)) == FG_ERR_ARG and call(out=p(None)) == FG_ERR_ARG and call(no_opts=True) == FG_ERR_ARG
        assert call(h=None) == FG_ERR_ARG
        if order == 2:
            assert call(gx=p(None)) == FG_ERR_ARG and call(gy=p(None)) == FG_ERR_ARG
        raw = fg.XgridPlan.create_empty(order, c["tnx"], c["tny"], c["nxo"], c["nyo"])
        assert call(h=raw._h) == FG_ERR_ARG
        if order == 2:
            rec, mb = _records(c, 0, 8, True)
            rec, mb = _dev(rec), _dev(mb)
            rcall = lambda hh=h, o=None, nz=8, r=rec, m=mb, ld=nsrc, oo=out: L.fg_plan_apply_records_levels_ex(
                hh, C.byref(o if o is not None else opts()), nz, p(r), p(m), ld, p(oo), gp)
            assert rcall(hh=raw._h) == FG_ERR_ARG and rcall(nz=0) == FG_ERR_ARG and rcall(nz=9) == FG_ERR_ARG
            assert rcall(r=None) == FG_ERR_ARG and rcall(m=None) == FG_ERR_ARG and rcall(oo=None) == FG_ERR_ARG
            assert rcall(o=opts(monotonic=1)) == FG_ERR_ARG and rcall(ld=7) == FG_ERR_ARG
            assert rcall(hh=cases("mid-201", 1)["plan"]._h) == FG_ERR_ARG             # a first-order plan
        raw.destroy()
        assert np.all(np.isnan(_get(plan, buf, out))) and np.all(np.isnan(gs))
        again, _ = _levels_ex(c, kw, ot, fa_t, 9)
        _assert_bits(again, first, "the next valid run")


def test_area_missing_under_valid_data_is_a_data_error(fg, cases):
    for order in (1, 2):
        c = cases("mid-201", order)
        kw = lx.inputs(c, order, "meas_z", True)
        ot = _opt_tensors(kw)
        first, _ = _levels_ex(c, kw, ot, _dev(kw["field_area"]), NLEV)
        # one valid (cell, level) of the 17 x nsrc, in the last chunk, under an exchange cell
        fa = kw["field_area"].copy()
        k = 16
        s = next(int(v) for v in c["src"] if not c["miss"][k, v])
        fa[k, s] = AREA_MISSING
        with pytest.raises(fg.FregridHipError, match="data is not missing but area is missing") as e:
            _levels_ex(c, kw, ot, _dev(fa), NLEV)
        assert e.value.code == FG_ERR_DATA
        shared = lx.inputs(c, order, "meas", True)
        fa1 = shared["field_area"].copy()
        fa1[s] = AREA_MISSING
        with pytest.raises(fg.FregridHipError, match="data is not missing but area is missing"):
            _levels_ex(c, shared, _opt_tensors(shared), _dev(fa1), NLEV)
        again, _ = _levels_ex(c, kw, ot, _dev(kw["field_area"]), NLEV)
        _assert_bits(again, first, "the next valid run")
