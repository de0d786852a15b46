"""The great-circle searches on inputs where the reference's clip ends the process (tests/gc_fatal_cases.py): the device must
return FG_ERR_GEOM with the reference's text for the code the _cr oracle returns -- never a plan -- and must build the next plan
as if nothing had happened.

Every case runs under fg_set_gc_split 0 / 1 (one-kernel clip / screen, solve, walk with the hand-over to the one-kernel clip) and
fg_set_search_async 0 / 1 (blocks handed back untagged after a drained stream / tagged with the plan's stream).  Codes and texts are
compared for equality, plans in bits; there is no tolerance here.  tests/test_gc_fatal_cases_cpu.py shows the compiled reference
dying with the same text on the same inputs.

Two grid cases hold the bad cell BESIDE the other grid, two degrees from its edge: no pair overlaps, the reference still ends
(its convexity checks come right after the range test), and so must the device -- its candidate scan has to offer those pairs.

After every failing create, on the same stream: the clean grid pair (or the list without the bad polygon) must equal the _cr
oracle as in tests/test_gpu_polylist_gc.py, and the failing create must fail again in the same way -- an error return that lost or
double-returned a block of the stream-ordered pool shows there.

Which route a fatal pair took under gc_split = 1 cannot be asserted: the only counter that tells the routes apart, stats()'s
`deferred` (pairs on the screen's list plus pairs the walk handed over), belongs to the plan, and a failing create returns none.
The per-pair codes of the one-kernel clip are pinned separately through fg_gc_clip_batch, and the split route is covered as far
as it can be by requiring the same code and text under both settings."""
import numpy as np
import pytest

import coupler_gc_cases as cg
import gc_fatal_cases as gf
import orc
import polylist_gc_cases as pc

pytestmark = pytest.mark.gpu
SETTINGS = [(split, asyn) for split in (0, 1) for asyn in (0, 1)]
IDS = [f"split{s}-async{a}" for s, a in SETTINGS]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class _settings:
    def __init__(self, fg, split, asyn):
        self.L, self.split, self.asyn = fg.lib(), split, asyn

    def __enter__(self):
        self.L.fg_set_gc_split(self.split)
        self.L.fg_set_search_async(self.asyn)

    def __exit__(self, *exc):
        self.L.fg_set_gc_split(1)
        self.L.fg_set_search_async(1)


def _text(code):
    return f"libfregrid_hip error {gf.FG_ERR_GEOM}: {gf.MESSAGES[code]}"


def _fails(make, code):
    """make() must raise FG_ERR_GEOM with the text of `code`"""
    with pytest.raises(Exception) as e:
        plan = make()
        n = plan.nxgrid
        plan.destroy()
        pytest.fail(f"a plan of {n} exchange cells where the reference ends the process (code {code})")
    assert getattr(e.value, "code", None) == gf.FG_ERR_GEOM, repr(e.value)
    assert str(e.value) == _text(code), (str(e.value), _text(code))


def _cfg(fg, g):
    return fg.GridConfig(g[0], g[1], g[2], g[3])


# ------------------------------------------------------------------------------------------------------------ quad x quad
def _torch_grid(fg, g, dev):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    return [t(v) for v in fg.latlon2xyz(g[2], g[3])]


def _grid_entries(fg, src, dst, mask, stream):
    """name -> callable that creates the plan through one entry; the _dev entry on the caller's stream"""
    import torch
    dev = torch.device("cuda", 0)
    masks = None if mask is None else [mask]

    def dev_entry():
        xs, xd = _torch_grid(fg, src, dev), _torch_grid(fg, dst, dev)
        mt = None if mask is None else [torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float64)).to(dev)]
        torch.cuda.synchronize()
        try:
            return fg.XgridPlan.create_great_circle_dev([src[0]], [src[1]], [xs], dst[0], dst[1], xd, stream=stream.cuda_stream, masks_t=mt)
        finally:
            stream.synchronize()                  # the tensors go away with this frame

    return {"create_great_circle": lambda: fg.XgridPlan.create_great_circle([_cfg(fg, src)], _cfg(fg, dst), masks=masks),
            "create_great_circle_lonlat": lambda: fg.XgridPlan.create_great_circle_lonlat([_cfg(fg, src)], _cfg(fg, dst), masks=masks),
            "create_great_circle_dev": dev_entry}


def _check_grid_plan(plan, o, what):
    assert plan.nxgrid == o["n"], what
    x = plan.get_xgrid() if o["n"] else {k: np.zeros(0, dtype=np.int32) for k in ("t_in", "i_in", "j_in", "i_out", "j_out", "area")}
    for k in ("i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(x[k], o[k]), (what, k)
    assert not np.any(x["t_in"]), what
    nd = int(np.count_nonzero(_bits(x["area"]) != _bits(o["area"]))) if o["n"] else 0
    assert nd == 0, f"{what}: {nd} of {o['n']} areas differ from the _cr oracle"


@pytest.mark.parametrize("split,asyn", SETTINGS, ids=IDS)
@pytest.mark.parametrize("name", gf.FATAL_GRIDS)
def test_fatal_grid_pair_is_the_references_error_and_the_next_plan_is_whole(fg, gpu_ok, name, split, asyn):
    """mixed cases: the device's documented order (grid box 1, grid box 2, the largest clip code) over the codes the oracle returns
    for the pairs of the case; the others hold one code, the grid-level oracle's"""
    import torch
    c = gf.GRID_CASES[name]
    facts = gf.grid_facts(name)[1]
    assert facts["result"][0] == "code"
    code = gf.device_code(facts["codes"])
    assert code in facts["codes"] and (name in gf.MIXED_GRIDS or code == facts["result"][1])
    kind, clean = gf.grid_result(c["clean"][0], c["clean"][1], None, True)
    assert kind == "n" and clean["n"] > 0
    stream = torch.cuda.Stream()
    with _settings(fg, split, asyn):
        bad = _grid_entries(fg, c["src"], c["dst"], c["mask"], stream)
        good = _grid_entries(fg, c["clean"][0], c["clean"][1], None, stream)
        for entry in bad:
            _fails(bad[entry], code)
            plan = good[entry]()
            _check_grid_plan(plan, clean, (name, entry, "clean pair after the error"))
            plan.destroy()
            _fails(bad[entry], code)


@pytest.mark.parametrize("split,asyn", SETTINGS, ids=IDS)
@pytest.mark.parametrize("name", gf.SILENT)
def test_silent_and_masked_grid_pairs_equal_the_oracle(fg, gpu_ok, name, split, asyn):
    """descending latitudes: no exchange cell and no error; the masked twins: the source cells of every fatal pair have mask 0, the
    reference never clips them (create_xgrid.c:1401), the rest of the exchange grid is there"""
    import torch
    c = gf.GRID_CASES[name]
    kind, o = gf.grid_result(c["src"], c["dst"], c["mask"], True)
    assert kind == "n"
    if name.endswith("_masked"):
        assert o["n"] > 0 and gf.grid_facts(name[:-len("_masked")])[1]["result"][0] == "code"
    stream = torch.cuda.Stream()
    with _settings(fg, split, asyn):
        for entry, make in _grid_entries(fg, c["src"], c["dst"], c["mask"], stream).items():
            plan = make()
            _check_grid_plan(plan, o, (name, entry))
            if split == 1 and o["n"]:
                assert plan.stats()["pairs"] >= o["n"]
            plan.destroy()


def test_one_kernel_clip_returns_the_oracles_code_pair_by_pair(fg, gpu_ok):
    """fg_gc_clip_batch (the packed clip, the array clip behind it, and the two convexity checks) on every fatal pair of every
    grid case and on the four-corner pair cases, with as many ordinary pairs between them: n_out equals the _cr oracle's, negative
    codes included -- the per-pair check that the searches' one error word cannot give"""
    a, b = [], []
    for name in gf.FATAL_GRIDS:
        c = gf.GRID_CASES[name]
        S, T = pc.Grid(*c["src"]), pc.Grid(*c["dst"])
        for s, d in gf.grid_pair_codes(c["src"], c["dst"], c["mask"], True):
            a.append(S.cells[s]); b.append(T.cells[d])
        S, T = pc.Grid(*c["clean"][0]), pc.Grid(*c["clean"][1])
        a.append(S.cells[0]); b.append(T.cells[0])
    for c in gf.PAIR_CASES.values():
        if len(c["poly"]) == 4:
            g = gf.PAIR_GRIDS[c["grid"]]
            for d in gf.pair_codes(c["poly"], g, True):
                a.append(c["poly"]); b.append(g.cells[d])
    want = np.array([orc.orc_clip_gc(p, q, cr=True)[0] for p, q in zip(a, b)], dtype=np.int32)
    assert {-int(v) for v in want if v < 0} >= {1, 2, 5, 6}, sorted(set(want.tolist()))
    n_out, _, _ = fg.gc_clip_batch(np.array(a), np.array(b))
    bad = np.flatnonzero(n_out != want)
    assert bad.size == 0, (bad[:8], n_out[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------------------------------------------------ polygon lists
def _list_entries(fg, n, xyz, ar, g, stream):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def dev_entry():
        xd = [t(v) for v in fg.latlon2xyz(g.lon, g.lat)]
        args = [t(np.ascontiguousarray(n, dtype=np.int32))] + [t(xyz[:, :, k]) for k in range(3)] + [t(ar)]
        torch.cuda.synchronize()
        try:
            return fg.XgridPlan.create_polylist_gc_dev(*args, g.nx, g.ny, xd, stream=stream.cuda_stream)
        finally:
            stream.synchronize()

    return {"create_polylist_gc": lambda: fg.XgridPlan.create_polylist_gc(n, xyz[:, :, 0], xyz[:, :, 1], xyz[:, :, 2], ar, fg.GridConfig(g.nx, g.ny, g.lon, g.lat)),
            "create_polylist_gc_dev": dev_entry}


def _check_list_plan(plan, ref, dst):
    """tests/test_gpu_polylist_gc.py's _check_plan"""
    assert plan.nxgrid == len(ref["poly"])
    x = plan.get_xgrid()
    assert np.array_equal(x["i_in"], ref["poly"]) and not x["j_in"].any() and not x["t_in"].any()
    assert np.array_equal(x["j_out"].astype(np.int64) * dst.nx + x["i_out"], ref["cell"])
    nd = int(np.count_nonzero(_bits(x["area"]) != _bits(ref["area"])))
    assert nd == 0, f"{nd} of {plan.nxgrid} areas differ from the _cr oracle"
    pg = plan.get_polygons(16)
    assert np.array_equal(pg["n"], ref["nv"])
    for k, ax in enumerate("xyz"):
        nd = int(np.count_nonzero(_bits(pg[ax]) != _bits(ref["verts"][:, :, k])))
        assert nd == 0, f"{nd} vertex {ax} values differ from the _cr oracle"


def _list_case(fg, n, xyz, g, code, stream):
    """the failing list through both entries; after each failure the four ordinary polygons on the clean grid, then the failure again"""
    n4, v4, ar4, g4, ref4 = gf.clean_reference()
    assert len(n) <= 8 and len(ref4["poly"]) > 0
    bad = _list_entries(fg, n, xyz, gf.area_ref(n, xyz), g, stream)
    good = _list_entries(fg, n4, v4, ar4, g4, stream)
    for entry in bad:
        _fails(bad[entry], code)
        plan = good[entry]()
        _check_list_plan(plan, ref4, g4)
        plan.destroy()
        _fails(bad[entry], code)


@pytest.mark.parametrize("split,asyn", SETTINGS, ids=IDS)
@pytest.mark.parametrize("name", list(gf.PAIR_CASES))
def test_fatal_polygon_in_a_list_is_the_references_error(fg, gpu_ok, name, split, asyn):
    """the bad polygon first, in the middle and last among the four ordinary ones"""
    import torch
    c = gf.PAIR_CASES[name]
    stream = torch.cuda.Stream()
    with _settings(fg, split, asyn):
        for position in (0, 2, 4):
            n, xyz = gf.polylist(name, position)
            _list_case(fg, n, xyz, gf.PAIR_GRIDS[c["grid"]], c["code"], stream)


@pytest.mark.parametrize("split,asyn", SETTINGS, ids=IDS)
@pytest.mark.parametrize("name", list(gf.MIXED_LISTS))
def test_mixed_list_reports_in_the_devices_order(fg, gpu_ok, name, split, asyn):
    """two bad polygons with different codes among the ordinary ones: grid box 1 before everything, else the larger clip code --
    and a code that the oracle returns for some pair of the list"""
    import torch
    n, xyz = gf.mixed_polylist(gf.MIXED_LISTS[name])
    g = gf.PAIR_GRIDS[gf.CLEAN_GRID]
    codes = gf.list_codes(n, xyz, g, True)
    assert len(codes) == 2
    with _settings(fg, split, asyn):
        _list_case(fg, n, xyz, g, gf.device_code(codes), torch.cuda.Stream())


# ------------------------------------------------------------------------------------------------------------ the coupler
def _coupler_case(fg, which):
    """own_c4 (the smallest coupler case with land of its own) with one interior corner of the ocean or of the land grid moved
    north past its neighbour: (clean case, broken case)"""
    c = cg.own_c4(fg)
    b = dict(c)
    if which == "ocean":
        g = c["ocn"]
        lat = g.lat.copy()
        lat[8, 5] = lat[9, 5] + 0.9 * (lat[9, 5] - lat[8, 5])
        b["ocn"] = pc.Grid(g.nx, g.ny, g.lon, lat)
    else:
        g = c["lnd"][0]
        lat = g.lat.copy()
        lat[3, 4] = lat[4, 4] + 0.9 * (lat[4, 4] - lat[3, 4])
        b["lnd"] = [pc.Grid(g.nx, g.ny, g.lon, lat)]
    return c, b


def _restatement_error(b):
    """the code of the first fatal clip of coupler_gc_cases' restatement under the _cr primitives"""
    P = pc.prims_oracle(True)
    with pytest.raises(RuntimeError) as e:
        cg.reference_coupler_gc(b["atm"], b["lnd"], b["ocn"], b["omask"], P, ocn_south_ext=b["ext"])
    head = f"{P.name}: clip error -"
    assert str(e.value).startswith(head), str(e.value)
    return int(str(e.value)[len(head):].split()[0])


def _mosaic(fg, c):
    cfg = lambda g: fg.GridConfig(g.nx, g.ny, g.lon, g.lat)
    return fg.CouplerMosaic([cfg(g) for g in c["atm"]], [cfg(g) for g in c["lnd"]], cfg(c["ocn"]), c["omask"], interp_order=1,
                            ocn_south_ext=c["ext"], clip_method="great_circle")


@pytest.mark.parametrize("split,asyn", SETTINGS, ids=IDS)
@pytest.mark.parametrize("which", ["ocean", "land"])
def test_coupler_with_a_cell_that_is_not_convex(fg, gpu_ok, which, split, asyn):
    """CouplerMosaic(clip_method="great_circle"): a displaced ocean corner fails in the atmosphere x ocean, polygon x ocean and
    land x ocean searches, a displaced land corner already in the atmosphere x land search; code and text are those of the
    restatement's first fatal clip.  A second mosaic on the clean grids then equals the _cr restatement of own_c4."""
    import test_gpu_coupler_gc as tg
    clean, broken = pc.cached(("gc_fatal_coupler", which), lambda: _coupler_case(fg, which))
    code = pc.cached(("gc_fatal_coupler_code", which), lambda: _restatement_error(broken))
    assert code in (1, 2)
    c, r = cg.reference_of("own_c4", fg, pc.prims_oracle(True))
    with _settings(fg, split, asyn):
        for _ in range(2):
            with _mosaic(fg, broken) as m:
                with pytest.raises(fg.FregridHipError) as e:
                    m.run()
            assert e.value.code == gf.FG_ERR_GEOM and str(e.value) == _text(code), str(e.value)
            with _mosaic(fg, clean) as m:
                m.run()
                tg._compare(m, c, r)
