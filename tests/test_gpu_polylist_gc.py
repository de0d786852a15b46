"""The great-circle polygon-list plan (fg_plan_create_polylist_gc: source cells are convex polygons of 3..8 unit-vector vertices,
every pair through the n-gon x quad clip k_gc_clip_poly) against the _cr oracle pair by pair: orc_clip_2dx2d_great_circle(cr=True)
plus orc_great_circle_area(cr=True), brute force over every (polygon, cell) pair the clip's own range test lets through
(tests/polylist_gc_cases.py).  Exchange cells in polygon-major, cell-ascending order; vertex counts, vertices, areas and the
destination cells' areas BIT-IDENTICAL, no tolerance.  The _cr oracle is tied to the compiled reference on the CPU
(tests/test_polylist_gc_cpu.py)."""
import numpy as np
import pytest

import polylist_gc_cases as pc

pytestmark = pytest.mark.gpu
FG_ERR_ARG, FG_ERR_MAXV = -1, -3


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_plan(plan, ref, dst):
    assert plan.nxgrid == len(ref["poly"])
    x = plan.get_xgrid()
    assert np.array_equal(x["i_in"], ref["poly"]) and not x["j_in"].any() and not x["t_in"].any()
    assert np.array_equal(x["j_out"].astype(np.int64) * dst.nx + x["i_out"], ref["cell"])      # polygon-major, cells ascending
    nd = int(np.count_nonzero(_bits(x["area"]) != _bits(ref["area"])))
    assert nd == 0, f"{nd} of {plan.nxgrid} areas differ from the _cr oracle"
    pg = plan.get_polygons(16)
    assert np.array_equal(pg["n"], ref["nv"])
    for k, ax in enumerate("xyz"):
        nd = int(np.count_nonzero(_bits(pg[ax]) != _bits(ref["verts"][:, :, k])))
        assert nd == 0, f"{nd} vertex {ax} values differ from the _cr oracle"


def _own_c4(fg):
    def make():
        c = pc.own_c4(fg)
        P = pc.prims_oracle(True)
        r = pc.remembered_polygons(c["atm"], c["lnd"], P)
        return c, r, pc.polylist_reference(r["n"], r["xyz"], r["area_ref"], c["ocn"], P)
    return pc.cached("own_c4_cr", make)


def _crafted(fg):
    """the crafted batch without the kinds on which the reference's clip ends the process (the plain oracle, pinned to the compiled
    reference, returns its negative code there): (dst, kinds kept, dropped, n, xyz, area_ref, _cr reference).  What the device
    says about polygons of that kind is tests/test_gpu_gc_fatal.py's subject (inputs: tests/gc_fatal_cases.py)."""
    def make():
        dst, kinds, n, xyz = pc.crafted(fg)
        plain = pc.prims_oracle(False)
        bad = pc.polylist_reference(n, xyz, np.ones(len(n)), dst, plain)["errors"]
        keep = [k for k in range(len(n)) if k not in bad]
        n, xyz = n[keep], xyz[keep]
        P = pc.prims_oracle(True)
        area_ref = np.array([pc.own_area(xyz[k, :n[k]], P) for k in range(len(n))])
        return dst, [kinds[k] for k in keep], [kinds[k] for k in bad], n, xyz, area_ref, pc.polylist_reference(n, xyz, area_ref, dst, P)
    return pc.cached("crafted_cr", make)


def _grid(fg, g):
    return fg.GridConfig(g.nx, g.ny, g.lon, g.lat)


def test_remembered_polygons_of_own_c4_against_its_ocean(fg, gpu_ok):
    c, r, ref = _own_c4(fg)
    assert r["cover"].get(3, 0) >= 1 and sum(v for k, v in r["cover"].items() if k >= 6) >= 1, r["cover"]     # both ends of the n-gon path
    assert not ref["errors"] and len(ref["poly"]) > 1000
    plan = fg.XgridPlan.create_polylist_gc(r["n"], r["xyz"][:, :, 0], r["xyz"][:, :, 1], r["xyz"][:, :, 2], r["area_ref"], _grid(fg, c["ocn"]))
    _check_plan(plan, ref, c["ocn"])
    a_in, a_out = plan.get_cell_area(c["ocn"].nx * c["ocn"].ny)
    assert np.array_equal(_bits(a_in), _bits(r["area_ref"]))
    assert np.array_equal(_bits(a_out), _bits(ref["area_dst"]))                     # get_grid_great_circle_area, pole cells included
    s = plan.stats()
    assert s["nxgrid"] == len(ref["poly"]) and s["pairs"] >= s["nonempty"] >= s["nxgrid"]
    plan.destroy()


def test_crafted_batch(fg, gpu_ok):
    dst, kinds, dropped, n, xyz, area_ref, ref = _crafted(fg)
    assert len(dropped) <= 1, f"the reference's clip ends the process on {dropped}"
    assert not ref["errors"]
    per_kind = {name: int(np.count_nonzero(ref["poly"] == k)) for k, name in enumerate(kinds)}
    assert per_kind.get("antipodal", 0) == 0                                        # opposite the grid: no cell
    assert all(v > 0 for name, v in per_kind.items() if name != "antipodal"), per_kind
    assert max(ref["cover"]) == 8                                                   # the 8-gon inside one cell comes back whole
    plan = fg.XgridPlan.create_polylist_gc(n, xyz[:, :, 0], xyz[:, :, 1], xyz[:, :, 2], area_ref, _grid(fg, dst))
    _check_plan(plan, ref, dst)
    plan.destroy()


def test_device_array_entry_matches_the_host_entry(fg, gpu_ok):
    """fg_plan_create_polylist_gc_dev on torch tensors (the destination's unit vectors from the host latlon2xyz): the same plan; a
    polygon of 9 vertices, which only the record kernel can see there, is FG_ERR_MAXV through the error word"""
    import torch
    c, r, ref = _own_c4(fg)
    o = c["ocn"]
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xyz_out = [t(v) for v in fg.latlon2xyz(o.lon, o.lat)]
    n_t, ar_t = t(r["n"]), t(r["area_ref"])
    v_t = [t(r["xyz"][:, :, k]) for k in range(3)]
    torch.cuda.synchronize()
    plan = fg.XgridPlan.create_polylist_gc_dev(n_t, v_t[0], v_t[1], v_t[2], ar_t, o.nx, o.ny, xyz_out)
    _check_plan(plan, ref, o)
    plan.destroy()
    n9 = r["n"].copy()
    n9[5] = 9
    with pytest.raises(fg.FregridHipError) as e:
        fg.XgridPlan.create_polylist_gc_dev(t(n9), v_t[0], v_t[1], v_t[2], ar_t, o.nx, o.ny, xyz_out)
    assert e.value.code == FG_ERR_MAXV


def test_nine_vertices_is_an_argument_error(fg, gpu_ok):
    dst, kinds, dropped, n, xyz, area_ref, ref = _crafted(fg)
    n9 = n.copy()
    n9[1] = 9
    with pytest.raises(fg.FregridHipError) as e:
        fg.XgridPlan.create_polylist_gc(n9, xyz[:, :, 0], xyz[:, :, 1], xyz[:, :, 2], area_ref, _grid(fg, dst))
    assert e.value.code == FG_ERR_ARG


def test_plans_of_no_polygon_and_of_one(fg, gpu_ok):
    dst, kinds, dropped, n, xyz, area_ref, ref = _crafted(fg)
    empty = fg.XgridPlan.create_polylist_gc(np.zeros(0, dtype=np.int32), np.zeros((0, 8)), np.zeros((0, 8)), np.zeros((0, 8)), np.zeros(0), _grid(fg, dst))
    assert empty.nxgrid == 0 and len(empty.get_xgrid()["area"]) == 0
    empty.destroy()
    k = kinds.index("octagon")
    sel = ref["poly"] == k
    one = {key: ref[key][sel] for key in ("cell", "nv", "verts", "area")}
    one["poly"] = np.zeros(int(sel.sum()), dtype=np.int64)
    plan = fg.XgridPlan.create_polylist_gc(n[k:k + 1], xyz[k:k + 1, :, 0], xyz[k:k + 1, :, 1], xyz[k:k + 1, :, 2], area_ref[k:k + 1], _grid(fg, dst))
    _check_plan(plan, one, dst)
    plan.destroy()
