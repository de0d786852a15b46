"""The device path against the reference's own conserve_interp.c directly (oracle/_ref/libconserve_ref.so), without the
restatement in between: the Python mirror's setup_conserve_interp (device search + centroid pass) and
do_scalar_conserve_interp (device sweep) against the reference's setup_conserve_interp + do_scalar_conserve_interp on the
grids of tests/test_conserve_interp_vs_ref.py and one case per sweep branch.

Tolerances are the suite's: the legacy path is bit-identical where the host libm runs its FMA build (orc.host_has_fma),
1e-10 relative otherwise.  The great-circle path has identical index lists and areas within 1e-10 of the reference's (a few
carry last-place differences from glibc's acosl, see test_gpu_great_circle.py); a remapped value is bit-identical unless one of
its exchange cells has such an area, and then within the same 1e-10.  Against the oracle that rounds like the device
(gc_oracle.c's _cr build, pinned in tests/test_gc_oracle_cr_cpu.py) every great-circle area and cell area is bit-identical."""
import numpy as np
import pytest

import orc
from test_conserve_interp_vs_ref import Case, _id, grids, orc_setup_gc, sweep_inputs

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not orc.conserve_ref_available(), reason="oracle/_ref/libconserve_ref.so not built")]
RTOL = 1e-10


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def close(a, b, rtol=RTOL, scale=None):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape
    if rtol is None:
        return np.array_equal(_bits(a), _bits(b))
    s = np.abs(b) if scale is None else scale
    return bool(np.all(np.abs(a - b) <= rtol * s))


def legacy_close(a, b, scale=None):
    return close(a, b, None) if orc.host_has_fma() else close(a, b, RTOL, scale)


def mirror_setup(fg, order, gin, gout, great_circle=False):
    grid_in = [fg.GridConfig(nx, ny, lo, la) for (nx, ny, lo, la) in gin]
    grid_out = [fg.GridConfig(nx, ny, lo, la) for (nx, ny, lo, la) in gout]
    interp = [fg.InterpConfig() for _ in gout]
    opcode = (fg.CONSERVE_ORDER2 if order == 2 else fg.CONSERVE_ORDER1) | (fg.GREAT_CIRCLE if great_circle else 0)
    fg.setup_conserve_interp(len(gin), grid_in, len(gout), grid_out, interp, opcode)
    return grid_in, grid_out, interp


def check_setup(fg, order, gin, gout, r, grid_in, grid_out, interp, great_circle=False):
    for n, ic in enumerate(interp):
        s = slice(int(r["xoff"][n]), int(r["xoff"][n + 1]))
        assert ic.nxgrid == s.stop - s.start, n
        if ic.nxgrid == 0:
            continue
        for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(getattr(ic, k), r[k][s]), (n, k)
        if great_circle:
            assert close(ic.area, r["area"][s])
        else:
            assert legacy_close(ic.area, r["area"][s])
        if order == 2:
            for k, ref_k in (("di_in", "di"), ("dj_in", "dj")):
                # d crosses zero; outside FMA hosts judge the weight area*d on its own scale (test_gpu_pipeline.check_xgrid)
                w_ref = r[ref_k][s] * r["area"][s]
                if orc.host_has_fma():
                    assert close(getattr(ic, k), r[ref_k][s], None), (n, k)
                else:
                    assert close(getattr(ic, k) * ic.area, w_ref, RTOL, RTOL * np.max(np.abs(w_ref))), (n, k)
    for g, a in zip(grid_in, r["cell_area_in"]):
        assert close(g.cell_area, a) if great_circle else legacy_close(g.cell_area, a)
    for g, a in zip(grid_out, r["cell_area_out"]):
        assert close(g.cell_area, a) if great_circle else legacy_close(g.cell_area, a)


GRIDS = ["c24_to_72x36", "c24_to_regional", "latlon_to_cube6", "tripolar_to_cube", "c12_to_0.5deg", "c48_to_10deg"]


@pytest.mark.parametrize("name,order", [(n, o) for n in GRIDS for o in (1, 2)],
                         ids=[f"{n}-order{o}" for n in GRIDS for o in (1, 2)])
def test_setup_vs_reference(fg, gpu_ok, name, order):
    gin, gout = grids(fg, name)
    r = orc.cref_setup(order, gin, gout)
    grid_in, grid_out, interp = mirror_setup(fg, order, gin, gout)
    check_setup(fg, order, gin, gout, r, grid_in, grid_out, interp)


@pytest.mark.parametrize("name", ["c24_to_72x36", "tripolar_to_cube"])
def test_setup_great_circle_vs_reference(fg, gpu_ok, name):
    gin, gout = grids(fg, name)
    r = orc.cref_setup(1, gin, gout, great_circle=True)
    grid_in, grid_out, interp = mirror_setup(fg, 1, gin, gout, great_circle=True)
    check_setup(fg, 1, gin, gout, r, grid_in, grid_out, interp, great_circle=True)
    # against the oracle that rounds like the device (gc_oracle.c's _cr build), tile by tile: every area and cell area in bits
    ocr = orc_setup_gc(gin, gout, cr=True)
    assert np.array_equal(ocr["xoff"], r["xoff"])
    for n, ic in enumerate(interp):
        s = slice(int(ocr["xoff"][n]), int(ocr["xoff"][n + 1]))
        assert np.array_equal(ic.t_in, ocr["t_in"][s]) and np.array_equal(ic.i_in, ocr["i_in"][s]) and np.array_equal(ic.j_out, ocr["j_out"][s])
        nd = int(np.count_nonzero(_bits(ic.area) != _bits(ocr["area"][s])))
        assert nd == 0, f"destination tile {n}: {nd} of {ic.nxgrid} exchange-cell areas differ from the _cr oracle"
    for which, gs, areas in (("source", grid_in, ocr["cell_area_in"]), ("destination", grid_out, ocr["cell_area_out"])):
        for t, (g, a) in enumerate(zip(gs, areas)):
            nd = int(np.count_nonzero(_bits(g.cell_area) != _bits(a)))
            assert nd == 0, f"{which} tile {t}: {nd} of {a.size} cell areas differ from the _cr oracle"
    # a field through the mirror's great-circle sweep against the reference's sweep over the reference's own lists
    _, _, _, kw = sweep_inputs(fg, Case(1, missing="pattern", grid=name))
    ref, _ = orc.cref_apply(1, r, kw["nx_in"], kw["ny_in"], kw["data"], None, None, None, True, kw["missing"],
                            [g[0] for g in gout], [g[1] for g in gout], 1, cell_area_in=r["cell_area_in"],
                            cell_area_out=r["cell_area_out"])
    var = fg.VarConfig(name="cref", interp_method=fg.CONSERVE_ORDER1, has_missing=1, missing=kw["missing"])
    field_in = [fg.FieldConfig(data=kw["data"][t].reshape(1, g[1], g[0]), var=[var]) for t, g in enumerate(gin)]
    field_out = [fg.FieldConfig() for _ in gout]
    fg.do_scalar_conserve_interp(interp, 0, len(gin), grid_in, len(gout), grid_out, field_in, field_out, fg.CONSERVE_ORDER1, 1)
    for n in range(len(gout)):
        got = field_out[n].data.ravel()
        valid = ref[n] != kw["missing"]
        assert np.array_equal(got == kw["missing"], ~valid)
        # the sweep adds in the reference's order: a destination cell differs only where one of its exchange cells
        # carries an area off in the last places, and then by no more than that area's tolerance
        s = slice(int(r["xoff"][n]), int(r["xoff"][n + 1]))
        off = interp[n].area != r["area"][s]
        nx2 = gout[n][0]
        touched = np.zeros(got.size, dtype=bool)
        touched[r["j_out"][s][off].astype(np.int64) * nx2 + r["i_out"][s][off]] = True
        assert np.all(_bits(got)[~touched] == _bits(ref[n])[~touched])
        assert close(got[valid], ref[n][valid], RTOL)


GPU_SWEEP_CASES = [
    Case(1), Case(2, 3), Case(1, 8, weight="random"), Case(2, missing="pattern"),
    Case(1, missing="block", weight="zero_block"), Case(2, missing="block", weight="zero_block"),
    Case(1, missing="block", weight="zero_block", sum=True), Case(2, missing="pattern", sum=True),
    Case(2, missing="pattern", meas=True), Case(2, meas=True, target=True), Case(1, 3, target=True),
    Case(1, meas=True, target=True, volume=True),
    Case(2, mono=True), Case(2, mono=True, gmask=True), Case(2, missing="halo", mono=True, gmask=True),
    Case(2, missing="pattern", meas=True, target=True, mono=True),
    Case(2, 3, check=True), Case(1, missing="pattern", meas=True, check=True),
    Case(2, 3, grid="latlon_to_cube6"), Case(2, mono=True, target=True, grid="latlon_to_cube6"),
    Case(2, missing="pattern", meas=True, grid="c24_to_regional"),
    Case(1, missing="block", sum=True, grid="tripolar_to_cube"),
]

_MIRROR = {}


def mirror_plans(fg, grid, order):
    key = (grid, order)
    if key not in _MIRROR:
        gin, gout = grids(fg, grid)
        _MIRROR[key] = mirror_setup(fg, order, gin, gout)
    return _MIRROR[key]


@pytest.mark.parametrize("c", GPU_SWEEP_CASES, ids=[_id(c) for c in GPU_SWEEP_CASES])
def test_sweep_vs_reference(fg, gpu_ok, c, capsys):
    gin, gout, x, kw = sweep_inputs(fg, c)
    ref, printed = orc.cref_apply(c.order, x, kw["nx_in"], kw["ny_in"], kw["data"], kw["grad_x"], kw["grad_y"],
                                  kw["grad_mask"], kw["has_missing"], kw["missing"], [g[0] for g in gout],
                                  [g[1] for g in gout], c.nz, weight=kw["weight"], cell_methods_sum=c.sum,
                                  field_area=kw["field_area"], area_missing=kw["area_missing"],
                                  cell_area_in=kw["cell_area_in"], target_grid=c.target, cell_area_out=x["cell_area_out"],
                                  monotonic=c.mono, use_volume=c.volume, check_conserve=c.check)
    grid_in, grid_out, interp = mirror_plans(fg, c.grid, c.order)
    h = 1 if c.order == 2 else 0
    var = fg.VarConfig(name="cref", interp_method=fg.CONSERVE_ORDER2 if c.order == 2 else fg.CONSERVE_ORDER1,
                       has_missing=int(kw["has_missing"]), missing=kw["missing"], cell_measures=int(c.meas),
                       cell_methods=fg.CELL_METHODS_SUM if c.sum else fg.CELL_METHODS_MEAN, area_missing=kw["area_missing"],
                       use_volume=int(c.volume))
    field_in = []
    for t, (nx, ny, _, _) in enumerate(gin):
        f = fg.FieldConfig(data=kw["data"][t].reshape(c.nz, ny + 2 * h, nx + 2 * h), var=[var])
        if c.order == 2:
            f.grad_x = kw["grad_x"][t].reshape(c.nz, ny, nx)
            f.grad_y = kw["grad_y"][t].reshape(c.nz, ny, nx)
            f.grad_mask = kw["grad_mask"][t]
        if c.meas:
            f.area = kw["field_area"][t]
        field_in.append(f)
    for t, g in enumerate(grid_in):
        g.weight = kw["weight"][t] if c.weight else None
        g.weight_exist = 1 if c.weight else 0
    opcode = ((fg.CONSERVE_ORDER2 if c.order == 2 else fg.CONSERVE_ORDER1) | (fg.TARGET if c.target else 0) |
              (fg.MONOTONIC if c.mono else 0) | (fg.CHECK_CONSERVE if c.check else 0))
    field_out = [fg.FieldConfig() for _ in gout]
    capsys.readouterr()
    fg.do_scalar_conserve_interp(interp, 0, len(gin), grid_in, len(gout), grid_out, field_in, field_out, opcode, c.nz)
    mine = capsys.readouterr().out
    for t, g in enumerate(grid_in):
        g.weight, g.weight_exist = None, 0
    for n in range(len(gout)):
        got = field_out[n].data.ravel()
        assert np.array_equal(got == kw["missing"], ref[n] == kw["missing"]), n
        assert legacy_close(got, ref[n], scale=np.max(np.abs(ref[n][ref[n] != kw["missing"]]), initial=0.0)), \
            (n, int(np.count_nonzero(_bits(got) != _bits(ref[n]))))
    if c.check:
        pick = lambda s: [ln.split("output = ")[1].split(",")[0] for ln in s.splitlines() if "flux(data*area)" in ln]
        assert pick(mine) == pick(printed) and len(pick(printed)) == 1, (mine, printed)
