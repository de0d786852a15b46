"""The restatement of fregrid's conservative interpolation (oracle/xgrid_oracle.c: orc_setup_conserve_interp,
orc_do_scalar_conserve_interp_ex) against the reference's own tools/fregrid/conserve_interp.c compiled in place
(oracle/_ref/libconserve_ref.so, oracle/conserve_ref_adapter.c).  Both sides are host C over the same libm: exchange-cell
lists identical, area / di / dj / remapped fields bit-identical.  The GPU sweep tests compare the device with the
restatement; this file pins the restatement itself, so a misreading shared by both cannot pass unseen."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.skipif(not orc.conserve_ref_available(),
                                reason="oracle/_ref/libconserve_ref.so not built (needs the reference sources)")
HERE = os.path.dirname(os.path.abspath(__file__))
MISSING = 1.0e20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------ grids
def _cube(fg, ni, tiles=range(6)):
    lon, lat = fg.gnomonic_ed_corners(ni)
    return [(ni, ni, lon[t], lat[t]) for t in tiles]


def _latlon(fg, nlon, nlat, *window):
    lo, la = fg.latlon_corners(nlon, nlat, *window)
    return [(nlon, nlat, lo, la)]


def grids(fg, name):
    """(source tiles, destination tiles) of each setup case; every case stays below ~1e8 candidate cell pairs."""
    if name == "c24_to_72x36":
        return _cube(fg, 24), _latlon(fg, 72, 36)
    if name == "c24_to_regional":            # lon 30..130, lat -20..50: partly covered source cells (AREA_RATIO fallback)
        return _cube(fg, 24), _latlon(fg, 50, 35, 30.0, 130.0, -20.0, 50.0)
    if name == "latlon_to_cube6":            # ntiles_out = 6: jstart/jend window per tile, cell sums over every output tile
        return _latlon(fg, 48, 24), _cube(fg, 10)
    if name == "tripolar_to_cube":
        lo, la = fg.tripolar_corners(60, 40)
        return [(60, 40, lo, la)], _cube(fg, 8, (0, 2, 5))
    if name == "c12_to_0.5deg":              # two source tiles (equatorial, polar) x 259200 destination cells
        return _cube(fg, 12, (0, 2)), _latlon(fg, 720, 360)
    if name == "c48_to_10deg":
        return _cube(fg, 48), _latlon(fg, 36, 18)
    raise KeyError(name)


SETUP_CASES = [(name, order) for name in ("c24_to_72x36", "c24_to_regional", "latlon_to_cube6", "tripolar_to_cube",
                                          "c12_to_0.5deg", "c48_to_10deg") for order in (1, 2)]


def orc_setup_gc(gin, gout, cr=False):
    """The restatement's great-circle setup, composed the way conserve_interp.c:164-168 searches: whole source tiles, one
    create_xgrid_great_circle per (destination tile, source tile), t_in = source tile.  cr: gc_oracle.c's build with the device's
    arc cosine."""
    keys = ("t_in", "i_in", "j_in", "i_out", "j_out", "area")
    parts, xoff = {k: [] for k in keys}, [0]
    for (nx2, ny2, lo2, la2) in gout:
        for m, (nx1, ny1, lo1, la1) in enumerate(gin):
            x = orc.orc_create_xgrid_gc(nx1, ny1, nx2, ny2, lo1, la1, lo2, la2, cr=cr)
            x["t_in"] = np.full(x["n"], m, dtype=np.int32)
            for k in keys:
                parts[k].append(x[k])
        xoff.append(sum(len(a) for a in parts["area"]))
    out = {k: np.concatenate(v) for k, v in parts.items()}
    out.update(n=xoff[-1], xoff=np.array(xoff), cell_area_in=[orc.orc_get_grid_gc_area(*g, cr=cr) for g in gin],
               cell_area_out=[orc.orc_get_grid_gc_area(*g, cr=cr) for g in gout])
    return out


def check_setup_equal(r, o, order):
    assert r["n"] == o["n"] > 0
    assert np.array_equal(r["xoff"], o["xoff"])
    for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
        assert np.array_equal(r[k], o[k]), k
    for k in ("area", "di", "dj") if order == 2 else ("area",):
        assert _same_bits(r[k], o[k]), (k, int(np.count_nonzero(_bits(r[k]) != _bits(o[k]))))
    for a, b in zip(r["cell_area_in"], o["cell_area_in"]):
        assert _same_bits(a, b)


@pytest.mark.parametrize("name,order", SETUP_CASES, ids=[f"{n}-order{o}" for n, o in SETUP_CASES])
def test_setup_matches_reference(fg, name, order):
    gin, gout = grids(fg, name)
    r = orc.cref_setup(order, gin, gout)
    o = orc.orc_setup(order, gin, gout)
    check_setup_equal(r, o, order)
    for a, g in zip(r["cell_area_out"], gout):
        assert _same_bits(a, orc.orc_get_grid_area(*g))
    if name == "c24_to_regional" and order == 2:
        # the window leaves source cells partly covered: their centroid comes from the whole cell (AREA_RATIO branch)
        ca = np.zeros(sum(g[0] * g[1] for g in gin))
        base = np.cumsum([0] + [g[0] * g[1] for g in gin])
        np.add.at(ca, base[r["t_in"]] + r["j_in"].astype(np.int64) * gin[0][0] + r["i_in"], r["area"])
        full = np.concatenate(r["cell_area_in"])
        touched = ca > 0
        assert np.count_nonzero(np.abs(ca[touched] - full[touched]) / full[touched] >= 1e-3) > 10


@pytest.mark.parametrize("name", ["c24_to_72x36", "tripolar_to_cube"])
def test_setup_great_circle_matches_reference(fg, name):
    gin, gout = grids(fg, name)
    r = orc.cref_setup(1, gin, gout, great_circle=True)
    o = orc_setup_gc(gin, gout)
    check_setup_equal(r, o, 1)
    for a, b in zip(r["cell_area_out"], o["cell_area_out"]):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------------------------ sweep
class Case:
    def __init__(self, order, nz=1, missing=None, weight=None, sum=False, meas=False, target=False, mono=False,
                 volume=False, gmask=False, check=False, grid="c24_to_72x36"):
        self.__dict__.update(order=order, nz=nz, missing=missing, weight=weight, sum=sum, meas=meas, target=target,
                             mono=mono, volume=volume, gmask=gmask, check=check, grid=grid)


def _id(c):
    parts = [f"o{c.order}", f"nz{c.nz}"]
    if c.missing:
        parts.append("missing-" + c.missing)
    if c.weight:
        parts.append("weight-" + c.weight)
    for flag, word in ((c.sum, "sum"), (c.meas, "cell_measures"), (c.target, "target"), (c.volume, "use_volume"),
                       (c.mono, "monotonic"), (c.gmask, "grad_mask"), (c.check, "check_conserve")):
        if flag:
            parts.append(word)
    if c.grid != "c24_to_72x36":
        parts.append(c.grid)
    return "-".join(parts)


SWEEP_CASES = [
    # the GPU suite's EX_CASES matrix (test_gpu_pipeline.py) as the floor
    Case(1), Case(2, 3), Case(1, 3, weight="random"), Case(2, 2, weight="random", target=True),
    Case(1, missing="pattern", weight="random", sum=True), Case(2, missing="pattern", sum=True),
    Case(1, missing="pattern", meas=True, target=True), Case(2, missing="pattern", weight="random", meas=True),
    Case(2, meas=True, target=True), Case(2, mono=True), Case(2, missing="pattern", weight="random", mono=True),
    Case(2, missing="pattern", sum=True, mono=True), Case(2, meas=True, target=True, mono=True),
    # plain branches at nz 1, 3, 8
    Case(1, 8), Case(2), Case(2, 8), Case(1, 3, target=True), Case(2, 8, weight="random", target=True),
    # missing sources: destination cells covered only by missing sources (-> missing) or only by zero-weight valid ones
    # (-> 0.0): the out_miss rule of the mean and of the sum normalisation
    Case(1, missing="block", weight="zero_block"), Case(2, missing="block", weight="zero_block"),
    Case(1, missing="block", weight="zero_block", sum=True), Case(2, missing="block", weight="zero_block", sum=True),
    Case(1, missing="block", sum=True), Case(2, missing="block", meas=True, target=True),
    # cell_measures alone, TARGET with and without it, use_volume switching TARGET off
    Case(1, meas=True), Case(2, missing="pattern", meas=True), Case(1, target=True), Case(2, target=True),
    Case(1, meas=True, target=True, volume=True), Case(2, 3, target=True, volume=True),
    # monotone limiter: active, missing halo neighbours, grad_mask, nz > 1 (level 0 only), with weight / measures
    Case(2, mono=True, gmask=True), Case(2, missing="halo", mono=True), Case(2, missing="halo", mono=True, gmask=True),
    Case(2, 3, mono=True), Case(2, missing="pattern", meas=True, target=True, mono=True),
    Case(2, missing="halo", gmask=True),
    # CHECK_CONSERVE: the sums the reference prints
    Case(1, check=True), Case(2, 3, check=True), Case(1, missing="pattern", meas=True, check=True),
    Case(2, missing="block", sum=True, check=True), Case(2, mono=True, check=True),
    # other grids: several destination tiles, the regional window, a tripolar source
    Case(1, missing="block", weight="zero_block", grid="latlon_to_cube6"), Case(2, 3, grid="latlon_to_cube6"),
    Case(2, mono=True, target=True, grid="latlon_to_cube6"), Case(2, missing="pattern", meas=True, grid="c24_to_regional"),
    Case(2, mono=True, grid="c24_to_regional"), Case(1, missing="block", sum=True, check=True, grid="tripolar_to_cube"),
    Case(2, missing="pattern", weight="random", target=True, grid="tripolar_to_cube"),
]

_SETUPS = {}


def reference_setup(fg, grid, order):
    key = (grid, order)
    if key not in _SETUPS:
        gin, gout = grids(fg, grid)
        _SETUPS[key] = (gin, gout, orc.cref_setup(order, gin, gout))
    return _SETUPS[key]


def sweep_inputs(fg, c, seed=0):
    """Fields and options of one case, in the layouts of orc_apply_ex / cref_apply (per source tile, flat)."""
    from gridutil import cell_centres
    gin, gout, x = reference_setup(fg, c.grid, c.order)
    rng = np.random.default_rng(seed + 101 * c.order + 7 * c.nz)
    h = 1 if c.order == 2 else 0
    kw = dict(nx_in=[g[0] for g in gin], ny_in=[g[1] for g in gin], nz=c.nz, has_missing=c.missing is not None,
              missing=MISSING if c.missing else -1.0e20, cell_area_in=x["cell_area_in"], area_missing=-1.0e20)
    data, gx, gy, gm, w, fa = [], [], [], [], [], []
    for t, (nx, ny, lo, la) in enumerate(gin):
        clon, clat = cell_centres(np.asarray(lo).reshape(ny + 1, nx + 1), np.asarray(la).reshape(ny + 1, nx + 1))
        d = rng.standard_normal((c.nz, ny + 2 * h, nx + 2 * h)) + 5.0
        g1 = rng.standard_normal((c.nz, ny, nx)) * (4.0 if c.mono else 1.0)     # steep enough for the limiter to act
        g2 = rng.standard_normal((c.nz, ny, nx)) * (4.0 if c.mono else 1.0)
        core = d[0, h:h + ny, h:h + nx]
        if c.missing == "pattern":
            d[0][(np.add.outer(np.arange(ny + 2 * h), np.arange(nx + 2 * h)) % 10) == 0] = MISSING
        elif c.missing == "block":
            core[clat > np.deg2rad(55.0)] = MISSING
        elif c.missing == "halo":                      # missing cells next to valid ones, inside the halo ring too
            d[0][(np.add.outer(3 * np.arange(ny + 2 * h), np.arange(nx + 2 * h)) % 7) == 0] = MISSING
        data.append(d.reshape(c.nz, -1))
        gx.append(g1.reshape(c.nz, -1))
        gy.append(g2.reshape(c.nz, -1))
        m = np.zeros((ny, nx), dtype=np.int32)
        if c.gmask or c.missing:
            m = ((np.add.outer(np.arange(ny), 2 * np.arange(nx)) % 5) == 0).astype(np.int32)
        gm.append(m)
        wt = rng.uniform(0.2, 1.0, (ny, nx))
        if c.weight == "zero_block":
            wt[(clat > np.deg2rad(20.0)) & (clat < np.deg2rad(40.0))] = 0.0
        w.append(wt)
        fa.append(np.asarray(x["cell_area_in"][t]).reshape(ny, nx) * rng.uniform(0.3, 1.0, (ny, nx)))
    kw.update(data=data, grad_x=gx if c.order == 2 else None, grad_y=gy if c.order == 2 else None,
              grad_mask=gm if c.order == 2 else None, weight=w if c.weight else None, cell_methods_sum=c.sum,
              field_area=fa if c.meas else None)
    return gin, gout, x, kw


def _tile(x, n):
    s = slice(int(x["xoff"][n]), int(x["xoff"][n + 1]))
    return {k: x[k][s] for k in ("t_in", "i_in", "j_in", "i_out", "j_out", "area", "di", "dj") if k in x}


def orc_sweep(c, gin, gout, x, kw):
    """orc_apply_ex once per destination tile.  TARGET is off under use_volume (conserve_interp.c:536): the restatement
    leaves that rule to its caller.  Returns (outs, gsum_out over the tiles, gsum_in)."""
    outs, gs = [], 0.0
    target = c.target and not c.volume
    for n, (nx2, ny2, _, _) in enumerate(gout):
        rc, out, g = orc.orc_apply_ex(c.order, _tile(x, n), kw["nx_in"], kw["ny_in"], kw["data"], kw["grad_x"], kw["grad_y"],
                                      kw["grad_mask"], kw["has_missing"], kw["missing"], nx2, ny2, c.nz, weight=kw["weight"],
                                      cell_methods_sum=c.sum, field_area=kw["field_area"], area_missing=kw["area_missing"],
                                      cell_area_in=kw["cell_area_in"], target_grid=target,
                                      cell_area_out=x["cell_area_out"][n] if target else None, monotonic=c.mono)
        assert rc == 0, orc.ORC_APPLY_ERRORS.get(rc, rc)
        outs.append(out)
        gs += g
    L = orc.oracle()
    nxi, nyi = (np.asarray(kw[k], dtype=np.int32) for k in ("nx_in", "ny_in"))
    pa = lambda v: orc._ptr_array([orc.f64(a).ravel() for a in v]) if v is not None else None
    gsum_in = L.orc_gsum_in_ex(c.order, len(gin), orc._ip(nxi), orc._ip(nyi), pa(kw["data"]), pa(kw["cell_area_in"]),
                               pa(kw["field_area"]), 1 if c.sum else 0, 1 if kw["has_missing"] else 0, kw["missing"], c.nz)
    return outs, gs, gsum_in


def cref_sweep(c, gin, gout, x, kw):
    return orc.cref_apply(c.order, x, kw["nx_in"], kw["ny_in"], kw["data"], kw["grad_x"], kw["grad_y"], kw["grad_mask"],
                          kw["has_missing"], kw["missing"], [g[0] for g in gout], [g[1] for g in gout], c.nz,
                          weight=kw["weight"], cell_methods_sum=c.sum, field_area=kw["field_area"],
                          area_missing=kw["area_missing"], cell_area_in=kw["cell_area_in"], target_grid=c.target,
                          cell_area_out=x["cell_area_out"], monotonic=c.mono, use_volume=c.volume, check_conserve=c.check)


@pytest.mark.parametrize("c", SWEEP_CASES, ids=[_id(c) for c in SWEEP_CASES])
def test_sweep_matches_reference(fg, c):
    gin, gout, x, kw = sweep_inputs(fg, c)
    ref, printed = cref_sweep(c, gin, gout, x, kw)
    got, gsum_out, gsum_in = orc_sweep(c, gin, gout, x, kw)
    for n, (a, b) in enumerate(zip(got, ref)):
        assert _same_bits(a, b), (n, int(np.count_nonzero(_bits(a) != _bits(b))), a.size)
    # the case exercises what its name says
    allout = np.concatenate(ref)
    if c.missing == "block":
        assert np.any(allout == kw["missing"])
    if c.weight == "zero_block" and c.missing == "block" and not c.sum:
        assert np.any(allout == 0.0)                 # out_area == 0 with out_miss == 1
    if c.check:
        line = [s for s in printed.splitlines() if s.startswith("the flux(data*area) sum of cref")]
        assert len(line) == 1, printed
        assert line[0] == "the flux(data*area) sum of cref: input = %g, output = %g, diff = %g. " % (
            gsum_in, gsum_out, gsum_out - gsum_in)
    else:
        assert "flux" not in printed


def test_monotone_limiter_acts(fg):
    """The monotone cases above are not vacuous: the limited field differs from the plain second-order one."""
    c = Case(2, mono=True)
    gin, gout, x, kw = sweep_inputs(fg, c)
    mono, _ = cref_sweep(c, gin, gout, x, kw)
    c.mono = False
    plain, _ = cref_sweep(c, gin, gout, x, kw)
    assert np.count_nonzero(mono[0] != plain[0]) > 100


# ------------------------------------------------------------------------------------------------------------------ fatal
FATAL_CASES = [
    ("nz2_has_missing", Case(1, 2, missing="pattern"), -1),
    ("nz2_cell_measures", Case(2, 2, meas=True), -5),
    ("nz3_sum", Case(1, 3, sum=True), -6),
    ("area_missing_o1", Case(1, missing="pattern", meas=True), -2),
    ("area_missing_o2", Case(2, missing="pattern", meas=True), -2),
]

_CHILD = """
import sys
sys.path.insert(0, {here!r})
import pickle, orc
args, kw = pickle.load(open({path!r}, "rb"))
orc.cref_apply(*args, **kw)
print("returned")
"""


@pytest.mark.parametrize("name,c,code", FATAL_CASES, ids=[f[0] for f in FATAL_CASES])
def test_fatal_checks_match_reference(fg, tmp_path, name, c, code):
    """The reference's data checks end its process through mpp_error (exit 1): run it in a child.  The restatement returns
    the check's code, whose message is the reference's."""
    gin, gout, x, kw = sweep_inputs(fg, c)
    if c.meas and c.nz == 1:                         # a missing cell_measures area under valid data
        t = len(gin) - 1
        h = c.order - 1
        nx, ny = gin[t][0], gin[t][1]
        core = kw["data"][t][0].reshape(ny + 2 * h, nx + 2 * h)[h:h + ny, h:h + nx].ravel()
        sel = x["t_in"] == t
        used = set((x["j_in"][sel].astype(np.int64) * nx + x["i_in"][sel]).tolist())
        k = next(v for v in np.nonzero(core != MISSING)[0] if int(v) in used)
        kw["field_area"][t] = kw["field_area"][t].copy()
        kw["field_area"][t].ravel()[k] = kw["area_missing"]
    rc, _, _ = orc.orc_apply_ex(c.order, _tile(x, 0), kw["nx_in"], kw["ny_in"], kw["data"], kw["grad_x"], kw["grad_y"],
                                kw["grad_mask"], kw["has_missing"], kw["missing"], gout[0][0], gout[0][1], c.nz,
                                weight=kw["weight"], cell_methods_sum=c.sum, field_area=kw["field_area"],
                                area_missing=kw["area_missing"], cell_area_in=kw["cell_area_in"])
    assert rc == code
    path = str(tmp_path / "case.pkl")
    xs = {k: v for k, v in x.items() if k not in ("cell_area_in", "cell_area_out")}
    args = [c.order, xs, kw["nx_in"], kw["ny_in"], kw["data"], kw["grad_x"], kw["grad_y"], kw["grad_mask"],
            kw["has_missing"], kw["missing"], [g[0] for g in gout], [g[1] for g in gout], c.nz]
    with open(path, "wb") as f:
        pickle.dump((args, dict(weight=kw["weight"], cell_methods_sum=c.sum, field_area=kw["field_area"],
                                area_missing=kw["area_missing"], cell_area_in=kw["cell_area_in"],
                                cell_area_out=x["cell_area_out"])), f)
    p = subprocess.run([sys.executable, "-c", _CHILD.format(here=HERE, path=path)], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 1, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    assert "returned" not in p.stdout
    assert "Error from pe 0: " + orc.ORC_APPLY_ERRORS[code] in p.stderr, p.stderr[-500:]
