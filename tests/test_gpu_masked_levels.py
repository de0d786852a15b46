"""Fields with missing values, many levels per call (fg_plan_apply_levels, fg_c2l_records_levels + fg_plan_apply_records_levels,
fg_sweep_run_levels): level k of the output must be what the reference's do_scalar_conserve_interp(nz = 1, has_missing = 1)
gives on level k alone (conserve_interp.c:562-591, :744-783, :815-839; the level loop of fregrid.c:1045-1083).

Yardstick: the reference itself (oracle/_ref/libconserve_ref.so): orc.cref_setup for the exchange cells, which the plans take
through create_empty + set_xgrid, and orc.cref_apply once per level, its order-2 gradients and gradient masks from the CPU
oracle's one-level preparation (test_gpu_c2l.oracle_prepare).  Plan and reference hold the same exchange cells, so the
comparison is bit for bit where the suite asserts bit identity (orc.host_has_fma), 1e-10 relative otherwise; the equalities
between device paths are bit for bit everywhere.

Shapes (the smallest that reach each path of the masked k_apply_ep8g):
  short   C9 -> 30 x 15: rows of a few exchange cells, 32 rows per tile, 450 rows = 14 tiles and a partial one
  mid8    C9 -> 12 x 6, mid2: C9 -> 6 x 4: the tiles of 8 and 2 rows
  long    C24 -> 4 x 2: one row per tile, every row longer than the staging capacity (the chunk walk)
  empty   tile 1 of C9 alone -> global 30 x 15: most rows are empty
Masks are integer functions of (tile, j, i, level), see _depth / _missing_at.

No exchange cell of a real grid pair has area 0, so no row here has a counted cell under an area sum of 0: the middle outcome of
conserve_interp.c:815-839 (0.0 by the `touched` flag, against `missing` where no cell counted) is tested on the hand-made lists of
tests/sweep_cases.py, in tests/test_gpu_sweep_synthetic.py::test_apply_levels."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from test_gpu_c2l import oracle_prepare

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not orc.conserve_ref_available(), reason="oracle/_ref/libconserve_ref.so not built")]

FG_ERR_ARG = -1
DEV = "cuda:0"
NLEV = 17                     # levels of the shared reference; the tests sweep its first 1, 7, 8, 9, 17
LEVEL_COUNTS = (1, 7, 8, 9, 17)
K_FULL, K_NONE = 3, 5         # the level without a missing value and the level that is missing everywhere
MISSING = -1.0e10             # exact in float32 and float64
DEEP = 1000
SHAPES = {"short": (9, None, 30, 15), "mid8": (9, None, 12, 6), "mid2": (9, None, 6, 4), "long": (24, None, 4, 2),
          "empty": (9, 1, 30, 15)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ref_close(got, ref):
    """the suite's parity rule against the reference: bit-identical on an FMA host, 1e-10 relative otherwise; the missing
    pattern is identical either way"""
    got, ref = np.asarray(got).ravel(), np.asarray(ref).ravel()
    if not np.array_equal(got == MISSING, ref == MISSING):
        return False
    if orc.host_has_fma():
        return _same(got, ref)
    return bool(np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref)))


def _mosaic(fg, ni):
    lon, lat, lont, latt = fg.gnomonic_ed_grid(ni)
    nx, ny = [ni] * 6, [ni] * 6
    A = np.ascontiguousarray
    m = dict(nx=nx, ny=ny, lon=[A(lon[t]) for t in range(6)], lat=[A(lat[t]) for t in range(6)],
             lont=[A(lont[t]) for t in range(6)], latt=[A(latt[t]) for t in range(6)])
    m["contacts"] = fg.find_contacts(nx, ny, m["lon"], m["lat"])
    return m


def _halo_sources(fg, ni, contacts):
    """(tile, j, i) of the interior cell that update_halo copies into halo element (tile t, halo'd row r, halo'd column c), or
    None where no contact fills it (the cube's corners)"""
    off, hmap = fg.halo_map([ni] * 6, [ni] * 6, contacts)
    w = ni + 2

    def src(t, r, c):
        e = int(hmap[int(off[t]) + r * w + c])
        if e < 0:
            return None
        t2 = int(np.searchsorted(off, e, side="right")) - 1
        loc = e - int(off[t2])
        return t2, loc // w - 1, loc % w - 1
    return src


def _depth(fg, ni, contacts):
    """Bathymetry: depth[t][j][i] = the first level at which the cell is missing (DEEP: never).
      * every fifth cell is a sea mount of depth 0 .. 11: destination cells lose some of their exchange cells level by level
        (the renormalised case) and gradient masks change from level to level;
      * the low quarter of tile 3 is a shelf of depth 2 .. 4: destination cells inside it are valid near the surface and
        missing below;
      * two probes on tile 1, each with a 3 x 3 neighbourhood of deep water in its own tile: cell (j, i) = (ni // 2, 0) on
        the west edge, whose neighbour ACROSS THE EDGE, in another tile, is land (depth 0), and the corner cell (0, 0), whose
        neighbour in another tile of that cube corner falls dry at level 4.
    Returns (depth, probes): probes = dict(edge=(t, j, i), corner=(t, j, i))."""
    depth = np.full((6, ni, ni), DEEP, dtype=np.int64)
    c = np.arange(6 * ni * ni).reshape(6, ni, ni)
    mount = c % 5 == 2
    depth[mount] = (c[mount] // 5) % 12
    j, i = np.meshgrid(np.arange(ni), np.arange(ni), indexing="ij")
    shelf = (i < ni // 2) & (j < ni // 2)
    depth[3][shelf] = 2 + ((i + j) % 3)[shelf]
    src = _halo_sources(fg, ni, contacts)
    probes = dict(edge=(1, ni // 2, 0), corner=(1, 0, 0))
    for (t, pj, pi) in probes.values():
        depth[t, max(pj - 1, 0):pj + 2, max(pi - 1, 0):pi + 2] = DEEP
    for name, dry in (("edge", 0), ("corner", 4)):
        t, pj, pi = probes[name]
        s = src(t, pj + 1, 0)                       # the halo element west of the probe
        assert s is not None and s[0] != t, (name, s)
        depth[s] = dry
        # the other cells of that tile along the same edge stay wet, so that the probe's mask has this one cause
        for dj in (-1, 1):
            s2 = src(t, pj + 1 + dj, 0)
            if s2 is not None and s2[0] != t and s2 != s:
                depth[s2] = DEEP
    t, pj, pi = probes["corner"]                   # the corner probe's neighbours across the south edge stay wet as well
    for ci in (1, 2):
        s2 = src(t, 0, ci)
        if s2 is not None and s2 != src(t, 1, 0):
            depth[s2] = DEEP
    return depth, probes


def _missing_at(depth, k):
    if k % 17 == K_FULL:
        return np.zeros(depth.shape, dtype=bool)
    if k % 17 == K_NONE:
        return np.ones(depth.shape, dtype=bool)
    return depth <= k


def _values(ni, k):
    """exact in float32: 1 + quarter steps + 16 per level"""
    c = np.arange(6 * ni * ni, dtype=np.int64).reshape(6, ni, ni)
    return 1.0 + ((7 * c + 3 * k) % 13) * 0.25 + 16.0 * k


def _field(depth, ni, nlev):
    f = np.empty((nlev, 6, ni, ni))
    for k in range(nlev):
        f[k] = np.where(_missing_at(depth, k), MISSING, _values(ni, k))
    return f


def build_host(fg, name, order):
    """Everything of a case that needs no device: exchange cells and the per-level reference of the reference library."""
    ni, only, nlon, nlat = SHAPES[name]
    m = _mosaic(fg, ni)
    depth, probes = _depth(fg, ni, m["contacts"])
    f = _field(depth, ni, NLEV)                                      # [NLEV][6][ni][ni]
    tiles = [only] if only is not None else list(range(6))
    nx, ny = [ni] * len(tiles), [ni] * len(tiles)
    lo, la = fg.latlon_corners(nlon, nlat)
    x = orc.cref_setup(order, [(ni, ni, m["lon"][t], m["lat"][t]) for t in tiles], [(nlon, nlat, lo, la)])
    c = dict(name=name, order=order, ni=ni, tiles=tiles, nx=nx, ny=ny, nlon=nlon, nlat=nlat, x=x, m=m, depth=depth,
             probes=probes, ndst=nlon * nlat, ncell=len(tiles) * ni * ni)
    c["src"] = np.ascontiguousarray(f[:, tiles].reshape(NLEV, -1))   # [NLEV][ncell], unpadded
    if order == 2:
        # the preparation always sees the whole mosaic (the neighbours of a tile are the other five)
        d, gx, gy, gm, _, _ = oracle_prepare(fg, ni, m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"],
                                             [f[:, t] for t in range(6)], NLEV, missing=MISSING)
        c["halo"] = [d[t].reshape(NLEV, -1) for t in tiles]
        c["gx"], c["gy"], c["gm"] = [gx[t] for t in tiles], [gy[t] for t in tiles], [gm[t] for t in tiles]
        c["data"] = np.ascontiguousarray(np.concatenate(c["halo"], axis=1))
        c["grad_x"] = np.ascontiguousarray(np.concatenate(c["gx"], axis=1))
        c["grad_y"] = np.ascontiguousarray(np.concatenate(c["gy"], axis=1))
        c["grad_mask"] = np.ascontiguousarray(np.concatenate(c["gm"], axis=1).astype(np.int32))
        c["gm_all"] = gm
    else:
        c["data"] = c["src"]
    ref = np.empty((NLEV, nlon * nlat))
    for k in range(NLEV):
        if order == 2:
            r, _ = orc.cref_apply(2, x, nx, ny, [a[k] for a in c["halo"]], [a[k] for a in c["gx"]], [a[k] for a in c["gy"]],
                                  [a[k] for a in c["gm"]], True, MISSING, nlon, nlat, 1)
        else:
            r, _ = orc.cref_apply(1, x, nx, ny, [c["src"][k, q * ni * ni:(q + 1) * ni * ni] for q in range(len(tiles))],
                                  None, None, None, True, MISSING, nlon, nlat, 1)
        ref[k] = r
    c["ref"] = ref
    check_preconditions(c)
    return c


def check_preconditions(c):
    """What the masks must exercise, asserted on the reference's own output: a case that does not meet them is an error."""
    ref, x, ni, name = c["ref"], c["x"], c["ni"], c["name"]
    miss = ref == MISSING
    d_idx = x["j_out"].astype(np.int64) * c["nlon"] + x["i_out"]
    s_idx = x["t_in"].astype(np.int64) * ni * ni + x["j_in"].astype(np.int64) * ni + x["i_in"]
    touched = np.bincount(d_idx, minlength=c["ndst"]) > 0
    assert np.all(miss[K_NONE])                                                  # a level that is missing everywhere
    assert np.array_equal(miss[K_FULL], ~touched)                                # a level without a missing value
    bathy = [k for k in range(NLEV) if k not in (K_FULL, K_NONE)]
    src_miss = c["src"] == MISSING                                               # [NLEV][ncell]
    # some but not all exchange cells of a destination cell masked in a level: the renormalised case
    partial = False
    for k in bathy:
        n_bad = np.bincount(d_idx, weights=src_miss[k][s_idx].astype(np.float64), minlength=c["ndst"])
        n_all = np.bincount(d_idx, minlength=c["ndst"])
        partial = partial or bool(np.any((n_bad > 0) & (n_bad < n_all)))
    assert partial
    if name == "long":
        assert np.max(np.bincount(d_idx, minlength=c["ndst"])) > 256             # (the device constant is asserted in the test)
    if name == "empty":
        assert np.count_nonzero(~touched) > c["ndst"] // 2 and np.all(miss[:, ~touched])
    if name == "short":
        assert np.all(touched)
        mb = miss[bathy]
        assert np.any(np.any(mb, axis=0) & ~np.all(mb, axis=0))                  # missing in one level, valid in another
        assert np.any(~np.any(mb, axis=0))                                       # valid in every bathymetry level
    if c["order"] == 2 and len(c["tiles"]) == 6:
        gm = c["gm_all"]
        depth = c["depth"]
        for pname, k_dry, k_wet in (("edge", 0, K_FULL), ("corner", 4, 2)):
            t, pj, pi = c["probes"][pname]
            cell = pj * ni + pi
            own = depth[t, max(pj - 1, 0):pj + 2, max(pi - 1, 0):pi + 2]
            assert np.all(own == DEEP)                                           # valid centre, no cause inside its own tile
            assert gm[t][k_dry, cell] == 1 and gm[t][k_wet, cell] == 0, pname     # masked from another tile; differs by level
        assert any(np.any(gm[t][0] != gm[t][7]) for t in range(6))


@pytest.fixture(scope="module")
def cases(fg, gpu_ok):
    made = {}

    def get(name, order):
        if (name, order) not in made:
            c = build_host(fg, name, order)
            plan = fg.XgridPlan.create_empty(order, c["nx"], c["ny"], c["nlon"], c["nlat"])
            x = c["x"]
            plan.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], x.get("di"), x.get("dj"))
            c["plan"] = plan
            c["prep"] = None
            if order == 2 and len(c["tiles"]) == 6:
                m = c["m"]
                c["prep"] = fg.C2lPrep(m["nx"], m["ny"], m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"])
            c["dev"] = {k: torch.from_numpy(c[k]).to(DEV) for k in ("data", "grad_x", "grad_y", "grad_mask", "src") if k in c}
            made[(name, order)] = c
        return made[(name, order)]
    yield get
    for c in made.values():
        if c["prep"] is not None:
            c["prep"].destroy()
        c["plan"].destroy()


def _apply_levels(c, nlev, want_gsum=True):
    d = c["dev"]
    out = torch.full((nlev, c["ndst"]), float("nan"), dtype=torch.float64, device=DEV)
    g = c["plan"].apply_levels(d["data"], out, nlev, MISSING, d.get("grad_x"), d.get("grad_y"), d.get("grad_mask"), want_gsum=want_gsum)
    c["plan"].sync()
    return out.cpu().numpy(), g


PARAMS = [("short", o, n) for o in (1, 2) for n in LEVEL_COUNTS] + [("long", o, n) for o in (1, 2) for n in LEVEL_COUNTS] + \
         [(s, o, 9) for s in ("mid8", "mid2", "empty") for o in (1, 2)]


@pytest.mark.parametrize("name,order,nlev", PARAMS, ids=[f"{s}-order{o}-{n}lev" for s, o, n in PARAMS])
def test_apply_levels(fg, cases, name, order, nlev):
    c = cases(name, order)
    plan, d = c["plan"], c["dev"]
    if name == "long":
        rows = np.bincount(c["x"]["j_out"].astype(np.int64) * c["nlon"] + c["x"]["i_out"], minlength=c["ndst"])
        assert rows.max() > fg.XgridPlan.levels_capacity() == 256
    got, gsum = _apply_levels(c, nlev)
    bad = [k for k in range(nlev) if not _ref_close(got[k], c["ref"][k])]
    assert not bad, f"levels that differ from the reference: {bad}"
    # == nlev one-level calls of the existing path, values and sums, bit for bit
    one = torch.empty(c["ndst"], dtype=torch.float64, device=DEV)
    for k in range(nlev):
        kw = dict(grad_x_t=d["grad_x"][k], grad_y_t=d["grad_y"][k], grad_mask_t=d["grad_mask"][k]) if order == 2 else {}
        g1 = plan.apply_ex(d["data"][k], one, nz=1, has_missing=True, missing=MISSING, want_gsum=True, **kw)
        assert _same(one.cpu().numpy(), got[k]), k
        assert _bits(np.array([g1]))[0] == _bits(gsum[k:k + 1])[0], (k, g1, gsum[k])
    # a level without a missing value carries the plain sweep's bits wherever a row has exchange cells
    if nlev > K_FULL:
        kw = dict(grad_x_t=d["grad_x"][K_FULL], grad_y_t=d["grad_y"][K_FULL]) if order == 2 else {}
        plan.apply(d["data"][K_FULL], one, nz=1, **kw); plan.sync()
        plain = one.cpu().numpy()
        rows = got[K_FULL] != MISSING
        assert _same(plain[rows], got[K_FULL][rows]) and (name == "empty" or np.all(rows))
    if nlev > K_NONE:
        assert np.all(got[K_NONE] == MISSING)
    # == the records path (order 2): records and mask bits straight from the unpadded levels
    if c["prep"] is not None:
        rec = torch.empty(c["ncell"], 3, 8, dtype=torch.float64, device=DEV)
        mb = torch.empty(c["ncell"], dtype=torch.uint8, device=DEV)
        for k0 in range(0, nlev, 8):
            nl = min(8, nlev - k0)
            o = torch.full((nl, c["ndst"]), float("nan"), dtype=torch.float64, device=DEV)
            c["prep"].records_levels(d["src"][k0:k0 + nl].contiguous(), nl, MISSING, rec, mb); c["prep"].sync()
            g = plan.apply_records_levels(nl, rec, mb, o, MISSING, want_gsum=True); plan.sync()
            assert _same(o.cpu().numpy(), got[k0:k0 + nl]), k0
            assert np.array_equal(_bits(g), _bits(gsum[k0:k0 + nl])), k0
            want = np.zeros(c["ncell"], dtype=np.uint8)
            for k in range(nl):
                want |= (c["grad_mask"][k0 + k] != 0).astype(np.uint8) << k
            assert np.array_equal(mb.cpu().numpy(), want), k0


# ---------------------------------------------------------------------------------------------------------------- streamed
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


def _view(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


S_NLEV = 19                    # three chunks: the third reuses no slot, the object's second run reuses all of them
S_OUT = ((0.0, 180.0, 16, 15), (180.0, 360.0, 14, 15))       # two output tiles of different sizes


@pytest.fixture(scope="module")
def stream_cases(fg, gpu_ok):
    """(order, dtype name) -> plans of the two output tiles on C9, the typed source levels with their missing cells, the
    resident result (apply_levels on the widened levels) and the reference's, both still in double"""
    made = {}
    ni = 9

    def get(order, kind):
        if (order, kind) in made:
            return made[(order, kind)]
        m = _mosaic(fg, ni)
        depth, _ = _depth(fg, ni, m["contacts"])
        if kind == "float32":
            dtype, scale, offset, missing = np.float32, 0.5, 3.25, MISSING
            raw = np.stack([_values(ni, k) for k in range(S_NLEV)]).astype(np.float32)
        else:
            dtype, scale, offset, missing = np.int16, 0.01, 273.15, -32768.0
            cidx = np.arange(6 * ni * ni, dtype=np.int64).reshape(6, ni, ni)
            raw = np.stack([((37 * cidx + 101 * k) % 20011) - 10000 for k in range(S_NLEV)]).astype(np.int16)
        for k in range(S_NLEV):
            raw[k][_missing_at(depth, k)] = missing
        raw = np.ascontiguousarray(raw.reshape(S_NLEV, -1))
        f64 = _widen(raw, scale, offset, missing)
        assert np.array_equal(f64 == missing, raw == missing) and np.any(raw == missing)
        gout = []
        for (x0, x1, nlon, nlat) in S_OUT:
            lo, la = fg.latlon_corners(nlon, nlat, x0, x1, -90.0, 90.0)
            gout.append((nlon, nlat, lo, la))
        x = orc.cref_setup(order, [(ni, ni, m["lon"][t], m["lat"][t]) for t in range(6)], gout)
        plans = []
        for n, (nlon, nlat, _, _) in enumerate(gout):
            s = slice(int(x["xoff"][n]), int(x["xoff"][n + 1]))
            p = fg.XgridPlan.create_empty(order, [ni] * 6, [ni] * 6, nlon, nlat)
            p.set_xgrid(x["t_in"][s], x["i_in"][s], x["j_in"][s], x["i_out"][s], x["j_out"][s], x["area"][s],
                        x["di"][s] if order == 2 else None, x["dj"][s] if order == 2 else None)
            plans.append(p)
        prep = fg.C2lPrep(m["nx"], m["ny"], m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"]) if order == 2 else None
        tiles = [f64[:, t * ni * ni:(t + 1) * ni * ni] for t in range(6)]
        if order == 2:
            d, gx, gy, gm, _, _ = oracle_prepare(fg, ni, m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"],
                                                 [a.reshape(S_NLEV, ni, ni) for a in tiles], S_NLEV, missing=missing)
            halo = [a.reshape(S_NLEV, -1) for a in d]
        ref = [np.empty((S_NLEV, g[0] * g[1])) for g in gout]
        for k in range(S_NLEV):
            if order == 2:
                r, _ = orc.cref_apply(2, x, [ni] * 6, [ni] * 6, [a[k] for a in halo], [a[k] for a in gx], [a[k] for a in gy],
                                      [a[k] for a in gm], True, missing, [g[0] for g in gout], [g[1] for g in gout], 1)
            else:
                r, _ = orc.cref_apply(1, x, [ni] * 6, [ni] * 6, [a[k] for a in tiles], None, None, None, True, missing,
                                      [g[0] for g in gout], [g[1] for g in gout], 1)
            for n in range(len(gout)):
                ref[n][k] = r[n]
        # resident: apply_levels on the widened levels
        res = []
        for n, p in enumerate(plans):
            out = torch.empty(S_NLEV, gout[n][0] * gout[n][1], dtype=torch.float64, device=DEV)
            if order == 2:
                ts = [torch.from_numpy(np.ascontiguousarray(np.concatenate(a, axis=1))).to(DEV) for a in (halo, gx, gy)]
                tm = torch.from_numpy(np.ascontiguousarray(np.concatenate(gm, axis=1).astype(np.int32))).to(DEV)
                p.apply_levels(ts[0], out, S_NLEV, missing, ts[1], ts[2], tm)
            else:
                p.apply_levels(torch.from_numpy(f64).to(DEV), out, S_NLEV, missing)
            p.sync()
            res.append(out.cpu().numpy())
        made[(order, kind)] = dict(plans=plans, prep=prep, raw=raw, dtype=dtype, scale=scale, offset=offset, missing=missing,
                                   ref=ref, res=res)
        return made[(order, kind)]
    yield get
    for c in made.values():
        if c["prep"] is not None:
            c["prep"].destroy()
        for p in c["plans"]:
            p.destroy()


@pytest.mark.parametrize("order,kind,pinned", [(o, k, p) for o in (1, 2) for k in ("float32", "int16") for p in (True, False)],
                         ids=[f"order{o}-{k}-{'pinned' if p else 'pageable'}" for o in (1, 2) for k in ("float32", "int16") for p in (True, False)])
def test_streamed_levels(fg, stream_cases, order, kind, pinned):
    c = stream_cases(order, kind)
    dtype, scale, offset, missing = c["dtype"], c["scale"], c["offset"], c["missing"]
    want = [_narrow(r, scale, offset, missing, dtype) for r in c["res"]]         # fregrid_util.c:2376-2406; missing left alone
    for r, g in zip(c["ref"], c["res"]):
        assert np.array_equal(r == missing, g == missing) and np.any(r == missing) and np.any(r != missing)
        if orc.host_has_fma():
            assert _same(r, g)
        else:
            v = r != missing
            assert np.all(np.abs(g[v] - r[v]) <= 1e-10 * np.abs(r[v]))
    if np.dtype(dtype).kind == "i":                                             # inside the type's range: the cast is pinned
        for r in c["res"]:
            chk = _narrow(r, scale, offset, missing, np.float64)
            assert chk.min() >= -32768 and chk.max() < 32767
    sw = fg.Sweep(c["plans"], c["prep"], dtype, dtype)
    bufs = []
    if pinned:
        hin = fg.HostBuffer(c["raw"].shape, dtype); hin.array[:] = c["raw"]; bufs.append(hin)
        houts = [fg.HostBuffer(w.shape, dtype) for w in want]; bufs += houts
        a_in, a_out = hin.array, [h.array for h in houts]
    else:
        a_in, a_out = c["raw"].copy(), [np.empty(w.shape, dtype=dtype) for w in want]
    for _ in range(2):                                                          # the second run reuses every slot
        for a in a_out:
            a[...] = 77
        sw.run_levels(a_in, a_out, scale=scale, offset=offset, missing=missing)
        for n, (a, w) in enumerate(zip(a_out, want)):
            bad = np.nonzero(np.any(_view(a) != _view(w), axis=1))[0]
            assert bad.size == 0, f"tile {n}: levels that differ from the resident result: {bad.tolist()}"
    a_in = a_out = None
    sw.destroy()
    for b in bufs:
        b.free()


# ------------------------------------------------------------------------------------------------------------------ errors
def test_refusals_leave_outputs_and_objects_alone(fg, cases):
    L = fg.lib()
    c1, c2 = cases("short", 1), cases("short", 2)
    first = {o: _apply_levels(c, 9)[0] for o, c in ((1, c1), (2, c2))}
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    for order, c in ((1, c1), (2, c2)):
        d, h = c["dev"], c["plan"]._h
        out = torch.full((9, c["ndst"]), float("nan"), dtype=torch.float64, device=DEV)
        g = np.full(9, np.nan)
        gp = g.ctypes.data_as(C.POINTER(C.c_double))
        args = lambda **kw: [kw.get(k, v) for k, v in (("h", h), ("data", p(d["data"])), ("gx", p(d.get("grad_x"))), ("gy", p(d.get("grad_y"))),
                                                        ("gm", p(d.get("grad_mask"))), ("missing", MISSING), ("nlev", 9), ("out", p(out)), ("g", gp))]
        assert L.fg_plan_apply_levels(*args(nlev=0)) == FG_ERR_ARG
        assert L.fg_plan_apply_levels(*args(nlev=-3)) == FG_ERR_ARG
        assert L.fg_plan_apply_levels(*args(data=p(None))) == FG_ERR_ARG
        assert L.fg_plan_apply_levels(*args(out=p(None))) == FG_ERR_ARG
        assert L.fg_plan_apply_levels(*args(h=None)) == FG_ERR_ARG
        if order == 2:
            assert L.fg_plan_apply_levels(*args(gm=p(None))) == FG_ERR_ARG
            assert L.fg_plan_apply_levels(*args(gx=p(None))) == FG_ERR_ARG
            assert L.fg_plan_apply_levels(*args(gy=p(None))) == FG_ERR_ARG
        # a plan that is not finalized
        raw = fg.XgridPlan.create_empty(order, c["nx"], c["ny"], c["nlon"], c["nlat"])
        assert L.fg_plan_apply_levels(*args(h=raw._h)) == FG_ERR_ARG
        if order == 2:
            rec = torch.zeros(c["ncell"], 3, 8, dtype=torch.float64, device=DEV)
            mb = torch.zeros(c["ncell"], dtype=torch.uint8, device=DEV)
            assert L.fg_plan_apply_records_levels(raw._h, 8, p(rec), p(mb), MISSING, p(out), gp) == FG_ERR_ARG
            assert L.fg_plan_apply_records_levels(h, 0, p(rec), p(mb), MISSING, p(out), gp) == FG_ERR_ARG
            assert L.fg_plan_apply_records_levels(h, 9, p(rec), p(mb), MISSING, p(out), gp) == FG_ERR_ARG
            assert L.fg_plan_apply_records_levels(h, 8, p(rec), p(None), MISSING, p(out), gp) == FG_ERR_ARG
            assert L.fg_plan_apply_records_levels(h, 8, p(None), p(mb), MISSING, p(out), gp) == FG_ERR_ARG
            assert L.fg_plan_apply_records_levels(cases("short", 1)["plan"]._h, 8, p(rec), p(mb), MISSING, p(out), gp) == FG_ERR_ARG
            ph = c["prep"]._h
            assert L.fg_c2l_records_levels(ph, p(d["src"]), 0, MISSING, p(rec), p(mb)) == FG_ERR_ARG
            assert L.fg_c2l_records_levels(ph, p(d["src"]), 9, MISSING, p(rec), p(mb)) == FG_ERR_ARG
            assert L.fg_c2l_records_levels(ph, p(d["src"]), 8, MISSING, p(rec), p(None)) == FG_ERR_ARG
            assert L.fg_c2l_records_levels(ph, p(None), 8, MISSING, p(rec), p(mb)) == FG_ERR_ARG
            assert torch.all(rec == 0).item() and torch.all(mb == 0).item()
        raw.destroy()
        torch.cuda.synchronize()
        assert torch.all(torch.isnan(out)).item() and np.all(np.isnan(g))
        # the existing entry points keep their refusal
        o2 = torch.full((2, c["ndst"]), float("nan"), dtype=torch.float64, device=DEV)
        with pytest.raises(fg.FregridHipError, match="has_missing should be false when nz > 1"):
            c["plan"].apply(d["data"], o2, nz=2, grad_x_t=d.get("grad_x"), grad_y_t=d.get("grad_y"), grad_mask_t=d.get("grad_mask"),
                            has_missing=True, missing=MISSING)
        assert torch.all(torch.isnan(o2)).item()
        assert _same(_apply_levels(c, 9)[0], first[order])                       # the next valid run: the first run's bits


def test_streamed_refusals(fg, cases, stream_cases):
    L = fg.lib()
    c = stream_cases(2, "float32")
    dtype = c["dtype"]
    sw = fg.Sweep(c["plans"], c["prep"], dtype, dtype)
    outs = [np.empty(r.shape, dtype=dtype) for r in c["res"]]
    sw.run_levels(c["raw"], outs, scale=c["scale"], offset=c["offset"], missing=c["missing"])
    first = [o.copy() for o in outs]
    for o in outs:
        o[...] = 77
    run = L.fg_sweep_run_levels
    ptrs = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    p_in = c["raw"].ctypes.data_as(C.c_void_p)
    a = (c["scale"], c["offset"], c["missing"])
    assert run(sw._h, p_in, 0, *a, ptrs) == FG_ERR_ARG
    assert run(sw._h, None, S_NLEV, *a, ptrs) == FG_ERR_ARG
    assert run(sw._h, p_in, S_NLEV, *a, None) == FG_ERR_ARG
    assert run(sw._h, p_in, S_NLEV, *a, (C.c_void_p * 2)(outs[0].ctypes.data, None)) == FG_ERR_ARG
    assert run(None, p_in, S_NLEV, *a, ptrs) == FG_ERR_ARG
    # a plan that is not finalized, in a sweep of its own
    c1 = cases("short", 1)
    raw_plan = fg.XgridPlan.create_empty(1, c1["nx"], c1["ny"], c1["nlon"], c1["nlat"])
    sw1 = fg.Sweep([raw_plan], None, np.float64, np.float64)
    o1 = np.full((9, c1["ndst"]), 77.0)
    assert run(sw1._h, c1["src"][:9].ctypes.data_as(C.c_void_p), 9, 0.0, 0.0, MISSING, (C.c_void_p * 1)(o1.ctypes.data)) == FG_ERR_ARG
    assert np.all(o1 == 77.0)
    sw1.destroy(); raw_plan.destroy()
    assert all(np.all(o == 77) for o in outs)
    # Sweep.run keeps refusing a variable with missing values, and says where it goes
    with pytest.raises(ValueError, match="run_levels"):
        sw.run(c["raw"][:2], [o[:2] for o in outs], has_missing=True)
    assert all(np.all(o == 77) for o in outs)
    sw.run_levels(c["raw"], outs, scale=c["scale"], offset=c["offset"], missing=c["missing"])
    for o, f in zip(outs, first):
        assert np.array_equal(_view(o), _view(f))
    sw.destroy()
