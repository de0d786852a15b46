"""Inputs and yardsticks for the monotone limiter on the gradient object's records (fg_c2l_records_levels_mono,
fg_plan_apply_records_levels_mono, fg_plan_mono_records_*, fg_sweep_run_levels_mono).  No GPU, no torch.

A chunk of 1 <= nz <= 8 levels is three buffers: rec [nsrc][3][8] = field | grad_x | grad_y (zero beyond nz), maskbits uint8
[nsrc] (bit k = the gradient mask of level k) and the bounds records b8 [nsrc][4][8] = f_bar_max | f_bar_min | f_max | f_min.
Rows 0 and 1 of b8 are the maximum and minimum over the nine values of the cell's 3 x 3 neighbourhood in the halo'd field that
differ from `missing`, the centre included, starting from -1e20 and +1e20 (conserve_interp.c:622-645); rows 2 and 3, and all
four rows of a level >= nz, are those start values.

  chunk()       the three buffers of levels k0 .. k0 + nz of a hand-made one-tile list of tests/mono_levels_cases.py, from its
                frame, vals, gx, gy, miss and gm, masked or unmasked
  bounds8()     the bounds records of any halo'd field, tiles back to back: the yardstick of the device's one-pass kernel
  real_pair()   C9 -> 30 x 15 with six tiles: tame values (one decade, either sign, so an excess of the limiter is an ulp and the
                fatal check cannot fire) under the depth-dependent mask of tests/test_gpu_masked_levels.py; exchange cells
                from the project's own CPU search (oracle/), halo fill and gradients from the CPU preparation (oracle/), so
                the fixture needs neither the reference library nor a device
  real_plain()  mono_levels_cases' float64 loop on that pair: its limiter indexes the halo'd field of ONE tile, so the
                neighbourhood bounds are taken per tile here (limited_on()), the sums are mono_levels_cases.sweep()
REAL_SEED is fixed so that check_real_preconditions() holds (tests/test_mono_records_cases_cpu.py asserts it on the CPU)."""
import functools

import numpy as np

import mono_levels_cases as mc
import orc
import sweep_cases as sc

MISSING, NLEV, K_FULL, K_NONE = mc.MISSING, mc.NLEV, mc.K_FULL, mc.K_NONE
F_MAX0, F_MIN0 = -1.0e20, 1.0e20                                     # the start values of a maximum / a minimum
REAL_NI, REAL_NLON, REAL_NLAT, REAL_SEED = 9, 30, 15, 5
REAL_OPTS = ("none", "meas", "meas_target")


# ------------------------------------------------------------------------------------------------------------ bounds records
def neighbourhood_bounds(halo, tiles, missing):
    """halo [L][F], the halo'd tiles ((nx, ny), ...) back to back -> (f_bar_max, f_bar_min) [L][ncells], cells tile by tile.
    Walks the nine offsets cell by cell through flat indices of the halo'd layout (not the shifted views of
    mono_levels_cases.limited)."""
    halo = np.asarray(halo, dtype=np.float64)
    L = halo.shape[0]
    centre = []
    width = []
    off = 0
    for nx, ny in tiles:
        j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        centre.append((off + (j + 1) * (nx + 2) + i + 1).ravel())
        width.append(np.full(nx * ny, nx + 2))
        off += (nx + 2) * (ny + 2)
    assert halo.shape[1] == off, (halo.shape, off)
    centre, width = np.concatenate(centre), np.concatenate(width)
    mx = np.full((L, centre.size), F_MAX0)
    mn = np.full((L, centre.size), F_MIN0)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            v = halo[:, centre + dj * width + di]
            ok = v != missing
            mx = np.where(ok & (v > mx), v, mx)
            mn = np.where(ok & (v < mn), v, mn)
    return mx, mn


def bounds8(halo, tiles, missing, nz=None):
    """b8 [ncells][4][8] of the first nz (default: all, at most 8) levels of halo [L][F]"""
    nz = halo.shape[0] if nz is None else nz
    assert 1 <= nz <= 8 and nz <= halo.shape[0]
    mx, mn = neighbourhood_bounds(halo[:nz], tiles, missing)
    b8 = np.empty((mx.shape[1], 4, 8))
    b8[:, 0], b8[:, 1], b8[:, 2], b8[:, 3] = F_MAX0, F_MIN0, F_MAX0, F_MIN0
    b8[:, 0, :nz], b8[:, 1, :nz] = mx.T, mn.T
    return b8


def records8(field, gx, gy, gm, nz):
    """rec [nsrc][3][8] and maskbits [nsrc] of the first nz levels of field / gx / gy [L][nsrc] and gm [L][nsrc] or None"""
    nsrc = field.shape[1]
    rec = np.zeros((nsrc, 3, 8))
    for w, a in enumerate((field, gx, gy)):
        rec[:, w, :nz] = a[:nz].T
    mb = np.zeros(nsrc, dtype=np.uint8)
    if gm is not None:
        for k in range(nz):
            mb |= (np.asarray(gm[k]) != 0).astype(np.uint8) << k
    return rec, mb


def chunk(name, masked, k0, nz, with_gm=None):
    """(rec, maskbits or None, b8, missing) of levels k0 .. k0 + nz of the hand-made list `name`; maskbits is None where the
    variant has no gradient mask (mono_levels_cases.inputs: the unmasked variant without with_gm)"""
    c, v = sc.make(name), mc.values(name)
    assert c["one_tile"] and 1 <= nz <= 8 and k0 + nz <= NLEV
    with_gm = masked if with_gm is None else with_gm
    missing = MISSING if masked else -1.0e20
    lv = slice(k0, k0 + nz)
    vals = np.where(c["miss"][lv], MISSING, v["vals"][lv]) if masked else v["vals"][lv]
    halo = v["frame"][lv].copy()
    halo[:, c["inner"]] = vals
    rec, mb = records8(vals, v["gx"][lv], v["gy"][lv], c["gm"][lv] if with_gm else None, nz)
    return rec, (mb if with_gm else None), bounds8(halo, c["tiles"], missing, nz), missing


# ------------------------------------------------------------------------------------------------------------ the real pair
def _mosaic(fg, ni):
    lon, lat, lont, latt = fg.gnomonic_ed_grid(ni)
    A = np.ascontiguousarray
    m = dict(nx=[ni] * 6, ny=[ni] * 6, lon=[A(lon[t]) for t in range(6)], lat=[A(lat[t]) for t in range(6)],
             lont=[A(lont[t]) for t in range(6)], latt=[A(latt[t]) for t in range(6)])
    m["contacts"] = fg.find_contacts(m["nx"], m["ny"], m["lon"], m["lat"])
    return m


_REAL = {}


def real_pair(fg):
    """the fixture, built once per process"""
    if "c" in _REAL:
        return _REAL["c"]
    import test_gpu_masked_levels as ml                              # the depth-dependent mask of the existing real pair
    from test_gpu_c2l import oracle_prepare
    ni, nlon, nlat = REAL_NI, REAL_NLON, REAL_NLAT
    m = _mosaic(fg, ni)
    depth, _ = ml._depth(fg, ni, m["contacts"])
    rng = np.random.default_rng(REAL_SEED)
    vals = rng.choice([-1.0, 1.0], (NLEV, 6, ni, ni)) * rng.uniform(1.0, 10.0, (NLEV, 6, ni, ni))
    f = np.stack([np.where(ml._missing_at(depth, k), MISSING, vals[k]) for k in range(NLEV)])          # [NLEV][6][ni][ni]
    lo, la = fg.latlon_corners(nlon, nlat)
    x = orc.orc_setup(2, [(ni, ni, m["lon"][t], m["lat"][t]) for t in range(6)], [(nlon, nlat, lo, la)])
    d, gx, gy, gm, _, _ = oracle_prepare(fg, ni, m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"], [f[:, t] for t in range(6)],
                                         NLEV, missing=MISSING)
    ncell, ndst = 6 * ni * ni, nlon * nlat
    src = x["t_in"].astype(np.int64) * ni * ni + x["j_in"].astype(np.int64) * ni + x["i_in"]
    dst = x["j_out"].astype(np.int64) * nlon + x["i_out"]
    lens = np.bincount(dst, minlength=ndst)
    ca_in = np.concatenate([np.asarray(a).ravel() for a in x["cell_area_in"]])
    c = dict(ni=ni, nlon=nlon, nlat=nlat, m=m, x=x, depth=depth, tiles=((ni, ni),) * 6, tnx=[ni] * 6, tny=[ni] * 6, ncell=ncell, nsrc=ncell,
             ndst=ndst, nx=len(src), src=src, dst=dst, lens=lens, row_ptr=np.concatenate([[0], np.cumsum(lens)]),
             field=np.ascontiguousarray(f.reshape(NLEV, ncell)),
             halo=np.ascontiguousarray(np.concatenate([d[t].reshape(NLEV, -1) for t in range(6)], axis=1)),
             gx=np.ascontiguousarray(np.concatenate(gx, axis=1)), gy=np.ascontiguousarray(np.concatenate(gy, axis=1)),
             gm=np.ascontiguousarray(np.concatenate(gm, axis=1).astype(np.int32)),
             cell_area_in=ca_in, field_area=ca_in * (0.5 + ((3 * np.arange(ncell)) % 8) / 8.0),
             cell_area_out=orc.orc_get_grid_area(nlon, nlat, lo, la).ravel())
    _REAL["c"] = c
    return c


def real_options(c, opt):
    assert opt in REAL_OPTS
    meas = opt in ("meas", "meas_target")
    return dict(weight=None, sum=False, field_area=c["field_area"] if meas else None, cell_area_in=c["cell_area_in"] if meas else None,
                cell_area_out=c["cell_area_out"] if opt == "meas_target" else None, has_missing=True, missing=MISSING)


def limited_on(c, kw, fbmax, fbmin):
    """mono_levels_cases.limited (conserve_interp.c:647-714) with the neighbourhood bounds given, [L][nsrc] each, and the field
    per source cell, kw["field"] [L][nsrc]: (xdata [L][nx], facts)"""
    s, x, missing = c["src"], c["x"], kw["missing"]
    gx, gy, gm = kw["gx"], kw["gy"], kw["gm"]
    L = kw["field"].shape[0]
    fbar = kw["field"][:, s]
    full = (fbar + gx[:, s] * x["di"]) + gy[:, s] * x["dj"]
    xd = full if gm is None else np.where(gm[:, s] != 0, fbar, full)
    ok = fbar != missing
    xd = np.where(ok, xd, missing)
    fmax, fmin = np.full((L, c["nsrc"]), F_MAX0), np.full((L, c["nsrc"]), F_MIN0)
    for k in range(L):
        np.maximum.at(fmax[k], s[ok[k]], xd[k][ok[k]])
        np.minimum.at(fmin[k], s[ok[k]], xd[k][ok[k]])
    live = xd != missing
    bmx, bmn, mx, mn = fbmax[:, s], fbmin[:, s], fmax[:, s], fmin[:, s]
    up = live & (mx > bmx)
    dn = live & ~up & (mn < bmn)
    with np.errstate(all="ignore"):
        xu = fbar + ((xd - fbar) / (mx - fbar)) * (bmx - fbar)
        xl = fbar + ((xd - fbar) / (mn - fbar)) * (bmn - fbar)
    over, under = up & (xu > bmx), dn & (xl < bmn)
    exc_u, exc_l = np.where(over, xu - bmx, 0.0), np.where(under, bmn - xl, 0.0)
    for k in range(L):
        if np.any(exc_u[k] >= mc.TOLERANCE) or np.any(exc_l[k] >= mc.TOLERANCE):
            raise mc.LimiterFatal(mc.MSG_ABOVE if np.any(exc_u[k] >= mc.TOLERANCE) else mc.MSG_BELOW, k,
                                  float(max(exc_u[k].max(), exc_l[k].max())))
    out = np.where(up, np.where(over, bmx, xu), np.where(dn, np.where(under, bmn, xl), xd))
    facts = dict(up=np.any(up, axis=1), dn=np.any(dn, axis=1), excess=np.maximum(exc_u.max(axis=1, initial=0.0), exc_l.max(axis=1, initial=0.0)))
    return out, facts


@functools.lru_cache(maxsize=None)
def _real_plain(opt):
    c = _REAL["c"]
    kw = dict(real_options(c, opt), field=c["field"], gx=c["gx"], gy=c["gy"], gm=c["gm"])
    fbmax, fbmin = neighbourhood_bounds(c["halo"], c["tiles"], MISSING)
    xd, facts = limited_on(c, kw, fbmax, fbmin)
    return mc.sweep(c, kw, xd), facts


def real_plain(fg, opt):
    """([NLEV][ndst], facts) of the float64 loop on the real pair; raises LimiterFatal where the reference would end the process"""
    real_pair(fg)
    return _real_plain(opt)


def check_real_preconditions(fg):
    """asserted, not skipped"""
    c = real_pair(fg)
    ni, f = c["ni"], c["field"]
    assert np.all(f[K_NONE] == MISSING) and not np.any(f[K_FULL] == MISSING) and np.any(f == MISSING)
    # a cell on a cube edge, and one next to a cube corner, whose bound comes from a cell of ANOTHER tile: the bound over the
    # whole neighbourhood differs from the one over its own tile's cells (every halo element a contact fills set to `missing`,
    # which no bound takes; the elements no contact fills keep their 0.0)
    _, hmap = fg.halo_map([ni] * 6, [ni] * 6, c["m"]["contacts"])
    own = c["halo"].copy()
    own[:, np.asarray(hmap) >= 0] = MISSING
    mx, mn = neighbourhood_bounds(c["halo"], c["tiles"], MISSING)
    mx0, mn0 = neighbourhood_bounds(own, c["tiles"], MISSING)
    foreign = ((mx != mx0) | (mn != mn0)).reshape(NLEV, 6, ni, ni)
    j, i = np.meshgrid(np.arange(ni), np.arange(ni), indexing="ij")
    on_i, on_j = (i == 0) | (i == ni - 1), (j == 0) | (j == ni - 1)
    corner, edge = on_i & on_j, (on_i ^ on_j)
    assert np.any(foreign[:, :, edge]) and np.any(foreign[:, :, corner])
    assert not np.any(foreign[:, :, ~(on_i | on_j)])
    out, facts = real_plain(fg, "none")                               # (did not raise: no fatal excess on any level)
    assert np.all(facts["excess"] < 1e-12), facts["excess"].max()
    live = [k for k in range(NLEV) if k != K_NONE]
    assert np.all(facts["up"][live]) and np.all(facts["dn"][live])
    assert not facts["up"][K_NONE] and not facts["dn"][K_NONE]
    assert np.all(out[K_NONE] == MISSING) and np.any(out[K_FULL] != MISSING)
    return c
