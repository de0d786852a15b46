"""Inputs and yardsticks for the level loop with options (fg_plan_apply_levels_ex, fg_plan_apply_records_levels_ex,
fg_sweep_run_levels_ex; k_apply_ep8x in csrc/apply_kernels.hip).  No GPU, no torch.

The exchange lists, fields, masks and option arrays are those of tests/sweep_cases.py: all NLEV = 17 levels of a case, with one
option set of do_scalar_conserve_interp from OPTS, each with has_missing 1 and 0 (the reference allows every one of them on one
level; it refuses nz > 1 for has_missing, cell_measures and sum, conserve_interp.c:544-546, which is why the yardstick is one
call per level).

  weight0        --weight_field; the weights have exact zeros (rows whose counted cells all weigh 0: 0.0 by `touched`)
  sum            cell_methods = "area: sum"
  meas           cell_measures with an area variable without a z axis: field_area [nsrc]
  meas_z         ... with a z axis (area_has_zaxis, fregrid_util.c:2156-2162): field_area [NLEV][nsrc], area_z()
  meas_target, meas_z_target   the same with --target_grid
  weight0+sum, weight0+meas

area_z(c) is field_area[s] * (0.75 + ((7 s + 3 k) % 13) / 17): positive, different in every level.  With has_missing the
per-level sets carry AREA_MISSING in a third of the (cell, level) pairs whose data is missing in that level -- legal (the check
of conserve_interp.c:582-586 comes after the missing test), and its term enters the --target_grid sum, which takes every cell.
The shared area cannot carry it: level K_FULL has no missing cell, so no source cell is missing in every level.

Yardsticks: reference() is orc.cref_apply once per level, the reference's own object code; plain() is a float64 loop in list
order, for where the reference library is not built, with switches that break it on purpose (test_levels_ex_cases_cpu.py).

check_preconditions() asserts what the cases must exercise; a case that misses one is an error, not a skip."""
import functools

import numpy as np

import orc
import sweep_cases as sc

MISSING, NLEV, K_FULL, K_NONE = sc.MISSING, sc.NLEV, sc.K_FULL, sc.K_NONE
AREA_MISSING = -9.0e15
OPTS = {
    "weight0": dict(weight=True),
    "sum": dict(sum=True),
    "meas": dict(meas=True),
    "meas_z": dict(meas=True, z=True),
    "meas_target": dict(meas=True, target=True),
    "meas_z_target": dict(meas=True, z=True, target=True),
    "weight0+sum": dict(weight=True, sum=True),
    "weight0+meas": dict(weight=True, meas=True),
}
SETS = tuple((opt, masked) for opt in OPTS for masked in (True, False))
# the smallest sweep_cases cases that reach every tiling and chunk walk of k_apply_ep8x
CASES = ("short-201", "short-5", "short-1", "eights-804", "spike-804", "mid-201", "long-201", "huge-99")
# rows per tile of k_apply_ep8x per bin of nx // ndst (fgd_apply_levels8x): with an area shared by the levels on chunks of
# fg_plan_levels_ex_capacity(0) exchange cells, with an area per level on chunks of fg_plan_levels_ex_capacity(1)
ROWS_PER_TILE = {"<=6": (32, 16), "7..24": (16, 8), "25..96": (2, 2), ">96": (1, 1)}
CAPACITY = (256, 128)            # what the library reports (asserted against it in test_gpu_levels_ex.py)


def set_id(opt, masked):
    return f"{opt}-{'missing' if masked else 'plain'}"


def area_z(c):
    s, k = np.arange(c["nsrc"])[None, :], np.arange(NLEV)[:, None]
    return c["field_area"][None, :] * (0.75 + ((7 * s + 3 * k) % 13) / 17.0)


def inputs(c, order, opt, masked):
    """everything one option set takes, all NLEV levels: the keyword names are those of plain()"""
    o = OPTS[opt]
    kw = dict(order=order, has_missing=masked, missing=MISSING if masked else -1.0e20, data=sc.field(c, order, masked),
              gx=c["gx"] if order == 2 else None, gy=c["gy"] if order == 2 else None, gm=c["gm"] if order == 2 else None,
              weight=c["weight"] if o.get("weight") else None, sum=bool(o.get("sum")), field_area=None, per_level=bool(o.get("z")),
              cell_area_in=c["cell_area_in"] if (o.get("sum") or o.get("meas")) else None,
              cell_area_out=c["cell_area_out"] if o.get("target") else None, area_missing=AREA_MISSING)
    if o.get("meas"):
        fa = area_z(c) if o.get("z") else c["field_area"].copy()
        if o.get("z") and masked:
            s, k = np.arange(c["nsrc"])[None, :], np.arange(NLEV)[:, None]
            fa[c["miss"] & ((s + 2 * k) % 3 == 0)] = AREA_MISSING
        kw["field_area"] = np.ascontiguousarray(fa)
    return kw


def level_area(kw, k):
    fa = kw["field_area"]
    return fa[k] if (fa is not None and kw["per_level"]) else fa


# ---------------------------------------------------------------------------------------------------------------- yardsticks
@functools.lru_cache(maxsize=None)
def _reference(name, order, opt, masked):
    c = sc.make(name)
    kw = inputs(c, order, opt, masked)
    pt = lambda a, halo=False: sc._per_tile(c, a, halo) if a is not None else None
    out = np.empty((NLEV, c["ndst"]))
    for k in range(NLEV):
        lv = lambda a: a[k] if a is not None else None
        out[k], _ = orc.cref_apply(order, c["x"], c["tnx"], c["tny"], pt(kw["data"][k], order == 2), pt(lv(kw["gx"])), pt(lv(kw["gy"])),
                                   pt(lv(kw["gm"])) if masked else None, masked, kw["missing"], c["nxo"], c["nyo"], 1, weight=pt(kw["weight"]),
                                   cell_methods_sum=kw["sum"], field_area=pt(level_area(kw, k)), area_missing=AREA_MISSING,
                                   cell_area_in=pt(kw["cell_area_in"]), target_grid=kw["cell_area_out"] is not None,
                                   cell_area_out=kw["cell_area_out"])
    out.setflags(write=False)
    return out


def reference(name, order, opt, masked):
    """[NLEV][ndst]: the reference's do_scalar_conserve_interp(nz = 1) on every level alone"""
    return _reference(name, order, opt, masked)


def plain(c, order, opt, masked, reverse=False, left_assoc=False, shared_area=False, target_valid_only=False, parts=False):
    """The reference's loops in float64, every sum in list order, all levels at once (step r adds cell r of every row that has
    one), then the finish of conserve_interp.c:815-866.  The switches break it on purpose: reverse = the cells in reversed
    list order; left_assoc = a*fa/ca where the reference has a*(fa/ca); shared_area = level 0's area for every level;
    target_valid_only = the --target_grid sum without the cells whose data is missing.  parts: also (asum, touched, asum_t)."""
    kw = inputs(c, order, opt, masked)
    x, s, d = c["x"], c["src"], c["dst"]
    fi = c["fidx"] if order == 2 else s
    ndst, missing = c["ndst"], kw["missing"]
    a0 = x["area"][None, :]
    a = a0 * kw["weight"][s][None, :] if kw["weight"] is not None else a0
    v = kw["data"][:, fi]
    valid = (v != missing) if masked else np.ones(v.shape, dtype=bool)
    fa = kw["field_area"]
    if fa is not None:
        fa = fa if kw["per_level"] else fa[None, :]
        fa = (fa[:1] if shared_area else fa)[:, s]
    ca = kw["cell_area_in"][s][None, :] if kw["cell_area_in"] is not None else None
    with np.errstate(all="ignore"):
        if kw["sum"]:
            a = a / ca
        elif fa is not None:
            a = (a * fa / ca) if left_assoc else a * (fa / ca)
        if order == 2:
            full = (v + kw["gx"][:, s] * x["di"]) + kw["gy"][:, s] * x["dj"]
            v = np.where(kw["gm"][:, s] != 0, v, full) if masked else full
        a = np.broadcast_to(a, v.shape)
        p = v * a
        t = (a0 * fa / ca) if (fa is not None and not kw["sum"]) else a0
        t = np.broadcast_to(t, v.shape)
        if target_valid_only:
            t = np.where(valid, t, 0.0)
    lst = np.arange(c["nx"])[::-1] if reverse else np.arange(c["nx"])
    csr = lst[np.argsort(d[lst], kind="stable")]
    lens, row_ptr = c["lens"], c["row_ptr"]
    acc, asum, asum_t = np.zeros((NLEV, ndst)), np.zeros((NLEV, ndst)), np.zeros((NLEV, ndst))
    touched = np.zeros((NLEV, ndst), dtype=bool)
    by_len = np.argsort(-lens, kind="stable")
    longest = int(lens.max(initial=0))
    nrows = np.searchsorted(-lens[by_len], -np.arange(longest), side="left")           # rows longer than r
    for r in range(longest):
        rows = by_len[:nrows[r]]
        n = csr[row_ptr[rows] + r]
        ok = valid[:, n]
        acc[:, rows] = np.where(ok, acc[:, rows] + p[:, n], acc[:, rows])
        asum[:, rows] = np.where(ok, asum[:, rows] + a[:, n], asum[:, rows])
        asum_t[:, rows] += t[:, n]
        touched[:, rows] |= ok
    with np.errstate(all="ignore"):
        if kw["sum"]:
            out = np.where(asum == 0, np.where(touched, 0.0, missing), acc)
        else:
            out = np.where(asum > 0, acc / asum, np.where(touched, 0.0, missing))
            if kw["cell_area_out"] is not None:
                out = np.where(out != missing, out * (asum_t / kw["cell_area_out"][None, :]), out)
    return (out, asum, touched, asum_t) if parts else out


def yardstick(name, order, opt, masked):
    """(which, [NLEV][ndst]): the reference library where it is built, else the plain loop"""
    if orc.conserve_ref_available():
        return "reference", reference(name, order, opt, masked)
    return "plain", _plain_cached(name, order, opt, masked)


@functools.lru_cache(maxsize=None)
def _plain_cached(name, order, opt, masked):
    out = plain(sc.make(name), order, opt, masked)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------ preconditions
def tilings(c, capacity=CAPACITY):
    """the (rows per tile, chunk size) pairs of k_apply_ep8x in the case's bin: shared area, per-level area"""
    r = ROWS_PER_TILE[c["bin"]]
    return ((r[0], capacity[0]), (r[1], capacity[1]))


def check_crossings(c, capacity=CAPACITY):
    """At least one row crosses a chunk boundary of every tiling the kernel uses in the case's bin.  The profile `short` is the
    other path: its tiles hold fewer cells than any chunk (asserted as such)."""
    for rpt, cap in tilings(c, capacity):
        inside, _ = sc.crossings(c["row_ptr"], rpt, cap)
        if c["profile"] == "short":
            q0 = c["row_ptr"][np.arange(0, c["ndst"], rpt)]
            assert np.all(np.diff(np.append(q0, c["nx"])) <= cap) and not np.any(inside), (c["name"], rpt, cap)
        else:
            assert np.any(inside > 0), (c["name"], rpt, cap)


def check_preconditions(c, order=2):
    name, big = c["name"], c["ndst"] >= 99
    check_crossings(c)
    for opt, o in OPTS.items():
        out, asum, touched, _ = plain(c, order, opt, True, parts=True)
        kw = inputs(c, order, opt, True)
        # the three outcomes of conserve_interp.c:815-839 (:821-830 for sum)
        oc = np.where(touched & ((asum != 0) if kw["sum"] else (asum > 0)), 0, np.where(touched, 1, 2))
        assert np.array_equal(out == MISSING, oc == 2), (name, opt)
        assert np.all(out[oc == 1] == 0), (name, opt)                   # (-0.0 where --target_grid scales 0.0 by a negative sum)
        if big:
            assert all(np.any(oc == v) for v in (0, 1, 2)), (name, opt, [int(np.count_nonzero(oc == v)) for v in (0, 1, 2)])
            assert np.all(oc[K_NONE] == 2) and np.any(oc[K_FULL] == 0) and np.any(oc[K_FULL] == 1), (name, opt)
        if o.get("z"):
            fa = kw["field_area"]
            assert np.any(fa == AREA_MISSING) and not np.any((fa == AREA_MISSING) & ~c["miss"]), (name, opt)
            assert np.all(fa[fa != AREA_MISSING] > 0) and np.all(np.any(fa[1:] != fa[:1], axis=0)), (name, opt)
            if big:                                                       # ... and under exchange cells of rows that have a value
                hit = (fa[:, c["src"]] == AREA_MISSING)
                rows = np.stack([np.bincount(c["dst"], weights=h.astype(np.float64), minlength=c["ndst"]) for h in hit]) > 0
                assert np.any(rows & (oc == 0)), (name, opt)
        if o.get("target") and big:
            nmiss = np.stack([np.bincount(c["dst"], weights=m.astype(np.float64), minlength=c["ndst"]) for m in c["miss"][:, c["src"]]])
            assert np.any(out == MISSING) and np.any((out != MISSING) & (nmiss > 0)), (name, opt)
    return True
