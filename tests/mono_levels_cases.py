"""Inputs and yardsticks for the monotone limiter on many levels (fg_plan_apply_levels_mono, fg_plan_mono_levels_*; k_mono_bounds8,
k_mono_extremes8, k_apply_ep8m).  No GPU, no torch.

Level k of the device's result must carry the bits of do_scalar_conserve_interp(nz = 1) with MONOTONIC set on level k alone
(conserve_interp.c:617-742, :815-866).  The lists are the one-tile cases of tests/sweep_cases.py -- the reference's monotone branch
indexes every tile with the LAST tile's nx (:653), so a hand-made list needs one tile.  sweep_cases.make() reads the -1t suffix
generically, so beside spike-804-1t, eights-804-1t and long-201-1t it builds mid-201-1t and huge-99-1t, and all four row-length
bins of ep_tile are reached.

Values: NLEV = 17 levels of "tame" values, sweep_cases' recipe for its level 0 -- +-uniform(1, 10) for the field, the halo frame and
both gradients -- drawn per (case, level).  The limiter's result may exceed the neighbourhood's bound by rounding; the reference
ends the process unless the excess is below 1e-10.  With values of one decade the excess is an ulp, about 1e-15, so the fatal
check cannot fire: plain() verifies that for every case and level, and raises LimiterFatal where it would.
  The 1e-10 snap fires where f_bar + (f_bar_max - f_bar) rounds above f_bar_max, and that needs an inexact difference: f_bar_max
  beyond twice f_bar, or of the other sign.  A cell is limited only where f_bar + gx di + gy dj passes f_bar_max, and with
  gradients of one decade and |di|, |dj| <= 0.02 the step is at most 0.4 -- f_bar_max - f_bar is then exact (Sterbenz) and the
  snap never fires: measured here, 0 snaps on every case and level.  So the levels STEEP_LEVELS, one per chunk of eight, carry
  gradients 100 times steeper (the field and the frame stay tame, so the excess stays an ulp of a value below 10): 17 to 64
  snaps per such level, and check_preconditions asserts them.
The case's own
miss[k] (K_FULL and K_NONE kept) and gm[k] apply per level in the masked variant; the unmasked variant has neither missing values
nor (by default) a gradient mask -- the branch reads grad_mask whether or not the field has missing values (:656), with_gm=True
gives that combination.

Option sets: none, weight, sum, meas, meas_target, the arrays the case's.

Two yardsticks per (case, option set, variant): the reference, one orc.cref_apply(monotonic=True, nz=1) per level, where oracle/_ref
is built; plain(), a float64 loop that generalises sweep_cases._mono_xdata and ._sweep to levels.  plain() always runs first: the
reference would end the process on the fatal check.  Neither yardstick has the per-level global sum: the device reduces its row sums
as a tree, so gsum_out[k] is pinned to fg_plan_apply_ex(monotonic, nz = 1)'s bits, as the header states it.

fatal_level(): a steep level of long-201-1t's recipe scaled by 1e8 -- an ulp is then about 1.2e-7 > 1e-10 -- with the first seed at which
plain() finds an excess of at least 1e-10."""
import functools
import zlib

import numpy as np

import orc
import sweep_cases as sc

MISSING, NLEV, K_FULL, K_NONE = sc.MISSING, sc.NLEV, sc.K_FULL, sc.K_NONE
CASES = ("spike-804-1t", "eights-804-1t", "long-201-1t", "mid-201-1t", "huge-99-1t")
BINS = {"spike-804-1t": "<=6", "eights-804-1t": "<=6", "mid-201-1t": "7..24", "long-201-1t": "25..96", "huge-99-1t": ">96"}
OPTS = ("none", "weight", "sum", "meas", "meas_target")
SETS = tuple((o, m) for o in OPTS for m in (False, True))
TOLERANCE = 1.0e-10
FATAL_CASE, FATAL_SCALE = "long-201-1t", 1.0e8
STEEP_LEVELS, STEEP = (2, 9, 16), 100.0                              # one level per chunk of eight whose gradients are 100 times steeper
MSG_ABOVE, MSG_BELOW = " xdata is greater than f_bar_max ", " xdata is less than f_bar_min "


class LimiterFatal(Exception):
    """the reference's mpp_error of :697 / :709"""
    def __init__(self, message, level, excess):
        super().__init__(f"{message!r} on level {level}: excess {excess!r}")
        self.message, self.level, self.excess = message, level, excess


def set_id(opt, masked):
    return f"{opt}-{'masked' if masked else 'unmasked'}"


def _tame(rng, n, scale=1.0):
    return rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 10.0, n) * scale


def _draw_level(c, seed, scale=1.0, steep=False):
    rng = np.random.default_rng(seed)
    g = scale * (STEEP if steep else 1.0)
    return dict(frame=_tame(rng, c["nhalo"], scale), vals=_tame(rng, c["nsrc"], scale), gx=_tame(rng, c["nsrc"], g), gy=_tame(rng, c["nsrc"], g))


@functools.lru_cache(maxsize=None)
def values(name):
    """{frame [NLEV][nhalo], vals, gx, gy [NLEV][nsrc]}: the seed is drawn per (case, level)"""
    c = sc.make(name)
    assert c["one_tile"]
    lv = [_draw_level(c, [zlib.crc32(name.encode()), 0x6D6F6E6F, k], steep=k in STEEP_LEVELS) for k in range(NLEV)]
    return {key: np.stack([l[key] for l in lv]) for key in ("frame", "vals", "gx", "gy")}


def _field(c, frame, vals, miss):
    f = frame.copy()
    f[:, c["inner"]] = vals if miss is None else np.where(miss, MISSING, vals)
    return np.ascontiguousarray(f)


def _options(c, opt):
    assert opt in OPTS
    return dict(weight=c["weight"] if opt == "weight" else None, sum=opt == "sum",
                field_area=c["field_area"] if opt in ("meas", "meas_target") else None,
                cell_area_in=c["cell_area_in"] if opt in ("sum", "meas", "meas_target") else None,
                cell_area_out=c["cell_area_out"] if opt == "meas_target" else None)


def inputs(name, opt, masked, with_gm=None):
    """the arguments of one sweep of NLEV levels: data [NLEV][nhalo] with the halo, gx / gy [NLEV][nsrc], gm int32 [NLEV][nsrc] or None"""
    c, v = sc.make(name), values(name)
    with_gm = masked if with_gm is None else with_gm
    kw = dict(data=_field(c, v["frame"], v["vals"], c["miss"] if masked else None), gx=v["gx"], gy=v["gy"],
              gm=c["gm"] if with_gm else None, has_missing=masked, missing=MISSING if masked else -1.0e20)
    kw.update(_options(c, opt))
    return kw


# ------------------------------------------------------------------------------------------------------------ the plain loop
def limited(c, kw):
    """conserve_interp.c:621-714 on every level of kw: (xdata [L][nx], facts).  Raises LimiterFatal where the reference's fatal
    check fires.  facts: per level whether each branch was taken, how many values the 1e-10 snap caught, the largest excess;
    `limited_src` [L][nsrc] marks the source cells whose values were limited."""
    (nx, ny), = c["tiles"]
    s, fi, x, missing = c["src"], c["fidx"], c["x"], kw["missing"]
    f, gx, gy, gm = kw["data"], kw["gx"], kw["gy"], kw["gm"]
    L = f.shape[0]
    f3 = f.reshape(L, ny + 2, nx + 2)
    nb = np.stack([f3[:, 1 + dj:1 + dj + ny, 1 + di:1 + di + nx].reshape(L, -1) for dj in (-1, 0, 1) for di in (-1, 0, 1)])
    fbmax = np.max(np.where(nb != missing, nb, -1.0e20), axis=0)
    fbmin = np.min(np.where(nb != missing, nb, 1.0e20), axis=0)
    fbar = f[:, fi]
    full = (fbar + gx[:, s] * x["di"]) + gy[:, s] * x["dj"]
    xd = full if gm is None else np.where(gm[:, s] != 0, fbar, full)
    ok = fbar != missing
    xd = np.where(ok, xd, missing)
    fmax, fmin = np.full((L, c["nsrc"]), -1.0e20), np.full((L, c["nsrc"]), 1.0e20)
    for k in range(L):
        np.maximum.at(fmax[k], s[ok[k]], xd[k][ok[k]])
        np.minimum.at(fmin[k], s[ok[k]], xd[k][ok[k]])
    live = xd != missing                                             # :687
    bmx, bmn, mx, mn = fbmax[:, s], fbmin[:, s], fmax[:, s], fmin[:, s]
    up = live & (mx > bmx)
    dn = live & ~up & (mn < bmn)
    with np.errstate(all="ignore"):
        xu = fbar + ((xd - fbar) / (mx - fbar)) * (bmx - fbar)
        xl = fbar + ((xd - fbar) / (mn - fbar)) * (bmn - fbar)
    over, under = up & (xu > bmx), dn & (xl < bmn)
    exc_u, exc_l = np.where(over, xu - bmx, 0.0), np.where(under, bmn - xl, 0.0)
    for k in range(L):
        if np.any(exc_u[k] >= TOLERANCE) or np.any(exc_l[k] >= TOLERANCE):
            n_u = int(np.argmax(exc_u[k] >= TOLERANCE)) if np.any(exc_u[k] >= TOLERANCE) else c["nx"]
            n_l = int(np.argmax(exc_l[k] >= TOLERANCE)) if np.any(exc_l[k] >= TOLERANCE) else c["nx"]
            # the reference walks the list and stops at the first; the device reports ABOVE before BELOW (ex_error_word)
            raise LimiterFatal(MSG_ABOVE if n_u < c["nx"] else MSG_BELOW, k, float(max(exc_u[k].max(), exc_l[k].max())))
    xu = np.where(over, bmx, xu)
    xl = np.where(under, bmn, xl)
    out = np.where(up, xu, np.where(dn, xl, xd))
    lim = np.zeros((L, c["nsrc"]), dtype=bool)
    for k in range(L):
        lim[k, s[up[k] | dn[k]]] = True
    facts = dict(up=np.any(up, axis=1), dn=np.any(dn, axis=1), snaps=np.count_nonzero(over | under, axis=1),
                 excess=np.maximum(exc_u.max(axis=1, initial=0.0), exc_l.max(axis=1, initial=0.0)), limited_src=lim)
    return out, facts


def sweep(c, kw, xdata):
    """:722-740 and :815-866 on the limited values xdata [L][nx]: every sum in float64 and in list order, vectorised over the levels
    and the rows (step r adds cell r of every row that has one).  The branch never sets out_miss."""
    x, s, d, missing = c["x"], c["src"], c["dst"], kw["missing"]
    L, ndst = xdata.shape[0], c["ndst"]
    a0 = x["area"]
    a = a0 * kw["weight"][s] if kw["weight"] is not None else a0
    if kw["sum"]:
        a = a / kw["cell_area_in"][s]
    elif kw["field_area"] is not None:
        a = a * (kw["field_area"][s] / kw["cell_area_in"][s])
    valid = xdata != missing
    p = xdata * a
    t = (a0 * kw["field_area"][s] / kw["cell_area_in"][s]) if kw["field_area"] is not None else a0
    csr = np.argsort(d, kind="stable")
    lens, row_ptr = c["lens"], c["row_ptr"]
    acc, asum, asum_t = np.zeros((L, ndst)), np.zeros((L, ndst)), np.zeros(ndst)
    by_len = np.argsort(-lens, kind="stable")
    longest = int(lens.max(initial=0))
    nrows = np.searchsorted(-lens[by_len], -np.arange(longest), side="left")                     # rows longer than r
    for r in range(longest):
        rows = by_len[:nrows[r]]
        n = csr[row_ptr[rows] + r]
        ok = valid[:, n]
        acc[:, rows] = np.where(ok, acc[:, rows] + p[:, n], acc[:, rows])
        asum[:, rows] = np.where(ok, asum[:, rows] + a[n], asum[:, rows])
        asum_t[rows] += t[n]
    with np.errstate(all="ignore"):
        if kw["sum"]:
            return np.where(asum == 0, missing, acc)
        out = np.where(asum > 0, acc / asum, missing)
        if kw["cell_area_out"] is not None:
            out = np.where(out != missing, out * (asum_t / kw["cell_area_out"]), out)
    return out


def plain_kw(c, kw):
    xd, facts = limited(c, kw)
    return sweep(c, kw, xd), facts


@functools.lru_cache(maxsize=None)
def plain(name, opt, masked, with_gm=None):
    """([NLEV][ndst], facts of the limiter)"""
    return plain_kw(sc.make(name), inputs(name, opt, masked, with_gm))


def reference_kw(c, kw):
    """one orc.cref_apply(monotonic=True, nz=1) per level"""
    pt = lambda a: [np.ascontiguousarray(a).ravel()] if a is not None else None
    L = kw["data"].shape[0]
    out = np.empty((L, c["ndst"]))
    for k in range(L):
        out[k], _ = orc.cref_apply(2, c["x"], c["tnx"], c["tny"], pt(kw["data"][k]), pt(kw["gx"][k]), pt(kw["gy"][k]),
                                   pt(kw["gm"][k]) if kw["gm"] is not None else None, kw["has_missing"], kw["missing"], c["nxo"], c["nyo"], 1,
                                   weight=pt(kw["weight"]), cell_methods_sum=kw["sum"], field_area=pt(kw["field_area"]),
                                   cell_area_in=pt(kw["cell_area_in"]), target_grid=kw["cell_area_out"] is not None,
                                   cell_area_out=kw["cell_area_out"], monotonic=True)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, opt, masked, with_gm=None):
    plain(name, opt, masked, with_gm)                                # raises where the reference would end the process
    return reference_kw(sc.make(name), inputs(name, opt, masked, with_gm))


def yardstick(name, opt, masked, with_gm=None):
    """(which, [NLEV][ndst]): the reference library where it is built, else the plain loop"""
    if orc.conserve_ref_available():
        return "reference", reference(name, opt, masked, with_gm)
    return "plain", plain(name, opt, masked, with_gm)[0]


# ------------------------------------------------------------------------------------------------------------ preconditions
def check_preconditions(name):
    """asserted, not skipped: a case that misses one is an error"""
    c = sc.make(name)
    assert c["one_tile"] and c["bin"] == BINS[name], (name, c["bin"])
    lo, hi = sc.BINS[c["bin"]]
    assert lo <= c["nx"] // c["ndst"] <= hi
    used = np.zeros(c["nsrc"], dtype=bool)
    used[c["src"]] = True
    # a source cell whose exchange cells lie in two different destination rows
    first_row = np.full(c["nsrc"], -1)
    first_row[c["src"][::-1]] = c["dst"][::-1]
    spread = np.zeros(c["nsrc"], dtype=bool)
    spread[c["src"][c["dst"] != first_row[c["src"]]]] = True
    for masked in (False, True):
        for with_gm in ((None,) if masked else (None, True)):
            out, facts = plain(name, "none", masked, with_gm)        # (did not raise: no fatal excess on any level)
            assert np.all(facts["excess"] < 1e-12), (name, masked, facts["excess"].max())
            live = [k for k in range(NLEV) if not (masked and k == K_NONE)]
            assert np.all(facts["up"][live]) and np.all(facts["dn"][live]), (name, masked)
            assert np.any(facts["snaps"] > 0), (name, masked)
            assert np.any(facts["limited_src"] & spread[None, :]), (name, masked)
            if masked:
                assert not facts["up"][K_NONE] and not facts["dn"][K_NONE]
                for opt in OPTS:
                    assert np.all(plain(name, opt, True)[0][K_NONE] == MISSING), (name, opt)
                assert np.any(out[K_FULL] != MISSING)
    return dict(unused_sources=int(np.count_nonzero(~used)))


def check_all_preconditions():
    """... and over the cases: at least one source cell has no exchange cell at all (the long-row lists use every source cell:
    15 000 cells drawn from 1 073)"""
    unused = {name: check_preconditions(name)["unused_sources"] for name in CASES}
    assert unused["spike-804-1t"] > 0 and unused["eights-804-1t"] > 0, unused
    return unused


# ------------------------------------------------------------------------------------------------------------ the fatal input
@functools.lru_cache(maxsize=None)
def fatal_level():
    """(seed, {data [1][nhalo], gx, gy [1][nsrc]}, LimiterFatal): level 0 of FATAL_CASE's recipe times FATAL_SCALE, unmasked, at the
    first seed whose excess reaches 1e-10"""
    c = sc.make(FATAL_CASE)
    for seed in range(64):
        lv = _draw_level(c, [zlib.crc32(FATAL_CASE.encode()), 0x66617461, seed], FATAL_SCALE, steep=True)
        kw = dict(data=_field(c, lv["frame"][None], lv["vals"][None], None), gx=lv["gx"][None], gy=lv["gy"][None], gm=None, has_missing=False,
                  missing=-1.0e20)
        kw.update(_options(c, "none"))
        try:
            limited(c, kw)
        except LimiterFatal as e:
            assert e.excess >= TOLERANCE
            return seed, kw, e
    raise AssertionError("no seed gives a fatal excess")


def with_fatal_level(name, position, nlev):
    """nlev tame unmasked levels of `name` (= FATAL_CASE) with the fatal level at `position`"""
    assert name == FATAL_CASE
    kw = inputs(name, "none", False)
    _, bad, _ = fatal_level()
    out = {k: (np.ascontiguousarray(kw[k][:nlev]).copy() if isinstance(kw[k], np.ndarray) and kw[k].ndim == 2 and kw[k].shape[0] == NLEV else kw[k])
           for k in kw}
    for k in ("data", "gx", "gy"):
        out[k][position] = bad[k][0]
    return out
