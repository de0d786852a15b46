"""Bilinear cubed-sphere -> lat-lon on the MI355X against the reference's own bilinear_interp.c (oracle/_ref/libbilinear_ref.so),
past the C24 fixtures.  Both sides get the same halo'd centres: this repository's gnomonic generator and fg_halo_map.

A. The apply kernels with the search taken out: a plan built from the reference's own index / weight (the READ-branch
   constructor) must give every output bit for bit -- scalar and vector, every (has_missing, fill_missing), nz = 4 levels in
   one device call against one-level reference calls.
B. The search and the weights: index identical at every point, weights within 2 ulp and >= 99.9 % bit-identical, and the
   fields of A through the device's own plan within close_fields (without has_missing only the level free of missing
   values: elsewhere a last-place weight difference moves sums of -1e20 onto or off the missing value).

Every reference setup runs in a child process (orc.bref_setup_child), all cases at once when the module first needs them."""
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import __graft_entry__
import orc
from test_gpu_bilinear import close_fields, ulps

pytestmark = pytest.mark.gpu
MISSING = -1.0e20
FG_ERR_BILIN_NOTFOUND = -11


def _corner_window():
    """+-12 degrees around the cube corner shared by tiles 1, 2 and 3 (the generator's corner (i, j) = (N, 0) of tile 1)"""
    fg = __graft_entry__.load_package()
    lonc, latc, _, _ = fg.gnomonic_ed_grid(48)
    lo = float(np.degrees(np.asarray(lonc[0]).reshape(49, 49)[0, -1]))
    la = float(np.degrees(np.asarray(latc[0]).reshape(49, 49)[0, -1]))
    return dict(lonbegin=lo - 12.0, lonend=lo + 12.0, latbegin=la - 12.0, latend=la + 12.0)


def _case(name, N, nlon, nlat, fs=0, **kw):
    return dict(name=name, N=N, nlon=nlon, nlat=nlat, finer_step=fs, **kw)


CASES = [
    _case("c48_144x73_fs0", 48, 144, 73),
    _case("c96_360x181_fs0", 96, 360, 181),
    _case("c96_180x91_fs1", 96, 180, 91, 1),
    _case("c48_72x37_fs2", 48, 72, 37, 2),
    _case("c48_36x19_fs3", 48, 36, 19, 3),
    _case("c25_72x37_fs0", 25, 72, 37),
    _case("c45_90x46_centery", 45, 90, 46, center_y=True),
    _case("c48_corner_window", 48, 48, 49, corner=True),
    _case("c48_polar_fs1", 48, 180, 16, 1, latbegin=60.0, latend=90.0),
    _case("c48_regional_fs2", 48, 80, 51, 2, lonbegin=230.0, lonend=310.0, latbegin=15.0, latend=65.0),
    _case("c24_4x2", 24, 4, 2),
    _case("c48_eps_lon", 48, 144, 73, lonbegin=1e-11, lonend=360.0 + 1e-11),
    _case("c24_lon_m180", 24, 72, 37, lonbegin=-180.0, lonend=180.0),
    _case("c48_lon_m180", 48, 144, 73, lonbegin=-180.0, lonend=180.0),
    _case("c384_1440x721_fs0", 384, 1440, 721),
]
IDS = [c["name"] for c in CASES]
BYNAME = {c["name"]: c for c in CASES}
COMBOS = [(False, False), (False, True), (True, False), (True, True)]       # (has_missing, fill_missing)
VARIANTS = ["u", "v", "uv"]                                                  # where the vector levels carry missing values


def cfg_of(case):
    c = {k: case[k] for k in ("N", "nlon", "nlat", "finer_step")}
    if case.get("corner"):
        c.update(_corner_window())
    for k in ("center_y", "lonbegin", "lonend", "latbegin", "latend"):
        if k in case:
            c[k] = case[k]
    return c


@pytest.fixture(scope="module")
def fg():
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    return fg


_GRID = {}


def grid(fg, N):
    """(contacts, lont [6][N,N], latt, lont_h, latt_h, halo, vlon_in, vlat_in)"""
    if N not in _GRID:
        lonc, latc, lont, latt = fg.gnomonic_ed_grid(N)
        contacts = fg.find_contacts([N] * 6, [N] * 6, list(lonc), list(latc))
        _, m = fg.halo_map([N] * 6, [N] * 6, contacts)
        e = np.nonzero(m >= 0)[0]

        def halo(tiles):
            h = np.zeros((6, N + 2, N + 2))
            h[:, 1:-1, 1:-1] = np.asarray(tiles).reshape(6, N, N)
            h = h.reshape(-1)
            h[e] = h[m[e]]
            return h.reshape(6, N + 2, N + 2)
        lont = [np.asarray(a).reshape(N, N) for a in lont]
        latt = [np.asarray(a).reshape(N, N) for a in latt]
        lh, ah = halo(lont), halo(latt)
        vi, wi = orc.bref_unit_vect_latlon(lh, ah)
        _GRID[N] = (contacts, lont, latt, lh, ah, halo, vi, wi)
    return _GRID[N]


@pytest.fixture(scope="module")
def refs(fg):
    """one reference setup per case, in child processes, all at once: name -> (setup or None, fell_back, printed)"""
    if not orc.bilinear_ref_available():
        pytest.fail("oracle/_ref/libbilinear_ref.so is missing: build() makes it where the reference exists")
    for N in sorted({c["N"] for c in CASES}):
        grid(fg, N)
    tmp = tempfile.mkdtemp(prefix="bref_")

    def run(case):
        wd = os.path.join(tmp, case["name"])
        os.makedirs(wd)
        g = _GRID[case["N"]]
        r, printed, fell_back = orc.bref_setup_child(cfg_of(case), g[3], g[4], wd, timeout=300)
        return case["name"], (r, fell_back, printed)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(ex.map(run, CASES))


def levels(case, lont, latt):
    """nz = 4 source levels [4, 6, N, N] of s, u, v and their missing masks: none; every 37th cell; 3x3 blocks (all four
    corners of the cells inside them missing); everything but tile 2"""
    N = case["N"]
    lo, la = np.stack(lont), np.stack(latt)
    k = np.arange(4.0)[:, None, None, None]
    s = 10.0 * np.sin(lo + la + 0.3 * k) + 3.0 * np.cos(2.0 * la) + k
    u = 20.0 * np.cos(la) + 5.0 * np.sin(2.0 * lo + k) + 0.0 * k
    v = 8.0 * np.sin(lo - 0.2 * k) * np.cos(la) + 0.0 * k
    mask = np.zeros((4, 6, N, N), dtype=bool)
    mask[1].reshape(-1)[::37] = True
    jj, ii = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    mask[2][:, (ii % 9 < 3) & (jj % 9 < 3)] = True
    mask[3][[0, 1, 3, 4, 5]] = True
    return s, u, v, mask


_REF_OUT = {}


def reference_outputs(fg, case, r):
    """the reference's one-level applies with its own plan, for every field A and B compare: key -> [4, nlat, nlon]"""
    name = case["name"]
    if name in _REF_OUT:
        return _REF_OUT[name]
    cfg = cfg_of(case)
    _, lont, latt, lh, ah, halo, vi, wi = grid(fg, case["N"])
    s, u, v, mask = levels(case, lont, latt)
    sm = np.where(mask, MISSING, s)
    out = {}
    for hm, fm in COMBOS:
        out[("s", hm, fm)] = (sm, np.stack([orc.bref_apply_scalar(cfg, r, halo(sm[k]), hm, MISSING, fm) for k in range(4)]))
        for var in VARIANTS:
            um = np.where(mask, MISSING, u) if "u" in var else u
            vm = np.where(mask, MISSING, v) if "v" in var else v
            res = [orc.bref_apply_vector(cfg, r, vi, wi, halo(um[k]), halo(vm[k]), hm, MISSING, fm) for k in range(4)]
            out[("vec", var, hm, fm)] = (um, vm, np.stack([a for a, _ in res]), np.stack([b for _, b in res]))
    _REF_OUT[name] = out
    return out


def device_plan(fg, case, **kw):
    cfg = cfg_of(case)
    contacts, lont, latt = grid(fg, case["N"])[:3]
    return fg.BilinearPlan(lont, latt, contacts, cfg["nlon"], cfg["nlat"], finer_step=cfg["finer_step"],
                           lonbegin=cfg.get("lonbegin", 0.0), lonend=cfg.get("lonend", 360.0), latbegin=cfg.get("latbegin", -90.0),
                           latend=cfg.get("latend", 90.0), center_y=bool(cfg.get("center_y", False)), **kw)


def fields_close(a, b):
    """close_fields, also for a field the reference leaves missing everywhere"""
    if np.all(np.asarray(b) == MISSING):
        assert np.all(np.asarray(a) == MISSING)
        return 1.0
    return close_fields(a, b, MISSING)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", IDS)
def test_apply_with_reference_plan_bit_identical(fg, refs, name):
    """A: the gather, the vector projection and rotation, the missing-value rules and the coarsening, nz = 4 in one call"""
    case = BYNAME[name]
    r, fell_back, printed = refs[name]
    if fell_back:
        assert "global sweep" in printed
        print(f"{name}: the reference took its global-sweep fallback; no reference plan (test B checks the refusal)")
        return
    assert "global sweep" not in printed
    out = reference_outputs(fg, case, r)
    N = case["N"]
    w = np.asarray(r["weight"])
    tied = int(np.sum(np.sum(w == w.max(axis=1, keepdims=True), axis=1) > 1))
    with device_plan(fg, case, index=r["index"], weight=r["weight"]) as p:
        for key, val in out.items():
            if key[0] == "s":
                _, hm, fm = key
                got = p.apply_scalar(val[0].reshape(4, 6 * N * N), hm, MISSING, fm).cpu().numpy()
                assert np.array_equal(bits(got), bits(val[1])), (key, int(np.sum(bits(got) != bits(val[1]))))
            else:
                _, var, hm, fm = key
                gu, gv = p.apply_vector(val[0].reshape(4, 6 * N * N), val[1].reshape(4, 6 * N * N), hm, MISSING, fm)
                for g_, ref in ((gu, val[2]), (gv, val[3])):
                    g_ = g_.cpu().numpy()
                    assert np.array_equal(bits(g_), bits(ref)), (key, int(np.sum(bits(g_) != bits(ref))))
    filled = ""
    if case["finer_step"] == 0:              # points whose value some level took from a tied maximum under fill_missing
        hit = np.any(out[("s", True, False)][1].reshape(4, -1) == MISSING, axis=0)
        tmask = np.sum(w == w.max(axis=1, keepdims=True), axis=1) > 1
        filled = f", {int(np.sum(hit & tmask))} of them filled from a missing corner"
    print(f"{name}: bit-identical at every point; fine points with a tied maximum weight {tied}{filled}")


@pytest.mark.parametrize("name", IDS)
def test_search_and_weights_match_reference(fg, refs, name):
    """B: the device search against the reference's: identical index, weights within 2 ulp, fields within close_fields"""
    case = BYNAME[name]
    r, fell_back, printed = refs[name]
    if fell_back:
        with pytest.raises(fg.FregridHipError) as e:
            device_plan(fg, case)
        assert e.value.code == FG_ERR_BILIN_NOTFOUND
        print(f"{name}: the reference fell back to its global sweep; the device refused with FG_ERR_BILIN_NOTFOUND")
        return
    N = case["N"]
    with device_plan(fg, case) as p:
        index, weight = p.index_weight()
        ties = p.ambiguous_ties
        bad = np.nonzero(np.any(index != r["index"], axis=1))[0]
        assert bad.size == 0, (bad.size, bad[:10], index[bad[:5]], r["index"][bad[:5]])
        u = ulps(weight, r["weight"])
        assert u.max() <= 2, u.max()
        frac_w = float(np.mean(u == 0))
        assert frac_w >= 0.999, frac_w
        out = reference_outputs(fg, case, r)
        fr = []
        for key, val in out.items():
            hm = key[1] if key[0] == "s" else key[2]
            lev = range(4) if hm else range(1)
            if key[0] == "s":
                got = p.apply_scalar(val[0].reshape(4, 6 * N * N), key[1], MISSING, key[2]).cpu().numpy()
                fr += [fields_close(got[k], val[1][k]) for k in lev]
            else:
                gu, gv = p.apply_vector(val[0].reshape(4, 6 * N * N), val[1].reshape(4, 6 * N * N), key[2], MISSING, key[3])
                gu, gv = gu.cpu().numpy(), gv.cpu().numpy()
                fr += [fields_close(gu[k], val[2][k]) for k in lev]
                fr += [fields_close(gv[k], val[3][k]) for k in lev]
    print(f"{name}: reference fell back: no; index identical; weights bit-identical {frac_w:.6f} (max {int(u.max())} ulp); "
          f"ambiguous_ties {ties}; fields bit-identical min {min(fr):.6f} mean {float(np.mean(fr)):.6f}")
