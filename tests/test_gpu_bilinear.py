"""Bilinear cubed-sphere -> lat-lon on the MI355X against the reference's own bilinear_interp.c (fixtures from
tests/golden/make_golden_bilinear.py) and, at C384 -> 0.25 degree, against its defining properties."""
import glob
import os

import numpy as np
import pytest

import __graft_entry__

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "bilinear_c24_*.npz")))


@pytest.fixture(scope="module")
def fg():
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    return fg


_MOSAIC = {}


def mosaic(fg, N):
    if N not in _MOSAIC:
        lonc, latc, lont, latt = fg.gnomonic_ed_grid(N)
        contacts = fg.find_contacts([N] * 6, [N] * 6, list(lonc), list(latc))
        _MOSAIC[N] = (contacts, [np.asarray(a).reshape(N, N) for a in lont], [np.asarray(a).reshape(N, N) for a in latt])
    return _MOSAIC[N]


def plan_for(fg, d, **kw):
    N, nlon, nlat, fs, cy, lb, le, ab, ae, _ = d["config"]
    contacts, lont, latt = mosaic(fg, int(N))
    return fg.BilinearPlan(lont, latt, contacts, int(nlon), int(nlat), finer_step=int(fs), lonbegin=lb, lonend=le, latbegin=ab,
                           latend=ae, center_y=bool(cy), **kw)


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    ia, ib = a.view(np.int64), b.view(np.int64)
    ia = np.where(ia < 0, np.int64(-0x8000000000000000) - ia, ia)
    ib = np.where(ib < 0, np.int64(-0x8000000000000000) - ib, ib)
    return np.abs(ia - ib)


def close_fields(a, b, missing):
    """remapped values: missing exactly where the reference has it; elsewhere equal up to the rounding of weights that differ
    in the last place (reported as the bit-identical fraction)"""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    assert np.array_equal(a == missing, b == missing)
    ok = b != missing
    scale = np.max(np.abs(b[ok])) if ok.any() else 1.0
    assert np.max(np.abs(a[ok] - b[ok])) <= 1e-14 * scale, np.max(np.abs(a[ok] - b[ok]))
    frac = float(np.mean(a.view(np.int64) == b.view(np.int64)))
    assert frac >= 0.999, frac                  # only points whose weights differ in the last place differ
    return frac


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[9:-4] for p in CASES])
def test_index_weights_and_fields_match_reference(fg, path):
    d = np.load(path)
    missing = float(d["config"][9])
    with plan_for(fg, d) as p:
        index, weight = p.index_weight()
        assert np.array_equal(index, d["index"])                       # every point, every case
        ties = p.ambiguous_ties
        # acosl / acos / sin / asin come from the host libm as in the reference; what remains is a rare last-place rounding
        u = ulps(weight, d["weight"])
        assert u.max() <= 2, u.max()
        frac_w = float(np.mean(u == 0))
        assert frac_w >= 0.999, frac_w
        s = d["s"].reshape(1, -1)
        out = {"s_plain": p.apply_scalar(s), "s_missing": p.apply_scalar(d["s_miss"].reshape(1, -1), True, missing),
               "s_fill": p.apply_scalar(d["s_miss"].reshape(1, -1), True, missing, True)}
        uo, vo = p.apply_vector(d["u"].reshape(1, -1), d["v"].reshape(1, -1))
        out["u_out"], out["v_out"] = uo, vo
        fr = {k: close_fields(v.cpu().numpy()[0], d[k], missing) for k, v in out.items()}
    print(os.path.basename(path), "bit-identical weights", frac_w, "fields", fr, "ambiguous nearest-centre ties", ties)


def test_read_branch_equals_computed_plan(fg, tmp_path):
    d = np.load(CASES[[os.path.basename(c) for c in CASES].index("bilinear_c24_72x37_fs1.npz")])
    N, nlon, nlat, fs = (int(x) for x in d["config"][:4])
    contacts, lont, latt = mosaic(fg, N)
    path = str(tmp_path / "bilinear_remap.nc")
    p1 = fg.setup_bilinear_interp(lont, latt, contacts, nlon, nlat, opcode=512, remap_file=path, finer_step=fs)   # WRITE
    p2 = fg.setup_bilinear_interp(lont, latt, contacts, nlon, nlat, opcode=256, remap_file=path, finer_step=fs)   # READ
    i1, w1 = p1.index_weight()
    i2, w2 = p2.index_weight()
    assert np.array_equal(i1, i2) and np.array_equal(w1.view(np.int64), w2.view(np.int64))
    s = d["s_miss"].reshape(1, -1)
    a = fg.do_scalar_bilinear_interp(p1, s, True, -1e20, True)
    b = fg.do_scalar_bilinear_interp(p2, s, True, -1e20, True)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    ua, va = fg.do_vector_bilinear_interp(p1, d["u"].reshape(1, -1), d["v"].reshape(1, -1))
    ub, vb = fg.do_vector_bilinear_interp(p2, d["u"].reshape(1, -1), d["v"].reshape(1, -1))
    assert np.array_equal(ua.view(np.int64), ub.view(np.int64)) and np.array_equal(va.view(np.int64), vb.view(np.int64))


@pytest.mark.parametrize("name", ["c24_72x37_fs1", "c24_36x19_fs2"])
def test_nz_levels_equal_single_level_calls(fg, name):
    import torch
    d = np.load(os.path.join(ROOT, "tests", "golden", f"bilinear_{name}.npz"))
    rng = np.random.default_rng(5)
    with plan_for(fg, d) as p:
        base = d["s_miss"].reshape(-1)
        lev = np.stack([base * (1.0 + 0.1 * k) + rng.standard_normal(base.size) for k in range(8)])
        lev[:, ::37] = -1e20
        for hm, fill in ((False, False), (True, False), (True, True)):
            many = p.apply_scalar(lev, hm, -1e20, fill).cpu().numpy()
            one = np.stack([p.apply_scalar(lev[k:k + 1], hm, -1e20, fill).cpu().numpy()[0] for k in range(8)])
            assert np.array_equal(many.view(np.int64), one.view(np.int64)), (hm, fill)
        u = np.stack([d["u"].reshape(-1) * (1 + k) for k in range(8)])
        v = np.stack([d["v"].reshape(-1) * (2 - 0.1 * k) for k in range(8)])
        U, V = p.apply_vector(u, v)
        for k in range(8):
            uk, vk = p.apply_vector(u[k:k + 1], v[k:k + 1])
            assert torch.equal(U[k], uk[0]) and torch.equal(V[k], vk[0])


def test_c384_quarter_degree_properties(fg):
    """C384 -> 1440 x 721: every point found (creation fails otherwise), weights non-negative and summing to 1 within 4 ulp,
    a constant field reproduced to 1e-14 at finer_step 0 and 1, two runs bit-identical"""
    contacts, lont, latt = mosaic(fg, 384)
    res = []
    for fs, nlon, nlat in ((0, 1440, 721), (1, 720, 361)):
        p = fg.BilinearPlan(lont, latt, contacts, nlon, nlat, finer_step=fs)
        index, weight = p.index_weight()
        N = 384
        assert index[:, 0].min() >= 0 and index[:, 0].max() <= N and index[:, 1].min() >= 0 and index[:, 1].max() <= N
        assert index[:, 2].min() >= 0 and index[:, 2].max() <= 5
        assert weight.min() >= 0.0
        ssum = weight.sum(axis=1)
        assert np.max(np.abs(ssum - 1.0)) <= 4 * np.finfo(np.float64).eps, np.max(np.abs(ssum - 1.0))
        const = np.full((1, 6 * N * N), 7.25)
        out = p.apply_scalar(const).cpu().numpy()
        assert np.max(np.abs(out - 7.25)) <= 1e-14 * 7.25, np.max(np.abs(out - 7.25))
        res.append((index, weight))
        p.destroy()
    p = fg.BilinearPlan(lont, latt, contacts, 1440, 721, finer_step=0)
    i2, w2 = p.index_weight()
    assert np.array_equal(i2, res[0][0]) and np.array_equal(w2.view(np.int64), res[0][1].view(np.int64))


# ---- get_closest_index (bilinear_interp.c:648-818) on the host, vectorised, with the reference's spherical_angle: the
# products in double, acosl through numpy's long double (x86-64 x87)
def _sa(v1, v2, v3):
    px = v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1]
    py = v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2]
    pz = v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]
    qx = v1[:, 1] * v3[:, 2] - v1[:, 2] * v3[:, 1]
    qy = v1[:, 2] * v3[:, 0] - v1[:, 0] * v3[:, 2]
    qz = v1[:, 0] * v3[:, 1] - v1[:, 1] * v3[:, 0]
    ddd = (px * px + py * py + pz * pz) * (qx * qx + qy * qy + qz * qz)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (px * qx + py * qy + pz * qz) / np.sqrt(ddd)
    c = np.where(np.abs(c - 1) < 1e-30, 1.0, c)
    c = np.where(np.abs(c + 1) < 1e-30, -1.0, c)
    inside = (c >= -1.0) & (c <= 1.0)
    ang = np.where(c < 0, np.pi, 0.0)
    ang[inside] = np.arccos(c[inside].astype(np.longdouble)).astype(np.float64)
    return np.where(ddd <= 0.0, 0.0, ang)


def _le(a, b, c):
    m = np.where(a > b, a, b)
    return m <= c


def _closest(X, N, l, i, j, v0):
    """get_closest_index for cell (i, j) of tile l (arrays): (found, i_result, j_result)"""
    V = lambda jj, ii: X[l, jj, ii]
    v1, v2, v3 = V(j, i), V(j, i + 1), V(j + 1, i)
    b1 = _le(_sa(v1, v2, v0), _sa(v1, v3, v0), _sa(v1, v2, v3))
    corner = (i == N) & (j == N)
    v4 = V(j + 1, np.minimum(i + 1, N + 1))
    ok1 = np.where(corner, _le(_sa(v2, v1, v0), _sa(v2, v3, v0), _sa(v2, v3, v1)), _le(_sa(v4, v2, v0), _sa(v4, v3, v0), _sa(v4, v3, v2)))
    w4 = V(j, i - 1)
    b2 = _le(_sa(v1, v3, v0), _sa(v1, w4, v0), _sa(v1, v3, w4))
    v5, v6 = V(j + 1, i - 1), V(j, i - 1)
    c2 = (i == 1) & (j == N)
    ok2 = np.where(c2, _le(_sa(v3, w4, v0), _sa(v3, v1, v0), _sa(v3, v1, w4)), _le(_sa(v5, v6, v0), _sa(v5, v3, v0), _sa(v5, v3, v6)))
    u5, u6 = V(j, i - 1), V(j - 1, i)
    b3 = _le(_sa(v1, w4, v0), _sa(v1, u6, v0), _sa(v1, u5, u6)) & (i > 1) & (j > 1)
    v7 = V(j - 1, i - 1)
    ok3 = _le(_sa(v7, u5, v0), _sa(v7, u6, v0), _sa(v7, u6, u5))
    b4 = _le(_sa(v1, u6, v0), _sa(v1, v2, v0), _sa(v1, u6, v2))
    c4 = (i == N) & (j == 1)
    v8 = V(j - 1, np.minimum(i + 1, N + 1))
    ok4 = np.where(c4, _le(_sa(v2, u6, v0), _sa(v2, v1, v0), _sa(v2, v1, u6)), _le(_sa(v8, u6, v0), _sa(v8, v2, v0), _sa(v8, v2, u6)))
    found = np.where(b1, ok1, np.where(b2, ok2, np.where(b3, ok3, b4 & ok4)))
    ri = np.where(b1 | (~b2 & ~b3), i, i - 1)
    rj = np.where(b1 | b2, j, j - 1)
    return found, ri, rj


def test_c384_every_point_inside_its_cell_by_get_closest_index(fg):
    """C384 -> 1440 x 721 (no reference at this size): every lat-lon point's (ic, jc, tile) is what the reference's own
    get_closest_index returns for the point from one of that cell's four centres -- the test the search accepted it by"""
    import ctypes as C
    from fre_nctools_amd import bilinear
    N = 384
    contacts, lont, latt = mosaic(fg, N)
    p = fg.BilinearPlan(lont, latt, contacts, 1440, 721)
    print("C384 -> 1440x721 ambiguous nearest-centre ties", p.ambiguous_ties)
    index, _ = p.index_weight()
    p.destroy()
    _, m = fg.halo_map([N] * 6, [N] * 6, contacts)
    L = fg.lib()
    dp = C.POINTER(C.c_double)

    def xyz(lon, lat):
        lon, lat = np.ascontiguousarray(lon, dtype=np.float64).ravel(), np.ascontiguousarray(lat, dtype=np.float64).ravel()
        out = np.empty((3, lon.size))
        L.fg_latlon2xyz(lon.size, lon.ctypes.data_as(dp), lat.ctypes.data_as(dp), out[0].ctypes.data_as(dp),
                        out[1].ctypes.data_as(dp), out[2].ctypes.data_as(dp))
        return out.T.copy()

    def halo(tiles):
        h = np.zeros((6, N + 2, N + 2))
        h[:, 1:-1, 1:-1] = np.asarray(tiles).reshape(6, N, N)
        h = h.reshape(-1)
        e = np.nonzero(m >= 0)[0]
        h[e] = h[m[e]]
        return h
    X = xyz(halo(lont), halo(latt)).reshape(6, N + 2, N + 2, 3)
    lo, la, _ = bilinear.fine_grid(1440, 721)
    P = xyz(lo, la)
    ic, jc, l = index[:, 0], index[:, 1], index[:, 2]
    ok = np.zeros(len(P), dtype=bool)
    for di, dj, in ((0, 0), (1, 0), (1, 1), (0, 1)):           # the centre the search started from: (ic, jc) + (di, dj)
        bi, bj = ic + di, jc + dj
        sel = ~ok & (bi >= 1) & (bi <= N) & (bj >= 1) & (bj <= N)
        if not sel.any():
            continue
        f, ri, rj = _closest(X, N, l[sel], bi[sel], bj[sel], P[sel])
        hit = f & (ri == ic[sel]) & (rj == jc[sel])
        ok[np.nonzero(sel)[0][hit]] = True
    assert ok.all(), (int((~ok).sum()), np.nonzero(~ok)[0][:10])
