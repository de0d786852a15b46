"""GPU parity of the great-circle path (create_xgrid_great_circle semantics) against two builds of the
oracle (gc_oracle.c):
* the plain one, pinned bit for bit to the compiled reference: exchange-cell lists identical, areas within 1e-10 relative and
  more than 98 % of them bit-identical -- the allowance for the x87 fpatan inside glibc's acosl, which rounds an angle
  differently from the device's correctly rounded replacement (csrc/fp80.h's fg_acosl) once in a few thousand;
* the _cr one, the same text with fg_acosl, pinned to the plain one with every differing value accounted for
  (tests/test_gc_oracle_cr_cpu.py): ALL areas bit-identical, no tolerance and no allowed fraction."""
import numpy as np
import pytest

import gc_cases
import orc

pytestmark = pytest.mark.gpu
RTOL = 1e-10


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _nbits(a, b):
    """how many values differ in bits"""
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape
    return int(np.count_nonzero(a != b))


_cases = gc_cases.grid_cases


@pytest.mark.parametrize("name", ["c24_tile1_144x90", "c24_tile3_polar_144x90", "latlon_aligned_2x", "latlon_regional_offset",
                                  "latlon_to_cubed_polar", "tripolar_to_cubed"])
def test_create_xgrid_great_circle_vs_oracle(fg, gpu_ok, name):
    args = _cases(fg)[name]
    o = orc.orc_create_xgrid_gc(*args)
    n, i_in, j_in, i_out, j_out, area, clon, clat = fg.create_xgrid_great_circle(*args)
    assert n == o["n"] and n > 0
    assert np.array_equal(i_in, o["i_in"]) and np.array_equal(j_in, o["j_in"])
    assert np.array_equal(i_out, o["i_out"]) and np.array_equal(j_out, o["j_out"])
    rel = np.abs(area - o["area"]) / o["area"]
    assert rel.max() < RTOL
    same = np.mean(_bits(area) == _bits(o["area"]))
    assert same > 0.98, same                       # the rest: one final double rounding of an angle (fpatan vs exact)
    ocr = orc.orc_create_xgrid_gc(*args, cr=True)  # the oracle that rounds like the device: every value
    assert ocr["n"] == n
    nd = _nbits(area, ocr["area"])
    assert nd == 0, f"{nd} of {n} exchange-cell areas differ from the _cr oracle"
    assert not clon.any() and not clat.any()       # create_xgrid.c:1446-1447
    ca = fg.get_grid_great_circle_area(args[0], args[1], args[4], args[5])
    cref = orc.orc_get_grid_gc_area(args[0], args[1], args[4], args[5])
    assert np.max(np.abs(ca - cref) / np.abs(cref)) < RTOL
    assert np.mean(_bits(ca) == _bits(cref)) > 0.98
    for nx, ny, lo, la in (args[0:2] + args[4:6], args[2:4] + args[6:8]):
        nd = _nbits(fg.get_grid_great_circle_area(nx, ny, lo, la), orc.orc_get_grid_gc_area(nx, ny, lo, la, cr=True))
        assert nd == 0, f"{nd} of {nx * ny} grid-cell areas differ from the _cr oracle"


def test_clip_vertices_bitwise(fg, gpu_ok):
    """clip_2dx2d_great_circle vertex lists: the soft-x87 intersection solve reproduces the reference's vertices bit for
    bit (no acos involved in the vertices)."""
    import ctypes as C
    O = orc.oracle()
    lon, lat = fg.gnomonic_ed_corners(24)
    lo, la = fg.latlon_corners(144, 90)
    x1, y1, z1 = fg.latlon2xyz(lon[2], lat[2])
    x2, y2, z2 = fg.latlon2xyz(lo, la)
    ox, oy, oz = (np.empty(25 * 25) for _ in range(3))
    O.orc_latlon2xyz(25 * 25, orc._dp(orc.f64(lon[2]).ravel()), orc._dp(orc.f64(lat[2]).ravel()), orc._dp(ox), orc._dp(oy), orc._dp(oz))
    assert np.array_equal(_bits(x1), _bits(ox)) and np.array_equal(_bits(y1), _bits(oy)) and np.array_equal(_bits(z1), _bits(oz))
    cell = lambda x, nxp, i, j: np.array([x[j * nxp + i], x[(j + 1) * nxp + i], x[(j + 1) * nxp + i + 1], x[j * nxp + i + 1]])
    gc = orc.orc_create_xgrid_gc(24, 24, 144, 90, lon[2], lat[2], lo, la)
    idx = np.arange(0, gc["n"], 3)
    a = np.stack([np.stack([cell(v, 25, int(gc["i_in"][k]), int(gc["j_in"][k])) for v in (x1, y1, z1)], axis=1) for k in idx])
    b = np.stack([np.stack([cell(v, 145, int(gc["i_out"][k]), int(gc["j_out"][k])) for v in (x2, y2, z2)], axis=1) for k in idx])
    n_out, verts, area = fg.gc_clip_batch(a, b)
    nbad_area = nbad_cr = 0
    for q, k in enumerate(idx):
        aa = [np.ascontiguousarray(a[q][:, ax]) for ax in range(3)]
        bb = [np.ascontiguousarray(b[q][:, ax]) for ax in range(3)]
        oo = [np.zeros(50) for _ in range(3)]
        no = O.orc_clip_2dx2d_great_circle(*[orc._dp(v) for v in aa], 4, *[orc._dp(v) for v in bb], 4, *[orc._dp(v) for v in oo])
        assert no == n_out[q] and no >= 3
        for ax in range(3):
            assert np.array_equal(_bits(verts[q, :no, ax]), _bits(oo[ax][:no]))
        ar = O.orc_great_circle_area(no, *[orc._dp(v) for v in oo])
        assert abs(ar - area[q]) <= RTOL * abs(ar)
        nbad_area += ar != area[q]
        nbad_cr += _nbits(O.orc_great_circle_area_cr(no, *[orc._dp(v) for v in oo]), area[q])
    assert nbad_area < 0.02 * len(idx)
    assert nbad_cr == 0, f"{nbad_cr} of {len(idx)} areas differ from the _cr oracle"
    # an antipodal cell (whose edge planes do cross the first cell's chords) is rejected by the reference's bounding box
    # (create_xgrid.c:1508-1528) and so it is here
    anti = -a[0][::-1]
    n_far, _, _ = fg.gc_clip_batch(a[:1], anti[None])
    assert n_far[0] == 0


def test_setup_conserve_interp_great_circle_and_sweep(fg, gpu_ok, capsys):
    """opcode GREAT_CIRCLE through the mirror API: whole-tile search for all six tiles, first-order sweep, conservation."""
    ni, nlon, nlat = 16, 48, 24
    lon, lat = fg.gnomonic_ed_corners(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    grid_in = [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]
    grid_out = [fg.GridConfig(nlon, nlat, lo, la)]
    interp = [fg.InterpConfig()]
    fg.setup_conserve_interp(6, grid_in, 1, grid_out, interp, fg.CONSERVE_ORDER1 | fg.GREAT_CIRCLE)
    tot = 0
    for t in range(6):
        o = orc.orc_create_xgrid_gc(ni, ni, nlon, nlat, lon[t], lat[t], lo, la)
        sel = interp[0].t_in == t
        assert sel.sum() == o["n"]
        assert np.array_equal(interp[0].i_in[sel], o["i_in"]) and np.array_equal(interp[0].j_out[sel], o["j_out"])
        assert np.max(np.abs(interp[0].area[sel] - o["area"]) / o["area"]) < RTOL
        nd = _nbits(interp[0].area[sel], orc.orc_create_xgrid_gc(ni, ni, nlon, nlat, lon[t], lat[t], lo, la, cr=True)["area"])
        assert nd == 0, f"tile {t}: {nd} of {o['n']} exchange-cell areas differ from the _cr oracle"
        tot += o["n"]
    assert interp[0].nxgrid == tot
    R = 6371000.0
    assert abs(interp[0].area.sum() / (4 * np.pi * R * R) - 1) < 1e-9          # great-circle cells tile the sphere
    # cell areas handed back are the great-circle ones (get_input_output_cell_area with GREAT_CIRCLE)
    assert np.max(np.abs(grid_in[2].cell_area - orc.orc_get_grid_gc_area(ni, ni, lon[2], lat[2])) / grid_in[2].cell_area) < RTOL
    for t in range(6):
        nd = _nbits(grid_in[t].cell_area, orc.orc_get_grid_gc_area(ni, ni, lon[t], lat[t], cr=True))
        assert nd == 0, f"tile {t}: {nd} of {ni * ni} cell areas differ from the _cr oracle"
    rng = np.random.default_rng(2)
    field_in = [fg.FieldConfig(data=rng.standard_normal((1, ni, ni)) + 3.0, var=[fg.VarConfig(name="t", interp_method=fg.CONSERVE_ORDER1)])
                for _ in range(6)]
    field_out = [fg.FieldConfig()]
    gin, gout = fg.do_scalar_conserve_interp(interp, 0, 6, grid_in, 1, grid_out, field_in, field_out,
                                             fg.CONSERVE_ORDER1 | fg.CHECK_CONSERVE, 1)
    assert abs(gout - gin) < 1e-10 * abs(gin)
    with pytest.raises(ValueError):
        fg.setup_conserve_interp(6, grid_in, 1, grid_out, [fg.InterpConfig()], fg.CONSERVE_ORDER2 | fg.GREAT_CIRCLE)


def test_conserve_interp_great_circle_b1(fg, gpu_ok):
    """interp.c:312 drop-in against the same formula on the oracle's exchange cells (sum of area fractions per
    destination cell, in exchange-cell order)."""
    ni, nlon, nlat = 12, 36, 18
    lon, lat = fg.gnomonic_ed_corners(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    rng = np.random.default_rng(9)
    data = rng.standard_normal(ni * ni) + 2.0
    mask = np.ones(ni * ni); mask[5] = 0.0
    got = fg.conserve_interp_great_circle(ni, ni, nlon, nlat, lon[0], lat[0], lo, la, mask, data)
    o = orc.orc_create_xgrid_gc(ni, ni, nlon, nlat, lon[0], lat[0], lo, la, mask=mask)
    d = o["j_out"].astype(np.int64) * nlon + o["i_out"]
    dst_area = np.zeros(nlon * nlat)
    for k in range(o["n"]):
        dst_area[d[k]] += o["area"][k]
    ref = np.zeros(nlon * nlat)
    for k in range(o["n"]):
        ref[d[k]] += data[o["j_in"][k] * ni + o["i_in"][k]] * (o["area"][k] / dst_area[d[k]])
    assert np.max(np.abs(got - ref)) < 1e-12 * np.max(np.abs(ref))
    assert np.count_nonzero(got) == np.count_nonzero(ref) > 0
    # the same loop on the _cr oracle's areas: same addends in the same order, so the bits
    ocr = orc.orc_create_xgrid_gc(ni, ni, nlon, nlat, lon[0], lat[0], lo, la, mask=mask, cr=True)
    assert ocr["n"] == o["n"]
    dst_area = np.zeros(nlon * nlat)
    for k in range(o["n"]):
        dst_area[d[k]] += ocr["area"][k]
    ref_cr = np.zeros(nlon * nlat)
    for k in range(o["n"]):
        ref_cr[d[k]] += data[o["j_in"][k] * ni + o["i_in"][k]] * (ocr["area"][k] / dst_area[d[k]])
    nd = _nbits(got, ref_cr)
    assert nd == 0, f"{nd} of {nlon * nlat} destination values differ from the replay on the _cr oracle's areas"
    if orc.ref_available():                     # the reference's own conserve_interp_great_circle (interp.c:312)
        cref = np.empty(nlon * nlat)
        orc.ref().conserve_interp_great_circle(ni, ni, nlon, nlat, orc._dp(orc.f64(lon[0])), orc._dp(orc.f64(lat[0])),
                                               orc._dp(orc.f64(lo)), orc._dp(orc.f64(la)), orc._dp(mask), orc._dp(data),
                                               orc._dp(cref))
        assert np.max(np.abs(got - cref)) < 1e-12 * np.max(np.abs(cref))
        assert np.count_nonzero(got) == np.count_nonzero(cref) > 0


def test_great_circle_degenerate_cases(fg, gpu_ok):
    """Edge cases against the oracle: identical grids (every edge pair coincident: u snapped to 0/1 everywhere), disjoint
    regional grids (no exchange cells), single cells, and a masked-out source."""
    lo, la = fg.latlon_corners(24, 12)
    o = orc.orc_create_xgrid_gc(24, 12, 24, 12, lo, la, lo, la)
    r = fg.create_xgrid_great_circle(24, 12, 24, 12, lo, la, lo, la)
    assert r[0] == o["n"] and np.array_equal(r[1], o["i_in"]) and np.array_equal(r[3], o["i_out"]) and np.array_equal(r[4], o["j_out"])
    assert np.max(np.abs(r[5] - o["area"]) / o["area"]) < RTOL
    nd = _nbits(r[5], orc.orc_create_xgrid_gc(24, 12, 24, 12, lo, la, lo, la, cr=True)["area"])
    assert nd == 0, f"{nd} of {r[0]} areas differ from the _cr oracle"
    assert r[0] >= 24 * 12                              # every cell at least meets itself
    lon, lat = fg.gnomonic_ed_corners(8)
    o = orc.orc_create_xgrid_gc(8, 8, 8, 8, lon[3], lat[3], lon[3], lat[3])
    r = fg.create_xgrid_great_circle(8, 8, 8, 8, lon[3], lat[3], lon[3], lat[3])
    assert r[0] == o["n"] and np.array_equal(r[3], o["i_out"]) and np.array_equal(r[4], o["j_out"])
    assert np.max(np.abs(r[5] - o["area"]) / o["area"]) < RTOL
    nd = _nbits(r[5], orc.orc_create_xgrid_gc(8, 8, 8, 8, lon[3], lat[3], lon[3], lat[3], cr=True)["area"])
    assert nd == 0, f"{nd} of {r[0]} areas differ from the _cr oracle"
    # disjoint regions
    lo1, la1 = fg.latlon_corners(6, 6, 10.0, 40.0, 10.0, 40.0)
    lo2, la2 = fg.latlon_corners(5, 5, 100.0, 140.0, -40.0, -10.0)
    assert orc.orc_create_xgrid_gc(6, 6, 5, 5, lo1, la1, lo2, la2)["n"] == 0
    assert orc.orc_create_xgrid_gc(6, 6, 5, 5, lo1, la1, lo2, la2, cr=True)["n"] == 0
    assert fg.create_xgrid_great_circle(6, 6, 5, 5, lo1, la1, lo2, la2)[0] == 0
    # single cells, partial overlap
    lo3, la3 = fg.latlon_corners(1, 1, 10.0, 20.0, 10.0, 20.0)
    lo4, la4 = fg.latlon_corners(1, 1, 15.0, 30.0, 5.0, 15.0)
    o = orc.orc_create_xgrid_gc(1, 1, 1, 1, lo3, la3, lo4, la4)
    r = fg.create_xgrid_great_circle(1, 1, 1, 1, lo3, la3, lo4, la4)
    assert r[0] == o["n"] == 1 and abs(r[5][0] - o["area"][0]) < RTOL * o["area"][0]
    nd = _nbits(r[5], orc.orc_create_xgrid_gc(1, 1, 1, 1, lo3, la3, lo4, la4, cr=True)["area"])
    assert nd == 0, f"{nd} of 1 areas differ from the _cr oracle"
    # fully masked source
    r = fg.create_xgrid_great_circle(6, 6, 6, 6, lo1, la1, lo1, la1, mask_in=np.zeros(36))
    assert r[0] == 0
    # partly masked source (the exchange-cell area is multiplied by the mask value)
    (margs, mask) = gc_cases.degenerate_cases(fg)["masked_cubed_to_latlon"]
    o = orc.orc_create_xgrid_gc(*margs, mask=mask)
    r = fg.create_xgrid_great_circle(*margs, mask_in=mask)
    assert r[0] == o["n"] > 0 and np.array_equal(r[1], o["i_in"]) and np.array_equal(r[2], o["j_in"])
    assert np.array_equal(r[3], o["i_out"]) and np.array_equal(r[4], o["j_out"])
    assert np.max(np.abs(r[5] - o["area"]) / o["area"]) < RTOL
    nd = _nbits(r[5], orc.orc_create_xgrid_gc(*margs, mask=mask, cr=True)["area"])
    assert nd == 0, f"{nd} of {r[0]} areas differ from the _cr oracle"


@pytest.mark.parametrize("ni,nlon,nlat", [(24, 144, 90), (96, 360, 180), (48, 1440, 720)])
def test_three_pass_clip_equals_the_one_kernel_clip(fg, gpu_ok, ni, nlon, nlat):
    """The great-circle clip runs as three passes (k_gc_screen / k_gc_solve / k_gc_walk) for ordinary pairs and as the
    one-kernel clip (the version pinned to the oracle above) for the rest.  Here every pair goes through each of the two
    and the plans must be bit-identical; only a small fraction of the pairs may be handed back by the three passes."""
    lon, lat = fg.gnomonic_ed_corners(ni)
    lo, la = fg.latlon_corners(nlon, nlat)
    grids = [fg.GridConfig(ni, ni, lon[t], lat[t]) for t in range(6)]
    res = []
    try:
        # one kernel | three passes | three passes with a task buffer 64 times too small
        for split in (0, 1, 2):
            fg.lib().fg_set_gc_split(split)
            plan = fg.XgridPlan.create_great_circle(grids, fg.GridConfig(nlon, nlat, lo, la))
            plan.finalize()
            res.append((plan.get_xgrid(), plan.stats()))
            plan.destroy()
    finally:
        fg.lib().fg_set_gc_split(1)
    a, sa = res[0]
    assert len(a["area"]) > 0 and sa["deferred"] == 0
    for b, sb in res[1:]:
        assert len(a["area"]) == len(b["area"])
        for k in ("t_in", "i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(a[k], b[k])
        assert np.array_equal(_bits(a["area"]), _bits(b["area"]))
        assert sa["below"] == sb["below"] and sa["borderline"] == sb["borderline"]
    assert res[1][1]["deferred"] < 0.1 * sa["pairs"] + 4000   # pole cells, tile-edge cells on lat-lon lines, snapped intersections
    assert res[2][1]["deferred"] > 0.1 * sa["pairs"]          # the overflow path really ran


def test_three_pass_clip_on_awkward_grid_pairs(fg, gpu_ok):
    """Pairs of grids chosen to sit on the branches of the three-pass clip: edges and corners that almost coincide (shifts of
    1e-9 .. 1e-5 rad: snapped, nearly snapped and borderline-inside cases), generic crossings at odd angles (rotated grids),
    coarse against fine, tripolar folds, regional windows (gc_cases.awkward_pairs).  Three passes == one-kernel clip bit for bit;
    the small cases also against the oracle: lists, areas to 1e-10 against the plain build and in bits against the _cr build."""
    cases = gc_cases.awkward_pairs(fg)
    def run(args):
        """plan API (errors come back as exceptions instead of the reference's exit): (xgrid dict | None, message)"""
        nxi, nyi, nxo, nyo, loi, lai, loo, lao = args
        try:
            plan = fg.XgridPlan.create_great_circle([fg.GridConfig(nxi, nyi, loi, lai)], fg.GridConfig(nxo, nyo, loo, lao))
        except Exception as e:                       # the reference's own fatal checks (mpp_error) on this input
            return None, str(e)
        x = plan.get_xgrid() if plan.nxgrid else {"area": np.zeros(0)}
        plan.destroy()
        return x, ""

    nok = 0
    for ci, args in enumerate(cases):
        outs = []
        try:
            for split in (0, 1):
                fg.lib().fg_set_gc_split(split)
                outs.append(run(args))
        finally:
            fg.lib().fg_set_gc_split(1)
        (a, ea), (b, eb) = outs
        assert ea == eb, (ci, ea, eb)                # same fatal check, same message -- or none
        if a is None:
            continue
        nok += 1
        assert len(a["area"]) == len(b["area"]), ci
        if len(a["area"]) == 0:
            continue
        for k in ("i_in", "j_in", "i_out", "j_out"):
            assert np.array_equal(a[k], b[k]), (ci, k)
        assert np.array_equal(_bits(a["area"]), _bits(b["area"])), ci
        if args[0] * args[1] * args[2] * args[3] <= 40 * 30 * 40 * 30:
            o = orc.orc_create_xgrid_gc(*args)
            assert len(b["area"]) == o["n"], ci
            assert np.array_equal(b["i_in"], o["i_in"]) and np.array_equal(b["j_in"], o["j_in"]), ci
            assert np.array_equal(b["i_out"], o["i_out"]) and np.array_equal(b["j_out"], o["j_out"]), ci
            assert np.max(np.abs(b["area"] - o["area"]) / o["area"]) < RTOL, ci
            nd = _nbits(b["area"], orc.orc_create_xgrid_gc(*args, cr=True)["area"])
            assert nd == 0, f"case {ci}: {nd} of {o['n']} areas differ from the _cr oracle"
    assert nok >= 5


@pytest.fixture(scope="module")
def crafted():
    """the crafted batch with what the oracle makes of it, computed once: n_out and vertices from the plain build, areas from the
    _cr build (great_circle_area with the device's arc cosine)"""
    a, b, fam = gc_cases.crafted_batch()
    n_ref = np.zeros(len(a), dtype=np.int32)
    v_ref = np.zeros((len(a), 16, 3))
    area_cr = np.zeros(len(a))
    for q in range(len(a)):
        n, v = orc.orc_clip_gc(a[q], b[q])
        assert 0 <= n <= 16
        n_ref[q] = n
        v_ref[q, :n] = v
        if n > 0:
            area_cr[q] = orc.orc_great_circle_area(*v.T, cr=True)
    return a, b, fam, n_ref, v_ref, area_cr


@pytest.mark.parametrize("size", [1, 63, 64, 65, 257, "all"])
def test_clip_batch_on_the_crafted_batch(fg, gpu_ok, crafted, size):
    """fg_gc_clip_batch on cell pairs made for the arc cosine's hard arguments (shifted and turned copies from 1e-9 rad, a vertex
    at a pole, quads 1e-4 as tall as wide, sliver triangles, cells whose area glibc's acosl rounds the other way:
    gc_cases.crafted_batch, shown to reach them in tests/test_gc_oracle_cr_cpu.py), at batch sizes with a partial last wave (one
    block is one wave of 64) and the whole batch: n_out and vertices in bits against the plain oracle, ALL areas in bits
    against great_circle_area with the device's arc cosine.  The short batches are taken across the families."""
    a, b, fam, n_ref, v_ref, area_cr = crafted
    sel = np.arange(len(a)) if size == "all" else np.arange(size) * (len(a) // size)
    n_out, verts, area = fg.gc_clip_batch(a[sel], b[sel])
    assert np.array_equal(n_out, n_ref[sel]), np.flatnonzero(n_out != n_ref[sel])[:10]
    nd = _nbits(verts, v_ref[sel])                      # (both zero past n_out)
    assert nd == 0, f"{nd} vertex coordinates differ from the oracle"
    bad = np.flatnonzero(_bits(area) != _bits(area_cr[sel]))
    assert len(bad) == 0, f"{len(bad)} of {len(sel)} areas differ from the _cr oracle, first: pair {sel[bad[0]]} ({fam[sel[bad[0]]]})"
    if size == "all":
        assert np.count_nonzero(n_out) > 2000
