"""Inputs shared by the great-circle tests (tests/test_gc_oracle_cr_cpu.py on the CPU, tests/test_gpu_great_circle.py on the
device): the grid pairs, a crafted batch of cell pairs for the arc cosine's hard arguments, and the accounting for one polygon
whose two areas differ.  Numpy, the package's host-side grid generators and the CPU oracle; nothing here touches the device."""
import numpy as np

R2 = 6371000.0 ** 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rotated(lon, lat, ax, ang):
    """corner arrays rotated about the unit axis `ax` by `ang` (a curvilinear grid whose edges cross everything at odd angles)"""
    x, y, z = np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)
    v = np.stack([x, y, z], -1)
    ax = np.asarray(ax, float) / np.linalg.norm(ax)
    c, s = np.cos(ang), np.sin(ang)
    r = v * c + np.cross(ax, v) * s + ax * (v @ ax)[..., None] * (1 - c)
    lo = np.arctan2(r[..., 1], r[..., 0])
    lo[lo < 0] += 2 * np.pi
    return np.ascontiguousarray(lo), np.ascontiguousarray(np.arcsin(np.clip(r[..., 2], -1, 1)))


def grid_cases(fg):
    """name -> (nx1, ny1, nx2, ny2, lon1, lat1, lon2, lat2): the six pairs of test_create_xgrid_great_circle_vs_oracle"""
    c24 = fg.gnomonic_ed_corners(24)
    c12 = fg.gnomonic_ed_corners(12)
    return {
        "c24_tile1_144x90": (24, 24, 144, 90, c24[0][0], c24[1][0]) + fg.latlon_corners(144, 90),
        "c24_tile3_polar_144x90": (24, 24, 144, 90, c24[0][2], c24[1][2]) + fg.latlon_corners(144, 90),
        "latlon_aligned_2x": (36, 18, 72, 36) + fg.latlon_corners(36, 18) + fg.latlon_corners(72, 36),
        "latlon_regional_offset": (30, 20, 45, 33) + fg.latlon_corners(30, 20, 10., 70., -30., 30.) + fg.latlon_corners(45, 33, 0., 90., -40., 40.),
        "latlon_to_cubed_polar": (40, 20, 12, 12) + fg.latlon_corners(40, 20) + (c12[0][5], c12[1][5]),
        "tripolar_to_cubed": (45, 27, 12, 12) + fg.tripolar_corners(45, 27) + (c12[0][2], c12[1][2]),
    }


def awkward_pairs(fg):
    """The grid pairs of test_three_pass_clip_on_awkward_grid_pairs, in its order: edges and corners that almost coincide (shifts
    of 1e-9 .. 1e-5 rad), crossings at odd angles (rotated grids), coarse against fine, a tripolar fold, regional windows."""
    lo72, la72 = fg.latlon_corners(72, 36)
    reg = fg.latlon_corners(40, 30, 20.0, 100.0, -35.0, 40.0)
    c16 = fg.gnomonic_ed_corners(16)
    tri = fg.tripolar_corners(60, 40)
    cases = []
    for sh in (1e-9, 3e-8, 1e-6, 1e-5):
        cases.append((72, 36, 72, 36, lo72, la72, np.ascontiguousarray(lo72 + sh), la72))
    cases.append((40, 30, 40, 30) + reg + rotated(*reg, (0.3, -0.5, 0.8), 0.37))
    cases.append((72, 36, 40, 30, lo72, la72) + rotated(*reg, (1.0, 0.2, 0.1), 1.1))
    cases.append((16, 16, 40, 30, c16[0][1], c16[1][1]) + reg)
    cases.append((16, 16, 16, 16, c16[0][0], c16[1][0]) + rotated(c16[0][0], c16[1][0], (0.1, 0.9, 0.4), 0.05))
    cases.append((60, 40, 72, 36) + tri + (lo72, la72))
    return cases


AWKWARD_NAMES = ["shift_1e-9", "shift_3e-8", "shift_1e-6", "shift_1e-5", "regional_rotated", "latlon_to_rotated_regional",
                 "cubed_to_regional", "cubed_rotated", "tripolar_to_latlon"]


def degenerate_cases(fg):
    """name -> (args of create_xgrid_great_circle, mask or None): identical grids, disjoint windows, single cells, masked sources"""
    lo, la = fg.latlon_corners(24, 12)
    lon, lat = fg.gnomonic_ed_corners(8)
    lo1, la1 = fg.latlon_corners(6, 6, 10.0, 40.0, 10.0, 40.0)
    lo2, la2 = fg.latlon_corners(5, 5, 100.0, 140.0, -40.0, -10.0)
    lo3, la3 = fg.latlon_corners(1, 1, 10.0, 20.0, 10.0, 20.0)
    lo4, la4 = fg.latlon_corners(1, 1, 15.0, 30.0, 5.0, 15.0)
    lon12, lat12 = fg.gnomonic_ed_corners(12)
    lo36, la36 = fg.latlon_corners(36, 18)
    mask = np.ones(144)
    mask[5] = 0.0
    mask[40:60] = 0.0
    return {
        "identical_latlon": ((24, 12, 24, 12, lo, la, lo, la), None),
        "identical_cubed": ((8, 8, 8, 8, lon[3], lat[3], lon[3], lat[3]), None),
        "disjoint": ((6, 6, 5, 5, lo1, la1, lo2, la2), None),
        "single_cells": ((1, 1, 1, 1, lo3, la3, lo4, la4), None),
        "fully_masked": ((6, 6, 6, 6, lo1, la1, lo1, la1), np.zeros(36)),
        "masked_cubed_to_latlon": ((12, 12, 36, 18, lon12[0], lat12[0], lo36, la36), mask),
    }


# ------------------------------------------------------------------------------ the crafted batch
def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frame(rng):
    """a random point of the sphere with its tangent frame: (centre, east, north), right-handed seen from outside"""
    c = _unit(rng.standard_normal(3))
    e = _unit(np.cross([0.0, 0.0, 1.0], c) if abs(c[2]) < 0.9 else np.cross([0.0, 1.0, 0.0], c))
    return c, e, np.cross(c, e)


def _gnomonic(fr, xy):
    """points of the tangent plane at fr onto the sphere; straight lines of the plane become great circles"""
    c, e, n = fr
    xy = np.asarray(xy, float)
    return _unit(c + xy[:, :1] * e + xy[:, 1:] * n)


def _rect(w, h, x0=0.0, y0=0.0, th=0.0):
    """corners of a w x h rectangle in the reference's cell order (j,i) (j+1,i) (j+1,i+1) (j,i+1), clockwise seen from outside,
    turned by th about its centre (x0, y0)"""
    p = np.array([[-w / 2, -h / 2], [-w / 2, h / 2], [w / 2, h / 2], [w / 2, -h / 2]])
    c, s = np.cos(th), np.sin(th)
    return p @ np.array([[c, s], [-s, c]]) + [x0, y0]


def _rot(v, ax, ang):
    ax = _unit(ax)
    c, s = np.cos(ang), np.sin(ang)
    return _unit(v * c + np.cross(ax, v) * s + ax * (v @ ax)[:, None] * (1 - c))


_CRAFTED = None


def crafted_batch():
    """(a, b, family): a, b [n, 4, 3] unit vectors, a few thousand cell pairs whose clipped polygons have interior angles next to
    0 and next to pi (arguments of the arc cosine next to +1 and -1) besides ordinary ones.  Deterministic; built once."""
    global _CRAFTED
    if _CRAFTED is not None:
        return _CRAFTED
    rng = np.random.default_rng(20240611)
    A, B, fam = [], [], []

    def add(a, b, name):
        A.append(a); B.append(b); fam.append(name)

    # 0. the cells of a fine curvilinear grid whose area the two arc cosines round differently (about one in ten thousand; the
    #    families below, a few thousand polygons, may hold none): each inside a larger quad, so that the clip hands the cell
    #    back in its own order, and against itself.  First in the batch, so that every leading or strided part of it holds one
    import orc
    nx = ny = 256
    lo, la = np.meshgrid(np.linspace(0.3, 1.5, nx + 1), np.linspace(-0.6, 0.6, ny + 1))
    lo, la = rotated(lo, la, (0.2, 0.7, -0.4), 0.9)
    ar = orc.orc_get_grid_gc_area(nx, ny, lo, la), orc.orc_get_grid_gc_area(nx, ny, lo, la, cr=True)
    x, y, z = (np.empty(lo.size) for _ in range(3))
    orc.oracle().orc_latlon2xyz(lo.size, orc._dp(orc.f64(lo).ravel()), orc._dp(orc.f64(la).ravel()), orc._dp(x), orc._dp(y), orc._dp(z))
    v = np.stack([x, y, z], -1).reshape(ny + 1, nx + 1, 3)
    for c in np.flatnonzero(bits(ar[0]) != bits(ar[1])):
        j, i = divmod(int(c), nx)
        a = np.array([v[j, i], v[j + 1, i], v[j + 1, i + 1], v[j, i + 1]])
        add(a, _unit(a.mean(0) + 1.5 * (a - a.mean(0))), "rounding")
        add(a, a.copy(), "rounding")
    per = 500
    # 1. shifted copies of a quad: 1e-9 .. 1e-2 rad along a random direction of the tangent plane
    for k in range(per):
        fr = _frame(rng)
        w, h = rng.uniform(0.02, 0.2, 2)
        a = _gnomonic(fr, _rect(w, h, th=rng.uniform(0, np.pi)))
        d = rng.uniform(0, 2 * np.pi)
        add(a, _rot(a, np.cos(d) * fr[1] + np.sin(d) * fr[2], 10.0 ** rng.uniform(-9, -2)), "shifted")
    # 2. copies turned by a small angle about a random axis, and about the quad's own centre (edges cross at that angle: vertices
    #    of the clipped polygon whose interior angle is pi minus it)
    for k in range(per):
        fr = _frame(rng)
        w, h = rng.uniform(0.02, 0.2, 2)
        a = _gnomonic(fr, _rect(w, h, th=rng.uniform(0, np.pi)))
        ax = fr[0] if k % 2 else rng.standard_normal(3)
        add(a, _rot(a, ax, 10.0 ** rng.uniform(-9, -2)), "turned")
    # 3. a vertex at a pole: lat-lon cells whose upper edge is the pole (two corners coincide), and generic quads with one
    #    corner exactly (0, 0, +-1); against a copy turned about an axis through the neighbourhood
    for k in range(per):
        sgn = 1.0 if k % 4 < 2 else -1.0
        if k % 2:
            l0, dl, la = rng.uniform(0, 2 * np.pi), rng.uniform(0.02, 0.3), rng.uniform(0.02, 0.2)
            lon = np.array([l0, l0, l0 + dl, l0 + dl])
            lat = np.array([np.pi / 2 - la, np.pi / 2, np.pi / 2, np.pi / 2 - la])
            a = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], -1)
            a[1] = a[2] = [0.0, 0.0, 1.0]
        else:
            w, h = rng.uniform(0.02, 0.2, 2)
            th = rng.uniform(0, np.pi)
            q = _rect(w, h, th=th)
            fr = (np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
            a = _gnomonic(fr, q - q[k // 2 % 4])
            a[k // 2 % 4] = [0.0, 0.0, 1.0]
        if sgn < 0:
            a = np.ascontiguousarray((a * [1.0, 1.0, -1.0])[::-1])     # mirrored to the south pole; the reversal keeps it clockwise
        ax = _unit(a.mean(0) + 0.3 * rng.standard_normal(3))
        add(a, _rot(a, ax, rng.uniform(0.01, 0.5) if k % 3 else 10.0 ** rng.uniform(-8, -3)), "pole")
    # 4. quads 1e-4 as tall as wide, against a copy shifted across, turned about its centre, or crossing it at a right angle
    for k in range(per):
        fr = _frame(rng)
        w = rng.uniform(0.05, 0.2)
        h = 1e-4 * w
        th = rng.uniform(0, np.pi)
        a = _gnomonic(fr, _rect(w, h, th=th))
        m = k % 3
        if m == 0:
            b = _gnomonic(fr, _rect(w, h, x0=rng.uniform(-0.3, 0.3) * w, y0=rng.uniform(-0.8, 0.8) * h, th=th))
        elif m == 1:
            b = _gnomonic(fr, _rect(w, h, th=th + 10.0 ** rng.uniform(-7, -1)))
        else:
            b = _gnomonic(fr, _rect(w, h, th=th + np.pi / 2 + rng.uniform(-0.2, 0.2)))
        add(a, b, "thin")
    # 5. sliver triangles: an edge of b leaves a through its lower edge at a shallow angle just before a's corner, so the clip is
    #    the triangle (crossing, corner, crossing) with interior angles th, pi/2 and pi/2 - th
    for k in range(per):
        fr = _frame(rng)
        w, h = rng.uniform(0.05, 0.2, 2)
        th = 10.0 ** rng.uniform(-7.5, -2)
        dist = rng.uniform(0.2, 0.8) * w                  # from the crossing on the lower edge to the corner
        L, M, back = 2 * w, 0.5 * h, 0.3 * w
        c, s = np.cos(th), np.sin(th)
        p1 = np.array([w / 2 - dist, -h / 2])
        o = p1 - back * np.array([c, s])                  # b's upper-left corner, below a's lower edge
        along, down = np.array([c, s]), np.array([s, -c])
        bq = np.array([o + M * down, o, o + L * along, o + L * along + M * down])
        add(_gnomonic(fr, _rect(w, h)), _gnomonic(fr, bq), "sliver")
    # 6. ordinary overlaps: a quad against a turned, shifted copy of another size
    for k in range(per):
        fr = _frame(rng)
        w, h = rng.uniform(0.02, 0.2, 2)
        a = _gnomonic(fr, _rect(w, h, th=rng.uniform(0, np.pi)))
        b = _gnomonic(fr, _rect(*rng.uniform(0.02, 0.2, 2), x0=rng.uniform(-0.5, 0.5) * w, y0=rng.uniform(-0.5, 0.5) * h,
                                th=rng.uniform(0, np.pi)))
        add(a, b, "ordinary")
    _CRAFTED = (np.ascontiguousarray(np.stack(A)), np.ascontiguousarray(np.stack(B)), np.array(fam))
    return _CRAFTED


# ------------------------------------------------------------------------------ accounting for one polygon
def polygon_angles(p, cr):
    """the n angles great_circle_area adds up (mosaic_util.c:763-787), in its order, from the oracle's spherical_angle"""
    import orc
    n = len(p)
    return np.array([orc.orc_spherical_angle(p[(i + 1) % n], p[(i + 2) % n], p[i], cr=cr) for i in range(n)])


def dedup(p):
    """addEnd (mosaic_util.c:1096-1135): a point within 1e-10 of an earlier one is not added"""
    out = []
    for v in p:
        if not any(np.all(np.abs(v - u) <= 1e-10) for u in out):
            out.append(v)
    return np.array(out)


def account(p, area_plain, area_cr, scale=1.0):
    """The one legitimate reason for two areas of the polygon p [n, 3] to differ: the arc cosine rounded an angle the other
    way.  Returns None if that explains (area_plain, area_cr), else what does not hold.
    (a) at least one angle differs; (b) each by exactly one double ulp; (c) |d area| <= n (ulp(pi) + ulp(S)) R^2 with S the
    largest partial sum: a changed addend moves the sum by at most ulp(pi), and each of the n additions may round one ulp(S)
    differently.  scale is the mask value the exchange cell's area was multiplied by (at most 1)."""
    n = len(p)
    ap, ac = polygon_angles(p, False), polygon_angles(p, True)
    d = bits(ap).astype(np.int64) - bits(ac).astype(np.int64)
    if not d.any():
        return f"areas {area_plain!r} / {area_cr!r} differ but none of the {n} angles does"
    if np.abs(d).max() != 1:
        return f"an angle differs by {np.abs(d).max()} ulp: {ap.tolist()} / {ac.tolist()}"
    S = max(np.cumsum(ap).max(), np.cumsum(ac).max())
    bound = n * (np.spacing(np.pi) + np.spacing(S)) * R2 * scale
    if not abs(area_plain - area_cr) <= bound:
        return f"|d area| {abs(area_plain - area_cr)!r} m^2 above the bound {bound!r}"
    return None
