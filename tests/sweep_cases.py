"""Hand-made exchange lists for the sweep kernels (csrc/apply_kernels.hip) and their two yardsticks.  No GPU, no torch.

Every test of the sweep so far takes its exchange cells from a real grid pair.  Real pairs have nearly uniform row lengths, list
their cells in source order inside a destination row, and have no row whose counted cells all have area 0.  The lists made here
have none of the three; XgridPlan.create_empty + set_xgrid take them as they are (only the index ranges are checked) and
orc.cref_apply runs the reference's own do_scalar_conserve_interp on them.

A case is named  <profile>-<rows>[-1t]  and is a deterministic function of that name (seeded default_rng):
  source grid   three tiles of 23x17, 40x25 and 8x31 cells (cell_off and the halo index of order 2 matter); -1t: one tile of
                37x29 (the reference's monotone branch indexes every tile with the LAST tile's nx, conserve_interp.c:653,
                so the monotone cases need tiles of one size)
  rows          201 = 67 x 3, 99 = 11 x 9, 5 = 5 x 1, 1 = 1 x 1, and 804 = 67 x 12 for the two profiles whose contents do not
                fit a mean of <= 6 cells per row on 201 rows (spike: 3004 cells in seven rows alone)
  profile       the vector of row lengths, see PROFILES; each names the bin of nx // ndst it must land in -- the kernels are
                chosen by that mean (by_row_length, fgd_csr_sortgather, the `nx <= 6 * ndst` of k_apply_ep8)
The cells are listed in shuffled order: runs of 1..5 cells of one row, the runs of all rows interleaved, the sources inside a
row in random order, some (source, destination) pairs twice.

Chunks are counted from a tile's first record (c0 = T.q0 in the kernels), not from CSR position 0, so the chunk crossings are
computed per (rows per tile, chunk size) pair a kernel uses in the case's bin: see crossings().

Areas are uniform in [1e-6, 1e-3] with exact zeros: single cells, whole rows over sources that are never missing (Z: 0.0
expected), whole rows over sources that are always missing (ZM: `missing` with has_missing, else 0.0), and rows whose
zero-area cells are always valid while their positive ones are missing at levels k % 3 == 1 (FL).  MR rows have positive areas
over always-missing sources.  Level K_FULL misses nothing, level K_NONE everything.

reference() is the reference library, plain() a float64 loop that adds in list order -- the second yardstick and the one that
exists where the library is not built.  check_preconditions() asserts every property above on the list and on the yardstick's
output: a case that misses one is an error, not a skip."""
import functools
import zlib

import numpy as np

import orc

MISSING = -1.0e10
NLEV = 17
K_FULL, K_NONE = 3, 5
SRC3 = ((23, 17), (40, 25), (8, 31))
SRC1 = ((37, 29),)
SHAPES = {201: (67, 3), 99: (11, 9), 5: (5, 1), 1: (1, 1), 804: (67, 12)}
BINS = {"<=6": (0, 6), "7..24": (7, 24), "25..96": (25, 96), ">96": (97, 1 << 30)}
EIGHTS = (7, 8, 9, 15, 16, 17, 23, 24, 25)
SPIKES = (255, 256, 257, 511, 512, 513, 700)
# (rows per tile, records per chunk) of the chunked kernels per bin: k_apply_ep1 / k_apply_epx <R, CAP 512> with R = 64, 16, 4, 1
# (fgd_apply1, fgd_apply_ex); k_apply_ep8g MASKED <CAP 256> with R = 32, 8, 2, 1 (fgd_apply_levels8); k_apply_ep8g unmasked
# <CAP 256> with R = 8, 2, 1 above the first bin (fgd_apply_il, fgd_apply_il_merged); k_apply_ep8 <32 rows, 256 records> in the first
TILINGS = {"<=6": ((64, 512), (32, 256)), "7..24": ((16, 512), (8, 256)), "25..96": ((4, 512), (2, 256)), ">96": ((1, 512), (1, 256))}
# profile -> (bin on the shapes with at least 99 rows, shapes)
PROFILES = {
    "short": ("<=6", (201, 99, 5, 1)),     # lengths 0..13, empty rows first, last and as a run of 64; rows of 12 and 13 (SHORT of the sort)
    "spike": ("<=6", (804,)),              # one row each of SPIKES among short and empty rows
    "eights": ("<=6", (804,)),             # rows of EIGHTS; every length crosses a chunk boundary of both tilings of the bin
    "mid": ("7..24", (201, 5)),            # 0..30 mixed
    "long": ("25..96", (201, 99, 1)),      # 20..100 mixed, a row of 300, some empty
    "huge": (">96", (201, 99, 5)),         # a row of 2503 (beyond the sort's staging of 2048), one of exactly 2048, the rest 50..300
}
CASES = tuple(f"{p}-{n}" for p, (_, shapes) in PROFILES.items() for n in shapes) + ("eights-201", "spike-804-1t", "eights-804-1t", "long-201-1t")
N_DUP = 40
EX_OPTS = ("weight0", "sum", "meas", "meas_target", "mono", "mono_missing")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def parse(name):
    p = name.split("-")
    return p[0], int(p[1]), len(p) > 2 and p[2] == "1t"


def bin_of(name):
    profile, ndst, _ = parse(name)
    if name == "eights-201":
        return "7..24"
    if profile == "huge" or ndst >= 99:
        return PROFILES[profile][0]
    return {"short": "<=6", "mid": "7..24", "long": "25..96"}[profile]


# -------------------------------------------------------------------------------------------------------------- row lengths
def _place(rng, lens, values, free):
    rows = rng.choice(free, size=len(values), replace=False)
    lens[rows] = values
    return {int(v): int(r) for v, r in zip(values, rows)}


def _eights_tile(rng, want512, want256):
    """64 rows: 34 of EIGHTS and 30 empty, the first 32 rows holding more than 256 cells, such that the row that crosses record
    512 of the 64-row tile has length want512, the row that crosses record 256 of its first 32-row tile has length want256,
    and both start inside a block of eight of their row (the crossing splits the row in two parts that are no multiple of 8)."""
    for _ in range(200000):
        a = np.concatenate([rng.choice(EIGHTS, 18), np.zeros(14, dtype=np.int64)])
        b = np.concatenate([rng.choice(EIGHTS, 16), np.zeros(16, dtype=np.int64)])
        rng.shuffle(a); rng.shuffle(b)
        ln = np.concatenate([a, b])
        end = np.cumsum(ln)
        beg = end - ln
        r5 = np.nonzero((beg < 512) & (end > 512))[0]
        r2 = np.nonzero((beg[:32] < 256) & (end[:32] > 256))[0]
        if r5.size == 1 and r2.size == 1 and ln[r5[0]] == want512 and ln[r2[0]] == want256 and \
                (512 - beg[r5[0]]) % 8 and (end[r5[0]] - 512) % 8 and (256 - beg[r2[0]]) % 8 and (end[r2[0]] - 256) % 8:
            return ln
    raise AssertionError("no arrangement found")


def _lengths(rng, profile, ndst, name):
    """-> (lens [ndst], pins: rows whose length is part of the profile and must stay ordinary rows)"""
    lens = np.zeros(ndst, dtype=np.int64)
    pins = {}
    if profile == "short":
        if ndst == 1:
            lens[:] = 5
        elif ndst == 5:
            lens[:] = (0, 12, 3, 13, 0)
        else:
            lens = rng.integers(0, 10, ndst)
            run = (64, 128) if ndst == 201 else (32, 64)
            lens[0] = lens[-1] = 0
            lens[run[0]:run[1]] = 0
            free = np.array([d for d in range(1, ndst - 1) if not run[0] <= d < run[1]])
            rows = rng.choice(free, size=4, replace=False)
            lens[rows] = (12, 13, 12, 13)
            pins = {f"len{v}_{k}": int(r) for k, (v, r) in enumerate(zip((12, 13, 12, 13), rows))}
    elif profile == "spike":
        # 257 and 700 share a 64-row tile, so that the row of 700 starts inside a chunk of 512 and ends two chunks later
        lens = rng.choice(np.array([0, 0, 1, 2, 3, 4, 5]), ndst)
        t0 = 64 * int(rng.integers(1, ndst // 64))
        lens[[t0 + 2, t0 + 45]] = (257, 700)
        free = np.array([d for d in range(1, ndst - 1) if not t0 <= d < t0 + 64])
        pins = {f"len{v}": r for v, r in _place(rng, lens, [v for v in SPIKES if v not in (257, 700)], free).items()}
        pins.update(len257=t0 + 2, len700=t0 + 45)
    elif profile == "eights" and ndst == 201:
        lens = np.resize(np.array(EIGHTS), ndst)
    elif profile == "eights":
        lens = rng.choice(np.array([0, 0, 1, 2, 3, 4]), ndst)
        for k in range(9):                                   # nine 64-row tiles, each with its own pair of crossing lengths
            lens[64 * k:64 * (k + 1)] = _eights_tile(rng, EIGHTS[k], EIGHTS[(k + 4) % 9])
    elif profile == "mid":
        if ndst == 5:
            lens[:] = (9, 0, 24, 17, 11)
        else:
            lens = rng.integers(0, 31, ndst)
            lens[0] = 0
    elif profile == "long":
        if ndst == 1:
            lens[:] = 60
        else:
            lens = rng.integers(20, 101, ndst)
            lens[rng.choice(ndst, size=3, replace=False)] = 0
            pins = {f"len{v}": r for v, r in _place(rng, lens, (300,), np.arange(ndst)).items()}
    elif profile == "huge":
        if ndst == 5:
            lens[:] = (2503, 2048, 300, 50, 120)
            pins = {"len2503": 0, "len2048": 1}
        else:
            lens = rng.integers(50, 161, ndst)
            pins = {f"len{v}": r for v, r in _place(rng, lens, (2503, 2048, 300, 300), np.arange(ndst)).items()}
    else:
        raise KeyError(name)
    return lens.astype(np.int64), pins


def crossings(row_ptr, rows_per_tile, cap):
    """per row: (chunk boundaries strictly inside the row, whether it starts off a boundary), chunks counted from the first
    record of the row's tile as the kernels do"""
    ndst = len(row_ptr) - 1
    d = np.arange(ndst)
    q0 = row_ptr[(d // rows_per_tile) * rows_per_tile]
    b, e = row_ptr[:-1] - q0, row_ptr[1:] - q0
    inside = np.where(e > b, (e - 1) // cap - b // cap, 0)
    return inside, (b % cap) != 0


def _structure_ok(profile, ndst, lens, pins, bin_name):
    """the conditions on the row offsets that a placement can miss (the generator retries with the next sub-seed)"""
    row_ptr = np.concatenate([[0], np.cumsum(lens)])
    lo, hi = BINS[bin_name]
    if not lo <= int(row_ptr[-1]) // ndst <= hi:
        return False
    if profile == "spike":
        for rpt, cap in TILINGS[bin_name]:
            inside, off = crossings(row_ptr, rpt, cap)
            if not any(inside[r] >= 2 and off[r] for r in pins.values()):
                return False
    return True


# ------------------------------------------------------------------------------------------------------------------ the case
@functools.lru_cache(maxsize=None)
def make(name):
    """The case of that name.  A draw whose row offsets miss the profile (_structure_ok), or whose sums do not depend on the order
    of addition in enough rows (order_sensitive), is drawn again with the next sub-seed: still a function of the name alone."""
    seed = zlib.crc32(name.encode())
    for attempt in range(64):
        c = _draw(name, np.random.default_rng([seed, attempt]))
        if c is not None and all(2 * a >= b for a, b in order_sensitive(c).values()):
            return c
    raise AssertionError(f"{name}: no draw meets the profile")


def _draw(name, rng):
    profile, ndst, one_tile = parse(name)
    tiles = SRC1 if one_tile else SRC3
    nxo, nyo = SHAPES[ndst]
    bin_name = bin_of(name)
    lens, pins = _lengths(rng, profile, ndst, name)
    if not _structure_ok(profile, ndst, lens, pins, bin_name):
        return None
    cell_off = np.concatenate([[0], np.cumsum([nx * ny for nx, ny in tiles])]).astype(np.int64)
    halo_off = np.concatenate([[0], np.cumsum([(nx + 2) * (ny + 2) for nx, ny in tiles])]).astype(np.int64)
    nsrc, nhalo = int(cell_off[-1]), int(halo_off[-1])
    # three disjoint sets of source cells: D always missing, A never, F missing at levels k % 3 == 1
    perm = rng.permutation(nsrc)
    ns = max(nsrc // 16, 8)
    D, A, F = perm[:ns], perm[ns:2 * ns], perm[2 * ns:3 * ns]
    special = {}
    if ndst >= 99:
        cand = np.array([d for d in range(ndst) if lens[d] >= 4 and d not in pins.values()])
        if cand.size < 12:
            return None
        pick = rng.choice(cand, size=12, replace=False)
        special = {int(d): kind for d, kind in zip(pick, ("Z", "ZM", "MR", "FL") * 3)}
    nx = int(lens.sum())
    assert 0 < nx < 40000, (name, nx)
    dst = np.repeat(np.arange(ndst), lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)])
    src = np.empty(nx, dtype=np.int64)
    area = rng.uniform(1e-6, 1e-3, nx)
    area[rng.random(nx) < 0.03] = 0.0
    for d in range(ndst):
        b, e, n = int(row_ptr[d]), int(row_ptr[d + 1]), int(lens[d])
        if n == 0:
            continue
        kind = special.get(d)
        if kind == "Z":
            src[b:e] = rng.choice(A, n); area[b:e] = 0.0
        elif kind == "ZM":
            src[b:e] = rng.choice(D, n); area[b:e] = 0.0
        elif kind == "MR":
            src[b:e] = rng.choice(D, n)
        elif kind == "FL":
            h = n // 2
            src[b:b + h] = rng.choice(A, h); area[b:b + h] = 0.0
            src[b + h:e] = rng.choice(F, n - h); area[b + h:e] = rng.uniform(1e-6, 1e-3, n - h)
        else:
            src[b:e] = rng.choice(nsrc, n, replace=n > nsrc)
    # the same (source, destination) pair twice
    ordinary = rng.permutation(np.array([d for d in range(ndst) if lens[d] >= 2 and d not in special]))
    forced = []                                                      # the second of a pair starts a run of its own
    for d in ordinary[:N_DUP]:
        a, b = sorted(rng.choice(int(lens[d]), size=2, replace=False))
        src[row_ptr[d] + b] = src[row_ptr[d] + a]
        forced.append(int(row_ptr[d] + b))
    # list order: runs of 1..5 cells of a row, the runs of all rows shuffled
    cut = np.ones(nx, dtype=bool)
    run_left = 0
    steps = rng.integers(1, 6, nx)
    row_start = np.zeros(nx + 1, dtype=bool)
    row_start[row_ptr] = True
    row_start[forced] = True
    for n in range(nx):
        if row_start[n] or run_left == 0:
            run_left = int(steps[n])
        else:
            cut[n] = False
        run_left -= 1
    seg = np.cumsum(cut) - 1
    key = rng.permutation(int(seg[-1]) + 1)
    order = np.lexsort((np.arange(nx), key[seg]))
    src, dst, area = src[order], dst[order], area[order]
    t_in = np.searchsorted(cell_off, src, side="right") - 1
    loc = src - cell_off[t_in]
    tnx = np.array([t[0] for t in tiles])[t_in]
    i_in, j_in = loc % tnx, loc // tnx
    x = dict(t_in=t_in.astype(np.int32), i_in=i_in.astype(np.int32), j_in=j_in.astype(np.int32),
             i_out=(dst % nxo).astype(np.int32), j_out=(dst // nxo).astype(np.int32), area=area,
             di=rng.uniform(-0.02, 0.02, nx), dj=rng.uniform(-0.02, 0.02, nx))
    c = dict(name=name, profile=profile, ndst=ndst, nxo=nxo, nyo=nyo, tiles=tiles, nsrc=nsrc, nhalo=nhalo, bin=bin_name, lens=lens,
             row_ptr=row_ptr, pins=pins, special=special, x=x, src=src, dst=dst, nx=nx, cell_off=cell_off, halo_off=halo_off,
             tnx=[t[0] for t in tiles], tny=[t[1] for t in tiles], one_tile=one_tile,
             fidx=halo_off[t_in] + (j_in + 1) * (tnx + 2) + i_in + 1, sets=dict(D=D, A=A, F=F))
    # ---- fields: float64 of both signs, a quarter of the values anywhere in 1e-8 .. 1e8, the others within two decades -- were
    # all of them spread over sixteen decades, most short rows would round to their largest term whatever the order of addition
    wild = lambda shape: rng.choice([-1.0, 1.0], shape) * 10.0 ** np.where(rng.random(shape) < 0.25, rng.uniform(-8.0, 8.0, shape),
                                                                            rng.uniform(0.0, 2.0, shape))
    c["vals"] = wild((NLEV, nsrc))
    c["gx"], c["gy"] = wild((NLEV, nsrc)), wild((NLEV, nsrc))
    gm = rng.choice(np.array([0, 0, 0, 0, 0, 0, 0, 1, 1, 2], dtype=np.int32), (NLEV, nsrc))   # the code tests `!= 0`
    c["gm"] = np.ascontiguousarray(gm)
    miss = rng.random((NLEV, nsrc)) < 0.3
    miss[:, D] = True
    miss[:, A] = False
    miss[:, F] = (np.arange(NLEV) % 3 == 1)[:, None]
    miss[K_FULL] = False
    miss[K_NONE] = True
    c["miss"] = miss
    c["frame"] = wild((NLEV, nhalo))                                 # the halo holds values of its own: a wrong halo index shows
    inner = np.concatenate([halo_off[t] + ((np.arange(ny)[:, None] + 1) * (nx_ + 2) + np.arange(nx_)[None, :] + 1).ravel()
                            for t, (nx_, ny) in enumerate(tiles)])
    c["inner"] = inner
    # ---- the options of do_scalar_conserve_interp
    w = rng.uniform(0.25, 4.0, nsrc)
    w[rng.random(nsrc) < 0.15] = 0.0
    w[F] = 0.0                                                       # FL rows: zero areas on A, zero weights on F -> 0.0 by `touched`
    c["weight"] = w
    c["cell_area_in"] = rng.uniform(0.5e-3, 2e-3, nsrc)
    c["field_area"] = rng.uniform(0.5e-3, 2e-3, nsrc)
    c["cell_area_out"] = rng.uniform(0.5e-2, 2e-2, ndst)
    # ---- the monotone limiter: values of one decade.  Its result may exceed the neighbourhood's bound by rounding, the reference
    # then ends the process unless the excess is below 1e-10 -- far above an ulp of these values, far below one of 1e8
    tame = lambda shape: rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 10.0, shape)
    c["tame"] = dict(frame=tame(nhalo), vals=tame(nsrc), gx=tame(nsrc), gy=tame(nsrc))
    return c


def field(c, order, masked, levels=None, tame=False):
    """the field as the device entry points and the reference take it: [levels][cells], order 2 with its halo"""
    if tame:
        v, fr, miss = c["tame"]["vals"][None], c["tame"]["frame"][None], c["miss"][:1]
    else:
        v, fr, miss = c["vals"], c["frame"], c["miss"]
    v = np.where(miss, MISSING, v) if masked else v
    if order == 2:
        f = fr.copy()
        f[:, c["inner"]] = v
        v = f
    v = np.ascontiguousarray(v)
    return v if levels is None else np.ascontiguousarray(v[levels])


def _per_tile(c, a, halo):
    """[levels][all tiles] -> per tile [levels * tile size]"""
    off = c["halo_off"] if halo else c["cell_off"]
    return [np.ascontiguousarray(a[..., off[t]:off[t + 1]]).ravel() for t in range(len(c["tiles"]))]


# ---------------------------------------------------------------------------------------------------------------- yardsticks
def reference(c, order, masked):
    """[NLEV][ndst] from the reference library: one call of nz = NLEV without missing values (conserve_interp.c:592-615, :784-812),
    one call per level with them (:544)"""
    f = field(c, order, masked)
    grads = lambda k: ([_per_tile(c, c[g][k], False) for g in ("gx", "gy")] if order == 2 else [None, None])
    if not masked:
        gx, gy = grads(slice(None))
        r, _ = orc.cref_apply(order, c["x"], c["tnx"], c["tny"], _per_tile(c, f, order == 2), gx, gy, None, False, 0.0,
                              c["nxo"], c["nyo"], NLEV)
        return r.reshape(NLEV, c["ndst"])
    out = np.empty((NLEV, c["ndst"]))
    for k in range(NLEV):
        gx, gy = grads(k)
        gm = _per_tile(c, c["gm"][k], False) if order == 2 else None
        out[k], _ = orc.cref_apply(order, c["x"], c["tnx"], c["tny"], _per_tile(c, f[k], order == 2), gx, gy, gm, True, MISSING,
                                   c["nxo"], c["nyo"], 1)
    return out


def ex_inputs(c, order, opt):
    """level 0 with one option set of apply_ex"""
    assert opt in EX_OPTS and (not opt.startswith("mono") or (order == 2 and c["one_tile"]))
    mono = opt.startswith("mono")
    masked = opt != "mono"
    k = 0
    kw = dict(order=order, has_missing=masked, missing=MISSING if masked else -1.0e20, monotonic=mono, data=field(c, order, masked, k, tame=mono),
              weight=c["weight"] if opt == "weight0" else None, sum=opt == "sum", field_area=c["field_area"] if opt.startswith("meas") else None,
              cell_area_in=c["cell_area_in"] if opt in ("sum", "meas", "meas_target") else None,
              cell_area_out=c["cell_area_out"] if opt == "meas_target" else None, gx=None, gy=None, gm=None)
    if mono:
        kw["data"] = field(c, 2, masked, 0, tame=True)
        kw["gx"], kw["gy"] = c["tame"]["gx"], c["tame"]["gy"]
        kw["gm"] = c["gm"][0] if masked else None
    elif order == 2:
        kw["gx"], kw["gy"], kw["gm"] = c["gx"][k], c["gy"][k], c["gm"][k]
    return kw


def reference_ex(c, order, opt):
    kw = ex_inputs(c, order, opt)
    # the limiter's fatal checks end the process in the reference: plain() raises on them first
    if kw["monotonic"]:
        plain_ex(c, order, opt)
    pt = lambda a, halo=False: _per_tile(c, a, halo) if a is not None else None
    r, _ = orc.cref_apply(order, c["x"], c["tnx"], c["tny"], pt(kw["data"], order == 2), pt(kw["gx"]), pt(kw["gy"]), pt(kw["gm"]),
                          kw["has_missing"], kw["missing"], c["nxo"], c["nyo"], 1, weight=pt(kw["weight"]), cell_methods_sum=kw["sum"],
                          field_area=pt(kw["field_area"]), cell_area_in=pt(kw["cell_area_in"]), target_grid=kw["cell_area_out"] is not None,
                          cell_area_out=kw["cell_area_out"], monotonic=kw["monotonic"])
    return r


def _mono_xdata(c, f, gx, gy, gm, missing):
    """conserve_interp.c:621-714 on one tile: the limited second-order value of every exchange cell"""
    (nx, ny), = c["tiles"]
    s, fi, x = c["src"], c["fidx"], c["x"]
    f2 = f.reshape(ny + 2, nx + 2)
    nb = np.stack([f2[1 + dj:1 + dj + ny, 1 + di:1 + di + nx].ravel() for dj in (-1, 0, 1) for di in (-1, 0, 1)])
    fbmax = np.max(np.where(nb != missing, nb, -1.0e20), axis=0)
    fbmin = np.min(np.where(nb != missing, nb, 1.0e20), axis=0)
    fbar = f[fi]
    flat = np.zeros(c["nx"], dtype=bool) if gm is None else gm[s] != 0
    xd = np.where(flat, fbar, (fbar + gx[s] * x["di"]) + gy[s] * x["dj"])
    ok = fbar != missing
    fmax, fmin = np.full(c["nsrc"], -1.0e20), np.full(c["nsrc"], 1.0e20)
    np.maximum.at(fmax, s[ok], xd[ok])
    np.minimum.at(fmin, s[ok], xd[ok])
    up = ok & (fmax[s] > fbmax[s])
    dn = ok & ~up & (fmin[s] < fbmin[s])
    with np.errstate(all="ignore"):
        xu = fbar + ((xd - fbar) / (fmax[s] - fbar)) * (fbmax[s] - fbar)
        xl = fbar + ((xd - fbar) / (fmin[s] - fbar)) * (fbmin[s] - fbar)
    xu = np.where((xu > fbmax[s]) & (xu - fbmax[s] < 1e-10), fbmax[s], xu)
    xl = np.where((xl < fbmin[s]) & (fbmin[s] - xl < 1e-10), fbmin[s], xl)
    assert not np.any(up & (xu > fbmax[s])) and not np.any(dn & (xl < fbmin[s])), "the limiter's fatal check"
    assert np.any(up) and np.any(dn)
    xd = np.where(up, xu, np.where(dn, xl, xd))
    return np.where(ok, xd, missing)


def _sweep(c, order, f, gx, gy, gm, has_missing, missing, weight=None, sum_=False, field_area=None, cell_area_in=None,
           cell_area_out=None, xdata=None, reverse=False):
    """The reference's loop over the exchange cells in list order (reverse: in reversed list order) on levels f [nlev][cells], every
    sum in float64 and in that order, then the finish of conserve_interp.c:815-866.  Vectorised over the levels and over the rows:
    step r adds cell r of every row that has one."""
    x, s, fi, d = c["x"], c["src"], c["fidx"] if order == 2 else c["src"], c["dst"]
    nlev, ndst = f.shape[0], c["ndst"]
    a0 = x["area"]
    a = a0 * weight[s] if weight is not None else a0
    if xdata is not None:
        v = xdata[None]
        valid = v != missing
    else:
        v = f[:, fi]
        valid = (v != missing) if has_missing else np.ones(v.shape, dtype=bool)
    if sum_:
        a = a / cell_area_in[s]
    elif field_area is not None:
        a = a * (field_area[s] / cell_area_in[s])
    if order == 2 and xdata is None:
        full = (v + gx[:, s] * x["di"]) + gy[:, s] * x["dj"]
        v = np.where(gm[:, s] != 0, v, full) if (has_missing and gm is not None) else full
    p = v * a
    t = (a0 * field_area[s] / cell_area_in[s]) if field_area is not None else a0
    lst = np.arange(c["nx"])[::-1] if reverse else np.arange(c["nx"])
    csr = lst[np.argsort(d[lst], kind="stable")]
    lens, row_ptr = c["lens"], c["row_ptr"]
    acc, asum = np.zeros((nlev, ndst)), np.zeros((nlev, ndst))
    asum_t = np.zeros(ndst)
    touched = np.zeros((nlev, ndst), dtype=bool)
    by_len = np.argsort(-lens, kind="stable")
    nrows = np.searchsorted(-lens[by_len], -np.arange(int(lens.max(initial=0))), side="left")    # rows longer than r
    for r in range(int(lens.max(initial=0))):
        rows = by_len[:nrows[r]]
        n = csr[row_ptr[rows] + r]
        ok = valid[:, n]
        acc[:, rows] = np.where(ok, acc[:, rows] + p[:, n], acc[:, rows])
        asum[:, rows] = np.where(ok, asum[:, rows] + a[n], asum[:, rows])
        asum_t[rows] += t[n]
        if xdata is None:                                            # the monotone branch never sets out_miss
            touched[:, rows] |= ok
    with np.errstate(all="ignore"):
        if sum_:
            return np.where(asum == 0, np.where(touched, 0.0, missing), acc)
        out = np.where(asum > 0, acc / asum, np.where(touched, 0.0, missing))
        if cell_area_out is not None:
            out = np.where(out != missing, out * (asum_t / cell_area_out), out)
    return out


def plain(c, order, masked, reverse=False, levels=slice(None)):
    f = field(c, order, masked)[levels]
    return _sweep(c, order, f, c["gx"][levels], c["gy"][levels], c["gm"][levels], masked, MISSING if masked else -1.0e20, reverse=reverse)


def plain_ex(c, order, opt):
    kw = ex_inputs(c, order, opt)
    lv = lambda a: a[None] if a is not None else None
    xd = _mono_xdata(c, kw["data"], kw["gx"], kw["gy"], kw["gm"], kw["missing"]) if kw["monotonic"] else None
    return _sweep(c, order, kw["data"][None], lv(kw["gx"]), lv(kw["gy"]), lv(kw["gm"]), kw["has_missing"], kw["missing"], weight=kw["weight"],
                  sum_=kw["sum"], field_area=kw["field_area"], cell_area_in=kw["cell_area_in"], cell_area_out=kw["cell_area_out"], xdata=xd)[0]


def yardstick(c, order, masked):
    """(which, [NLEV][ndst]): the reference library where it is built, else the plain loop"""
    key = ("yard", order, masked)
    if key not in c:
        c[key] = ("reference", reference(c, order, masked)) if orc.conserve_ref_available() else ("plain", plain(c, order, masked))
    return c[key]


def yardstick_ex(c, order, opt):
    key = ("yard_ex", order, opt)
    if key not in c:
        c[key] = ("reference", reference_ex(c, order, opt)) if orc.conserve_ref_available() else ("plain", plain_ex(c, order, opt))
    return c[key]


# ------------------------------------------------------------------------------------------------------------ preconditions
def order_sensitive(c):
    """{check: (rows whose bits change when the cells are added in reversed list order, rows asked)} at level 0: rows of 4 or
    more cells without missing values, order 1 and 2; rows of 4 or more valid cells with them, order 2"""
    if "order_sensitive" not in c:
        lev = slice(0, 1)
        rows4 = c["lens"] >= 4
        valid4 = np.bincount(c["dst"], weights=(~c["miss"][0][c["src"]]).astype(np.float64), minlength=c["ndst"]) >= 4
        out = {}
        for key, order, masked, rows in (("order1", 1, False, rows4), ("order2", 2, False, rows4), ("order2-missing", 2, True, valid4)):
            changed = bits(plain(c, order, masked, levels=lev)[0]) != bits(plain(c, order, masked, reverse=True, levels=lev)[0])
            out[key] = (int(np.count_nonzero(changed & rows)), int(np.count_nonzero(rows)))
        c["order_sensitive"] = out
    return c["order_sensitive"]


def outcomes(c, masked):
    """per (level, row): 0 = a counted cell and a positive area sum, 1 = a counted cell but area sum 0, 2 = no counted cell"""
    valid = ~c["miss"][:, c["src"]] if masked else np.ones((NLEV, c["nx"]), dtype=bool)
    cnt = np.stack([np.bincount(c["dst"], weights=v.astype(np.float64), minlength=c["ndst"]) for v in valid])
    pos = np.stack([np.bincount(c["dst"], weights=(v & (c["x"]["area"] > 0)).astype(np.float64), minlength=c["ndst"]) for v in valid])
    return np.where(pos > 0, 0, np.where(cnt > 0, 1, 2))


def check_preconditions(c):
    name, profile, ndst, lens, row_ptr, pins = c["name"], c["profile"], c["ndst"], c["lens"], c["row_ptr"], c["pins"]
    src, dst, nx = c["src"], c["dst"], c["nx"]
    big = ndst >= 99
    # the list is what the profile says
    assert np.array_equal(np.bincount(dst, minlength=ndst), lens)
    lo, hi = BINS[c["bin"]]
    assert lo <= nx // ndst <= hi, (name, nx // ndst)
    assert nx < 40000
    tilings = TILINGS[c["bin"]]
    if profile == "short" and big:
        run = (64, 128) if ndst == 201 else (32, 64)
        assert lens[0] == 0 and lens[-1] == 0 and np.count_nonzero(lens[1:-1] == 0) > run[1] - run[0]
        assert np.all(lens[run[0]:run[1]] == 0)                      # a tile of 64 and two of 32 rows (201 rows), one of 32 (99) own no record
        assert sorted(lens[list(pins.values())]) == [12, 12, 13, 13] and lens.max() == 13
    if profile == "short" and ndst == 5:
        assert 12 in lens and 13 in lens and lens[0] == 0 and lens[-1] == 0
    if profile == "spike":
        assert sorted(lens[list(pins.values())]) == list(SPIKES) and np.sort(lens)[-8] <= 5
        for rpt, cap in tilings:
            inside, off = crossings(row_ptr, rpt, cap)
            assert any(inside[r] >= 2 and off[r] for r in pins.values()), (rpt, cap)
            q0 = row_ptr[np.arange(0, ndst, rpt)]
            assert np.any(np.diff(np.append(q0, nx)) > cap)          # k_apply_ep8's row-serial tile; the sort's unstaged block
    if profile == "eights":
        assert set(lens[lens > 6]) == set(EIGHTS) or ndst == 804
        if ndst == 804:
            for rpt, cap in tilings:
                inside, off = crossings(row_ptr, rpt, cap)
                cross = np.nonzero(inside > 0)[0]
                assert set(EIGHTS) <= set(lens[cross]), (rpt, cap, sorted(set(lens[cross])))
                # ... and the boundary splits every one of them off the blocks of eight of ep_row_add
                q0 = row_ptr[(cross // rpt) * rpt]
                head = cap - (row_ptr[cross] - q0) % cap
                split = {int(n) for n, h in zip(lens[cross], head) if int(h) % 8 != 0 and int(n - h) % 8 != 0}
                assert set(EIGHTS) <= split, (rpt, cap, sorted(split))
    if profile == "long" and big:
        assert lens.max() == 300 and np.count_nonzero(lens == 0) >= 3
    if profile == "huge":
        assert np.sort(lens)[-1] == 2503 and np.sort(lens)[-2] == 2048 and 2503 > 2048     # CAP of k_csr_sortgather<., 16, ., 256>
        assert np.all(np.sort(lens)[:-2] <= 300) and np.sort(lens)[0] >= 50
        if ndst == 5:
            assert nx > 256 * ndst                                   # the sort's one-row-per-block mode
    if profile in ("mid", "long", "huge"):
        assert 8 * ndst < nx <= 256 * ndst or ndst == 5              # the sort's 16-rows-per-block mode
    if c["bin"] == "<=6":
        assert nx <= 6 * ndst + ndst - 1 and nx <= 8 * ndst          # the sort's 64-rows-per-block mode
    # list order: rows interleaved, sources not ascending, pairs twice
    assert big is False or np.count_nonzero(np.diff(dst) != 0) > nx // 8
    csr = np.argsort(dst, kind="stable")
    rows3 = [d for d in range(ndst) if lens[d] >= 3]
    unsorted = sum(bool(np.any(np.diff(src[csr[row_ptr[d]:row_ptr[d + 1]]]) < 0)) for d in rows3)
    assert 2 * unsorted >= len(rows3), (unsorted, len(rows3))
    pair = dst.astype(np.int64) * c["nsrc"] + src
    first = {}
    apart = set()
    for n, p in enumerate(pair.tolist()):
        if p in first and n - first[p] > 1:
            apart.add(p)
        first.setdefault(p, n)
    # (twenty where the rows can hold them; a single short row holds five cells)
    assert len(apart) >= (20 if nx >= 100 else 0), len(apart)
    # the three finish outcomes, on the list and on the yardstick's output
    for masked in (False, True):
        oc = outcomes(c, masked)
        for order in (1, 2):
            which, ref = yardstick(c, order, masked)
            assert np.array_equal(ref == (MISSING if masked else -1.0e20), oc == 2), (name, order, masked)
            assert np.all(bits(ref[oc == 1]) == 0), (name, order, masked)                   # +0.0
        if big:
            for k in (0, 1) if masked else (0,):
                n = [int(np.count_nonzero(oc[k] == v)) for v in range(3)]
                assert n[0] >= 2 and n[1] >= 2 and (n[2] >= 2 or profile in ("eights", "long", "huge")), (name, masked, k, n)
            if masked:
                assert np.all(oc[K_NONE] == 2) and np.count_nonzero(oc[K_FULL] == 1) >= 2
                assert np.count_nonzero(np.any(oc == 1, axis=0) & np.any(oc == 0, axis=0)) >= 2      # 0.0 at one level, a value at another
                kinds = {k: [d for d, v in c["special"].items() if v == k] for k in ("Z", "ZM", "MR", "FL")}
                assert all(len(v) == 3 for v in kinds.values())
                assert np.all(oc[0][kinds["Z"]] == 1) and np.all(oc[0][kinds["ZM"]] == 2) and np.all(oc[0][kinds["MR"]] == 2)
                assert np.all(oc[1][kinds["FL"]] == 1) and np.all(oc[0][kinds["FL"]] == 0)
            else:
                assert np.count_nonzero(oc[0] == 1) >= 4                                    # Z and ZM rows
    # an order mistake cannot hide: adding in reversed order changes the bits of at least half of the rows with 4 or more cells
    for key, (changed, rows) in order_sensitive(c).items():
        assert 2 * changed >= rows, (name, key, changed, rows)
    return True
