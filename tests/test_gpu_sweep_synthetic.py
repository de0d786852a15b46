"""The sweep kernels (csrc/apply_kernels.hip) on the hand-made exchange lists of tests/sweep_cases.py: row lengths far from the
mean the kernels are chosen by, list order that is not source order, pairs listed twice, rows whose counted cells all have area 0.
Plans come from create_empty + set_xgrid.  Every output is compared bit for bit, no cell left out, with the reference's own
do_scalar_conserve_interp on the same list (oracle/_ref/libconserve_ref.so; where it is not built, with the plain float64 loop of
sweep_cases.plain, and the test prints which one ran).  Every output buffer is followed by NaN slack that must stay NaN.

What each profile is meant to reach (bin = nx // ndst; lines of csrc/apply_kernels.hip the choice was read from -- a change of a
threshold there needs a new look at this table):

  entry point            profile (bin)                kernel                                                   dispatch
  set_xgrid              short, spike, eights (<=6)   k_csr_sortgather<., 64, ., 64>: staged blocks, the        fgd_csr_sortgather :1105-1107,
                                                      unstaged block (spike: > 512 cells in 64 rows), rows      kernel :96, :103, :136-190
                                                      of 12 / 13 (SHORT), 255..512 through LDS, 513 / 700
                                                      through tmp
                         mid, long, huge (8 < mean    k_csr_sortgather<., 16, ., 256>: huge: the row of 2048    :1105, :117, :149, :159
                         <= 256)                      ranks in LDS, the row of 2503 through tmp
                         huge-5 (mean > 256)          k_csr_sortgather<., 1, ., 256>                            :1105
  apply nz = 1           every profile                k_apply_ep1<O, MISSING, 256, 512, R>, R = 64 / 16 / 4 / 1  fgd_apply1 :1134-1143,
                                                      by bin; spike, eights: the chunk walk inside a 64-row     by_row_length :1125
                                                      tile; huge: a tile of one row walking 5 chunks
                         (fg_set_apply_ep(0))         k_apply1<O, MISSING>                                      :1145-1152
  apply nz = 2..17       order 1, <=6                 k_apply_il<1, NB, V>, NB = 2 / 4 / 8 (nz 9, 17: a last     fgd_apply_il :1189-1196
                                                      chunk of one level through fgd_apply1)
                         order 1, other bins, NB 8    k_apply_ep8g<1, false, 256, 256, R>, R = 8 / 2 / 1        :1185-1186
                         order 2, NB 2 / 4            k_apply_il<2, NB, 2, MERGED>                              fgd_apply_il_merged :1211-1212
                         order 2, NB 8, <=6           k_apply_ep8<256, 256>; spike, eights: tiles of more than   :1206-1207, kernel :790, :823-832
                                                      256 records take its row-serial path, past sh_e
                         order 2, NB 8, other bins    k_apply_ep8g<2, false, 256, 256, R>                       :1208-1209
                         (ep(0), vec(1 / 2 / 4))      k_apply_il<1, 8, 1 / 2 / 4>, k_apply_il<2, 8, 2 / 4,       :1189-1196, :1210
                                                      MERGED>
  apply_interleaved      nb 16, 8                     k_apply_il<O, 16, 4>, k_apply_il<O, 8, 4>; order 1 nb 8    fgd_apply_il :1185-1196
                                                      above the first bin: k_apply_ep8g, interleaved output
  apply_records          spike, long                  as order 2 above, records built here                      fgd_apply_il_merged
  apply_levels,          every profile                k_apply_ep8g<O, true, 256, 256, R>, R = 32 / 8 / 2 / 1:    fgd_apply_levels8 :1220-1221
  apply_records_levels                                `touched` against the area sum (Z, ZM, MR, FL rows)       kernel :924-934
  apply_ex               spike, eights, long          k_apply_epx<O, MONO, 256, 512, R>; ep(0): k_apply_ex       fgd_apply_ex :1275-1291
  fg_set_apply_xcd       huge, short on 201, 99 rows  d_xcd_block with 201, 99, 7, 4, 2 tiles                   :237-250
"""
import numpy as np
import pytest
import torch

import orc
import sweep_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MISSING, NLEV, K_FULL, K_NONE = sc.MISSING, sc.NLEV, sc.K_FULL, sc.K_NONE
SLACK = 64
ORDERS = (1, 2)
HOOK_DEFAULTS = dict(fg_set_apply_ep=1, fg_set_apply_vec=0, fg_set_apply_xcd=64)


class Hooks:
    """the tuning hooks set for a block of calls, back at their defaults afterwards whatever happens"""
    def __init__(self, fg, **kw):
        self.L, self.kw = fg.lib(), kw

    def __enter__(self):
        try:
            for k, v in self.kw.items():
                getattr(self.L, "fg_set_apply_" + k)(v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *a):
        for k, v in HOOK_DEFAULTS.items():
            getattr(self.L, k)(v)


def _out(*shape):
    """an output of that shape with SLACK doubles behind it, all NaN"""
    n = int(np.prod(shape))
    buf = torch.full((n + SLACK,), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()                                                          # the plan sweeps on a stream of its own
    return buf, buf[:n].view(*shape)


def _get(c, buf, view):
    c["plan"].sync()
    host = buf.cpu().numpy()
    assert np.all(np.isnan(host[view.numel():])), "the slack behind the output was written"
    return host[:view.numel()].reshape(tuple(view.shape))


def _assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(sc.bits(got) != sc.bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} cells differ, first at {bad[:4].tolist()}: " \
                          f"{got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}"


@pytest.fixture(scope="module")
def cases(fg, gpu_ok):
    made = {}
    print("yardstick:", "the reference library" if orc.conserve_ref_available() else "the plain float64 loop (oracle/_ref not built)")

    def get(name, order):
        if (name, order) not in made:
            c = dict(sc.make(name))
            sc.check_preconditions(sc.make(name))
            x = c["x"]
            plan = fg.XgridPlan.create_empty(order, c["tnx"], c["tny"], c["nxo"], c["nyo"])
            plan.set_xgrid(x["t_in"], x["i_in"], x["j_in"], x["i_out"], x["j_out"], x["area"], x["di"] if order == 2 else None,
                           x["dj"] if order == 2 else None)
            assert plan.nxgrid == c["nx"] and plan.ncells_in == c["nsrc"]
            c["plan"], c["order"] = plan, order
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
            c["f"] = {m: dev(sc.field(c, order, m)) for m in (False, True)}
            c["g"] = dict(gx=dev(c["gx"]), gy=dev(c["gy"]), gm=dev(c["gm"])) if order == 2 else dict(gx=None, gy=None, gm=None)
            c["ref"] = {m: sc.yardstick(sc.make(name), order, m)[1] for m in (False, True)}
            c["dev"] = dev
            made[(name, order)] = c
        return made[(name, order)]
    yield get
    for c in made.values():
        c["plan"].destroy()


def _grads(c, k):
    """keyword arguments of the order-2 gradients of level(s) k"""
    if c["order"] != 2:
        return {}
    return dict(grad_x_t=c["g"]["gx"][k], grad_y_t=c["g"]["gy"][k])


def _apply(c, nz, masked=False, k0=0, want_gsum=False):
    """plan.apply on levels [k0, k0 + nz) -> ([nz][ndst], gsum)"""
    buf, out = _out(nz, c["ndst"])
    k = slice(k0, k0 + nz)
    kw = _grads(c, k)
    if masked and c["order"] == 2:
        kw["grad_mask_t"] = c["g"]["gm"][k0]
    g = c["plan"].apply(c["f"][masked][k].contiguous(), out, nz=nz, has_missing=masked, missing=MISSING, want_gsum=want_gsum, **kw)
    return _get(c, buf, out), g


ALL = [(n, o) for n in sc.CASES for o in ORDERS]
ids = lambda ps: ["-".join(str(v) if not isinstance(v, int) or k == 0 else f"order{v}" for k, v in enumerate(p)) for p in ps]


# ------------------------------------------------------------------------------------------------------------- one level
@pytest.mark.parametrize("masked", (False, True), ids=("plain", "missing"))
@pytest.mark.parametrize("name,order", ALL, ids=ids(ALL))
def test_apply_one_level(fg, cases, name, order, masked):
    """k_apply_ep1 at the four rows-per-tile values, and k_apply1 (fg_set_apply_ep(0))"""
    c = cases(name, order)
    for ep in (1, 0):
        with Hooks(fg, ep=ep):
            for k in (0, 1, K_FULL, K_NONE):
                got, _ = _apply(c, 1, masked, k)
                _assert_bits(got[0], c["ref"][masked][k], f"ep {ep} level {k}")
    if masked:
        assert np.all(got[0] == MISSING)                                              # K_NONE


# --------------------------------------------------------------------------------------------------- levels, nothing missing
@pytest.mark.parametrize("name,order", ALL, ids=ids(ALL))
def test_apply_levels_without_missing(fg, cases, name, order):
    """k_apply_il at NB 2 / 4 / 8, k_apply_ep8 (order 2, first bin), k_apply_ep8g unmasked; nz 9 and 17 end in a one-level chunk"""
    c = cases(name, order)
    for nz in (2, 3, 4, 5, 8, 9, 16, 17):
        got, _ = _apply(c, nz)
        _assert_bits(got, c["ref"][False][:nz], f"nz {nz}")


HOOKED = [(n, o) for n in ("spike-804", "long-201") for o in ORDERS]


@pytest.mark.parametrize("name,order", HOOKED, ids=ids(HOOKED))
def test_apply_levels_hooks(fg, cases, name, order):
    """the same with fg_set_apply_ep(0) and fg_set_apply_vec(1 / 2 / 4): k_apply_il at one, two and four levels per lane"""
    c = cases(name, order)
    for ep in (0, 1):
        for vec in (0, 1, 2, 4):
            with Hooks(fg, ep=ep, vec=vec):
                for nz in (2, 4, 8, 9):
                    got, _ = _apply(c, nz)
                    _assert_bits(got, c["ref"][False][:nz], f"ep {ep} vec {vec} nz {nz}")


@pytest.mark.parametrize("name,order", HOOKED, ids=ids(HOOKED))
def test_apply_interleaved(fg, cases, name, order):
    c = cases(name, order)
    for nb in (16, 8):
        f = c["dev"](sc.field(c, order, False)[:nb].T)                                 # [cells (with halo)][nb]
        g = [c["dev"](c[k][:nb].T) for k in ("gx", "gy")] if order == 2 else [None, None]
        assert f.shape == ((c["nhalo"] if order == 2 else c["nsrc"]), nb)
        buf, out = _out(c["ndst"], nb)
        c["plan"].apply_interleaved(nb, f, out, g[0], g[1])
        _assert_bits(_get(c, buf, out).T, c["ref"][False][:nb], f"nb {nb}")


def _records(c, k0, nz, nbp, masked):
    """[source cell][3][nbp]: field, grad_x, grad_y of levels [k0, k0 + nz), zero beyond; built on the host"""
    rec = np.zeros((c["nsrc"], 3, nbp))
    f = np.where(c["miss"], MISSING, c["vals"]) if masked else c["vals"]
    for w, a in enumerate((f, c["gx"], c["gy"])):
        rec[:, w, :nz] = a[k0:k0 + nz].T
    return rec


RECORDS = ["spike-804", "long-201"]


@pytest.mark.parametrize("name", RECORDS)
def test_apply_records(fg, cases, name):
    c = cases(name, 2)
    for nz, nbp in ((8, 8), (5, 8), (3, 4), (2, 2), (1, 2)):
        rec = c["dev"](_records(c, 0, nz, nbp, False))
        buf, out = _out(nz, c["ndst"])
        g = c["plan"].apply_records(nz, rec, out, want_gsum=True)
        got = _get(c, buf, out)
        _assert_bits(got, c["ref"][False][:nz], f"records nz {nz}")
        if nz > 1:                                                                    # (one level: apply takes k_apply_ep1, its sum another tree)
            mine, g2 = _apply(c, nz, want_gsum=True)
            _assert_bits(got, mine, f"records against apply, nz {nz}")
            assert sc.bits(np.array([g]))[0] == sc.bits(np.array([g2]))[0], (nz, g, g2)


# ------------------------------------------------------------------------------------------------- levels with missing values
def _apply_levels(c, nlev, want_gsum=True):
    buf, out = _out(nlev, c["ndst"])
    g = c["g"]
    gs = c["plan"].apply_levels(c["f"][True][:nlev].contiguous(), out, nlev, MISSING, g["gx"], g["gy"], g["gm"], want_gsum=want_gsum)
    return _get(c, buf, out), gs


@pytest.mark.parametrize("name,order", ALL, ids=ids(ALL))
def test_apply_levels(fg, cases, name, order):
    """the MASKED k_apply_ep8g: every level is the reference's one-level call; sums as the one-level apply returns them"""
    c = cases(name, order)
    sums = {}
    for nlev in (1, 7, 8, 9, 17):
        got, sums[nlev] = _apply_levels(c, nlev)
        _assert_bits(got, c["ref"][True][:nlev], f"{nlev} levels")
    assert np.all(got[K_NONE] == MISSING)
    for nlev in (1, 7, 8, 9):
        assert np.array_equal(sc.bits(sums[nlev]), sc.bits(sums[17][:nlev])), nlev
    for k in range(NLEV):
        _, g1 = _apply(c, 1, True, k, want_gsum=True)
        assert sc.bits(np.array([g1]))[0] == sc.bits(sums[17][k:k + 1])[0], (k, g1, sums[17][k])
    got_nosum, none = _apply_levels(c, 9, want_gsum=False)
    assert none is None
    _assert_bits(got_nosum, c["ref"][True][:9], "9 levels, no sums")


@pytest.mark.parametrize("name", RECORDS)
def test_apply_records_levels(fg, cases, name):
    c = cases(name, 2)
    want, wsum = _apply_levels(c, NLEV)
    for k0, nz in ((0, 8), (8, 8), (16, 1), (2, 5)):
        rec = c["dev"](_records(c, k0, nz, 8, True))
        mb = np.zeros(c["nsrc"], dtype=np.uint8)
        for k in range(nz):
            mb |= (c["gm"][k0 + k] != 0).astype(np.uint8) << k
        buf, out = _out(nz, c["ndst"])
        g = c["plan"].apply_records_levels(nz, rec, c["dev"](mb), out, MISSING, want_gsum=True)
        _assert_bits(_get(c, buf, out), want[k0:k0 + nz], f"levels {k0}..{k0 + nz}")
        assert np.array_equal(sc.bits(g), sc.bits(wsum[k0:k0 + nz])), (k0, nz)


# ------------------------------------------------------------------------------------------------------------ every option
EX = [(n, o, opt) for n in ("spike-804", "eights-804", "long-201") for o in ORDERS for opt in sc.EX_OPTS[:4]] + \
     [(n + "-1t", 2, opt) for n in ("spike-804", "eights-804", "long-201") for opt in sc.EX_OPTS[4:]]


@pytest.mark.parametrize("name,order,opt", EX, ids=ids(EX))
def test_apply_ex(fg, cases, name, order, opt):
    """k_apply_epx and, with fg_set_apply_ep(0), k_apply_ex against the reference with the same options"""
    c = cases(name, order)
    kw = sc.ex_inputs(c, order, opt)
    which, ref = sc.yardstick_ex(sc.make(name), order, opt)
    t = lambda a, dt=None: c["dev"](a if dt is None else np.asarray(a, dtype=dt)) if a is not None else None
    args = dict(nz=1, grad_x_t=t(kw["gx"]), grad_y_t=t(kw["gy"]), grad_mask_t=t(kw["gm"], np.int32), has_missing=kw["has_missing"],
                missing=kw["missing"], weight_t=t(kw["weight"]), cell_methods_sum=kw["sum"], field_area_t=t(kw["field_area"]),
                cell_area_in_t=t(kw["cell_area_in"]), cell_area_out_t=t(kw["cell_area_out"]), monotonic=kw["monotonic"])
    data = t(kw["data"])
    for ep in (1, 0):
        with Hooks(fg, ep=ep):
            buf, out = _out(c["ndst"])
            c["plan"].apply_ex(data, out, **args)
            _assert_bits(_get(c, buf, out), ref, f"{opt} ep {ep} against {which}")


# ------------------------------------------------------------------------------------------------------------ tile mapping
MAPPED = [(n, o) for n in ("huge-201", "huge-99", "short-201", "short-99") for o in ORDERS]


@pytest.mark.parametrize("name,order", MAPPED, ids=ids(MAPPED))
def test_tile_mapping(fg, cases, name, order):
    """fg_set_apply_xcd(0 / 1 / 2) with 201, 99, 7, 4 and 2 tiles: no multiples of 8, below and above one round of chunks"""
    c = cases(name, order)
    ntiles = lambda rows: -(-c["ndst"] // rows)
    if c["profile"] == "huge":
        assert ntiles(1) == c["ndst"]
    else:
        assert (ntiles(64), ntiles(32)) == ((4, 7) if c["ndst"] == 201 else (2, 4))
    kw = sc.ex_inputs(c, order, "meas_target")
    _, ref_ex = sc.yardstick_ex(sc.make(name), order, "meas_target")
    t = lambda a, dt=None: c["dev"](a if dt is None else np.asarray(a, dtype=dt)) if a is not None else None
    args = dict(nz=1, grad_x_t=t(kw["gx"]), grad_y_t=t(kw["gy"]), grad_mask_t=t(kw["gm"], np.int32), has_missing=True, missing=MISSING,
                field_area_t=t(kw["field_area"]), cell_area_in_t=t(kw["cell_area_in"]), cell_area_out_t=t(kw["cell_area_out"]))
    data = t(kw["data"])
    for xcd in (0, 1, 2):
        with Hooks(fg, xcd=xcd):
            for masked in (False, True):
                got, _ = _apply(c, 1, masked)
                _assert_bits(got[0], c["ref"][masked][0], f"xcd {xcd} one level")
            for nz in (4, 8):
                got, _ = _apply(c, nz)
                _assert_bits(got, c["ref"][False][:nz], f"xcd {xcd} nz {nz}")
            buf, out = _out(c["ndst"])
            c["plan"].apply_ex(data, out, **args)
            _assert_bits(_get(c, buf, out), ref_ex, f"xcd {xcd} apply_ex")
            got, _ = _apply_levels(c, 8, want_gsum=False)                               # (the masked kernel keeps the identity mapping)
            _assert_bits(got, c["ref"][True][:8], f"xcd {xcd} levels")
