"""Order-2 input preparation on the device against the CPU oracle at the shapes the aligned C16 .. C48 cases never reach
(tests/gridutil.py:c2l_mosaic): cell counts that are no multiple of the record kernels' blocks (64 / 128 cells), so that
d_store_records runs a short first pass, a short second pass and an empty one; tiles with nx != ny; tiles of different
sizes, which tell dx_off from dy_off and ew_off from es_off; one tile alone; edges without a contact, whose halo keeps
init_halo's zero.  Every comparison is bit equality on uint64 views and no cell is left out: the missing marker is a
moderate -999.0, so that no gradient overflows."""
import numpy as np
import pytest

import gridutil
import orc
from test_gpu_c2l import oracle_prepare

pytestmark = pytest.mark.gpu
MOSAICS = ["c9", "c10", "patches", "unequal", "single"]
MISSING = -999.0
DEV = "cuda:0"
SLACK = 128                                   # cells: one block of the widest record kernel


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def mosaics(fg, gpu_ok):
    """name -> (mosaic, C2lPrep), built on first use, destroyed with the module"""
    made = {}

    def get(name):
        if name not in made:
            m = gridutil.c2l_mosaic(fg, name)
            made[name] = (m, fg.C2lPrep(m["nx"], m["ny"], m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"]))
        return made[name]
    yield get
    for _, prep in made.values():
        prep.destroy()


def _cat(per_tile, nz):
    """per-tile [nz][...] arrays -> [nz][sum of the tiles' sizes], tiles back to back"""
    return np.ascontiguousarray(np.stack([np.concatenate([np.asarray(a[k]).ravel() for a in per_tile]) for k in range(nz)]))


def _missing_levels(nz):
    """level -> what is missing there: everything on level 0 of a single level and on level 2 of three or more, the edge
    row alone on level 3; the other levels have no missing cell"""
    lev = {0: "all"} if nz < 3 else {2: "all"}
    if nz >= 4:
        lev[3] = "edge"
    return lev


def _put_missing(m, interior, nz):
    nx, ny = m["nx"], m["ny"]
    for k, what in _missing_levels(nz).items():
        interior[0][k][ny[0] - 1, :] = MISSING                     # tile 0's whole north row: its neighbour sees it through the halo
        if what == "all":
            for t in range(len(nx)):                               # the cells in the four corners, next to init_halo's zero
                for j in (0, ny[t] - 1):
                    for i in (0, nx[t] - 1):
                        interior[t][k][j, i] = MISSING
            interior[0][k][ny[0] // 2, nx[0] // 2] = MISSING       # one cell away from the edges (where the tile has such)


def _fields(m, nz, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((nz, m["ny"][t], m["nx"][t])) + 4.0 for t in range(len(m["nx"]))]


def _nan(n, dtype=None):
    import torch
    return torch.full((n,), float("nan"), dtype=dtype or torch.float64, device=DEV)


def _check_records(prep, nz, rec_flat, field, gx, gy, what):
    """rec_flat: (ncells + SLACK) records; the first ncells hold {field, grad_x, grad_y} x levels, zero padded, the rest is
    untouched"""
    nb = type(prep).records_nb(nz)
    r = rec_flat.cpu().numpy().reshape(prep.ncells + SLACK, 3, nb)
    assert np.all(np.isnan(r[prep.ncells:])), what + ": store past the last cell"
    r = r[:prep.ncells]
    assert np.array_equal(_bits(r[:, 0, :nz].T), _bits(field)), what + ": field"
    assert np.array_equal(_bits(r[:, 1, :nz].T), _bits(gx)), what + ": grad_x"
    assert np.array_equal(_bits(r[:, 2, :nz].T), _bits(gy)), what + ": grad_y"
    assert np.array_equal(_bits(r[:, :, nz:]), _bits(np.zeros_like(r[:, :, nz:]))), what + ": padding levels"


@pytest.mark.parametrize("nz", range(1, 9))
@pytest.mark.parametrize("name", MOSAICS)
def test_prepare_bitwise_at_awkward_shapes(fg, mosaics, name, nz):
    """fill_halo + gradient (+ mask), gradient_records and records against the oracle, all three record widths (2, 4, 8 levels),
    padded and exact."""
    import torch
    m, prep = mosaics(name)
    nx, ny = m["nx"], m["ny"]
    nt = len(nx)
    assert prep.ncells == sum(a * b for a, b in zip(nx, ny)) and prep.F == sum((a + 2) * (b + 2) for a, b in zip(nx, ny))
    interior = _fields(m, nz, 100 * MOSAICS.index(name) + nz)
    _put_missing(m, interior, nz)
    data_o, gx_o, gy_o, mask_o, xt_o, yt_o = oracle_prepare(fg, (nx, ny), m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"],
                                                            interior, nz, MISSING)
    ref_h, ref_gx, ref_gy, ref_m = _cat(data_o, nz), _cat(gx_o, nz), _cat(gy_o, nz), _cat(mask_o, nz)
    src_np = _cat(interior, nz)
    assert np.all(np.isfinite(ref_gx)) and np.all(np.isfinite(ref_gy))           # nothing overflows: nothing is excluded
    nc, F = prep.ncells, prep.F
    src = torch.from_numpy(src_np).to(DEV)
    halo, gx, gy = _nan(nz * F + 256), _nan(nz * nc + 256), _nan(nz * nc + 256)
    gm = torch.full((nz * nc + 256,), -7, dtype=torch.int32, device=DEV)
    nb = fg.C2lPrep.records_nb(nz)
    rec_a, rec_b = _nan((nc + SLACK) * 3 * nb), _nan((nc + SLACK) * 3 * nb)
    torch.cuda.synchronize()                   # (the fills run on torch's stream, the library on its own)
    prep.fill_halo(src, halo, nz)
    prep.gradient(halo, nz, gx, gy, gm, has_missing=True, missing=MISSING)
    prep.gradient_records(halo, nz, rec_a)
    prep.records(src, nz, rec_b)
    prep.sync()
    h, x, y, k = halo.cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy(), gm.cpu().numpy()
    assert np.all(np.isnan(h[nz * F:])) and np.all(np.isnan(x[nz * nc:])) and np.all(np.isnan(y[nz * nc:])) and np.all(k[nz * nc:] == -7)
    assert np.array_equal(_bits(h[:nz * F].reshape(nz, F)), _bits(ref_h))
    cx, cy = prep.centres()
    assert np.array_equal(_bits(cx), _bits(np.concatenate([a.ravel() for a in xt_o])))
    assert np.array_equal(_bits(cy), _bits(np.concatenate([a.ravel() for a in yt_o])))
    assert np.array_equal(_bits(x[:nz * nc].reshape(nz, nc)), _bits(ref_gx))
    assert np.array_equal(_bits(y[:nz * nc].reshape(nz, nc)), _bits(ref_gy))
    got_m = k[:nz * nc].reshape(nz, nc)
    assert np.array_equal(got_m, ref_m)
    marked = _missing_levels(nz)
    for lev in range(nz):
        assert (ref_m[lev].sum() > 0) if lev in marked else (ref_m[lev].sum() == 0), lev
        if marked.get(lev) == "edge" and len(m["contacts"]["tile1"]):
            assert ref_m[lev][nx[0] * ny[0]:].sum() > 0        # the neighbour tile sees tile 0's row, and only through its halo
    _check_records(prep, nz, rec_a, src_np, ref_gx, ref_gy, "gradient_records")
    _check_records(prep, nz, rec_b, src_np, ref_gx, ref_gy, "records")
    if nt > 1 and not len(m["contacts"]["tile1"]):
        assert np.all(ref_h.reshape(nz, F)[:, np.concatenate([_halo_ring(nx[t], ny[t]) for t in range(nt)])] == 0.0)


def _halo_ring(nx, ny):
    r = np.ones((ny + 2, nx + 2), dtype=bool)
    r[1:-1, 1:-1] = False
    return r.ravel()


@pytest.mark.parametrize("nz", range(1, 9))
@pytest.mark.parametrize("name", ["unequal", "single", "patches"])
def test_caller_supplied_halos(fg, mosaics, name, nz):
    """fill_halo(src=None): interiors and halos come from the caller, random halo values, so the a2b edge and corner formulas
    work on non-zero halos with nx != ny.  Where a contact exists ('patches') the update overwrites its halo cells, in the
    oracle as on the device."""
    import torch
    m, prep = mosaics(name)
    nx, ny = m["nx"], m["ny"]
    nt = len(nx)
    rng = np.random.default_rng(900 + 10 * nz + len(name))
    given = [rng.standard_normal((nz, ny[t] + 2, nx[t] + 2)) + 4.0 for t in range(nt)]
    data_o, gx_o, gy_o, _, _, _ = oracle_prepare(fg, (nx, ny), m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"],
                                                 None, nz, None, halo_data=given)
    ref_h, ref_gx, ref_gy = _cat(data_o, nz), _cat(gx_o, nz), _cat(gy_o, nz)
    if not len(m["contacts"]["tile1"]):
        assert np.array_equal(_bits(ref_h), _bits(_cat(given, nz)))
    nc, F = prep.ncells, prep.F
    halo = torch.from_numpy(_cat(given, nz)).to(DEV)
    gx, gy = _nan(nz * nc + 256), _nan(nz * nc + 256)
    rec = _nan((nc + SLACK) * 3 * fg.C2lPrep.records_nb(nz))
    torch.cuda.synchronize()
    prep.fill_halo(None, halo, nz)
    prep.gradient(halo, nz, gx, gy)
    prep.gradient_records(halo, nz, rec)
    prep.sync()
    assert np.array_equal(_bits(halo.cpu().numpy()), _bits(ref_h))
    x, y = gx.cpu().numpy(), gy.cpu().numpy()
    assert np.all(np.isnan(x[nz * nc:])) and np.all(np.isnan(y[nz * nc:]))
    assert np.array_equal(_bits(x[:nz * nc].reshape(nz, nc)), _bits(ref_gx))
    assert np.array_equal(_bits(y[:nz * nc].reshape(nz, nc)), _bits(ref_gy))
    field = _cat([d[:, 1:-1, 1:-1] for d in data_o], nz)
    _check_records(prep, nz, rec, field, ref_gx, ref_gy, "gradient_records")


@pytest.mark.parametrize("nz", [1, 5, 8])
def test_records_to_sweep_end_to_end_c10(fg, mosaics, nz):
    """C10 -> 30 x 15 conserve_order2: records -> XgridPlan.apply_records against oracle_prepare -> orc_apply, on a plan that
    holds the oracle's exchange cells (create_empty + set_xgrid), bit for bit."""
    import torch
    m, prep = mosaics("c10")
    nx, ny = m["nx"], m["ny"]
    nlon, nlat = 30, 15
    lo, la = fg.latlon_corners(nlon, nlat)
    o = orc.orc_setup(2, [(nx[t], ny[t], m["lon"][t], m["lat"][t]) for t in range(6)], [(nlon, nlat, lo, la)])
    interior = _fields(m, nz, 40 + nz)
    data_o, gx_o, gy_o, _, _, _ = oracle_prepare(fg, (nx, ny), m["lon"], m["lat"], m["lont"], m["latt"], m["contacts"], interior, nz)
    ref, _ = orc.orc_apply(2, o, nx, ny, [d.reshape(nz, -1) for d in data_o], gx_o, gy_o, None, False, 0.0, nlon, nlat, nz)
    plan = fg.XgridPlan.create_empty(2, nx, ny, nlon, nlat)
    plan.set_xgrid(o["t_in"], o["i_in"], o["j_in"], o["i_out"], o["j_out"], o["area"], o["di"], o["dj"])
    src = torch.from_numpy(_cat(interior, nz)).to(DEV)
    rec = _nan((prep.ncells + SLACK) * 3 * fg.C2lPrep.records_nb(nz))
    out = _nan(nz * nlon * nlat + 256)
    torch.cuda.synchronize()
    prep.records(src, nz, rec)
    prep.sync()
    plan.apply_records(nz, rec, out)
    plan.sync()
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[nz * nlon * nlat:]))
    assert np.array_equal(_bits(got[:nz * nlon * nlat]), _bits(ref))
    plan.destroy()
