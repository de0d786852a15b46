"""fg_extrap_run_batch_dev -- several records of the --extrapolate fill per launch -- against the REFERENCE's answers through the
fixtures of the single-record fill (tests/golden/extrapolate_*.npz, inputs rebuilt by tests/extrap_cases.py).  The contract is
that every record comes back, bit for bit, as fg_extrap_run_dev gives it alone: whatever the other records are, in whatever
order, for every fg_set_extrap_batch and both coefficient modes.  No tolerance anywhere: bits, counts, and the six digits of the
largest residual the reference printed."""
import ctypes as C
import itertools

import numpy as np
import pytest

import extrap_cases as ec

pytestmark = pytest.mark.gpu
_dpt = C.POINTER(C.c_double)
_ipt = C.POINTER(C.c_int)
TRIO = ["warm", "none_missing", "whole_level"]            # 72 x 45 cyclic, missing = -1e20; warm truncated to its levels 0-1
TRIO_ITERS = [[283, 71], [0, 0], [265, 82]]               # the reference's counts (from the fixtures, asserted below)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def trio():
    """[(name, case, record [2, nj, ni], fixture)] -- computed once, never written to"""
    recs = []
    for name in TRIO:
        c, fx = ec.extrap_case(name), np.load(ec.golden_path(name))
        rec = np.ascontiguousarray(c["data"][:2])
        rec.setflags(write=False)
        recs.append((name, c, rec, fx))
    assert [list(fx["iters"][:2]) for _, _, _, fx in recs] == TRIO_ITERS
    # the records stop in different launches on both levels and end them in different buffers; one never iterates
    assert [[(n + 1) & 1 for n in it] for it in TRIO_ITERS] == [[0, 0], [1, 1], [0, 1]]
    return recs


def make(fg, c):
    return fg.Extrapolator(c["lon"], c["lat"], c["is_cyclic"])


def check_record(name, fx, out, iters, resmax, nk):
    print(name, "iters", list(iters), "reference", list(fx["iters"][:nk]), "resmax", list(resmax), "printed", list(fx["maxres_printed"][:nk]))
    assert np.array_equal(iters, fx["iters"][:nk])
    for k in range(nk):
        assert "%g" % resmax[k] == str(fx["maxres_printed"][k])
    assert np.array_equal(bits(out), bits(fx["out"][:nk]))


def test_three_records_that_stop_in_different_launches(fg, gpu_ok, trio):
    """a shared stop, a shared parity or a shared mask word (72 * 45 = 3240 cells is no multiple of 64) fails here"""
    data = np.stack([rec for _, _, rec, _ in trio])
    with make(fg, trio[0][1]) as ex:
        out, iters, resmax = ex.run_batch(data, -1.0e20, 0.005)
        assert out.shape == data.shape and iters.shape == resmax.shape == (3, 2)
        for r, (name, _, _, fx) in enumerate(trio):
            check_record(name, fx, out[r], iters[r], resmax[r], 2)
        assert ex.last_syncs == 5 + 2                                     # ceil(284 / 64) + ceil(83 / 64)


@pytest.mark.parametrize("stored", [0, 1])
@pytest.mark.parametrize("batch", [1, 7, 64])
def test_every_order_every_batch_both_coefficient_modes(fg, gpu_ok, trio, batch, stored):
    import torch
    try:
        fg.set_extrap_batch(batch)
        fg.set_extrap_coef(stored)
        with make(fg, trio[0][1]) as ex:
            for order in itertools.permutations(range(3)):
                d = torch.from_numpy(np.stack([trio[q][2] for q in order])).cuda()
                out, iters, resmax = ex.run_batch(d, -1.0e20, 0.005)
                out = out.cpu().numpy()
                for r, q in enumerate(order):
                    check_record(trio[q][0], trio[q][3], out[r], iters[r], resmax[r], 2)
                want = sum(-(-(max(TRIO_ITERS[q][k] for q in range(3)) + 1) // batch) for k in range(2))
                assert ex.last_syncs == want
    finally:
        fg.set_extrap_batch(0)
        fg.set_extrap_coef(0)


def test_two_records_run_to_the_cap(fg, gpu_ok):
    c, fx = ec.extrap_case("cap"), np.load(ec.golden_path("cap"))
    with make(fg, c) as ex:
        out, iters, resmax = ex.run_batch(np.stack([c["data"], c["data"]]), c["missing"], 0.0)
    for r in range(2):
        assert iters[r, 0] == 3999
        check_record("cap", fx, out[r], iters[r], resmax[r], 1)


@pytest.mark.parametrize("name", ["regional", "stretched", "eps"])
def test_one_record_equals_the_single_record_entry(fg, gpu_ok, name):
    """non-cyclic 60 x 40; non-uniform axes; missing = -999 with the <= 1e-10 rule"""
    c, fx = ec.extrap_case(name), np.load(ec.golden_path(name))
    with make(fg, c) as ex:
        out, iters, resmax = ex.run_batch(c["data"][None], c["missing"], c["stop_crit"])
        one, it1, rm1 = ex.run(c["data"], c["missing"], c["stop_crit"])
    check_record(name, fx, out[0], iters[0], resmax[0], c["nk"])
    assert np.array_equal(bits(out[0]), bits(one)) and np.array_equal(iters[0], it1) and np.array_equal(bits(resmax[0]), bits(rm1))


def test_real_grid_with_a_record_of_permuted_levels(fg, gpu_ok):
    name = "real_360x180"
    c, fx = ec.extrap_case(name), np.load(ec.golden_path(name))
    other = np.ascontiguousarray(c["data"][[2, 0, 1]])
    with make(fg, c) as ex:
        out, iters, resmax = ex.run_batch(np.stack([c["data"], other]), c["missing"], c["stop_crit"])
        one, it1, rm1 = ex.run(other, c["missing"], c["stop_crit"])
    print("iters", iters.tolist(), "reference", list(fx["iters"]), "alone", list(it1))
    assert np.array_equal(iters[0], fx["iters"]) and ["%g" % v for v in resmax[0]] == [str(s) for s in fx["maxres_printed"]]
    assert ec.sha256(out[0]) == str(fx["sha256"])
    assert np.array_equal(bits(out[0].reshape(-1)[ec.sample_index(out[0].size)]), bits(fx["sample"]))
    assert np.array_equal(bits(out[1]), bits(one)) and np.array_equal(iters[1], it1) and np.array_equal(bits(resmax[1]), bits(rm1))


def test_in_place_and_with_padding(fg, gpu_ok, trio):
    import torch
    ncell = 72 * 45
    lstride, rstride = ncell + 100, 2 * (ncell + 100) + 37
    buf = torch.full((3, rstride), 7.0, dtype=torch.float64, device="cuda")
    for r, (_, _, rec, _) in enumerate(trio):
        for k in range(2):
            buf[r, k * lstride:k * lstride + ncell] = torch.from_numpy(rec[k].reshape(-1).copy()).cuda()
    iters, resmax = np.empty((3, 2), dtype=np.int32), np.empty((3, 2))
    with make(fg, trio[0][1]) as ex:
        torch.cuda.synchronize()
        fg._lib.check(fg.lib().fg_extrap_run_batch_dev(ex.handle, 3, buf.data_ptr(), buf.data_ptr(), 2, lstride, rstride, -1.0e20, 0.005,
                                                       iters.ctypes.data_as(_ipt), resmax.ctypes.data_as(_dpt)))
    h = buf.cpu().numpy()
    for r, (name, _, _, fx) in enumerate(trio):
        got = np.stack([h[r, k * lstride:k * lstride + ncell].reshape(45, 72) for k in range(2)])
        check_record(name, fx, got, iters[r], resmax[r], 2)
        for k in range(2):
            assert np.all(h[r, k * lstride + ncell:(k + 1) * lstride] == 7.0)              # the padding comes back untouched
        assert np.all(h[r, 2 * lstride:] == 7.0)


def test_argument_errors_leave_the_handle_usable(fg, gpu_ok, trio):
    import torch
    ncell = 72 * 45
    d = torch.from_numpy(np.stack([rec for _, _, rec, _ in trio])).cuda()
    o = torch.empty_like(d)
    with make(fg, trio[0][1]) as ex:
        run = lambda nrec, nk, ls, rs, a=d.data_ptr(), b=o.data_ptr(): fg.lib().fg_extrap_run_batch_dev(  # noqa: E731
            ex.handle, nrec, a, b, nk, ls, rs, -1.0e20, 0.005, None, None)
        torch.cuda.synchronize()
        for args in ((0, 2, 0, 0), (-1, 2, 0, 0), (3, 0, 0, 0), (3, 2, ncell - 1, 0), (3, 2, 0, 2 * ncell - 1), (3, 2, ncell + 8, 2 * ncell + 7)):
            assert run(*args) == -1, args
            assert fg._lib.last_error()
        assert run(3, 2, 0, 0, a=None) == -1 and run(3, 2, 0, 0, b=None) == -1
        assert fg.lib().fg_extrap_run_batch_dev(None, 3, d.data_ptr(), o.data_ptr(), 2, 0, 0, -1.0e20, 0.005, None, None) == -1
        assert run(3, 2, 0, 0) == 0                                        # NULL iters / resmax are allowed
        out = o.cpu().numpy()
        for r, (name, _, _, fx) in enumerate(trio):
            assert np.array_equal(bits(out[r]), bits(fx["out"][:2]))
