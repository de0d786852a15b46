"""runoff_regrid without a device: the uncontracted wide sincos against this host's libm, the shared conversion and distance
code of csrc/runoff.h (a host build, run as a stand-alone program) against the reference's imap / jmap in every fixture, and
the fixtures' data_out against a numpy restatement of process_data's loops."""
import subprocess

import numpy as np
import pytest

import runoff_cases as rc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("seed", [31, 32])
def test_wide_sincos_bit_identical_to_host_sincos(seed):
    """8e6 arguments per seed: a quarter uniform in [-4 pi, 4 pi], k pi/2 +- 2^-e, the hand-over points 0.855 and 2.4262, reduced
    arguments around 0.126, an eighth uniform in [-1024, 1024], the bound itself; NaN beyond it.  libm's sincos() evaluates
    without contraction on every x86-64 host, with or without FMA, so this holds on both."""
    res = subprocess.run([rc.hostcheck_exe(), "sincos", "8000000", str(seed)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.startswith("bad 0 "), res.stdout + res.stderr


@pytest.mark.parametrize("name", rc.CASES)
def test_host_build_reproduces_reference_maps(name, tmp_path):
    fx, gi, go = rc.load(name)
    imap, jmap = rc.hostcheck_nearest(tmp_path, go["mask"], go["xt"], go["yt"])[:2]
    assert np.array_equal(imap, fx["imap"]) and np.array_equal(jmap, fx["jmap"])


@pytest.mark.parametrize("name", rc.CASES)
def test_fixture_data_out_is_process_data_on_its_own_list(name):
    fx, gi, go = rc.load(name)
    for lev in range(3):
        out = rc.process_data_numpy(fx, go, gi, fx["data_in"][lev])
        assert np.array_equal(_bits(out), _bits(fx["data_out"][lev])), (name, lev)
        tin = 0.0
        for v, a, m in zip(fx["data_in"][lev].ravel(), gi["area"].ravel(), gi["mask"].ravel()):
            if m > 0:
                tin += v * a
        assert tin == fx["totals"][lev, 0]


def test_fixture_cases_hold_what_they_are_for():
    fx, gi, go = rc.load("dup_points")
    assert go["xt"][5, 4] == go["xt"][7, 9] and go["yt"][5, 4] == go["yt"][7, 9] and go["mask"][5, 4] != 0 and go["mask"][7, 9] != 0
    assert ((fx["jmap"] == 5) & (fx["imap"] == 4)).any() and not ((fx["jmap"] == 7) & (fx["imap"] == 9)).any()
    fx, gi, go = rc.load("tripolar_small")
    assert go["n_ext"] == 1 and np.all(go["mask"][0] == 0) and go["xt"].min() < -2.4263 and go["xt"].max() > 0.9
    assert np.array_equal(go["yt"][0], (0.5 * (-90 + fx["y_super"][0, 0:-1:2])) * (np.pi / 180))
    fx, gi, go = rc.load("latlon_regular")
    assert go["n_ext"] == 0 and go["mask"][14, 10] != 0 and np.all(go["mask"][13:16, 9:12].ravel()[[0, 1, 2, 3, 5, 6, 7, 8]] == 0)
    fx, gi, go = rc.load("one_ocean_cell")
    land = go["mask"] == 0
    assert (go["mask"] != 0).sum() == 1 and np.all(fx["imap"][land] == 7) and np.all(fx["jmap"][land] == 6)
    for name in rc.CASES:
        fx = rc.load(name)[0]
        d = fx["data_in"]
        valid = d[0] != rc.MISSING
        lev = d[:2][:, valid]
        pos = lev[lev > 0]
        assert lev.min() == 0 and np.log10(pos.max() / pos.min()) > 11          # non-negative, zeros, 12 decades
        assert (d[2][valid] < 0).any() and (d[2][valid] == 0).any() and not np.isnan(d).any()
