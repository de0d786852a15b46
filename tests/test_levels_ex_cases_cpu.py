"""tests/levels_ex_cases.py on the CPU: the preconditions of every case the GPU tests use, the plain float64 loop against the
reference's own do_scalar_conserve_interp per level for every option set, and the yardstick's teeth -- each mistake the new
kernel could make changes what the yardstick says."""
import numpy as np
import pytest

import orc
import levels_ex_cases as lx
import sweep_cases as sc

needs_ref = pytest.mark.skipif(not orc.conserve_ref_available(), reason="oracle/_ref/libconserve_ref.so not built")
TEETH = ("eights-804", "long-201")


@pytest.mark.parametrize("name", lx.CASES)
def test_preconditions(name):
    c = sc.make(name)
    assert sc.check_preconditions(c) and lx.check_preconditions(c)


def test_every_tiling_is_crossed_in_every_bin():
    """every bin of the chooser has a case other than `short`, so every (rows per tile, chunk) pair of the kernel walks chunks"""
    bins = {sc.make(n)["bin"] for n in lx.CASES if sc.parse(n)[0] != "short"}
    assert bins == set(lx.ROWS_PER_TILE)


@needs_ref
@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("name", lx.CASES)
def test_plain_loop_equals_the_reference(name, order):
    c = sc.make(name)
    for opt, masked in lx.SETS:
        ref, mine = lx.reference(name, order, opt, masked), lx.plain(c, order, opt, masked)
        bad = np.argwhere(sc.bits(ref) != sc.bits(mine))
        assert bad.size == 0, (lx.set_id(opt, masked), len(bad), bad[:4].tolist())


def _changed(a, b):
    return int(np.count_nonzero(sc.bits(a) != sc.bits(b)))


@pytest.mark.parametrize("name", TEETH)
def test_yardstick_has_teeth(name):
    c = sc.make(name)
    for order in (1, 2):
        for opt in lx.OPTS:
            base = lx.plain(c, order, opt, True)
            assert _changed(base, lx.plain(c, order, opt, True, reverse=True)) > c["ndst"], (opt, "order of addition")
        for opt in ("meas", "meas_z", "weight0+meas"):
            base = lx.plain(c, order, opt, True)
            assert _changed(base, lx.plain(c, order, opt, True, left_assoc=True)) > c["ndst"], (opt, "a*fa/ca")
        for opt in ("meas_z", "meas_z_target"):
            for masked in (True, False):
                base = lx.plain(c, order, opt, masked)
                other = lx.plain(c, order, opt, masked, shared_area=True)
                assert lx.sc.same(base[0], other[0]) and _changed(base[1:], other[1:]) > c["ndst"], (opt, "shared area")
        for opt in ("meas_target", "meas_z_target"):
            base = lx.plain(c, order, opt, True)
            other = lx.plain(c, order, opt, True, target_valid_only=True)
            v = (base != lx.MISSING) & (base != 0)
            assert np.array_equal(base == lx.MISSING, other == lx.MISSING)
            assert np.count_nonzero(np.abs(other[v] - base[v]) > 1e-6 * np.abs(base[v])) > c["ndst"], (opt, "target sum")
