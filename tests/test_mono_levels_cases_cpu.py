"""tests/mono_levels_cases.py on the CPU: the plain float64 loop equals the reference's monotone branch bit for bit on every case,
option set and level; the preconditions the GPU tests rely on hold; the fatal input is fatal."""
import numpy as np
import pytest

import mono_levels_cases as mc
import orc
import sweep_cases as sc


@pytest.mark.parametrize("name", mc.CASES)
def test_preconditions(name):
    facts = mc.check_preconditions(name)
    print(name, facts)


def test_preconditions_over_the_cases():
    print(mc.check_all_preconditions())


@pytest.mark.parametrize("name", mc.CASES)
def test_plain_loop_is_the_reference(name):
    if not orc.conserve_ref_available():
        pytest.skip("oracle/_ref/libconserve_ref.so not built")
    variants = [(o, m, None) for o, m in mc.SETS] + [("none", False, True)]
    for opt, masked, with_gm in variants:
        got, _ = mc.plain(name, opt, masked, with_gm)
        ref = mc.reference(name, opt, masked, with_gm)
        bad = np.argwhere(sc.bits(got) != sc.bits(ref))
        assert bad.size == 0, f"{name} {mc.set_id(opt, masked)} gm={with_gm}: {len(bad)} of {got.size} differ, first (level, cell) {bad[:4].tolist()}"
        assert np.any(got != (mc.MISSING if masked else -1.0e20))


def test_plain_loop_is_sweep_cases_one_level_loop():
    """on level 0 of sweep_cases' own tame field the generalised loop is sweep_cases.plain_ex, whichever library is built"""
    for name in ("spike-804-1t", "eights-804-1t", "long-201-1t"):
        c = sc.make(name)
        for opt, sc_opt in (("none", "mono"), ("none", "mono_missing")):
            kw = sc.ex_inputs(c, 2, sc_opt)
            mine = dict(data=kw["data"][None], gx=kw["gx"][None], gy=kw["gy"][None], gm=kw["gm"][None] if kw["gm"] is not None else None,
                        has_missing=kw["has_missing"], missing=kw["missing"], weight=None, sum=False, field_area=None, cell_area_in=None,
                        cell_area_out=None)
            got, _ = mc.plain_kw(c, mine)
            assert sc.same(got[0], sc.plain_ex(c, 2, sc_opt)), (name, sc_opt)


def test_the_fatal_input_is_fatal():
    seed, kw, e = mc.fatal_level()
    print("seed", seed, "excess", e.excess, e.message)
    assert e.excess >= mc.TOLERANCE and e.message in (mc.MSG_ABOVE, mc.MSG_BELOW)
    c = sc.make(mc.FATAL_CASE)
    with pytest.raises(mc.LimiterFatal):
        mc.plain_kw(c, kw)
    mixed = mc.with_fatal_level(mc.FATAL_CASE, 4, 9)
    with pytest.raises(mc.LimiterFatal) as ei:
        mc.plain_kw(c, mixed)
    assert ei.value.level == 4
    tame = {k: (np.delete(v, 4, axis=0) if isinstance(v, np.ndarray) and v.ndim == 2 and v.shape[0] == 9 else v) for k, v in mixed.items()}
    out, _ = mc.plain_kw(c, tame)                                    # the other eight levels are tame
    assert out.shape == (8, c["ndst"])
