"""The hand-made exchange lists of tests/sweep_cases.py on the host: every case meets what its profile claims
(check_preconditions), and the reference's do_scalar_conserve_interp (oracle/_ref/libconserve_ref.so) gives on them, bit for bit,
what the plain float64 loop in list order gives -- unsorted lists, pairs listed twice, zero areas, rows of zero areas only, values
over sixteen decades.  The sweep calls no libm, so the comparison needs no tolerance and does not depend on orc.host_has_fma()."""
import numpy as np
import pytest

import orc
import sweep_cases as sc

needs_ref = pytest.mark.skipif(not orc.conserve_ref_available(), reason="oracle/_ref/libconserve_ref.so not built")
EX_CASES = [(n, o, opt) for n in ("spike-804", "eights-804", "long-201") for o in (1, 2) for opt in sc.EX_OPTS[:4]] + \
           [(n + "-1t", 2, opt) for n in ("spike-804", "eights-804", "long-201") for opt in sc.EX_OPTS[4:]]


@pytest.mark.parametrize("name", sc.CASES)
def test_preconditions(name):
    assert sc.check_preconditions(sc.make(name))


def test_cases_are_functions_of_their_names():
    a = sc.make("short-99")
    sc.make.cache_clear()
    b = sc.make("short-99")
    assert a is not b
    for k in ("t_in", "i_in", "j_in", "i_out", "j_out", "area", "di", "dj"):
        assert np.array_equal(a["x"][k], b["x"][k])
    assert sc.same(a["vals"], b["vals"]) and np.array_equal(a["miss"], b["miss"])


@needs_ref
@pytest.mark.parametrize("name", sc.CASES)
def test_reference_equals_plain(name):
    c = sc.make(name)
    for order in (1, 2):
        for masked in (False, True):
            ref, mine = sc.reference(c, order, masked), sc.plain(c, order, masked)
            bad = np.argwhere(sc.bits(ref) != sc.bits(mine))
            assert bad.size == 0, (order, masked, bad[:5].tolist())


@needs_ref
@pytest.mark.parametrize("name,order,opt", EX_CASES, ids=[f"{n}-order{o}-{opt}" for n, o, opt in EX_CASES])
def test_reference_equals_plain_with_options(name, order, opt):
    c = sc.make(name)
    ref, mine = sc.reference_ex(c, order, opt), sc.plain_ex(c, order, opt)
    assert sc.same(ref, mine), np.nonzero(sc.bits(ref) != sc.bits(mine))[0][:5].tolist()
    miss = ref == sc.ex_inputs(c, order, opt)["missing"]
    assert np.any(miss) and np.any(~miss)
    if not opt.startswith("mono"):
        assert np.count_nonzero(sc.bits(ref) == 0) >= 2              # rows at 0.0 by the "touched" rule
