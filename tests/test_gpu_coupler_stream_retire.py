"""A CouplerMosaic handle makes a stream of its own, runs its plans on it and destroys it with the handle.  Those plans give their
device blocks back to the pool tagged with the stream, and the pool keeps one ordering event per batch (csrc/dev_pool.h).  An event
that was recorded on a stream must not outlive the stream inside the pool: asked about such an event later (a search on another
stream that wants one of the blocks), the HIP runtime follows it to the destroyed stream and has answered "operation not permitted
when stream is capturing", which the next search of the process then met as its own error.  fg_coupler_destroy retires the stream
in the pool first: afterwards the pool holds no more events than before the handle existed, and a search sized by counting --
the one that asks the pool for many blocks again -- runs clean."""
import ctypes as C

import numpy as np
import pytest

import coupler_cases as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("clip_method", ["legacy", "great_circle"])
def test_no_event_of_the_handles_stream_stays_in_the_pool(fg, gpu_ok, clip_method):
    L = fg.lib()
    L.fg_pool_live_events.restype = C.c_long
    c = cc.case_c(fg, 0.5)
    L.fg_pool_release()                                         # an empty pool: no cached block, no event
    before = L.fg_pool_live_events()
    assert before == 0
    with fg.CouplerMosaic(c["atm"], None, c["ocn"], c["omask"], interp_order=1, clip_method=clip_method) as m:
        m.run()
        held = L.fg_pool_live_events()
    assert held > before                                        # (the runs' plans did leave sealed batches behind: the test has an object)
    assert L.fg_pool_live_events() == 0
    lo, la = fg.latlon_corners(36, 18)
    L.fg_set_search_mode(1)                                     # capacities by counting: a repeated attempt takes its blocks from the pool again
    try:
        p = fg.XgridPlan.create(1, c["atm"], fg.GridConfig(36, 18, lo, la))
        assert p.nxgrid > 0
        p.destroy()
    finally:
        L.fg_set_search_mode(0)
