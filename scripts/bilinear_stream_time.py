"""Times of the streamed bilinear field loop (fg_bilin_sweep) against the per-level chain it replaces.

  C384 -> 1440 x 721 (finer_step 0) and C384 -> 720 x 361 at finer_step 1 (fine 1440 x 721), 50 NC_FLOAT levels in and out,
  a scalar field and a vector field, from page-locked (fg_host_alloc) and from pageable host arrays:
      chain     per level and component: fg_dev_upload, fg_dev_widen, fg_bilin_apply_scalar / _vector(nz = 1), fg_dev_narrow,
                fg_dev_download -- entry points the parent commit has; the plan runs on the null stream, so the chain needs no
                synchronise of its own beyond those inside the conversions and the copies
      streamed  fg_bilin_sweep_run_scalar / _vector
  The streamed outputs are asserted bit-identical to the chain's before anything is timed.  Device events around each leg after
  a warm-up; the legs alternate; the median, the best and the worst round are printed, one JSON line per workload.

  --part kernels runs a few repetitions of one chunk of 8 levels both ways -- the resident kernels k_widen, k_bl_gather_*,
  (k_redu2x_*,) k_narrow and the streamed k_bl_stream_* (k_redu2x_x, k_redu2x_y_typed) -- for a kernel trace:
      rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bilinear_stream_time.py --part kernels

  python scripts/bilinear_stream_time.py [--part time|kernels] [--rounds N] [--nlev N] [--ni N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MISSING = float(np.float32(-1.0e20))
WORKLOADS = [("fs0_1440x721", 1440, 721, 0), ("fs1_720x361", 720, 361, 1)]


def make_plan(fg, ni, nlon, nlat, fs):
    lonc, latc, lont, latt = fg.gnomonic_ed_grid(ni)
    contacts = fg.find_contacts([ni] * 6, [ni] * 6, list(lonc), list(latc))
    lont = [np.asarray(a).reshape(ni, ni) for a in lont]
    latt = [np.asarray(a).reshape(ni, ni) for a in latt]
    plan = fg.BilinearPlan(lont, latt, contacts, nlon, nlat, finer_step=fs)
    plan.set_stream(0)                              # the null stream: ordered with fg_dev_widen / fg_dev_narrow
    return plan, np.stack(lont).reshape(-1), np.stack(latt).reshape(-1)


def fields(lo, la, nlev):
    """winds and a scalar as a history file holds them: NC_FLOAT, a few missing cells on every level"""
    k = np.arange(nlev, dtype=np.float64)[:, None]
    s = (10.0 * np.sin(lo + la + 0.3 * k) + 3.0 * np.cos(2.0 * la) + k).astype(np.float32)
    u = (20.0 * np.cos(la) + 5.0 * np.sin(2.0 * lo + k)).astype(np.float32)
    v = (8.0 * np.sin(lo - 0.2 * k) * np.cos(la) + 0.0 * k).astype(np.float32)
    for a in (s, u):
        a[:, ::37] = MISSING
    return s, u, v


class Chain:
    """the per-level chain on device buffers of one level"""

    def __init__(self, fg, torch, plan, ncomp):
        self.L, self.plan, self.ncomp = fg.lib(), plan, ncomp
        self.n_in, self.n_out = plan.ncells, plan.nlat * plan.nlon
        dev = "cuda:0"
        mk = lambda n, dt: [torch.empty(n, dtype=dt, device=dev) for _ in range(ncomp)]
        self.raw, self.f64 = mk(self.n_in, torch.float32), mk(self.n_in, torch.float64)
        self.res, self.fin = mk(self.n_out, torch.float64), mk(self.n_out, torch.float32)
        self.nc_float = fg.field_io.nc_type_of(np.float32)

    def level(self, ins, outs, k):
        L, vp, z, m = self.L, C.c_void_p, C.c_double(0.0), C.c_double(MISSING)
        for c in range(self.ncomp):
            L.fg_dev_upload(vp(self.raw[c].data_ptr()), vp(ins[c][k].ctypes.data), self.n_in * 4)
            L.fg_dev_widen(C.c_int(self.nc_float), C.c_long(self.n_in), vp(self.raw[c].data_ptr()), z, z, m, vp(self.f64[c].data_ptr()))
        if self.ncomp == 1:
            rc = L.fg_bilin_apply_scalar(self.plan._h, vp(self.f64[0].data_ptr()), 1, 1, MISSING, 0, vp(self.res[0].data_ptr()))
        else:
            rc = L.fg_bilin_apply_vector(self.plan._h, vp(self.f64[0].data_ptr()), vp(self.f64[1].data_ptr()), 1, 1, MISSING, 0,
                                         vp(self.res[0].data_ptr()), vp(self.res[1].data_ptr()))
        assert rc == 0
        for c in range(self.ncomp):
            L.fg_dev_narrow(C.c_int(self.nc_float), C.c_long(self.n_out), vp(self.res[c].data_ptr()), z, z, m, vp(self.fin[c].data_ptr()))
            L.fg_dev_download(vp(outs[c][k].ctypes.data), vp(self.fin[c].data_ptr()), self.n_out * 4)

    def run(self, ins, outs):
        for k in range(ins[0].shape[0]):
            self.level(ins, outs, k)


def streamed(sw, ins, outs):
    if len(ins) == 1:
        sw.run_scalar(ins[0], outs[0], missing=MISSING, has_missing=True)
    else:
        sw.run_vector(ins[0], ins[1], outs[0], outs[1], conv_u=(0.0, 0.0, MISSING), conv_v=(0.0, 0.0, MISSING), has_missing=True)


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(torch, legs, rounds):
    for fn in legs.values():
        fn()
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t[k].append(event_ms(torch, fn))
    return {k: dict(median=round(statistics.median(v), 3), best=round(min(v), 3), worst=round(max(v), 3)) for k, v in t.items()}


def host_arrays(fg, srcs, n_out, pinned, keep):
    def arr(shape, fill=None):
        if pinned:
            hb = fg.HostBuffer(shape, np.float32); keep.append(hb); a = hb.array
        else:
            a = np.empty(shape, dtype=np.float32)
        if fill is not None:
            a[...] = fill
        return a
    nlev = srcs[0].shape[0]
    return [arr(s.shape, s) for s in srcs], [arr((nlev, n_out)) for _ in srcs], [arr((nlev, n_out)) for _ in srcs]


def time_part(fg, torch, a):
    for wname, nlon, nlat, fs in WORKLOADS:
        plan, lo, la = make_plan(fg, a.ni, nlon, nlat, fs)
        s, u, v = fields(lo, la, a.nlev)
        sw = plan.sweep(np.float32, np.float32)
        for kind, srcs in (("scalar", [s]), ("vector", [u, v])):
            chain = Chain(fg, torch, plan, len(srcs))
            for pinned in (True, False):
                keep = []
                ins, o_chain, o_stream = host_arrays(fg, srcs, nlon * nlat, pinned, keep)
                chain.run(ins, o_chain); streamed(sw, ins, o_stream)
                same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(o_chain, o_stream))
                assert same, (wname, kind, pinned)
                res = alternate(torch, {"per_level_chain": lambda: chain.run(ins, o_chain), "streamed": lambda: streamed(sw, ins, o_stream)},
                                a.rounds)
                mb = lambda arrs: round(sum(x.nbytes for x in arrs) / 1e6, 1)
                print(json.dumps({"workload": f"C{a.ni} -> {nlon}x{nlat} finer_step {fs}", "field": kind, "levels": a.nlev,
                                  "host": "page-locked" if pinned else "pageable", "unit": "ms per run (device events)",
                                  "rounds": a.rounds, "MB_in": mb(ins), "MB_out": mb(o_stream), **res,
                                  "speedup_median": round(res["per_level_chain"]["median"] / res["streamed"]["median"], 2),
                                  "bits_equal_to_chain": same}), flush=True)
                ins = o_chain = o_stream = None
                for hb in keep:
                    hb.free()
        sw.destroy(); plan.destroy()


def kernels_part(fg, torch, a):
    """one chunk of 8 levels, resident kernels and streamed kernels, a few times each: for rocprofv3 --kernel-trace --stats"""
    L, vp, nl, dev = fg.lib(), C.c_void_p, 8, "cuda:0"
    nc_float = fg.field_io.nc_type_of(np.float32)
    z, m = C.c_double(0.0), C.c_double(MISSING)
    for wname, nlon, nlat, fs in WORKLOADS:
        plan, lo, la = make_plan(fg, a.ni, nlon, nlat, fs)
        s, u, v = fields(lo, la, nl)
        n_in, n_out = nl * plan.ncells, nl * nlon * nlat
        raw = [torch.from_numpy(x).to(dev) for x in (u, v)]
        f64 = [torch.empty(n_in, dtype=torch.float64, device=dev) for _ in range(2)]
        res = [torch.empty(n_out, dtype=torch.float64, device=dev) for _ in range(2)]
        fin = [torch.empty(n_out, dtype=torch.float32, device=dev) for _ in range(2)]
        sw = plan.sweep(np.float32, np.float32)
        keep = []
        ins, _, outs = host_arrays(fg, [u, v], nlon * nlat, True, keep)
        for _ in range(a.rounds):
            for c in range(2):
                L.fg_dev_widen(C.c_int(nc_float), C.c_long(n_in), vp(raw[c].data_ptr()), z, z, m, vp(f64[c].data_ptr()))
            L.fg_bilin_apply_scalar(plan._h, vp(f64[0].data_ptr()), nl, 1, MISSING, 0, vp(res[0].data_ptr()))
            L.fg_bilin_apply_vector(plan._h, vp(f64[0].data_ptr()), vp(f64[1].data_ptr()), nl, 1, MISSING, 0, vp(res[0].data_ptr()),
                                    vp(res[1].data_ptr()))
            for c in range(2):
                L.fg_dev_narrow(C.c_int(nc_float), C.c_long(n_out), vp(res[c].data_ptr()), z, z, m, vp(fin[c].data_ptr()))
            streamed(sw, ins[:1], outs[:1])
            streamed(sw, ins, outs)
        torch.cuda.synchronize()
        print(json.dumps({"part": "kernels", "workload": wname, "chunk_levels": nl, "rounds": a.rounds}), flush=True)
        ins = outs = None
        for hb in keep:
            hb.free()
        sw.destroy(); plan.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="time", choices=["time", "kernels"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--nlev", type=int, default=50)
    ap.add_argument("--ni", type=int, default=384)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    fg = g.load_package()
    fg._lib.require_gpu()
    (time_part if a.part == "time" else kernels_part)(fg, torch, a)


if __name__ == "__main__":
    main()
