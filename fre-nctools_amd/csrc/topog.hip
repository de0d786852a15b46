// topog.hip -- host orchestration of make_topog's realistic topography on the device (fg_topog_*): create_realistic_topog
// (tools/make_topog/topog.c:355-549) with filter_topo (:687) and process_topo (:551) on arrays the caller has read from the
// topography file and the model grid.  Kernels: topog_kernels.hip; arithmetic: topog.h; design: DESIGN.md 3.12.
//
// The host does what is O(nx + ny): the source's axis bounds, the row trim (with the extremes of the destination latitudes, one
// pass over the caller's array), p_cell_min, the checks of zw.  The source's 2-D corner arrays, its depth and mask, the remap (a
// first-order plan made by the device entries of plan.hip, then the area-fraction sweep), the filter passes, kmt / ht with their
// halo, remove_isolated_cells (in the last kernel, or as the in-place sweep by anti-diagonals), and the last adjustments stay in device memory; the
// depth is read back by fg_topog_get alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <memory>
#include <vector>
#include "topog.h"
#include "fg_host.h"
#include "plan_internal.h"

// 1 (default, the faster one: profiles/topog_summary.md): remove_isolated_cells for every cell at once in the last kernel;
// 0: as the reference's sequential sweep, one launch per anti-diagonal.  Same results.
static std::atomic<int> g_sweep_fused{1};
extern "C" void fg_set_topog_sweep(int fused) { g_sweep_fused = fused ? 1 : 0; }

struct fg_topog {
  int device = 0, nx = 0, ny = 0;
  long n = 0;
  fg_topog_opts o;
  hipStream_t stream = nullptr;
  FgDev dev;                                  // what lives as long as the handle
  std::unique_ptr<FgDev> src;                 // what a source owns: replaced by the next fg_topog_set_source
  double y_min = 0, y_max = 0;
  double *d_xout = nullptr, *d_yout = nullptr;
  double *d_depth[2] = {nullptr, nullptr}, *d_rmask = nullptr, *d_ht = nullptr, *d_partial = nullptr;
  int *d_kmt = nullptr, *d_levels = nullptr;
  TpCounts *d_cnt = nullptr;
  int cur = 0;                                // which of d_depth holds the depth
  // the source
  int nx_src = 0, ny_src = 0, ny_now = 0, jstart = 0, jend = 0;
  double missing = 0;
  double *d_xsrc = nullptr, *d_ysrc = nullptr, *d_depth_src = nullptr, *d_mask_src = nullptr;
  bool have_source = false, have_depth = false, have_levels = false;
  long nxgrid = -1, launches = 0;
  TpCounts cnt = {0, 0, 0, 0};
  double deepest = 0;
  int verdict = -1;
  float ms[5] = {0, 0, 0, 0, 0};              // create; set_source; remap; filter; process
};

extern "C" void fg_topog_default_opts(fg_topog_opts *o)
{
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->scale_factor = 1;                        // make_topog.c:297-323
  o->num_filter_pass = 1;
  o->adjust_topo = 1;
  o->fill_isolated_cells = 1;
  o->kmt_min = 2;
  o->min_thickness = 0.1;
  o->open_very_this_cell = 1;
  o->fraction_full_cell = 0.2;
}

extern "C" void fg_topog_destroy(fg_topog *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    fg_pool_retire_stream(h->stream);             // the remap's plan ran on this stream (dev_pool.h: retire)
    (void)hipStreamDestroy(h->stream);
  }
  delete h;
}

extern "C" void *fg_topog_stream(fg_topog *h) { return h ? (void *)h->stream : nullptr; }

extern "C" int fg_topog_create(int nx_dst, int ny_dst, const double *x_dst, const double *y_dst, const fg_topog_opts *opts, int device, fg_topog **out)
{
  if (!out) return fg_fail(FG_ERR_ARG, "fg_topog_create: null output handle");
  *out = nullptr;
  if (nx_dst < 1 || ny_dst < 1 || (double)(nx_dst + 2) * (ny_dst + 2) > 0x3fffffff || !x_dst || !y_dst)
    return fg_fail(FG_ERR_ARG, "fg_topog_create: bad model grid argument");
  fg_topog *h = new fg_topog;
  struct Guard { fg_topog *&h; bool keep = false; ~Guard() { if (!keep) fg_topog_destroy(h); } } guard{h};
  h->device = device; h->nx = nx_dst; h->ny = ny_dst; h->n = (long)nx_dst * ny_dst;
  if (opts) h->o = *opts; else fg_topog_default_opts(&h->o);
  if (h->o.num_filter_pass < 0) return fg_fail(FG_ERR_ARG, "fg_topog_create: num_filter_pass %d is negative", h->o.num_filter_pass);
  const long np = (long)(nx_dst + 1) * (ny_dst + 1);
  // :431-438 the extremes of the destination latitudes in radians, in the reference's order of comparisons
  h->y_min = h->y_max = y_dst[0] * TP_D2R;
  for (long i = 1; i < np; i++) {
    const double y = y_dst[i] * TP_D2R;
    if (y < h->y_min) h->y_min = y;
    if (y > h->y_max) h->y_max = y;
  }
  if (int rc = fg_use_device("fg_topog_create", device)) return rc;
  const double t0 = fg_now_ms();
  FGCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  FgDev &dev = h->dev;
  FgDev tmp;
  const double *d_xdeg = tmp.put(x_dst, np), *d_ydeg = tmp.put(y_dst, np);
  h->d_xout = dev.get<double>(np); h->d_yout = dev.get<double>(np);
  h->d_depth[0] = dev.get<double>(h->n); h->d_depth[1] = dev.get<double>(h->n); h->d_rmask = dev.get<double>(h->n);
  const long nh = (long)(nx_dst + 2) * (ny_dst + 2);
  h->d_ht = dev.get<double>(nh); h->d_kmt = dev.get<int>(nh); h->d_levels = dev.get<int>(h->n);
  h->d_partial = dev.get<double>(TP_REDUCE_BLOCKS + 1); h->d_cnt = dev.get<TpCounts>(1);
  if (!d_xdeg || !d_ydeg || !h->d_xout || !h->d_yout || !h->d_depth[0] || !h->d_depth[1] || !h->d_rmask || !h->d_ht || !h->d_kmt || !h->d_levels ||
      !h->d_partial || !h->d_cnt)
    return fg_fail(FG_ERR_HIP, "fg_topog_create: device allocation or upload failed");
  fgd_tp_scale(np, d_xdeg, d_ydeg, h->d_xout, h->d_yout, h->stream);
  FGCHK(hipGetLastError());
  FGCHK(hipStreamSynchronize(h->stream));
  h->ms[0] = (float)(fg_now_ms() - t0);
  guard.keep = true;
  *out = h;
  return 0;
}

extern "C" int fg_topog_set_source(fg_topog *h, int nx_src, int ny_src, const double *xt_src, const double *yt_src, const void *data, int dtype,
                                   double missing)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_topog_set_source: null handle");
  if (nx_src < 1 || ny_src < 1 || (double)(nx_src + 1) * (ny_src + 1) > 0x3fffffff || !xt_src || !yt_src || !data)
    return fg_fail(FG_ERR_ARG, "fg_topog_set_source: bad source argument");
  if (dtype != TP_NC_DOUBLE && dtype != TP_NC_FLOAT && dtype != TP_NC_INT)
    return fg_fail(FG_ERR_ARG, "topog.c: nc_type should be NC_DOUBLE, NC_FLOAT or NC_INT");
  FGCHK(hipSetDevice(h->device));
  const double t0 = fg_now_ms();
  h->have_source = false; h->have_depth = false; h->have_levels = false; h->nxgrid = -1;
  std::vector<double> xc(nx_src + 1), yc(ny_src + 1);
  tp_axis_bounds(nx_src, xt_src, xc.data());
  tp_axis_bounds(ny_src, yt_src, yc.data());
  int jstart, jend;
  tp_trim(ny_src, yc.data(), h->y_min, h->y_max, &jstart, &jend);
  const int ny_now = jend - jstart + 1;
  if (ny_now < 1) return fg_fail(FG_ERR_ARG, "fg_topog_set_source: no source row lies within the model grid's latitudes");
  if (h->o.on_grid && (long)nx_src * ny_now != h->n)
    return fg_fail(FG_ERR_ARG, "fg_topog_set_source: on_grid needs %ld source cells after the row trim, the source has %d x %d", h->n, nx_src, ny_now);
  FGCHK(hipStreamSynchronize(h->stream));
  h->src.reset(new FgDev);
  FgDev &s = *h->src;
  const long nsrc = (long)nx_src * ny_now, npsrc = (long)(nx_src + 1) * (ny_now + 1);
  const size_t esz = dtype == TP_NC_DOUBLE ? 8 : 4;
  const double *d_xc = s.put(xc), *d_yc = s.put(yc.data() + jstart, (size_t)ny_now + 1);
  const char *d_raw = s.put((const char *)data + (size_t)jstart * nx_src * esz, (size_t)nsrc * esz);       // the rows :467-469 read, in the file's type
  h->d_xsrc = s.get<double>(npsrc); h->d_ysrc = s.get<double>(npsrc);
  h->d_depth_src = s.get<double>(nsrc); h->d_mask_src = s.get<double>(nsrc);
  if (!d_xc || !d_yc || !d_raw || !h->d_xsrc || !h->d_ysrc || !h->d_depth_src || !h->d_mask_src)
    return fg_fail(FG_ERR_HIP, "fg_topog_set_source: device allocation or upload failed");
  fgd_tp_expand(nx_src + 1, ny_now + 1, d_xc, d_yc, h->d_xsrc, h->d_ysrc, h->stream);
  fgd_tp_prepare(nsrc, d_raw, dtype, missing, h->o.scale_factor, h->d_depth_src, h->d_mask_src, h->stream);
  FGCHK(hipGetLastError());
  FGCHK(hipStreamSynchronize(h->stream));
  h->nx_src = nx_src; h->ny_src = ny_src; h->ny_now = ny_now; h->jstart = jstart; h->jend = jend; h->missing = missing;
  h->have_source = true;
  h->ms[1] = (float)(fg_now_ms() - t0);
  return 0;
}

extern "C" int fg_topog_get_source(const fg_topog *h, double *x_src, double *y_src, double *depth_src, double *mask_src)
{
  if (!h || !h->have_source) return fg_fail(FG_ERR_ARG, "fg_topog_get_source: no source on this handle");
  FGCHK(hipSetDevice(h->device));
  const size_t nsrc = (size_t)h->nx_src * h->ny_now, npsrc = (size_t)(h->nx_src + 1) * (h->ny_now + 1);
  if (x_src) FGCHK(hipMemcpy(x_src, h->d_xsrc, npsrc * sizeof(double), hipMemcpyDeviceToHost));
  if (y_src) FGCHK(hipMemcpy(y_src, h->d_ysrc, npsrc * sizeof(double), hipMemcpyDeviceToHost));
  if (depth_src) FGCHK(hipMemcpy(depth_src, h->d_depth_src, nsrc * sizeof(double), hipMemcpyDeviceToHost));
  if (mask_src) FGCHK(hipMemcpy(mask_src, h->d_mask_src, nsrc * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

static int tp_remap(fg_topog *h)
{
  if (!h->have_source) return fg_fail(FG_ERR_ARG, "fg_topog_remap: fg_topog_set_source has not been called on this handle");
  const double t0 = fg_now_ms();
  h->have_levels = false;
  if (h->o.on_grid) {
    fgd_tp_ongrid(h->n, h->d_depth_src, h->missing, h->d_depth[h->cur], h->stream);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(h->stream));
    h->nxgrid = 0;
  } else {
    const double *lons[1] = {h->d_xsrc}, *lats[1] = {h->d_ysrc}, *masks[1] = {h->d_mask_src};
    fg_plan *pl = nullptr;
    const long nx = h->o.use_great_circle_algorithm
      ? fg_plan_create_great_circle_lonlat_dev(1, &h->nx_src, &h->ny_now, lons, lats, masks, h->nx, h->ny, h->d_xout, h->d_yout, 0, 0, h->device,
                                               h->stream, 1, &pl)
      : fg_plan_create_dev(FG_CONSERVE_ORDER1, 1, &h->nx_src, &h->ny_now, lons, lats, masks, h->nx, h->ny, h->d_xout, h->d_yout, 0, 0, h->device,
                           h->stream, 1, &pl);
    if (nx < 0) return (int)nx;                                     // the message is the plan's (a source too large for one plan among them)
    int rc = fg_plan_finalize(pl, nullptr);
    if (!rc) rc = fg_plan_apply_frac_dev(pl, h->d_depth_src, h->d_depth[h->cur]);
    fg_plan_destroy(pl);
    if (rc) return rc;
    h->nxgrid = nx;
  }
  h->have_depth = true;
  h->ms[2] = (float)(fg_now_ms() - t0);
  return 0;
}

static int tp_deepest(fg_topog *h, int nk, const double *zw)
{
  fgd_tp_deepest(h->n, h->d_depth[h->cur], h->d_partial, h->d_partial + TP_REDUCE_BLOCKS, h->stream);
  FGCHK(hipGetLastError());
  FGCHK(hipMemcpyAsync(&h->deepest, h->d_partial + TP_REDUCE_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  FGCHK(hipStreamSynchronize(h->stream));
  h->verdict = -1;
  if (nk > 0 && zw) {                                               // show_deepest :964-979
    if ((h->deepest - zw[nk - 1]) > 1.0) h->verdict = 0;
    else if (nk > 1 && h->deepest <= zw[nk - 2]) h->verdict = 1;
    else h->verdict = 2;
  }
  return 0;
}

static int tp_filter(fg_topog *h)
{
  if (!h->have_depth) return fg_fail(FG_ERR_ARG, "fg_topog_filter: the handle holds no depth (fg_topog_remap or fg_topog_set_depth first)");
  const double t0 = fg_now_ms();
  h->have_levels = false;
  fgd_tp_rmask(h->n, h->d_depth[h->cur], h->d_rmask, h->stream);
  if (h->nx >= 3 && h->ny >= 3)
    for (int p = 0; p < h->o.num_filter_pass; p++) {
      fgd_tp_filter(h->nx, h->ny, h->d_depth[h->cur], h->d_rmask, h->o.smooth_topo_allow_deepening, h->d_depth[h->cur ^ 1], h->stream);
      h->cur ^= 1;
    }
  FGCHK(hipGetLastError());
  FGCHK(hipStreamSynchronize(h->stream));
  h->ms[3] = (float)(fg_now_ms() - t0);
  return 0;
}

static int tp_check_vgrid(const fg_topog *h, int nk, const double *zw)
{
  if (nk < 1 || !zw) return fg_fail(FG_ERR_ARG, "fg_topog_process: nk >= 1 levels and zw are required");
  for (int k = 1; k < nk; k++) if (zw[k] < zw[k - 1]) return fg_fail(FG_ERR_ARG, "nearest_index: array must be monotonically increasing");
  if (h->o.adjust_topo) {
    if (nk < h->o.kmt_min) return fg_fail(FG_ERR_ARG, "topog: number of vertical cells=%d, is less than kmt_min=%d", nk, h->o.kmt_min);
    if (h->o.kmt_min < 1) return fg_fail(FG_ERR_ARG, "fg_topog_process: kmt_min %d is less than 1 (the reference would read zw[-1])", h->o.kmt_min);
    if ((h->o.round_shallow != 0) + (h->o.fill_shallow != 0) + (h->o.deepen_shallow != 0) > 1)
      return fg_fail(FG_ERR_ARG, "topog: at most one of round_shallow/deepen_shallow/fill_shallow can be set to true");
  }
  return 0;
}

static int tp_process(fg_topog *h, int nk, const double *zw)
{
  if (!h->have_depth) return fg_fail(FG_ERR_ARG, "fg_topog_process: the handle holds no depth (fg_topog_remap or fg_topog_set_depth first)");
  if (int rc = tp_check_vgrid(h, nk, zw)) return rc;
  const double t0 = fg_now_ms();
  const fg_topog_opts &o = h->o;
  const int ni = h->nx, nj = h->ny;
  const long nh = (long)(ni + 2) * (nj + 2);
  FgDev t;
  std::vector<double> pc(nk);
  tp_p_cell_min(nk, zw, o.fraction_full_cell, o.min_thickness, pc.data());
  const double *d_zw = t.put(zw, (size_t)nk), *d_pc = t.put(pc);
  if (!d_zw || !d_pc) return fg_fail(FG_ERR_HIP, "fg_topog_process: device allocation or upload failed");
  hipStream_t st = h->stream;
  FGCHK(hipMemsetAsync(h->d_cnt, 0, sizeof(TpCounts), st));
  FGCHK(hipMemsetAsync(h->d_ht, 0, nh * sizeof(double), st));              // :574-577: ht = 0
  FGCHK(hipMemsetAsync(h->d_kmt, 0xff, nh * sizeof(int), st));             //           kmt = -1
  fgd_tp_kmt(ni, nj, nk, d_zw, h->d_depth[h->cur], o.min_thickness, o.full_cell, o.flat_bottom, h->d_ht, h->d_kmt, st);
  if (o.tripolar_grid || o.cyclic_y) fgd_tp_halo_y(ni, nj, o.tripolar_grid, h->d_ht, h->d_kmt, st);
  if (o.cyclic_x) fgd_tp_halo_x(ni, nj, h->d_ht, h->d_kmt, st);
  h->launches = 0;
  const int nj_max = o.tripolar_grid ? nj - 1 : nj, fill = o.adjust_topo && o.fill_isolated_cells, fused = g_sweep_fused;
  if (fill && !fused) h->launches = fgd_tp_isolated(ni, nj_max, o.dont_change_landmask, h->d_ht, h->d_kmt, h->d_cnt, st);
  fgd_tp_finish(ni, nj, nk, d_zw, d_pc, h->d_ht, h->d_kmt, fill && fused ? nj_max : 0, o.dont_change_landmask, o.adjust_topo, o.open_very_this_cell, o.kmt_min, o.round_shallow, o.deepen_shallow,
                o.fill_shallow, h->d_depth[h->cur], h->d_levels, h->d_cnt, st);
  FGCHK(hipGetLastError());
  FGCHK(hipMemcpyAsync(&h->cnt, h->d_cnt, sizeof(TpCounts), hipMemcpyDeviceToHost, st));
  FGCHK(hipStreamSynchronize(st));
  h->have_levels = true;
  h->ms[4] = (float)(fg_now_ms() - t0);
  return 0;
}

extern "C" int fg_topog_remap(fg_topog *h)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_topog_remap: null handle");
  FGCHK(hipSetDevice(h->device));
  return tp_remap(h);
}

extern "C" int fg_topog_filter(fg_topog *h)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_topog_filter: null handle");
  FGCHK(hipSetDevice(h->device));
  if (int rc = tp_filter(h)) return rc;
  return tp_deepest(h, 0, nullptr);
}

extern "C" int fg_topog_process(fg_topog *h, int nk, const double *zw)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_topog_process: null handle");
  FGCHK(hipSetDevice(h->device));
  return tp_process(h, nk, zw);
}

// :512-536
extern "C" int fg_topog_run(fg_topog *h, int nk, const double *zw)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_topog_run: null handle");
  if (nk < 0 || (nk > 0 && !zw)) return fg_fail(FG_ERR_ARG, "fg_topog_run: nk levels need zw");
  FGCHK(hipSetDevice(h->device));
  if (nk > 0) if (int rc = tp_check_vgrid(h, nk, zw)) return rc;       // before any work, the reference after the remap: the same error
  if (int rc = tp_remap(h)) return rc;
  h->ms[3] = h->ms[4] = 0;
  if (h->o.filter_topog) if (int rc = tp_filter(h)) return rc;
  if (int rc = tp_deepest(h, nk, zw)) return rc;
  if (h->o.fill_first_row) {
    fgd_tp_zero_row(h->nx, h->d_depth[h->cur], h->stream);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(h->stream));
  }
  if (nk > 0) return tp_process(h, nk, zw);
  return 0;
}

extern "C" int fg_topog_set_depth(fg_topog *h, const double *depth)
{
  if (!h || !depth) return fg_fail(FG_ERR_ARG, "fg_topog_set_depth: bad argument");
  FGCHK(hipSetDevice(h->device));
  FGCHK(hipStreamSynchronize(h->stream));
  FGCHK(hipMemcpy(h->d_depth[h->cur], depth, h->n * sizeof(double), hipMemcpyHostToDevice));
  h->have_depth = true; h->have_levels = false;
  return 0;
}

extern "C" int fg_topog_get(const fg_topog *h, double *depth, int *num_levels)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_topog_get: null handle");
  if (!h->have_depth) return fg_fail(FG_ERR_ARG, "fg_topog_get: the handle holds no depth");
  if (num_levels && !h->have_levels) return fg_fail(FG_ERR_ARG, "fg_topog_get: no levels: fg_topog_process has not run on this depth");
  FGCHK(hipSetDevice(h->device));
  FGCHK(hipStreamSynchronize(h->stream));
  if (depth) FGCHK(hipMemcpy(depth, h->d_depth[h->cur], h->n * sizeof(double), hipMemcpyDeviceToHost));
  if (num_levels) FGCHK(hipMemcpy(num_levels, h->d_levels, h->n * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int fg_topog_stats(const fg_topog *h, long *s, double *deepest, int n)
{
  if (!h || !s || n < 0) return fg_fail(FG_ERR_ARG, "fg_topog_stats: bad argument");
  const long v[9] = {h->jstart, h->jend, h->nxgrid, (long)h->cnt.isolated, (long)h->cnt.partial, (long)h->cnt.shallow, h->verdict, h->launches, h->ny_now};
  for (int k = 0; k < n && k < 9; k++) s[k] = v[k];
  if (deepest) *deepest = h->deepest;
  return 0;
}

extern "C" int fg_topog_phase_ms(const fg_topog *h, float *ms, int n)
{
  if (!h || !ms || n < 0) return fg_fail(FG_ERR_ARG, "fg_topog_phase_ms: bad argument");
  for (int k = 0; k < n && k < 5; k++) ms[k] = h->ms[k];
  return 0;
}
