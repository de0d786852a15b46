// runoff.hip -- host orchestration of runoff_regrid on the device (fg_runoff_*, fg_nearest_unmasked): setup_remap
// (tools/runoff_regrid/runoff_regrid.c:430-539) and the arithmetic of process_data (:626-675).  Kernels: runoff_kernels.hip.
//
// Setup: the 1dx2d order-1 exchange list through the box search (plan.hip), the nearest ocean point of every land point of
// the output grid (exact), and two stable counting sorts on the host: the exchange list by destination cell,
// the land points by their ocean target.  A time level is then three launches without atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <vector>
#include "runoff.h"
#include "fg_host.h"

long fg_box_xgrid_lists(int dev, int box_is_src, int order, int nxb, int nyb, const double *lon_b, const double *lat_b,
                        int nxq, int nyq, const double *lon_q, const double *lat_q, const double *mask,
                        std::vector<int> idx[4], std::vector<double> &area, std::vector<double> *clon, std::vector<double> *clat);

static std::atomic<int> g_prune{1};
extern "C" void fg_set_runoff_prune(int on) { g_prune = on ? 1 : 0; }
extern "C" int fg_runoff_tile(void) { return RO_TILE; }

// nearest() for nq points of the grid itself.  d_xyz: the converted points [3][n] on the device.  stats (may be null):
// queries, tiles, tiles visited in all, most tiles visited by one query.
static int ro_search(hipStream_t st, int nlon, int nlat, const double *mask, const double *d_xyz, int nq, const int *qindex,
                     int *iout, int *jout, long *stats, float *kernel_ms)
{
  const long n = (long)nlon * nlat;
  std::vector<int> oidx, orank(n + 1);
  for (long i = 0; i < n; i++) { orank[i] = (int)oidx.size(); if (!(mask[i] == 0.0)) oidx.push_back((int)i); }   // :717
  orank[n] = (int)oidx.size();
  const int nocean = (int)oidx.size();
  if (stats) { stats[0] = nq; stats[1] = stats[2] = stats[3] = 0; }
  if (nocean == 0) return fg_fail(FG_ERR_ARG, "fg_runoff: mask has no ocean point (every value is 0): there is nothing to map the land points to");
  if (nq < 1) return 0;
  const RoTiles tl = ro_tiles_of(nocean);
  const int ntiles = tl.ntiles, ngroups = tl.ngroups;
  FgDev dev;
  int *d_oidx = dev.put(oidx.data(), oidx.size()), *d_orank = dev.put(orank.data(), orank.size()), *d_q = dev.put(qindex, (size_t)nq);
  RoPoint *d_pts = dev.get<RoPoint>((size_t)ntiles * RO_TILE);
  RoBall *d_ball = dev.get<RoBall>(ntiles), *d_gball = dev.get<RoBall>(ngroups);
  int *d_out = dev.get<int>(3 * (size_t)nq);
  if (!d_oidx || !d_orank || !d_q || !d_pts || !d_ball || !d_gball || !d_out) return fg_fail(FG_ERR_HIP, "fg_runoff: device allocation or upload failed");
  fgd_ro_tiles(nocean, d_oidx, d_xyz, d_xyz + n, d_xyz + 2 * n, d_pts, d_ball, d_gball, st);
  RoSearch p;
  p.x = d_xyz; p.y = d_xyz + n; p.z = d_xyz + 2 * n;
  p.pts = d_pts; p.ball = d_ball; p.gball = d_gball; p.orank = d_orank; p.qindex = d_q;
  p.iout = d_out; p.jout = d_out + nq; p.visited = d_out + 2 * (size_t)nq;
  p.n = (int)n; p.nlon = nlon; p.nq = nq; p.ntiles = ntiles; p.ngroups = ngroups;
  p.r0 = ro_r0();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kernel_ms) { FGCHK(hipEventCreate(&e0)); FGCHK(hipEventCreate(&e1)); FGCHK(hipEventRecord(e0, st)); }
  fgd_ro_nearest(p, g_prune, st);
  FGCHK(hipGetLastError());
  if (kernel_ms) FGCHK(hipEventRecord(e1, st));
  std::vector<int> out(3 * (size_t)nq);
  FGCHK(hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  FGCHK(hipStreamSynchronize(st));
  if (kernel_ms) { FGCHK(hipEventElapsedTime(kernel_ms, e0, e1)); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); }
  memcpy(iout, out.data(), (size_t)nq * sizeof(int));
  memcpy(jout, out.data() + nq, (size_t)nq * sizeof(int));
  if (stats) {
    stats[1] = ntiles;
    for (int q = 0; q < nq; q++) { const long v = out[2 * (size_t)nq + q]; stats[2] += v; if (v > stats[3]) stats[3] = v; }
  }
  return 0;
}

static int ro_check_grid(const char *who, int nlon, int nlat, const double *mask, const double *lon, const double *lat)
{
  if (nlon < 1 || nlat < 1 || (long)nlon * nlat > 0x7fffffffL / RO_TILE) return fg_fail(FG_ERR_ARG, "%s: bad grid size %d x %d", who, nlon, nlat);
  if (!mask || !lon || !lat) return fg_fail(FG_ERR_ARG, "%s: null grid argument", who);
  return 0;
}

extern "C" int fg_nearest_unmasked(int nlon, int nlat, const double *mask, const double *lon, const double *lat, int nq,
                                   const int *qindex, int *iout, int *jout)
{
  int rc = ro_check_grid("fg_nearest_unmasked", nlon, nlat, mask, lon, lat);
  if (rc) return rc;
  const long n = (long)nlon * nlat;
  if (nq < 0 || (nq > 0 && (!qindex || !iout || !jout))) return fg_fail(FG_ERR_ARG, "fg_nearest_unmasked: bad query arguments");
  for (int q = 0; q < nq; q++) if (qindex[q] < 0 || qindex[q] >= n) return fg_fail(FG_ERR_ARG, "fg_nearest_unmasked: query %d (%d) is outside the grid", q, qindex[q]);
  rc = fg_use_device("fg_nearest_unmasked", fg_env_device());
  if (rc) return rc;
  FgDev dev;
  double *d_ll = dev.get<double>(2 * (size_t)n), *d_xyz = dev.get<double>(3 * (size_t)n);
  if (!d_ll || !d_xyz) return fg_fail(FG_ERR_HIP, "fg_nearest_unmasked: out of device memory");
  FGCHK(hipMemcpy(d_ll, lon, n * sizeof(double), hipMemcpyHostToDevice));
  FGCHK(hipMemcpy(d_ll + n, lat, n * sizeof(double), hipMemcpyHostToDevice));
  fgd_ro_xyz(n, d_ll, d_ll + n, d_xyz, d_xyz + n, d_xyz + 2 * n, nullptr);
  return ro_search(nullptr, nlon, nlat, mask, d_xyz, nq, qindex, iout, jout, nullptr, nullptr);
}

struct fg_runoff {
  int device = 0, nx_in = 0, ny_in = 0, nx_out = 0, ny_out = 0;
  hipStream_t stream = nullptr;
  FgDev dev;
  double *d_xyz = nullptr, *d_tmp = nullptr, *d_totals = nullptr;
  RoApply a;
  std::vector<int> xi[4];                    // i_in, j_in, i_out, j_out
  std::vector<double> xarea;
  std::vector<int> imap, jmap;
  long stats[4] = {0, 0, 0, 0};
  float ms[5] = {0, 0, 0, 0, 0};             // setup: exchange list, conversion, nearest search, its kernel alone, sorts + uploads
};

extern "C" void fg_runoff_destroy(fg_runoff *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  delete h;
}

// everything but the exchange list: the points, the maps, the inverted map, the sorted list
static int ro_setup(fg_runoff *h, const double *mask_in, const double *area_in, const double *xt, const double *yt,
                    const double *mask_out, const double *area_out)
{
  const int nx = h->nx_out, ny = h->ny_out;
  const long n = (long)nx * ny, n_in = (long)h->nx_in * h->ny_in, nxg = (long)h->xarea.size();
  FGCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  FgDev &dev = h->dev;
  h->d_xyz = dev.get<double>(3 * (size_t)n);
  h->d_tmp = dev.get<double>((size_t)n);
  h->d_totals = dev.get<double>(2);
  if (!h->d_xyz || !h->d_tmp || !h->d_totals) return fg_fail(FG_ERR_HIP, "fg_runoff: out of device memory");
  double t0 = fg_now_ms();
  {
    FgDev t;
    double *d_lon = t.put(xt, (size_t)n), *d_lat = t.put(yt, (size_t)n);
    if (!d_lon || !d_lat) return fg_fail(FG_ERR_HIP, "fg_runoff: grid upload failed");
    fgd_ro_xyz(n, d_lon, d_lat, h->d_xyz, h->d_xyz + n, h->d_xyz + 2 * n, h->stream);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(h->stream));
  }
  std::vector<int> qindex;
  for (long i = 0; i < n; i++) if (mask_out[i] == 0.0) qindex.push_back((int)i);             // :517
  const int nq = (int)qindex.size();
  std::vector<int> qi(nq), qj(nq);
  double t1 = fg_now_ms();
  h->ms[1] = (float)(t1 - t0);
  int rc = ro_search(h->stream, nx, ny, mask_out, h->d_xyz, nq, qindex.data(), qi.data(), qj.data(), h->stats, &h->ms[3]);
  if (rc) return rc;
  t0 = fg_now_ms();
  h->ms[2] = (float)(t0 - t1);
  h->imap.assign(n, -1); h->jmap.assign(n, -1);
  for (int q = 0; q < nq; q++) { h->imap[qindex[q]] = qi[q]; h->jmap[qindex[q]] = qj[q]; }
  // land points by target, ascending within a target (the order the reference's loop over l adds them in)
  std::vector<int> tptr(n + 1, 0), tsrc;
  std::vector<unsigned char> land(n, 0);
  long nmapped = 0;
  for (int q = 0; q < nq; q++) if (qi[q] >= 0) { tptr[(long)qj[q] * nx + qi[q] + 1]++; land[qindex[q]] = 1; nmapped++; }
  for (long c = 0; c < n; c++) tptr[c + 1] += tptr[c];
  tsrc.resize(nmapped);
  {
    std::vector<int> fill(tptr.begin(), tptr.end() - 1);
    for (int q = 0; q < nq; q++) if (qi[q] >= 0) tsrc[fill[(long)qj[q] * nx + qi[q]]++] = qindex[q];
  }
  // the exchange list by destination cell, list order kept within a cell
  std::vector<int> rowptr(n + 1, 0), src(nxg);
  std::vector<double> xa(nxg);
  for (long l = 0; l < nxg; l++) {
    const int i1 = h->xi[0][l], j1 = h->xi[1][l], i2 = h->xi[2][l], j2 = h->xi[3][l];
    if (i1 < 0 || i1 >= h->nx_in || j1 < 0 || j1 >= h->ny_in || i2 < 0 || i2 >= nx || j2 < 0 || j2 >= ny)
      return fg_fail(FG_ERR_ARG, "fg_runoff: exchange entry %ld lies outside the grids", l);
    rowptr[(long)j2 * nx + i2 + 1]++;
  }
  for (long c = 0; c < n; c++) rowptr[c + 1] += rowptr[c];
  {
    std::vector<int> fill(rowptr.begin(), rowptr.end() - 1);
    for (long l = 0; l < nxg; l++) {
      const int k = fill[(long)h->xi[3][l] * nx + h->xi[2][l]]++;
      src[k] = h->xi[1][l] * h->nx_in + h->xi[0][l];
      xa[k] = h->xarea[l];
    }
  }
  RoApply &a = h->a;
  a.rowptr = dev.put(rowptr.data(), rowptr.size()); a.src = dev.put(src.data(), src.size()); a.xarea = dev.put(xa.data(), xa.size());
  a.tptr = dev.put(tptr.data(), tptr.size()); a.tsrc = dev.put(tsrc.data(), tsrc.size()); a.land = dev.put(land.data(), land.size());
  a.area_out = dev.put(area_out, (size_t)n); a.area_in = dev.put(area_in, (size_t)n_in); a.mask_in = dev.put(mask_in, (size_t)n_in);
  a.ncell_out = (int)n; a.ncell_in = (int)n_in;
  if (!a.rowptr || !a.src || !a.xarea || !a.tptr || !a.tsrc || !a.land || !a.area_out || !a.area_in || !a.mask_in)
    return fg_fail(FG_ERR_HIP, "fg_runoff: device allocation or upload failed");
  h->ms[4] = (float)(fg_now_ms() - t0);
  return 0;
}

static int ro_new(const char *who, int nx_in, int ny_in, int nx_out, int ny_out, const double *xt, const double *yt,
                  const double *mask_out, const double *area_out, int device, fg_runoff **out, fg_runoff **h)
{
  if (!out) return fg_fail(FG_ERR_ARG, "%s: null output handle", who);
  *out = nullptr;
  if (nx_in < 1 || ny_in < 1 || (long)nx_in * ny_in > 0x7fffffffL) return fg_fail(FG_ERR_ARG, "%s: bad input grid size", who);
  int rc = ro_check_grid(who, nx_out, ny_out, mask_out, xt, yt);
  if (rc) return rc;
  if (!area_out) return fg_fail(FG_ERR_ARG, "%s: null area_out", who);
  long nocean = 0;
  for (long i = 0; i < (long)nx_out * ny_out; i++) nocean += !(mask_out[i] == 0.0);
  if (nocean == 0) return fg_fail(FG_ERR_ARG, "%s: mask_out has no ocean point (every value is 0): there is nothing to map the land points to", who);
  rc = fg_use_device(who, device);
  if (rc) return rc;
  *h = new fg_runoff;
  (*h)->device = device; (*h)->nx_in = nx_in; (*h)->ny_in = ny_in; (*h)->nx_out = nx_out; (*h)->ny_out = ny_out;
  return 0;
}

extern "C" int fg_runoff_create_from_xgrid(int nx_in, int ny_in, const double *mask_in, const double *area_in, int nx_out, int ny_out,
                                           const double *xt, const double *yt, const double *mask_out, const double *area_out,
                                           long nxgrid, const int *i_in, const int *j_in, const int *i_out, const int *j_out,
                                           const double *xgrid_area, int device, fg_runoff **out)
{
  fg_runoff *h = nullptr;
  int rc = ro_new("fg_runoff_create_from_xgrid", nx_in, ny_in, nx_out, ny_out, xt, yt, mask_out, area_out, device, out, &h);
  if (rc) return rc;
  if (!mask_in || !area_in || nxgrid < 0 || (nxgrid > 0 && (!i_in || !j_in || !i_out || !j_out || !xgrid_area))) {
    fg_runoff_destroy(h);
    return fg_fail(FG_ERR_ARG, "fg_runoff_create_from_xgrid: null argument");
  }
  const int *lists[4] = {i_in, j_in, i_out, j_out};
  for (int k = 0; k < 4; k++) h->xi[k].assign(lists[k], lists[k] + nxgrid);
  h->xarea.assign(xgrid_area, xgrid_area + nxgrid);
  rc = ro_setup(h, mask_in, area_in, xt, yt, mask_out, area_out);
  if (rc) { fg_runoff_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" int fg_runoff_create(int nx_in, int ny_in, const double *lonb_in, const double *latb_in, const double *mask_in,
                                int nx_out, int ny_out, const double *xc, const double *yc, const double *xt, const double *yt,
                                const double *mask_out, const double *area_out, int device, fg_runoff **out)
{
  fg_runoff *h = nullptr;
  int rc = ro_new("fg_runoff_create", nx_in, ny_in, nx_out, ny_out, xt, yt, mask_out, area_out, device, out, &h);
  if (rc) return rc;
  if (!lonb_in || !latb_in || !mask_in || !xc || !yc) { fg_runoff_destroy(h); return fg_fail(FG_ERR_ARG, "fg_runoff_create: null argument"); }
  const double t0 = fg_now_ms();
  // setup_remap :472: the box grid is the source, the list comes back as (box i, box j, quad i, quad j) = (i_in, j_in, i_out, j_out)
  const long nx = fg_box_xgrid_lists(device, 1, FG_CONSERVE_ORDER1, nx_in, ny_in, lonb_in, latb_in, nx_out, ny_out, xc, yc, mask_in,
                                     h->xi, h->xarea, nullptr, nullptr);
  if (nx < 0) { fg_runoff_destroy(h); return (int)nx; }
  // get_input_grid :290-295: the input cell areas from the expanded corner arrays
  std::vector<double> cx((size_t)(nx_in + 1) * (ny_in + 1)), cy(cx.size()), area_in((size_t)nx_in * ny_in);
  for (int j = 0; j <= ny_in; j++) for (int i = 0; i <= nx_in; i++) { cx[(size_t)j * (nx_in + 1) + i] = lonb_in[i]; cy[(size_t)j * (nx_in + 1) + i] = latb_in[j]; }
  const double dl[4] = {0, 0.01, 0, 0.01}, da[4] = {0, 0, 0.01, 0.01};
  const double *lons[1] = {cx.data()}, *lats[1] = {cy.data()};
  fg_plan *pl = nullptr;
  long prc = fg_plan_create(FG_CONSERVE_ORDER1, 1, &nx_in, &ny_in, lons, lats, nullptr, 1, 1, dl, da, device, &pl);
  if (prc >= 0) prc = fg_plan_get_cell_area(pl, area_in.data(), nullptr);
  if (pl) fg_plan_destroy(pl);
  if (prc < 0) { fg_runoff_destroy(h); return (int)prc; }
  h->ms[0] = (float)(fg_now_ms() - t0);
  rc = ro_setup(h, mask_in, area_in.data(), xt, yt, mask_out, area_out);
  if (rc) { fg_runoff_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" long fg_runoff_nxgrid(const fg_runoff *h) { return h ? (long)h->xarea.size() : FG_ERR_ARG; }
extern "C" void *fg_runoff_stream(fg_runoff *h) { return h ? (void *)h->stream : nullptr; }

extern "C" int fg_runoff_get_xgrid(const fg_runoff *h, int *i_in, int *j_in, int *i_out, int *j_out, double *xgrid_area)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_runoff_get_xgrid: null handle");
  int *dst[4] = {i_in, j_in, i_out, j_out};
  for (int k = 0; k < 4; k++) if (dst[k]) memcpy(dst[k], h->xi[k].data(), h->xi[k].size() * sizeof(int));
  if (xgrid_area) memcpy(xgrid_area, h->xarea.data(), h->xarea.size() * sizeof(double));
  return 0;
}

extern "C" int fg_runoff_get_maps(const fg_runoff *h, int *imap, int *jmap)
{
  if (!h || !imap || !jmap) return fg_fail(FG_ERR_ARG, "fg_runoff_get_maps: null argument");
  memcpy(imap, h->imap.data(), h->imap.size() * sizeof(int));
  memcpy(jmap, h->jmap.data(), h->jmap.size() * sizeof(int));
  return 0;
}

extern "C" int fg_runoff_get_xyz(fg_runoff *h, double *x, double *y, double *z)
{
  if (!h || !x || !y || !z) return fg_fail(FG_ERR_ARG, "fg_runoff_get_xyz: null argument");
  const size_t n = (size_t)h->nx_out * h->ny_out;
  FGCHK(hipSetDevice(h->device));
  FGCHK(hipMemcpy(x, h->d_xyz, n * sizeof(double), hipMemcpyDeviceToHost));
  FGCHK(hipMemcpy(y, h->d_xyz + n, n * sizeof(double), hipMemcpyDeviceToHost));
  FGCHK(hipMemcpy(z, h->d_xyz + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int fg_runoff_search_stats(const fg_runoff *h, long *stats)
{
  if (!h || !stats) return fg_fail(FG_ERR_ARG, "fg_runoff_search_stats: null argument");
  memcpy(stats, h->stats, sizeof h->stats);
  return 0;
}

extern "C" int fg_runoff_phase_ms(const fg_runoff *h, float *ms, int n)
{
  if (!h || !ms || n < 0) return fg_fail(FG_ERR_ARG, "fg_runoff_phase_ms: bad argument");
  for (int k = 0; k < n && k < 5; k++) ms[k] = h->ms[k];
  return 0;
}

extern "C" int fg_runoff_apply_dev(fg_runoff *h, const double *d_in, double *d_out, double *totals)
{
  if (!h || !d_in || !d_out) return fg_fail(FG_ERR_ARG, "fg_runoff_apply_dev: null argument");
  if (d_in == d_out) return fg_fail(FG_ERR_ARG, "fg_runoff_apply_dev: in and out must be different arrays");
  FGCHK(hipSetDevice(h->device));
  fgd_ro_apply(h->a, d_in, h->d_tmp, d_out, h->d_totals, h->stream);
  FGCHK(hipGetLastError());
  if (totals) {
    FGCHK(hipMemcpyAsync(totals, h->d_totals, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    FGCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

extern "C" int fg_runoff_apply(fg_runoff *h, const double *in, double *out, double *totals)
{
  if (!h || !in || !out) return fg_fail(FG_ERR_ARG, "fg_runoff_apply: null argument");
  FGCHK(hipSetDevice(h->device));
  const size_t n_in = (size_t)h->nx_in * h->ny_in, n = (size_t)h->nx_out * h->ny_out;
  FgDev t;
  double *d_in = t.put(in, n_in), *d_out = t.get<double>(n);
  if (!d_in || !d_out) return fg_fail(FG_ERR_HIP, "fg_runoff_apply: device allocation or upload failed");
  double tot[2];
  int rc = fg_runoff_apply_dev(h, d_in, d_out, tot);                 // synchronises the handle's stream
  if (rc) return rc;
  FGCHK(hipMemcpy(out, d_out, n * sizeof(double), hipMemcpyDeviceToHost));
  if (totals) { totals[0] = tot[0]; totals[1] = tot[1]; }
  return 0;
}
