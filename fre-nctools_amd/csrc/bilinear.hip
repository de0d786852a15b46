// bilinear.hip -- host orchestration of the bilinear plan (fg_bilin_*): setup_bilinear_interp's compute and READ branches
// (tools/fregrid/bilinear_interp.c:72-434) and do_scalar / do_vector_bilinear_interp (:436-560) on the device.
// At the end: fg_bilin_sweep, the field loop that streams levels in their file type through a plan.
// Kernels: bilinear_kernels.hip.  Host arithmetic that must round like the reference: bilinear_host.c, c2l_host.c.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>
#include "bilinear.h"
#include "fg_host.h"
#include "stream_slots.h"

extern "C" {
void fg_unit_vect_latlon(long size, const double *lon, const double *lat, double *vlon, double *vlat);
void fg_bilin_fine_grid(int nlon, int nlat, int finer_step, double lonbegin, double lonend, double latbegin, double latend,
                        int center_y, double *lont, double *latt, double *latt1d);
void fg_bilin_redu2x_coef(int ny, const double *ylat, double *cosp, double *acosp);
void fg_bilin_cell_dist(int N, long c0, long c1, const double *x, const double *y, const double *z, double *dist);
void fg_bilin_dist2side_tail(long n, const double *angle, const double *acos_arg, const double *side_cos, double *dist);
}

// host threads for the libm passes (bilinear_host.c); each processes [lo, hi) of an index range
template <typename F> static void bl_parallel(long n, F fn)
{
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
  if (n < 65536) nt = 1;
  std::vector<std::thread> w;
  const long chunk = (n + nt - 1) / nt;
  for (unsigned t = 1; t < nt; t++) {
    const long lo = t * chunk, hi = lo + chunk < n ? lo + chunk : n;
    if (lo < hi) w.emplace_back(fn, lo, hi);
  }
  fn(0L, chunk < n ? chunk : n);
  for (std::thread &x : w) x.join();
}

#define BL_MAX_ITER 10                    // setup_bilinear_interp's max_iter (:76)

struct fg_bilin {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int N = 0, nlon = 0, nlat = 0, finer_step = 0, nxo = 0, nyo = 0;
  long npts = 0, ncells = 0, F = 0;
  unsigned ambiguous_ties = 0;             // nearest-centre comparisons libm rounding could decide otherwise (search)
  std::vector<void *> owned;
  double *xt = nullptr, *lont = nullptr, *vlon_in = nullptr, *vlat_in = nullptr;   // xt holds xt | yt | zt; lont holds lont | latt
  double *xo = nullptr, *vlon_o = nullptr, *vlat_o = nullptr;                       // xo holds xo | yo | zo
  double *cell_dist = nullptr;                                                      // [ncells], see BlGeom
  int *cell_of = nullptr, *index = nullptr, *elem = nullptr, *cell = nullptr;
  double *weight = nullptr;
  std::vector<double *> cosp, acosp;       // per coarsening step, device
  double *ws = nullptr;                    // apply workspace
  size_t ws_cap = 0;
  template <typename T> T *alloc(size_t n)
  {
    void *p = nullptr;
    if (hipMalloc(&p, n * sizeof(T) + 16) != hipSuccess) return nullptr;
    owned.push_back(p);
    return (T *)p;
  }
  BlGeom geom() const
  {
    BlGeom g;
    g.N = N; g.nxo = nxo; g.nyo = nyo;
    g.xt = xt; g.yt = xt + F; g.zt = xt + 2 * F; g.lont = lont; g.latt = lont + F;
    g.xo = xo; g.yo = xo + npts; g.zo = xo + 2 * npts;
    g.cell_dist = cell_dist;
    return g;
  }
};

extern "C" void fg_bilin_destroy(fg_bilin *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->own_stream) (void)hipStreamDestroy(h->stream);
  for (void *p : h->owned) (void)hipFree(p);
  if (h->ws) (void)hipFree(h->ws);
  delete h;
}

template <typename T> static bool up(T *dst, const T *src, size_t n)
{
  return hipMemcpy(dst, src, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

// everything but the search: the halo'd source geometry, the fine lat-lon grid, the coarsening factors
static int bl_prepare(int ntiles, const int *nx, const int *ny, const double *const *lont, const double *const *latt, int ncontacts,
                      const int *tile1, const int *tile2, const int *istart1, const int *iend1, const int *jstart1, const int *jend1,
                      const int *istart2, const int *iend2, const int *jstart2, const int *jend2, int nlon, int nlat, int finer_step,
                      double lonbegin, double lonend, double latbegin, double latend, int center_y, int device, fg_bilin **out,
                      std::vector<double> *lat_fine_out)
{
  if (!out) return fg_fail(FG_ERR_ARG, "fg_bilin: null output handle");
  *out = nullptr;
  if (ntiles != 6) return fg_fail(FG_ERR_ARG, "bilinear_interp: source mosaic should be cubic mosaic and have six tiles when using bilinear option");
  if (ncontacts != 12) return fg_fail(FG_ERR_ARG, "bilinear_interp: a cubic mosaic has 12 contacts, got %d", ncontacts);
  if (finer_step < 0) return fg_fail(FG_ERR_ARG, "bilinear_interp: finer_step must be >= 0");
  if (nlat < 2) return fg_fail(FG_ERR_ARG, "bilinear_interp: nlat must be >= 2");
  if (nlon < 1 || finer_step > 10) return fg_fail(FG_ERR_ARG, "bilinear_interp: bad nlon / finer_step");
  if (!nx || !ny || !lont || !latt || !tile1 || !tile2) return fg_fail(FG_ERR_ARG, "fg_bilin: null argument");
  for (int t = 0; t < 6; t++)
    if (nx[t] != nx[0] || ny[t] != nx[0] || nx[t] < 2 || nx[t] > 8191 || !lont[t] || !latt[t])
      return fg_fail(FG_ERR_ARG, "bilinear_interp: the six tiles must be N x N with the same 2 <= N <= 8191");
  if (int rc = fg_use_device("fg_bilin", device)) return rc;

  const int N = nx[0], nxd = N + 2;
  const long T = (long)nxd * nxd, F = 6 * T, ncells = 6L * N * N;
  // halo map -> halo'd centres with init_halo's zero corners (fregrid_util.c:236-297), and the cell each element holds
  std::vector<long> map_off(7);
  std::vector<int> map(F);
  int rc = fg_halo_map(6, nx, ny, ncontacts, tile1, tile2, istart1, iend1, jstart1, jend1, istart2, iend2, jstart2, jend2,
                       map_off.data(), map.data());
  if (rc) return fg_fail(rc, "fregrid_util: inconsistent contact description (size mismatch between the boundary)");
  std::vector<double> lh(2 * F, 0.0);
  std::vector<int> cell_of(F, -1);
  for (int t = 0; t < 6; t++)
    for (int j = 0; j < N; j++) for (int i = 0; i < N; i++) {
      const long e = t * T + (long)(j + 1) * nxd + i + 1;
      lh[e] = lont[t][(long)j * N + i];
      lh[F + e] = latt[t][(long)j * N + i];
      cell_of[e] = (int)((long)t * N * N + (long)j * N + i);
    }
  for (long e = 0; e < F; e++)
    if (map[e] >= 0) { lh[e] = lh[map[e]]; lh[F + e] = lh[F + map[e]]; cell_of[e] = cell_of[map[e]]; }
  std::vector<double> xyz(3 * F), vlon(3 * F), vlat(3 * F);
  fg_latlon2xyz(F, lh.data(), lh.data() + F, xyz.data(), xyz.data() + F, xyz.data() + 2 * F);
  std::vector<double> cdist(ncells);
  bl_parallel(ncells, [&](long lo, long hi) { fg_bilin_cell_dist(N, lo, hi, xyz.data(), xyz.data() + F, xyz.data() + 2 * F, cdist.data()); });
  fg_unit_vect_latlon(F, lh.data(), lh.data() + F, vlon.data(), vlat.data());
  // fine lat-lon grid (get_output_grid_by_size, fregrid_util.c:564-641)
  const int nxo = (int)(pow(2, finer_step) * nlon), nyo = (int)(pow(2, finer_step) * (nlat - 1) + 1);
  const long npts = (long)nxo * nyo;
  std::vector<double> lo(npts), la(npts), la1(nyo), xo(3 * npts), vlo(3 * npts), vla(3 * npts);
  fg_bilin_fine_grid(nlon, nlat, finer_step, lonbegin, lonend, latbegin, latend, center_y, lo.data(), la.data(), la1.data());
  fg_latlon2xyz(npts, lo.data(), la.data(), xo.data(), xo.data() + npts, xo.data() + 2 * npts);
  fg_unit_vect_latlon(npts, lo.data(), la.data(), vlo.data(), vla.data());

  fg_bilin *h = new fg_bilin();
  h->device = device; h->N = N; h->nlon = nlon; h->nlat = nlat; h->finer_step = finer_step;
  h->nxo = nxo; h->nyo = nyo; h->npts = npts; h->ncells = ncells; h->F = F;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return fg_fail(FG_ERR_HIP, "hipStreamCreate failed"); }
  h->own_stream = true;
  h->xt = h->alloc<double>(3 * F); h->lont = h->alloc<double>(2 * F);
  h->vlon_in = h->alloc<double>(3 * F); h->vlat_in = h->alloc<double>(3 * F);
  h->xo = h->alloc<double>(3 * npts); h->vlon_o = h->alloc<double>(3 * npts); h->vlat_o = h->alloc<double>(3 * npts);
  h->cell_dist = h->alloc<double>(ncells);
  h->cell_of = h->alloc<int>(F); h->index = h->alloc<int>(3 * npts); h->weight = h->alloc<double>(4 * npts);
  h->elem = h->alloc<int>(4 * npts); h->cell = h->alloc<int>(4 * npts);
  bool ok = h->cell_dist && h->xt && h->lont && h->vlon_in && h->vlat_in && h->xo && h->vlon_o && h->vlat_o && h->cell_of && h->index &&
            h->weight && h->elem && h->cell;
  ok = ok && up(h->xt, xyz.data(), 3 * F) && up(h->lont, lh.data(), 2 * F) && up(h->vlon_in, vlon.data(), 3 * F) &&
       up(h->vlat_in, vlat.data(), 3 * F) && up(h->xo, xo.data(), 3 * npts) && up(h->vlon_o, vlo.data(), 3 * npts) &&
       up(h->vlat_o, vla.data(), 3 * npts) && up(h->cell_of, cell_of.data(), F) && up(h->cell_dist, cdist.data(), ncells);
  // coarsening factors per step (do_latlon_coarsening :994-1040): step 1 on the fine latitudes, later steps on -90..90
  int ny_s = nyo;
  for (int s = 1; s <= finer_step && ok; s++) {
    std::vector<double> c(ny_s), a(ny_s);
    fg_bilin_redu2x_coef(ny_s, s == 1 ? la1.data() : nullptr, c.data(), a.data());
    double *dc = h->alloc<double>(ny_s), *da = h->alloc<double>(ny_s);
    ok = dc && da && up(dc, c.data(), ny_s) && up(da, a.data(), ny_s);
    h->cosp.push_back(dc); h->acosp.push_back(da);
    ny_s = (ny_s - 1) / 2 + 1;
  }
  if (!ok) { fg_bilin_destroy(h); return fg_fail(FG_ERR_HIP, "fg_bilin: out of device memory or upload failed"); }
  if (lat_fine_out) *lat_fine_out = la1;
  *out = h;
  return 0;
}

// fregrid.c:944-963: the search's longitude / latitude span and origin
static void bl_span(double lonbegin, double lonend, double latbegin, double latend, double *dlon_in, double *dlat_in,
                    double *lonbegin_in, double *latbegin_in)
{
  const double D2R = M_PI / 180, EPSLN10 = 1.e-10;
  *dlon_in = (fabs(lonend - lonbegin - 360) < EPSLN10) ? M_PI + M_PI : (lonend - lonbegin) * D2R;
  *dlat_in = (fabs(latend - latbegin - 180) < EPSLN10) ? M_PI : (latend - latbegin) * D2R;
  *lonbegin_in = (fabs(lonbegin) < EPSLN10) ? 0.0 : lonbegin * D2R;
  *latbegin_in = (fabs(latbegin + 90) < EPSLN10) ? -0.5 * M_PI : latbegin * D2R;
}

extern "C" int fg_bilin_create(int ntiles, const int *nx, const int *ny, const double *const *lont, const double *const *latt,
                               int ncontacts, const int *tile1, const int *tile2, const int *istart1, const int *iend1,
                               const int *jstart1, const int *jend1, const int *istart2, const int *iend2, const int *jstart2,
                               const int *jend2, int nlon, int nlat, int finer_step, double lonbegin, double lonend,
                               double latbegin, double latend, int center_y, int device, fg_bilin **out)
{
  fg_bilin *h = nullptr;
  int rc = bl_prepare(ntiles, nx, ny, lont, latt, ncontacts, tile1, tile2, istart1, iend1, jstart1, jend1, istart2, iend2, jstart2,
                      jend2, nlon, nlat, finer_step, lonbegin, lonend, latbegin, latend, center_y, device, &h, nullptr);
  if (rc) return rc;
  double dlon_in, dlat_in, lonbegin_in, latbegin_in;
  bl_span(lonbegin, lonend, latbegin, latend, &dlon_in, &dlat_in, &lonbegin_in, &latbegin_in);
  const double dlon = dlon_in / h->nxo, dlat = dlat_in / (h->nyo - 1);
  const long ncell = h->ncells, nb = fgd_bl_scan_blocks(ncell);
  // search scratch
  BlWin *win = h->alloc<BlWin>(ncell);
  unsigned long long *cnt = h->alloc<unsigned long long>(ncell), *off = h->alloc<unsigned long long>(ncell);
  unsigned long long *bsum = h->alloc<unsigned long long>(nb + 1), *total = h->alloc<unsigned long long>(1);
  unsigned long long *key = h->alloc<unsigned long long>(h->npts);
  int *found = h->alloc<int>(h->npts);
  unsigned *unfound = h->alloc<unsigned>(BL_MAX_ITER + 2);      // [BL_MAX_ITER + 1]: ambiguous ties
  if (!win || !cnt || !off || !bsum || !total || !key || !found || !unfound) { fg_bilin_destroy(h); return fg_fail(FG_ERR_HIP, "fg_bilin: out of device memory"); }
  hipStream_t st = h->stream;
  bool ok = hipMemsetAsync(key, 0xff, h->npts * sizeof(unsigned long long), st) == hipSuccess &&
            hipMemsetAsync(found, 0, h->npts * sizeof(int), st) == hipSuccess &&
            hipMemsetAsync(unfound, 0, (BL_MAX_ITER + 2) * sizeof(unsigned), st) == hipSuccess &&
            hipMemsetAsync(h->index, 0, 3 * h->npts * sizeof(int), st) == hipSuccess;
  hipDeviceProp_t prop;
  int pair_blocks = 4096;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) pair_blocks = prop.multiProcessorCount * 16;
  const BlGeom g = h->geom();
  for (int iter = 1; iter <= BL_MAX_ITER && ok; iter++)
    fgd_bl_search_iter(g, iter, dlon, dlat, lonbegin_in, latbegin_in, unfound, win, cnt, off, bsum, total, found, key, h->index,
                       unfound + BL_MAX_ITER + 1, pair_blocks, st);
  unsigned left2[2] = {0, 0};
  ok = ok && hipGetLastError() == hipSuccess &&
       hipMemcpyAsync(left2, unfound + BL_MAX_ITER, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipStreamSynchronize(st) == hipSuccess;
  const unsigned left = left2[0];
  h->ambiguous_ties = left2[1];
  if (!ok) { fg_bilin_destroy(h); return fg_fail(FG_ERR_HIP, "fg_bilin: search kernels failed"); }
  if (left) {
    fg_bilin_destroy(h);
    return fg_fail(FG_ERR_BILIN_NOTFOUND, "bilinear_interp: %u lat-lon points have no lower-left corner after %d sweeps "
                   "(the reference would start its global sweep here, which reads past its arrays; not reproduced)", left, BL_MAX_ITER);
  }
  // weights: angles, acosl arguments and side cosines on the device, acosl / acos / sin / asin with the host libm, the
  // combination on the device
  {
    const long n4 = 4 * h->npts;
    double *dev = h->alloc<double>(3 * n4);
    std::vector<double> side(3 * n4), dist(n4);
    ok = dev != nullptr;
    if (ok) fgd_bl_weight_sides(g, h->index, dev, dev + n4, dev + 2 * n4, st);
    ok = ok && hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(side.data(), dev, 3 * n4 * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
    if (ok) bl_parallel(n4, [&](long lo, long hi) {
      fg_bilin_dist2side_tail(hi - lo, side.data() + lo, side.data() + n4 + lo, side.data() + 2 * n4 + lo, dist.data() + lo);
    });
    ok = ok && hipMemcpyAsync(dev, dist.data(), n4 * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) fgd_bl_weight_final(h->npts, h->N, h->index, dev, h->weight, st);
    if (ok) fgd_bl_corners(g, h->index, h->cell_of, h->elem, h->cell, st);
    ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    for (size_t k = 0; dev && k < h->owned.size(); k++) if (h->owned[k] == dev) { (void)hipFree(dev); h->owned.erase(h->owned.begin() + k); break; }
  }
  // the search scratch goes back at once
  for (void *p : {(void *)win, (void *)cnt, (void *)off, (void *)bsum, (void *)total, (void *)key, (void *)found, (void *)unfound}) {
    for (size_t k = 0; k < h->owned.size(); k++) if (h->owned[k] == p) { (void)hipFree(p); h->owned.erase(h->owned.begin() + k); break; }
  }
  if (!ok) { fg_bilin_destroy(h); return fg_fail(FG_ERR_HIP, "fg_bilin: weight kernel failed"); }
  *out = h;
  return 0;
}

extern "C" int fg_bilin_create_from_weights(int ntiles, const int *nx, const int *ny, const double *const *lont,
                                            const double *const *latt, int ncontacts, const int *tile1, const int *tile2,
                                            const int *istart1, const int *iend1, const int *jstart1, const int *jend1,
                                            const int *istart2, const int *iend2, const int *jstart2, const int *jend2, int nlon,
                                            int nlat, int finer_step, double lonbegin, double lonend, double latbegin, double latend,
                                            int center_y, const int *index, const double *weight, int device, fg_bilin **out)
{
  if (!index || !weight) return fg_fail(FG_ERR_ARG, "fg_bilin_create_from_weights: null index / weight");
  fg_bilin *h = nullptr;
  int rc = bl_prepare(ntiles, nx, ny, lont, latt, ncontacts, tile1, tile2, istart1, iend1, jstart1, jend1, istart2, iend2, jstart2,
                      jend2, nlon, nlat, finer_step, lonbegin, lonend, latbegin, latend, center_y, device, &h, nullptr);
  if (rc) return rc;
  for (long n = 0; n < h->npts; n++)                   // every corner read by the gather must lie in the halo'd tile
    if (index[3 * n] < 0 || index[3 * n] > h->N || index[3 * n + 1] < 0 || index[3 * n + 1] > h->N || index[3 * n + 2] < 0 ||
        index[3 * n + 2] > 5) {
      fg_bilin_destroy(h);
      return fg_fail(FG_ERR_ARG, "fg_bilin_create_from_weights: index of point %ld out of range", n);
    }
  if (!up(h->index, index, 3 * h->npts) || !up(h->weight, weight, 4 * h->npts)) { fg_bilin_destroy(h); return fg_fail(FG_ERR_HIP, "upload failed"); }
  fgd_bl_corners(h->geom(), h->index, h->cell_of, h->elem, h->cell, h->stream);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) { fg_bilin_destroy(h); return fg_fail(FG_ERR_HIP, "corner kernel failed"); }
  *out = h;
  return 0;
}

extern "C" int fg_bilin_get_index_weight(const fg_bilin *h, int *index, double *weight)
{
  if (!h) return fg_fail(FG_ERR_ARG, "null handle");
  FGCHK(hipSetDevice(h->device));
  FGCHK(hipStreamSynchronize(h->stream));
  if (index) FGCHK(hipMemcpy(index, h->index, 3 * h->npts * sizeof(int), hipMemcpyDeviceToHost));
  if (weight) FGCHK(hipMemcpy(weight, h->weight, 4 * h->npts * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" long fg_bilin_npoints_fine(const fg_bilin *h) { return h ? h->npts : FG_ERR_ARG; }
extern "C" int fg_bilin_nlon_fine(const fg_bilin *h) { return h ? h->nxo : FG_ERR_ARG; }
extern "C" int fg_bilin_nlat_fine(const fg_bilin *h) { return h ? h->nyo : FG_ERR_ARG; }
extern "C" int fg_bilin_nlon(const fg_bilin *h) { return h ? h->nlon : FG_ERR_ARG; }
extern "C" int fg_bilin_nlat(const fg_bilin *h) { return h ? h->nlat : FG_ERR_ARG; }
extern "C" long fg_bilin_ncells(const fg_bilin *h) { return h ? h->ncells : FG_ERR_ARG; }
extern "C" long fg_bilin_ambiguous_ties(const fg_bilin *h) { return h ? (long)h->ambiguous_ties : FG_ERR_ARG; }

extern "C" int fg_bilin_set_stream(fg_bilin *h, void *stream)
{
  if (!h) return fg_fail(FG_ERR_ARG, "null handle");
  FGCHK(hipSetDevice(h->device));
  FGCHK(hipStreamSynchronize(h->stream));
  if (h->own_stream) FGCHK(hipStreamDestroy(h->stream));
  h->stream = (hipStream_t)stream; h->own_stream = false;
  return 0;
}
extern "C" int fg_bilin_sync(fg_bilin *h)
{
  if (!h) return fg_fail(FG_ERR_ARG, "null handle");
  FGCHK(hipSetDevice(h->device));
  FGCHK(hipStreamSynchronize(h->stream));
  return 0;
}

static double *bl_workspace(fg_bilin *h, size_t n)
{
  if (n <= h->ws_cap) return h->ws;
  if (h->ws) { (void)hipStreamSynchronize(h->stream); (void)hipFree(h->ws); h->ws = nullptr; h->ws_cap = 0; }
  if (hipMalloc(&h->ws, n * sizeof(double)) != hipSuccess) { h->ws = nullptr; return nullptr; }
  h->ws_cap = n;
  return h->ws;
}

// do_latlon_coarsening (:994-1040) of nz levels: fine [nz][nyo][nxo] -> out [nz][nlat][nlon]; fine and b are scratch of the same
// size (overwritten), tmp holds nz * nyo * nxo / 2
static void bl_coarsen(fg_bilin *h, double *fine, double *b, double *tmp, int nz, int has_missing, double missing, double *out)
{
  int nx = h->nxo, ny = h->nyo;
  double *cur = fine, *other = b;
  for (int s = 1; s <= h->finer_step; s++) {
    double *dst = (s == h->finer_step) ? out : other;
    fgd_bl_redu2x(cur, nx, ny, nz, h->cosp[s - 1], h->acosp[s - 1], has_missing, missing, tmp, dst, h->stream);
    other = cur; cur = dst;
    nx = nx / 2; ny = (ny - 1) / 2 + 1;
  }
}

extern "C" int fg_bilin_apply_scalar(fg_bilin *h, const double *src, int nz, int has_missing, double missing, int fill_missing,
                                     double *out)
{
  if (!h || !src || !out || nz < 1) return fg_fail(FG_ERR_ARG, "fg_bilin_apply_scalar: bad argument");
  FGCHK(hipSetDevice(h->device));
  const size_t nf = (size_t)nz * h->npts;
  if (h->finer_step == 0) {
    fgd_bl_gather_scalar(h->npts, h->ncells, nz, h->cell, h->weight, src, has_missing, missing, fill_missing, out, h->stream);
  } else {
    double *ws = bl_workspace(h, 3 * nf);
    if (!ws) return fg_fail(FG_ERR_HIP, "fg_bilin_apply_scalar: out of device memory");
    fgd_bl_gather_scalar(h->npts, h->ncells, nz, h->cell, h->weight, src, has_missing, missing, fill_missing, ws, h->stream);
    bl_coarsen(h, ws, ws + nf, ws + 2 * nf, nz, has_missing, missing, out);
  }
  FGCHK(hipGetLastError());
  return 0;
}

extern "C" int fg_bilin_apply_vector(fg_bilin *h, const double *u, const double *v, int nz, int has_missing, double missing,
                                     int fill_missing, double *u_out, double *v_out)
{
  if (!h || !u || !v || !u_out || !v_out || nz < 1) return fg_fail(FG_ERR_ARG, "fg_bilin_apply_vector: bad argument");
  FGCHK(hipSetDevice(h->device));
  const size_t nf = (size_t)nz * h->npts;
  if (h->finer_step == 0) {
    fgd_bl_gather_vector(h->npts, h->ncells, nz, h->elem, h->cell, h->weight, h->vlon_in, h->vlat_in, h->vlon_o, h->vlat_o, u, v,
                         has_missing, missing, fill_missing, u_out, v_out, h->stream);
  } else {
    double *ws = bl_workspace(h, 4 * nf);
    if (!ws) return fg_fail(FG_ERR_HIP, "fg_bilin_apply_vector: out of device memory");
    fgd_bl_gather_vector(h->npts, h->ncells, nz, h->elem, h->cell, h->weight, h->vlon_in, h->vlat_in, h->vlon_o, h->vlat_o, u, v,
                         has_missing, missing, fill_missing, ws, ws + nf, h->stream);
    bl_coarsen(h, ws, ws + 2 * nf, ws + 3 * nf, nz, has_missing, missing, u_out);
    bl_coarsen(h, ws + nf, ws + 2 * nf, ws + 3 * nf, nz, has_missing, missing, v_out);
  }
  FGCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// fg_bilin_sweep: the field loop (include/fregrid_hip.h, "streamed bilinear fields").  fg_sweep's pipeline (sweep.hip) around
// the bilinear plan: levels travel in the file's type through NSLOT slots of CHUNK levels on a copy-in, a compute and a
// copy-out stream; events order the three, the host waits only when it wants a slot back.  One launch per chunk gathers,
// widens at the corners and narrows at the points (k_bl_stream_*); finer_step > 0 gathers into a double workspace shared by the
// chunks (the compute stream is in order) and narrows in the last coarsening step.  The object reads the plan's device arrays,
// which never change after the plan's creation, and launches on its own compute stream: the plan's stream is not touched, so
// sweeps may share a plan and either may be destroyed first.
using namespace fg_stream;
static_assert(CHUNK == BL_CHUNK, "the slots hold what one k_bl_stream_* launch takes");

struct fg_bilin_sweep {
  fg_bilin *plan = nullptr;
  int device = 0, in_type = FG_NC_DOUBLE, out_type = FG_NC_DOUBLE;
  size_t in_sz = 8, out_sz = 8;
  long ncells = 0, npts = 0, nout = 0;     // source cells, fine points and output points of one level
  hipStream_t s_in = nullptr, s_comp = nullptr, s_out = nullptr;
  double *ws = nullptr;                    // finer_step > 0: fine levels (two fields for vectors) | ping-pong | x-sweep
  size_t ws_cap = 0;
  struct Slot {
    void *d_raw[2] = {nullptr, nullptr}, *d_fin[2] = {nullptr, nullptr};     // [1]: the second component, on the first vector run
    void *pin_in[2] = {nullptr, nullptr}, *pin_out[2] = {nullptr, nullptr};  // staging for pageable user memory, on first need
    hipEvent_t e_in = nullptr, e_comp = nullptr, e_out = nullptr;
    bool busy = false, staged_out = false;
    long l0 = 0; int nl = 0;
  } slot[NSLOT];
};

extern "C" void fg_bilin_sweep_destroy(fg_bilin_sweep *sw)
{
  if (!sw) return;
  (void)hipSetDevice(sw->device);
  for (hipStream_t s : {sw->s_in, sw->s_comp, sw->s_out}) if (s) (void)hipStreamSynchronize(s);
  for (auto &sl : sw->slot) {                    // (the plan is not touched: it may be gone already)
    for (int c = 0; c < 2; c++) {
      if (sl.d_raw[c]) (void)hipFree(sl.d_raw[c]);
      if (sl.d_fin[c]) (void)hipFree(sl.d_fin[c]);
      if (sl.pin_in[c]) (void)hipHostFree(sl.pin_in[c]);
      if (sl.pin_out[c]) (void)hipHostFree(sl.pin_out[c]);
    }
    for (hipEvent_t e : {sl.e_in, sl.e_comp, sl.e_out}) if (e) (void)hipEventDestroy(e);
  }
  if (sw->ws) (void)hipFree(sw->ws);
  for (hipStream_t s : {sw->s_in, sw->s_comp, sw->s_out}) if (s) (void)hipStreamDestroy(s);
  delete sw;
}

extern "C" int fg_bilin_sweep_create(fg_bilin *h, int in_type, int out_type, fg_bilin_sweep **out)
{
  if (!h || !out) return fg_fail(FG_ERR_ARG, "fg_bilin_sweep_create: null argument");
  *out = nullptr;
  if (!type_size(in_type) || !type_size(out_type))
    return fg_fail(FG_ERR_ARG, "fg_bilin_sweep_create: types must be FG_NC_SHORT, FG_NC_INT, FG_NC_FLOAT or FG_NC_DOUBLE");
  if (int rc = fg_use_device("fg_bilin_sweep_create", h->device)) return rc;
  fg_bilin_sweep *sw = new fg_bilin_sweep();
  sw->plan = h; sw->device = h->device; sw->in_type = in_type; sw->out_type = out_type;
  sw->in_sz = type_size(in_type); sw->out_sz = type_size(out_type);
  sw->ncells = h->ncells; sw->npts = h->npts; sw->nout = (long)h->nlon * h->nlat;
  bool ok = hipStreamCreateWithFlags(&sw->s_in, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&sw->s_comp, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&sw->s_out, hipStreamNonBlocking) == hipSuccess;
  for (auto &sl : sw->slot) {
    ok = ok && hipMalloc(&sl.d_raw[0], (size_t)CHUNK * sw->ncells * sw->in_sz) == hipSuccess &&
         hipMalloc(&sl.d_fin[0], (size_t)CHUNK * sw->nout * sw->out_sz) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&sl.e_in, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&sl.e_comp, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&sl.e_out, hipEventDisableTiming) == hipSuccess;
  }
  if (!ok) { (void)hipGetLastError(); fg_bilin_sweep_destroy(sw); return fg_fail(FG_ERR_HIP, "fg_bilin_sweep_create: out of device memory (or stream / event creation failed)"); }
  *out = sw;
  return 0;
}

// The staging copy of a chunk between pageable user memory and a pinned slot, on up to four host threads: the chunks are tens
// of megabytes, one core copies them slower than the link moves them, and the host would then be what the pipeline waits for.
static void bls_copy(void *dst, const void *src, size_t bytes)
{
  const size_t piece_min = (size_t)4 << 20;
  unsigned hw = std::thread::hardware_concurrency();
  size_t nt = bytes / piece_min;
  nt = nt > 4 ? 4 : nt;
  if (hw && nt > hw) nt = hw;
  if (nt < 2) { memcpy(dst, src, bytes); return; }
  const size_t part = ((bytes + nt - 1) / nt + 63) & ~(size_t)63;
  std::vector<std::thread> w;
  for (size_t t = 1; t < nt; t++) {
    const size_t lo = t * part, n = lo >= bytes ? 0 : (bytes - lo < part ? bytes - lo : part);
    if (!n) break;
    try { w.emplace_back([=] { memcpy((char *)dst + lo, (const char *)src + lo, n); }); }
    catch (...) { memcpy((char *)dst + lo, (const char *)src + lo, n); }       // no thread to be had: this piece here
  }
  memcpy(dst, src, part < bytes ? part : bytes);
  for (std::thread &x : w) x.join();
}

// wait for a slot's chunk to be back on the host, then hand staged outputs to the user's pageable arrays
static int bls_retire(fg_bilin_sweep *sw, fg_bilin_sweep::Slot &sl, int ncomp, void *const *host_out)
{
  if (!sl.busy) return 0;
  FGCHK(hipEventSynchronize(sl.e_out));
  if (sl.staged_out)
    for (int c = 0; c < ncomp; c++)
      bls_copy((char *)host_out[c] + (size_t)sl.l0 * sw->nout * sw->out_sz, sl.pin_out[c], (size_t)sl.nl * sw->nout * sw->out_sz);
  sl.busy = false;
  return 0;
}

// ncomp 1: a scalar field (in[0], cv[0], out[0]); 2: the components u, v of a vector field
static int bls_run(fg_bilin_sweep *sw, const char *who, int ncomp, const void *const *in, long nlev, const fg_field_conv *const *cv,
                   int has_missing, int fill_missing, void *const *out)
{
  if (!sw || nlev < 1) return fg_fail(FG_ERR_ARG, "%s: null sweep or no level", who);
  for (int c = 0; c < ncomp; c++) if (!in[c] || !cv[c] || !out[c]) return fg_fail(FG_ERR_ARG, "%s: null argument", who);
  fg_bilin *h = sw->plan;
  FGCHK(hipSetDevice(sw->device));
  // On every way out -- errors included -- the three streams are drained and the slots cleared, so that a later run never
  // copies a failed run's staged outputs.
  struct Drain {
    fg_bilin_sweep *sw;
    ~Drain()
    {
      for (hipStream_t s : {sw->s_in, sw->s_comp, sw->s_out}) (void)hipStreamSynchronize(s);
      for (auto &sl : sw->slot) { sl.busy = false; sl.staged_out = false; }
    }
  } drain{sw};
  const size_t nin = (size_t)CHUNK * sw->ncells, nfin = (size_t)CHUNK * sw->nout, nf = (size_t)CHUNK * sw->npts;
  if (ncomp == 2)
    for (auto &sl : sw->slot) {
      if (!sl.d_raw[1]) FGCHK(hipMalloc(&sl.d_raw[1], nin * sw->in_sz));
      if (!sl.d_fin[1]) FGCHK(hipMalloc(&sl.d_fin[1], nfin * sw->out_sz));
    }
  const int fs = h->finer_step;
  if (fs > 0 && sw->ws_cap < (size_t)(ncomp + 2) * nf) {
    if (sw->ws) { (void)hipFree(sw->ws); sw->ws = nullptr; sw->ws_cap = 0; }      // (the streams are idle between runs)
    FGCHK(hipMalloc((void **)&sw->ws, (size_t)(ncomp + 2) * nf * sizeof(double)));
    sw->ws_cap = (size_t)(ncomp + 2) * nf;
  }
  bool in_pinned = true, out_pinned = true;
  for (int c = 0; c < ncomp; c++) { in_pinned = in_pinned && is_pinned(in[c]); out_pinned = out_pinned && is_pinned(out[c]); }
  BlConv conv[2], none = {0.0, 0.0, 0.0};
  for (int c = 0; c < ncomp; c++) conv[c] = {cv[c]->scale, cv[c]->offset, cv[c]->missing};
  const double missing = conv[0].missing;          // the interpolation's and the coarsening's: u's for a vector field
  BlStream a;
  a.npts = sw->npts; a.ncells = sw->ncells; a.nl = 0; a.elem = h->elem; a.cell = h->cell; a.weight = h->weight;
  a.vlon_in = h->vlon_in; a.vlat_in = h->vlat_in; a.vlon_out = h->vlon_o; a.vlat_out = h->vlat_o;
  a.has_missing = has_missing; a.fill_missing = fill_missing;
  long chunk = 0;
  for (long l0 = 0; l0 < nlev; l0 += CHUNK, chunk++) {
    const int nl = (int)((nlev - l0 < CHUNK) ? nlev - l0 : CHUNK);
    fg_bilin_sweep::Slot &sl = sw->slot[chunk % NSLOT];
    { int rc = bls_retire(sw, sl, ncomp, out); if (rc) return rc; }
    // --- upload (copy-in stream)
    const size_t bytes_in = (size_t)nl * sw->ncells * sw->in_sz;
    for (int c = 0; c < ncomp; c++) {
      const char *src = (const char *)in[c] + (size_t)l0 * sw->ncells * sw->in_sz;
      if (!in_pinned) {
        if (!sl.pin_in[c]) FGCHK(hipHostMalloc(&sl.pin_in[c], nin * sw->in_sz, hipHostMallocDefault));
        bls_copy(sl.pin_in[c], src, bytes_in);
        src = (const char *)sl.pin_in[c];
      }
      FGCHK(hipMemcpyAsync(sl.d_raw[c], src, bytes_in, hipMemcpyHostToDevice, sw->s_in));
    }
    FGCHK(hipEventRecord(sl.e_in, sw->s_in));
    // --- gather (widen at the corners, narrow at the points), coarsening (compute stream)
    FGCHK(hipStreamWaitEvent(sw->s_comp, sl.e_in, 0));
    a.nl = nl;
    if (fs == 0) {
      if (ncomp == 1) fgd_bl_stream_scalar(sw->in_type, sw->out_type, a, sl.d_raw[0], conv[0], conv[0], sl.d_fin[0], sw->s_comp);
      else fgd_bl_stream_vector(sw->in_type, sw->out_type, a, sl.d_raw[0], sl.d_raw[1], conv[0], conv[1], conv[0], conv[1], sl.d_fin[0],
                                sl.d_fin[1], sw->s_comp);
    } else {
      const size_t nfl = (size_t)nl * sw->npts;      // the chunk's levels lie back to back, as fg_bilin_apply_* lays them out
      double *fine[2] = {sw->ws, sw->ws + nfl}, *pong = sw->ws + (size_t)ncomp * nf, *tmp = pong + nf;
      if (ncomp == 1) fgd_bl_stream_scalar(sw->in_type, FG_NC_DOUBLE, a, sl.d_raw[0], conv[0], none, fine[0], sw->s_comp);
      else fgd_bl_stream_vector(sw->in_type, FG_NC_DOUBLE, a, sl.d_raw[0], sl.d_raw[1], conv[0], conv[1], none, none, fine[0], fine[1],
                                sw->s_comp);
      for (int c = 0; c < ncomp; c++) {              // do_latlon_coarsening (:994-1040), as bl_coarsen above
        int nx = h->nxo, ny = h->nyo;
        double *cur = fine[c], *other = pong;
        for (int s = 1; s <= fs; s++) {
          if (s < fs) {
            fgd_bl_redu2x(cur, nx, ny, nl, h->cosp[s - 1], h->acosp[s - 1], has_missing, missing, tmp, other, sw->s_comp);
            double *t = cur; cur = other; other = t;
          } else
            fgd_bl_redu2x_typed(sw->out_type, cur, nx, ny, nl, h->cosp[s - 1], h->acosp[s - 1], has_missing, missing, tmp, conv[c],
                                sl.d_fin[c], sw->s_comp);
          nx = nx / 2; ny = (ny - 1) / 2 + 1;
        }
      }
    }
    FGCHK(hipGetLastError());
    FGCHK(hipEventRecord(sl.e_comp, sw->s_comp));
    // --- download (copy-out stream)
    FGCHK(hipStreamWaitEvent(sw->s_out, sl.e_comp, 0));
    const size_t bytes_out = (size_t)nl * sw->nout * sw->out_sz;
    for (int c = 0; c < ncomp; c++) {
      if (!out_pinned && !sl.pin_out[c]) FGCHK(hipHostMalloc(&sl.pin_out[c], nfin * sw->out_sz, hipHostMallocDefault));
      char *dst = out_pinned ? (char *)out[c] + (size_t)l0 * sw->nout * sw->out_sz : (char *)sl.pin_out[c];
      FGCHK(hipMemcpyAsync(dst, sl.d_fin[c], bytes_out, hipMemcpyDeviceToHost, sw->s_out));
    }
    FGCHK(hipEventRecord(sl.e_out, sw->s_out));
    sl.busy = true; sl.l0 = l0; sl.nl = nl; sl.staged_out = !out_pinned;
  }
  // drain in chunk order
  for (long c = (chunk > NSLOT ? chunk - NSLOT : 0); c < chunk; c++) { int rc = bls_retire(sw, sw->slot[c % NSLOT], ncomp, out); if (rc) return rc; }
  return 0;
}

extern "C" int fg_bilin_sweep_run_scalar(fg_bilin_sweep *sw, const void *host_in, long nlev, const fg_field_conv *conv, int has_missing,
                                         int fill_missing, void *host_out)
{
  const void *in[1] = {host_in}; const fg_field_conv *cv[1] = {conv}; void *out[1] = {host_out};
  return bls_run(sw, "fg_bilin_sweep_run_scalar", 1, in, nlev, cv, has_missing, fill_missing, out);
}

extern "C" int fg_bilin_sweep_run_vector(fg_bilin_sweep *sw, const void *host_u, const void *host_v, long nlev, const fg_field_conv *conv_u,
                                         const fg_field_conv *conv_v, int has_missing, int fill_missing, void *host_u_out,
                                         void *host_v_out)
{
  const void *in[2] = {host_u, host_v}; const fg_field_conv *cv[2] = {conv_u, conv_v}; void *out[2] = {host_u_out, host_v_out};
  return bls_run(sw, "fg_bilin_sweep_run_vector", 2, in, nlev, cv, has_missing, fill_missing, out);
}
