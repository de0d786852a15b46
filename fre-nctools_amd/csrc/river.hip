// river.hip -- host orchestration of river_regrid on the device (fg_river_*): calc_max_subA, calc_tocell, calc_river_data,
// sort_basin and check_river_data (tools/river_regrid/river_regrid.c:694-1376) on the arrays that get_source_data and
// get_mosaic_grid leave in river_type.  Kernels: river_kernels.hip; arithmetic: river.h; design: DESIGN.md 3.11.
//
// The host builds, once per handle: the halo map (update_halo_double :776 resolved to interior cells), the next-not-missing
// table and the adjust_lon targets of the source grid, the list of full-land cells.  A run is: the max-subA search, the tocell
// stencil, the outlets with an exclusive scan for their numbers, pointer jumping for travel and basin, one launch per travel
// level for the accumulated subA, then sort_basin and check_river_data on the host.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <utility>
#include <vector>
#include "river.h"
#include "xgrid_device.h"
#include "fg_host.h"

static std::atomic<int> g_prune{1};
extern "C" void fg_set_river_prune(int on) { g_prune = on ? 1 : 0; }

// qsort_index (:1538): the reference's own quicksort, whose order among equal values sort_basin's ids depend on.  The same
// exchanges in the same order within a range; the two halves are disjoint, so the smaller one recurses and the larger one loops.
static void rv_qsort_index(double *a, int start, int end, int *idx)
{
  while (end > start) {
    int l = start + 1, r = end;
    const int p = start + (end - start) / 2;
    std::swap(a[start], a[p]); std::swap(idx[start], idx[p]);
    const double pivot = a[start];
    while (l < r) {
      if (a[l] <= pivot) l++;
      else {
        while (l < r && a[r] >= pivot) --r;
        std::swap(a[l], a[r]); std::swap(idx[l], idx[r]);
      }
    }
    if (l != end || a[end] > pivot) {
      l--;
      std::swap(a[start], a[l]); std::swap(idx[start], idx[l]);
      if (l - start < end - r) { rv_qsort_index(a, start, l, idx); start = r; }
      else { rv_qsort_index(a, r, end, idx); end = l; }
    } else {                                   // the first element is the largest one
      std::swap(a[start], a[l]); std::swap(idx[start], idx[l]);
      end = l - 1;
    }
  }
}
extern "C" int fg_river_qsort_index(double *array, int n, int *index)
{
  if (n < 0 || (n > 0 && (!array || !index))) return fg_fail(FG_ERR_ARG, "fg_river_qsort_index: bad argument");
  rv_qsort_index(array, 0, n - 1, index);
  return 0;
}

// update_halo_double (:776-828) as a map: h[haloed index, tiles one after another] = the interior cell (flat over tiles) whose
// value the index holds after an update, -1 where no update ever writes (the value stays the initial one).  The assignments are
// carried out in the reference's order on the map itself, so an index filled from another filled index (the torus corners) resolves.
static std::vector<int> rv_halo_map(int ntiles, int nx, int ny, int opcode)
{
  const int nxp1 = nx + 1, nyp1 = ny + 1, nxp2 = nx + 2, per = (nx + 2) * (ny + 2);
  std::vector<int> h((size_t)ntiles * per, -1);
  for (int n = 0; n < ntiles; n++) for (int j = 1; j <= ny; j++) for (int i = 1; i <= nx; i++)
    h[(size_t)n * per + j * nxp2 + i] = (n * ny + (j - 1)) * nx + (i - 1);
  int *d0 = h.data();
  if (opcode & RV_X_CYCLIC) for (int j = 1; j < nyp1; j++) { d0[j * nxp2] = d0[j * nxp2 + nx]; d0[j * nxp2 + nxp1] = d0[j * nxp2 + 1]; }
  if (opcode & RV_Y_CYCLIC) for (int i = 1; i < nyp1; i++) { d0[i] = d0[ny * nxp2 + i]; d0[nyp1 * nxp2 + i] = d0[nxp2 + i]; }      // i = 1 .. ny, as written
  if ((opcode & RV_X_CYCLIC) && (opcode & RV_Y_CYCLIC)) {
    d0[0] = d0[ny * nxp2]; d0[nxp1] = d0[ny * nxp2 + 1]; d0[nyp1 * nxp2 + nxp1] = d0[nxp2 + 1]; d0[nyp1 * nxp2] = d0[nxp2 + nx];
  }
  if (opcode & RV_CUBIC_GRID) {
    for (int n = 0; n < ntiles; n++) {
      int *d = d0 + (size_t)n * per;
      if (n % 2) {
        const int *tw = d0 + (size_t)((n + 5) % ntiles) * per, *te = d0 + (size_t)((n + 2) % ntiles) * per;
        const int *ts = d0 + (size_t)((n + 4) % ntiles) * per, *tn = d0 + (size_t)((n + 1) % ntiles) * per;
        for (int j = 1; j < nyp1; j++) { d[j * nxp2] = tw[j * nxp2 + nx]; d[j * nxp2 + nxp1] = te[nxp2 + (nxp1 - j)]; }
        for (int i = 1; i < nxp1; i++) { d[i] = ts[(nyp1 - i) * nxp2 + nx]; d[nyp1 * nxp2 + i] = tn[nxp2 + i]; }
      } else {
        const int *tw = d0 + (size_t)((n + 4) % ntiles) * per, *te = d0 + (size_t)((n + 1) % ntiles) * per;
        const int *ts = d0 + (size_t)((n + 5) % ntiles) * per, *tn = d0 + (size_t)((n + 2) % ntiles) * per;
        for (int j = 1; j < nyp1; j++) { d[j * nxp2] = tw[ny * nxp2 + nxp1 - j]; d[j * nxp2 + nxp1] = te[j * nxp2 + 1]; }
        for (int i = 1; i < nxp1; i++) { d[i] = ts[ny * nxp2 + i]; d[nyp1 * nxp2 + i] = tn[(nyp1 - i) * nxp2 + 1]; }
      }
    }
  }
  return h;
}

struct fg_river {
  int device = 0, nx_in = 0, ny_in = 0, ntiles = 0, nx = 0, ny = 0, opcode = 0, pruned_ok = 1;
  long ncell = 0, nhalo = 0;
  double suba_cutoff = 1e12;
  double subA_missing = 0, cellarea_missing = 0, celllength_missing = 0;
  int tocell_missing = 0, travel_missing = 0, basin_missing = 0;
  hipStream_t stream = nullptr;
  FgDev dev;
  RvSource src;
  RvGrid grid;
  int nland = 0;
  int *d_land = nullptr;
  std::vector<int> hmap;
  std::vector<double> landfrac, maxsub_init;
  // results, interior cells, tiles one after another
  bool done = false;
  std::vector<double> maxsub, subA, cellarea, celllength;
  std::vector<int> tocell, travel, basin;
  long stats[7] = {0, 0, 0, 0, 0, 0, 0};
  float ms[5] = {0, 0, 0, 0, 0};             // create; max subA; tocell, outlets, travel and basin; accumulated subA; sort_basin and check
};

extern "C" void fg_river_destroy(fg_river *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  delete h;
}

static bool rv_int_missing(double v, int *out)
{
  if (!(v > -2147483648.0 && v < 0)) return false;
  *out = (int)v;
  return *out < 0;
}

extern "C" int fg_river_create(int nx_in, int ny_in, const double *xb_r, const double *yb_r, const double *subA_in, const double *missing6,
                               int ntiles, const int *nx_t, const int *ny_t, int opcode, const double *const *xb, const double *const *yb,
                               const double *const *xt, const double *const *yt, const double *const *area, const double *const *landfrac,
                               double suba_cutoff, int device, fg_river **out)
{
  if (!out) return fg_fail(FG_ERR_ARG, "fg_river_create: null output handle");
  *out = nullptr;
  if (nx_in < 1 || ny_in < 1 || (long)nx_in * ny_in > 0x3fffffffL || !xb_r || !yb_r || !subA_in || !missing6)
    return fg_fail(FG_ERR_ARG, "fg_river_create: bad source grid argument");
  if (ntiles < 1 || !nx_t || !ny_t || !xb || !yb || !xt || !yt || !area || !landfrac) return fg_fail(FG_ERR_ARG, "fg_river_create: bad mosaic argument");
  for (int n = 0; n < ntiles; n++) {
    if (nx_t[n] != nx_t[0] || ny_t[n] != ny_t[0]) return fg_fail(FG_ERR_ARG, "river_regrid: all the tiles should have the same grid size");
    if (!xb[n] || !yb[n] || !xt[n] || !yt[n] || !area[n] || !landfrac[n]) return fg_fail(FG_ERR_ARG, "fg_river_create: null tile array");
  }
  const int nx = nx_t[0], ny = ny_t[0];
  if (nx < 1 || ny < 1 || (double)ntiles * (nx + 2) * (ny + 2) > 0x3fffffff) return fg_fail(FG_ERR_ARG, "fg_river_create: bad tile size %d x %d", nx, ny);
  if (opcode & ~7) return fg_fail(FG_ERR_ARG, "fg_river_create: opcode %d is not a sum of 1 (x cyclic), 2 (y cyclic), 4 (cubic grid)", opcode);
  if ((opcode & RV_CUBIC_GRID) && ntiles != 6) return fg_fail(FG_ERR_ARG, "river_regrid: the mosaic must be a 6-tile cubic grid for 12 contacts.");
  if ((opcode & RV_CUBIC_GRID) && nx != ny) return fg_fail(FG_ERR_ARG, "fg_river_create: the tiles of a cubic grid must be square");
  if ((opcode & (RV_X_CYCLIC | RV_Y_CYCLIC)) && ntiles != 1) return fg_fail(FG_ERR_ARG, "river_regrid: number of tiles must be 1 for single contact");
  // update_halo_double's y-cyclic loop runs to ny along a row of nx + 2: with ny > nx it would write into the next rows
  if ((opcode & RV_Y_CYCLIC) && ny > nx) return fg_fail(FG_ERR_ARG, "fg_river_create: a y-cyclic grid with ny > nx is not supported (the reference's halo update runs its rows to ny)");
  fg_river *h = new fg_river;
  struct Guard { fg_river *&h; bool keep = false; ~Guard() { if (!keep) fg_river_destroy(h); } } guard{h};
  h->device = device; h->nx_in = nx_in; h->ny_in = ny_in; h->ntiles = ntiles; h->nx = nx; h->ny = ny; h->opcode = opcode; h->suba_cutoff = suba_cutoff;
  // init_river_data (:652-657) passes subA's missing value through an int; the three int fields take theirs from a double.  The
  // sweeps of calc_river_data and the outlet test take any value >= 0 for data, so those three must be negative.
  if (!(fabs(missing6[0]) < 2147483648.0)) return fg_fail(FG_ERR_ARG, "fg_river_create: subA's missing value %g does not fit the int that init_river_data keeps it in", missing6[0]);
  h->subA_missing = (double)(int)missing6[0];
  if (!rv_int_missing(missing6[1], &h->tocell_missing) || !rv_int_missing(missing6[2], &h->travel_missing) || !rv_int_missing(missing6[3], &h->basin_missing))
    return fg_fail(FG_ERR_ARG, "fg_river_create: the missing values of tocell, travel and basin must be negative integers (the reference's sweeps would take them for data)");
  h->cellarea_missing = missing6[4]; h->celllength_missing = missing6[5];
  const long per = (long)nx * ny, perh = (long)(nx + 2) * (ny + 2), perb = (long)(nx + 1) * (ny + 1);
  h->ncell = per * ntiles; h->nhalo = perh * ntiles;
  h->landfrac.resize(h->ncell);
  std::vector<double> areav(h->ncell), xbv(perb * ntiles), ybv(perb * ntiles), xtv(h->nhalo), ytv(h->nhalo);
  for (int n = 0; n < ntiles; n++) {
    memcpy(&h->landfrac[n * per], landfrac[n], per * sizeof(double));
    memcpy(&areav[n * per], area[n], per * sizeof(double));
    memcpy(&xbv[n * perb], xb[n], perb * sizeof(double));
    memcpy(&ybv[n * perb], yb[n], perb * sizeof(double));
    memcpy(&xtv[n * perh], xt[n], perh * sizeof(double));
    memcpy(&ytv[n * perh], yt[n], perh * sizeof(double));
  }
  for (long c = 0; c < h->ncell; c++)
    if (h->landfrac[c] > 1 || h->landfrac[c] < 0 || h->landfrac[c] != h->landfrac[c]) return fg_fail(FG_ERR_ARG, "river_regrid: land_frac should be between 0 or 1");
  if (int rc = fg_use_device("fg_river_create", device)) return rc;
  const double t0 = fg_now_ms();
  FGCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  // the halo of xt, yt (get_mosaic_grid :631): filled indices from their interior cell, the others as the caller gave them
  h->hmap = rv_halo_map(ntiles, nx, ny, opcode);
  {
    std::vector<double> xi(h->ncell), yi(h->ncell);
    for (long g = 0; g < h->nhalo; g++) {
      const long r = g % perh, j = r / (nx + 2), i = r % (nx + 2);
      if (j >= 1 && j <= ny && i >= 1 && i <= nx) { xi[h->hmap[g]] = xtv[g]; yi[h->hmap[g]] = ytv[g]; }
    }
    for (long g = 0; g < h->nhalo; g++) if (h->hmap[g] >= 0) { xtv[g] = xi[h->hmap[g]]; ytv[g] = yi[h->hmap[g]]; }
  }
  // the source grid: targets, next-not-missing table, and whether the pruned replay's premises hold
  std::vector<double> tlon(nx_in), sx(xb_r, xb_r + nx_in + 1), sy(yb_r, yb_r + ny_in + 1), ssub(subA_in, subA_in + (size_t)nx_in * ny_in);
  for (int i = 0; i < nx_in; i++) tlon[i] = 0.5 * (sx[i] + sx[i + 1]);
  for (int i = 0; i < nx_in; i++) if (!(sx[i] < sx[i + 1]) || (i > 0 && !(tlon[i - 1] <= tlon[i]))) h->pruned_ok = 0;
  for (int j = 0; j < ny_in; j++) if (!(sy[j] < sy[j + 1])) h->pruned_ok = 0;
  for (long c = 0; c < (long)xbv.size(); c++) if (xbv[c] != xbv[c] || ybv[c] != ybv[c]) h->pruned_ok = 0;
  std::vector<int> next((size_t)ny_in * (nx_in + 1));
  for (int j = 0; j < ny_in; j++) {
    int *row = &next[(size_t)j * (nx_in + 1)];
    row[nx_in] = nx_in;
    for (int i = nx_in - 1; i >= 0; i--) row[i] = (ssub[(size_t)j * nx_in + i] == h->subA_missing) ? row[i + 1] : i;
  }
  // :723: partial land and ocean get LARGE_VALUE, the full-land cells are searched
  std::vector<int> land;
  h->maxsub_init.assign(h->ncell, RV_LARGE);
  for (long c = 0; c < h->ncell; c++) if (!(h->landfrac[c] < 1)) { land.push_back((int)c); h->maxsub_init[c] = h->subA_missing; }
  h->nland = (int)land.size();
  FgDev &dev = h->dev;
  RvSource &s = h->src;
  s.xb = dev.put(sx); s.yb = dev.put(sy); s.tlon = dev.put(tlon); s.subA = dev.put(ssub); s.next = dev.put(next);
  s.nx = nx_in; s.ny = ny_in; s.missing = h->subA_missing;
  RvGrid &g = h->grid;
  g.ntiles = ntiles; g.nx = nx; g.ny = ny; g.opcode = opcode;
  g.xb = dev.put(xbv); g.yb = dev.put(ybv); g.xt = dev.put(xtv); g.yt = dev.put(ytv); g.area = dev.put(areav); g.landfrac = dev.put(h->landfrac);
  g.hmap = dev.put(h->hmap);
  h->d_land = dev.put(land);
  if (!s.xb || !s.yb || !s.tlon || !s.subA || !s.next || !g.xb || !g.yb || !g.xt || !g.yt || !g.area || !g.landfrac || !g.hmap || !h->d_land)
    return fg_fail(FG_ERR_HIP, "fg_river_create: device allocation or upload failed");
  h->ms[0] = (float)(fg_now_ms() - t0);
  guard.keep = true;
  *out = h;
  return 0;
}

// sort_basin (:1298-1376) on the interior arrays.  outlet[c]: last_point.
static int rv_sort_basin(fg_river *h, const std::vector<int> &outlet)
{
  int maxbasin = -1;
  for (long c = 0; c < h->ncell; c++) if (h->basin[c] > maxbasin) maxbasin = h->basin[c];
  const int nb = maxbasin > 0 ? maxbasin : 0;
  std::vector<double> maxsuba(nb, h->subA_missing);
  std::vector<int> indx(nb), rank(nb, -1);
  for (int n = 0; n < nb; n++) indx[n] = n;
  for (long c = 0; c < h->ncell; c++) if (outlet[c]) {
    const int b = h->basin[c];
    if (b > maxbasin || b < 1) return fg_fail(FG_ERR_ARG, "river_regrid: basin should be between 1 and maxbasin");
    maxsuba[b - 1] = h->subA[c];
  }
  for (int n = 0; n < nb; n++) if (maxsuba[n] == h->subA_missing) return fg_fail(FG_ERR_ARG, "river_regrid: maxsuba is not assigned for some basin");
  rv_qsort_index(maxsuba.data(), 0, nb - 1, indx.data());
  for (int n = 0; n < nb; n++) rank[indx[n]] = n;
  for (int n = 0; n < nb; n++) if (rank[n] < 0) return fg_fail(FG_ERR_ARG, "river_regrid: rank should be no less than 0");
  for (long c = 0; c < h->ncell; c++) {
    const int b = h->basin[c];
    if (b != h->basin_missing) {
      if (b > maxbasin || b < 1) return fg_fail(FG_ERR_ARG, "river_regrid: basin should be a positive integer no larger than maxbasin");
      h->basin[c] = maxbasin - rank[b - 1];
    }
  }
  return 0;
}

// check_river_data (:1180-1290): the counts, and its three fatal checks as errors
static int rv_check(fg_river *h, const std::vector<int> &outlet)
{
  const int nx = h->nx, ny = h->ny, nxp2 = nx + 2;
  const long per = (long)nx * ny, perh = (long)(nx + 2) * (ny + 2);
  int maxtravel = -1, maxbasin = -1;
  for (long c = 0; c < h->ncell; c++) { if (h->travel[c] > maxtravel) maxtravel = h->travel[c]; if (h->basin[c] > maxbasin) maxbasin = h->basin[c]; }
  long ncoast = 0, nsink = 0;
  for (long c = 0; c < h->ncell; c++) {
    const int tocell = h->tocell[c], travel = h->travel[c], basin = h->basin[c];
    const double subA = h->subA[c];
    if (h->landfrac[c] == 0) {
      if (tocell != h->tocell_missing || travel != h->travel_missing || basin != h->basin_missing || subA != h->subA_missing)
        return fg_fail(FG_ERR_ARG, "river_regrid, subA, tocell, travel, or basin is not missing value for some ocean points");
    } else if (tocell == h->tocell_missing || travel == h->travel_missing || basin == h->basin_missing || subA == h->subA_missing)
      return fg_fail(FG_ERR_ARG, "river_regrid, subA, tocell, travel, or basin is missing value for some river points");
    if (h->landfrac[c] == 1 && tocell == 0) {
      const long n = c / per, r = c % per, j = r / nx, i = r % nx;
      bool coast = false;
      for (int joff = 0; joff < 3 && !coast; joff++) for (int ioff = 0; ioff < 3; ioff++) {
        if (ioff == 1 && joff == 1) continue;
        const int hm = h->hmap[n * perh + (j + joff) * nxp2 + (i + ioff)];
        if ((hm >= 0 ? h->tocell[hm] : h->tocell_missing) == h->tocell_missing) { coast = true; break; }
      }
      if (coast) ncoast++; else nsink++;
    }
  }
  std::vector<int> cnt(maxbasin > 0 ? maxbasin : 0, 0);
  for (long c = 0; c < h->ncell; c++) if (outlet[c]) {
    const int b = h->basin[c];
    if (b >= 1 && b <= maxbasin) ++cnt[b - 1];
  }
  for (int n = 0; n < maxbasin; n++) {
    if (cnt[n] <= 0) return fg_fail(FG_ERR_ARG, "river_regrid: some river has no point with travel = 0");
    if (cnt[n] > 1) return fg_fail(FG_ERR_ARG, "river_regrid: some river has more than one point with travel = 0");
  }
  h->stats[0] = maxtravel; h->stats[1] = maxbasin; h->stats[2] = ncoast; h->stats[3] = nsink;
  return 0;
}

extern "C" int fg_river_run(fg_river *h)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_river_run: null handle");
  FGCHK(hipSetDevice(h->device));
  h->done = false;
  const long nc = h->ncell;
  hipStream_t st = h->stream;
  const RvGrid &g = h->grid;
  FgDev t;
  long launches = 0;
  const long ntile_scan = fgd_scan_tiles(nc);
  double *d_maxsub = t.put(h->maxsub_init), *d_cellarea = t.get<double>(nc), *d_celllength = t.get<double>(nc), *d_subA = t.get<double>(nc);
  int *d_tocell = t.get<int>(nc), *d_dir = t.get<int>(nc), *d_flag = t.get<int>(nc), *d_trav0 = t.get<int>(nc), *d_prefix = t.get<int>(nc + 1);
  int *d_succ[2] = {t.get<int>(nc), t.get<int>(nc)}, *d_hops[2] = {t.get<int>(nc), t.get<int>(nc)};
  int *d_travel = t.get<int>(nc), *d_basin = t.get<int>(nc), *d_cells = t.get<int>(nc);
  // zeroed words: [0] source cells visited, [1] the scan's total, [2] its ticket and error word, [3] the jump's flag, then the scan's status
  unsigned long long *d_z = t.get<unsigned long long>(4 + ntile_scan);
  if (!d_maxsub || !d_cellarea || !d_celllength || !d_subA || !d_tocell || !d_dir || !d_flag || !d_trav0 || !d_prefix || !d_succ[0] || !d_succ[1] ||
      !d_hops[0] || !d_hops[1] || !d_travel || !d_basin || !d_cells || !d_z)
    return fg_fail(FG_ERR_HIP, "fg_river_run: device allocation or upload failed");
  FGCHK(hipMemsetAsync(d_z, 0, (4 + ntile_scan) * sizeof(unsigned long long), st));
  unsigned *d_ticket = (unsigned *)(d_z + 2), *d_err = d_ticket + 1;
  int *d_changed = (int *)(d_z + 3);

  // 1. max subA (:719-762)
  double t0 = fg_now_ms();
  const int prune = g_prune && h->pruned_ok;
  fgd_rv_max_suba(h->src, g, h->nland, h->d_land, d_maxsub, d_z, prune, st); launches += h->nland > 0;
  FGCHK(hipGetLastError());
  h->maxsub.resize(nc);
  unsigned long long visited = 0;
  FGCHK(hipMemcpyAsync(h->maxsub.data(), d_maxsub, nc * sizeof(double), hipMemcpyDeviceToHost, st));
  FGCHK(hipMemcpyAsync(&visited, d_z, sizeof visited, hipMemcpyDeviceToHost, st));
  FGCHK(hipStreamSynchronize(st));
  double t1 = fg_now_ms();
  h->ms[1] = (float)(t1 - t0);

  // 3, 4, 6. tocell; outlets with their numbers; cellarea, celllength
  fgd_rv_tocell(g, d_maxsub, h->suba_cutoff, h->subA_missing, h->tocell_missing, d_tocell, d_dir, st);
  fgd_rv_outlets(g, d_tocell, d_dir, h->tocell_missing, h->cellarea_missing, h->celllength_missing, d_flag, d_trav0, d_succ[0], d_hops[0],
                 d_cellarea, d_celllength, st);
  fgd_exclusive_scan1(d_flag, nc, d_prefix, d_z + 4, d_ticket, d_z + 1, d_err, st);
  launches += 3;
  FGCHK(hipGetLastError());
  // 5. travel and basin: pointer jumping, the number of rounds is the logarithm of the longest river
  int cur = 0;
  for (int round = 0;; round++) {
    if (round > 40) return fg_fail(FG_ERR_ARG, "fg_river_run: the flow directions form a cycle");
    int changed = 0;
    FGCHK(hipMemsetAsync(d_changed, 0, sizeof(int), st));
    fgd_rv_jump(nc, d_succ[cur], d_hops[cur], d_succ[cur ^ 1], d_hops[cur ^ 1], d_changed, st); launches++;
    FGCHK(hipGetLastError());
    FGCHK(hipMemcpyAsync(&changed, d_changed, sizeof(int), hipMemcpyDeviceToHost, st));
    FGCHK(hipStreamSynchronize(st));
    cur ^= 1;
    if (!changed) break;
  }
  fgd_rv_finish(nc, d_tocell, h->tocell_missing, d_succ[cur], d_hops[cur], d_trav0, d_prefix, h->travel_missing, h->basin_missing, d_travel, d_basin, st);
  launches++;
  FGCHK(hipGetLastError());
  h->tocell.resize(nc); h->travel.resize(nc); h->basin.resize(nc); h->cellarea.resize(nc); h->celllength.resize(nc); h->subA.resize(nc);
  std::vector<int> outlet(nc), dirv(nc);
  unsigned scan_err = 0;
  FGCHK(hipMemcpyAsync(h->tocell.data(), d_tocell, nc * sizeof(int), hipMemcpyDeviceToHost, st));
  FGCHK(hipMemcpyAsync(dirv.data(), d_dir, nc * sizeof(int), hipMemcpyDeviceToHost, st));
  FGCHK(hipMemcpyAsync(h->travel.data(), d_travel, nc * sizeof(int), hipMemcpyDeviceToHost, st));
  FGCHK(hipMemcpyAsync(h->basin.data(), d_basin, nc * sizeof(int), hipMemcpyDeviceToHost, st));
  FGCHK(hipMemcpyAsync(outlet.data(), d_flag, nc * sizeof(int), hipMemcpyDeviceToHost, st));
  FGCHK(hipMemcpyAsync(h->cellarea.data(), d_cellarea, nc * sizeof(double), hipMemcpyDeviceToHost, st));
  FGCHK(hipMemcpyAsync(h->celllength.data(), d_celllength, nc * sizeof(double), hipMemcpyDeviceToHost, st));
  FGCHK(hipMemcpyAsync(&scan_err, d_err, sizeof scan_err, hipMemcpyDeviceToHost, st));
  FGCHK(hipStreamSynchronize(st));
  if (scan_err) return fg_fail(FG_ERR_HIP, "fg_river_run: the outlet scan failed (error bits %u)", scan_err);
  t0 = fg_now_ms();
  h->ms[2] = (float)(t0 - t1);

  // The reference's sweeps (:1095-1117) stop after the first one that assigns nothing.  Rivers that end in a cell next to the
  // ocean start at travel 1, so when no cell at all flows into a travel-0 cell the very first sweep is empty, and every cell
  // upstream of an outlet keeps its missing values: check_river_data then stops the reference.
  int maxtravel = -1;
  long level1 = 0, upstream = 0;
  for (long c = 0; c < nc; c++) {
    if (h->travel[c] > maxtravel) maxtravel = h->travel[c];
    if (!outlet[c] && dirv[c] >= 0) { upstream++; level1 += h->travel[c] == 1; }
  }
  if (upstream > 0 && level1 == 0)
    return fg_fail(FG_ERR_ARG, "river_regrid, subA, tocell, travel, or basin is missing value for some river points");
  // 7. accumulated subA by travel level, maxtravel down to 0 (:1130-1166)
  std::vector<int> start(maxtravel + 2, 0), cells(nc);
  for (long c = 0; c < nc; c++) if (h->travel[c] >= 0) start[h->travel[c] + 1]++;
  for (int l = 0; l <= maxtravel; l++) start[l + 1] += start[l];
  {
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (long c = 0; c < nc; c++) if (h->travel[c] >= 0) cells[fill[h->travel[c]]++] = (int)c;
  }
  FGCHK(hipMemcpyAsync(d_cells, cells.data(), nc * sizeof(int), hipMemcpyHostToDevice, st));
  {
    std::vector<double> miss(nc, h->subA_missing);
    FGCHK(hipMemcpyAsync(d_subA, miss.data(), nc * sizeof(double), hipMemcpyHostToDevice, st));
    FGCHK(hipStreamSynchronize(st));
  }
  for (int l = maxtravel; l >= 0; l--) {
    const int count = start[l + 1] - start[l];
    fgd_rv_level(g, l, count, d_cells + start[l], d_dir, d_travel, d_cellarea, h->subA_missing, d_subA, st); launches += count > 0;
  }
  FGCHK(hipGetLastError());
  FGCHK(hipMemcpyAsync(h->subA.data(), d_subA, nc * sizeof(double), hipMemcpyDeviceToHost, st));
  FGCHK(hipStreamSynchronize(st));
  t1 = fg_now_ms();
  h->ms[3] = (float)(t1 - t0);

  // 8, 9. sort_basin, check_river_data
  int rc = rv_sort_basin(h, outlet);
  if (rc) return rc;
  rc = rv_check(h, outlet);
  if (rc) return rc;
  h->stats[4] = h->nland; h->stats[5] = (long)visited; h->stats[6] = launches;
  h->ms[4] = (float)(fg_now_ms() - t1);
  h->done = true;
  return 0;
}

extern "C" int fg_river_get(const fg_river *h, int tile, double *subA, int *tocell, int *travel, int *basin, double *cellarea, double *celllength)
{
  if (!h || tile < 0 || tile >= h->ntiles) return fg_fail(FG_ERR_ARG, "fg_river_get: bad handle or tile");
  if (!h->done) return fg_fail(FG_ERR_ARG, "fg_river_get: fg_river_run has not completed on this handle");
  const size_t per = (size_t)h->nx * h->ny, o = per * tile;
  if (subA) memcpy(subA, &h->subA[o], per * sizeof(double));
  if (tocell) memcpy(tocell, &h->tocell[o], per * sizeof(int));
  if (travel) memcpy(travel, &h->travel[o], per * sizeof(int));
  if (basin) memcpy(basin, &h->basin[o], per * sizeof(int));
  if (cellarea) memcpy(cellarea, &h->cellarea[o], per * sizeof(double));
  if (celllength) memcpy(celllength, &h->celllength[o], per * sizeof(double));
  return 0;
}

extern "C" int fg_river_get_max_suba(const fg_river *h, int tile, double *out)
{
  if (!h || !out || tile < 0 || tile >= h->ntiles) return fg_fail(FG_ERR_ARG, "fg_river_get_max_suba: bad argument");
  if (h->maxsub.empty()) return fg_fail(FG_ERR_ARG, "fg_river_get_max_suba: fg_river_run has not searched on this handle");
  const size_t perh = (size_t)(h->nx + 2) * (h->ny + 2);
  for (size_t k = 0; k < perh; k++) { const int m = h->hmap[perh * tile + k]; out[k] = m >= 0 ? h->maxsub[m] : h->subA_missing; }
  return 0;
}

extern "C" int fg_river_stats(const fg_river *h, long *s, int n)
{
  if (!h || !s || n < 0) return fg_fail(FG_ERR_ARG, "fg_river_stats: bad argument");
  for (int k = 0; k < n && k < 7; k++) s[k] = h->stats[k];
  return 0;
}

extern "C" int fg_river_phase_ms(const fg_river *h, float *ms, int n)
{
  if (!h || !ms || n < 0) return fg_fail(FG_ERR_ARG, "fg_river_phase_ms: bad argument");
  for (int k = 0; k < n && k < 5; k++) ms[k] = h->ms[k];
  return 0;
}

extern "C" void *fg_river_stream(fg_river *h) { return h ? (void *)h->stream : nullptr; }
