// coupler.hip -- host orchestration of make_coupler_mosaic's exchange grids on the device (fg_coupler_*):
// tools/make_coupler_mosaic/make_coupler_mosaic.c:1198-2127 (atmosphere x land, atmosphere x ocean, the per-cell sums, the
// centroid distances, the masks) and :2466-2811 (land x ocean), one process, one ocean tile; a nested atmosphere tile (fg_coupler_set_nest),
// the wave grid :2976-3535 (fg_coupler_add_wave) and --check :3591-3661 (fg_coupler_check); LEGACY_CLIP (fg_coupler_create)
// or GREAT_CIRCLE_CLIP at first order (fg_coupler_create_gc: unit vectors, great-circle plans, the n-gon polygon-list search).
// Kernels: coupler_kernels.hip; shared declarations: coupler.h; design: DESIGN.md 3.13.
//
// The host decides what runs and how large the buffers are.  The three nested clip loops are plans (plan.hip) in the coupler's
// longitude frame; their exchange cells, the clipped atmosphere x land polygons and every list made of them stay in device
// memory from one search to the next (plan_internal.h), and so do the sums, distances and masks until a getter asks for them.
// What fg_coupler_run brings to the host is counted (fg_coupler_stats): list lengths, tile starts, the error word, and the
// counter block every search reads back.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "coupler.h"
#include "fg_host.h"
#include "plan_internal.h"
#include "xgrid_device.h"

namespace {
struct Grid {                                   // one tile in device memory
  int nx = 0, ny = 0, off = 0;                  // off: first cell in the grid's flattened numbering
  double *lon = nullptr, *lat = nullptr;
  double *x = nullptr, *y = nullptr, *z = nullptr;   // great-circle handle: the corners as unit vectors (fg_dev_latlon2xyz)
  double dlat = 0, dlon = 0;                    // what a search with this tile as destination takes (fg_dst_extents)
  int rect_hint = 0;
  long ncells() const { return (long)nx * ny; }
};
struct Cand {                                   // the remembered atmosphere x land polygons of one land tile (:1517-1546)
  int n = 0;
  int *pa = nullptr, *pl = nullptr, *pn = nullptr;
  double *plon = nullptr, *plat = nullptr, *lon_avg = nullptr, *area_ref = nullptr;
  double *px = nullptr, *py = nullptr, *pz = nullptr;      // great-circle handle: the vertices as unit vectors, [n][8] each
};
}  // namespace

struct fg_coupler {
  int device = 0, order = 2, south_ext = 0;
  double thresh = 1.0e-6;
  bool same = false;                            // land on the atmosphere grid (lnd_same_as_atm)
  bool gc = false;                              // GREAT_CIRCLE_CLIP (fg_coupler_create_gc): every clip is clip_2dx2d_great_circle, order 1
  int *d_iota = nullptr;                        // great-circle handle, land on the atmosphere grid: 0 .. na - 1
  hipStream_t stream = nullptr;
  FgDev dev;                                    // grids, areas, the ocean fraction: as long as the handle
  std::unique_ptr<FgDev> res;                   // what a run leaves: replaced by the next run
  std::vector<Grid> atm, lnd;                   // same: lnd is a copy of atm (the same device arrays)
  Grid ocn;
  int na = 0, nl = 0, no = 0;                   // cells of the three grids
  double *area_atm = nullptr, *area_lnd = nullptr, *area_ocn = nullptr, *omask = nullptr;
  int *d_aoff = nullptr;                        // [ntile_atm + 1] cell offsets of the atmosphere tiles
  // results
  bool ran = false;
  std::vector<CpList> axl, lxo;                 // per land tile
  CpList axo;
  std::vector<std::vector<int>> axl_start;      // [land tile][ntile_atm + 1]: where an atmosphere tile's cells begin in the list
  std::vector<int> axo_start;
  CpSums a{}, l{}, o{}, l2{}, o2{};             // l2 / o2: the sums of the land x ocean lists (:2699-2795)
  double *a_frac = nullptr, *l_frac = nullptr, *o_frac = nullptr;
  long d2h = 0, searches = 0, ncand = 0;
  int nbad = 0;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // create; atm x land candidates; atm x ocean; polygons x ocean; land x ocean; sums; run; wave x ocean
  // nested atmosphere tile (fg_coupler_set_nest): its terms stay out of the land and ocean cells' sums (:1765, :1792, :1857, :1903)
  int tile_nest = -1;
  // wave grid (fg_coupler_add_wave, :2976-3535)
  std::vector<Grid> wav;
  std::vector<std::pair<int, int>> wav_band;    // per wave tile: js_ocn, je_ocn of :3107-3117
  int nw = 0;
  bool wav_same = false;                        // wav_same_as_ocn: the file names of :3452-3455
  double *area_wav = nullptr;
  std::vector<CpList> wxo;                      // per wave tile
  CpSums w{}, ow{};                             // the wave cells' sums and the ocean cells' wave-side sums (:3294-3386)
  double *w_frac = nullptr;
};

extern "C" void fg_coupler_destroy(fg_coupler *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    fg_pool_retire_stream(h->stream);             // the plans of the runs left blocks and events tagged with this stream in the pool
    (void)hipStreamDestroy(h->stream);
  }
  delete h;
}
extern "C" void *fg_coupler_stream(fg_coupler *h) { return h ? (void *)h->stream : nullptr; }

// get_grid_area of the tiles of one grid (:614, :736, :896): the source records of a search against a dummy cell, as the
// library's own get_grid_area does, into area [cells of all tiles]
static int cp_grid_area(fg_coupler *h, const std::vector<Grid> &g, const double *d_dummy, double *area)
{
  std::vector<int> nx, ny;
  std::vector<const double *> lon, lat;
  for (const Grid &t : g) { nx.push_back(t.nx); ny.push_back(t.ny); lon.push_back(t.lon); lat.push_back(t.lat); }
  fg_plan *pl = nullptr;
  const long rc = fg_plan_create_dev_hint(FG_CONSERVE_ORDER1, (int)g.size(), nx.data(), ny.data(), lon.data(), lat.data(), 1, 1, d_dummy, d_dummy + 4,
                                          0.01, 0.01, 0, h->device, h->stream, &pl);
  if (rc < 0) return (int)rc;
  FgPlanView v;
  int e = fg_plan_view(pl, &v);
  if (!e && hipMemcpyAsync(area, v.src_area, (size_t)v.nsrc * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
    e = fg_fail(FG_ERR_HIP, "fg_coupler_create: copying the cell areas failed");
  if (!e && hipStreamSynchronize(h->stream) != hipSuccess) e = fg_fail(FG_ERR_HIP, "fg_coupler_create: the cell areas failed");
  fg_plan_destroy(pl);
  return e;
}

// get_grid_great_circle_area of the tiles of one grid (:607, :731, :890): the source records of a great-circle search against a dummy cell
static int cp_grid_area_gc(fg_coupler *h, const std::vector<Grid> &g, const double *d_dummy, double *area)
{
  std::vector<int> nx, ny;
  std::vector<const double *> x, y, z;
  for (const Grid &t : g) { nx.push_back(t.nx); ny.push_back(t.ny); x.push_back(t.x); y.push_back(t.y); z.push_back(t.z); }
  fg_plan *pl = nullptr;
  const long rc = fg_plan_create_great_circle_dev((int)g.size(), nx.data(), ny.data(), x.data(), y.data(), z.data(), nullptr, 1, 1, d_dummy, d_dummy + 4,
                                                  d_dummy + 8, 0.01, 0.01, h->device, h->stream, 1, &pl);
  if (rc < 0) return (int)rc;
  FgPlanView v;
  int e = fg_plan_view(pl, &v);
  if (!e && hipMemcpyAsync(area, v.src_area, (size_t)v.nsrc * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
    e = fg_fail(FG_ERR_HIP, "fg_coupler_create_gc: copying the cell areas failed");
  if (!e && hipStreamSynchronize(h->stream) != hipSuccess) e = fg_fail(FG_ERR_HIP, "fg_coupler_create_gc: the cell areas failed");
  fg_plan_destroy(pl);
  return e;
}
// latlon2xyz of every tile's corners on the device (:598-612, :722-760, :881-890), queued on the handle's stream
static int cp_grid_xyz(fg_coupler *h, std::vector<Grid> *g)
{
  for (Grid &t : *g) {
    const size_t np = (size_t)(t.nx + 1) * (t.ny + 1);
    double *d = h->dev.get<double>(3 * np);
    if (!d) return fg_fail(FG_ERR_HIP, "fg_coupler_create_gc: out of device memory");
    t.x = d; t.y = d + np; t.z = d + 2 * np;
    if (int rc = fg_dev_latlon2xyz((long)np, t.lon, t.lat, t.x, t.y, t.z, h->device, h->stream)) return rc;
  }
  return 0;
}

static int cp_put_grid(fg_coupler *h, const char *what, int ntiles, const int *nx, const int *ny, const double *const *lon, const double *const *lat,
                       std::vector<Grid> *out, int *total)
{
  if (ntiles < 1 || !nx || !ny || !lon || !lat) return fg_fail(FG_ERR_ARG, "fg_coupler_create: bad %s grid argument", what);
  long off = 0;
  for (int t = 0; t < ntiles; t++) {
    if (nx[t] < 1 || ny[t] < 1 || !lon[t] || !lat[t]) return fg_fail(FG_ERR_ARG, "fg_coupler_create: bad %s tile %d", what, t);
    Grid g;
    g.nx = nx[t]; g.ny = ny[t]; g.off = (int)off;
    const size_t np = (size_t)(nx[t] + 1) * (ny[t] + 1);
    g.lon = h->dev.put(lon[t], np); g.lat = h->dev.put(lat[t], np);
    if (!g.lon || !g.lat) return fg_fail(FG_ERR_HIP, "fg_coupler_create: device allocation or upload failed");
    fg_dst_extents(g.nx, g.ny, lon[t], lat[t], &g.dlat, &g.dlon, &g.rect_hint);
    off += g.ncells();
    if (off > (1L << 28)) return fg_fail(FG_ERR_ARG, "fg_coupler_create: the %s grid has more than 2^28 cells", what);
    out->push_back(g);
  }
  *total = (int)off;
  return 0;
}

static int cp_create(bool gc, int interp_order, double area_ratio_thresh, int ntile_atm, const int *nxa, const int *nya,
                     const double *const *lon_atm, const double *const *lat_atm, int ntile_lnd, const int *nxl, const int *nyl,
                     const double *const *lon_lnd, const double *const *lat_lnd, int nxo, int nyo, const double *lon_ocn,
                     const double *lat_ocn, const double *omask, int ocn_south_ext, int device, fg_coupler **out)
{
  if (!out) return fg_fail(FG_ERR_ARG, "fg_coupler_create: null output handle");
  *out = nullptr;
  if (interp_order != 1 && interp_order != 2) return fg_fail(FG_ERR_ARG, "make_coupler_mosaic: interp_order should be 1 or 2");
  if (gc && interp_order != 1)                 // :593
    return fg_fail(FG_ERR_ARG, "make_coupler_mosaic:  Currenly only implement interp_order = 1 when clip_method = 'conserve_great_circle'");
  // the searches accept a pair at area / min(area1, area2) > 1e-6 (create_xgrid.c); the coupler's own tests can only reject more
  // when its threshold is no smaller and the fractions are no larger than 1
  if (!(area_ratio_thresh >= 1.0e-6)) return fg_fail(FG_ERR_ARG, "fg_coupler_create: area_ratio_thresh %g is below 1e-6, the ratio at which the searches accept a pair", area_ratio_thresh);
  if (ntile_lnd < 0 || ntile_lnd > CP_MAX_LISTS || ntile_atm > CP_MAX_LISTS)
    return fg_fail(FG_ERR_ARG, "fg_coupler_create: at most %d atmosphere and land tiles", CP_MAX_LISTS);
  if (!lon_ocn || !lat_ocn || !omask || nxo < 1 || nyo < 1 || ocn_south_ext < 0 || ocn_south_ext >= nyo)
    return fg_fail(FG_ERR_ARG, "fg_coupler_create: bad ocean grid argument");
  for (long c = 0; c < (long)nxo * nyo; c++)
    if (!(omask[c] >= 0.0 && omask[c] <= 1.0)) return fg_fail(FG_ERR_ARG, "fg_coupler_create: the ocean fraction of cell %ld is %g, outside [0, 1]", c, omask[c]);
  fg_coupler *h = new fg_coupler;
  struct Guard { fg_coupler *&h; bool keep = false; ~Guard() { if (!keep) fg_coupler_destroy(h); } } guard{h};
  h->device = device; h->order = interp_order; h->thresh = area_ratio_thresh; h->south_ext = ocn_south_ext; h->same = ntile_lnd == 0;
  h->gc = gc;
  if (int rc = fg_use_device("fg_coupler_create", device)) return rc;
  const double t0 = fg_now_ms();
  FGCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  if (int rc = cp_put_grid(h, "atmosphere", ntile_atm, nxa, nya, lon_atm, lat_atm, &h->atm, &h->na)) return rc;
  if (gc) if (int rc = cp_grid_xyz(h, &h->atm)) return rc;
  if (h->same) { h->lnd = h->atm; h->nl = h->na; }
  else {
    if (int rc = cp_put_grid(h, "land", ntile_lnd, nxl, nyl, lon_lnd, lat_lnd, &h->lnd, &h->nl)) return rc;
    if (gc) if (int rc = cp_grid_xyz(h, &h->lnd)) return rc;
  }
  {
    std::vector<Grid> o;
    const double *lo[1] = {lon_ocn}, *la[1] = {lat_ocn};
    if (int rc = cp_put_grid(h, "ocean", 1, &nxo, &nyo, lo, la, &o, &h->no)) return rc;
    if (gc) if (int rc = cp_grid_xyz(h, &o)) return rc;
    h->ocn = o[0];
  }
  std::vector<int> aoff;
  for (const Grid &g : h->atm) aoff.push_back(g.off);
  aoff.push_back(h->na);
  const double dummy[8] = {0, 0.01, 0, 0.01, 0, 0, 0.01, 0.01};
  double dummy_xyz[12];                          // the same cell as unit vectors: x[4] | y[4] | z[4]
  fg_latlon2xyz(4, dummy, dummy + 4, dummy_xyz, dummy_xyz + 4, dummy_xyz + 8);
  const double *d_dummy = gc ? h->dev.put(dummy_xyz, 12) : h->dev.put(dummy, 8);
  h->area_atm = h->dev.get<double>(h->na); h->area_ocn = h->dev.get<double>(h->no);
  h->area_lnd = h->same ? h->area_atm : h->dev.get<double>(h->nl);
  h->omask = h->dev.put(omask, (size_t)h->no);
  h->d_aoff = h->dev.put(aoff);
  if (gc && h->same) {
    std::vector<int> iota((size_t)h->na);
    for (int c = 0; c < h->na; c++) iota[(size_t)c] = c;
    h->d_iota = h->dev.put(iota);
    if (!h->d_iota) return fg_fail(FG_ERR_HIP, "fg_coupler_create: device allocation or upload failed");
  }
  if (!d_dummy || !h->area_atm || !h->area_ocn || !h->area_lnd || !h->omask || !h->d_aoff)
    return fg_fail(FG_ERR_HIP, "fg_coupler_create: device allocation or upload failed");
  const auto grid_area = gc ? cp_grid_area_gc : cp_grid_area;
  if (int rc = grid_area(h, h->atm, d_dummy, h->area_atm)) return rc;
  if (!h->same) if (int rc = grid_area(h, h->lnd, d_dummy, h->area_lnd)) return rc;
  if (int rc = grid_area(h, std::vector<Grid>{h->ocn}, d_dummy, h->area_ocn)) return rc;
  h->ms[0] = (float)(fg_now_ms() - t0);
  guard.keep = true;
  *out = h;
  return 0;
}

extern "C" int fg_coupler_create(int interp_order, double area_ratio_thresh, int ntile_atm, const int *nxa, const int *nya,
                                 const double *const *lon_atm, const double *const *lat_atm, int ntile_lnd, const int *nxl, const int *nyl,
                                 const double *const *lon_lnd, const double *const *lat_lnd, int nxo, int nyo, const double *lon_ocn,
                                 const double *lat_ocn, const double *omask, int ocn_south_ext, int device, fg_coupler **out)
{
  return cp_create(false, interp_order, area_ratio_thresh, ntile_atm, nxa, nya, lon_atm, lat_atm, ntile_lnd, nxl, nyl, lon_lnd, lat_lnd, nxo, nyo,
                   lon_ocn, lat_ocn, omask, ocn_south_ext, device, out);
}
// GREAT_CIRCLE_CLIP (:587-594): the same arguments; interp_order must be 1
extern "C" int fg_coupler_create_gc(int interp_order, double area_ratio_thresh, int ntile_atm, const int *nxa, const int *nya,
                                    const double *const *lon_atm, const double *const *lat_atm, int ntile_lnd, const int *nxl, const int *nyl,
                                    const double *const *lon_lnd, const double *const *lat_lnd, int nxo, int nyo, const double *lon_ocn,
                                    const double *lat_ocn, const double *omask, int ocn_south_ext, int device, fg_coupler **out)
{
  return cp_create(true, interp_order, area_ratio_thresh, ntile_atm, nxa, nya, lon_atm, lat_atm, ntile_lnd, nxl, nyl, lon_lnd, lat_lnd, nxo, nyo,
                   lon_ocn, lat_ocn, omask, ocn_south_ext, device, out);
}

// A nested atmosphere tile (:626-640 finds it in the atmosphere mosaic's contacts; here the caller names it): an index into the
// atmosphere tiles, -1 for none.  Refused with land on the atmosphere grid (:742).  Takes effect with the next run.
extern "C" int fg_coupler_set_nest(fg_coupler *h, int tile_nest)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_coupler_set_nest: null handle");
  if (tile_nest < -1 || tile_nest >= (int)h->atm.size())
    return fg_fail(FG_ERR_ARG, "fg_coupler_set_nest: no atmosphere tile %d (the handle has %d)", tile_nest, (int)h->atm.size());
  if (tile_nest >= 0 && h->same)
    return fg_fail(FG_ERR_ARG, "make_coupler_mosaic: land mosaic must be different from atmos mosaic when there is nest region in atmos mosaic");
  h->tile_nest = tile_nest;
  h->ran = false;
  return 0;
}

// The wave grid (:2976-3535, legacy clip): its tiles, their areas (:1036) and per tile the ocean row band of :3107-3117.
// wav_same_as_ocn changes nothing with one ocean tile (:3119-3126) but the file names (:3452-3455).  Takes effect with the next run.
extern "C" int fg_coupler_add_wave(fg_coupler *h, int ntile_wav, const int *nx, const int *ny, const double *const *lon, const double *const *lat,
                                   int wav_same_as_ocn)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_coupler_add_wave: null handle");
  if (h->gc) return fg_fail(FG_ERR_ARG, "fg_coupler_add_wave: the great-circle handle takes no wave grid (it is first order only)");
  if (!h->wav.empty()) return fg_fail(FG_ERR_ARG, "fg_coupler_add_wave: the handle has a wave grid already");
  if (ntile_wav < 1 || ntile_wav > CP_MAX_LISTS) return fg_fail(FG_ERR_ARG, "fg_coupler_add_wave: 1 to %d wave tiles", CP_MAX_LISTS);
  FGCHK(hipSetDevice(h->device));
  std::vector<Grid> wav;
  int nw = 0;
  if (int rc = cp_put_grid(h, "wave", ntile_wav, nx, ny, lon, lat, &wav, &nw)) return rc;
  const double dummy[8] = {0, 0.01, 0, 0.01, 0, 0, 0.01, 0.01};
  const double *d_dummy = h->dev.put(dummy, 8);
  double *area = h->dev.get<double>((size_t)nw);
  int *d_band = h->dev.get<int>(2);
  if (!d_dummy || !area || !d_band) return fg_fail(FG_ERR_HIP, "fg_coupler_add_wave: device allocation or upload failed");
  if (int rc = cp_grid_area(h, wav, d_dummy, area)) return rc;
  std::vector<std::pair<int, int>> bands;
  for (const Grid &g : wav) {
    const double *y = lat[&g - wav.data()];
    double yw_min = 9999, yw_max = -9999;                                  // :3071-3104 (one process: every cell of the tile)
    for (size_t p = 0; p < (size_t)(g.nx + 1) * (g.ny + 1); p++) { if (y[p] > yw_max) yw_max = y[p]; if (y[p] < yw_min) yw_min = y[p]; }
    int band[2] = {h->ocn.ny, -1};                                         // :3108
    FGCHK(hipMemcpyAsync(d_band, band, sizeof band, hipMemcpyHostToDevice, h->stream));
    fgd_cp_row_band(h->ocn.nx, h->ocn.ny, h->ocn.lat, yw_min, yw_max, d_band, h->stream);
    FGCHK(hipGetLastError());
    FGCHK(hipMemcpyAsync(band, d_band, sizeof band, hipMemcpyDeviceToHost, h->stream));
    FGCHK(hipStreamSynchronize(h->stream));
    bands.push_back({std::max(0, band[0] - 1), std::min(h->ocn.ny - 1, band[1] + 1)});      // :3116-3117
  }
  h->wav = wav; h->nw = nw; h->area_wav = area; h->wav_band = bands; h->wav_same = wav_same_as_ocn != 0;
  h->ran = false;
  return 0;
}

// --------------------------------------------------------------------------------------------------------------- the run
namespace {
struct Run {
  fg_coupler *h;
  FgDev &res;
  hipStream_t st;
  unsigned *d_err = nullptr;
  int *d_nbad = nullptr;

  int fetch(void *dst, const void *src, size_t bytes)          // device -> host, counted
  {
    FGCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    FGCHK(hipStreamSynchronize(st));
    h->d2h += (long)bytes;
    return 0;
  }
  bool alloc_list(CpList *l, long cap)
  {
    *l = CpList{};
    l->cap = cap;
    const size_t n = (size_t)(cap > 0 ? cap : 1);
    l->c1 = res.get<int>(n); l->c2 = res.get<int>(n);
    l->area = res.get<double>(n); l->clon = res.get<double>(n); l->clat = res.get<double>(n);
    bool ok = l->c1 && l->c2 && l->area && l->clon && l->clat;
    for (int q = 0; q < 4; q++) { l->d[q] = res.get<double>(n); ok = ok && l->d[q]; }
    if (ok) ok = hipMemsetAsync(l->clon, 0, n * sizeof(double), st) == hipSuccess && hipMemsetAsync(l->clat, 0, n * sizeof(double), st) == hipSuccess;
    return ok;
  }
  bool alloc_sums(CpSums *s, long n)
  {
    const size_t m = (size_t)(n > 0 ? n : 1);
    s->area = res.get<double>(m); s->clon = res.get<double>(m); s->clat = res.get<double>(m);
    if (!s->area || !s->clon || !s->clat) return false;
    return hipMemsetAsync(s->area, 0, m * sizeof(double), st) == hipSuccess && hipMemsetAsync(s->clon, 0, m * sizeof(double), st) == hipSuccess &&
           hipMemsetAsync(s->clat, 0, m * sizeof(double), st) == hipSuccess;
  }
  // flags -> offsets and the total on the host
  int scan_total(FgDev &t, long n, const int *flag, int **offs, int *total)
  {
    *offs = t.get<int>((size_t)(n > 0 ? n : 1));
    int *bsum = t.get<int>((size_t)fgd_cp_scan_blocks(n)), *d_tot = t.get<int>(1);
    if (!*offs || !bsum || !d_tot) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    fgd_cp_scan(n, flag, *offs, bsum, d_tot, st);
    FGCHK(hipGetLastError());
    return fetch(total, d_tot, sizeof(int));
  }
  long search(int ntiles, const std::vector<Grid> &src, const Grid &dst, fg_plan **pl)
  {
    std::vector<int> nx_, ny;
    std::vector<const double *> lon, lat;
    for (int t = 0; t < ntiles; t++) { nx_.push_back(src[t].nx); ny.push_back(src[t].ny); lon.push_back(src[t].lon); lat.push_back(src[t].lat); }
    h->searches++;
    long nx;
    if (h->gc) {                                   // clip_2dx2d_great_circle on every pair the caps let through
      std::vector<const double *> x, y, z;
      for (int t = 0; t < ntiles; t++) { x.push_back(src[t].x); y.push_back(src[t].y); z.push_back(src[t].z); }
      nx = fg_plan_create_great_circle_dev(ntiles, nx_.data(), ny.data(), x.data(), y.data(), z.data(), nullptr, dst.nx, dst.ny, dst.x, dst.y, dst.z,
                                           dst.dlat, dst.dlon, h->device, st, 1, pl);
    } else
      nx = fg_plan_create_dev_hint(h->order, ntiles, nx_.data(), ny.data(), lon.data(), lat.data(), dst.nx, dst.ny, dst.lon, dst.lat, dst.dlat,
                                   dst.dlon, dst.rect_hint, h->device, st, pl);
    if (nx >= 0) h->d2h += fg_plan_search_d2h(*pl);
    return nx;
  }
  int check_err()
  {
    unsigned e = 0;
    if (int rc = fetch(&e, d_err, sizeof e)) return rc;
    if (e & CP_ERR_NVERT) return fg_fail(FG_ERR_GEOM, "make_coupler_mosaic: inconsistent number of grid box coreners");
    if (e & CP_ERR_MAXV) return fg_fail(FG_ERR_GEOM, "fg_coupler_run: an atmosphere x land polygon has more than 8 vertices");
    return 0;
  }

  bool alloc_cand(Cand *c, long n)
  {
    const size_t m = (size_t)(n > 0 ? n : 1);
    c->pa = res.get<int>(m); c->pl = res.get<int>(m); c->pn = res.get<int>(m);
    c->area_ref = res.get<double>(m);
    if (h->gc) {                                   // unit vectors; no longitude frame, so no lon_avg
      c->px = res.get<double>(m * 8); c->py = res.get<double>(m * 8); c->pz = res.get<double>(m * 8);
      return c->pa && c->pl && c->pn && c->area_ref && c->px && c->py && c->pz;
    }
    c->plon = res.get<double>(m * 8); c->plat = res.get<double>(m * 8); c->lon_avg = res.get<double>(m);
    return c->pa && c->pl && c->pn && c->plon && c->plat && c->lon_avg && c->area_ref;
  }
  // great-circle handle, :1426-1437 and :1483-1507 for the cells of atmosphere tile t: the remembered polygon is the cell itself, so
  // only its flag is kept -- ref [cells of the tile] = min(area_lnd, area_atm) where the cell is remembered, +inf where it is not
  // (no term and no list entry can then pass a ratio test)
  int cand_same_gc(int t, double *ref, long *count)
  {
    const Grid &g = h->atm[t];
    const long n = g.ncells();
    FgDev tmp;
    double *cells = tmp.get<double>((size_t)n * 12), *xarea = tmp.get<double>((size_t)n);
    int *four = tmp.get<int>((size_t)n), *flag = tmp.get<int>((size_t)n), *offs = nullptr, total = 0;
    if (!cells || !xarea || !four || !flag) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    fgd_cp_cells_xyz(g.nx, g.ny, g.x, g.y, g.z, cells, four, st);
    fgd_gc_area_batch((int)n, 4, cells, four, xarea, st);                                  // :1485 on the four corners as they are
    fgd_cp_same_gc_flag(n, xarea, h->area_atm + g.off, h->thresh, flag, ref, st);
    if (int rc = scan_total(tmp, n, flag, &offs, &total)) return rc;
    *count = total;
    return 0;
  }
  // great-circle handle, :1439 and :1483-1548 for land tile t of its own
  int cand_own_gc(int t, Cand *c)
  {
    const Grid &g = h->lnd[t];
    fg_plan *pl = nullptr;
    const long nx = search((int)h->atm.size(), h->atm, g, &pl);
    if (nx < 0) return (int)nx;
    struct Destroy { fg_plan *p; ~Destroy() { fg_plan_destroy(p); } } destroy{pl};
    FgPlanView v;
    if (int rc = fg_plan_view(pl, &v)) return rc;
    FgDev tmp;
    const size_t m = (size_t)(nx > 0 ? nx : 1);
    int *flag = tmp.get<int>(m), *pn = tmp.get<int>(m), *offs = nullptr, total = 0;
    double *px = tmp.get<double>(m * 8), *py = tmp.get<double>(m * 8), *pz = tmp.get<double>(m * 8);
    if (!flag || !pn || !px || !py || !pz) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    const double *area_lnd = h->area_lnd + g.off;
    if (nx > 0) if (int rc = fg_plan_polygons_gc_dev(pl, pn, px, py, pz)) return rc;
    fgd_cp_cand_flag(nx, v.x_src, v.x_dst, v.x_area, h->area_atm, area_lnd, h->thresh, flag, st);
    if (int rc = scan_total(tmp, nx, flag, &offs, &total)) return rc;
    if (!alloc_cand(c, total)) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    c->n = total;
    fgd_cp_cand_emit_gc(nx, v.x_src, v.x_dst, flag, offs, pn, px, py, pz, h->area_atm, area_lnd, c->pa, c->pl, c->pn, c->px, c->py, c->pz, c->area_ref,
                        d_err, st);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(st));
    return 0;
  }
  // :1463-1477 for the cells of atmosphere tile t
  int cand_same(int t, Cand *c)
  {
    const Grid &g = h->atm[t];
    const long n = g.ncells();
    FgDev tmp;
    int *flag = tmp.get<int>((size_t)n), *offs = nullptr, total = 0;
    if (!flag) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    const double *area = h->area_atm + g.off;
    fgd_cp_same_flag(g.nx, g.ny, g.lon, g.lat, area, h->thresh, flag, d_err, st);
    if (int rc = scan_total(tmp, n, flag, &offs, &total)) return rc;
    if (!alloc_cand(c, total)) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    c->n = total;
    fgd_cp_same_emit(g.nx, g.ny, g.lon, g.lat, area, flag, offs, g.off, c->pa, c->pl, c->pn, c->plon, c->plat, c->lon_avg, c->area_ref, d_err, st);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(st));
    return 0;
  }
  // :1396-1551 for land tile t of its own: a search, its polygons, the coupler's ratio test
  int cand_own(int t, Cand *c)
  {
    const Grid &g = h->lnd[t];
    fg_plan *pl = nullptr;
    const long nx = search((int)h->atm.size(), h->atm, g, &pl);
    if (nx < 0) return (int)nx;
    struct Destroy { fg_plan *p; ~Destroy() { fg_plan_destroy(p); } } destroy{pl};
    FgPlanView v;
    if (int rc = fg_plan_view(pl, &v)) return rc;
    FgDev tmp;
    const size_t m = (size_t)(nx > 0 ? nx : 1);
    int *flag = tmp.get<int>(m), *pn = tmp.get<int>(m), *offs = nullptr, total = 0;
    double *plon = tmp.get<double>(m * 8), *plat = tmp.get<double>(m * 8);
    if (!flag || !pn || !plon || !plat) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    const double *area_lnd = h->area_lnd + g.off;
    if (nx > 0) if (int rc = fg_plan_polygons_dev(pl, pn, plon, plat)) return rc;
    fgd_cp_cand_flag(nx, v.x_src, v.x_dst, v.x_area, h->area_atm, area_lnd, h->thresh, flag, st);
    if (int rc = scan_total(tmp, nx, flag, &offs, &total)) return rc;
    if (!alloc_cand(c, total)) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    c->n = total;
    fgd_cp_cand_emit(nx, v.x_src, v.x_dst, flag, offs, pn, plon, plat, v.src_lon_avg, h->area_atm, area_lnd, c->pa, c->pl, c->pn, c->plon, c->plat,
                     c->lon_avg, c->area_ref, d_err, st);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(st));
    return 0;
  }
  // :1604-1661 (src = the atmosphere) and :2598-2690 (src = one land tile): the search, the ocean-fraction tests, the survivors
  // keep != null: the plan is handed to the caller instead of destroyed (great-circle handle with land on the atmosphere grid: step 4
  // works on the same pairs)
  // band != null (wave x ocean, :3107-3117, :3162): only the ocean rows band->first .. band->second are looked at
  int ocean_list(int ntiles, const std::vector<Grid> &src, const double *area_src, CpList *out, fg_plan **keep = nullptr,
                 const std::pair<int, int> *band = nullptr)
  {
    fg_plan *pl = nullptr;
    const long nx = search(ntiles, src, h->ocn, &pl);
    if (nx < 0) return (int)nx;
    struct Destroy { fg_plan *p; fg_plan **keep; ~Destroy() { if (keep && *keep == p) return; fg_plan_destroy(p); } } destroy{pl, keep};
    FgPlanView v;
    if (int rc = fg_plan_view(pl, &v)) return rc;
    FgDev tmp;
    int *flag = tmp.get<int>((size_t)(nx > 0 ? nx : 1)), *offs = nullptr, total = 0;
    if (!flag) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    fgd_cp_ocean_flag(nx, v.x_src, v.x_dst, v.x_area, h->omask, h->area_ocn, area_src, h->thresh, flag, st);
    if (band) fgd_cp_band_mask(nx, v.x_dst, h->ocn.nx, band->first, band->second, flag, st);
    if (int rc = scan_total(tmp, nx, flag, &offs, &total)) return rc;
    if (!alloc_list(out, total)) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    out->n = total;
    fgd_cp_ocean_emit(nx, v.x_src, v.x_dst, v.x_area, v.x_c1, v.x_c2, h->omask, flag, offs, *out, st);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(st));
    if (keep) *keep = pl;
    return 0;
  }
  // the tail of :1662-1719 for `npoly` polygons numbered as x_src numbers them: the sums per polygon, the final test, the list.
  // pa / pl: the atmosphere cell and the land cell of every polygon
  int poly_tail(int npoly, const FgPlanView &v, const double *area_ref, const int *pa, const int *pl_, std::vector<CpList *> outs,
                const std::vector<int> &first, const std::vector<int> &count)
  {
    FgDev tmp;
    const size_t m = (size_t)(npoly > 0 ? npoly : 1);
    double *s_area = tmp.get<double>(m), *s_clon = tmp.get<double>(m), *s_clat = tmp.get<double>(m);
    int *flag = tmp.get<int>(m);
    if (!s_area || !s_clon || !s_clat || !flag) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    fgd_cp_poly_sums(npoly, v.nx, v.x_src, v.x_dst, v.x_area, v.x_c1, v.x_c2, h->omask, area_ref, h->thresh, s_area, s_clon, s_clat, flag, st);
    for (size_t q = 0; q < outs.size(); q++) {           // one list per land tile: polygons [first, first + count)
      int *offs = nullptr, total = 0;
      const int f = first[q], n = count[q];
      if (int rc = scan_total(tmp, n, flag + f, &offs, &total)) return rc;
      if (!alloc_list(outs[q], total)) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
      outs[q]->n = total;
      // (pa is indexed by polygon, hence + f; pl_ is NOT offset when f > 0: that only happens with land on the atmosphere grid, where
      // pl_ is 0, 1, 2, ... and the land cell of the tile's polygon q is q, the cell's index inside its tile)
      fgd_cp_poly_emit(n, pa + f, pl_, s_area + f, s_clon + f, s_clat + f, flag + f, offs, *outs[q], st);
      FGCHK(hipGetLastError());
      FGCHK(hipStreamSynchronize(st));
    }
    return 0;
  }
  // great-circle handle, :1662-1719 with land of its own: the polygon-list search, then the tail
  int poly_list_gc(const Cand &c, CpList *out)
  {
    if (c.n == 0) { if (!alloc_list(out, 0)) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory"); return 0; }
    fg_plan *pl = nullptr;
    h->searches++;
    const Grid &o = h->ocn;
    const long nx = fg_plan_create_polylist_gc_dev(c.n, c.pn, c.px, c.py, c.pz, c.area_ref, o.nx, o.ny, o.x, o.y, o.z, o.dlat, o.dlon, h->device, st, 1, &pl);
    if (nx == FG_ERR_MAXV) return fg_fail(FG_ERR_GEOM, "fg_coupler_run: an atmosphere x land polygon has more than 8 vertices");
    if (nx < 0) return (int)nx;
    struct Destroy { fg_plan *p; ~Destroy() { fg_plan_destroy(p); } } destroy{pl};
    h->d2h += fg_plan_search_d2h(pl);
    FgPlanView v;
    if (int rc = fg_plan_view(pl, &v)) return rc;
    return poly_tail(c.n, v, c.area_ref, c.pa, c.pl, {out}, {0}, {c.n});
  }
  // :1662-1719: the remembered polygons against the ocean cells over land, the sums per polygon, the final area test
  int poly_list(const Cand &c, CpList *out)
  {
    if (c.n == 0) { if (!alloc_list(out, 0)) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory"); return 0; }
    fg_plan *pl = nullptr;
    h->searches++;
    const Grid &o = h->ocn;
    const long nx = fg_plan_create_polylist_dev(h->order, c.n, c.pn, c.plon, c.plat, c.lon_avg, c.area_ref, o.nx, o.ny, o.lon, o.lat, o.dlat, o.dlon,
                                                o.rect_hint, h->device, st, &pl);
    if (nx == FG_ERR_MAXV) return fg_fail(FG_ERR_GEOM, "fg_coupler_run: an atmosphere x land polygon has more than 8 vertices");
    if (nx < 0) return (int)nx;
    struct Destroy { fg_plan *p; ~Destroy() { fg_plan_destroy(p); } } destroy{pl};
    h->d2h += fg_plan_search_d2h(pl);
    FgPlanView v;
    if (int rc = fg_plan_view(pl, &v)) return rc;
    FgDev tmp;
    const size_t m = (size_t)c.n;
    double *s_area = tmp.get<double>(m), *s_clon = tmp.get<double>(m), *s_clat = tmp.get<double>(m);
    int *flag = tmp.get<int>(m), *offs = nullptr, total = 0;
    if (!s_area || !s_clon || !s_clat || !flag) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    fgd_cp_poly_sums(c.n, nx, v.x_src, v.x_dst, v.x_area, v.x_c1, v.x_c2, h->omask, c.area_ref, h->thresh, s_area, s_clon, s_clat, flag, st);
    if (int rc = scan_total(tmp, c.n, flag, &offs, &total)) return rc;
    if (!alloc_list(out, total)) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    out->n = total;
    fgd_cp_poly_emit(c.n, c.pa, c.pl, s_area, s_clon, s_clat, flag, offs, *out, st);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(st));
    return 0;
  }
  // the terms of a list onto the cells of its first (which = 1) or second grid, in list order
  int row_sums(const CpList &l, int which, long ncells, CpSums s)
  {
    if (l.n == 0) return 0;
    FgDev tmp;
    int *cnt = tmp.get<int>((size_t)ncells), *fill = tmp.get<int>((size_t)ncells), *rowptr = tmp.get<int>((size_t)ncells), *perm = tmp.get<int>((size_t)l.n);
    int *bsum = tmp.get<int>((size_t)fgd_cp_scan_blocks(ncells)), *d_tot = tmp.get<int>(1);
    if (!cnt || !fill || !rowptr || !perm || !bsum || !d_tot) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    FGCHK(hipMemsetAsync(cnt, 0, (size_t)ncells * sizeof(int), st));
    FGCHK(hipMemsetAsync(fill, 0, (size_t)ncells * sizeof(int), st));
    const int *key = which == 1 ? l.c1 : l.c2;
    fgd_cp_row_count(l.n, key, cnt, st);
    fgd_cp_scan(ncells, cnt, rowptr, bsum, d_tot, st);
    fgd_cp_row_fill(l.n, key, rowptr, fill, perm, st);
    fgd_cp_row_sums((int)ncells, rowptr, cnt, perm, l.area, l.clon, l.clat, h->order, s, st);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(st));
    return 0;
  }
  int tile_starts(const CpList &l, std::vector<int> *starts)
  {
    const int nt = (int)h->atm.size();
    FgDev tmp;
    int *d = tmp.get<int>((size_t)nt + 1);
    if (!d) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    fgd_cp_tile_starts(nt, h->d_aoff, l.n, l.c1, d, st);
    FGCHK(hipGetLastError());
    starts->resize((size_t)nt + 1);
    return fetch(starts->data(), d, ((size_t)nt + 1) * sizeof(int));
  }

  int go()
  {
    const int ntl = (int)h->lnd.size();
    d_err = res.get<unsigned>(1); d_nbad = res.get<int>(1);
    if (!d_err || !d_nbad) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    FGCHK(hipMemsetAsync(d_err, 0, sizeof(unsigned), st));
    FGCHK(hipMemsetAsync(d_nbad, 0, sizeof(int), st));
    double t0 = fg_now_ms();
    // 2. atmosphere x land candidates
    std::vector<Cand> cand(ntl);
    const bool same_gc = h->gc && h->same;
    double *same_ref = nullptr;                    // great-circle handle, land on the atmosphere grid: see cand_same_gc
    if (same_gc) {
      same_ref = res.get<double>((size_t)h->na);
      if (!same_ref) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    }
    for (int t = 0; t < ntl; t++) {
      if (same_gc) {
        long count = 0;
        if (int rc = cand_same_gc(t, same_ref + h->atm[t].off, &count)) return rc;
        h->ncand += count;
        continue;
      }
      if (int rc = h->same ? cand_same(t, &cand[t]) : (h->gc ? cand_own_gc(t, &cand[t]) : cand_own(t, &cand[t]))) return rc;
      h->ncand += cand[t].n;
    }
    if (int rc = check_err()) return rc;
    double t1 = fg_now_ms(); h->ms[1] = (float)(t1 - t0); t0 = t1;
    // 3. atmosphere x ocean over sea
    fg_plan *axo_plan = nullptr;
    struct Destroy { fg_plan *&p; ~Destroy() { fg_plan_destroy(p); } } destroy_axo{axo_plan};
    if (int rc = ocean_list((int)h->atm.size(), h->atm, h->area_atm, &h->axo, same_gc ? &axo_plan : nullptr)) return rc;
    t1 = fg_now_ms(); h->ms[2] = (float)(t1 - t0); t0 = t1;
    // 4. the remembered polygons x ocean over land
    h->axl.assign(ntl, CpList{});
    if (same_gc) {
      // the remembered polygon IS the atmosphere cell: its clips against the ocean cells are step 3's pairs, whose unweighted areas the
      // plan still holds (a pair that passes :1678 passes the plan's own test: lnd_frac <= 1, thresh >= 1e-6, min(.., area_ocn) <= area_atm)
      FgPlanView v;
      if (int rc = fg_plan_view(axo_plan, &v)) return rc;
      std::vector<CpList *> outs;
      std::vector<int> first, count;
      for (int t = 0; t < ntl; t++) { outs.push_back(&h->axl[t]); first.push_back(h->atm[t].off); count.push_back((int)h->atm[t].ncells()); }
      if (int rc = poly_tail(h->na, v, same_ref, h->d_iota, h->d_iota, outs, first, count)) return rc;
      fg_plan_destroy(axo_plan); axo_plan = nullptr;
    } else
    for (int t = 0; t < ntl; t++) if (int rc = h->gc ? poly_list_gc(cand[t], &h->axl[t]) : poly_list(cand[t], &h->axl[t])) return rc;
    t1 = fg_now_ms(); h->ms[3] = (float)(t1 - t0); t0 = t1;
    // 5. land x ocean
    h->lxo.assign(h->same ? 0 : ntl, CpList{});
    for (size_t t = 0; t < h->lxo.size(); t++)
      if (int rc = ocean_list(1, std::vector<Grid>{h->lnd[t]}, h->area_lnd + h->lnd[t].off, &h->lxo[t])) return rc;
    t1 = fg_now_ms(); h->ms[4] = (float)(t1 - t0); t0 = t1;
    // 5w. wave x ocean (:3044-3231): the land x ocean step with a wave tile for the land tile, inside the tile's ocean row band
    h->wxo.assign(h->wav.size(), CpList{});
    for (size_t t = 0; t < h->wxo.size(); t++)
      if (int rc = ocean_list(1, std::vector<Grid>{h->wav[t]}, h->area_wav + h->wav[t].off, &h->wxo[t], nullptr, &h->wav_band[t])) return rc;
    if (!h->wav.empty()) { t1 = fg_now_ms(); h->ms[7] = (float)(t1 - t0); t0 = t1; }
    // where the tiles begin in the atmosphere-major lists
    h->axl_start.assign(ntl, std::vector<int>());
    for (int t = 0; t < ntl; t++) if (int rc = tile_starts(h->axl[t], &h->axl_start[t])) return rc;
    if (int rc = tile_starts(h->axo, &h->axo_start)) return rc;
    // 6. per-cell sums
    if (!alloc_sums(&h->a, h->na) || !alloc_sums(&h->l, h->nl) || !alloc_sums(&h->o, h->no) || !alloc_sums(&h->l2, h->nl) || !alloc_sums(&h->o2, h->no))
      return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    h->a_frac = res.get<double>((size_t)h->na); h->l_frac = res.get<double>((size_t)h->nl); h->o_frac = res.get<double>((size_t)h->no);
    if (!h->a_frac || !h->l_frac || !h->o_frac) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
    CpListRefs refs;
    refs.count = 0;
    for (int t = 0; t < ntl; t++) refs.l[refs.count++] = CpListRef{h->axl[t].c1, h->axl[t].area, h->axl[t].clon, h->axl[t].clat, h->axl[t].n};
    refs.l[refs.count++] = CpListRef{h->axo.c1, h->axo.area, h->axo.clon, h->axo.clat, h->axo.n};
    fgd_cp_a_sums(h->na, refs, h->order, h->a, st);
    FGCHK(hipGetLastError());
    if (h->tile_nest >= 0 && h->order == 2) {
      // :1857 and :1903 enclose the a_area / a_clon / a_clat additions of :1882-1885 and :1927-1930 too: the reference's temporary a_area
      // of the nest tile stays 0, :1946-1951 divide nothing, and the nest lists' tile-1 distances are clon / area - 0.  The cell's area
      // sum is kept (it is atm_xarea of :2210 / :2333, which has no guard: fg_coupler_check, a_frac); the centroid is what the
      // distances subtract: 0
      const Grid &g = h->atm[(size_t)h->tile_nest];
      FGCHK(hipMemsetAsync(h->a.clon + g.off, 0, (size_t)g.ncells() * sizeof(double), st));
      FGCHK(hipMemsetAsync(h->a.clat + g.off, 0, (size_t)g.ncells() * sizeof(double), st));
    }
    auto tile = [](CpSums s, int off) { return CpSums{s.area + off, s.clon + off, s.clat + off}; };
    // the terms of an atmosphere-major list onto the cells of its second grid, without the nest tile's (:1765, :1792, :1857, :1903):
    // the list before the nest tile's range, then the list after it, which is the reference's order with that tile skipped
    auto part = [](const CpList &l, long k0, long k1) {
      CpList s = l;
      s.n = k1 - k0; s.c1 += k0; s.c2 += k0; s.area += k0; s.clon += k0; s.clat += k0;
      for (int q = 0; q < 4; q++) s.d[q] += k0;
      return s;
    };
    auto second_grid_sums = [&](const CpList &l, const std::vector<int> &start, long ncells, CpSums s) {
      if (h->tile_nest < 0) return row_sums(l, 2, ncells, s);
      if (int rc = row_sums(part(l, 0, start[(size_t)h->tile_nest]), 2, ncells, s)) return rc;
      return row_sums(part(l, start[(size_t)h->tile_nest + 1], l.n), 2, ncells, s);
    };
    for (int t = 0; t < ntl; t++) if (int rc = second_grid_sums(h->axl[t], h->axl_start[t], h->lnd[t].ncells(), tile(h->l, h->lnd[t].off))) return rc;
    if (int rc = second_grid_sums(h->axo, h->axo_start, h->no, h->o)) return rc;
    for (size_t t = 0; t < h->lxo.size(); t++) {
      if (int rc = row_sums(h->lxo[t], 1, h->lnd[t].ncells(), tile(h->l2, h->lnd[t].off))) return rc;
      if (int rc = row_sums(h->lxo[t], 2, h->no, h->o2)) return rc;
    }
    if (h->order == 2) {
      // 7. centroids where the area is > 0, then the distances
      fgd_cp_centroid(h->nl, h->l, st); fgd_cp_centroid(h->no, h->o, st);
      fgd_cp_centroid(h->nl, h->l2, st); fgd_cp_centroid(h->no, h->o2, st);
      for (int t = 0; t < ntl; t++) fgd_cp_distances(h->axl[t], h->a, tile(h->l, h->lnd[t].off), st);
      fgd_cp_distances(h->axo, h->a, h->o, st);
      for (size_t t = 0; t < h->lxo.size(); t++) fgd_cp_distances(h->lxo[t], tile(h->l2, h->lnd[t].off), h->o2, st);
    }
    // the wave grid's sums (:3237-3402).  Order 1: the reference's loop (:3262-3267) gathers io / jo into g_iw / g_jw and adds into
    // w_area2, which is never allocated -- that statement cannot execute; w_area is formed as the order-2 branch forms it
    // (:3325-3326) and nothing else
    if (!h->wav.empty()) {
      if (!alloc_sums(&h->w, h->nw) || !alloc_sums(&h->ow, h->no)) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
      h->w_frac = res.get<double>((size_t)h->nw);
      if (!h->w_frac) return fg_fail(FG_ERR_HIP, "fg_coupler_run: out of device memory");
      for (size_t t = 0; t < h->wxo.size(); t++) {
        if (int rc = row_sums(h->wxo[t], 1, h->wav[t].ncells(), tile(h->w, h->wav[t].off))) return rc;
        if (h->order == 2) if (int rc = row_sums(h->wxo[t], 2, h->no, h->ow)) return rc;
      }
      if (h->order == 2) {
        fgd_cp_centroid(h->nw, h->w, st); fgd_cp_centroid(h->no, h->ow, st);                  // :3344-3349, :3366-3371
        for (size_t t = 0; t < h->wxo.size(); t++) fgd_cp_distances(h->wxo[t], tile(h->w, h->wav[t].off), h->ow, st);
      }
      fgd_cp_fraction(h->nw, h->w.area, h->area_wav, nullptr, 0, h->w_frac, nullptr, st);     // :3397-3402
    }
    // 8. masks
    fgd_cp_fraction(h->na, h->a.area, h->area_atm, nullptr, 0, h->a_frac, nullptr, st);
    fgd_cp_fraction(h->nl, h->l.area, h->area_lnd, nullptr, 0, h->l_frac, nullptr, st);
    fgd_cp_fraction(h->no, h->o.area, h->area_ocn, h->omask, h->south_ext * h->ocn.nx, h->o_frac, d_nbad, st);
    FGCHK(hipGetLastError());
    if (int rc = fetch(&h->nbad, d_nbad, sizeof(int))) return rc;
    h->ms[5] = (float)(fg_now_ms() - t0);
    return 0;
  }
};
}  // namespace

extern "C" int fg_coupler_run(fg_coupler *h)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_coupler_run: null handle");
  FGCHK(hipSetDevice(h->device));
  FGCHK(hipStreamSynchronize(h->stream));
  const double t0 = fg_now_ms();
  h->ran = false;
  h->res.reset(new FgDev);
  h->d2h = 0; h->searches = 0; h->ncand = 0; h->nbad = 0;
  Run r{h, *h->res, h->stream};
  // legacy: fix_lon(cell, xa_avg) per pair (:1455, :1597, :2652), for this thread's searches only; unit vectors have no frame
  const int saved = h->gc ? 0 : fg_search_frame_override(1);
  const int rc = r.go();
  if (!h->gc) fg_search_frame_override(saved);
  if (rc) { (void)hipStreamSynchronize(h->stream); h->res.reset(); return rc; }
  h->ran = true;
  h->ms[6] = (float)(fg_now_ms() - t0);
  return 0;
}

// which: 0 atmosphere x land (tile1 = atmosphere tile, tile2 = land tile), 1 atmosphere x ocean (tile1), 2 land x ocean (tile1 = land tile),
// 3 wave x ocean (tile1 = wave tile)
static int cp_pick(const fg_coupler *h, const char *who, int which, int t1, int t2, const CpList **l, long *k0, long *n, int *off1, int *nx1, int *nx2)
{
  if (!h) return fg_fail(FG_ERR_ARG, "%s: null handle", who);
  if (!h->ran) return fg_fail(FG_ERR_STATE, "%s: fg_coupler_run has not run on this handle", who);
  const int nta = (int)h->atm.size(), ntl = (int)h->lnd.size();
  if (which == 0) {
    if (t1 < 0 || t1 >= nta || t2 < 0 || t2 >= ntl) return fg_fail(FG_ERR_ARG, "%s: no atmosphere tile %d x land tile %d", who, t1, t2);
    *l = &h->axl[t2]; *k0 = h->axl_start[t2][t1]; *n = h->axl_start[t2][t1 + 1] - *k0;
    *off1 = h->atm[t1].off; *nx1 = h->atm[t1].nx; *nx2 = h->lnd[t2].nx;
  } else if (which == 1) {
    if (t1 < 0 || t1 >= nta || t2 != 0) return fg_fail(FG_ERR_ARG, "%s: no atmosphere tile %d x ocean tile %d", who, t1, t2);
    *l = &h->axo; *k0 = h->axo_start[t1]; *n = h->axo_start[t1 + 1] - *k0;
    *off1 = h->atm[t1].off; *nx1 = h->atm[t1].nx; *nx2 = h->ocn.nx;
  } else if (which == 2) {
    if (t2 != 0 || t1 < 0 || (!h->same && t1 >= ntl)) return fg_fail(FG_ERR_ARG, "%s: no land tile %d x ocean tile %d", who, t1, t2);
    if (h->same) return fg_fail(FG_ERR_ARG, "%s: land is on the atmosphere grid: there is no land x ocean list", who);
    *l = &h->lxo[t1]; *k0 = 0; *n = h->lxo[t1].n;
    *off1 = 0; *nx1 = h->lnd[t1].nx; *nx2 = h->ocn.nx;
  } else if (which == 3) {
    if (h->wav.empty()) return fg_fail(FG_ERR_ARG, "%s: the handle has no wave grid", who);
    if (t2 != 0 || t1 < 0 || t1 >= (int)h->wav.size()) return fg_fail(FG_ERR_ARG, "%s: no wave tile %d x ocean tile %d", who, t1, t2);
    *l = &h->wxo[t1]; *k0 = 0; *n = h->wxo[t1].n;
    *off1 = 0; *nx1 = h->wav[t1].nx; *nx2 = h->ocn.nx;
  } else return fg_fail(FG_ERR_ARG, "%s: which must be 0 (atmosphere x land), 1 (atmosphere x ocean), 2 (land x ocean) or 3 (wave x ocean)", who);
  return 0;
}

extern "C" long fg_coupler_count(const fg_coupler *h, int which, int tile1, int tile2)
{
  const CpList *l; long k0, n; int off1, nx1, nx2;
  if (int rc = cp_pick(h, "fg_coupler_count", which, tile1, tile2, &l, &k0, &n, &off1, &nx1, &nx2)) return rc;
  return n;
}

extern "C" int fg_coupler_get(const fg_coupler *h, int which, int tile1, int tile2, int *i1, int *j1, int *i2, int *j2, double *area, double *clon,
                              double *clat, double *di1, double *dj1, double *di2, double *dj2)
{
  const CpList *l; long k0, n; int off1, nx1, nx2;
  if (int rc = cp_pick(h, "fg_coupler_get", which, tile1, tile2, &l, &k0, &n, &off1, &nx1, &nx2)) return rc;
  if (h->order != 2 && (clon || clat || di1 || dj1 || di2 || dj2)) return fg_fail(FG_ERR_ARG, "fg_coupler_get: centroids and distances need interp_order 2");
  if (n == 0) return 0;
  FGCHK(hipSetDevice(h->device));
  if (i1 || j1 || i2 || j2) {
    FgDev tmp;
    int *d = tmp.get<int>(4 * (size_t)n);
    if (!d) return fg_fail(FG_ERR_HIP, "fg_coupler_get: out of device memory");
    fgd_cp_indices(n, l->c1 + k0, l->c2 + k0, off1, nx1, nx2, d, d + n, d + 2 * n, d + 3 * n, h->stream);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(h->stream));
    int *dst[4] = {i1, j1, i2, j2};
    for (int q = 0; q < 4; q++) if (dst[q]) FGCHK(hipMemcpy(dst[q], d + (size_t)q * n, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  }
  const double *src[7] = {l->area, l->clon, l->clat, l->d[0], l->d[1], l->d[2], l->d[3]};
  double *dst[7] = {area, clon, clat, di1, dj1, di2, dj2};
  for (int q = 0; q < 7; q++) if (dst[q]) FGCHK(hipMemcpy(dst[q], src[q] + k0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// grid: 0 atmosphere, 1 land, 2 ocean (tile 0), 3 wave (frac: the wave mask w_area / area_wav, :3397-3402).  model_area: get_grid_area; xarea: the exchange-cell area the cell collected
// (a_area, l_area, o_area); frac = xarea / model_area (the land and ocean masks of :2037, :2089); clon / clat: the cell's centroid
// (order 2; the plain sums where xarea is not > 0)
extern "C" int fg_coupler_get_cells(const fg_coupler *h, int grid, int tile, double *model_area, double *xarea, double *frac, double *clon, double *clat)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_coupler_get_cells: null handle");
  if (!h->ran) return fg_fail(FG_ERR_STATE, "fg_coupler_get_cells: fg_coupler_run has not run on this handle");
  const std::vector<Grid> one{h->ocn};
  const std::vector<Grid> &g = grid == 0 ? h->atm : (grid == 1 ? h->lnd : (grid == 3 ? h->wav : one));
  if (grid < 0 || grid > 3 || tile < 0 || tile >= (int)g.size()) return fg_fail(FG_ERR_ARG, "fg_coupler_get_cells: no tile %d of grid %d", tile, grid);
  if (h->order != 2 && (clon || clat)) return fg_fail(FG_ERR_ARG, "fg_coupler_get_cells: centroids need interp_order 2");
  const int off = grid == 2 ? 0 : g[tile].off;
  const size_t bytes = (size_t)g[tile].ncells() * sizeof(double);
  const CpSums &s = grid == 0 ? h->a : (grid == 1 ? h->l : (grid == 3 ? h->w : h->o));
  const double *src[5] = {grid == 0 ? h->area_atm : (grid == 1 ? h->area_lnd : (grid == 3 ? h->area_wav : h->area_ocn)), s.area,
                          grid == 0 ? h->a_frac : (grid == 1 ? h->l_frac : (grid == 3 ? h->w_frac : h->o_frac)), s.clon, s.clat};
  double *dst[5] = {model_area, xarea, frac, clon, clat};
  FGCHK(hipSetDevice(h->device));
  for (int q = 0; q < 5; q++) if (dst[q]) FGCHK(hipMemcpy(dst[q], src[q] + off, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// The ocean cells' wave-side sums (:3329-3332, :3366-3371; order 2 only -- at order 1 the reference forms none): the exchange area the
// wave x ocean lists left on every ocean cell and its centroid.  They are not the atmosphere-side o_area of fg_coupler_get_cells.
extern "C" int fg_coupler_get_wave_ocean(const fg_coupler *h, double *xarea, double *clon, double *clat)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_coupler_get_wave_ocean: null handle");
  if (!h->ran) return fg_fail(FG_ERR_STATE, "fg_coupler_get_wave_ocean: fg_coupler_run has not run on this handle");
  if (h->wav.empty()) return fg_fail(FG_ERR_ARG, "fg_coupler_get_wave_ocean: the handle has no wave grid");
  if (h->order != 2) return fg_fail(FG_ERR_ARG, "fg_coupler_get_wave_ocean: the ocean cells' wave-side sums need interp_order 2");
  const double *src[3] = {h->ow.area, h->ow.clon, h->ow.clat};
  double *dst[3] = {xarea, clon, clat};
  FGCHK(hipSetDevice(h->device));
  for (int q = 0; q < 3; q++) if (dst[q]) FGCHK(hipMemcpy(dst[q], src[q], (size_t)h->no * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// --check (:2199-2219, :2326-2342, :3504, :3591-3661).  out: [0] the largest |atm_xarea - area_atm| / area_atm  [1] its tile  [2] i  [3] j
// (the first cell with that ratio, as the `>` of :3619 picks it; -1 when no cell has a ratio)  [4] area_atm and [5] atm_xarea there
// [6] atm_area_sum  [7] axl_area_sum  [8] axo_area_sum  [9] ocean and [10] land percentage  [11] the tiling error in percent
// [12 .. 17] the same six for the nest tile (0 without one)  [18] wxo_area_sum (0 without a wave grid).
// atm_xarea is a_area: the land lists' terms, then the ocean list's, in list order (:2210, :2333) -- the argmax is one device
// reduction.  The scalar sums depend on the order of millions of terms: the area columns are brought to the host and added there
// in the reference's order.  Nothing here is counted in fg_coupler_stats' bytes: those are fg_coupler_run's.
#define CP_CHECK_N 19
extern "C" int fg_coupler_check(const fg_coupler *h, double *out, int n)
{
  if (!h || !out || n < 0) return fg_fail(FG_ERR_ARG, "fg_coupler_check: bad argument");
  if (!h->ran) return fg_fail(FG_ERR_STATE, "fg_coupler_check: fg_coupler_run has not run on this handle");
  FGCHK(hipSetDevice(h->device));
  double v[CP_CHECK_N] = {0};
  const int nta = (int)h->atm.size(), ntl = (int)h->lnd.size();
  {
    FgDev tmp;
    const size_t nb = (size_t)fgd_cp_check_blocks(h->na);
    double *sc_r = tmp.get<double>(nb), *d_best = tmp.get<double>(1);
    int *sc_c = tmp.get<int>(nb), *d_cell = tmp.get<int>(1);
    if (!sc_r || !sc_c || !d_best || !d_cell) return fg_fail(FG_ERR_HIP, "fg_coupler_check: out of device memory");
    fgd_cp_check_ratio(h->na, h->a.area, h->area_atm, sc_r, sc_c, d_best, d_cell, h->stream);
    FGCHK(hipGetLastError());
    FGCHK(hipStreamSynchronize(h->stream));
    int cell = -1;
    FGCHK(hipMemcpy(&v[0], d_best, sizeof(double), hipMemcpyDeviceToHost));
    FGCHK(hipMemcpy(&cell, d_cell, sizeof(int), hipMemcpyDeviceToHost));
    v[1] = v[2] = v[3] = -1;
    for (int t = 0; t < nta && cell >= 0; t++) {
      const Grid &g = h->atm[t];
      if (cell < g.off || cell >= g.off + g.ncells()) continue;
      v[1] = t; v[2] = (cell - g.off) % g.nx; v[3] = (cell - g.off) / g.nx;                  // :3621-3623
      FGCHK(hipMemcpy(&v[4], h->area_atm + cell, sizeof(double), hipMemcpyDeviceToHost));
      FGCHK(hipMemcpy(&v[5], h->a.area + cell, sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  std::vector<double> col;
  auto column = [&](const double *d, long m) {
    col.resize((size_t)(m > 0 ? m : 1));
    if (m > 0 && hipMemcpy(col.data(), d, (size_t)m * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return fg_fail(FG_ERR_HIP, "fg_coupler_check: copying an area column failed");
    return 0;
  };
  if (int rc = column(h->area_atm, h->na)) return rc;
  for (int t = 0; t < nta; t++) {                                          // :3636-3641
    double &s = t == h->tile_nest ? v[12] : v[6];
    for (long c = h->atm[t].off; c < h->atm[t].off + h->atm[t].ncells(); c++) s += col[(size_t)c];
  }
  {
    std::vector<std::vector<double>> axl((size_t)ntl);
    for (int l = 0; l < ntl; l++) { if (int rc = column(h->axl[l].area, h->axl[l].n)) return rc; axl[(size_t)l] = col; }
    for (int t = 0; t < nta; t++)                                          // :2215-2218: atmosphere tile, land tile, list order
      for (int l = 0; l < ntl; l++) {
        double &s = t == h->tile_nest ? v[13] : v[7];
        for (int k = h->axl_start[l][t]; k < h->axl_start[l][t + 1]; k++) s += axl[(size_t)l][(size_t)k];
      }
  }
  if (int rc = column(h->axo.area, h->axo.n)) return rc;
  for (int t = 0; t < nta; t++) {                                          // :2338-2341
    double &s = t == h->tile_nest ? v[14] : v[8];
    for (int k = h->axo_start[t]; k < h->axo_start[t + 1]; k++) s += col[(size_t)k];
  }
  v[9] = v[8] / v[6] * 100;                                                // :3642-3644
  v[10] = v[7] / v[6] * 100;
  v[11] = (v[6] - v[8] - v[7]) / v[6] * 100;
  if (h->tile_nest >= 0) {                                                 // :3653-3655
    v[15] = v[14] / v[12] * 100;
    v[16] = v[13] / v[12] * 100;
    v[17] = (v[12] - v[14] - v[13]) / v[12] * 100;
  }
  for (const CpList &l : h->wxo) {                                         // :3504: wave tile, list order
    if (int rc = column(l.area, l.n)) return rc;
    for (long k = 0; k < l.n; k++) v[18] += col[(size_t)k];
  }
  for (int k = 0; k < n && k < CP_CHECK_N; k++) out[k] = v[k];
  return 0;
}

// s: [0] bytes fg_coupler_run brought to the host  [1] nbad (:2038)  [2] searches  [3] atmosphere x ocean cells  [4] atmosphere x land
// cells  [5] land x ocean cells  [6] remembered atmosphere x land polygons  [7] ocn_south_ext  [8] wave x ocean cells
extern "C" int fg_coupler_stats(const fg_coupler *h, long *s, int n)
{
  if (!h || !s || n < 0) return fg_fail(FG_ERR_ARG, "fg_coupler_stats: bad argument");
  long naxl = 0, nlxo = 0, nwxo = 0;
  for (const CpList &l : h->axl) naxl += l.n;
  for (const CpList &l : h->lxo) nlxo += l.n;
  for (const CpList &l : h->wxo) nwxo += l.n;
  const long v[9] = {h->d2h, h->nbad, h->searches, h->ran ? h->axo.n : 0, h->ran ? naxl : 0, h->ran ? nlxo : 0, h->ncand, h->south_ext,
                     h->ran ? nwxo : 0};
  for (int k = 0; k < n && k < 9; k++) s[k] = v[k];
  return 0;
}

extern "C" int fg_coupler_phase_ms(const fg_coupler *h, float *ms, int n)
{
  if (!h || !ms || n < 0) return fg_fail(FG_ERR_ARG, "fg_coupler_phase_ms: bad argument");
  for (int k = 0; k < n && k < 8; k++) ms[k] = h->ms[k];
  return 0;
}

// ------------------------------------------------------------------------------------------------------------- the files
namespace {
enum { CP_NC_CHAR = 2, CP_NC_INT = 4, CP_NC_DOUBLE = 6, CP_STRING = 255 };      // netcdf.h's codes; mpp.h's STRING
struct NcClose { fg_ncfile *f = nullptr; ~NcClose() { if (f) (void)fg_nc_close(f); } };
int nc_fail(const char *what) { return fg_fail(FG_ERR_IO, "fg_coupler_write: %s: %s", what, fg_nc_last_error()); }
int nc_var(fg_ncfile *f, const char *name, int type, int ndims, const int *dims, std::initializer_list<std::pair<const char *, const char *>> atts)
{
  const int v = fg_nc_def_var(f, name, type, ndims, dims);
  if (v < 0) return v;
  for (const auto &a : atts) if (fg_nc_put_att_text(f, v, a.first, a.second) < 0) return -1;
  return v;
}
}  // namespace

// One exchange-grid file from host arrays (:2158-2244, :2277-2370, :2840-2920): 0-based (i, j) of the two grids' cells, written as
// i + 1, j1 + 1, j2 + j2_shift (1, or 1 - ocn_south_ext for an ocean second grid: :2309, :2876); di1 .. dj2 all given (order 2) or all NULL.
// std1 / std2: the standard_name of tile1_cell / tile2_cell (the wave x ocean files have their own, :3476-3477)
static int cp_xgrid_file(const char *std1, const char *std2, const char *path_, const char *contact_, long n, const int *i1, const int *j1,
                         const int *i2, const int *j2, int j2_shift, const double *area_, const double *di1, const double *dj1, const double *di2,
                         const double *dj2)
{
  if (!path_ || !contact_ || n < 1 || !i1 || !j1 || !i2 || !j2 || !area_) return fg_fail(FG_ERR_ARG, "fg_coupler_write_xgrid: bad argument (an empty list gets no file)");
  const bool o2 = di1 != nullptr;
  if ((dj1 != nullptr) != o2 || (di2 != nullptr) != o2 || (dj2 != nullptr) != o2) return fg_fail(FG_ERR_ARG, "fg_coupler_write_xgrid: four distance arrays or none");
  const std::string path(path_), contact(contact_);
  const int *idx[4] = {i1, j1, i2, j2};
  const double *d[4] = {di1, dj1, di2, dj2}, *area = area_;
  std::vector<int> cell(2 * (size_t)n);
  std::vector<double> pair(o2 ? 2 * (size_t)n : 0);
  NcClose c;
  if (fg_nc_create(path.c_str(), 2, &c.f) < 0) return nc_fail(path.c_str());
  fg_ncfile *f = c.f;
  const int d_str = fg_nc_def_dim(f, "string", CP_STRING), d_n = fg_nc_def_dim(f, "ncells", n), d_two = fg_nc_def_dim(f, "two", 2);
  if (d_str < 0 || d_n < 0 || d_two < 0) return nc_fail("dimensions");
  const int dims[2] = {d_n, d_two};
  const int v_contact = o2
    ? nc_var(f, "contact", CP_NC_CHAR, 1, &d_str, {{"standard_name", "grid_contact_spec"}, {"contact_type", "exchange"}, {"parent1_cell", "tile1_cell"},
             {"parent2_cell", "tile2_cell"}, {"xgrid_area_field", "xgrid_area"}, {"distant_to_parent1_centroid", "tile1_distance"},
             {"distant_to_parent2_centroid", "tile2_distance"}})
    : nc_var(f, "contact", CP_NC_CHAR, 1, &d_str, {{"standard_name", "grid_contact_spec"}, {"contact_type", "exchange"}, {"parent1_cell", "tile1_cell"},
             {"parent2_cell", "tile2_cell"}, {"xgrid_area_field", "xgrid_area"}});
  const int v_t1 = nc_var(f, "tile1_cell", CP_NC_INT, 2, dims, {{"standard_name", std1}});
  const int v_t2 = nc_var(f, "tile2_cell", CP_NC_INT, 2, dims, {{"standard_name", std2}});
  const int v_area = nc_var(f, "xgrid_area", CP_NC_DOUBLE, 1, &d_n, {{"standard_name", "exchange_grid_area"}, {"units", "m2"}});
  int v_d1 = 0, v_d2 = 0;
  if (o2) {
    v_d1 = nc_var(f, "tile1_distance", CP_NC_DOUBLE, 2, dims, {{"standard_name", "distance_from_parent1_cell_centroid"}});
    v_d2 = nc_var(f, "tile2_distance", CP_NC_DOUBLE, 2, dims, {{"standard_name", "distance_from_parent2_cell_centroid"}});
  }
  if (v_contact < 0 || v_t1 < 0 || v_t2 < 0 || v_area < 0 || v_d1 < 0 || v_d2 < 0 || fg_nc_enddef(f) < 0) return nc_fail("definitions");
  const long s0[2] = {0, 0}, c_all[2] = {n, 2}, c_text[1] = {CP_STRING};
  char text[CP_STRING] = {0};
  memcpy(text, contact.c_str(), std::min<size_t>(contact.size(), CP_STRING));
  bool ok = fg_nc_put_vara(f, v_contact, s0, c_text, text) >= 0;
  for (long k = 0; k < n; k++) { cell[2 * k] = idx[0][k] + 1; cell[2 * k + 1] = idx[1][k] + 1; }                  // :2185-2190: Fortran indices
  ok = ok && fg_nc_put_vara(f, v_t1, s0, c_all, cell.data()) >= 0;
  for (long k = 0; k < n; k++) { cell[2 * k] = idx[2][k] + 1; cell[2 * k + 1] = idx[3][k] + j2_shift; }
  ok = ok && fg_nc_put_vara(f, v_t2, s0, c_all, cell.data()) >= 0;
  ok = ok && fg_nc_put_vara(f, v_area, s0, c_all, area) >= 0;
  if (o2) {
    for (long k = 0; k < n; k++) { pair[2 * k] = d[0][k]; pair[2 * k + 1] = d[1][k]; }
    ok = ok && fg_nc_put_vara(f, v_d1, s0, c_all, pair.data()) >= 0;
    for (long k = 0; k < n; k++) { pair[2 * k] = d[2][k]; pair[2 * k + 1] = d[3][k]; }
    ok = ok && fg_nc_put_vara(f, v_d2, s0, c_all, pair.data()) >= 0;
  }
  if (!ok) return nc_fail("data");
  fg_ncfile *g = c.f; c.f = nullptr;
  return fg_nc_close(g) < 0 ? nc_fail("close") : 0;
}

extern "C" int fg_coupler_write_xgrid(const char *path, const char *contact, long n, const int *i1, const int *j1, const int *i2, const int *j2,
                                      int j2_shift, const double *area, const double *di1, const double *dj1, const double *di2, const double *dj2)
{
  return cp_xgrid_file("parent_cell_indices_in_mosaic1", "parent_cell_indices_in_mosaic2", path, contact, n, i1, j1, i2, j2, j2_shift, area, di1, dj1,
                       di2, dj2);
}
// a wave x ocean exchange-grid file from host arrays (:3461-3527): the same variables; tile1_cell / tile2_cell carry :3476-3477's names
extern "C" int fg_coupler_write_wave_xgrid(const char *path, const char *contact, long n, const int *iw, const int *jw, const int *io, const int *jo,
                                           int jo_shift, const double *area, const double *diw, const double *djw, const double *dio,
                                           const double *djo)
{
  return cp_xgrid_file("parent1_cell_indices", "parent2_cell_indices", path, contact, n, iw, jw, io, jo, jo_shift, area, diw, djw, dio, djo);
}

// one list of the handle into its file; nothing for an empty list (:2136)
static int cp_write_xgrid(const fg_coupler *h, const std::string &path, const std::string &contact, int which, int t1, int t2, int j2_shift)
{
  const long n = fg_coupler_count(h, which, t1, t2);
  if (n <= 0) return (int)n;
  const bool o2 = h->order == 2;
  std::vector<int> idx(4 * (size_t)n);
  std::vector<double> area((size_t)n), d(o2 ? 4 * (size_t)n : 0);
  double *dp[4] = {o2 ? d.data() : nullptr, o2 ? d.data() + n : nullptr, o2 ? d.data() + 2 * n : nullptr, o2 ? d.data() + 3 * n : nullptr};
  if (int rc = fg_coupler_get(h, which, t1, t2, idx.data(), idx.data() + n, idx.data() + 2 * n, idx.data() + 3 * n, area.data(), nullptr, nullptr, dp[0], dp[1],
                              dp[2], dp[3]))
    return rc;
  return (which == 3 ? fg_coupler_write_wave_xgrid : fg_coupler_write_xgrid)(path.c_str(), contact.c_str(), n, idx.data(), idx.data() + n,
                                                                             idx.data() + 2 * n, idx.data() + 3 * n, j2_shift, area.data(), dp[0], dp[1],
                                                                             dp[2], dp[3]);
}

// ocean_mask.nc (:2055-2066) / land_mask[_tileN].nc (:2103-2117): [ny][nx] doubles, `fields` = {name, standard_name, data}
namespace { struct MaskField { const char *name, *std; const double *data; }; }
static int cp_write_mask(const std::string &path, int nx, int ny, std::initializer_list<MaskField> fields)
{
  NcClose c;
  if (fg_nc_create(path.c_str(), 2, &c.f) < 0) return nc_fail(path.c_str());
  fg_ncfile *f = c.f;
  int dims[2];
  dims[1] = fg_nc_def_dim(f, "nx", nx);
  dims[0] = fg_nc_def_dim(f, "ny", ny);
  if (dims[0] < 0 || dims[1] < 0) return nc_fail("dimensions");
  std::vector<int> ids;
  for (const MaskField &m : fields) {
    if (!m.data) { ids.push_back(-1); continue; }
    const int v = nc_var(f, m.name, CP_NC_DOUBLE, 2, dims, {{"standard_name", m.std}, {"units", "none"}});
    if (v < 0) return nc_fail("definitions");
    ids.push_back(v);
  }
  if (fg_nc_enddef(f) < 0) return nc_fail("definitions");
  const long s0[2] = {0, 0}, cnt[2] = {ny, nx};
  size_t k = 0;
  for (const MaskField &m : fields) { if (m.data && fg_nc_put_vara(f, ids[k], s0, cnt, m.data) < 0) return nc_fail("data"); k++; }
  fg_ncfile *g = c.f; c.f = nullptr;
  return fg_nc_close(g) < 0 ? nc_fail("close") : 0;
}

// names: NULL, or [0] atmosphere, [1] land, [2] ocean mosaic name, then the atmosphere tiles' names, the land tiles' names (as many as
// the handle has land tiles: the atmosphere's count when land is on its grid) and the ocean tile's name; a NULL entry or a NULL table
// gives "atmos_mosaic", "land_mosaic", "ocean_mosaic", "tile<k>".
extern "C" int fg_coupler_write(const fg_coupler *h, const char *directory, const char *const *names)
{
  if (!h || !directory) return fg_fail(FG_ERR_ARG, "fg_coupler_write: bad argument");
  if (!h->ran) return fg_fail(FG_ERR_STATE, "fg_coupler_write: fg_coupler_run has not run on this handle");
  const int nta = (int)h->atm.size(), ntl = (int)h->lnd.size();
  auto name = [&](int k, const std::string &dflt) { return std::string(names && names[k] ? names[k] : dflt.c_str()); };
  const std::string dir = std::string(directory) + "/", am = name(0, "atmos_mosaic"), lm = name(1, "land_mosaic"), omn = name(2, "ocean_mosaic");
  std::vector<std::string> at, lt;
  for (int t = 0; t < nta; t++) at.push_back(name(3 + t, "tile" + std::to_string(t + 1)));
  for (int t = 0; t < ntl; t++) lt.push_back(name(3 + nta + t, "tile" + std::to_string(t + 1)));
  const std::string ot = name(3 + nta + ntl, "tile1");
  const int shift = 1 - h->south_ext;
  for (int ta = 0; ta < nta; ta++) {
    for (int tl = 0; tl < ntl; tl++)
      if (int rc = cp_write_xgrid(h, dir + am + "_" + at[ta] + "X" + lm + "_" + lt[tl] + ".nc", am + ":" + at[ta] + "::" + lm + ":" + lt[tl], 0, ta, tl, 1)) return rc;
    if (int rc = cp_write_xgrid(h, dir + am + "_" + at[ta] + "X" + omn + "_" + ot + ".nc", am + ":" + at[ta] + "::" + omn + ":" + ot, 1, ta, 0, shift)) return rc;
  }
  if (!h->same)
    for (int tl = 0; tl < ntl; tl++)
      if (int rc = cp_write_xgrid(h, dir + lm + "_" + lt[tl] + "X" + omn + "_" + ot + ".nc", lm + ":" + lt[tl] + "::" + omn + ":" + ot, 2, tl, 0, shift)) return rc;
  {
    const size_t n = (size_t)h->no, skip = (size_t)h->south_ext * h->ocn.nx;
    std::vector<double> area(n), xarea(n), frac(n);
    if (int rc = fg_coupler_get_cells(h, 2, 0, area.data(), xarea.data(), frac.data(), nullptr, nullptr)) return rc;
    if (int rc = fg_coupler_write_mask((dir + "ocean_mask.nc").c_str(), 1, h->ocn.nx, h->ocn.ny - h->south_ext, frac.data() + skip, area.data() + skip,
                                       xarea.data() + skip, nullptr)) return rc;
  }
  for (int tl = 0; tl < ntl; tl++) {
    const Grid &g = h->lnd[tl];
    const size_t n = (size_t)g.ncells();
    std::vector<double> area(n), xarea(n), frac(n), aatm;
    if (int rc = fg_coupler_get_cells(h, 1, tl, area.data(), xarea.data(), frac.data(), nullptr, nullptr)) return rc;
    if (h->same) {                       // (with land of its own the reference indexes area_atm with the land tile, :2094: left out)
      aatm.resize(n);
      if (int rc = fg_coupler_get_cells(h, 0, tl, aatm.data(), nullptr, nullptr, nullptr, nullptr)) return rc;
    }
    const std::string file = ntl > 1 ? "land_mask_tile" + std::to_string(tl + 1) + ".nc" : std::string("land_mask.nc");
    if (int rc = fg_coupler_write_mask((dir + file).c_str(), 0, g.nx, g.ny, frac.data(), area.data(), xarea.data(), h->same ? aatm.data() : nullptr)) return rc;
  }
  return 0;
}

// ocean_mask.nc (ocean != 0: a = areaO, b = areaX) or a land mask file (a = area_lnd, b = l_area, area_atm or NULL) from host arrays [ny][nx]
extern "C" int fg_coupler_write_mask(const char *path, int ocean, int nx, int ny, const double *mask, const double *a, const double *b, const double *area_atm)
{
  if (!path || nx < 1 || ny < 1 || !mask || !a || !b) return fg_fail(FG_ERR_ARG, "fg_coupler_write_mask: bad argument");
  if (ocean) return cp_write_mask(path, nx, ny, {{"mask", "ocean fraction at T-cell centers", mask}, {"areaO", "ocean grid area", a}, {"areaX", "ocean exchange grid area", b}});
  return cp_write_mask(path, nx, ny, {{"mask", "land fraction at T-cell centers", mask}, {"area_atm", "area atm ", area_atm}, {"area_lnd", "area land ", a},
                                      {"l_area", "land x area", b}});
}

// wave_mask.nc / wave_mask_tileN.nc (:3405-3419) from a host array [ny][nx]: the single variable mask
extern "C" int fg_coupler_write_wave_mask(const char *path, int nx, int ny, const double *mask)
{
  if (!path || nx < 1 || ny < 1 || !mask) return fg_fail(FG_ERR_ARG, "fg_coupler_write_wave_mask: bad argument");
  return cp_write_mask(path, nx, ny, {{"mask", "land/sea fraction at T-cell centers", mask}});
}

// The wave grid's files (:3397-3421, :3430-3535).  names: NULL, or [0] the wave, [1] the ocean mosaic name, then the wave tiles' names
// and the ocean tile's name; a NULL entry or a NULL table gives "wave_mosaic", "ocean_mosaic", "tile<k>".  fg_coupler_write's name table
// is not touched.  With wav_same_as_ocn the exchange-grid files are named wav_<mosaic>_<tile>Xocn_<mosaic>_<tile>.nc (:3452-3455).
extern "C" int fg_coupler_write_wave(const fg_coupler *h, const char *directory, const char *const *names)
{
  if (!h || !directory) return fg_fail(FG_ERR_ARG, "fg_coupler_write_wave: bad argument");
  if (h->wav.empty()) return fg_fail(FG_ERR_ARG, "fg_coupler_write_wave: the handle has no wave grid");
  if (!h->ran) return fg_fail(FG_ERR_STATE, "fg_coupler_write_wave: fg_coupler_run has not run on this handle");
  const int ntw = (int)h->wav.size();
  auto name = [&](int k, const std::string &dflt) { return std::string(names && names[k] ? names[k] : dflt.c_str()); };
  const std::string dir = std::string(directory) + "/", wm = name(0, "wave_mosaic"), omn = name(1, "ocean_mosaic"), ot = name(2 + ntw, "tile1");
  for (int tw = 0; tw < ntw; tw++) {
    const std::string wt = name(2 + tw, "tile" + std::to_string(tw + 1));
    const std::string file = h->wav_same ? "wav_" + wm + "_" + wt + "Xocn_" + omn + "_" + ot + ".nc" : wm + "_" + wt + "X" + omn + "_" + ot + ".nc";
    if (int rc = cp_write_xgrid(h, dir + file, wm + ":" + wt + "::" + omn + ":" + ot, 3, tw, 0, 1 - h->south_ext)) return rc;      // :3492
    const Grid &g = h->wav[tw];
    std::vector<double> frac((size_t)g.ncells());
    if (int rc = fg_coupler_get_cells(h, 3, tw, nullptr, nullptr, frac.data(), nullptr, nullptr)) return rc;
    const std::string mask = ntw > 1 ? "wave_mask_tile" + std::to_string(tw + 1) + ".nc" : std::string("wave_mask.nc");
    if (int rc = fg_coupler_write_wave_mask((dir + mask).c_str(), g.nx, g.ny, frac.data())) return rc;
  }
  return 0;
}
