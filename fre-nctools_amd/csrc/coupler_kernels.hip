// coupler_kernels.hip -- device side of make_coupler_mosaic's exchange grids (coupler.h; host: coupler.hip; design: DESIGN.md 3.13).
// The searches are plans (plan.hip); the kernels here are what the tool does with their lists: the ocean- and land-fraction
// weights and the two acceptance tests, the compaction of the survivors in the reference's order, the ordered per-polygon and
// per-cell sums, the centroid distances and the masks.  Every sum that the reference forms one term after another is formed by
// ONE lane in that order; rows are found with integer atomics and sorted, never summed with floating-point atomics.
#include "coupler.h"
#include "geom.hip.h"

static inline unsigned cp_blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

// ------------------------------------------------------------------------------------------------- exclusive scan of ints
// three launches: the sum of every tile of CP_TILE values, the scan of those sums by one block, the tiles rescanned from their base
#define CP_TILE 2048
#define CP_ITEMS 8
long fgd_cp_scan_blocks(long n) { return (n + CP_TILE - 1) / CP_TILE + 1; }

__device__ __forceinline__ int cp_block_exscan(int v, int *sh, int *block_total)
{
  // 256 lanes: exclusive scan of v over the block (Hillis-Steele on LDS)
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const int incl = sh[t];
  if (block_total) *block_total = sh[255];
  __syncthreads();
  return incl - v;
}
__global__ __launch_bounds__(256) void k_cp_tile_sums(long n, const int *in, int *bsum)
{
  __shared__ int sh[256];
  const long base = (long)blockIdx.x * CP_TILE + (long)threadIdx.x * CP_ITEMS;
  int s = 0;
  for (int q = 0; q < CP_ITEMS; q++) if (base + q < n) s += in[base + q];
  int tot;
  cp_block_exscan(s, sh, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void k_cp_scan_sums(long nb, int *bsum, int *total)
{
  __shared__ int sh[256];
  int carry = 0;
  for (long b0 = 0; b0 < nb; b0 += 256) {
    const long b = b0 + threadIdx.x;
    const int v = b < nb ? bsum[b] : 0;
    int tot;
    const int ex = cp_block_exscan(v, sh, &tot);
    if (b < nb) bsum[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(256) void k_cp_tile_scan(long n, const int *in, const int *bsum, int *offs)
{
  __shared__ int sh[256];
  const long base = (long)blockIdx.x * CP_TILE + (long)threadIdx.x * CP_ITEMS;
  int v[CP_ITEMS], s = 0;
  for (int q = 0; q < CP_ITEMS; q++) { v[q] = base + q < n ? in[base + q] : 0; s += v[q]; }
  int run = bsum[blockIdx.x] + cp_block_exscan(s, sh, nullptr);
  for (int q = 0; q < CP_ITEMS; q++) if (base + q < n) { offs[base + q] = run; run += v[q]; }
}
void fgd_cp_scan(long n, const int *in, int *offs, int *bsum, int *total, hipStream_t st)
{
  if (n <= 0) { (void)hipMemsetAsync(total, 0, sizeof(int), st); return; }
  const long nb = (n + CP_TILE - 1) / CP_TILE;
  k_cp_tile_sums<<<(unsigned)nb, 256, 0, st>>>(n, in, bsum);
  k_cp_scan_sums<<<1, 256, 0, st>>>(nb, bsum, total);
  k_cp_tile_scan<<<(unsigned)nb, 256, 0, st>>>(n, in, bsum, offs);
}

// ------------------------------------------------------------------------------- land on the atmosphere grid (:1378-1394, :1444-1477)
// The atmosphere cell after fix_lon(pi) gives xa_min, xa_max, xa_avg; the "land" cell is the same corners after fix_lon(xa_avg).
// Returns the count of the land copy (0: the pair is skipped by one of the reference's tests), the polygon in xl / yl.
__device__ inline int d_same_cell(int nx, const double *lon, const double *lat, int c, double *xl, double *yl, double *xa_avg, unsigned *err)
{
  const int j = c / nx, i = c - j * nx;
  const long n0 = (long)j * (nx + 1) + i, n1 = n0 + 1, n2 = (long)(j + 1) * (nx + 1) + i + 1, n3 = n2 - 1;
  double xa[G_FIXCAP], ya[G_FIXCAP];
  xa[0] = lon[n0]; xa[1] = lon[n1]; xa[2] = lon[n2]; xa[3] = lon[n3];
  ya[0] = lat[n0]; ya[1] = lat[n1]; ya[2] = lat[n2]; ya[3] = lat[n3];
  for (int q = 0; q < 4; q++) { xl[q] = xa[q]; yl[q] = ya[q]; }
  double y_min = ya[0], y_max = ya[0];                                    // minval_double / maxval_double (mosaic_util.c)
  for (int q = 1; q < 4; q++) { if (ya[q] < y_min) y_min = ya[q]; if (ya[q] > y_max) y_max = ya[q]; }
  const int na_in = d_fix_lon(xa, ya, 4, G_PI);
  if (na_in < 0) { atomicOr(err, CP_ERR_MAXV); return 0; }
  double xa_min = xa[0], xa_max = xa[0], avg = 0;
  for (int q = 1; q < na_in; q++) { if (xa[q] < xa_min) xa_min = xa[q]; if (xa[q] > xa_max) xa_max = xa[q]; }
  for (int q = 0; q < na_in; q++) avg += xa[q];
  avg /= na_in;
  *xa_avg = avg;
  if (y_min >= y_max || y_max <= y_min) return 0;                          // :1454 with yl == ya
  const int nl_in = d_fix_lon(xl, yl, 4, avg);
  if (nl_in < 0) { atomicOr(err, CP_ERR_MAXV); return 0; }
  double xl_min = xl[0], xl_max = xl[0];
  for (int q = 1; q < nl_in; q++) { if (xl[q] < xl_min) xl_min = xl[q]; if (xl[q] > xl_max) xl_max = xl[q]; }
  if (xa_min >= xl_max || xa_max <= xl_min) return 0;                      // :1462
  if (na_in != nl_in) { atomicOr(err, CP_ERR_NVERT); return 0; }           // :1465
  if (nl_in > G_MAXV) { atomicOr(err, CP_ERR_MAXV); return 0; }
  return nl_in;
}
__global__ __launch_bounds__(64) void k_cp_same_flag(int nx, int ny, const double *lon, const double *lat, const double *area, double thresh,
                                                      int *flag, unsigned *err)
{
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= nx * ny) return;
  double xl[G_FIXCAP], yl[G_FIXCAP], xa_avg;
  const int n = d_same_cell(nx, lon, lat, c, xl, yl, &xa_avg, err);
  int keep = 0;
  if (n > 0) {
    const double xarea = d_poly_area<1>(xl, yl, n);                        // :1487
    const double min_area = CP_MIN(area[c], area[c]);                      // :1488, area_lnd is area_atm here
    keep = xarea / min_area > thresh;                                      // :1507
  }
  flag[c] = keep;
}
__global__ __launch_bounds__(64) void k_cp_same_emit(int nx, int ny, const double *lon, const double *lat, const double *area, const int *flag,
                                                      const int *offs, int cell_off, int *pa, int *pl, int *pn, double *plon, double *plat,
                                                      double *lon_avg, double *area_ref, unsigned *err)
{
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= nx * ny || !flag[c]) return;
  double xl[G_FIXCAP], yl[G_FIXCAP], xa_avg;
  const int n = d_same_cell(nx, lon, lat, c, xl, yl, &xa_avg, err);
  const int k = offs[c];
  pa[k] = cell_off + c; pl[k] = c; pn[k] = n;
  for (int q = 0; q < 8; q++) { plon[(size_t)k * 8 + q] = q < n ? xl[q] : 0.0; plat[(size_t)k * 8 + q] = q < n ? yl[q] : 0.0; }
  lon_avg[k] = xa_avg;
  area_ref[k] = CP_MIN(area[c], area[c]);
}
void fgd_cp_same_flag(int nx, int ny, const double *lon, const double *lat, const double *area, double thresh, int *flag, unsigned *err,
                      hipStream_t st)
{
  k_cp_same_flag<<<cp_blocks((long)nx * ny, 64), 64, 0, st>>>(nx, ny, lon, lat, area, thresh, flag, err);
}
void fgd_cp_same_emit(int nx, int ny, const double *lon, const double *lat, const double *area, const int *flag, const int *offs, int cell_off,
                      int *pa, int *pl, int *pn, double *plon, double *plat, double *lon_avg, double *area_ref, unsigned *err, hipStream_t st)
{
  k_cp_same_emit<<<cp_blocks((long)nx * ny, 64), 64, 0, st>>>(nx, ny, lon, lat, area, flag, offs, cell_off, pa, pl, pn, plon, plat, lon_avg,
                                                              area_ref, err);
}

// ------------------------------------------------------------------------------------------ land of its own (:1483-1548)
__global__ __launch_bounds__(256) void k_cp_cand_flag(long n, const int *x_src, const int *x_dst, const double *x_area, const double *area_atm,
                                                       const double *area_lnd, double thresh, int *flag)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double al = area_lnd[x_dst[k]], aa = area_atm[x_src[k]];
  const double min_area = CP_MIN(al, aa);                                  // :1488
  flag[k] = x_area[k] / min_area > thresh;                                 // :1507
}
__global__ __launch_bounds__(256) void k_cp_cand_emit(long n, const int *x_src, const int *x_dst, const int *flag, const int *offs, const int *n_in,
                                                       const double *lon_in, const double *lat_in, const double *src_lon_avg,
                                                       const double *area_atm, const double *area_lnd, int *pa, int *pl, int *pn, double *plon,
                                                       double *plat, double *lon_avg, double *area_ref, unsigned *err)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n || !flag[k]) return;
  const int o = offs[k], a = x_src[k], l = x_dst[k], nv = n_in[k];
  if (nv > G_MAXV) atomicOr(err, CP_ERR_MAXV);
  pa[o] = a; pl[o] = l; pn[o] = nv;
  for (int q = 0; q < 8; q++) { plon[(size_t)o * 8 + q] = lon_in[(size_t)k * 8 + q]; plat[(size_t)o * 8 + q] = lat_in[(size_t)k * 8 + q]; }
  lon_avg[o] = src_lon_avg[a];
  const double al = area_lnd[l], aa = area_atm[a];
  area_ref[o] = CP_MIN(al, aa);                                            // :1677, :1703
}
void fgd_cp_cand_flag(long n, const int *x_src, const int *x_dst, const double *x_area, const double *area_atm, const double *area_lnd,
                      double thresh, int *flag, hipStream_t st)
{
  if (n > 0) k_cp_cand_flag<<<cp_blocks(n, 256), 256, 0, st>>>(n, x_src, x_dst, x_area, area_atm, area_lnd, thresh, flag);
}
void fgd_cp_cand_emit(long n, const int *x_src, const int *x_dst, const int *flag, const int *offs, const int *n_in, const double *lon_in,
                      const double *lat_in, const double *src_lon_avg, const double *area_atm, const double *area_lnd, int *pa, int *pl, int *pn,
                      double *plon, double *plat, double *lon_avg, double *area_ref, unsigned *err, hipStream_t st)
{
  if (n > 0) k_cp_cand_emit<<<cp_blocks(n, 256), 256, 0, st>>>(n, x_src, x_dst, flag, offs, n_in, lon_in, lat_in, src_lon_avg, area_atm, area_lnd,
                                                               pa, pl, pn, plon, plat, lon_avg, area_ref, err);
}

// ------------------------------------------------------------------------------------------ great-circle handle (GREAT_CIRCLE_CLIP)
// the cells of one tile as [cell][4][3] unit vectors, clockwise (:1367-1375): (j, i) (j+1, i) (j+1, i+1) (j, i+1); four [cell] = 4
__global__ __launch_bounds__(256) void k_cp_cells_xyz(int nx, int ny, const double *x, const double *y, const double *z, double *cells, int *four)
{
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nx * ny) return;
  const int j = c / nx, i = c - j * nx;
  const long n[4] = {(long)j * (nx + 1) + i, (long)(j + 1) * (nx + 1) + i, (long)(j + 1) * (nx + 1) + i + 1, (long)j * (nx + 1) + i + 1};
  double *o = cells + (size_t)c * 12;
  for (int q = 0; q < 4; q++) { o[q * 3] = x[n[q]]; o[q * 3 + 1] = y[n[q]]; o[q * 3 + 2] = z[n[q]]; }
  four[c] = 4;
}
// land on the atmosphere grid (:1426-1437): the polygon is the cell, xarea its great_circle_area (:1485); the :1507 test
__global__ __launch_bounds__(256) void k_cp_same_gc_flag(long n, const double *xarea, const double *area, double thresh, int *flag, double *ref)
{
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const double min_area = CP_MIN(area[c], area[c]);                        // :1488, area_lnd is area_atm here
  const int keep = xarea[c] / min_area > thresh;                           // :1507
  flag[c] = keep;
  ref[c] = keep ? min_area : (double)INFINITY;                             // :1677, :1703; not remembered: nothing passes a ratio against it
}
// land of its own (:1517-1534): the survivors of the plan's list with their vertices as unit vectors
__global__ __launch_bounds__(256) void k_cp_cand_emit_gc(long n, const int *x_src, const int *x_dst, const int *flag, const int *offs, const int *n_in,
                                                          const double *x_in, const double *y_in, const double *z_in, const double *area_atm,
                                                          const double *area_lnd, int *pa, int *pl, int *pn, double *px, double *py, double *pz,
                                                          double *area_ref, unsigned *err)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n || !flag[k]) return;
  const int o = offs[k], a = x_src[k], l = x_dst[k], nv = n_in[k];
  if (nv > G_MAXV) atomicOr(err, CP_ERR_MAXV);
  pa[o] = a; pl[o] = l; pn[o] = nv;
  for (int q = 0; q < 8; q++) {
    px[(size_t)o * 8 + q] = x_in[(size_t)k * 8 + q]; py[(size_t)o * 8 + q] = y_in[(size_t)k * 8 + q]; pz[(size_t)o * 8 + q] = z_in[(size_t)k * 8 + q];
  }
  const double al = area_lnd[l], aa = area_atm[a];
  area_ref[o] = CP_MIN(al, aa);                                            // :1677, :1703
}
void fgd_cp_cells_xyz(int nx, int ny, const double *x, const double *y, const double *z, double *cells, int *four, hipStream_t st)
{
  k_cp_cells_xyz<<<cp_blocks((long)nx * ny, 256), 256, 0, st>>>(nx, ny, x, y, z, cells, four);
}
void fgd_cp_same_gc_flag(long n, const double *xarea, const double *area, double thresh, int *flag, double *ref, hipStream_t st)
{
  if (n > 0) k_cp_same_gc_flag<<<cp_blocks(n, 256), 256, 0, st>>>(n, xarea, area, thresh, flag, ref);
}
void fgd_cp_cand_emit_gc(long n, const int *x_src, const int *x_dst, const int *flag, const int *offs, const int *n_in, const double *x_in,
                         const double *y_in, const double *z_in, const double *area_atm, const double *area_lnd, int *pa, int *pl, int *pn,
                         double *px, double *py, double *pz, double *area_ref, unsigned *err, hipStream_t st)
{
  if (n > 0) k_cp_cand_emit_gc<<<cp_blocks(n, 256), 256, 0, st>>>(n, x_src, x_dst, flag, offs, n_in, x_in, y_in, z_in, area_atm, area_lnd, pa, pl, pn,
                                                                  px, py, pz, area_ref, err);
}

// ------------------------------------------------------------------------ a grid x ocean over sea (:1601-1659, :2628, :2660-2686)
__global__ __launch_bounds__(256) void k_cp_ocean_flag(long n, const int *x_src, const int *x_dst, const double *x_area, const double *omask,
                                                        const double *area_ocn, const double *area_src, double thresh, int *flag)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int o = x_dst[k];
  const double ocn_frac = omask[o];
  int keep = 0;
  if (ocn_frac > CP_MIN_AREA_FRAC) {                                       // :1604
    const double xarea = x_area[k] * ocn_frac;                             // :1640
    const double ao = area_ocn[o], as = area_src[x_src[k]];
    const double min_area = CP_MIN(ao, as);                                // :1643
    keep = xarea / min_area > thresh;                                      // :1646
  }
  flag[k] = keep;
}
__global__ __launch_bounds__(256) void k_cp_ocean_emit(long n, const int *x_src, const int *x_dst, const double *x_area, const double *x_c1,
                                                        const double *x_c2, const double *omask, const int *flag, const int *offs, CpList out)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n || !flag[k]) return;
  const int p = offs[k], o = x_dst[k];
  const double ocn_frac = omask[o];
  out.c1[p] = x_src[k]; out.c2[p] = o;
  out.area[p] = x_area[k] * ocn_frac;
  if (x_c1) { out.clon[p] = x_c1[k] * ocn_frac; out.clat[p] = x_c2[k] * ocn_frac; }      // :1654-1655
}
void fgd_cp_ocean_flag(long n, const int *x_src, const int *x_dst, const double *x_area, const double *omask, const double *area_ocn,
                       const double *area_src, double thresh, int *flag, hipStream_t st)
{
  if (n > 0) k_cp_ocean_flag<<<cp_blocks(n, 256), 256, 0, st>>>(n, x_src, x_dst, x_area, omask, area_ocn, area_src, thresh, flag);
}
void fgd_cp_ocean_emit(long n, const int *x_src, const int *x_dst, const double *x_area, const double *x_c1, const double *x_c2,
                       const double *omask, const int *flag, const int *offs, CpList out, hipStream_t st)
{
  if (n > 0) k_cp_ocean_emit<<<cp_blocks(n, 256), 256, 0, st>>>(n, x_src, x_dst, x_area, x_c1, x_c2, omask, flag, offs, out);
}

// first index k in [0, n) with a[k] >= v (a ascending)
__device__ __forceinline__ long d_lower_bound(const int *a, long n, int v)
{
  long lo = 0, hi = n;
  while (lo < hi) { const long mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}

// ------------------------------------------------------------------ remembered polygons x ocean over land (:1662-1719)
// The polygon-list plan is polygon-major with the ocean cells of a polygon ascending: the reference's order for one polygon.
__global__ __launch_bounds__(128) void k_cp_poly_sums(int npoly, long nx, const int *x_src, const int *x_dst, const double *x_area,
                                                       const double *x_c1, const double *x_c2, const double *omask, const double *area_ref,
                                                       double thresh, double *sum_area, double *sum_clon, double *sum_clat, int *flag)
{
  const int l = blockIdx.x * 128 + threadIdx.x;
  if (l >= npoly) return;
  const double min_area = area_ref[l];
  double s_area = 0, s_clon = 0, s_clat = 0;                               // :1521-1525
  const long k1 = d_lower_bound(x_src, nx, l + 1);
  for (long k = d_lower_bound(x_src, nx, l); k < k1; k++) {
    const double lnd_frac = 1 - omask[x_dst[k]];                           // :1602
    if (!(lnd_frac > CP_MIN_AREA_FRAC)) continue;                          // :1662
    const double xarea = x_area[k] * lnd_frac;                             // :1676
    if (xarea / min_area > thresh) {                                       // :1678
      s_area += xarea;                                                     // :1689
      if (x_c1) { s_clon += x_c1[k] * lnd_frac; s_clat += x_c2[k] * lnd_frac; }      // :1691-1692
    }
  }
  sum_area[l] = s_area; sum_clon[l] = s_clon; sum_clat[l] = s_clat;
  flag[l] = s_area / min_area > thresh;                                    // :1706
}
__global__ __launch_bounds__(256) void k_cp_poly_emit(int npoly, const int *pa, const int *pl, const double *sum_area, const double *sum_clon,
                                                       const double *sum_clat, const int *flag, const int *offs, CpList out)
{
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= npoly || !flag[l]) return;
  const int p = offs[l];
  out.c1[p] = pa[l]; out.c2[p] = pl[l];
  out.area[p] = sum_area[l]; out.clon[p] = sum_clon[l]; out.clat[p] = sum_clat[l];
}
void fgd_cp_poly_sums(int npoly, long nx, const int *x_src, const int *x_dst, const double *x_area, const double *x_c1, const double *x_c2,
                      const double *omask, const double *area_ref, double thresh, double *sum_area, double *sum_clon, double *sum_clat, int *flag,
                      hipStream_t st)
{
  if (npoly > 0) k_cp_poly_sums<<<cp_blocks(npoly, 128), 128, 0, st>>>(npoly, nx, x_src, x_dst, x_area, x_c1, x_c2, omask, area_ref, thresh, sum_area,
                                                                     sum_clon, sum_clat, flag);
}
void fgd_cp_poly_emit(int npoly, const int *pa, const int *pl, const double *sum_area, const double *sum_clon, const double *sum_clat,
                      const int *flag, const int *offs, CpList out, hipStream_t st)
{
  if (npoly > 0) k_cp_poly_emit<<<cp_blocks(npoly, 256), 256, 0, st>>>(npoly, pa, pl, sum_area, sum_clon, sum_clat, flag, offs, out);
}

// ------------------------------------------------------------------------------------------- per-cell sums
// An atmosphere cell's terms lie together in every list (the lists are atmosphere-cell major): one lane walks them.
__global__ __launch_bounds__(128) void k_cp_a_sums(int ncells, CpListRefs refs, int order, CpSums a)
{
  const int c = blockIdx.x * 128 + threadIdx.x;
  if (c >= ncells) return;
  double s_area = 0, s_clon = 0, s_clat = 0;
  for (int q = 0; q < refs.count; q++) {
    const CpListRef &r = refs.l[q];
    if (r.n == 0) continue;
    const long k1 = d_lower_bound(r.c1, r.n, c + 1);
    for (long k = d_lower_bound(r.c1, r.n, c); k < k1; k++) {
      s_area += r.area[k];                                                 // :1883, :1928
      if (order == 2) { s_clon += r.clon[k]; s_clat += r.clat[k]; }
    }
  }
  if (order == 2 && s_area > 0) { s_clon /= s_area; s_clat /= s_area; }   // :1946-1951
  a.area[c] = s_area; a.clon[c] = s_clon; a.clat[c] = s_clat;
}
void fgd_cp_a_sums(int ncells, CpListRefs refs, int order, CpSums a, hipStream_t st)
{
  if (ncells > 0) k_cp_a_sums<<<cp_blocks(ncells, 128), 128, 0, st>>>(ncells, refs, order, a);
}

__global__ __launch_bounds__(256) void k_cp_row_count(long n, const int *key, int *cnt)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k < n) atomicAdd(&cnt[key[k]], 1);
}
__global__ __launch_bounds__(256) void k_cp_row_fill(long n, const int *key, const int *rowptr, int *fill, int *perm)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int c = key[k];
  perm[rowptr[c] + atomicAdd(&fill[c], 1)] = (int)k;
}
// one lane per cell: its entries back into list order (insertion sort of the row's slice of perm -- rows hold the few cells of
// the other grid that overlap this one), then the terms added one by one onto what the cell already holds
__global__ __launch_bounds__(128) void k_cp_row_sums(int ncells, const int *rowptr, const int *cnt, int *perm, const double *area,
                                                      const double *clon, const double *clat, int order, CpSums s)
{
  const int c = blockIdx.x * 128 + threadIdx.x;
  if (c >= ncells) return;
  const int m = cnt[c];
  if (m == 0) return;
  int *p = perm + rowptr[c];
  for (int i = 1; i < m; i++) {
    const int v = p[i];
    int j = i - 1;
    while (j >= 0 && p[j] > v) { p[j + 1] = p[j]; j--; }
    p[j + 1] = v;
  }
  double s_area = s.area[c], s_clon = s.clon[c], s_clat = s.clat[c];
  for (int i = 0; i < m; i++) {
    const int k = p[i];
    s_area += area[k];
    if (order == 2) { s_clon += clon[k]; s_clat += clat[k]; }
  }
  s.area[c] = s_area; s.clon[c] = s_clon; s.clat[c] = s_clat;
}
__global__ __launch_bounds__(256) void k_cp_centroid(int ncells, CpSums s)
{
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncells) return;
  const double a = s.area[c];
  if (a > 0) { s.clon[c] /= a; s.clat[c] /= a; }                          // :1978-1981, :1997-2000, :2769-2772, :2791-2794
}
void fgd_cp_row_count(long n, const int *key, int *cnt, hipStream_t st)
{
  if (n > 0) k_cp_row_count<<<cp_blocks(n, 256), 256, 0, st>>>(n, key, cnt);
}
void fgd_cp_row_fill(long n, const int *key, const int *rowptr, int *fill, int *perm, hipStream_t st)
{
  if (n > 0) k_cp_row_fill<<<cp_blocks(n, 256), 256, 0, st>>>(n, key, rowptr, fill, perm);
}
void fgd_cp_row_sums(int ncells, const int *rowptr, const int *cnt, int *perm, const double *area, const double *clon, const double *clat, int order,
                     CpSums s, hipStream_t st)
{
  if (ncells > 0) k_cp_row_sums<<<cp_blocks(ncells, 128), 128, 0, st>>>(ncells, rowptr, cnt, perm, area, clon, clat, order, s);
}
void fgd_cp_centroid(int ncells, CpSums s, hipStream_t st)
{
  if (ncells > 0) k_cp_centroid<<<cp_blocks(ncells, 256), 256, 0, st>>>(ncells, s);
}

// ------------------------------------------------------------------------------------------- distances, masks, getters
__global__ __launch_bounds__(256) void k_cp_distances(CpList l, CpSums s1, CpSums s2)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= l.n) return;
  const int c1 = l.c1[k], c2 = l.c2[k];
  const double a = l.area[k], clon = l.clon[k], clat = l.clat[k];
  l.d[0][k] = clon / a - s1.clon[c1];                                      // :1957
  l.d[1][k] = clat / a - s1.clat[c1];
  l.d[2][k] = clon / a - s2.clon[c2];                                      // :1986
  l.d[3][k] = clat / a - s2.clat[c2];
}
void fgd_cp_distances(CpList l, CpSums s1, CpSums s2, hipStream_t st)
{
  if (l.n > 0) k_cp_distances<<<cp_blocks(l.n, 256), 256, 0, st>>>(l, s1, s2);
}
__global__ __launch_bounds__(256) void k_cp_fraction(int ncells, const double *xarea, const double *area, const double *omask, int first_cell,
                                                      double *frac, int *nbad)
{
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncells) return;
  const double f = xarea[c] / area[c];                                     // :2037, :2089
  frac[c] = f;
  if (omask && c >= first_cell && fabs(omask[c] - f) > CP_TOLERANCE) atomicAdd(nbad, 1);      // :2038
}
void fgd_cp_fraction(int ncells, const double *xarea, const double *area, const double *omask, int first_cell, double *frac, int *nbad,
                     hipStream_t st)
{
  if (ncells > 0) k_cp_fraction<<<cp_blocks(ncells, 256), 256, 0, st>>>(ncells, xarea, area, omask, first_cell, frac, nbad);
}
__global__ void k_cp_tile_starts(int ntiles, const int *cell_off, long n, const int *c1, int *starts)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t <= ntiles) starts[t] = (int)d_lower_bound(c1, n, cell_off[t]);
}
void fgd_cp_tile_starts(int ntiles, const int *cell_off, long n, const int *c1, int *starts, hipStream_t st)
{
  k_cp_tile_starts<<<cp_blocks(ntiles + 1, 64), 64, 0, st>>>(ntiles, cell_off, n, c1, starts);
}
__global__ __launch_bounds__(256) void k_cp_indices(long n, const int *c1, const int *c2, int off1, int nx1, int nx2, int *i1, int *j1, int *i2,
                                                     int *j2)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int a = c1[k] - off1, b = c2[k];
  j1[k] = a / nx1; i1[k] = a - (a / nx1) * nx1;
  j2[k] = b / nx2; i2[k] = b - (b / nx2) * nx2;
}
void fgd_cp_indices(long n, const int *c1, const int *c2, int off1, int nx1, int nx2, int *i1, int *j1, int *i2, int *j2, hipStream_t st)
{
  if (n > 0) k_cp_indices<<<cp_blocks(n, 256), 256, 0, st>>>(n, c1, c2, off1, nx1, nx2, i1, j1, i2, j2);
}

// ------------------------------------------------------------------------------------------- wave x ocean row band (:3107-3117)
// one block per corner row of the ocean grid: does any corner lie strictly inside (lo, hi)?  Integer atomics on the two row numbers.
__global__ __launch_bounds__(256) void k_cp_row_band(int nx, const double *lat, double lo, double hi, int *band)
{
  __shared__ int any;
  const int j = blockIdx.x;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  int mine = 0;
  for (int i = threadIdx.x; i <= nx; i += 256) {
    const double yy = lat[(size_t)j * (nx + 1) + i];
    if (yy > lo && yy < hi) mine = 1;                                      // :3111
  }
  if (mine) atomicOr(&any, 1);
  __syncthreads();
  if (threadIdx.x == 0 && any) { atomicMin(&band[0], j); atomicMax(&band[1], j); }      // :3112-3113
}
__global__ __launch_bounds__(256) void k_cp_band_mask(long n, const int *x_dst, int nx, int js, int je, int *flag)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int jo = x_dst[k] / nx;
  if (jo < js || jo > je) flag[k] = 0;                                     // :3162: the loop never reaches the row
}
void fgd_cp_row_band(int nx, int ny, const double *lat, double lo, double hi, int *band, hipStream_t st)
{
  k_cp_row_band<<<(unsigned)(ny + 1), 256, 0, st>>>(nx, lat, lo, hi, band);
}
void fgd_cp_band_mask(long n, const int *x_dst, int nx, int js, int je, int *flag, hipStream_t st)
{
  if (n > 0) k_cp_band_mask<<<cp_blocks(n, 256), 256, 0, st>>>(n, x_dst, nx, js, je, flag);
}

// ------------------------------------------------------------------------------------------- --check (:3612-3626)
// The loop keeps the first cell with the largest ratio (`>`): the comparison is exact, so the largest ratio with the lowest cell
// index among equals is the same cell whatever the order of the reduction.  A NaN ratio never passes `>` and is never kept.
#define CP_CHECK_PER_BLOCK 2048
long fgd_cp_check_blocks(long n) { return (n + CP_CHECK_PER_BLOCK - 1) / CP_CHECK_PER_BLOCK + 1; }
__device__ __forceinline__ void cp_check_take(double r, int c, double &best, int &cell)
{
  if (c >= 0 && (r > best || (r == best && (cell < 0 || c < cell)))) { best = r; cell = c; }
}
__device__ __forceinline__ void cp_check_block(double &best, int &cell, double *sh_r, int *sh_c)
{
  const int t = threadIdx.x;
  sh_r[t] = best; sh_c[t] = cell;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (t < d) {
      double b = sh_r[t]; int c = sh_c[t];
      cp_check_take(sh_r[t + d], sh_c[t + d], b, c);
      sh_r[t] = b; sh_c[t] = c;
    }
    __syncthreads();
  }
  best = sh_r[0]; cell = sh_c[0];
}
__global__ __launch_bounds__(256) void k_cp_check_ratio(long n, const double *xarea, const double *area, double *sc_ratio, int *sc_cell)
{
  __shared__ double sh_r[256];
  __shared__ int sh_c[256];
  double best = -1; int cell = -1;                                         // :3607-3610
  const long base = (long)blockIdx.x * CP_CHECK_PER_BLOCK;
  for (int q = threadIdx.x; q < CP_CHECK_PER_BLOCK; q += 256) {
    const long c = base + q;
    if (c >= n) break;
    const double a = area[c];
    const double r = fabs(xarea[c] - a) / a;                               // :3614
    if (r > best) { best = r; cell = (int)c; }                            // :3619 (a lane's cells ascend)
  }
  cp_check_block(best, cell, sh_r, sh_c);
  if (threadIdx.x == 0) { sc_ratio[blockIdx.x] = best; sc_cell[blockIdx.x] = cell; }
}
__global__ __launch_bounds__(256) void k_cp_check_final(long nb, const double *sc_ratio, const int *sc_cell, double *best_out, int *cell_out)
{
  __shared__ double sh_r[256];
  __shared__ int sh_c[256];
  double best = -1; int cell = -1;
  for (long b = threadIdx.x; b < nb; b += 256) cp_check_take(sc_ratio[b], sc_cell[b], best, cell);
  cp_check_block(best, cell, sh_r, sh_c);
  if (threadIdx.x == 0) { *best_out = best; *cell_out = cell; }
}
void fgd_cp_check_ratio(long n, const double *xarea, const double *area, double *sc_ratio, int *sc_cell, double *best, int *cell, hipStream_t st)
{
  const long nb = n > 0 ? (n + CP_CHECK_PER_BLOCK - 1) / CP_CHECK_PER_BLOCK : 0;
  if (nb > 0) k_cp_check_ratio<<<(unsigned)nb, 256, 0, st>>>(n, xarea, area, sc_ratio, sc_cell);
  k_cp_check_final<<<1, 256, 0, st>>>(nb, sc_ratio, sc_cell, best, cell);
}
