// topog.h -- what topog_kernels.hip (device), topog.hip (host orchestration) and tests/hostcheck/topog_check.cpp (a host build)
// share of make_topog's realistic topography (tools/make_topog/topog.c):
//   the source axes (:416-427)     tp_axis_bounds: bounds from centres, the end extrapolation, *D2R
//   the row trim (:437-449)        tp_trim: strict inequalities, one row added at each end, clamped
//   nearest_index (mosaic_util.c:81) tp_nearest_index: the ends, value <= array[i], the tie towards the upper level
//   kmt and ht of one cell (:582-619) tp_kmt_cell
//   remove_isolated_cells (:851-862) tp_isolated_cell: one cell of the in-place sweep, on the haloed arrays as they stand
//   restrict_partial_cells (:900-933), enforce_min_depth (:1012-1037)  tp_restrict_cell, tp_enforce_cell
// min and max are the reference's macros (mosaic_util.h:34-35), operand order included.  Nothing here is contracted.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#ifndef FG_HD
#ifdef __HIPCC__
#define FG_HD __host__ __device__ __forceinline__
#else
#define FG_HD static inline
#endif
#endif

#define TP_PI 3.14159265358979323846
#define TP_D2R (TP_PI / 180)             /* constant.h:42 */
#define TP_NC_INT 4                      /* netcdf.h's nc_type codes */
#define TP_NC_FLOAT 5
#define TP_NC_DOUBLE 6

#define TP_MIN(a, b) ((a) < (b) ? (a) : (b))
#define TP_MAX(a, b) ((a) > (b) ? (a) : (b))

/* xc [n+1] in radians from the centres xt [n] in degrees */
static inline void tp_axis_bounds(int n, const double *xt, double *xc)
{
  for (int i = 1; i < n; i++) xc[i] = (xt[i - 1] + xt[i]) * 0.5;
  xc[0] = 2 * xt[0] - xc[1];
  xc[n] = 2 * xt[n - 1] - xc[n - 1];
  for (int i = 0; i <= n; i++) xc[i] = xc[i] * TP_D2R;
}

/* the rows of the source that the destination's latitudes reach; yc [ny_src+1] radians */
static inline void tp_trim(int ny_src, const double *yc, double y_min, double y_max, int *jstart, int *jend)
{
  int js = ny_src, je = -1;
  for (int j = 0; j <= ny_src; j++) {
    const double yy = yc[j];
    if (yy > y_min && yy < y_max) {
      if (j > je) je = j;
      if (j < js) js = j;
    }
  }
  *jstart = TP_MAX(0, js - 1);
  *jend = TP_MIN(ny_src - 1, je + 1);
}

/* :492-502 for one cell: d is the file's value as a double.  `missing` is tested before scaling and the cell keeps it; <= 0 after
 * scaling is masked.  Returns depth_src. */
FG_HD double tp_prepare_cell(double d, double missing, double scale, double *mask)
{
  *mask = 0.0;
  if (!(d == missing)) {
    d = d * scale;
    *mask = d <= 0.0 ? 0.0 : 1.0;
  }
  return d;
}

/* :623-636 for column i = 1 .. ni.  tripolar: the fold of the last row into the north halo; else cyclic_y: both halo rows */
FG_HD void tp_halo_y_cell(int ni, int nj, int tripolar, double *ht, int *kmt, int i)
{
  const long nip = ni + 2;
  if (tripolar) {
    kmt[(nj + 1) * nip + i] = kmt[nj * nip + (ni - i + 1)];
    ht[(nj + 1) * nip + i] = ht[nj * nip + (ni - i + 1)];
  } else {
    kmt[i] = kmt[nj * nip + i];
    kmt[(nj + 1) * nip + i] = kmt[nip + i];
    ht[i] = ht[nj * nip + i];
    ht[(nj + 1) * nip + i] = ht[nip + i];
  }
}
/* :638-645 for row j = 0 .. nj+1: after the rows above, so the halo rows are wrapped too */
FG_HD void tp_halo_x_cell(int ni, double *ht, int *kmt, int j)
{
  const long nip = ni + 2;
  kmt[j * nip] = kmt[j * nip + ni];
  kmt[j * nip + ni + 1] = kmt[j * nip + 1];
  ht[j * nip] = ht[j * nip + ni];
  ht[j * nip + ni + 1] = ht[j * nip + 1];
}

/* the rows jlo .. jhi of the cells (t - 2j, j) with 1 <= t - 2j <= ni and 1 <= j <= nj_max; 0 when there is none */
static inline int tp_diagonal(int ni, int nj_max, int t, int *jlo, int *jhi)
{
  int lo = t - ni <= 0 ? 1 : (t - ni + 1) / 2, hi = (t - 1) / 2;
  if (lo < 1) lo = 1;
  if (hi > nj_max) hi = nj_max;
  *jlo = lo; *jhi = hi;
  return hi >= lo;
}

/* one interior cell (1 <= i < nx-1, 1 <= j < ny-1) of one pass of filter_topo (:730-744): the nine terms in the reference's
 * order, ip (x) outer, jp (y) inner, from 0.0; a land neighbour replaced by the centre value */
FG_HD double tp_filter_cell(int nx, const double *in, const double *rmask, int i, int j, int allow_deepening)
{
  const double f[9] = {1.0 / 16.0, 1.0 / 8.0, 1.0 / 16.0, 1.0 / 8.0, 1.0 / 4.0, 1.0 / 8.0, 1.0 / 16.0, 1.0 / 8.0, 1.0 / 16.0};
  const long c = (long)j * nx + i;
  const double d_old = in[c];
  double s = 0.0;
  for (int ip = -1; ip <= 1; ip++)
    for (int jp = -1; jp <= 1; jp++) {
      const int m = (ip + 1) * 3 + jp + 1;
      const long q = (long)(j + jp) * nx + i + ip;
      if (rmask[q] == 0.0) s = s + d_old * f[m];
      else s = s + in[q] * f[m];
    }
  if (!allow_deepening) { if (s > d_old) s = d_old; }
  return s * rmask[c];
}

/* (with ia == 1 and value == array[0] the reference reads array[1]; here that case returns 0) */
FG_HD int tp_nearest_index(double value, const double *array, int ia)
{
  if (value < array[0]) return 0;
  if (value > array[ia - 1]) return ia - 1;
  for (int i = 1; i < ia; i++)
    if (value <= array[i]) return (array[i] - value > value - array[i - 1]) ? i - 1 : i;
  return 0;
}

/* :582-619 for one cell: *ht in, *ht and the level out (-1 and the depth untouched on land) */
FG_HD int tp_kmt_cell(double *ht, const double *zw, int nk, double min_thickness, int full_cell, int flat_bottom)
{
  double h = *ht;
  int k = -1;
  if (h > 0) {
    k = tp_nearest_index(h, zw, nk);
    if (zw[k] < h) {
      if ((h - zw[k]) < min_thickness) h = zw[k];
      else if (k == nk - 1) h = zw[k];
      else k++;
    }
  }
  if (full_cell && h > 0) h = zw[k];
  if (flat_bottom && h > 0) { h = zw[nk - 1]; k = nk - 1; }
  *ht = h;
  return k;
}

FG_HD int tp_min4i(int a, int b, int c, int d)       /* kmin goes through min4_double: the same order of comparisons */
{
  const int x1 = TP_MIN(a, b), x2 = TP_MIN(c, d);
  return TP_MIN(x1, x2);
}
FG_HD int tp_max4i(int a, int b, int c, int d)
{
  const int x1 = TP_MAX(a, b), x2 = TP_MAX(c, d);
  return TP_MAX(x1, x2);
}
FG_HD double tp_min4d(double a, double b, double c, double d)
{
  const double x1 = TP_MIN(a, b), x2 = TP_MIN(c, d);
  return TP_MIN(x1, x2);
}
FG_HD double tp_max4d(double a, double b, double c, double d)
{
  const double x1 = TP_MAX(a, b), x2 = TP_MAX(c, d);
  return TP_MAX(x1, x2);
}
FG_HD int tp_kmin(int nip, const int *kmt, int i, int j)
{
  return tp_min4i(kmt[j * nip + i], kmt[j * nip + i + 1], kmt[(j + 1) * nip + i], kmt[(j + 1) * nip + i + 1]);
}
FG_HD double tp_hmin(int nip, const double *ht, int i, int j)
{
  return tp_min4d(ht[j * nip + i], ht[j * nip + i + 1], ht[(j + 1) * nip + i], ht[(j + 1) * nip + i + 1]);
}

/* one cell (i, j; 1-based on the haloed arrays) of remove_isolated_cells (:852-861) on the arrays as they stand: 1 when the cell
 * is to be reset, with its new level and depth in *k_new, *ht_new */
FG_HD int tp_isolated_eval(int ni, const double *ht, const int *kmt, int i, int j, int dont_change_landmask, int *k_new, double *ht_new)
{
  const int nip = ni + 2;
  const int k = tp_max4i(tp_kmin(nip, kmt, i, j), tp_kmin(nip, kmt, i - 1, j), tp_kmin(nip, kmt, i, j - 1), tp_kmin(nip, kmt, i - 1, j - 1));
  if ((k >= 0 || !dont_change_landmask) && kmt[j * nip + i] != k) {
    *ht_new = tp_max4d(tp_hmin(nip, ht, i, j), tp_hmin(nip, ht, i - 1, j), tp_hmin(nip, ht, i, j - 1), tp_hmin(nip, ht, i - 1, j - 1));
    *k_new = k;
    return 1;
  }
  return 0;
}
/* the same in place: one step of the sequential sweep */
FG_HD int tp_isolated_cell(int ni, double *ht, int *kmt, int i, int j, int dont_change_landmask)
{
  int k;
  double h;
  if (!tp_isolated_eval(ni, ht, kmt, i, j, dont_change_landmask, &k, &h)) return 0;
  ht[j * (ni + 2) + i] = h;
  kmt[j * (ni + 2) + i] = k;
  return 1;
}

/* p_cell_min [nk] (:888-893) */
static inline void tp_p_cell_min(int nk, const double *zw, double fraction_full_cell, double min_thickness, double *p)
{
  if (fraction_full_cell == 0.0) for (int k = 0; k < nk; k++) p[k] = TP_MIN(50.0, zw[0]);
  else {
    p[0] = fraction_full_cell * zw[0];
    for (int k = 1; k < nk; k++) p[k] = TP_MAX(fraction_full_cell * (zw[k] - zw[k - 1]), min_thickness);
  }
}

/* restrict_partial_cells for one cell; 1 when the depth was reset */
FG_HD int tp_restrict_cell(double *ht, int *kmt, const double *zw, const double *p_cell_min, int open_very_this_cell)
{
  const int k = *kmt;
  if (k > 0 && (*ht - zw[k - 1]) < p_cell_min[k]) {
    double tmp;
    if (open_very_this_cell) tmp = zw[k - 1] + p_cell_min[k];
    else {
      const double tmp1 = *ht - zw[k - 1], tmp2 = zw[k - 1] + p_cell_min[k] - *ht;
      if (tmp2 > tmp1) { *kmt = k - 1; tmp = zw[k - 1]; }
      else tmp = zw[k - 1] + p_cell_min[k];
    }
    *ht = tmp;
    return 1;
  }
  return 0;
}

/* enforce_min_depth for one cell; 1 when the cell was shallow.  The three branches run one after another as written there (at
 * most one of the switches is set: the caller has checked). */
FG_HD int tp_enforce_cell(double *depth, int *kmt, const double *zw, int kmt_min, int round_shallow, int deepen_shallow, int fill_shallow)
{
  const int kml = kmt_min - 1;
  if (*depth > 0 && *kmt < kml) {
    if (round_shallow || (!deepen_shallow && !fill_shallow)) {
      if (zw[*kmt < 0 ? 0 : *kmt] < 0.5 * zw[kml]) { *depth = 0.0; *kmt = -1; }
      else { *depth = zw[kml]; *kmt = kml; }
    }
    if (fill_shallow) { *depth = 0.0; *kmt = -1; }
    if (deepen_shallow) { *depth = zw[kml]; *kmt = kml; }
    return 1;
  }
  return 0;
}

#ifdef __HIPCC__
struct TpCounts { unsigned isolated, partial, shallow, pad; };

void fgd_tp_scale(long n, const double *x_deg, const double *y_deg, double *x_r, double *y_r, hipStream_t st);
void fgd_tp_expand(int nxp, int nyp, const double *xc, const double *yc, double *x2, double *y2, hipStream_t st);
void fgd_tp_prepare(long n, const void *raw, int dtype, double missing, double scale, double *depth_src, double *mask_src, hipStream_t st);
void fgd_tp_ongrid(long n, const double *depth_src, double missing, double *depth, hipStream_t st);
void fgd_tp_rmask(long n, const double *depth, double *rmask, hipStream_t st);
void fgd_tp_filter(int nx, int ny, const double *in, const double *rmask, int allow_deepening, double *out, hipStream_t st);
void fgd_tp_zero_row(int nx, double *depth, hipStream_t st);
void fgd_tp_kmt(int ni, int nj, int nk, const double *zw, const double *depth, double min_thickness, int full_cell, int flat_bottom,
                double *ht, int *kmt, hipStream_t st);
void fgd_tp_halo_y(int ni, int nj, int tripolar, double *ht, int *kmt, hipStream_t st);
void fgd_tp_halo_x(int ni, int nj, double *ht, int *kmt, hipStream_t st);
int  fgd_tp_isolated(int ni, int nj_max, int dont_change_landmask, double *ht, int *kmt, TpCounts *cnt, hipStream_t st);    /* -> launches */
void fgd_tp_finish(int ni, int nj, int nk, const double *zw, const double *p_cell_min, const double *ht, const int *kmt, int fused_nj_max,
                   int dont_change_landmask, int adjust_topo, int open_very_this_cell, int kmt_min, int round_shallow, int deepen_shallow, int fill_shallow, double *depth, int *num_levels,
                   TpCounts *cnt, hipStream_t st);
void fgd_tp_deepest(long n, const double *depth, double *partial, double *result, hipStream_t st);
#define TP_REDUCE_BLOCKS 256
#endif
