// river.h -- what river_kernels.hip (device), river.hip (host orchestration) and tests/hostcheck/river_check.cpp (a host
// build) share of river_regrid (tools/river_regrid/river_regrid.c):
//   adjust_lon (:856)      rv_unwrap + rv_adjust_lon: the unwrap of the four longitudes in place and the shift by 2 pi
//   the candidate (:746-758) rv_accept: the lon reject, clip (create_xgrid.c:1159), poly_area (mosaic_util.c:417), the ratio
//   calc_max_subA (:737-761) rv_cell_literal: every call in the reference's order; rv_cell_pruned: only the calls that
//                          change the four longitudes, and the candidates between them
//   distance (:1508)       rv_distance, in degrees, cos as libm's
// Nothing here is contracted (-ffp-contract=off).  The same functions serve one lane alone (lane 0 of 1, the host build) and
// the 64 lanes of a wave, which evaluate the replay redundantly and deal the candidates among themselves.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include "sincos_glibc.h"

#define RV_PI 3.14159265358979323846
#define RV_TPI (2 * RV_PI)
#define RV_D2R (RV_PI / 180.)          /* constant.h */
#define RV_RADIUS 6371000.             /* constant.h */
#define RV_LARGE 1e20                  /* LARGE_VALUE :86 */
#define RV_MIN_AREA_RATIO 1.e-6        /* :93 */
#define RV_SMALL 1.e-10                /* mosaic_util.c: SMALL_VALUE */
#define RV_CAP 8                       /* a quadrilateral cut by four half planes has at most eight vertices */
#define RV_X_CYCLIC 1
#define RV_Y_CYCLIC 2
#define RV_CUBIC_GRID 4

/* the source grid as calc_max_subA reads it, and the two tables of the pruned replay */
struct RvSource {
  const double *xb, *yb;     /* [nx+1], [ny+1] radians */
  const double *tlon;        /* [nx] 0.5 * (xb[i] + xb[i+1]): adjust_lon's target */
  const double *subA;        /* [ny*nx] */
  const int *next;           /* [ny*(nx+1)] the first cell at or after i of row j that is not missing; nx if there is none */
  int nx, ny;
  double missing;            /* river_out's subA_missing: river_in's after init_river_data's pass through an int (:652) */
};

/* the unwrap of adjust_lon: x[i] = x[i-1] + dx.  Returns x_sum. */
FG_HD double rv_unwrap(double x[4])
{
  double x_sum = x[0];
  for (int i = 1; i < 4; i++) {
    double dx = x[i] - x[i - 1];
    if (dx < -RV_PI) dx = dx + RV_TPI;
    else if (dx > RV_PI) dx = dx - RV_TPI;
    x_sum += (x[i] = x[i - 1] + dx);
  }
  return x_sum;
}
/* +1 / -1 / 0: the shift by 2 pi that adjust_lon applies for this mean and target */
FG_HD int rv_shift(double x_sum, double tlon)
{
  const double dx = (x_sum / 4) - tlon;
  if (dx < -RV_PI) return 1;
  if (dx > RV_PI) return -1;
  return 0;
}
FG_HD void rv_apply_shift(double x[4], int s)
{
  if (s > 0) for (int i = 0; i < 4; i++) x[i] += RV_TPI;
  else if (s < 0) for (int i = 0; i < 4; i++) x[i] -= RV_TPI;
}
FG_HD void rv_adjust_lon(double x[4], double tlon)
{
  const double x_sum = rv_unwrap(x);
  rv_apply_shift(x, rv_shift(x_sum, tlon));
}

/* one half plane of clip: SIDE 0 x >= b, 1 x <= b, 2 y >= b, 3 y <= b; the reference's expression trees */
template <int SIDE>
FG_HD int rv_clip_side(const double *xi, const double *yi, int n, double b, double *xo, double *yo)
{
  if (n <= 0) return 0;
  double x_last = xi[n - 1], y_last = yi[n - 1];
  int m = 0;
  int inside_last = SIDE == 0 ? (x_last >= b) : SIDE == 1 ? (x_last <= b) : SIDE == 2 ? (y_last >= b) : (y_last <= b);
  for (int k = 0; k < n; k++) {
    const double xk = xi[k], yk = yi[k];
    const int inside = SIDE == 0 ? (xk >= b) : SIDE == 1 ? (xk <= b) : SIDE == 2 ? (yk >= b) : (yk <= b);
    if (inside != inside_last) {
      if (m < RV_CAP) {
        if (SIDE < 2) { xo[m] = b; yo[m] = y_last + (b - x_last) * (yk - y_last) / (xk - x_last); }
        else { yo[m] = b; xo[m] = x_last + (b - y_last) * (xk - x_last) / (yk - y_last); }
      }
      m++;
    }
    if (inside) { if (m < RV_CAP) { xo[m] = xk; yo[m] = yk; } m++; }
    x_last = xk; y_last = yk; inside_last = inside;
  }
  return m > RV_CAP ? 0 : m;      /* cannot happen for a quadrilateral */
}
FG_HD int rv_clip(const double x[4], const double y[4], double ll_x, double ll_y, double ur_x, double ur_y, double *xo, double *yo)
{
  double xt[RV_CAP], yt[RV_CAP];
  int n = rv_clip_side<0>(x, y, 4, ll_x, xt, yt);
  n = rv_clip_side<1>(xt, yt, n, ur_x, xo, yo);
  n = rv_clip_side<2>(xo, yo, n, ll_y, xt, yt);
  return rv_clip_side<3>(xt, yt, n, ur_y, xo, yo);
}
FG_HD double rv_poly_area(const double *x, const double *y, int n)
{
  double area = 0.0;
  for (int i = 0; i < n; i++) {
    const int ip = (i + 1 == n) ? 0 : i + 1;
    double dx = (x[ip] - x[i]);
    const double lat1 = y[ip], lat2 = y[i];
    if (dx > RV_PI) dx = dx - 2.0 * RV_PI;
    if (dx < -RV_PI) dx = dx + 2.0 * RV_PI;
    if (fabs(dx + RV_PI) < RV_SMALL || fabs(dx - RV_PI) < RV_SMALL) { area += RV_PI; continue; }
    if (fabs(lat1 - lat2) < RV_SMALL)
      area -= dx * fgs_sin(0.5 * (lat1 + lat2));
    else {
      const double dy = 0.5 * (lat1 - lat2);
      const double dat = fgs_sin(dy) / dy;
      area -= dx * fgs_sin(0.5 * (lat1 + lat2)) * dat;
    }
  }
  if (area < 0) return -area * RV_RADIUS * RV_RADIUS;
  return area * RV_RADIUS * RV_RADIUS;
}

/* :751-756: does source cell (ll, ur) count for the land cell (x, y) of this area? */
FG_HD bool rv_accept(const double x[4], const double y[4], double ll_x, double ll_y, double ur_x, double ur_y, double area)
{
  if ((x[0] <= ll_x) && (x[1] <= ll_x) && (x[2] <= ll_x) && (x[3] <= ll_x)) return false;
  if ((x[0] >= ur_x) && (x[1] >= ur_x) && (x[2] >= ur_x) && (x[3] >= ur_x)) return false;
  double xo[RV_CAP], yo[RV_CAP];
  const int n = rv_clip(x, y, ll_x, ll_y, ur_x, ur_y, xo, yo);
  if (n <= 0) return false;
  const double xarea = rv_poly_area(xo, yo, n);
  if (xarea / area < RV_MIN_AREA_RATIO) return false;
  return true;
}

FG_HD double rv_min4(const double v[4]) { double m = v[0]; for (int i = 1; i < 4; i++) if (v[i] < m) m = v[i]; return m; }
FG_HD double rv_max4(const double v[4]) { double m = v[0]; for (int i = 1; i < 4; i++) if (v[i] > m) m = v[i]; return m; }
/* how many of the n ascending values are < v, <= v */
FG_HD int rv_count_lt(const double *a, int n, double v)
{
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}
FG_HD int rv_count_le(const double *a, int n, double v)
{
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] <= v) lo = mid + 1; else hi = mid; }
  return lo;
}

/* The literal loop (:737-761): every row, every source cell, every adjust_lon call.  A chunk of `nl` calls is replayed by every
 * lane, lane k keeps the longitudes as they stand after call k, then each lane tests its own cell.  *visited counts source cells
 * (lane 0 alone adds). */
FG_HD double rv_cell_literal(const RvSource &s, double x[4], const double y[4], double area, int lane, int nl, long *visited)
{
  double best = s.missing;
  for (int jj = 0; jj < s.ny; jj++) {
    const double ll_y = s.yb[jj], ur_y = s.yb[jj + 1];
    if (lane == 0) *visited += s.nx;
    if ((y[0] <= ll_y) && (y[1] <= ll_y) && (y[2] <= ll_y) && (y[3] <= ll_y)) continue;
    if ((y[0] >= ur_y) && (y[1] >= ur_y) && (y[2] >= ur_y) && (y[3] >= ur_y)) continue;
    for (int base = 0; base < s.nx; base += nl) {
      double xs[4] = {0, 0, 0, 0};
      bool mine = false;
      for (int k = 0; k < nl && base + k < s.nx; k++) {
        const int ii = base + k;
        if (s.subA[(long)jj * s.nx + ii] == s.missing) continue;
        rv_adjust_lon(x, 0.5 * (s.xb[ii] + s.xb[ii + 1]));
        if (k == lane) { mine = true; for (int v = 0; v < 4; v++) xs[v] = x[v]; }
      }
      if (mine) {
        const int ii = base + lane;
        const double a = s.subA[(long)jj * s.nx + ii];
        if (rv_accept(xs, y, s.xb[ii], ll_y, s.xb[ii + 1], ur_y, area) && a > best) best = a;
      }
    }
  }
  return best;
}

/* the cells lo..hi of row jj with the longitudes x as they stand: the lon reject is an index interval of xb */
FG_HD void rv_segment(const RvSource &s, const double x[4], const double y[4], double area, int jj, int lo, int hi, int lane, int nl,
                      double *best, long *visited)
{
  const int a = rv_count_le(s.xb, s.nx + 1, rv_min4(x)) - 1, b = rv_count_lt(s.xb, s.nx + 1, rv_max4(x)) - 1;
  if (a > lo) lo = a;
  if (b < hi) hi = b;
  for (int ii = lo + lane; ii <= hi; ii += nl) {
    const double v = s.subA[(long)jj * s.nx + ii];
    if (v == s.missing) continue;
    *visited += 1;
    if (rv_accept(x, y, s.xb[ii], s.yb[jj], s.xb[ii + 1], s.yb[jj + 1], area) && v > *best) *best = v;
  }
}

/* The pruned replay.  Needs xb, yb strictly ascending and tlon ascending (river.hip checks; otherwise the literal loop runs).
 * Rows: those that pass the latitude test are an index interval of yb.  Within a row the calls go to the cells that are not
 * missing, in ascending order.  While the unwrap leaves the four values as they are (x is a fixed point of rv_unwrap), a call
 * changes them only by its shift, and the shift depends on x_sum/4 - tlon alone, which falls as tlon rises: `> pi` can only
 * hold for the first call of the row, `< -pi` holds from some index on, found by bisection, and the call that fires is the next
 * cell that is not missing from there.  Where the unwrap does change a value the call is carried out as it stands.
 * *visited counts the source cells tested (every lane adds its own). */
FG_HD double rv_cell_pruned(const RvSource &s, double x[4], const double y[4], double area, int lane, int nl, long *visited)
{
  double best = s.missing;
  const int j0 = rv_count_le(s.yb, s.ny + 1, rv_min4(y)) - 1, j1 = rv_count_lt(s.yb, s.ny + 1, rv_max4(y)) - 1;
  for (int jj = (j0 < 0 ? 0 : j0); jj <= j1 && jj < s.ny; jj++) {
    const int *next = s.next + (long)jj * (s.nx + 1);
    int ii = next[0];
    while (ii < s.nx) {
      double u[4] = {x[0], x[1], x[2], x[3]};
      const double x_sum = rv_unwrap(u);
      const bool stable = (u[0] == x[0]) && (u[1] == x[1]) && (u[2] == x[2]) && (u[3] == x[3]);
      const int sh = rv_shift(x_sum, s.tlon[ii]);
      if (!stable || sh != 0) {                 /* the call at ii changes the longitudes */
        for (int v = 0; v < 4; v++) x[v] = u[v];
        rv_apply_shift(x, sh);
        rv_segment(s, x, y, area, jj, ii, ii, lane, nl, &best, visited);
        ii = next[ii + 1];
        continue;
      }
      /* nothing changes at ii, nor until x_sum/4 - tlon < -pi */
      const double mean = x_sum / 4;
      int lo = ii + 1, hi = s.nx;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (mean - s.tlon[mid] < -RV_PI) hi = mid; else lo = mid + 1; }
      const int e = next[lo];
      rv_segment(s, x, y, area, jj, ii, e - 1, lane, nl, &best, visited);
      ii = e;
    }
  }
  return best;
}

/* distance (:1508): degrees in, metres out */
FG_HD double rv_distance(double lon1, double lat1, double lon2, double lat2)
{
  double dx = lon2 - lon1, dist;
  if (dx > 180.) dx = dx - 360.;
  if (dx < -180.) dx = dx + 360.;
  if (lon1 == lon2)
    dist = fabs(lat2 - lat1) * RV_D2R;
  else if (lat1 == lat2)
    dist = fabs(dx) * RV_D2R * fgs_cos(lat1 * RV_D2R);
  else {
    const double s1 = fabs(dx) * RV_D2R * fgs_cos(lat1 * RV_D2R);
    const double s2 = fabs(lat2 - lat1) * RV_D2R;
    dist = sqrt(s1 * s1 + s2 * s2);
  }
  dist *= RV_RADIUS;
  return dist;
}

/* calc_tocell's choice among the eight neighbours (:912-973).  sub[joff*3+ioff]: the 3 x 3 block of max subA, the cell itself
 * at [4].  Returns the slot 0..8 the cell flows to, or -1 (tocell = 0). */
FG_HD int rv_tocell_slot(const double sub[9], double suba_cutoff, double subA_missing)
{
  const double me = sub[4];
  double tval = -999;
  int get = -1;
  if (me > suba_cutoff) {
    for (int k = 0; k < 9; k++) {
      if (k == 4) continue;
      const double v = sub[k];
      if (v > me) {
        if (tval == -999) { if (v > tval) { get = k; tval = v; } }
        else if (tval < RV_LARGE) { if (v > tval && v < RV_LARGE) { get = k; tval = v; } }
        else { get = k; tval = v; }
      }
    }
  } else {
    for (int k = 0; k < 9; k++) {
      if (k == 4) continue;
      const double v = sub[k];
      if (v != subA_missing) { if (v >= tval) { get = k; tval = v; } }
    }
  }
  if (get >= 0 && tval > me) return get;
  return -1;
}

#ifdef __HIPCC__
struct RvGrid {               /* the output mosaic on the device */
  int ntiles, nx, ny, opcode;
  const double *xb, *yb;      /* [ntiles][(ny+1)*(nx+1)] radians */
  const double *xt, *yt;      /* [ntiles][(ny+2)*(nx+2)] degrees, halo filled */
  const double *area, *landfrac;   /* [ntiles*ny*nx] */
  const int *hmap;            /* [ntiles][(ny+2)*(nx+2)] the interior cell (tile, j, i -> flat) a haloed index reads, -1: never filled */
};
void fgd_rv_max_suba(const RvSource &s, const RvGrid &g, int nland, const int *land, double *maxsub, unsigned long long *visited, int prune, hipStream_t st);
void fgd_rv_tocell(const RvGrid &g, const double *maxsub, double suba_cutoff, double subA_missing, int tocell_missing, int *tocell, int *dir, hipStream_t st);
void fgd_rv_outlets(const RvGrid &g, const int *tocell, const int *dir, int tocell_missing, double cellarea_missing, double celllength_missing,
                    int *flag, int *trav0, int *succ, int *hops, double *cellarea, double *celllength, hipStream_t st);
void fgd_rv_jump(long n, const int *succ, const int *hops, int *succ2, int *hops2, int *changed, hipStream_t st);
void fgd_rv_finish(long n, const int *tocell, int tocell_missing, const int *succ, const int *hops, const int *trav0, const int *prefix,
                   int travel_missing, int basin_missing, int *travel, int *basin, hipStream_t st);
void fgd_rv_level(const RvGrid &g, int level, int count, const int *cells, const int *dir, const int *travel, const double *cellarea,
                  double subA_missing, double *subA, hipStream_t st);
#endif
