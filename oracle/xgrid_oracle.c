/*
 * xgrid_oracle.c -- CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE)
 *
 * A clean-room C restatement of the FRE-NCtools conservative-regrid hot path,
 * written to be *bit-identical* (same FP64 expression trees, same evaluation
 * order, gcc -O2 -ffp-contract=off, glibc libm) to the reference so that it can
 * arbitrate parity for the HIP path in fre-nctools_amd/csrc.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library.  The product (libfregrid_hip.so) never links or calls it.
 *
 * Parity status: PINNED.  tests/test_oracle_vs_ref.py checks every function
 * here against the reference's own sources compiled in place (oracle/_ref,
 * see oracle/Makefile), and tests/golden holds vectors produced by that
 * compiled reference (tests/golden/make_golden.py).
 *
 * Reference citations (paths relative to /root/reference):
 *   fix_lon                    tools/libfrencutils/mosaic_util.c:667-738
 *   poly_area(_main)           tools/libfrencutils/mosaic_util.c:417-459,474-515
 *   clip_2dx2d / inside_edge   tools/libfrencutils/create_xgrid.c:1266-1341,2342-2350
 *   pimod                      tools/libfrencutils/create_xgrid.c:1343-1349
 *   poly_ctrlat / poly_ctrlon  tools/libfrencutils/create_xgrid.c:2096-2121,2170-2217
 *   get_grid_area              tools/libfrencutils/create_xgrid.c:66-88
 *   create_xgrid_2dx2d_order1  tools/libfrencutils/create_xgrid.c:621-871
 *   create_xgrid_2dx2d_order2  tools/libfrencutils/create_xgrid.c:893-1152
 *   setup_conserve_interp      tools/fregrid/conserve_interp.c:127-358
 *   do_scalar_conserve_interp  tools/fregrid/conserve_interp.c:507-910
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define ORC_RADIUS 6371000.0                 /* constant.h:23 */
#define ORC_PI     3.14159265358979323846    /* M_PI */
#define ORC_TPI    (2.0 * ORC_PI)            /* constant.h:43 */
#define ORC_HPI    (0.5 * ORC_PI)            /* constant.h:44 */
#define ORC_SMALL  1.e-10                    /* mosaic_util.h:36 SMALL_VALUE */
#define ORC_POLE_TOL 1.e-6                   /* mosaic_util.c:35 TOLORENCE */
#define ORC_AREA_RATIO_THRESH 1.e-6          /* create_xgrid.c:27 */
#define ORC_MASK_THRESH 0.5                  /* create_xgrid.c:28 */
#define ORC_MAXV 8                           /* create_xgrid.c:627 MAX_V */
#define ORC_MV 50                            /* create_xgrid.h:31 */
#define ORC_CENTROID_AREA_RATIO 1.e-3        /* conserve_interp.c:35 AREA_RATIO */
#define ORC_MAXVAL 1.e20                     /* conserve_interp.c:36 */

/* ------------------------------------------------------------------------- */
/* small helpers: mosaic_util.c:157-205                                       */
/* ------------------------------------------------------------------------- */
static double vmin(int n, const double *v)
{
  double m = v[0];
  for (int k = 1; k < n; k++) if (v[k] < m) m = v[k];
  return m;
}
static double vmax(int n, const double *v)
{
  double m = v[0];
  for (int k = 1; k < n; k++) if (v[k] > m) m = v[k];
  return m;
}
static double vavg(int n, const double *v)
{
  double s = 0;
  for (int k = 0; k < n; k++) s += v[k];
  s /= n;
  return s;
}

static int is_pole_lat(double lat) { return fabs(lat) >= ORC_HPI - ORC_POLE_TOL; }

static int vtx_remove(double *x, double *y, int n, int at)
{
  for (int k = at; k < n - 1; k++) { x[k] = x[k + 1]; y[k] = y[k + 1]; }
  return n - 1;
}
static int vtx_insert(double *x, double *y, int n, int at, double lon, double lat)
{
  for (int k = n - 1; k >= at; k--) { x[k + 1] = x[k]; y[k + 1] = y[k]; }
  x[at] = lon; y[at] = lat;
  return n + 1;
}

/* mosaic_util.c:667-738 */
int orc_fix_lon(double *x, double *y, int n, double tlon)
{
  int nn = n, i;

  /* pole vertices must come in pairs (mosaic_util.c:682-692) */
  for (i = 0; i < nn; i++) {
    if (!is_pole_lat(y[i])) continue;
    int im = (i + nn - 1) % nn, ip = (i + 1) % nn;
    if (y[im] == y[i] && y[ip] == y[i]) {
      nn = vtx_remove(x, y, nn, i);
      i--;
    } else if (y[im] != y[i] && y[ip] != y[i]) {
      nn = vtx_insert(x, y, nn, i, x[i], y[i]);
      i++;
    }
  }
  /* pole pair takes the longitudes of its non-pole neighbours (:695-700) */
  for (i = 0; i < nn; i++) {
    if (!is_pole_lat(y[i])) continue;
    int im = (i + nn - 1) % nn, ip = (i + 1) % nn;
    if (y[im] != y[i]) x[i] = x[im];
    if (y[ip] != y[i]) x[i] = x[ip];
  }
  /* an edge with |dlon| == pi passes through a pole: insert twin pole vertices (:704-717) */
  for (i = 0; i < nn; i++) {
    int im = (i + nn - 1) % nn;
    double dx = x[i] - x[im];
    if (fabs(dx + ORC_PI) < ORC_SMALL || fabs(dx - ORC_PI) < ORC_SMALL) {
      double xa = x[im], xb = x[i];
      double ypole = ORC_HPI;
      if (y[i] < 0.0) ypole = -ORC_HPI;
      nn = vtx_insert(x, y, nn, i, xb, ypole);
      nn = vtx_insert(x, y, nn, i, xa, ypole);
      break;
    }
  }
  if (!nn) return 0;
  /* unwrap successive differences into (-pi, pi] (:718-725) */
  double x_sum = x[0];
  for (i = 1; i < nn; i++) {
    double dx = x[i] - x[i - 1];
    if (dx < -ORC_PI)      dx = dx + ORC_TPI;
    else if (dx > ORC_PI)  dx = dx - ORC_TPI;
    x_sum += (x[i] = x[i - 1] + dx);
  }
  /* recentre the mean longitude to within pi of tlon (:727-729) */
  double d = (x_sum / nn) - tlon;
  if (d < -ORC_PI)      for (i = 0; i < nn; i++) x[i] += ORC_TPI;
  else if (d > ORC_PI)  for (i = 0; i < nn; i++) x[i] -= ORC_TPI;
  return nn;
}

/* mosaic_util.c:417-459 (poly_area with rotate_poly_flag == 0, :483-485) */
double orc_poly_area(const double *x, const double *y, int n)
{
  double area = 0.0;
  for (int i = 0; i < n; i++) {
    int ip = (i + 1) % n;
    double dx = (x[ip] - x[i]);
    double lat1 = y[ip], lat2 = y[i];
    if (dx > ORC_PI)  dx = dx - 2.0 * ORC_PI;
    if (dx < -ORC_PI) dx = dx + 2.0 * ORC_PI;
    if (fabs(dx + ORC_PI) < ORC_SMALL || fabs(dx - ORC_PI) < ORC_SMALL) {
      area += ORC_PI;            /* edge through a pole */
      continue;
    }
    if (fabs(lat1 - lat2) < ORC_SMALL)
      area -= dx * sin(0.5 * (lat1 + lat2));
    else {
      double dy = 0.5 * (lat1 - lat2);
      double dat = sin(dy) / dy;
      area -= dx * sin(0.5 * (lat1 + lat2)) * dat;
    }
  }
  if (area < 0) return -area * ORC_RADIUS * ORC_RADIUS;
  return area * ORC_RADIUS * ORC_RADIUS;
}

/* create_xgrid.c:2342-2350 */
static int edge_keeps(double x0, double y0, double x1, double y1, double x, double y)
{
  double product = (x - x0) * (y1 - y0) + (x0 - x1) * (y - y0);
  return (product <= 1.e-12) ? 1 : 0;
}

/* create_xgrid.c:1343-1349 */
void orc_pimod(double *x, int n)
{
  for (int i = 0; i < n; i++) {
    if (x[i] < -ORC_PI)     x[i] += ORC_TPI;
    else if (x[i] > ORC_PI) x[i] -= ORC_TPI;
  }
}

/* create_xgrid.c:1266-1341.  Polygon 1 is the one being cut down, polygon 2
 * supplies the cutting edges.  Returns -1 where the reference would call
 * error_handler (parallel edges, :1314-1317). */
int orc_clip_2dx2d(const double *lon1, const double *lat1, int n1,
                   const double *lon2, const double *lat2, int n2,
                   double *lon_out, double *lat_out)
{
  double cx[ORC_MV], cy[ORC_MV], ex[ORC_MV], ey[ORC_MV];
  int wrap = 0, n_cur = n1;

  for (int k = 0; k < n1; k++) {
    cx[k] = lon1[k]; cy[k] = lat1[k];
    if (cx[k] > ORC_TPI || cx[k] < 0.0) wrap = 1;
  }
  for (int k = 0; k < n2; k++) { ex[k] = lon2[k]; ey[k] = lat2[k]; }
  if (wrap) { orc_pimod(cx, n1); orc_pimod(ex, n2); }

  double x2_0 = ex[n2 - 1], y2_0 = ey[n2 - 1];
  for (int e = 0; e < n2; e++) {
    double x2_1 = ex[e], y2_1 = ey[e];
    double x1_0 = cx[n_cur - 1], y1_0 = cy[n_cur - 1];
    int was_in = edge_keeps(x2_0, y2_0, x2_1, y2_1, x1_0, y1_0);
    int n_new = 0;
    for (int k = 0; k < n_cur; k++) {
      double x1_1 = cx[k], y1_1 = cy[k];
      int is_in = edge_keeps(x2_0, y2_0, x2_1, y2_1, x1_1, y1_1);
      if (is_in != was_in) {
        double dy1 = y1_1 - y1_0;
        double dy2 = y2_1 - y2_0;
        double dx1 = x1_1 - x1_0;
        double dx2 = x2_1 - x2_0;
        double ds1 = y1_0 * x1_1 - y1_1 * x1_0;
        double ds2 = y2_0 * x2_1 - y2_1 * x2_0;
        double determ = dy2 * dx1 - dy1 * dx2;
        if (fabs(determ) < 1.0e-30) return -1;
        lon_out[n_new]   = (dx2 * ds1 - dx1 * ds2) / determ;
        lat_out[n_new++] = (dy2 * ds1 - dy1 * ds2) / determ;
      }
      if (is_in) { lon_out[n_new] = x1_1; lat_out[n_new++] = y1_1; }
      x1_0 = x1_1; y1_0 = y1_1; was_in = is_in;
    }
    n_cur = n_new;
    if (!n_cur) return 0;
    for (int k = 0; k < n_cur; k++) { cx[k] = lon_out[k]; cy[k] = lat_out[k]; }
    x2_0 = x2_1; y2_0 = y2_1;
  }
  return n_cur;
}

/* create_xgrid.c:2096-2121 */
double orc_poly_ctrlat(const double *x, const double *y, int n)
{
  double ctrlat = 0.0;
  for (int i = 0; i < n; i++) {
    int ip = (i + 1) % n;
    double dx = (x[ip] - x[i]);
    double lat1 = y[ip], lat2 = y[i];
    double dy = lat2 - lat1;
    double hdy = dy * 0.5;
    double avg_y = (lat1 + lat2) * 0.5;
    if (dx == 0.0) continue;
    if (dx > ORC_PI)   dx = dx - 2.0 * ORC_PI;
    if (dx <= -ORC_PI) dx = dx + 2.0 * ORC_PI;
    if (fabs(hdy) < ORC_SMALL)
      ctrlat -= dx * (2 * cos(avg_y) + lat2 * sin(avg_y) - cos(lat1));
    else
      ctrlat -= dx * ((sin(hdy) / hdy) * (2 * cos(avg_y) + lat2 * sin(avg_y)) - cos(lat1));
  }
  return (ctrlat * ORC_RADIUS * ORC_RADIUS);
}

/* create_xgrid.c:2170-2217 */
double orc_poly_ctrlon(const double *x, const double *y, int n, double clon)
{
  double ctrlon = 0.0;
  for (int i = 0; i < n; i++) {
    int ip = (i + 1) % n;
    double phi1 = x[ip], phi2 = x[i];
    double lat1 = y[ip], lat2 = y[i];
    double dphi = phi1 - phi2;
    if (dphi == 0.0) continue;
    double f1 = 0.5 * (cos(lat1) * sin(lat1) + lat1);
    double f2 = 0.5 * (cos(lat2) * sin(lat2) + lat2);
    if (dphi > ORC_PI)  dphi = dphi - 2.0 * ORC_PI;
    if (dphi < -ORC_PI) dphi = dphi + 2.0 * ORC_PI;
    double dphi1 = phi1 - clon;
    if (dphi1 > ORC_PI)  dphi1 -= 2.0 * ORC_PI;
    if (dphi1 < -ORC_PI) dphi1 += 2.0 * ORC_PI;
    double dphi2 = phi2 - clon;
    if (dphi2 > ORC_PI)  dphi2 -= 2.0 * ORC_PI;
    if (dphi2 < -ORC_PI) dphi2 += 2.0 * ORC_PI;
    if (fabs(dphi2 - dphi1) < ORC_PI) {
      ctrlon -= dphi * (dphi1 * f1 + dphi2 * f2) / 2.0;
    } else {
      double fac = (dphi1 > 0.0) ? ORC_PI : -ORC_PI;
      double fint = f1 + (f2 - f1) * (fac - dphi1) / fabs(dphi);
      ctrlon -= 0.5 * dphi1 * (dphi1 - fac) * f1 - 0.5 * dphi2 * (dphi2 + fac) * f2
                + 0.5 * fac * (dphi1 + dphi2) * fint;
    }
  }
  return (ctrlon * ORC_RADIUS * ORC_RADIUS);
}

/* load the 4 corners of cell (i,j) counter-clockwise: SW, SE, NE, NW
 * (create_xgrid.c:76-83, :1035-1040) */
static void load_quad(const double *lon, const double *lat, int nxp, int i, int j,
                      double *x, double *y)
{
  int n0 = j * nxp + i, n1 = j * nxp + i + 1;
  int n2 = (j + 1) * nxp + i + 1, n3 = (j + 1) * nxp + i;
  x[0] = lon[n0]; y[0] = lat[n0];
  x[1] = lon[n1]; y[1] = lat[n1];
  x[2] = lon[n2]; y[2] = lat[n2];
  x[3] = lon[n3]; y[3] = lat[n3];
}

/* create_xgrid.c:66-88 */
void orc_get_grid_area(int nx, int ny, const double *lon, const double *lat, double *area)
{
  double x[20], y[20];
  for (int j = 0; j < ny; j++)
    for (int i = 0; i < nx; i++) {
      load_quad(lon, lat, nx + 1, i, j, x, y);
      int n = orc_fix_lon(x, y, 4, ORC_PI);
      area[j * nx + i] = orc_poly_area(x, y, n);
    }
}

/* per-destination-cell record: create_xgrid.c:991-1016 ("get_grid_cell_struct") */
typedef struct {
  double lat_min, lat_max, lon_min, lon_max, lon_avg;
  int nv;
  double x[ORC_MAXV], y[ORC_MAXV];
} OrcCell;

/* returns 0, or -2 if a cell ends up with more than MAX_V vertices (:1007) */
static int build_cells(int nx, int ny, const double *lon, const double *lat, OrcCell *c)
{
  double x[ORC_MV], y[ORC_MV];
  for (int ij = 0; ij < nx * ny; ij++) {
    int i = ij % nx, j = ij / nx;
    load_quad(lon, lat, nx + 1, i, j, x, y);
    c[ij].lat_min = vmin(4, y);
    c[ij].lat_max = vmax(4, y);
    int n = orc_fix_lon(x, y, 4, ORC_PI);
    if (n > ORC_MAXV) return -2;
    c[ij].lon_min = vmin(n, x);
    c[ij].lon_max = vmax(n, x);
    c[ij].lon_avg = vavg(n, x);
    c[ij].nv = n;
    for (int l = 0; l < n; l++) { c[ij].x[l] = x[l]; c[ij].y[l] = y[l]; }
  }
  return 0;
}

/*
 * The reference's brute-force exchange-grid search with nthreads == 1
 * (create_xgrid.c:1028-1101 for order 2, :750-826 for order 1).
 * order==1: xclon/xclat may be NULL.  j1_beg/j1_end restrict the source rows
 * scanned (used only by the multi-threaded CPU baseline; the full call passes
 * 0, ny1).  Returns nxgrid, -1 (parallel-edge fatal), -2 (n2 > MAX_V) or
 * -3 (capacity exceeded, the reference's MAXXGRID fatal :1087).
 */
long orc_create_xgrid_2dx2d_rows(int order, int nx1, int ny1, int nx2, int ny2,
                                 const double *lon_in, const double *lat_in,
                                 const double *lon_out, const double *lat_out,
                                 const double *mask_in, int j1_beg, int j1_end, long capacity,
                                 int *i_in, int *j_in, int *i_out, int *j_out,
                                 double *xarea, double *xclon, double *xclat)
{
  double *area_in = (double *)malloc(sizeof(double) * nx1 * ny1);
  double *area_out = (double *)malloc(sizeof(double) * nx2 * ny2);
  OrcCell *cells = (OrcCell *)malloc(sizeof(OrcCell) * (size_t)nx2 * ny2);
  long nxgrid = 0;

  orc_get_grid_area(nx1, ny1, lon_in, lat_in, area_in);
  orc_get_grid_area(nx2, ny2, lon_out, lat_out, area_out);
  int rc = build_cells(nx2, ny2, lon_out, lat_out, cells);
  if (rc) { nxgrid = rc; goto done; }

  for (int j1 = j1_beg; j1 < j1_end; j1++)
    for (int i1 = 0; i1 < nx1; i1++) {
      if (!(mask_in[j1 * nx1 + i1] > ORC_MASK_THRESH)) continue;
      double x1[ORC_MV], y1[ORC_MV], xo[ORC_MV], yo[ORC_MV];
      load_quad(lon_in, lat_in, nx1 + 1, i1, j1, x1, y1);
      double lat_in_min = vmin(4, y1);
      double lat_in_max = vmax(4, y1);
      int n1 = orc_fix_lon(x1, y1, 4, ORC_PI);
      double lon_in_min = vmin(n1, x1);
      double lon_in_max = vmax(n1, x1);
      double lon_in_avg = vavg(n1, x1);

      for (int ij = 0; ij < nx2 * ny2; ij++) {
        const OrcCell *c = &cells[ij];
        if (c->lat_min >= lat_in_max || c->lat_max <= lat_in_min) continue;
        int n2 = c->nv;
        double x2[ORC_MAXV], y2[ORC_MAXV];
        for (int l = 0; l < n2; l++) { x2[l] = c->x[l]; y2[l] = c->y[l]; }
        double lon_out_min = c->lon_min, lon_out_max = c->lon_max;
        double dx = c->lon_avg - lon_in_avg;
        if (dx < -ORC_PI) {
          lon_out_min += ORC_TPI; lon_out_max += ORC_TPI;
          for (int l = 0; l < n2; l++) x2[l] += ORC_TPI;
        } else if (dx > ORC_PI) {
          lon_out_min -= ORC_TPI; lon_out_max -= ORC_TPI;
          for (int l = 0; l < n2; l++) x2[l] -= ORC_TPI;
        }
        if (lon_out_min >= lon_in_max || lon_out_max <= lon_in_min) continue;
        int n_out = orc_clip_2dx2d(x1, y1, n1, x2, y2, n2, xo, yo);
        if (n_out < 0) { nxgrid = -1; goto done; }
        if (n_out > 0) {
          double xa = orc_poly_area(xo, yo, n_out) * mask_in[j1 * nx1 + i1];
          double a1 = area_in[j1 * nx1 + i1], a2 = area_out[ij];
          double min_area = (a1 < a2 ? a1 : a2);
          if (xa / min_area > ORC_AREA_RATIO_THRESH) {
            if (nxgrid >= capacity) { nxgrid = -3; goto done; }
            xarea[nxgrid] = xa;
            if (order == 2) {
              xclon[nxgrid] = orc_poly_ctrlon(xo, yo, n_out, lon_in_avg);
              xclat[nxgrid] = orc_poly_ctrlat(xo, yo, n_out);
            }
            i_in[nxgrid] = i1; j_in[nxgrid] = j1;
            i_out[nxgrid] = ij % nx2; j_out[nxgrid] = ij / nx2;
            nxgrid++;
          }
        }
      }
    }
done:
  free(area_in); free(area_out); free(cells);
  return nxgrid;
}

long orc_create_xgrid_2dx2d_order1(int nx1, int ny1, int nx2, int ny2,
                                   const double *lon_in, const double *lat_in,
                                   const double *lon_out, const double *lat_out,
                                   const double *mask_in, long capacity,
                                   int *i_in, int *j_in, int *i_out, int *j_out, double *xarea)
{
  return orc_create_xgrid_2dx2d_rows(1, nx1, ny1, nx2, ny2, lon_in, lat_in, lon_out, lat_out, mask_in,
                                     0, ny1, capacity, i_in, j_in, i_out, j_out, xarea, NULL, NULL);
}

long orc_create_xgrid_2dx2d_order2(int nx1, int ny1, int nx2, int ny2,
                                   const double *lon_in, const double *lat_in,
                                   const double *lon_out, const double *lat_out,
                                   const double *mask_in, long capacity,
                                   int *i_in, int *j_in, int *i_out, int *j_out,
                                   double *xarea, double *xclon, double *xclat)
{
  return orc_create_xgrid_2dx2d_rows(2, nx1, ny1, nx2, ny2, lon_in, lat_in, lon_out, lat_out, mask_in,
                                     0, ny1, capacity, i_in, j_in, i_out, j_out, xarea, xclon, xclat);
}

/* per-destination-cell records exposed for the get_grid_cell_struct parity test
 * (same quantities as the OpenACC twin tools/libfrencutils_gpu/create_xgrid_utils_gpu.c:646-701,
 *  defined by create_xgrid.c:991-1016) */
int orc_get_grid_cell_struct(int nx, int ny, const double *lon, const double *lat,
                             double *lat_min, double *lat_max, double *lon_min, double *lon_max,
                             double *lon_avg, int *nvert, double *vlon, double *vlat, double *area)
{
  OrcCell *c = (OrcCell *)malloc(sizeof(OrcCell) * (size_t)nx * ny);
  int rc = build_cells(nx, ny, lon, lat, c);
  if (!rc) {
    for (int ij = 0; ij < nx * ny; ij++) {
      lat_min[ij] = c[ij].lat_min; lat_max[ij] = c[ij].lat_max;
      lon_min[ij] = c[ij].lon_min; lon_max[ij] = c[ij].lon_max; lon_avg[ij] = c[ij].lon_avg;
      nvert[ij] = c[ij].nv;
      for (int l = 0; l < ORC_MAXV; l++) {
        vlon[ij * ORC_MAXV + l] = (l < c[ij].nv) ? c[ij].x[l] : 0.0;
        vlat[ij * ORC_MAXV + l] = (l < c[ij].nv) ? c[ij].y[l] : 0.0;
      }
      area[ij] = orc_poly_area(c[ij].x, c[ij].y, c[ij].nv);
    }
  }
  free(c);
  return rc;
}

/* ------------------------------------------------------------------------- */
/* setup_conserve_interp, compute branch: conserve_interp.c:127-358           */
/* ------------------------------------------------------------------------- */
/*
 * One destination tile per call chain is not enough: the per-source-cell sums
 * cell_in[m].{area,clon,clat} accumulate over ALL destination tiles (:136-147 sit
 * outside the n loop), so the whole (ntiles_out x ntiles_in) sweep is done here.
 *
 * Inputs are arrays of per-tile pointers.  cell_area_in[m] = get_grid_area of
 * source tile m (fregrid_util.c:363-390).  Outputs are concatenated over the
 * destination tiles; xoff[n]..xoff[n+1] is the slice for destination tile n
 * (xoff has ntiles_out+1 entries).  order 1: di/dj untouched (may be NULL).
 * Returns total nxgrid or a negative error code.
 */
long orc_setup_conserve_interp(int order, int ntiles_in, const int *nx_in, const int *ny_in,
                               const double *const *lon_in, const double *const *lat_in,
                               const double *const *cell_area_in,
                               int ntiles_out, const int *nx_out, const int *ny_out,
                               const double *const *lon_out, const double *const *lat_out,
                               long capacity, long *xoff,
                               int *t_in, int *i_in, int *j_in, int *i_out, int *j_out,
                               double *area, double *di, double *dj)
{
  long total = 0;
  double **ca = NULL, **cl = NULL, **ct = NULL;
  if (order == 2) {
    ca = (double **)malloc(sizeof(double *) * ntiles_in);
    cl = (double **)malloc(sizeof(double *) * ntiles_in);
    ct = (double **)malloc(sizeof(double *) * ntiles_in);
    for (int m = 0; m < ntiles_in; m++) {
      size_t nc = (size_t)nx_in[m] * ny_in[m];
      ca[m] = (double *)calloc(nc, sizeof(double));
      cl[m] = (double *)calloc(nc, sizeof(double));
      ct[m] = (double *)calloc(nc, sizeof(double));
    }
  }

  for (int n = 0; n < ntiles_out; n++) {
    xoff[n] = total;
    int nx2 = nx_out[n], ny2 = ny_out[n];
    double y_min = vmin((nx2 + 1) * (ny2 + 1), lat_out[n]);
    double y_max = vmax((nx2 + 1) * (ny2 + 1), lat_out[n]);
    for (int m = 0; m < ntiles_in; m++) {
      int nx1 = nx_in[m], ny1 = ny_in[m];
      double *mask = (double *)malloc(sizeof(double) * nx1 * ny1);
      for (int k = 0; k < nx1 * ny1; k++) mask[k] = 1.0;
      /* trim source rows to the destination latitude range (:169-184) */
      int jstart = ny1, jend = -1;
      for (int j = 0; j <= ny1; j++)
        for (int i = 0; i <= nx1; i++) {
          double yy = lat_in[m][j * (nx1 + 1) + i];
          if (yy > y_min) { if (j < jstart) jstart = j; }
          if (yy < y_max) { if (j > jend) jend = j; }
        }
      jstart = (0 > jstart - 1) ? 0 : jstart - 1;
      jend = (ny1 - 1 < jend + 1) ? ny1 - 1 : jend + 1;
      int ny_now = jend - jstart + 1;
      long nx;
      double *xcl = NULL, *xct = NULL;
      if (order == 2) {
        xcl = (double *)malloc(sizeof(double) * (capacity - total + 1));
        xct = (double *)malloc(sizeof(double) * (capacity - total + 1));
      }
      nx = orc_create_xgrid_2dx2d_rows(order, nx1, ny_now, nx2, ny2,
                                       lon_in[m] + jstart * (nx1 + 1), lat_in[m] + jstart * (nx1 + 1),
                                       lon_out[n], lat_out[n], mask, 0, ny_now, capacity - total,
                                       i_in + total, j_in + total, i_out + total, j_out + total,
                                       area + total, xcl, xct);
      free(mask);
      if (nx < 0) { free(xcl); free(xct); total = nx; goto cleanup; }
      for (long k = 0; k < nx; k++) {
        j_in[total + k] += jstart;                     /* :200 */
        t_in[total + k] = m;
      }
      if (order == 2) {
        for (long k = 0; k < nx; k++) {                /* :216-221 */
          long ii = (long)j_in[total + k] * nx1 + i_in[total + k];
          ca[m][ii] += area[total + k];
          cl[m][ii] += xcl[k];
          ct[m][ii] += xct[k];
        }
        for (long k = 0; k < nx; k++) {                /* :256-257, :303-304 */
          di[total + k] = xcl[k] / area[total + k];
          dj[total + k] = xct[k] / area[total + k];
        }
        free(xcl); free(xct);
      }
      total += nx;
    }
  }
  xoff[ntiles_out] = total;

  if (order == 2) {
    /* source-cell centroids (:321-350) */
    for (int m = 0; m < ntiles_in; m++) {
      int nx1 = nx_in[m], ny1 = ny_in[m];
      for (int j = 0; j < ny1; j++)
        for (int i = 0; i < nx1; i++) {
          long ii = (long)j * nx1 + i;
          if (!(ca[m][ii] > 0)) continue;
          if (fabs(ca[m][ii] - cell_area_in[m][ii]) / cell_area_in[m][ii] < ORC_CENTROID_AREA_RATIO) {
            cl[m][ii] /= ca[m][ii];
            ct[m][ii] /= ca[m][ii];
          } else {
            double x[ORC_MV], y[ORC_MV];
            load_quad(lon_in[m], lat_in[m], nx1 + 1, i, j, x, y);
            int nv = orc_fix_lon(x, y, 4, ORC_PI);
            double lon_avg = vavg(nv, x);
            double clon = orc_poly_ctrlon(x, y, nv, lon_avg);
            double clat = orc_poly_ctrlat(x, y, nv);
            cl[m][ii] = clon / cell_area_in[m][ii];
            ct[m][ii] = clat / cell_area_in[m][ii];
          }
        }
    }
    /* distances from the source-cell centroid (:351-357) */
    for (long k = 0; k < total; k++) {
      int m = t_in[k];
      long ii = (long)j_in[k] * nx_in[m] + i_in[k];
      di[k] -= cl[m][ii];
      dj[k] -= ct[m][ii];
    }
  }

cleanup:
  if (order == 2) {
    for (int m = 0; m < ntiles_in; m++) { free(ca[m]); free(cl[m]); free(ct[m]); }
    free(ca); free(cl); free(ct);
  }
  return total;
}

/* ------------------------------------------------------------------------- */
/* do_scalar_conserve_interp: conserve_interp.c:507-910, one destination tile */
/* ------------------------------------------------------------------------- */
/*
 * Plain (no --weight_field, no cell_measures/cell_methods=sum, not monotonic,
 * no --target_grid) branch, i.e. what `fregrid --interp_method conserve_order{1,2}`
 * executes for an ordinary scalar:  order 1 :561-616, order 2 :743-813,
 * normalisation :831-839, flux sums :815-819, :895-900.
 *
 * field layout (as the reference): order 1  data[tile][k][ny][nx]
 *                                  order 2  data[tile][k][ny+2][nx+2] (halo 1),
 *                                           grad_x/grad_y/grad_mask [tile][k][ny][nx]
 * has_missing requires nz == 1 (:544).  out[k][ny2][nx2].
 * gsum_out (may be NULL) receives the sum of out*area before normalisation.
 */
int orc_do_scalar_conserve_interp(int order, long nxgrid,
                                  const int *t_in, const int *i_in, const int *j_in,
                                  const int *i_out, const int *j_out,
                                  const double *area, const double *di, const double *dj,
                                  int ntiles_in, const int *nx_in, const int *ny_in,
                                  const double *const *data, const double *const *grad_x,
                                  const double *const *grad_y, const int *const *grad_mask,
                                  int has_missing, double missing_in,
                                  int nx2, int ny2, int nz, double *out, double *gsum_out)
{
  (void)ntiles_in;
  double missing = -ORC_MAXVAL;
  if (has_missing) missing = missing_in;
  if (nz > 1 && has_missing) return -1;
  size_t nout = (size_t)nx2 * ny2 * nz;
  double *out_area = (double *)calloc(nout, sizeof(double));
  int *out_miss = (int *)calloc(nout, sizeof(int));
  for (size_t k = 0; k < nout; k++) out[k] = 0.0;

  for (long n = 0; n < nxgrid; n++) {
    int i2 = i_out[n], j2 = j_out[n], i1 = i_in[n], j1 = j_in[n], tile = t_in[n];
    double a = area[n];
    int nx1 = nx_in[tile], ny1 = ny_in[tile];
    if (order == 1) {
      if (has_missing) {
        int n1 = j1 * nx1 + i1, n0 = j2 * nx2 + i2;
        if (data[tile][n1] != missing) {
          out[n0] += (data[tile][n1] * a);
          out_area[n0] += a;
          out_miss[n0] = 1;
        }
      } else {
        for (int k = 0; k < nz; k++) {
          size_t n1 = (size_t)k * nx1 * ny1 + j1 * nx1 + i1;
          size_t n0 = (size_t)k * nx2 * ny2 + j2 * nx2 + i2;
          out[n0] += (data[tile][n1] * a);
          out_area[n0] += a;
          out_miss[n0] = 1;
        }
      }
    } else {
      double d_i = di[n], d_j = dj[n];
      if (has_missing) {
        int n2 = (j1 + 1) * (nx1 + 2) + i1 + 1, n0 = j2 * nx2 + i2;
        if (data[tile][n2] != missing) {
          int n1 = j1 * nx1 + i1;
          if (grad_mask[tile][n1])
            out[n0] += data[tile][n2] * a;
          else
            out[n0] += (data[tile][n2] + grad_x[tile][n1] * d_i + grad_y[tile][n1] * d_j) * a;
          out_area[n0] += a;
          out_miss[n0] = 1;
        }
      } else {
        for (int k = 0; k < nz; k++) {
          size_t n0 = (size_t)k * nx2 * ny2 + j2 * nx2 + i2;
          size_t n1 = (size_t)k * nx1 * ny1 + j1 * nx1 + i1;
          size_t n2 = (size_t)k * (nx1 + 2) * (ny1 + 2) + (j1 + 1) * (nx1 + 2) + i1 + 1;
          out[n0] += (data[tile][n2] + grad_x[tile][n1] * d_i + grad_y[tile][n1] * d_j) * a;
          out_area[n0] += a;
          out_miss[n0] = 1;
        }
      }
    }
  }
  if (gsum_out) {
    double g = 0;
    for (size_t k = 0; k < nout; k++) if (out_area[k] > 0) g += out[k];
    *gsum_out = g;
  }
  for (size_t k = 0; k < nout; k++) {
    if (out_area[k] > 0) out[k] /= out_area[k];
    else if (out_miss[k] == 1) out[k] = 0.0;
    else out[k] = missing;
  }
  free(out_area); free(out_miss);
  return 0;
}

/* conserve_interp.c:895-900: input flux sum for the plain branch */
double orc_gsum_in(int order, int ntiles_in, const int *nx_in, const int *ny_in,
                   const double *const *data, const double *const *cell_area,
                   int has_missing, double missing_in, int nz)
{
  int halo = (order == 2) ? 1 : 0;
  double missing = -ORC_MAXVAL;
  if (has_missing) missing = missing_in;
  double g = 0;
  for (int n = 0; n < ntiles_in; n++) {
    int nx1 = nx_in[n], ny1 = ny_in[n];
    for (int k = 0; k < nz; k++)
      for (int j = 0; j < ny1; j++)
        for (int i = 0; i < nx1; i++) {
          double dd = data[n][(size_t)k * (nx1 + 2 * halo) * (ny1 + 2 * halo) + (j + halo) * (nx1 + 2 * halo) + i + halo];
          if (dd != missing) g += dd * cell_area[n][j * nx1 + i];
        }
  }
  return g;
}

/* ------------------------------------------------------------------------------------------------
 * do_scalar_conserve_interp with every branch (conserve_interp.c:507-910): source weight field
 * (weight_exist, :574,:608,:737,:757,:799), cell_methods = sum (:580,:612,:741,:767,:803, final :821-830),
 * cell_measures (:582-588,:614,:743,:769-775,:805, area_missing fatal), the monotone limiter (:617-748) and the
 * --target_grid rescale (:842-869).  Test infrastructure only.  Pinned bit for bit to the reference's own
 * do_scalar_conserve_interp (oracle/_ref/libconserve_ref.so) by tests/test_conserve_interp_vs_ref.py; it must also
 * reproduce orc_do_scalar_conserve_interp above bit for bit when all options are off.
 * weight, field_area, cell_area_in: per tile [ny][nx] (NULL pointer = option off; cell_area_in required for
 * sum/measures/target with measures).  Returns 0 or the code of the reference's fatal check (tests/orc.py
 * ORC_APPLY_ERRORS holds its message): -1, -5, -6 (nz > 1 with has_missing, cell_measures, sum; :544-546), -2 ("data is
 * not missing but area is missing"), -3 (" xdata is greater than f_bar_max "), -4 (" xdata is less than f_bar_min ").
 * Monotone: the reference indexes level 0 only and takes nx1 from the last tile (:648-651); tiles of one mosaic
 * have equal sizes, so nx_in[tile] is used.  One process: the mpp_min/max_double of :672-677 are identities. */
#define ORC_TOLERANCE 1.e-10                 /* conserve_interp.c:37 */
int orc_do_scalar_conserve_interp_ex(int order, long nxgrid,
                                     const int *t_in, const int *i_in, const int *j_in,
                                     const int *i_out, const int *j_out,
                                     const double *area_x, const double *di_x, const double *dj_x,
                                     int ntiles_in, const int *nx_in, const int *ny_in,
                                     const double *const *data, const double *const *grad_x,
                                     const double *const *grad_y, const int *const *grad_mask,
                                     int has_missing, double missing_in,
                                     const double *const *weight, int cell_methods_sum,
                                     const double *const *field_area, double area_missing,
                                     const double *const *cell_area_in,
                                     int target_grid, const double *cell_area_out, int monotonic_in,
                                     int nx2, int ny2, int nz, double *out, double *gsum_out)
{
  const int weight_exist = weight != NULL, cell_measures = field_area != NULL;
  const int monotonic = (order == 2) ? monotonic_in : 0;                 /* :525-531 */
  double missing = -ORC_MAXVAL;
  if (has_missing) missing = missing_in;
  if (nz > 1 && has_missing) return -1;
  if (nz > 1 && cell_measures) return -5;
  if (nz > 1 && cell_methods_sum) return -6;
  size_t nout = (size_t)nx2 * ny2 * nz;
  double *out_area = (double *)calloc(nout, sizeof(double));
  int *out_miss = (int *)calloc(nout, sizeof(int));
  int rc = 0;
  for (size_t k = 0; k < nout; k++) out[k] = 0.0;

  if (order == 1) {
    for (long n = 0; n < nxgrid && !rc; n++) {
      int i2 = i_out[n], j2 = j_out[n], i1 = i_in[n], j1 = j_in[n], tile = t_in[n];
      double area = area_x[n];
      int nx1 = nx_in[tile], ny1 = ny_in[tile];
      if (weight_exist) area *= weight[tile][j1 * nx1 + i1];
      if (has_missing) {
        int n1 = j1 * nx1 + i1, n0 = j2 * nx2 + i2;
        if (data[tile][n1] != missing) {
          if (cell_methods_sum) area /= cell_area_in[tile][n1];
          else if (cell_measures) {
            if (field_area[tile][n1] == area_missing) { rc = -2; break; }
            area *= (field_area[tile][n1] / cell_area_in[tile][n1]);
          }
          out[n0] += (data[tile][n1] * area);
          out_area[n0] += area;
          out_miss[n0] = 1;
        }
      } else {
        for (int k = 0; k < nz; k++) {
          size_t n1 = (size_t)k * nx1 * ny1 + j1 * nx1 + i1;
          size_t n0 = (size_t)k * nx2 * ny2 + j2 * nx2 + i2;
          if (cell_methods_sum) area /= cell_area_in[tile][n1];
          else if (cell_measures) area *= (field_area[tile][n1] / cell_area_in[tile][n1]);
          out[n0] += (data[tile][n1] * area);
          out_area[n0] += area;
          out_miss[n0] = 1;
        }
      }
    }
  } else if (monotonic) {
    double **fbmax = (double **)malloc(ntiles_in * sizeof(double *)), **fbmin = (double **)malloc(ntiles_in * sizeof(double *));
    double **fmax = (double **)malloc(ntiles_in * sizeof(double *)), **fmin = (double **)malloc(ntiles_in * sizeof(double *));
    for (int n = 0; n < ntiles_in; n++) {
      int nx1 = nx_in[n], ny1 = ny_in[n];
      fbmax[n] = (double *)malloc((size_t)nx1 * ny1 * sizeof(double)); fbmin[n] = (double *)malloc((size_t)nx1 * ny1 * sizeof(double));
      fmax[n] = (double *)malloc((size_t)nx1 * ny1 * sizeof(double));  fmin[n] = (double *)malloc((size_t)nx1 * ny1 * sizeof(double));
      for (int j = 0; j < ny1; j++) for (int i = 0; i < nx1; i++) {
        int n1 = j * nx1 + i;
        fbmax[n][n1] = -ORC_MAXVAL; fbmin[n][n1] = ORC_MAXVAL; fmax[n][n1] = -ORC_MAXVAL; fmin[n][n1] = ORC_MAXVAL;
        for (int jj = j - 1; jj <= j + 1; jj++) for (int ii = i - 1; ii <= i + 1; ii++) {
          int n2 = (jj + 1) * (nx1 + 2) + ii + 1;
          if (data[n][n2] != missing) {
            if (data[n][n2] > fbmax[n][n1]) fbmax[n][n1] = data[n][n2];
            if (data[n][n2] < fbmin[n][n1]) fbmin[n][n1] = data[n][n2];
          }
        }
      }
    }
    double *xdata = (double *)malloc((nxgrid > 0 ? nxgrid : 1) * sizeof(double));
    for (long n = 0; n < nxgrid; n++) {
      int i1 = i_in[n], j1 = j_in[n], tile = t_in[n], nx1 = nx_in[tile];
      double di = di_x[n], dj = dj_x[n];
      int n1 = j1 * nx1 + i1, n2 = (j1 + 1) * (nx1 + 2) + i1 + 1;
      if (data[tile][n2] != missing) {
        if (grad_mask && grad_mask[tile] && grad_mask[tile][n1]) xdata[n] = data[tile][n2];
        else xdata[n] = data[tile][n2] + grad_x[tile][n1] * di + grad_y[tile][n1] * dj;
        if (xdata[n] > fmax[tile][n1]) fmax[tile][n1] = xdata[n];
        if (xdata[n] < fmin[tile][n1]) fmin[tile][n1] = xdata[n];
      } else
        xdata[n] = missing;
    }
    for (long n = 0; n < nxgrid && !rc; n++) {
      int i1 = i_in[n], j1 = j_in[n], tile = t_in[n], nx1 = nx_in[tile];
      int n1 = j1 * nx1 + i1, n2 = (j1 + 1) * (nx1 + 2) + i1 + 1;
      double f_bar = data[tile][n2];
      if (xdata[n] == missing) continue;
      if (fmax[tile][n1] > fbmax[tile][n1]) {
        xdata[n] = f_bar + ((xdata[n] - f_bar) / (fmax[tile][n1] - f_bar)) * (fbmax[tile][n1] - f_bar);
        if (xdata[n] > fbmax[tile][n1]) {
          if (xdata[n] - fbmax[tile][n1] < ORC_TOLERANCE) xdata[n] = fbmax[tile][n1];
          if (xdata[n] > fbmax[tile][n1]) rc = -3;
        }
      } else if (fmin[tile][n1] < fbmin[tile][n1]) {
        xdata[n] = f_bar + ((xdata[n] - f_bar) / (fmin[tile][n1] - f_bar)) * (fbmin[tile][n1] - f_bar);
        if (xdata[n] < fbmin[tile][n1]) {
          if (fbmin[tile][n1] - xdata[n] < ORC_TOLERANCE) xdata[n] = fbmin[tile][n1];
          if (xdata[n] < fbmin[tile][n1]) rc = -4;
        }
      }
    }
    for (int n = 0; n < ntiles_in; n++) { free(fbmax[n]); free(fbmin[n]); free(fmax[n]); free(fmin[n]); }
    free(fbmax); free(fbmin); free(fmax); free(fmin);
    for (long n = 0; n < nxgrid && !rc; n++) {
      int i2 = i_out[n], j2 = j_out[n], i1 = i_in[n], j1 = j_in[n], tile = t_in[n], nx1 = nx_in[tile];
      double area = area_x[n];
      if (xdata[n] == missing) continue;
      if (weight_exist) area *= weight[tile][j1 * nx1 + i1];
      int n1 = j1 * nx1 + i1, n0 = j2 * nx2 + i2;
      if (cell_methods_sum) area /= cell_area_in[tile][n1];
      else if (cell_measures) area *= (field_area[tile][n1] / cell_area_in[tile][n1]);
      out[n0] += xdata[n] * area;
      out_area[n0] += area;
    }
    free(xdata);
  } else {
    for (long n = 0; n < nxgrid && !rc; n++) {
      int i2 = i_out[n], j2 = j_out[n], i1 = i_in[n], j1 = j_in[n], tile = t_in[n];
      double di = di_x[n], dj = dj_x[n], area = area_x[n];
      int nx1 = nx_in[tile], ny1 = ny_in[tile];
      if (weight_exist) area *= weight[tile][j1 * nx1 + i1];
      if (has_missing) {
        int n2 = (j1 + 1) * (nx1 + 2) + i1 + 1, n0 = j2 * nx2 + i2;
        if (data[tile][n2] != missing) {
          int n1 = j1 * nx1 + i1;
          if (cell_methods_sum) area /= cell_area_in[tile][n1];
          else if (cell_measures) {
            if (field_area[tile][n1] == area_missing) { rc = -2; break; }
            area *= (field_area[tile][n1] / cell_area_in[tile][n1]);
          }
          if (grad_mask[tile][n1]) out[n0] += data[tile][n2] * area;
          else out[n0] += (data[tile][n2] + grad_x[tile][n1] * di + grad_y[tile][n1] * dj) * area;
          out_area[n0] += area;
          out_miss[n0] = 1;
        }
      } else {
        for (int k = 0; k < nz; k++) {
          size_t n0 = (size_t)k * nx2 * ny2 + j2 * nx2 + i2;
          size_t n1 = (size_t)k * nx1 * ny1 + j1 * nx1 + i1;
          size_t n2 = (size_t)k * (nx1 + 2) * (ny1 + 2) + (j1 + 1) * (nx1 + 2) + i1 + 1;
          if (cell_methods_sum) area /= cell_area_in[tile][n1];
          else if (cell_measures) area *= (field_area[tile][n1] / cell_area_in[tile][n1]);
          out[n0] += (data[tile][n2] + grad_x[tile][n1] * di + grad_y[tile][n1] * dj) * area;
          out_area[n0] += area;
          out_miss[n0] = 1;
        }
      }
    }
  }
  if (rc) { free(out_area); free(out_miss); return rc; }

  if (gsum_out) {                                                        /* :815-819 */
    double g = 0;
    for (size_t k = 0; k < nout; k++) if (out_area[k] > 0) g += out[k];
    *gsum_out = g;
  }
  if (cell_methods_sum) {                                                /* :821-830 */
    for (size_t i = 0; i < nout; i++)
      if (out_area[i] == 0) {
        if (out_miss[i] == 0) out[i] = missing;
        else out[i] = 0.0;
      }
  } else {
    for (size_t i = 0; i < nout; i++) {                                  /* :832-839 */
      if (out_area[i] > 0) out[i] /= out_area[i];
      else if (out_miss[i] == 1) out[i] = 0.0;
      else out[i] = missing;
    }
    if (target_grid) {                                                   /* :842-869 */
      for (int i = 0; i < nx2 * ny2; i++) out_area[i] = 0.0;
      for (long n = 0; n < nxgrid; n++) {
        int i2 = i_out[n], j2 = j_out[n], i1 = i_in[n], j1 = j_in[n], tile = t_in[n];
        double area = area_x[n];
        int nx1 = nx_in[tile];
        int n0 = j2 * nx2 + i2, n1 = j1 * nx1 + i1;
        if (cell_measures) out_area[n0] += (area * field_area[tile][n1] / cell_area_in[tile][n1]);
        else out_area[n0] += area;
      }
      for (size_t i = 0; i < nout; i++)
        if (out[i] != missing) {
          size_t i2 = i % ((size_t)nx2 * ny2);
          out[i] *= (out_area[i2] / cell_area_out[i2]);
        }
    }
  }
  free(out_area); free(out_miss);
  return 0;
}

/* conserve_interp.c:874-900: the three input flux sums */
double orc_gsum_in_ex(int order, int ntiles_in, const int *nx_in, const int *ny_in, const double *const *data,
                      const double *const *cell_area, const double *const *field_area, int cell_methods_sum,
                      int has_missing, double missing_in, int nz)
{
  int halo = (order == 2) ? 1 : 0;
  double missing = -ORC_MAXVAL;
  if (has_missing) missing = missing_in;
  double g = 0;
  for (int n = 0; n < ntiles_in; n++) {
    int nx1 = nx_in[n], ny1 = ny_in[n];
    if (field_area) {
      for (int j = 0; j < ny1; j++) for (int i = 0; i < nx1; i++) {
        double dd = data[n][(j + halo) * (nx1 + 2 * halo) + i + halo];
        if (dd != missing) g += dd * field_area[n][j * nx1 + i];
      }
    } else if (cell_methods_sum) {
      for (int j = 0; j < ny1; j++) for (int i = 0; i < nx1; i++) {
        double dd = data[n][(j + halo) * (nx1 + 2 * halo) + i + halo];
        if (dd != missing) g += dd;
      }
    } else {
      for (int k = 0; k < nz; k++) for (int j = 0; j < ny1; j++) for (int i = 0; i < nx1; i++) {
        double dd = data[n][(size_t)k * (nx1 + 2 * halo) * (ny1 + 2 * halo) + (j + halo) * (nx1 + 2 * halo) + i + halo];
        if (dd != missing) g += dd * cell_area[n][j * nx1 + i];
      }
    }
  }
  return g;
}

/* libm's sin / cos on an array (the device's latitude trig must equal these bit for bit, tests/test_gpu_xgrid.py) */
void orc_sincos(long n, const double *x, double *s, double *c)
{
  for (long i = 0; i < n; i++) { s[i] = sin(x[i]); c[i] = cos(x[i]); }
}
