/* bilinear_host.c -- host pieces of the bilinear path that must round like the reference's gcc -O2 build with the host
 * libm (tools/fregrid/fregrid_util.c, tools/libfrencutils/mosaic_util.c), and the bilinear remap file
 * (tools/fregrid/bilinear_interp.c:110-125 READ, :408-426 WRITE) over the classic-netCDF code of field_file.c. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "fregrid_hip.h"

#define BL_D2R (M_PI / 180)

/* unit_vect_latlon (mosaic_util.c:937-956) */
void fg_unit_vect_latlon(long size, const double *lon, const double *lat, double *vlon, double *vlat)
{
  long n;
  for (n = 0; n < size; n++) {
    double sin_lon = sin(lon[n]);
    double cos_lon = cos(lon[n]);
    double sin_lat = sin(lat[n]);
    double cos_lat = cos(lat[n]);
    vlon[3 * n] = -sin_lon;
    vlon[3 * n + 1] = cos_lon;
    vlon[3 * n + 2] = 0.;
    vlat[3 * n] = -sin_lat * cos_lon;
    vlat[3 * n + 1] = -sin_lat * sin_lon;
    vlat[3 * n + 2] = cos_lat;
  }
}

/* the fine grid of get_output_grid_by_size's BILINEAR branch (fregrid_util.c:611-641): lont / latt [ny_fine][nx_fine],
 * latt1D_fine [ny_fine]; radians */
void fg_bilin_fine_grid(int nlon, int nlat, int finer_step, double lonbegin, double lonend, double latbegin, double latend,
                        int center_y, double *lont, double *latt, double *latt1d)
{
  const int nx_fine = (int)(pow(2, finer_step) * nlon), ny_fine = (int)(pow(2, finer_step) * (nlat - 1) + 1);
  const double lon_range = lonend - lonbegin, lat_range = latend - latbegin;
  double dlon, dlat;
  int i, j;
  dlon = lon_range / nx_fine;
  for (i = 0; i < nx_fine; i++) {
    double lon_fine = (lonbegin + (i + 0.5) * dlon) * BL_D2R;
    for (j = 0; j < ny_fine; j++) lont[j * nx_fine + i] = lon_fine;
  }
  if (center_y) {
    dlat = lat_range / ny_fine;
    for (j = 0; j < ny_fine; j++) latt1d[j] = (latbegin + (j + 0.5) * dlat) * BL_D2R;
  } else {
    dlat = lat_range / (ny_fine - 1);
    for (j = 0; j < ny_fine; j++) latt1d[j] = (latbegin + j * dlat) * BL_D2R;
  }
  for (j = 0; j < ny_fine; j++)
    for (i = 0; i < nx_fine; i++) latt[j * nx_fine + i] = latt1d[j];
}

/* redu2x's cosine factors for one coarsening step (bilinear_interp.c:1075-1081): cosp[0] = cosp[ny-1] = 0, acosp on 1..ny-2;
 * ylat == NULL: the -90..90 latitudes do_latlon_coarsening regenerates for steps >= 2 (:1030-1033) */
void fg_bilin_redu2x_coef(int ny, const double *ylat, double *cosp, double *acosp)
{
  double *y = (double *)malloc(ny * sizeof(double));
  int j;
  if (ylat) memcpy(y, ylat, ny * sizeof(double));
  else {
    double dlat = M_PI / (ny - 1);
    y[0] = -0.5 * M_PI;
    y[ny - 1] = 0.5 * M_PI;
    for (j = 1; j < ny - 1; j++) y[j] = y[0] + j * dlat;
  }
  cosp[0] = 0.;
  cosp[ny - 1] = 0.;
  acosp[0] = acosp[ny - 1] = 0.;
  for (j = 1; j < ny - 1; j++) cosp[j] = cos(y[j]);
  for (j = 1; j < ny - 1; j++) acosp[j] = 1. / (cosp[j] + 0.5 * (cosp[j - 1] + cosp[j + 1]));
  free(y);
}

/* normalize_great_circle_distance (bilinear_interp.c:743-755) with the host libm's acos */
static double bl_ngcd(const double *v1, const double *v2)
{
  double dist;
  dist = (v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]) /
         sqrt((v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]) * (v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2]));
  {
    double m = 1. < fabs(dist) ? 1. : fabs(dist);
    dist = dist < 0 ? -fabs(m) : fabs(m);
  }
  return acos(dist);
}

/* the distance dcub scales in the search window (:146-152): cell (jc, ic) -> centre (jc+1, ic+1), for the cells c0 <= c < c1
 * (c = l*N*N + (jc-1)*N + ic-1); x, y, z: halo'd centres [6][N+2][N+2] (the halo corner of the last cell is the zero one) */
void fg_bilin_cell_dist(int N, long c0, long c1, const double *x, const double *y, const double *z, double *dist)
{
  const long nxd = N + 2, T = nxd * nxd;
  long c;
  for (c = c0; c < c1; c++) {
    const long l = c / ((long)N * N), rem = c - l * N * N, jc = rem / N + 1, ic = rem % N + 1;
    const long n1 = l * T + jc * nxd + ic, n2 = l * T + (jc + 1) * nxd + ic + 1;
    const double v1[3] = {x[n1], y[n1], z[n1]}, v2[3] = {x[n2], y[n2], z[n2]};
    dist[c] = bl_ngcd(v1, v2);
  }
}

/* the tail of dist2side (:806-815), asin(sin(side) * sin(angle)) with side = acos(side_cos), on n values.  angle is
 * spherical_angle's acosl(acos_arg) rounded to double (mosaic_util.c:834) where acos_arg is not NaN, else the device's angle of
 * the other branches */
void fg_bilin_dist2side_tail(long n, const double *angle, const double *acos_arg, const double *side_cos, double *dist)
{
  long k;
  for (k = 0; k < n; k++) {
    const double side = acos(side_cos[k]);
    const double a = isnan(acos_arg[k]) ? angle[k] : (double)acosl(acos_arg[k]);
    dist[k] = asin(sin(side) * sin(a));
  }
}

/* WRITE branch (:408-426): dimensions nlon, nlat, three, four; index NC_INT (three, nlat, nlon), weight NC_DOUBLE
 * (four, nlat, nlon), each written from the point-major arrays index[n][3] / weight[n][4] as they lie in memory */
int fg_bilin_remap_write(const char *path, int nlon_fine, int nlat_fine, const int *index, const double *weight)
{
  fg_ncfile *f = NULL;
  int rc, d[4], dims[3], vi, vw;
  long start[3] = {0, 0, 0}, c3[3] = {3, nlat_fine, nlon_fine}, c4[3] = {4, nlat_fine, nlon_fine};
  if (!path || !index || !weight || nlon_fine < 1 || nlat_fine < 1) return FG_ERR_ARG;
  if ((rc = fg_nc_create(path, 2, &f))) return rc;
  d[0] = fg_nc_def_dim(f, "nlon", nlon_fine);
  d[1] = fg_nc_def_dim(f, "nlat", nlat_fine);
  d[2] = fg_nc_def_dim(f, "three", 3);
  d[3] = fg_nc_def_dim(f, "four", 4);
  dims[0] = d[2]; dims[1] = d[1]; dims[2] = d[0];
  vi = fg_nc_def_var(f, "index", FG_NC_INT, 3, dims);
  dims[0] = d[3];
  vw = fg_nc_def_var(f, "weight", FG_NC_DOUBLE, 3, dims);
  rc = (d[0] < 0 || d[1] < 0 || d[2] < 0 || d[3] < 0 || vi < 0 || vw < 0) ? FG_ERR_IO : 0;
  if (!rc) rc = fg_nc_enddef(f);
  if (!rc) rc = fg_nc_put_vara(f, vi, start, c3, index);
  if (!rc) rc = fg_nc_put_vara(f, vw, start, c4, weight);
  {
    int rc2 = fg_nc_close(f);
    if (!rc) rc = rc2;
  }
  return rc;
}

/* READ branch (:110-125): the file's nlon / nlat must equal the fine grid's; index / weight read whole into the point-major
 * arrays.  Returns 0, FG_ERR_ARG on a size mismatch, FG_ERR_NOTFOUND when a dimension or variable is missing, or FG_ERR_IO. */
int fg_bilin_remap_read(const char *path, int nlon_fine, int nlat_fine, int *index, double *weight)
{
  fg_ncfile *f = NULL;
  int rc, dx, dy, vi, vw;
  long nx2 = 0, ny2 = 0, start[3] = {0, 0, 0}, c3[3] = {3, nlat_fine, nlon_fine}, c4[3] = {4, nlat_fine, nlon_fine};
  if (!path || !index || !weight) return FG_ERR_ARG;
  if ((rc = fg_nc_open(path, &f))) return rc;
  dx = fg_nc_inq_dimid(f, "nlon");
  dy = fg_nc_inq_dimid(f, "nlat");
  vi = fg_nc_inq_varid(f, "index");
  vw = fg_nc_inq_varid(f, "weight");
  if (dx < 0 || dy < 0 || vi < 0 || vw < 0) rc = FG_ERR_NOTFOUND;
  if (!rc) rc = fg_nc_inq_dim(f, dx, NULL, 0, &nx2);
  if (!rc) rc = fg_nc_inq_dim(f, dy, NULL, 0, &ny2);
  if (!rc && (nx2 != nlon_fine || ny2 != nlat_fine)) rc = FG_ERR_ARG;
  if (!rc) {
    int type = 0, nd = 0;
    long shape[8];
    rc = fg_nc_inq_var(f, vi, NULL, 0, &type, &nd, NULL, shape);
    if (!rc && (type != FG_NC_INT || nd != 3 || shape[0] != 3 || shape[1] != nlat_fine || shape[2] != nlon_fine)) rc = FG_ERR_IO;
    if (!rc) rc = fg_nc_inq_var(f, vw, NULL, 0, &type, &nd, NULL, shape);
    if (!rc && (type != FG_NC_DOUBLE || nd != 3 || shape[0] != 4 || shape[1] != nlat_fine || shape[2] != nlon_fine)) rc = FG_ERR_IO;
  }
  if (!rc) rc = fg_nc_get_vara(f, vi, start, c3, index);
  if (!rc) rc = fg_nc_get_vara(f, vw, start, c4, weight);
  fg_nc_close(f);
  return rc;
}
