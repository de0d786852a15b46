/* bilinear_ref_driver.c -- TEST HARNESS ONLY (tests/golden/make_golden_bilinear.py): runs the reference's
 * setup_bilinear_interp / do_scalar_bilinear_interp / do_vector_bilinear_interp (tools/fregrid/bilinear_interp.c, compiled
 * with mosaic_util.c and mpp.c in a temporary directory outside the repository) on one configuration and dumps what they
 * produce.  The Grid_config structs are filled the way get_input_grid (fregrid_util.c:236-312) and get_output_grid_by_size
 * (:564-641) fill them; the halo'd centres come from the caller.  The mpp_io calls of the WRITE / READ branches are served by
 * the stubs below, which record the layout the WRITE branch requests and the raw buffers it hands over (no libnetcdf here).
 *
 *   bilinear_ref_driver IN OUTDIR
 *   IN: int N, nlon, nlat, finer_step, center_y, setup_only; double lonbegin, lonend, latbegin, latend, missing;
 *       double lont[6][F], latt[6][F], s[6][F], s_miss[6][F], u[6][F], v[6][F]   (F = (N+2)^2, halo filled, corners 0)
 *   OUT: index.bin weight.bin s_plain.bin s_miss.bin s_fill.bin u.bin v.bin layout.txt put_index.bin put_weight.bin setup_s.txt */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <time.h>
#include "globals.h"
#include "mosaic_util.h"
#include "bilinear_interp.h"
#include "mpp.h"
#include "mpp_io.h"

#define DRV_EPSLN10 (1.e-10)      /* fregrid.c's EPSLN10 */

static const char *g_out;
static FILE *g_layout;
static int g_ndim = 0, g_dimlen[16];
static int g_nvar = 0, g_vtype[16], g_vnd[16], g_vdims[16][8];
static char g_vname[16][64];

static void path(char *buf, const char *name) { snprintf(buf, 4096, "%s/%s", g_out, name); }

int mpp_open(const char *file, int action)
{
  char p[4096];
  (void)action;
  path(p, "layout.txt");
  g_layout = fopen(p, "w");
  fprintf(g_layout, "file %s\n", file);
  return 0;
}
int mpp_def_dim(int fid, const char *name, int size)
{
  (void)fid;
  fprintf(g_layout, "dim %s %d\n", name, size);
  g_dimlen[g_ndim] = size;
  return g_ndim++;
}
int mpp_def_var(int fid, const char *name, nc_type type, int ndim, const int *dims, int natts, ...)
{
  int k;
  (void)fid; (void)natts;
  fprintf(g_layout, "var %s %d %d", name, (int)type, ndim);
  for (k = 0; k < ndim; k++) { fprintf(g_layout, " %d", dims[k]); g_vdims[g_nvar][k] = dims[k]; }
  fprintf(g_layout, "\n");
  strncpy(g_vname[g_nvar], name, 63);
  g_vtype[g_nvar] = (int)type; g_vnd[g_nvar] = ndim;
  return g_nvar++;
}
void mpp_end_def(int fid) { (void)fid; fprintf(g_layout, "enddef\n"); }
void mpp_put_var_value(int fid, int vid, const void *data)
{
  char name[128], p[4096];
  size_t n = 1, sz = g_vtype[vid] == 4 ? 4 : 8;
  int k;
  FILE *f;
  (void)fid;
  for (k = 0; k < g_vnd[vid]; k++) n *= (size_t)g_dimlen[g_vdims[vid][k]];
  snprintf(name, sizeof name, "put_%s.bin", g_vname[vid]);
  path(p, name);
  f = fopen(p, "wb");
  fwrite(data, sz, n, f);
  fclose(f);
  fprintf(g_layout, "put %s %zu\n", g_vname[vid], n);
}
void mpp_close(int fid) { (void)fid; if (g_layout) fclose(g_layout); g_layout = NULL; }
int mpp_get_dimlen(int fid, const char *name) { (void)fid; (void)name; mpp_error("driver: READ branch not driven"); return 0; }
int mpp_get_varid(int fid, const char *varname) { (void)fid; (void)varname; mpp_error("driver: READ branch not driven"); return 0; }
void mpp_get_var_value(int fid, int vid, void *data) { (void)fid; (void)vid; (void)data; mpp_error("driver: READ branch not driven"); }

static void dump(const char *name, const void *p, size_t sz, size_t n)
{
  char q[4096];
  FILE *f;
  path(q, name);
  f = fopen(q, "wb");
  fwrite(p, sz, n, f);
  fclose(f);
}
static void rd(FILE *f, void *p, size_t sz, size_t n)
{
  if (fread(p, sz, n, f) != n) { fprintf(stderr, "driver: short input\n"); exit(2); }
}

int main(int argc, char **argv)
{
  int hdr[6], N, nlon, nlat, fs, center_y, setup_only, n, i, j, F, nxf, nyf, npts;
  double dh[5], lonbegin, lonend, latbegin, latend, missing, dlon, dlat, *tile_in[4][6];
  Grid_config grid_in[6], grid_out;
  Interp_config interp;
  Field_config fin[6], fout, uin[6], vin[6], uout, vout;
  Var_config var;
  FILE *f;
  clock_t t0;
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUTDIR\n", argv[0]); return 2; }
  g_out = argv[2];
  f = fopen(argv[1], "rb");
  if (!f) return 2;
  rd(f, hdr, sizeof(int), 6);
  rd(f, dh, sizeof(double), 5);
  N = hdr[0]; nlon = hdr[1]; nlat = hdr[2]; fs = hdr[3]; center_y = hdr[4]; setup_only = hdr[5];
  lonbegin = dh[0]; lonend = dh[1]; latbegin = dh[2]; latend = dh[3]; missing = dh[4];
  F = (N + 2) * (N + 2);
  memset(grid_in, 0, sizeof grid_in);
  for (n = 0; n < 6; n++) {
    grid_in[n].nx = N; grid_in[n].ny = N;
    grid_in[n].lont = malloc(F * sizeof(double)); grid_in[n].latt = malloc(F * sizeof(double));
  }
  for (n = 0; n < 6; n++) rd(f, grid_in[n].lont, sizeof(double), F);
  for (n = 0; n < 6; n++) rd(f, grid_in[n].latt, sizeof(double), F);
  for (i = 0; i < 4; i++)
    for (n = 0; n < 6; n++) { tile_in[i][n] = malloc(F * sizeof(double)); if (!setup_only) rd(f, tile_in[i][n], sizeof(double), F); }
  fclose(f);
  /* get_input_grid's BILINEAR branch (fregrid_util.c:300-312) */
  for (n = 0; n < 6; n++) {
    grid_in[n].vlon_t = malloc(3 * F * sizeof(double)); grid_in[n].vlat_t = malloc(3 * F * sizeof(double));
    grid_in[n].xt = malloc(F * sizeof(double)); grid_in[n].yt = malloc(F * sizeof(double)); grid_in[n].zt = malloc(F * sizeof(double));
    latlon2xyz(F, grid_in[n].lont, grid_in[n].latt, grid_in[n].xt, grid_in[n].yt, grid_in[n].zt);
    unit_vect_latlon(F, grid_in[n].lont, grid_in[n].latt, grid_in[n].vlon_t, grid_in[n].vlat_t);
  }
  /* get_output_grid_by_size's BILINEAR branch (fregrid_util.c:564-641) */
  memset(&grid_out, 0, sizeof grid_out);
  grid_out.nx = nlon; grid_out.ny = nlat;
  grid_out.nx_fine = nxf = pow(2, fs) * nlon;
  grid_out.ny_fine = nyf = pow(2, fs) * (nlat - 1) + 1;
  npts = nxf * nyf;
  grid_out.latt1D_fine = malloc(nyf * sizeof(double));
  grid_out.lont = malloc(npts * sizeof(double)); grid_out.latt = malloc(npts * sizeof(double));
  grid_out.xt = malloc(npts * sizeof(double)); grid_out.yt = malloc(npts * sizeof(double)); grid_out.zt = malloc(npts * sizeof(double));
  grid_out.vlon_t = malloc(3 * npts * sizeof(double)); grid_out.vlat_t = malloc(3 * npts * sizeof(double));
  dlon = (lonend - lonbegin) / nxf;
  for (i = 0; i < nxf; i++) {
    double lon_fine = (lonbegin + (i + 0.5) * dlon) * D2R;
    for (j = 0; j < nyf; j++) grid_out.lont[j * nxf + i] = lon_fine;
  }
  if (center_y) {
    dlat = (latend - latbegin) / nyf;
    for (j = 0; j < nyf; j++) grid_out.latt1D_fine[j] = (latbegin + (j + 0.5) * dlat) * D2R;
  } else {
    dlat = (latend - latbegin) / (nyf - 1);
    for (j = 0; j < nyf; j++) grid_out.latt1D_fine[j] = (latbegin + j * dlat) * D2R;
  }
  for (j = 0; j < nyf; j++) for (i = 0; i < nxf; i++) grid_out.latt[j * nxf + i] = grid_out.latt1D_fine[j];
  latlon2xyz(npts, grid_out.lont, grid_out.latt, grid_out.xt, grid_out.yt, grid_out.zt);
  unit_vect_latlon(npts, grid_out.lont, grid_out.latt, grid_out.vlon_t, grid_out.vlat_t);
  /* fregrid.c:944-963 */
  {
    double dlon_in, dlat_in, lonbegin_in, latbegin_in;
    dlon_in = (fabs(lonend - lonbegin - 360) < DRV_EPSLN10) ? M_PI + M_PI : (lonend - lonbegin) * D2R;
    dlat_in = (fabs(latend - latbegin - 180) < DRV_EPSLN10) ? M_PI : (latend - latbegin) * D2R;
    lonbegin_in = (fabs(lonbegin) < DRV_EPSLN10) ? 0.0 : lonbegin * D2R;
    latbegin_in = (fabs(latbegin + 90) < DRV_EPSLN10) ? -0.5 * M_PI : latbegin * D2R;
    memset(&interp, 0, sizeof interp);
    strcpy(interp.remap_file, "remap_bilinear.nc");
    t0 = clock();
    setup_bilinear_interp(6, grid_in, 1, &grid_out, &interp, BILINEAR | (setup_only ? 0 : WRITE), dlon_in, dlat_in, lonbegin_in,
                          latbegin_in);
    {
      char p[4096];
      FILE *g;
      path(p, "setup_s.txt");
      g = fopen(p, "w");
      fprintf(g, "%.6f\n", (double)(clock() - t0) / CLOCKS_PER_SEC);
      fclose(g);
    }
  }
  dump("index.bin", interp.index, sizeof(int), 3 * (size_t)npts);
  dump("weight.bin", interp.weight, sizeof(double), 4 * (size_t)npts);
  if (setup_only) return 0;
  /* fields: Field_config as get_input_data leaves them (halo'd, one level) */
  memset(&var, 0, sizeof var);
  for (n = 0; n < 6; n++) {
    memset(&fin[n], 0, sizeof fin[n]); memset(&uin[n], 0, sizeof uin[n]); memset(&vin[n], 0, sizeof vin[n]);
    fin[n].var = uin[n].var = vin[n].var = &var;
    uin[n].data = tile_in[2][n]; vin[n].data = tile_in[3][n];
  }
  memset(&fout, 0, sizeof fout); memset(&uout, 0, sizeof uout); memset(&vout, 0, sizeof vout);
  fout.data = malloc((size_t)nlon * nlat * sizeof(double));
  uout.data = malloc((size_t)nlon * nlat * sizeof(double));
  vout.data = malloc((size_t)nlon * nlat * sizeof(double));
  var.missing = missing;
  var.has_missing = 0;
  for (n = 0; n < 6; n++) fin[n].data = tile_in[0][n];
  do_scalar_bilinear_interp(&interp, 0, 6, grid_in, &grid_out, fin, &fout, fs, 0);
  dump("s_plain.bin", fout.data, sizeof(double), (size_t)nlon * nlat);
  var.has_missing = 1;
  for (n = 0; n < 6; n++) fin[n].data = tile_in[1][n];
  do_scalar_bilinear_interp(&interp, 0, 6, grid_in, &grid_out, fin, &fout, fs, 0);
  dump("s_miss.bin", fout.data, sizeof(double), (size_t)nlon * nlat);
  do_scalar_bilinear_interp(&interp, 0, 6, grid_in, &grid_out, fin, &fout, fs, 1);
  dump("s_fill.bin", fout.data, sizeof(double), (size_t)nlon * nlat);
  var.has_missing = 0;
  do_vector_bilinear_interp(&interp, 0, 6, grid_in, 1, &grid_out, uin, vin, &uout, &vout, fs, 0);
  dump("u.bin", uout.data, sizeof(double), (size_t)nlon * nlat);
  dump("v.bin", vout.data, sizeof(double), (size_t)nlon * nlat);
  return 0;
}
