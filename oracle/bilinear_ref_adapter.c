/* oracle/bilinear_ref_adapter.c -- TEST INFRASTRUCTURE ONLY, linked into oracle/_ref/libbilinear_ref.so.
 *
 * Flat-array entry points over the reference's own setup_bilinear_interp, do_scalar_bilinear_interp and
 * do_vector_bilinear_interp (its tools/fregrid/bilinear_interp.c, compiled in place by oracle/Makefile), so tests/orc.py can
 * drive them through ctypes.  The Grid_config structs are filled as tests/capi/bilinear_ref_driver.c fills them: the BILINEAR
 * branches of get_input_grid (fregrid_util.c:300-312) and get_output_grid_by_size (:564-641), then fregrid.c:944-963's span
 * arguments with the EPSLN10 snapping.  The halo'd centres [6][N+2][N+2] come from the caller.
 *
 * Only the compute branch of setup runs: the opcode is BILINEAR alone (the remap-file I/O of READ / WRITE is stubbed in
 * oracle/conserve_ref_io_stubs.c).  When the reference's ten sweeps leave a point unfound it prints a warning and starts its
 * "global sweep", which reads past its arrays: a caller that may reach it runs bref_setup in a child process with
 * bref_init(1), so each printed line reaches the parent before the sweep starts. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "globals.h"
#include "mosaic_util.h"
#include "bilinear_interp.h"
#include "mpp.h"

#define BREF_EPSLN10 (1.e-10)      /* fregrid.c's EPSLN10 */

int max_weight_index(double *var, int nvar);
double normalize_great_circle_distance(const double *v1, const double *v2);
void do_latlon_coarsening(const double *var_latlon, const double *ylat, int nlon, int nlat, int nz, double *var_latlon_crs,
                          int finer_steps, int has_missing, double missvalue);

static int bref_ready = 0;

void bref_init(int line_buffered)
{
  if (line_buffered) setvbuf(stdout, NULL, _IOLBF, BUFSIZ);
  if (bref_ready) return;
  mpp_init(NULL, NULL);
  bref_ready = 1;
}

typedef struct {
  Grid_config in[6], out;
  double dlon_in, dlat_in, lonbegin_in, latbegin_in;
} Grids;

/* get_input_grid's and get_output_grid_by_size's BILINEAR branches, and fregrid.c:944-963 */
static void grids_fill(Grids *g, int N, const double *lont_h, const double *latt_h, int nlon, int nlat, int fs, int center_y,
                       double lonbegin, double lonend, double latbegin, double latend)
{
  const int F = (N + 2) * (N + 2);
  int n, i, j, nxf, nyf, npts;
  double dlon, dlat;
  memset(g, 0, sizeof *g);
  for (n = 0; n < 6; n++) {
    Grid_config *t = &g->in[n];
    t->nx = N; t->ny = N;
    t->lont = (double *)lont_h + (size_t)n * F; t->latt = (double *)latt_h + (size_t)n * F;
    t->vlon_t = malloc(3 * F * sizeof(double)); t->vlat_t = malloc(3 * F * sizeof(double));
    t->xt = malloc(F * sizeof(double)); t->yt = malloc(F * sizeof(double)); t->zt = malloc(F * sizeof(double));
    latlon2xyz(F, t->lont, t->latt, t->xt, t->yt, t->zt);
    unit_vect_latlon(F, t->lont, t->latt, t->vlon_t, t->vlat_t);
  }
  g->out.nx = nlon; g->out.ny = nlat;
  g->out.nx_fine = nxf = pow(2, fs) * nlon;
  g->out.ny_fine = nyf = pow(2, fs) * (nlat - 1) + 1;
  npts = nxf * nyf;
  g->out.latt1D_fine = malloc(nyf * sizeof(double));
  g->out.lont = malloc(npts * sizeof(double)); g->out.latt = malloc(npts * sizeof(double));
  g->out.xt = malloc(npts * sizeof(double)); g->out.yt = malloc(npts * sizeof(double)); g->out.zt = malloc(npts * sizeof(double));
  g->out.vlon_t = malloc(3 * npts * sizeof(double)); g->out.vlat_t = malloc(3 * npts * sizeof(double));
  dlon = (lonend - lonbegin) / nxf;
  for (i = 0; i < nxf; i++) {
    double lon_fine = (lonbegin + (i + 0.5) * dlon) * D2R;
    for (j = 0; j < nyf; j++) g->out.lont[j * nxf + i] = lon_fine;
  }
  if (center_y) {
    dlat = (latend - latbegin) / nyf;
    for (j = 0; j < nyf; j++) g->out.latt1D_fine[j] = (latbegin + (j + 0.5) * dlat) * D2R;
  } else {
    dlat = (latend - latbegin) / (nyf - 1);
    for (j = 0; j < nyf; j++) g->out.latt1D_fine[j] = (latbegin + j * dlat) * D2R;
  }
  for (j = 0; j < nyf; j++) for (i = 0; i < nxf; i++) g->out.latt[j * nxf + i] = g->out.latt1D_fine[j];
  latlon2xyz(npts, g->out.lont, g->out.latt, g->out.xt, g->out.yt, g->out.zt);
  unit_vect_latlon(npts, g->out.lont, g->out.latt, g->out.vlon_t, g->out.vlat_t);
  g->dlon_in = (fabs(lonend - lonbegin - 360) < BREF_EPSLN10) ? M_PI + M_PI : (lonend - lonbegin) * D2R;
  g->dlat_in = (fabs(latend - latbegin - 180) < BREF_EPSLN10) ? M_PI : (latend - latbegin) * D2R;
  g->lonbegin_in = (fabs(lonbegin) < BREF_EPSLN10) ? 0.0 : lonbegin * D2R;
  g->latbegin_in = (fabs(latbegin + 90) < BREF_EPSLN10) ? -0.5 * M_PI : latbegin * D2R;
}

static void grids_free(Grids *g)
{
  int n;
  for (n = 0; n < 6; n++) {
    free(g->in[n].vlon_t); free(g->in[n].vlat_t); free(g->in[n].xt); free(g->in[n].yt); free(g->in[n].zt);
  }
  free(g->out.latt1D_fine); free(g->out.lont); free(g->out.latt); free(g->out.xt); free(g->out.yt); free(g->out.zt);
  free(g->out.vlon_t); free(g->out.vlat_t);
}

static void cpy(double *dst, const double *src, size_t n) { if (dst) memcpy(dst, src, n * sizeof(double)); }

/* setup_bilinear_interp's compute branch.  lont_h / latt_h: [6][N+2][N+2] radians.  Outputs (fine grid, npts = nx_fine *
 * ny_fine): index [npts][3], weight [npts][4]; the fine grid as the reference's caller built it, each may be NULL: lont, latt
 * [npts], latt1d [ny_fine], xyz [3][npts] (xt | yt | zt), vlon / vlat [npts][3]. */
int bref_setup(int N, const double *lont_h, const double *latt_h, int nlon, int nlat, int finer_step, int center_y, double lonbegin,
               double lonend, double latbegin, double latend, int *index, double *weight, double *lont, double *latt, double *latt1d,
               double *xyz, double *vlon, double *vlat)
{
  Grids g;
  Interp_config interp;
  long npts;
  bref_init(0);
  grids_fill(&g, N, lont_h, latt_h, nlon, nlat, finer_step, center_y, lonbegin, lonend, latbegin, latend);
  npts = (long)g.out.nx_fine * g.out.ny_fine;
  memset(&interp, 0, sizeof interp);
  setup_bilinear_interp(6, g.in, 1, &g.out, &interp, BILINEAR, g.dlon_in, g.dlat_in, g.lonbegin_in, g.latbegin_in);
  fflush(stdout);
  memcpy(index, interp.index, 3 * npts * sizeof(int));
  memcpy(weight, interp.weight, 4 * npts * sizeof(double));
  cpy(lont, g.out.lont, npts); cpy(latt, g.out.latt, npts); cpy(latt1d, g.out.latt1D_fine, g.out.ny_fine);
  if (xyz) { cpy(xyz, g.out.xt, npts); cpy(xyz + npts, g.out.yt, npts); cpy(xyz + 2 * npts, g.out.zt, npts); }
  cpy(vlon, g.out.vlon_t, 3 * npts); cpy(vlat, g.out.vlat_t, 3 * npts);
  free(interp.index); free(interp.weight);
  grids_free(&g);
  return 0;
}

/* one level through do_scalar_bilinear_interp (vector == 0: a = data [6][N+2][N+2] halo'd, out_a [nlat][nlon]) or
 * do_vector_bilinear_interp (a, b = u, v halo'd -> out_a, out_b), with the plan's index / weight.  The Grid_config members the
 * two read are passed in as bref_setup returned them: latt1d, and for vectors vlon_out / vlat_out [npts][3] of the fine grid and
 * vlon_in / vlat_in [6][N+2][N+2][3] (bref_unit_vect_latlon of the halo'd centres). */
static int bref_apply(int vector, int N, int nlon, int nlat, int finer_step, const int *index, const double *weight,
                      const double *latt1d, const double *vlon_in, const double *vlat_in, const double *vlon_out,
                      const double *vlat_out, const double *a, const double *b, int has_missing, double missing, int fill_missing,
                      double *out_a, double *out_b)
{
  const int F = (N + 2) * (N + 2);
  Grid_config gin[6], gout;
  Interp_config interp;
  Var_config var;
  Field_config fa[6], fb[6], oa, ob;
  int n;
  bref_init(0);
  memset(gin, 0, sizeof gin);
  memset(&gout, 0, sizeof gout);
  for (n = 0; n < 6; n++) {
    gin[n].nx = N; gin[n].ny = N;
    if (vector) { gin[n].vlon_t = (double *)vlon_in + 3 * (size_t)n * F; gin[n].vlat_t = (double *)vlat_in + 3 * (size_t)n * F; }
  }
  gout.nx = nlon; gout.ny = nlat;
  gout.nx_fine = pow(2, finer_step) * nlon;
  gout.ny_fine = pow(2, finer_step) * (nlat - 1) + 1;
  gout.latt1D_fine = (double *)latt1d;
  gout.vlon_t = (double *)vlon_out; gout.vlat_t = (double *)vlat_out;
  memset(&interp, 0, sizeof interp);
  interp.index = (int *)index;
  interp.weight = (double *)weight;
  memset(&var, 0, sizeof var);
  var.has_missing = has_missing;
  var.missing = missing;
  for (n = 0; n < 6; n++) {
    memset(&fa[n], 0, sizeof fa[n]); memset(&fb[n], 0, sizeof fb[n]);
    fa[n].var = fb[n].var = &var;
    fa[n].data = (double *)a + (size_t)n * F;
    if (b) fb[n].data = (double *)b + (size_t)n * F;
  }
  memset(&oa, 0, sizeof oa); memset(&ob, 0, sizeof ob);
  oa.data = out_a; ob.data = out_b;
  if (vector) do_vector_bilinear_interp(&interp, 0, 6, gin, 1, &gout, fa, fb, &oa, &ob, finer_step, fill_missing);
  else do_scalar_bilinear_interp(&interp, 0, 6, gin, &gout, fa, &oa, finer_step, fill_missing);
  fflush(stdout);
  return 0;
}

int bref_apply_scalar(int N, int nlon, int nlat, int finer_step, const int *index, const double *weight, const double *latt1d,
                      const double *data, int has_missing, double missing, int fill_missing, double *out)
{
  return bref_apply(0, N, nlon, nlat, finer_step, index, weight, latt1d, NULL, NULL, NULL, NULL, data, NULL, has_missing, missing,
                    fill_missing, out, NULL);
}

int bref_apply_vector(int N, int nlon, int nlat, int finer_step, const int *index, const double *weight, const double *latt1d,
                      const double *vlon_in, const double *vlat_in, const double *vlon_out, const double *vlat_out, const double *u,
                      const double *v, int has_missing, double missing, int fill_missing, double *u_out, double *v_out)
{
  return bref_apply(1, N, nlon, nlat, finer_step, index, weight, latt1d, vlon_in, vlat_in, vlon_out, vlat_out, u, v, has_missing,
                    missing, fill_missing, u_out, v_out);
}

/* the reference's unit_vect_latlon (mosaic_util.c), vlon / vlat [size][3] */
void bref_unit_vect_latlon(int size, const double *lon, const double *lat, double *vlon, double *vlat)
{
  unit_vect_latlon(size, lon, lat, vlon, vlat);
}

/* the window distance of setup_bilinear_interp (:145-153, iter 1) for every cell (c = l*N*N + (jc-1)*N + ic-1):
 * normalize_great_circle_distance of the centres (jc, ic) and (jc+1, ic+1), on the reference's latlon2xyz of the halo'd centres */
void bref_cell_dist(int N, const double *lont_h, const double *latt_h, double *dist)
{
  const int nxd = N + 2, F = nxd * nxd;
  double *x = malloc(3 * (size_t)F * sizeof(double));
  int l, ic, jc;
  for (l = 0; l < 6; l++) {
    latlon2xyz(F, lont_h + (size_t)l * F, latt_h + (size_t)l * F, x, x + F, x + 2 * F);
    for (jc = 1; jc <= N; jc++) for (ic = 1; ic <= N; ic++) {
      const int n1 = jc * nxd + ic, n2 = (jc + 1) * nxd + ic + 1;
      const double v1[3] = {x[n1], x[F + n1], x[2 * F + n1]}, v2[3] = {x[n2], x[F + n2], x[2 * F + n2]};
      dist[(size_t)l * N * N + (size_t)(jc - 1) * N + ic - 1] = normalize_great_circle_distance(v1, v2);
    }
  }
  free(x);
}

/* max_weight_index on n rows of four weights */
void bref_max_weight_index(long n, const double *weight, int *ind)
{
  long k;
  for (k = 0; k < n; k++) ind[k] = max_weight_index((double *)weight + 4 * k, 4);
}
