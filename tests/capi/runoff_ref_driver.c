/* runoff_ref_driver.c -- TEST HARNESS ONLY (tests/golden/make_golden_runoff.py, scripts/runoff_time.py): runs the reference's
 * nearest() (tools/runoff_regrid/runoff_regrid.c:708), create_xgrid_1dx2d_order1 and get_grid_area on one case and dumps what
 * they produce.  Linked with the reference's runoff_regrid.c (compiled with -Dmain=runoff_regrid_main and -ffunction-sections
 * and linked with --gc-sections, so that none of its netCDF-bound functions is kept), create_xgrid.c, mosaic_util.c, mpp.c and
 * mpp_domain.c, in a temporary directory outside the repository.
 *
 * What is the reference's own code here: nearest() with distance(), create_xgrid_1dx2d_order1, get_grid_area.
 * What this file RESTATES, because the reference has it between netCDF and mpp_domain calls: setup_remap's loop over the land
 * points (:511-522) and the three loops and two sums of process_data (:626-653, :666-671).  The restatement is not pinned
 * against the tool itself.
 *
 *   runoff_ref_driver IN OUTDIR
 *   IN: int mode, nx_in, ny_in, nx_out, ny_out, ntime, nq; then double
 *       xc1d_in[nx_in+1], yc1d_in[ny_in+1], mask_in[ny_in][nx_in], xc[ny_out+1][nx_out+1], yc[..], xt[ny_out][nx_out], yt[..],
 *       mask_out[..], data_in[ntime][ny_in][nx_in]; then int qindex[nq] (mode 1 only)
 *   mode 0 -> OUTDIR/imap.bin, jmap.bin [ny_out][nx_out] int; nxgrid.txt; i_in.bin, j_in.bin, i_out.bin, j_out.bin int [nxgrid],
 *             xgrid_area.bin; area_in.bin, area_out.bin; data_out.bin [ntime][ny_out][nx_out]; totals.bin [ntime][2]
 *   mode 1 -> nearest() for the nq listed points only: OUTDIR/iq.bin, jq.bin int [nq], seconds.txt (the nq calls together) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

void nearest(int nlon, int nlat, double *mask, const double *lon, const double *lat, double plon, double plat, int *iout, int *jout);
int create_xgrid_1dx2d_order1(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out, const double *lon_in,
                              const double *lat_in, const double *lon_out, const double *lat_out, const double *mask_in, int *i_in,
                              int *j_in, int *i_out, int *j_out, double *xgrid_area);
void get_grid_area(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area);
int get_maxxgrid(void);

static void rd(void *p, size_t sz, size_t n, FILE *f)
{
  if (fread(p, sz, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}
static double *rdd(size_t n, FILE *f)
{
  double *p = (double *)malloc((n ? n : 1) * sizeof(double));
  rd(p, sizeof(double), n, f);
  return p;
}
static void dump(const char *dir, const char *name, const void *p, size_t bytes)
{
  char path[4096];
  FILE *f;
  snprintf(path, sizeof path, "%s/%s", dir, name);
  f = fopen(path, "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}

int main(int argc, char **argv)
{
  int hdr[7], i, j, l, n;
  FILE *f;
  char txt[128];
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUTDIR\n", argv[0]); return 2; }
  f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  rd(hdr, sizeof(int), 7, f);
  {
    int nx_in = hdr[1], ny_in = hdr[2], nx_out = hdr[3], ny_out = hdr[4];
    const int mode = hdr[0], ntime = hdr[5], nq = hdr[6];
    const size_t n_in = (size_t)nx_in * ny_in, n_out = (size_t)nx_out * ny_out, np_out = (size_t)(nx_out + 1) * (ny_out + 1);
    double *xc1d = rdd(nx_in + 1, f), *yc1d = rdd(ny_in + 1, f), *mask_in = rdd(n_in, f);
    double *xc = rdd(np_out, f), *yc = rdd(np_out, f), *xt = rdd(n_out, f), *yt = rdd(n_out, f), *mask_out = rdd(n_out, f);
    double *data_in = rdd(n_in * ntime, f);
    if (mode == 1) {
      int *q = (int *)malloc((nq ? nq : 1) * sizeof(int)), *iq = (int *)malloc((nq ? nq : 1) * sizeof(int)), *jq = (int *)malloc((nq ? nq : 1) * sizeof(int));
      struct timespec t0, t1;
      rd(q, sizeof(int), nq, f);
      clock_gettime(CLOCK_MONOTONIC, &t0);
      for (l = 0; l < nq; l++) {
        iq[l] = jq[l] = -1;
        nearest(nx_out, ny_out, mask_out, xt, yt, xt[q[l]], yt[q[l]], &iq[l], &jq[l]);
      }
      clock_gettime(CLOCK_MONOTONIC, &t1);
      dump(argv[2], "iq.bin", iq, nq * sizeof(int));
      dump(argv[2], "jq.bin", jq, nq * sizeof(int));
      snprintf(txt, sizeof txt, "%.6f\n", (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
      dump(argv[2], "seconds.txt", txt, strlen(txt));
      fclose(f);
      return 0;
    }
    {
      const int cap = get_maxxgrid();
      int *i_in = (int *)malloc(cap * sizeof(int)), *j_in = (int *)malloc(cap * sizeof(int));
      int *i_out = (int *)malloc(cap * sizeof(int)), *j_out = (int *)malloc(cap * sizeof(int));
      double *xarea = (double *)malloc(cap * sizeof(double));
      double *xc_in = (double *)malloc((size_t)(nx_in + 1) * (ny_in + 1) * sizeof(double)), *yc_in = (double *)malloc((size_t)(nx_in + 1) * (ny_in + 1) * sizeof(double));
      double *area_in = (double *)malloc(n_in * sizeof(double)), *area_out = (double *)malloc(n_out * sizeof(double));
      int *imap = (int *)malloc(n_out * sizeof(int)), *jmap = (int *)malloc(n_out * sizeof(int));
      double *data_out = (double *)malloc(n_out * (ntime ? ntime : 1) * sizeof(double)), *totals = (double *)malloc((ntime ? ntime : 1) * 2 * sizeof(double));
      int nxgrid;
      for (j = 0; j <= ny_in; j++) for (i = 0; i <= nx_in; i++) { xc_in[j * (nx_in + 1) + i] = xc1d[i]; yc_in[j * (nx_in + 1) + i] = yc1d[j]; }
      get_grid_area(&nx_in, &ny_in, xc_in, yc_in, area_in);
      get_grid_area(&nx_out, &ny_out, xc, yc, area_out);
      nxgrid = create_xgrid_1dx2d_order1(&nx_in, &ny_in, &nx_out, &ny_out, xc1d, yc1d, xc, yc, mask_in, i_in, j_in, i_out, j_out, xarea);
      /* setup_remap's loop over the land points, serial (isc = jsc = 0) */
      for (l = 0; l < (int)n_out; l++) {
        imap[l] = jmap[l] = -1;
        if (mask_out[l] == 0) nearest(nx_out, ny_out, mask_out, xt, yt, xt[l], yt[l], &imap[l], &jmap[l]);
      }
      /* process_data's loops per time level */
      for (n = 0; n < ntime; n++) {
        const double *din = data_in + (size_t)n * n_in;
        double *dout = data_out + (size_t)n * n_out;
        double total_in = 0, total_out = 0;
        for (i = 0; i < (int)n_out; i++) dout[i] = 0;
        for (l = 0; l < nxgrid; l++) dout[j_out[l] * nx_out + i_out[l]] += din[j_in[l] * nx_in + i_in[l]] * xarea[l];
        for (j = 0; j < ny_out; j++) for (i = 0; i < nx_out; i++) {
          l = j * nx_out + i;
          if (dout[l] > 0 && mask_out[l] == 0) {
            dout[jmap[l] * nx_out + imap[l]] += dout[l];
            dout[l] = 0;
          }
        }
        for (l = 0; l < (int)n_out; l++) dout[l] /= area_out[l];
        for (i = 0; i < (int)n_in; i++) if (mask_in[i] > 0) total_in += (din[i] * area_in[i]);
        for (i = 0; i < (int)n_out; i++) total_out += (dout[i] * area_out[i]);
        totals[2 * n] = total_in; totals[2 * n + 1] = total_out;
      }
      dump(argv[2], "imap.bin", imap, n_out * sizeof(int));
      dump(argv[2], "jmap.bin", jmap, n_out * sizeof(int));
      snprintf(txt, sizeof txt, "%d\n", nxgrid);
      dump(argv[2], "nxgrid.txt", txt, strlen(txt));
      dump(argv[2], "i_in.bin", i_in, nxgrid * sizeof(int));
      dump(argv[2], "j_in.bin", j_in, nxgrid * sizeof(int));
      dump(argv[2], "i_out.bin", i_out, nxgrid * sizeof(int));
      dump(argv[2], "j_out.bin", j_out, nxgrid * sizeof(int));
      dump(argv[2], "xgrid_area.bin", xarea, nxgrid * sizeof(double));
      dump(argv[2], "area_in.bin", area_in, n_in * sizeof(double));
      dump(argv[2], "area_out.bin", area_out, n_out * sizeof(double));
      dump(argv[2], "data_out.bin", data_out, n_out * ntime * sizeof(double));
      dump(argv[2], "totals.bin", totals, (size_t)ntime * 2 * sizeof(double));
    }
  }
  fclose(f);
  return 0;
}
