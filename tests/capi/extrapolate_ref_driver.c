/* extrapolate_ref_driver.c -- TEST HARNESS ONLY (tests/golden/make_golden_extrapolate.py, tests/test_extrapolate_cpu.py): runs the
 * reference's do_extrapolate (tools/fregrid/fregrid_util.c:2662) or setup_vertical_interp + do_vertical_interp (:756-819) on one
 * case and dumps what they produce.  Linked with the reference's fregrid_util.c (compiled with -ffunction-sections and linked
 * with --gc-sections, so that none of its netCDF-bound functions is kept), mpp.c and, for the vertical case, interp.c and
 * mosaic_util.c, in a temporary directory outside the repository.
 *
 *   extrapolate_ref_driver IN OUTDIR
 *   IN (mode 0): int 0, ni, nj, nk, is_cyclic; double missing, stop_crit; double lon[ni], lat[nj], data[nk][nj][ni]
 *      -> OUTDIR/out.bin [nk][nj][ni], OUTDIR/seconds.txt; the reference's "Stopped after %d iterations, maxres = %g" on stdout
 *   IN (mode 1): int 1, nxy, nk1, nk2, 0; double 0, 0; double z1[nk1], z2[nk2], data[nk1][nxy]
 *      -> OUTDIR/out.bin [nk1 or nk2][nxy], OUTDIR/kinfo.txt "kstart kend need_interp" */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "globals.h"
#include "mpp.h"
#include "fregrid_util.h"

void do_extrapolate(int ni, int nj, int nk, const double *lon, const double *lat, const double *data_in,
                    double *data_out, int is_cyclic, double missing_value, double stop_crit);

static void rd(void *p, size_t sz, size_t n, FILE *f)
{
  if (fread(p, sz, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
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
  int hdr[5];
  double par[2];
  FILE *f;
  char txt[128];
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUTDIR\n", argv[0]); return 2; }
  mpp_init(&argc, &argv);
  f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  rd(hdr, sizeof(int), 5, f);
  rd(par, sizeof(double), 2, f);
  if (hdr[0] == 0) {
    const int ni = hdr[1], nj = hdr[2], nk = hdr[3];
    const size_t n = (size_t)ni * nj * nk;
    double *lon = (double *)malloc(ni * sizeof(double)), *lat = (double *)malloc(nj * sizeof(double));
    double *in = (double *)malloc(n * sizeof(double)), *out = (double *)calloc(n, sizeof(double));
    struct timespec t0, t1;
    rd(lon, sizeof(double), ni, f); rd(lat, sizeof(double), nj, f); rd(in, sizeof(double), n, f);
    clock_gettime(CLOCK_MONOTONIC, &t0);
    do_extrapolate(ni, nj, nk, lon, lat, in, out, hdr[4], par[0], par[1]);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    fflush(stdout);
    dump(argv[2], "out.bin", out, n * sizeof(double));
    snprintf(txt, sizeof txt, "%.6f\n", (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
    dump(argv[2], "seconds.txt", txt, strlen(txt));
  } else {
    const int nxy = hdr[1], nk1 = hdr[2], nk2 = hdr[3];
    VGrid_config vin, vout;
    Grid_config grid;
    Field_config field;
    Var_config var;
    memset(&vin, 0, sizeof vin); memset(&vout, 0, sizeof vout); memset(&grid, 0, sizeof grid);
    memset(&field, 0, sizeof field); memset(&var, 0, sizeof var);
    vin.nz = nk1; vin.z = (double *)malloc(nk1 * sizeof(double));
    vout.nz = nk2; vout.z = (double *)malloc(nk2 * sizeof(double));
    field.data = (double *)malloc((size_t)nxy * nk1 * sizeof(double));
    rd(vin.z, sizeof(double), nk1, f); rd(vout.z, sizeof(double), nk2, f); rd(field.data, sizeof(double), (size_t)nxy * nk1, f);
    grid.nx = nxy; grid.ny = 1;                       /* do_vertical_interp only uses the product */
    var.has_zaxis = 1;
    field.var = &var;
    setup_vertical_interp(&vin, &vout);
    do_vertical_interp(&vin, &vout, &grid, &field, 0);
    fflush(stdout);
    dump(argv[2], "out.bin", field.data, (size_t)nxy * (vout.need_interp ? nk2 : nk1) * sizeof(double));
    snprintf(txt, sizeof txt, "%d %d %d\n", vout.kstart, vout.kend, vout.need_interp);
    dump(argv[2], "kinfo.txt", txt, strlen(txt));
  }
  fclose(f);
  return 0;
}
