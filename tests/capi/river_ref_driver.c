/* river_ref_driver.c -- TEST HARNESS ONLY (tests/golden/make_golden_river.py, tests/test_river_cpu.py, scripts/river_time.py):
 * runs the reference's init_river_data, calc_max_subA, calc_tocell, calc_river_data, sort_basin and check_river_data
 * (tools/river_regrid/river_regrid.c) on one case and dumps what they produce.  river_type is declared inside river_regrid.c,
 * so that file is included here (RIVER_C is its path, given on the command line of the compiler) with its main renamed; built
 * with -ffunction-sections and linked with --gc-sections against the reference's create_xgrid.c, mosaic_util.c, mpp.c and
 * mpp_domain.c in a temporary directory outside the repository, so that none of its netCDF-bound functions is kept.
 *
 * What is the reference's own code here: everything that computes.  What this file does in place of get_source_data and
 * get_mosaic_grid, which sit between netCDF calls: it fills river_in and river_out[] from the input file, calls get_grid_area or
 * get_grid_great_circle_area and update_halo_double for xt and yt as get_mosaic_grid does (:489-494, :631-632).
 *
 *   river_ref_driver IN OUTDIR
 *   IN: int nx_in, ny_in, ntiles, nx, ny, opcode, gca; double suba_cutoff, missing[6] (subA, tocell, travel, basin, cellarea,
 *       celllength); double xb_r[nx_in+1], yb_r[ny_in+1], subA[ny_in][nx_in]; then per tile double xb_r[(ny+1)*(nx+1)], yb_r[..],
 *       xt[(ny+2)*(nx+2)], yt[..] (degrees, the halo as the caller left it), landfrac[ny*nx]
 *   OUTDIR, tiles one after another: area.bin, xt.bin, yt.bin (after the halo update), max_suba.bin (haloed, before calc_tocell),
 *       subA.bin, cellarea.bin, celllength.bin (interior double), tocell.bin, travel.bin, basin.bin, basin_presort.bin,
 *       last_point.bin (interior int), seconds.txt (calc_max_subA, calc_tocell, calc_river_data, sort_basin, check_river_data).
 *   check_river_data's notes go to stdout, as in the tool. */
#include <time.h>
#define main river_regrid_main
#include RIVER_C
#undef main

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
static FILE *out_open(const char *dir, const char *name)
{
  char path[4096];
  FILE *f;
  snprintf(path, sizeof path, "%s/%s", dir, name);
  f = fopen(path, "wb");
  if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  return f;
}
static double now(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec + 1e-9 * t.tv_nsec;
}

int main(int argc, char **argv)
{
  int hdr[7], n, i, j;
  double par[7], t[6];
  FILE *f;
  river_type river_in, *river_out;
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUTDIR\n", argv[0]); return 2; }
  f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  rd(hdr, sizeof(int), 7, f);
  rd(par, sizeof(double), 7, f);
  {
    int nx_in = hdr[0], ny_in = hdr[1], ntiles = hdr[2], nx = hdr[3], ny = hdr[4];
    unsigned int opcode = (unsigned int)hdr[5];
    const int gca = hdr[6];
    const size_t per = (size_t)nx * ny, perh = (size_t)(nx + 2) * (ny + 2), perb = (size_t)(nx + 1) * (ny + 1);
    double **pxt, **pyt;
    int **presort;
    suba_cutoff = par[0];
    river_in.nx = nx_in; river_in.ny = ny_in;
    river_in.subA_missing = par[1];
    river_in.tocell_missing = par[2];
    river_in.travel_missing = par[3];
    river_in.basin_missing = par[4];
    river_in.cellarea_missing = par[5];
    river_in.celllength_missing = par[6];
    river_in.xb_r = rdd(nx_in + 1, f);
    river_in.yb_r = rdd(ny_in + 1, f);
    river_in.subA = rdd((size_t)nx_in * ny_in, f);
    river_out = (river_type *)malloc(ntiles * sizeof(river_type));
    pxt = (double **)malloc(ntiles * sizeof(double *));
    pyt = (double **)malloc(ntiles * sizeof(double *));
    presort = (int **)malloc(ntiles * sizeof(int *));
    for (n = 0; n < ntiles; n++) {
      river_out[n].nx = nx; river_out[n].ny = ny;
      river_out[n].xb_r = rdd(perb, f);
      river_out[n].yb_r = rdd(perb, f);
      river_out[n].xt = pxt[n] = rdd(perh, f);
      river_out[n].yt = pyt[n] = rdd(perh, f);
      river_out[n].landfrac = rdd(per, f);
      river_out[n].area = (double *)malloc(per * sizeof(double));
      if (gca) get_grid_great_circle_area(&nx, &ny, river_out[n].xb_r, river_out[n].yb_r, river_out[n].area);
      else get_grid_area(&nx, &ny, river_out[n].xb_r, river_out[n].yb_r, river_out[n].area);
    }
    fclose(f);
    update_halo_double(ntiles, pxt, nx, ny, opcode);
    update_halo_double(ntiles, pyt, nx, ny, opcode);
    init_river_data(ntiles, river_out, &river_in);
    t[0] = now();
    calc_max_subA(&river_in, river_out, ntiles, opcode);
    t[1] = now();
    f = out_open(argv[2], "max_suba.bin");
    for (n = 0; n < ntiles; n++) fwrite(river_out[n].subA, sizeof(double), perh, f);
    fclose(f);
    {
      const double t1 = now();
      calc_tocell(ntiles, river_out, opcode);
      t[2] = now();
      calc_river_data(ntiles, river_out, opcode);
      t[3] = now();
      for (n = 0; n < ntiles; n++) {
        presort[n] = (int *)malloc(per * sizeof(int));
        for (j = 0; j < ny; j++) for (i = 0; i < nx; i++) presort[n][j * nx + i] = river_out[n].basin[(j + 1) * (nx + 2) + i + 1];
      }
      t[4] = now();
      sort_basin(ntiles, river_out);
      t[5] = now();
      check_river_data(ntiles, river_out);
      {
        const double t6 = now();
        char txt[256];
        snprintf(txt, sizeof txt, "%.6f %.6f %.6f %.6f %.6f\n", t[1] - t[0], t[2] - t1, t[3] - t[2], t[5] - t[4], t6 - t[5]);
        f = out_open(argv[2], "seconds.txt");
        fwrite(txt, 1, strlen(txt), f);
        fclose(f);
      }
    }
    {
      const char *dnames[] = {"area.bin", "cellarea.bin", "celllength.bin"};
      for (i = 0; i < 3; i++) {
        f = out_open(argv[2], dnames[i]);
        for (n = 0; n < ntiles; n++) fwrite(i == 0 ? river_out[n].area : i == 1 ? river_out[n].cellarea : river_out[n].celllength, sizeof(double), per, f);
        fclose(f);
      }
      f = out_open(argv[2], "xt.bin");
      for (n = 0; n < ntiles; n++) fwrite(river_out[n].xt, sizeof(double), perh, f);
      fclose(f);
      f = out_open(argv[2], "yt.bin");
      for (n = 0; n < ntiles; n++) fwrite(river_out[n].yt, sizeof(double), perh, f);
      fclose(f);
      f = out_open(argv[2], "subA.bin");
      for (n = 0; n < ntiles; n++) for (j = 1; j <= ny; j++) fwrite(river_out[n].subA + j * (nx + 2) + 1, sizeof(double), nx, f);
      fclose(f);
      {
        const char *inames[] = {"tocell.bin", "travel.bin", "basin.bin"};
        for (i = 0; i < 3; i++) {
          f = out_open(argv[2], inames[i]);
          for (n = 0; n < ntiles; n++) for (j = 1; j <= ny; j++)
            fwrite((i == 0 ? river_out[n].tocell : i == 1 ? river_out[n].travel : river_out[n].basin) + j * (nx + 2) + 1, sizeof(int), nx, f);
          fclose(f);
        }
      }
      f = out_open(argv[2], "basin_presort.bin");
      for (n = 0; n < ntiles; n++) fwrite(presort[n], sizeof(int), per, f);
      fclose(f);
      f = out_open(argv[2], "last_point.bin");
      for (n = 0; n < ntiles; n++) fwrite(river_out[n].last_point, sizeof(int), per, f);
      fclose(f);
    }
  }
  return 0;
}
