/* topog_ref_driver.c -- TEST HARNESS ONLY (tests/golden/make_golden_topog.py, tests/test_topog_cpu.py, scripts/topog_time.py):
 * runs the reference's conserve_interp / conserve_interp_great_circle (tools/libfrencutils/interp.c), filter_topo, show_deepest
 * and process_topo (tools/make_topog/topog.c) on one case and dumps every intermediate.  Compiled in a temporary directory
 * outside the repository and linked with the reference's topog.c, interp.c, create_xgrid.c, mosaic_util.c, mpp.c and
 * mpp_domain.c (function sections, --gc-sections: create_realistic_topog itself and everything bound to netCDF is dropped).
 *
 * What is the reference's own code here: everything that computes.  What this file restates is what sits between netCDF calls in
 * create_realistic_topog (:416-511): the axis bounds, the row trim, the widening of the field, the mask and the on_grid copy,
 * in the same order of operations.
 *
 *   topog_ref_driver IN OUTDIR
 *   IN: int hdr[28] = mode, nx_dst, ny_dst, nx_src, ny_src, dtype (4 int32, 5 float32, 6 float64), nk, tripolar_grid, cyclic_x,
 *       cyclic_y, fill_first_row, filter_topog, num_filter_pass, smooth_topo_allow_deepening, round_shallow, fill_shallow,
 *       deepen_shallow, full_cell, flat_bottom, adjust_topo, fill_isolated_cells, dont_change_landmask, kmt_min,
 *       open_very_this_cell, use_great_circle_algorithm, on_grid, 0, 0;
 *       double par[4] = scale_factor, min_thickness, fraction_full_cell, missing; double zw[nk];
 *       mode 0 (the whole chain): double x_dst, y_dst [(ny_dst+1)*(nx_dst+1)] degrees, xt_src[nx_src], yt_src[ny_src], then the
 *       field [ny_src*nx_src] in its type;  mode 1 (stages from a given depth): double depth[ny_dst*nx_dst]
 *   OUTDIR: mode 0: trim.txt (jstart jend), x_src.bin, y_src.bin, depth_src.bin, mask_src.bin, depth_remap.bin; both modes:
 *       depth_filter.bin (after filter_topo, or the depth as it was when filter_topog is 0), depth_final.bin, num_levels.bin (nk > 0),
 *       seconds.txt (remap, filter, process).  The reference's debug notes go to stdout, as in the tool. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "constant.h"
#include "mosaic_util.h"
#include "interp.h"
#include "mpp.h"
#include "mpp_domain.h"

void filter_topo(int nx, int ny, int num_pass, int smooth_topo_allow_deepening, double *depth, domain2D domain);
void show_deepest(int nk, const double *zw, const double *depth, domain2D domain);
void process_topo(int nk, double *depth, int *num_levels, const double *zw, int tripolar_grid, int cyclic_x, int cyclic_y, int full_cell,
                  int flat_bottom, int adjust_topo, int fill_isolated_cells, double min_thickness, int open_very_this_cell,
                  double fraction_full_cell, int round_shallow, int deepen_shallow, int fill_shallow, int dont_change_landmask, int kmt_min,
                  domain2D domain, int debug);

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
static void dump(const char *dir, const char *name, const void *p, size_t sz, size_t n)
{
  char path[4096];
  FILE *f;
  snprintf(path, sizeof path, "%s/%s", dir, name);
  f = fopen(path, "wb");
  if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fwrite(p, sz, n, f);
  fclose(f);
}
/* xc [n+1]: midpoints of the centres xt [n], the two ends mirrored about the end centres, then degrees to radians */
static void bounds_rad(int n, const double *xt, double *xc)
{
  int i;
  for (i = 1; i < n; i++) xc[i] = (xt[i - 1] + xt[i]) * 0.5;
  xc[0] = 2 * xt[0] - xc[1];
  xc[n] = 2 * xt[n - 1] - xc[n - 1];
  for (i = 0; i <= n; i++) xc[i] = xc[i] * D2R;
}
static double now(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec + 1e-9 * t.tv_nsec;
}

int main(int argc, char **argv)
{
  int hdr[28], i, j, layout[2] = {1, 1};
  double par[4], *zw, *depth, sec[3] = {0, 0, 0}, t0;
  int *num_levels;
  FILE *f;
  domain2D domain;
  char txt[256];
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUTDIR\n", argv[0]); return 2; }
  mpp_init(&argc, &argv);
  mpp_domain_init();
  f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  rd(hdr, sizeof(int), 28, f);
  rd(par, sizeof(double), 4, f);
  {
    const int mode = hdr[0], nx_dst = hdr[1], ny_dst = hdr[2], nx_src = hdr[3], ny_src = hdr[4], dtype = hdr[5], nk = hdr[6];
    const int tripolar_grid = hdr[7], cyclic_x = hdr[8], cyclic_y = hdr[9], fill_first_row = hdr[10], filter_topog = hdr[11];
    const int num_filter_pass = hdr[12], smooth_topo_allow_deepening = hdr[13], round_shallow = hdr[14], fill_shallow = hdr[15];
    const int deepen_shallow = hdr[16], full_cell = hdr[17], flat_bottom = hdr[18], adjust_topo = hdr[19], fill_isolated_cells = hdr[20];
    const int dont_change_landmask = hdr[21], kmt_min = hdr[22], open_very_this_cell = hdr[23], use_great_circle_algorithm = hdr[24];
    const int on_grid = hdr[25];
    const double scale_factor = par[0], min_thickness = par[1], fraction_full_cell = par[2], missing = par[3];
    const size_t nd = (size_t)nx_dst * ny_dst;
    zw = rdd(nk, f);
    num_levels = (int *)malloc((nd ? nd : 1) * sizeof(int));
    mpp_define_domain2d(nx_dst, ny_dst, layout, 0, 0, &domain);
    if (mode == 1) depth = rdd(nd, f);
    else {
      const size_t npd = (size_t)(nx_dst + 1) * (ny_dst + 1);
      const int nxp_src = nx_src + 1, nyp_src = ny_src + 1;
      double *x_dst = rdd(npd, f), *y_dst = rdd(npd, f), *xt_src = rdd(nx_src, f), *yt_src = rdd(ny_src, f);
      double *xc_src = (double *)malloc(nxp_src * sizeof(double)), *yc_src = (double *)malloc(nyp_src * sizeof(double));
      double *x_out = (double *)malloc(npd * sizeof(double)), *y_out = (double *)malloc(npd * sizeof(double));
      double *x_src, *y_src, *depth_src, *mask_src, y_min, y_max;
      int jstart, jend, ny_now;
      size_t n, ns;
      depth = (double *)malloc((nd ? nd : 1) * sizeof(double));
      /* the cell bounds of both axes, in radians (:416-427) */
      bounds_rad(nx_src, xt_src, xc_src);
      bounds_rad(ny_src, yt_src, yc_src);
      /* the model grid in radians and the source rows its latitudes reach, one more at each end (:431-449) */
      for (n = 0; n < npd; n++) { x_out[n] = x_dst[n] * D2R; y_out[n] = y_dst[n] * D2R; }
      y_min = minval_double((int)npd, y_out);
      y_max = maxval_double((int)npd, y_out);
      jstart = ny_src; jend = -1;
      for (j = 0; j <= ny_src; j++)
        if (yc_src[j] > y_min && yc_src[j] < y_max) { if (j > jend) jend = j; if (j < jstart) jstart = j; }
      jstart = jstart - 1 < 0 ? 0 : jstart - 1;
      jend = jend + 1 > ny_src - 1 ? ny_src - 1 : jend + 1;
      ny_now = jend - jstart + 1;
      ns = (size_t)nx_src * ny_now;
      snprintf(txt, sizeof txt, "%d %d\n", jstart, jend);
      dump(argv[2], "trim.txt", txt, 1, strlen(txt));
      /* the corner arrays conserve_interp takes (:451-460) */
      x_src = (double *)malloc((size_t)nxp_src * (ny_now + 1) * sizeof(double));
      y_src = (double *)malloc((size_t)nxp_src * (ny_now + 1) * sizeof(double));
      depth_src = (double *)malloc(ns * sizeof(double));
      mask_src = (double *)malloc(ns * sizeof(double));
      for (j = 0; j <= ny_now; j++) for (i = 0; i < nxp_src; i++) {
        x_src[j * nxp_src + i] = xc_src[i];
        y_src[j * nxp_src + i] = yc_src[j + jstart];
      }
      /* the rows jstart .. jend as doubles (:471-488); netCDF widens NC_FLOAT and NC_INT the way the casts do */
      {
        const size_t esz = dtype == 6 ? 8 : 4;
        void *raw = malloc((size_t)nx_src * ny_src * esz);
        rd(raw, esz, (size_t)nx_src * ny_src, f);
        for (n = 0; n < ns; n++) {
          const size_t q = (size_t)jstart * nx_src + n;
          depth_src[n] = dtype == 6 ? ((double *)raw)[q] : dtype == 5 ? (double)((float *)raw)[q] : (double)((int *)raw)[q];
        }
        free(raw);
      }
      /* mask and scale (:492-502): missing is tested first, then the scaled value against 0 */
      for (n = 0; n < ns; n++) {
        mask_src[n] = 0.0;
        if (depth_src[n] != missing) {
          depth_src[n] = depth_src[n] * scale_factor;
          if (depth_src[n] > 0.0) mask_src[n] = 1.0;
        }
      }
      t0 = now();
      if (on_grid) {
        if (ns != nd) { fprintf(stderr, "on_grid: %zu source cells for %zu model cells\n", ns, nd); return 2; }
        for (n = 0; n < ns; n++) depth[n] = depth_src[n] == missing ? 0.0 : depth_src[n];     /* :505-510, on the scaled values */
      } else if (use_great_circle_algorithm)
        conserve_interp_great_circle(nx_src, ny_now, nx_dst, ny_dst, x_src, y_src, x_out, y_out, mask_src, depth_src, depth);
      else
        conserve_interp(nx_src, ny_now, nx_dst, ny_dst, x_src, y_src, x_out, y_out, mask_src, depth_src, depth);
      sec[0] = now() - t0;
      dump(argv[2], "x_src.bin", x_src, sizeof(double), (size_t)nxp_src * (ny_now + 1));
      dump(argv[2], "y_src.bin", y_src, sizeof(double), (size_t)nxp_src * (ny_now + 1));
      dump(argv[2], "depth_src.bin", depth_src, sizeof(double), ns);
      dump(argv[2], "mask_src.bin", mask_src, sizeof(double), ns);
      dump(argv[2], "depth_remap.bin", depth, sizeof(double), nd);
    }
    fclose(f);
    /* :522-536 */
    t0 = now();
    if (filter_topog) filter_topo(nx_dst, ny_dst, num_filter_pass, smooth_topo_allow_deepening, depth, domain);
    sec[1] = now() - t0;
    dump(argv[2], "depth_filter.bin", depth, sizeof(double), nd);
    if (nk > 0) show_deepest(nk, zw, depth, domain);
    if (fill_first_row) for (i = 0; i < nx_dst; i++) depth[i] = 0.0;
    t0 = now();
    if (nk > 0) process_topo(nk, depth, num_levels, zw, tripolar_grid, cyclic_x, cyclic_y,
                             full_cell, flat_bottom, adjust_topo, fill_isolated_cells, min_thickness,
                             open_very_this_cell, fraction_full_cell, round_shallow, deepen_shallow, fill_shallow,
                             dont_change_landmask, kmt_min, domain, 1);
    sec[2] = now() - t0;
    dump(argv[2], "depth_final.bin", depth, sizeof(double), nd);
    if (nk > 0) dump(argv[2], "num_levels.bin", num_levels, sizeof(int), nd);
    snprintf(txt, sizeof txt, "%.6f %.6f %.6f\n", sec[0], sec[1], sec[2]);
    dump(argv[2], "seconds.txt", txt, 1, strlen(txt));
  }
  return 0;
}
