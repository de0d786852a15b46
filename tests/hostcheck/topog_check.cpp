// topog_check.cpp -- TEST HARNESS ONLY: csrc/topog.h built for the host.  Runs the stages of make_topog's realistic topography
// through the same functions the device kernels call, cell by cell in the kernels' own order of launches, so that the arithmetic,
// the halo fill and the three orders of remove_isolated_cells are checked against the reference's fixtures without a device
// (and under host sanitizers).
//   topog_check IN OUT      IN: topog_ref_driver's input file
//   OUT: mode 0 (a chain case): int jstart, jend; double xc[nx_src+1], yc[ny_src+1] (radians); double depth_src, mask_src [ny_now*nx_src]
//        mode 1 (a stage case): double depth_filter[ny*nx]; then for each of the three orders (the sequential sweep j then i, the
//        anti-diagonals t = 2j + i, every cell at once): double depth_final[ny*nx], int num_levels[ny*nx], int counts[3]
//        (isolated, partial, shallow); nothing after depth_filter when nk == 0
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "topog.h"

static void rd(void *p, size_t sz, size_t n, FILE *f)
{
  if (n && fread(p, sz, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}
static void wr(const void *p, size_t sz, size_t n, FILE *f)
{
  if (n && fwrite(p, sz, n, f) != n) { fprintf(stderr, "short output\n"); exit(2); }
}

int main(int argc, char **argv)
{
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int hdr[28];
  double par[4];
  rd(hdr, sizeof(int), 28, f);
  rd(par, sizeof(double), 4, f);
  const int mode = hdr[0], nx = hdr[1], ny = hdr[2], nx_src = hdr[3], ny_src = hdr[4], dtype = hdr[5], nk = hdr[6];
  const int tripolar = hdr[7], cyclic_x = hdr[8], cyclic_y = hdr[9], filter_topog = hdr[11], num_pass = hdr[12], deepening = hdr[13];
  const int round_shallow = hdr[14], fill_shallow = hdr[15], deepen_shallow = hdr[16], full_cell = hdr[17], flat_bottom = hdr[18];
  const int adjust_topo = hdr[19], fill_isolated = hdr[20], dcl = hdr[21], kmt_min = hdr[22], open_very = hdr[23];
  const double scale = par[0], min_thickness = par[1], fraction = par[2], missing = par[3];
  std::vector<double> zw(nk);
  rd(zw.data(), sizeof(double), nk, f);
  const size_t n = (size_t)nx * ny;
  if (mode == 0) {
    const size_t np = (size_t)(nx + 1) * (ny + 1);
    std::vector<double> x_dst(np), y_dst(np), xt(nx_src), yt(ny_src), xc(nx_src + 1), yc(ny_src + 1);
    rd(x_dst.data(), sizeof(double), np, f); rd(y_dst.data(), sizeof(double), np, f);
    rd(xt.data(), sizeof(double), nx_src, f); rd(yt.data(), sizeof(double), ny_src, f);
    const size_t esz = dtype == TP_NC_DOUBLE ? 8 : 4;
    std::vector<char> raw((size_t)nx_src * ny_src * esz);
    rd(raw.data(), 1, raw.size(), f);
    tp_axis_bounds(nx_src, xt.data(), xc.data());
    tp_axis_bounds(ny_src, yt.data(), yc.data());
    double y_min = y_dst[0] * TP_D2R, y_max = y_min;                 // as fg_topog_create forms them
    for (size_t i = 1; i < np; i++) { const double y = y_dst[i] * TP_D2R; if (y < y_min) y_min = y; if (y > y_max) y_max = y; }
    int j2[2];
    tp_trim(ny_src, yc.data(), y_min, y_max, &j2[0], &j2[1]);
    const size_t ns = (size_t)nx_src * (j2[1] - j2[0] + 1);
    std::vector<double> depth_src(ns), mask_src(ns);
    const char *rows = raw.data() + (size_t)j2[0] * nx_src * esz;
    for (size_t c = 0; c < ns; c++)
      depth_src[c] = tp_prepare_cell(dtype == TP_NC_FLOAT ? (double)((const float *)rows)[c] : dtype == TP_NC_INT ? (double)((const int *)rows)[c]
                                                                                                               : ((const double *)rows)[c],
                                     missing, scale, &mask_src[c]);
    wr(j2, sizeof(int), 2, o);
    wr(xc.data(), sizeof(double), xc.size(), o); wr(yc.data(), sizeof(double), yc.size(), o);
    wr(depth_src.data(), sizeof(double), ns, o); wr(mask_src.data(), sizeof(double), ns, o);
  } else {
    std::vector<double> depth(n), other(n), rmask(n);
    rd(depth.data(), sizeof(double), n, f);
    if (filter_topog) {
      for (size_t c = 0; c < n; c++) rmask[c] = depth[c] == 0.0 ? 0.0 : 1.0;
      if (nx >= 3 && ny >= 3)
        for (int p = 0; p < num_pass; p++) {
          for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++)
            other[(size_t)j * nx + i] = (i < 1 || i >= nx - 1 || j < 1 || j >= ny - 1) ? depth[(size_t)j * nx + i]
                                                                                         : tp_filter_cell(nx, depth.data(), rmask.data(), i, j, deepening);
          depth.swap(other);
        }
    }
    wr(depth.data(), sizeof(double), n, o);
    if (nk > 0) {
      const int nip = nx + 2, nj_max = tripolar ? ny - 1 : ny;
      std::vector<double> pc(nk);
      tp_p_cell_min(nk, zw.data(), fraction, min_thickness, pc.data());
      for (int order = 0; order < 3; order++) {
        std::vector<double> ht((size_t)nip * (ny + 2), 0.0), out(n);
        std::vector<int> kmt((size_t)nip * (ny + 2), -1), lev(n);
        int counts[3] = {0, 0, 0};
        for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
          double h = depth[(size_t)j * nx + i];
          kmt[(size_t)(j + 1) * nip + i + 1] = tp_kmt_cell(&h, zw.data(), nk, min_thickness, full_cell, flat_bottom);
          ht[(size_t)(j + 1) * nip + i + 1] = h;
        }
        if (tripolar || cyclic_y) for (int i = 1; i <= nx; i++) tp_halo_y_cell(nx, ny, tripolar, ht.data(), kmt.data(), i);
        if (cyclic_x) for (int j = 0; j <= ny + 1; j++) tp_halo_x_cell(nx, ht.data(), kmt.data(), j);
        const bool fill = adjust_topo && fill_isolated;
        if (fill && order == 0)
          for (int j = 1; j <= nj_max; j++) for (int i = 1; i <= nx; i++) counts[0] += tp_isolated_cell(nx, ht.data(), kmt.data(), i, j, dcl);
        if (fill && order == 1)
          for (int t = 3; t <= 2 * nj_max + nx; t++) {
            int jlo, jhi;
            if (!tp_diagonal(nx, nj_max, t, &jlo, &jhi)) continue;
            for (int j = jhi; j >= jlo; j--) counts[0] += tp_isolated_cell(nx, ht.data(), kmt.data(), t - 2 * j, j, dcl);    // any order within a launch
          }
        for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
          const size_t q = (size_t)(j + 1) * nip + i + 1;
          double h = ht[q];
          int k = kmt[q];
          if (fill && order == 2 && j < nj_max) counts[0] += tp_isolated_eval(nx, ht.data(), kmt.data(), i + 1, j + 1, dcl, &k, &h);
          if (adjust_topo) {
            counts[1] += tp_restrict_cell(&h, &k, zw.data(), pc.data(), open_very);
            counts[2] += tp_enforce_cell(&h, &k, zw.data(), kmt_min, round_shallow, deepen_shallow, fill_shallow);
          }
          out[(size_t)j * nx + i] = h;
          lev[(size_t)j * nx + i] = k + 1;
        }
        wr(out.data(), sizeof(double), n, o); wr(lev.data(), sizeof(int), n, o); wr(counts, sizeof(int), 3, o);
      }
    }
  }
  fclose(f);
  if (fclose(o)) return 2;
  return 0;
}
