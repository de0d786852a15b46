// river_check.cpp -- TEST HARNESS ONLY: csrc/river.h built for the host.  Runs calc_max_subA's search for every full-land cell
// of a case through the same functions the device kernel calls (one lane of one), once as the literal loop and once as the
// pruned replay, so that the replay rule is checked against the reference's fixtures without a device.
//   river_check IN OUT      IN: river_ref_driver's input file followed by area[ntiles][ny*nx]
//   OUT: double literal[ntiles*ny*nx], pruned[ntiles*ny*nx] (the interior of max subA), long visited[2]
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "river.h"

static void rd(void *p, size_t sz, size_t n, FILE *f)
{
  if (fread(p, sz, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

int main(int argc, char **argv)
{
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[7];
  double par[7];
  rd(hdr, sizeof(int), 7, f);
  rd(par, sizeof(double), 7, f);
  const int nx_in = hdr[0], ny_in = hdr[1], ntiles = hdr[2], nx = hdr[3], ny = hdr[4];
  const size_t per = (size_t)nx * ny, perh = (size_t)(nx + 2) * (ny + 2), perb = (size_t)(nx + 1) * (ny + 1);
  std::vector<double> xb(nx_in + 1), yb(ny_in + 1), sub((size_t)nx_in * ny_in), tlon(nx_in);
  rd(xb.data(), sizeof(double), xb.size(), f);
  rd(yb.data(), sizeof(double), yb.size(), f);
  rd(sub.data(), sizeof(double), sub.size(), f);
  std::vector<double> txb(perb * ntiles), tyb(perb * ntiles), skip(perh), lf(per * ntiles), area(per * ntiles);
  for (int n = 0; n < ntiles; n++) {
    rd(&txb[n * perb], sizeof(double), perb, f);
    rd(&tyb[n * perb], sizeof(double), perb, f);
    rd(skip.data(), sizeof(double), perh, f);
    rd(skip.data(), sizeof(double), perh, f);
    rd(&lf[n * per], sizeof(double), per, f);
  }
  rd(area.data(), sizeof(double), area.size(), f);
  fclose(f);
  const double missing = (double)(int)par[1];
  std::vector<int> next((size_t)ny_in * (nx_in + 1));
  for (int j = 0; j < ny_in; j++) {
    int *row = &next[(size_t)j * (nx_in + 1)];
    row[nx_in] = nx_in;
    for (int i = nx_in - 1; i >= 0; i--) row[i] = (sub[(size_t)j * nx_in + i] == missing) ? row[i + 1] : i;
  }
  for (int i = 0; i < nx_in; i++) tlon[i] = 0.5 * (xb[i] + xb[i + 1]);
  RvSource s;
  s.xb = xb.data(); s.yb = yb.data(); s.tlon = tlon.data(); s.subA = sub.data(); s.next = next.data(); s.nx = nx_in; s.ny = ny_in; s.missing = missing;
  std::vector<double> out[2] = {std::vector<double>(per * ntiles, RV_LARGE), std::vector<double>(per * ntiles, RV_LARGE)};
  long visited[2] = {0, 0};
  for (int mode = 0; mode < 2; mode++)
    for (int n = 0; n < ntiles; n++) for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
      const size_t c = n * per + (size_t)j * nx + i;
      if (lf[c] < 1) continue;
      const double *bx = &txb[n * perb], *by = &tyb[n * perb];
      const int n0 = j * (nx + 1) + i, n1 = n0 + 1, n3 = n0 + nx + 1, n2 = n3 + 1;
      double x[4] = {bx[n0], bx[n1], bx[n2], bx[n3]};
      const double y[4] = {by[n0], by[n1], by[n2], by[n3]};
      out[mode][c] = mode ? rv_cell_pruned(s, x, y, area[c], 0, 1, &visited[1]) : rv_cell_literal(s, x, y, area[c], 0, 1, &visited[0]);
    }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(out[0].data(), sizeof(double), out[0].size(), f);
  fwrite(out[1].data(), sizeof(double), out[1].size(), f);
  fwrite(visited, sizeof(long), 2, f);
  fclose(f);
  return 0;
}
