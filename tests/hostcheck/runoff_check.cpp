// Host build of what the device shares with the host of runoff_regrid's nearest-ocean step (csrc/runoff.h, and the uncontracted
// wide sincos of csrc/sincos_glibc.h), as a stand-alone program (test infrastructure; built by tests/test_runoff_cpu.py; this is
// also the program to build with -fsanitize=address,undefined and run directly, if a sanitizer run is wanted).
//   runoff_check sincos N SEED     fgs_sincos_wide against this host's sincos(), bit for bit: densely over [-4 pi, 4 pi], around the
//                                  multiples of pi/2 and the hand-over points, sparsely out to 1024; NaN beyond.  Prints "bad K first X".
//   runoff_check nearest IN OUT    IN: int nlon, nlat; double mask[n], lon[n], lat[n].  OUT: int imap[n], jmap[n]; double x[n], y[n],
//                                  z[n].  nearest() for every point with mask == 0, brute force in the reference's own scan order
//                                  with its strict <; the same through ro_consider in a scrambled order must agree (exit 3 if not).
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include "runoff.h"

static const double HPI = 1.5707963267948966;
static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0; }
static double rsign() { return drand48() < 0.5 ? -1.0 : 1.0; }
static double draw(long i)
{
  switch (i % 8) {
    case 0: case 1: return (drand48() * 2 - 1) * 8 * HPI;                                   // [-4 pi, 4 pi]
    case 2: return ((long)(drand48() * 17) - 8) * HPI + rsign() * ldexp(1.0, -(int)(drand48() * 46));              // k pi/2 +- 2^-e
    case 3: return ((long)(drand48() * 17) - 8) * HPI + ldexp(drand48() * 2 - 1, -(int)(drand48() * 46));          // ... any mantissa
    case 4: return rsign() * (2.426265 + ldexp(drand48() - 0.5, -(int)(drand48() * 50)));                           // the hand-over
    case 5: return ((long)(drand48() * 17) - 8) * HPI + rsign() * (0.126 + ldexp(drand48() - 0.5, -(int)(drand48() * 40)));   // |a| ~ 0.126
    case 6: return rsign() * (0.85546875 + ldexp(drand48() - 0.5, -(int)(drand48() * 50)));                         // sincos()'s own
    default: return (drand48() * 2 - 1) * 1024.0;                                           // out to the bound
  }
}

static int check_sincos(long n, long seed)
{
  srand48(seed);
  long bad = 0;
  double first = 0;
  auto one = [&](double x) {
    double ls, lc, ws, wc;
    volatile double xv = x;
    sincos(xv, &ls, &lc);
    fgs_sincos_wide(x, &ws, &wc);
    if (!same(ws, ls) || !same(wc, lc)) { if (!bad) first = x; bad++; }
  };
  const double fixed[] = {0.0, -0.0, 1000.0, -1000.0, FGS_WIDE_MAX, -FGS_WIDE_MAX, FGS_WIDE_MIN, -FGS_WIDE_MIN, 4 * HPI, -4 * HPI, 2 * HPI, 8 * HPI, HPI, -HPI};
  for (double x : fixed) one(x);
  for (int k = -8; k <= 8; k++) for (int e = 0; e <= 45; e++) for (int s = -1; s <= 1; s++) one(k * HPI + s * ldexp(1.0, -e));
  for (long i = 0; i < n; i++) one(draw(i));
  const double beyond[] = {nextafter(FGS_WIDE_MAX, 2e3), -1025.0, 1e300, (double)INFINITY, -(double)INFINITY, (double)NAN};
  for (double x : beyond) {
    double s, c;
    fgs_sincos_wide(x, &s, &c);
    if (!std::isnan(s) || !std::isnan(c)) { if (!bad) first = x; bad++; }
  }
  printf("bad %ld first %.17g\n", bad, first);
  return bad ? 1 : 0;
}

static int check_nearest(const char *in, const char *out)
{
  FILE *f = fopen(in, "rb");
  int dims[2];
  if (!f || fread(dims, sizeof(int), 2, f) != 2) { fprintf(stderr, "cannot read %s\n", in); return 2; }
  const int nlon = dims[0], nlat = dims[1], n = nlon * nlat;
  std::vector<double> mask(n), lon(n), lat(n), x(n), y(n), z(n);
  if (fread(mask.data(), 8, n, f) != (size_t)n || fread(lon.data(), 8, n, f) != (size_t)n || fread(lat.data(), 8, n, f) != (size_t)n) { fprintf(stderr, "short input\n"); return 2; }
  fclose(f);
  for (int i = 0; i < n; i++) ro_xyz(lon[i], lat[i], &x[i], &y[i], &z[i]);
  const double r0 = ro_r0();
  std::vector<int> imap(n, -1), jmap(n, -1);
  int stride = 7;
  while (n % stride == 0) stride += 2;                                      // coprime with n: k * stride mod n visits every point once
  for (int q = 0; q < n; q++) {
    if (!(mask[q] == 0.0)) continue;
    double r = r0;
    int best = -1;
    for (int p = 0; p < n; p++) {                                           // runoff_regrid.c:715-724
      if (mask[p] == 0.0) continue;
      const double r1 = sqrt(ro_sumsq(x[q], y[q], z[q], x[p], y[p], z[p]));
      if (r1 < r) { best = p; r = r1; }
    }
    RoBest b = ro_best_init(r0);
    for (long k = 0; k < n; k++) {
      const int p = (int)((k * stride + q) % n);
      if (!(mask[p] == 0.0)) ro_consider(b, ro_sumsq(x[q], y[q], z[q], x[p], y[p], z[p]), p);
    }
    if (b.idx != best) { fprintf(stderr, "query %d: scan order gives %d, ro_consider in scrambled order %d\n", q, best, b.idx); return 3; }
    if (best >= 0) { imap[q] = best % nlon; jmap[q] = best / nlon; }
  }
  f = fopen(out, "wb");
  if (!f) { fprintf(stderr, "cannot write %s\n", out); return 2; }
  fwrite(imap.data(), sizeof(int), n, f); fwrite(jmap.data(), sizeof(int), n, f);
  fwrite(x.data(), 8, n, f); fwrite(y.data(), 8, n, f); fwrite(z.data(), 8, n, f);
  fclose(f);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 4 && !strcmp(argv[1], "sincos")) return check_sincos(atol(argv[2]), atol(argv[3]));
  if (argc == 4 && !strcmp(argv[1], "nearest")) return check_nearest(argv[2], argv[3]);
  fprintf(stderr, "usage: %s sincos N SEED | nearest IN OUT\n", argv[0]);
  return 2;
}
