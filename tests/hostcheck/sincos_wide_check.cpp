// Host check of the wide-range part of csrc/sincos_glibc.h (fgs_sin_wide, fgs_cos_wide, fgs_sincos_wide_f, fgs_latlon2xyz_vertex)
// against the host libm's sin()/cos() (test infrastructure; built by tests/test_sincos_wide_host.py).
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <cstdlib>
#include <cstring>
#include <cmath>
#include "sincos_glibc.h"

static const double HPI = 1.5707963267948966;
static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0; }
static double rsign() { return drand48() < 0.5 ? -1.0 : 1.0; }
static double draw(long i)
{
  switch (i % 8) {
    case 0: return (drand48() * 2 - 1) * 8 * HPI;                                           // [-4 pi, 4 pi]
    case 1: return drand48() * 4 * HPI;                                                     // [0, 2 pi]
    case 2: return ((long)(drand48() * 17) - 8) * HPI + rsign() * ldexp(1.0, -(int)(drand48() * 46));              // k pi/2 +- 2^-e
    case 3: return ((long)(drand48() * 17) - 8) * HPI + ldexp(drand48() * 2 - 1, -(int)(drand48() * 46));          // ... any mantissa
    case 4: return rsign() * (2.426265 + ldexp(drand48() - 0.5, -(int)(drand48() * 50)));                           // the hand-over
    case 5: return ((long)(drand48() * 17) - 8) * HPI + rsign() * (0.12601587 + ldexp(drand48() - 0.5, -(int)(drand48() * 40)));   // a*a ~ 0.01588
    case 6: return ((long)(drand48() * 17) - 8) * HPI + rsign() * (0.126 + ldexp(drand48() - 0.5, -(int)(drand48() * 40)));        // |a| ~ 0.126
    default: return (drand48() * 2 - 1) * 1000.0;                                           // up to +-1000
  }
}
static void one(double x, long *bad_sin, long *bad_cos, long *bad_fused, double *first_bad)
{
  volatile double xv = x;                         // keep gcc from fusing the two calls below into sincos()
  const double ls = sin(xv), lc = cos(xv);
  const double ws = fgs_sin_wide(x), wc = fgs_cos_wide(x);
  double fs, fc;
  fgs_sincos_wide_f(x, &fs, &fc);
  const bool first = !*bad_sin && !*bad_cos && !*bad_fused;
  if (!same(ws, ls)) { if (first) *first_bad = x; (*bad_sin)++; }
  if (!same(wc, lc)) { if (first) *first_bad = x; (*bad_cos)++; }
  if (!same(fs, ws) || !same(fc, wc)) { if (first) *first_bad = x; (*bad_fused)++; }
}
// bad_sin / bad_cos: fgs_sin_wide / fgs_cos_wide differ from libm; bad_fused: the fused form differs from the two single calls
extern "C" long sincos_wide_check(long n, long seed, long *bad_sin, long *bad_cos, long *bad_fused, double *first_bad)
{
  srand48(seed);
  *bad_sin = *bad_cos = *bad_fused = 0; *first_bad = 0;
  const double fixed[] = {0.0, -0.0, 1000.0, -1000.0, FGS_WIDE_MAX, -FGS_WIDE_MAX, FGS_WIDE_MIN, -FGS_WIDE_MIN, 4 * HPI, -4 * HPI, 2 * HPI, 8 * HPI};
  for (double x : fixed) one(x, bad_sin, bad_cos, bad_fused, first_bad);
  for (int k = -8; k <= 8; k++)
    for (int e = 0; e <= 45; e++)
      for (int s = -1; s <= 1; s++) one(k * HPI + s * ldexp(1.0, -e), bad_sin, bad_cos, bad_fused, first_bad);
  for (long i = 0; i < n; i++) one(draw(i), bad_sin, bad_cos, bad_fused, first_bad);
  return *bad_sin + *bad_cos + *bad_fused;
}
// the fused form against the two single calls only (needs no FMA host)
extern "C" long sincos_wide_fused_check(long n, long seed, double *first_bad)
{
  srand48(seed);
  long bad = 0; *first_bad = 0;
  for (long i = 0; i < n; i++) {
    const double x = draw(i);
    double fs, fc;
    fgs_sincos_wide_f(x, &fs, &fc);
    if (!same(fs, fgs_sin_wide(x)) || !same(fc, fgs_cos_wide(x))) { if (!bad) *first_bad = x; bad++; }
  }
  return bad;
}
// arguments beyond the bound and non-finite ones: every result must be NaN.  Returns the number that is not.
extern "C" long sincos_wide_nan_check(void)
{
  const double xs[] = {nextafter(FGS_WIDE_MAX, 2e3), -nextafter(FGS_WIDE_MAX, 2e3), 1025.0, 1e6, -1e6, 105414350.0, 1e300, -1e300,
                       (double)INFINITY, -(double)INFINITY, (double)NAN};
  long bad = 0;
  for (double x : xs) {
    double fs, fc;
    fgs_sincos_wide_f(x, &fs, &fc);
    bad += !std::isnan(fgs_sin_wide(x)) + !std::isnan(fgs_cos_wide(x)) + !std::isnan(fs) + !std::isnan(fc);
  }
  return bad;
}
// the per-vertex body of k_latlon2xyz over n vertices; returns the number of vertices outside the domain
extern "C" long latlon2xyz_vertex_loop(long n, const double *lon, const double *lat, double *x, double *y, double *z)
{
  long out = 0;
  for (long i = 0; i < n; i++) out += !fgs_latlon2xyz_vertex(lon[i], lat[i], &x[i], &y[i], &z[i]);
  return out;
}
