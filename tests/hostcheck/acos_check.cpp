// Host check of csrc/acos_dd.h against the host libm's acos / asin (tests/test_bilinear_cpu.py).
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "acos_dd.h"

static uint64_t g_s = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd()
{
  g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17;
  return g_s;
}
static double u01() { return (double)(rnd() >> 11) * 0x1p-53; }

// argument classes: uniform on [-1, 1], next to +-1 (what normalize_great_circle_distance sees for nearby points),
// small magnitudes spread over many binades, and sin*sin products of small angles (what dist2side hands to asin)
static double arg(long i)
{
  switch (i & 3) {
  case 0: return 2.0 * u01() - 1.0;
  case 1: { double d = ldexp(u01(), -(int)(rnd() % 40)); return (rnd() & 1) ? 1.0 - d : -1.0 + d; }
  case 2: { double v = ldexp(u01(), -(int)(rnd() % 60)); return (rnd() & 1) ? v : -v; }
  default: { double a = 0.05 * u01(), b = 3.0 * u01(); return sin(a) * sin(b); }
  }
}

static long ulps(double a, double b)
{
  int64_t ia, ib;
  memcpy(&ia, &a, 8); memcpy(&ib, &b, 8);
  const long d = (long)(ia - ib);
  return d < 0 ? -d : d;
}

// fails[0] / fails[1]: acos / asin results that differ from libm; fails[2]: the largest difference in ulps;
// fails[3]: differences where libm is the one nearer to the exact value (long double reference)
extern "C" long acos_check(long n, long *fails)
{
  fails[0] = fails[1] = fails[2] = fails[3] = 0;
  for (long i = 0; i < n; i++) {
    const double x = arg(i);
    const double r[2][2] = {{fg_acos_cr(x), acos(x)}, {fg_asin_cr(x), asin(x)}};
    const long double ex[2] = {acosl((long double)x), asinl((long double)x)};
    for (int f = 0; f < 2; f++) {
      const long u = ulps(r[f][0], r[f][1]);
      if (!u) continue;
      fails[f]++;
      if (u > fails[2]) fails[2] = u;
      if (fabsl((long double)r[f][1] - ex[f]) < fabsl((long double)r[f][0] - ex[f])) fails[3]++;
    }
  }
  return fails[0] + fails[1];
}
