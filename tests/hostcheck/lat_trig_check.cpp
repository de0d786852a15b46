// Host check of fgs_trig<M> (csrc/sincos_glibc.h): every result must carry the bits of fgs_sin / fgs_cos / fgs_sincos, and of
// the host libm's sin() / cos() / sincos() (test infrastructure; built by tests/test_lat_trig_host.py).
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdint>
#include "sincos_glibc.h"

static inline uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
static inline double ulps(double v, int n)      // v > 0 moved by n units in the last place (steps of the bit pattern)
{
  const uint64_t b = (uint64_t)((int64_t)bits(v) + n);
  double r; memcpy(&r, &b, 8); return r;
}

struct Want { double sf, cf, sn, cn; };
typedef void (*ref_fn)(double, Want *, bool);

static void ref_fgs(double x, Want *w, bool)
{
  w->sf = fgs_sin(x); w->cf = fgs_cos(x); fgs_sincos(x, &w->sn, &w->cn);
}
static void ref_libm(double x, Want *w, bool fma_host)
{
  volatile double xv = x;                       // keep gcc from fusing the two calls below into sincos()
  if (fma_host) { w->sf = sin(xv); w->cf = cos(xv); } else { w->sf = fgs_sin(x); w->cf = fgs_cos(x); }
  sincos(x, &w->sn, &w->cn);
}

// bad[j]: mismatches of result j (sin FMA, cos FMA, sin uncontracted, cos uncontracted) over all masks; a result outside the
// mask must be left untouched
template <int M>
static long check_mask(double x, const Want &w, long *bad)
{
  const double canary = 12345.678;
  double r[4] = {canary, canary, canary, canary};
  fgs_trig<M>(x, &r[0], &r[1], &r[2], &r[3]);
  const double want[4] = {w.sf, w.cf, w.sn, w.cn};
  long nb = 0;
  for (int j = 0; j < 4; j++) {
    const bool ok = (M >> j) & 1 ? bits(r[j]) == bits(want[j]) : bits(r[j]) == bits(canary);
    if (!ok) { bad[j]++; nb++; }
  }
  return nb;
}

static long check_arg(double x, ref_fn ref, bool fma_host, long *bad, double *first_bad)
{
  Want w;
  ref(x, &w, fma_host);
  long nb = 0;
  nb += check_mask<FGS_COS_F | FGS_SIN_N | FGS_COS_N>(x, w, bad);   // a vertex latitude in d_poly_area_ctr
  nb += check_mask<FGS_ALL>(x, w, bad);                            // an edge mid-latitude
  nb += check_mask<FGS_SIN_F>(x, w, bad);
  nb += check_mask<FGS_COS_F>(x, w, bad);
  nb += check_mask<FGS_SIN_F | FGS_COS_F>(x, w, bad);
  nb += check_mask<FGS_SIN_N | FGS_COS_N>(x, w, bad);
  if (nb && *first_bad == 0) *first_bad = x;
  return nb;
}

// libm = 0: against fgs_sin / fgs_cos / fgs_sincos; libm = 1: against the host libm (fma_host = 0: its sincos() only).
// Returns the number of mismatching results; *n_args is the number of arguments tried.
extern "C" long lat_trig_check(long n_uniform, long seed, int libm, int fma_host, long *bad, double *first_bad, long *n_args)
{
  const ref_fn ref = libm ? ref_libm : ref_fgs;
  long nb = 0, na = 0;
  bad[0] = bad[1] = bad[2] = bad[3] = 0; *first_bad = 0;
#define TRY(v) do { nb += check_arg((v), ref, fma_host != 0, bad, first_bad); na++; } while (0)
  srand48(seed);
  for (long i = 0; i < n_uniform; i++) TRY((drand48() * 2 - 1) * 2.426);
  TRY(0.0); TRY(-0.0);
  for (int k = 0; k <= 311; k++)                                   // every table node k/128 up to 2.426, +-0..4 ulp
    for (int d = -4; d <= 4; d++) {
      const double v = (k == 0) ? ldexp((double)d, -1074) : ulps(k / 128.0, d);
      if (fabs(v) > 2.426) continue;
      TRY(v); TRY(-v);
    }
  for (int k = 0; k <= 110; k++)                                   // the nodes of the reduction beyond 0.855: pi/2 -+ k/128
    for (int d = -4; d <= 4; d++) {
      const double lo = ulps(1.5707963267948966 - k / 128.0, d), up = ulps(1.5707963267948966 + k / 128.0, d);
      TRY(lo); TRY(-lo);
      if (up <= 2.426) { TRY(up); TRY(-up); }
    }
  // half way between two nodes big + |x| changes its rounding: the one place where sin()'s node beyond 0.855 (of pi/2 - |x|)
  // and the shared one (of the same plus pi/2's low word) differ, i.e. where fgs_trig reads the table a second time
  for (int k = 0; k <= 110; k++)
    for (int d = -4; d <= 4; d++) {
      const double m = (k + 0.5) / 128.0, lo = ulps(1.5707963267948966 - m, d), up = ulps(1.5707963267948966 + m, d);
      TRY(ulps(m, d)); TRY(-ulps(m, d)); TRY(lo); TRY(-lo);
      if (up <= 2.426) { TRY(up); TRY(-up); }
    }
  // the range thresholds, and where the reduced argument beyond 0.855 crosses the Taylor threshold (pi/2 -+ 0.126)
  const double edges[6] = {0x1p-27, 0x1p-26, 0.126, 0.85546875, 1.5707963267948966 - 0.126, 1.5707963267948966 + 0.126};
  for (int e = 0; e < 6; e++)
    for (int d = -4; d <= 4; d++) { TRY(ulps(edges[e], d)); TRY(-ulps(edges[e], d)); }
  {                                                                // the last 1e-6 below pi/2: random, and the last ulps
    const double hp = 1.5707963267948966;
    for (long i = 0; i < 200000; i++) { const double v = hp - drand48() * 1e-6; TRY(v); TRY(-v); }
    for (int d = 0; d <= 64; d++) { TRY(ulps(hp, -d)); TRY(-ulps(hp, -d)); }
    for (int j = 0; j < 60; j++) { const double v = hp - ldexp(1e-6, -j); TRY(v); TRY(-v); }
  }
#undef TRY
  *n_args = na;
  return nb;
}
