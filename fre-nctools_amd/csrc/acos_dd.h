// Correctly rounded acos / asin: atan2(y, x) in double-double on fp80.h's dd_atan2_pos (~1e-31, relative when the angle is
// below pi/128), rounded once -- the nearest double except when the exact value lies within ~1e-31 of a midpoint.
// The host libm (glibc 2.35 dbl-64) is NOT correctly rounded: it differs from these by one ulp on ~0.07 % of arguments
// (tests/test_bilinear_cpu.py).  So the bilinear path takes the libm values of the reference's acos / sin / asin on the host
// (bilinear_host.c), and uses this header only where a value is compared, not kept: the near-tie branch of the nearest-centre
// choice in k_bl_pairs, which counts the comparisons libm's rounding could decide otherwise.
#pragma once
#include "fp80.h"

// sqrt of a positive double-double, one Newton correction (relative error ~1e-32)
FG_HD dd2 dd_sqrt_pos(dd2 a)
{
  const double s = sqrt(a.hi);
  const dd2 sq = dd_two_prod(s, s);
  const dd2 e = dd_add(a, dd_neg(sq));
  return dd_fast_two_sum(s, e.hi / (2.0 * s));
}

// 1 - x*x as a double-double (exact up to the dd_add rounding, ~2^-106 relative)
FG_HD dd2 dd_one_minus_sq(double x)
{
  return dd_add(dd2{1.0, 0.0}, dd_neg(dd_two_prod(x, x)));
}

// acos(x), |x| <= 1
FG_HDN double fg_acos_cr(double x)
{
  if (x >= 1.0) return 0.0;
  if (x <= -1.0) return 3.14159265358979323846;
  return dd_atan2_pos(dd_sqrt_pos(dd_one_minus_sq(x)), dd2{x, 0.0}).hi;
}

// asin(x), |x| <= 1
FG_HDN double fg_asin_cr(double x)
{
  const double ax = fabs(x);
  if (ax < 0x1p-26) return x;                       // libm: asin(x) = x below 2^-26
  if (ax >= 1.0) return copysign(1.57079632679489661923, x);
  const double r = dd_atan2_pos(dd2{ax, 0.0}, dd_sqrt_pos(dd_one_minus_sq(ax))).hi;
  return copysign(r, x);
}
