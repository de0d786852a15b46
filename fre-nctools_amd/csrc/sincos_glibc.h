// sin / cos of latitude-like arguments (|x| < 2.426) with the operation sequence of the host libm the reference links
// against (glibc 2.35, sysdeps/ieee754/dbl-64/s_sin.c: do_sin / do_cos / TAYLOR_SIN over the 1/128-spaced table of
// sincostab.c), so that poly_area / poly_ctrlon / poly_ctrlat evaluate to the reference's BITS on the device.
// libm has two behaviours on an FMA-capable x86-64 host, and the reference's gcc -O2 object code uses both:
//   sin(), cos()   -> the multiarch FMA build of s_sin.c: the same source with gcc's mul+add contraction
//                     (fgs_sin, fgs_cos below: the contracted operations written out as explicit fma)
//   sincos()       -> no contraction (fgs_sincos); gcc turns sin(a) and cos(a) of one argument in one expression into
//                     this call -- poly_ctrlon's f1/f2, poly_ctrlat's 2*cos(avg_y)+lat2*sin(avg_y) in its general branch,
//                     box_ctrlat/ctrlon -- while poly_area_main and the remaining terms call sin()/cos() separately
// (they differ in the last place for 0.07 % of arguments).  geom.hip.h uses each where the compiled reference does.
// Nothing is taken on trust: tests/test_sincos_host.py compiles this header for the host and requires bit-identical
// results to libm's sin(), cos() and sincos() on tens of millions of arguments across the range.
// The end of the file adds the next branch of the same routine (longitudes, up to 1024 rad) and latlon2xyz's vertex on top of it.
// The library itself is built with -ffp-contract=off: the only fused operations are the explicit fma() calls here.
#pragma once
#include <stdint.h>
#include <math.h>
#include "sincos_table.h"

#ifndef FG_HD
#ifdef __HIPCC__
#define FG_HD __host__ __device__ __forceinline__
#else
#define FG_HD static inline
#endif
#endif

/* table access: a translation unit may redirect it (e.g. to a copy in LDS) by defining FGS_TAB before including this header */
#ifndef FGS_TAB
#define FGS_TAB(k, j) FG_SINCOS_TAB[k][j]
#endif

#define FGS_BIG 0x1.8p45                     /* ulp = 1/128: big + |x| rounds |x| to a table node */
#define FGS_HP0 1.5707963267948966           /* pi/2 high */
#define FGS_HP1 6.123233995736766e-17        /* pi/2 low  */

FG_HD int fgs_index(double u)               /* low word of big + |x|: the table node, 0..110 for every supported argument */
{
  union { double d; uint64_t b; } c; c.d = u;
  const uint32_t k = (uint32_t)c.b;
  return (int)(k > 111u ? 111u : k);        /* out-of-range or NaN input (rejected elsewhere) must not index past the table */
}

#define FGS_SN3 (-1.66666666666664880952546298448555E-01)
#define FGS_SN5 8.33333214285722277379541354343671E-03
#define FGS_CS2 4.99999999999999999999950396842453E-01
#define FGS_CS4 (-4.16666666666664434524222570944589E-02)
#define FGS_CS6 1.38888874007937613028114285595617E-03
#define FGS_S1 (-0x1.5555555555555p-3)
#define FGS_S2 0x1.1111111110ECEp-7
#define FGS_S3 (-0x1.A01A019DB08B8p-13)
#define FGS_S4 0x1.71DE27B9A7ED9p-19
#define FGS_S5 (-0x1.ADDFFC2FCDF59p-26)

/* FMA = true: the contraction pattern gcc applies to s_sin.c in the multiarch FMA build (libm sin/cos);
 * FMA = false: every operation rounded separately (libm sincos) */
template <bool FMA>
FG_HD double fgs_taylor_sin(double xx, double x, double dx)
{
  if (FMA) {
    double p = fma(FGS_S5, xx, FGS_S4); p = fma(p, xx, FGS_S3); p = fma(p, xx, FGS_S2); p = fma(p, xx, FGS_S1);
    const double r = fma(p, x, -(0.5 * dx));
    return x + fma(r, xx, dx);
  }
  const double poly = ((((FGS_S5 * xx + FGS_S4) * xx + FGS_S3) * xx + FGS_S2) * xx) + FGS_S1;
  const double t = ((poly * x - 0.5 * dx) * xx + dx);
  return x + t;
}

/* ZDX: the caller passes dx = 0 (arguments below 0.855): `0 + t`, `x*0 + v`, `fma(m, P, 0)`, `fma(x, 0, v)` and `xr + 0` are the
 * identity on the values that occur (xr >= +0 by construction, a - a = +0; the one sign-of-zero case, t = -0 with x = 0,
 * still sums to +0), so they are dropped -- which also lets the compiler share xx, the polynomials and c between the sine
 * and the cosine of one argument.  Checked bit for bit against libm like everything else in this file. */
template <bool FMA, bool ZDX>
FG_HD double fgs_do_sin(double x, double dx)
{
  const double xold = x;
  if (fabs(x) < 0.126) return fgs_taylor_sin<FMA>(x * x, x, ZDX ? 0.0 : dx);
  if (!ZDX && x <= 0) dx = -dx;
  const double u = FGS_BIG + fabs(x);
  x = fabs(x) - (u - FGS_BIG);
  const double xx = x * x;
  const int k = fgs_index(u);
  const double sn = FGS_TAB(k, 0), ssn = FGS_TAB(k, 1), cs = FGS_TAB(k, 2), ccs = FGS_TAB(k, 3);
  double s, c, cor;
  if (FMA) {
    const double P = fma(xx, FGS_SN5, FGS_SN3), Q = fma(xx, fma(xx, FGS_CS6, FGS_CS4), FGS_CS2);
    s = ZDX ? x + (x * xx) * P : x + fma(x * xx, P, dx);
    c = ZDX ? xx * Q : fma(x, dx, xx * Q);
    cor = fma(cs, s, fma(-sn, c, fma(s, ccs, ssn)));
  } else {
    const double P = FGS_SN3 + xx * FGS_SN5, Q = FGS_CS2 + xx * (FGS_CS4 + xx * FGS_CS6);
    s = ZDX ? x + x * xx * P : x + (dx + x * xx * P);
    c = ZDX ? xx * Q : x * dx + xx * Q;
    cor = (ssn + s * ccs - sn * c) + cs * s;
  }
  return copysign(sn + cor, xold);
}

template <bool FMA, bool ZDX>
FG_HD double fgs_do_cos(double x, double dx)
{
  if (!ZDX && x < 0) dx = -dx;
  const double u = FGS_BIG + fabs(x);
  x = ZDX ? fabs(x) - (u - FGS_BIG) : fabs(x) - (u - FGS_BIG) + dx;
  const double xx = x * x;
  const int k = fgs_index(u);
  const double sn = FGS_TAB(k, 0), ssn = FGS_TAB(k, 1), cs = FGS_TAB(k, 2), ccs = FGS_TAB(k, 3);
  double s, c, cor;
  if (FMA) {
    s = fma(x * xx, fma(xx, FGS_SN5, FGS_SN3), x);
    c = xx * fma(xx, fma(xx, FGS_CS6, FGS_CS4), FGS_CS2);
    cor = fma(-sn, s, fma(-cs, c, fma(-s, ssn, ccs)));
  } else {
    s = x + x * xx * (FGS_SN3 + xx * FGS_SN5);
    c = xx * (FGS_CS2 + xx * (FGS_CS4 + xx * FGS_CS6));
    cor = (ccs - s * ssn - cs * c) - sn * s;
  }
  return cs + cor;
}

/* libm sin() / cos() for |x| < 2.426265 on an FMA-capable host (larger arguments never occur for latitudes) */
FG_HD double fgs_sin(double x)
{
  const double ax = fabs(x);
  if (ax < 0x1p-26) return x;
  if (ax < 0.85546875) return fgs_do_sin<true, true>(x, 0);
  const double t = FGS_HP0 - ax;
  return copysign(fgs_do_cos<true, false>(t, FGS_HP1), x);
}
FG_HD double fgs_cos(double x)
{
  const double ax = fabs(x);
  if (ax < 0x1p-27) return 1.0;
  if (ax < 0.85546875) return fgs_do_cos<true, true>(x, 0);
  const double y = FGS_HP0 - ax;
  const double a = y + FGS_HP1;
  const double da = (y - a) + FGS_HP1;
  return fgs_do_sin<true, false>(a, da);
}
/* libm sincos() (s_sincos.c): uncontracted; beyond 0.855 both results come from the (a, da) reduction */
FG_HD void fgs_sincos(double x, double *sinx, double *cosx)
{
  const double ax = fabs(x);
  if (ax < 0x1p-27) { *sinx = x; *cosx = 1.0; return; }
  if (ax < 0.85546875) { *sinx = fgs_do_sin<false, true>(x, 0); *cosx = fgs_do_cos<false, true>(x, 0); return; }
  const double y = FGS_HP0 - ax;
  const double a = y + FGS_HP1;
  const double da = (y - a) + FGS_HP1;
  *sinx = copysign(fgs_do_cos<false, false>(a, da), x);
  *cosx = fgs_do_sin<false, false>(a, da);
}

/* ---------------------------------------------------------------------------------------------------------------------------
 * One evaluation of one argument for any subset of the four results above.  The polygon integrals of geom.hip.h need, of the
 * same latitude, libm's cos() and sincos() (a vertex) or sin(), cos() and sincos() (an edge mid-latitude); called one after the
 * other, each of fgs_sin / fgs_cos / fgs_sincos classifies |x|, reduces it to a table node and reads the node's four values
 * again.  fgs_trig<M> does that once wherever the requested results provably share it, and evaluates only the polynomials and
 * corrections of the results in M.  Every result carries the bits of the function it stands for (tests/test_lat_trig_host.py):
 *   FGS_SIN_F  fgs_sin(x)      FGS_COS_F  fgs_cos(x)      FGS_SIN_N, FGS_COS_N  the two results of fgs_sincos(x)
 * What is shared, by range of |x|:
 *   below 0.85546875   the reduction of |x| itself (dx = 0): one u, r, r*r, node; both cosines and, from 0.126 on, both sines.
 *                      Below 0.126 the sines are the Taylor polynomial of x.  Each result keeps its own tiny-argument
 *                      threshold (2^-26 for sin(), 2^-27 for cos() and sincos()); in between, the sincos() sine is Taylor.
 *   from 0.85546875    cos() and both results of sincos() reduce (a, da), a = (pi/2 - |x|) + low word: one u, r, node.  The
 *                      cosines are do_sin(a, da) -- dx apart from the reduced argument, Taylor for |a| < 0.126 -- the
 *                      sincos() sine is do_cos(a, da) -- dx folded into it.  sin() reduces (pi/2 - |x|, low word) instead:
 *                      its own u and r; its node is a's except when the two straddle a rounding boundary, so the node's
 *                      values are read again only when the indices differ.
 * A result that is not in M is left untouched. */
#define FGS_SIN_F 1
#define FGS_COS_F 2
#define FGS_SIN_N 4
#define FGS_COS_N 8
#define FGS_ALL   15

/* the table part of fgs_do_sin / fgs_do_cos beyond 0.855, on an argument already reduced: r = |x| - node (dx NOT added),
 * dx signed for |x|; the values of the node are passed in */
template <bool FMA>
FG_HD double fgs_sin_core(double r, double dx, double sn, double ssn, double cs, double ccs)
{
  const double xx = r * r;
  double s, c, cor;
  if (FMA) {
    const double P = fma(xx, FGS_SN5, FGS_SN3), Q = fma(xx, fma(xx, FGS_CS6, FGS_CS4), FGS_CS2);
    s = r + fma(r * xx, P, dx);
    c = fma(r, dx, xx * Q);
    cor = fma(cs, s, fma(-sn, c, fma(s, ccs, ssn)));
  } else {
    const double P = FGS_SN3 + xx * FGS_SN5, Q = FGS_CS2 + xx * (FGS_CS4 + xx * FGS_CS6);
    s = r + (dx + r * xx * P);
    c = r * dx + xx * Q;
    cor = (ssn + s * ccs - sn * c) + cs * s;
  }
  return sn + cor;                           /* the caller gives it the argument's sign */
}
template <bool FMA>
FG_HD double fgs_cos_core(double r, double dx, double sn, double ssn, double cs, double ccs)
{
  const double x = r + dx;
  const double xx = x * x;
  double s, c, cor;
  if (FMA) {
    s = fma(x * xx, fma(xx, FGS_SN5, FGS_SN3), x);
    c = xx * fma(xx, fma(xx, FGS_CS6, FGS_CS4), FGS_CS2);
    cor = fma(-sn, s, fma(-cs, c, fma(-s, ssn, ccs)));
  } else {
    s = x + x * xx * (FGS_SN3 + xx * FGS_SN5);
    c = xx * (FGS_CS2 + xx * (FGS_CS4 + xx * FGS_CS6));
    cor = (ccs - s * ssn - cs * c) - sn * s;
  }
  return cs + cor;
}

template <int M>
FG_HD void fgs_trig(double x, double *sin_f, double *cos_f, double *sin_n, double *cos_n)
{
  constexpr bool F = (M & (FGS_SIN_F | FGS_COS_F)) != 0, N = (M & (FGS_SIN_N | FGS_COS_N)) != 0;
  const double ax = fabs(x);
  const bool hi = !(ax < 0.85546875);
  double y = 0.0, a = 0.0, da = 0.0, aw = ax;
  if (hi) { y = FGS_HP0 - ax; a = y + FGS_HP1; da = (y - a) + FGS_HP1; aw = fabs(a); }
  /* the one reduction: of |x| below 0.855, of |a| from there on */
  const double u = FGS_BIG + aw;
  const double r = aw - (u - FGS_BIG);
  const int k = fgs_index(u);
  double sn = FGS_TAB(k, 0), ssn = FGS_TAB(k, 1), cs = FGS_TAB(k, 2), ccs = FGS_TAB(k, 3);
  if (!hi) {
    /* dx = 0 (the ZDX forms of fgs_do_sin / fgs_do_cos): within one contraction mode the sine and the cosine have xx, P, Q
     * and c in common, the uncontracted pair s as well.  They are formed here, ahead of the range tests below, so that each
     * exists once; the cosines need them at every |x|. */
    const double xx = r * r, x3 = r * xx;
    double sf = 0.0, sq = 0.0, cf = 0.0, cq = 0.0;
    double sN = 0.0, cN = 0.0, Pf = 0.0, cF = 0.0;
    if (N) {
      sN = r + x3 * (FGS_SN3 + xx * FGS_SN5);
      cN = xx * (FGS_CS2 + xx * (FGS_CS4 + xx * FGS_CS6));
      if (M & FGS_COS_N) cq = cs + ((ccs - sN * ssn - cs * cN) - sn * sN);
    }
    if (F) {
      Pf = fma(xx, FGS_SN5, FGS_SN3);
      cF = xx * fma(xx, fma(xx, FGS_CS6, FGS_CS4), FGS_CS2);
      if (M & FGS_COS_F) {
        const double s = fma(x3, Pf, r);
        cf = cs + fma(-sn, s, fma(-cs, cF, fma(-s, ssn, ccs)));
      }
    }
    if (M & (FGS_SIN_F | FGS_SIN_N)) {
      if (ax < 0.126) {
        const double x2 = x * x;
        if (M & FGS_SIN_F) sf = ax < 0x1p-26 ? x : fgs_taylor_sin<true>(x2, x, 0.0);
        if (M & FGS_SIN_N) sq = ax < 0x1p-27 ? x : fgs_taylor_sin<false>(x2, x, 0.0);
      } else {
        if (M & FGS_SIN_F) {
          const double s = r + x3 * Pf;
          sf = copysign(sn + fma(cs, s, fma(-sn, cF, fma(s, ccs, ssn))), x);
        }
        if (M & FGS_SIN_N) sq = copysign(sn + ((ssn + sN * ccs - sn * cN) + cs * sN), x);
      }
    }
    const bool tiny = ax < 0x1p-27;
    if (M & FGS_SIN_F) *sin_f = sf;
    if (M & FGS_SIN_N) *sin_n = sq;
    if (M & FGS_COS_F) *cos_f = tiny ? 1.0 : cf;
    if (M & FGS_COS_N) *cos_n = tiny ? 1.0 : cq;
    return;
  }
  const double dw = a < 0 ? -da : da;       /* do_sin flips on a <= 0, but a = 0 is its Taylor path: one sign for both */
  if (M & (FGS_COS_F | FGS_COS_N)) {
    if (fabs(a) < 0.126) {                   /* within 0.126 of a pole */
      const double aa = a * a;
      if (M & FGS_COS_F) *cos_f = fgs_taylor_sin<true>(aa, a, da);
      if (M & FGS_COS_N) *cos_n = fgs_taylor_sin<false>(aa, a, da);
    } else {
      if (M & FGS_COS_F) *cos_f = copysign(fgs_sin_core<true>(r, dw, sn, ssn, cs, ccs), a);
      if (M & FGS_COS_N) *cos_n = copysign(fgs_sin_core<false>(r, dw, sn, ssn, cs, ccs), a);
    }
  }
  if (M & FGS_SIN_N) *sin_n = copysign(fgs_cos_core<false>(r, dw, sn, ssn, cs, ccs), x);
  if (M & FGS_SIN_F) {
    const double ay = fabs(y);
    const double uy = FGS_BIG + ay;
    const double ry = ay - (uy - FGS_BIG);
    const int ky = fgs_index(uy);
    if (ky != k) { sn = FGS_TAB(ky, 0); ssn = FGS_TAB(ky, 1); cs = FGS_TAB(ky, 2); ccs = FGS_TAB(ky, 3); }
    *sin_f = copysign(fgs_cos_core<true>(ry, y < 0 ? -FGS_HP1 : FGS_HP1, sn, ssn, cs, ccs), x);
  }
}

/* ---------------------------------------------------------------------------------------------------------------------------
 * libm sin() / cos() beyond 2.426265 (longitudes): the next branch of s_sin.c, reduce_sincos + do_sincos, with the contractions
 * of the multiarch FMA build written out.  x is reduced by the nearest multiple n * pi/2 -- pi/2 split into mp1 + mp2 + pp3 + pp4,
 * the subtraction carried as a + da -- and the quadrant picks do_cos or do_sin (glibc 2.35's do_sincos: the sine is Taylor below |a| = 0.126, as in do_sin itself).
 * glibc takes this branch up to 105414350; here it ends at FGS_WIDE_MAX = 1024 rad, far outside any longitude frame and the
 * range tests/test_sincos_wide_host.py pins against the host libm.  Beyond it, and for a non-finite argument, the result is
 * NaN (glibc's huge-argument reduction, __branred, is not restated).  Below 2.426265 the results are fgs_sin / fgs_cos. */
#define FGS_WIDE_MIN 0x1.368fdp+1            /* s_sin.c compares the high word with 0x400368fd: 2.42626476..., its "2.426265" */
#define FGS_WIDE_MAX 1024.0
#define FGS_HPINV 0x1.45F306DC9C883p-1       /* 2/pi */
#define FGS_TOINT 0x1.8p52
#define FGS_MP1 0x1.921FB58p0
#define FGS_MP2 (-0x1.DDE973Cp-27)
#define FGS_PP3 (-0x1.CB3B398p-55)
#define FGS_PP4 (-0x1.d747f23e32ed7p-83)

/* x - n * pi/2 = a + da; returns n mod 4 */
FG_HD int fgs_reduce_wide(double x, double *a, double *da)
{
  const double t = fma(x, FGS_HPINV, FGS_TOINT);
  const double xn = t - FGS_TOINT;
  union { double d; uint64_t b; } c; c.d = t;
  const double y = fma(-xn, FGS_MP2, fma(-xn, FGS_MP1, x));
  const double t2 = fma(-xn, FGS_PP3, y);
  double db = fma(-xn, FGS_PP3, y - t2);
  const double b = fma(-xn, FGS_PP4, t2);
  db += fma(-xn, FGS_PP4, t2 - b);
  *a = b; *da = db;
  return (int)(c.b & 3u);
}
/* do_sincos: q = n for the sine, n + 1 for the cosine; odd = do_cos, even = do_sin */
FG_HD double fgs_quadrant(double a, double da, int q)
{
  const double r = (q & 1) ? fgs_do_cos<true, false>(a, da) : fgs_do_sin<true, false>(a, da);
  return (q & 2) ? -r : r;
}
FG_HD double fgs_sin_wide(double x)
{
  const double ax = fabs(x);
  if (ax < FGS_WIDE_MIN) return fgs_sin(x);
  if (!(ax <= FGS_WIDE_MAX)) return (double)NAN;
  double a, da;
  const int n = fgs_reduce_wide(x, &a, &da);
  return fgs_quadrant(a, da, n);
}
FG_HD double fgs_cos_wide(double x)
{
  const double ax = fabs(x);
  if (ax < FGS_WIDE_MIN) return fgs_cos(x);
  if (!(ax <= FGS_WIDE_MAX)) return (double)NAN;
  double a, da;
  const int n = fgs_reduce_wide(x, &a, &da);
  return fgs_quadrant(a, da, n + 1);
}
/* both of one argument: one (a, da, n), one table node.  Of q = n and q = n + 1 one is odd -- do_cos(a, da) -- and one even --
 * the sine of (a, da) -- so each is evaluated once and the quadrant deals them out. */
FG_HD void fgs_sincos_wide_f(double x, double *sinx, double *cosx)
{
  const double ax = fabs(x);
  if (ax < FGS_WIDE_MIN) { fgs_trig<FGS_SIN_F | FGS_COS_F>(x, sinx, cosx, nullptr, nullptr); return; }
  if (!(ax <= FGS_WIDE_MAX)) { *sinx = *cosx = (double)NAN; return; }
  double a, da;
  const int n = fgs_reduce_wide(x, &a, &da);
  const double aw = fabs(a);
  const double u = FGS_BIG + aw;
  const double r = aw - (u - FGS_BIG);
  const int k = fgs_index(u);
  const double sn = FGS_TAB(k, 0), ssn = FGS_TAB(k, 1), cs = FGS_TAB(k, 2), ccs = FGS_TAB(k, 3);
  const double dw = a < 0 ? -da : da;        /* do_sin flips on a <= 0, but a = 0 is its Taylor path: one sign for both */
  const double co = fgs_cos_core<true>(r, dw, sn, ssn, cs, ccs);
  const double si = aw < 0.126 ? fgs_taylor_sin<true>(a * a, a, da) : copysign(fgs_sin_core<true>(r, dw, sn, ssn, cs, ccs), a);
  const double rs = (n & 1) ? co : si, rc = (n & 1) ? si : co;
  *sinx = (n & 2) ? -rs : rs;
  *cosx = ((n + 1) & 2) ? -rc : rc;
}

/* ---------------------------------------------------------------------------------------------------------------------------
 * One vertex of latlon2xyz (mosaic_util.c:212-222): x = cos(lat) * cos(lon), y = cos(lat) * sin(lon), z = sin(lat), each
 * function libm's sin() / cos() (the reference's loop stores between the calls, so gcc does not pair them into sincos()).
 * The latitude is one fgs_trig (cos(lat) is the same value both times), the longitude one fused wide evaluation; the two
 * products are plain multiplies.  Outside the domain -- a non-finite coordinate, |lat| >= 2.426265, |lon| > FGS_WIDE_MAX --
 * the vertex is NaN and the return value false. */
FG_HD bool fgs_latlon2xyz_vertex(double lon, double lat, double *x, double *y, double *z)
{
  const bool ok = fabs(lat) < FGS_WIDE_MIN && fabs(lon) <= FGS_WIDE_MAX;     /* (false for NaN) */
  double sl = 0.0, cl = 0.0, so, co;
  fgs_trig<FGS_SIN_F | FGS_COS_F>(lat, &sl, &cl, nullptr, nullptr);
  fgs_sincos_wide_f(lon, &so, &co);
  *x = ok ? cl * co : (double)NAN;
  *y = ok ? cl * so : (double)NAN;
  *z = ok ? sl : (double)NAN;
  return ok;
}

/* ---------------------------------------------------------------------------------------------------------------------------
 * libm sincos() beyond 2.426265: the same branch of s_sincos.c (reduce_sincos + do_sincos twice, q = n and n + 1) WITHOUT
 * contraction -- every product and sum rounded on its own, as fgs_sincos is below the hand-over.  On the hosts the fixtures
 * come from, libm's sincos() is the uncontracted build on this branch too (tests/test_runoff_cpu.py pins it against the host,
 * bit for bit).  The compiled runoff_regrid.c calls sincos() for every sin/cos pair of distance(), longitudes included.
 * Same range as the siblings above: |x| <= FGS_WIDE_MAX, NaN beyond and for a non-finite argument. */
FG_HD int fgs_reduce_wide_n(double x, double *a, double *da)
{
  const double t = x * FGS_HPINV + FGS_TOINT;
  const double xn = t - FGS_TOINT;
  union { double d; uint64_t b; } c; c.d = t;
  const double y = (x - xn * FGS_MP1) - xn * FGS_MP2;
  double t1 = xn * FGS_PP3;
  const double t2 = y - t1;
  double db = (y - t2) - t1;
  t1 = xn * FGS_PP4;
  const double b = t2 - t1;
  db += (t2 - b) - t1;
  *a = b; *da = db;
  return (int)(c.b & 3u);
}
FG_HD void fgs_sincos_wide(double x, double *sinx, double *cosx)
{
  const double ax = fabs(x);
  if (ax < FGS_WIDE_MIN) { fgs_sincos(x, sinx, cosx); return; }
  if (!(ax <= FGS_WIDE_MAX)) { *sinx = *cosx = (double)NAN; return; }
  double a, da;
  const int n = fgs_reduce_wide_n(x, &a, &da);
  const double co = fgs_do_cos<false, false>(a, da);      /* the odd quadrant of the pair */
  const double si = fgs_do_sin<false, false>(a, da);      /* the even one (Taylor below |a| = 0.126, signed like a) */
  const double rs = (n & 1) ? co : si, rc = (n & 1) ? si : co;
  *sinx = (n & 2) ? -rs : rs;
  *cosx = ((n + 1) & 2) ? -rc : rc;
}
