// runoff.h -- what runoff_kernels.hip (device), runoff.hip (host orchestration) and tests/hostcheck/runoff_check.cpp (a host
// build) share of runoff_regrid's nearest-ocean step (tools/runoff_regrid/runoff_regrid.c:690-726):
//   distance()   z = sin(lat), x = cos(lat) cos(lon), y = cos(lat) sin(lon) per point, every sin/cos pair one libm sincos() (what
//                gcc -O2 makes of the function), then sqrt(((z1-z2)^2 + (x1-x2)^2) + (y1-y2)^2), nothing contracted
//   nearest()    the first ocean point in row-major order among those with the smallest rounded r, r < r0 strictly:
//                the lexicographic minimum of (r, index)
// The point triple depends on the point alone, so it is formed once per point (ro_xyz); a pair costs ro_sumsq and, only when
// the sum of squares can still win, one correctly rounded square root.
#pragma once
#include "sincos_glibc.h"

#define RO_TILE 16                 /* compacted ocean points per tile (fg_runoff_tile) */
#define RO_GROUP 64                /* tiles per group: one ballot step */
#define RO_WAVES 4                 /* queries (waves) per block */
/* Every coordinate is a product of sines and cosines, so |coordinate| <= 1, every chord is <= 2 sqrt(3) and a computed chord
 * is within 2^-49 of the true one; the prune margin is 2^-40. */
#define RO_MARGIN 0x1p-40

struct __attribute__((aligned(32))) RoPoint { double x, y, z; int idx, pad; };      /* one compacted ocean point: 32 bytes, read as two 16-byte loads */
struct __attribute__((aligned(32))) RoBall { double x, y, z, rad; };              /* centre, and a radius that is no smaller than the true one */

FG_HD void ro_xyz(double lon, double lat, double *x, double *y, double *z)
{
  double sl, cl, so, co;
  fgs_sincos_wide(lat, &sl, &cl);
  fgs_sincos_wide(lon, &so, &co);
  *z = sl; *x = cl * co; *y = cl * so;
}
FG_HD double ro_sumsq(double x1, double y1, double z1, double x2, double y2, double z2)
{
  const double dz = z1 - z2, dx = x1 - x2, dy = y1 - y2;
  return (dz * dz + dx * dx) + dy * dy;
}
/* nearest()'s "some big value": distance(0, pi/2, 0, -pi/2) */
FG_HD double ro_r0(void)
{
  double x1, y1, z1, x2, y2, z2;
  ro_xyz(0.0, M_PI / 2, &x1, &y1, &z1);
  ro_xyz(0.0, -M_PI / 2, &x2, &y2, &z2);
  return sqrt(ro_sumsq(x1, y1, z1, x2, y2, z2));
}

/* The running minimum of (r, idx).  s is the sum of squares r came from; shi bounds the sums that can still round to r. */
struct RoBest { double s, shi, r; int idx; };
FG_HD RoBest ro_best_init(double r0)
{
  RoBest b; b.s = (double)INFINITY; b.shi = (double)INFINITY; b.r = r0; b.idx = -1;   /* (r0, -1): r == r0 never wins */
  return b;
}
/* sqrt is monotone, so s > b.s gives r >= b.r: such a point can only tie, and only wins with a lower index; beyond
 * shi = s (1 + 2^-40) the roots differ by 2^10 ulp and cannot round to the same r.  A NaN sum fails every comparison. */
FG_HD void ro_merge(RoBest &b, double s, double r, int idx)
{
  if (r < b.r || (r == b.r && idx < b.idx)) { b.s = s; b.shi = s * (1.0 + 0x1p-40); b.r = r; b.idx = idx; }
}
FG_HD void ro_consider(RoBest &b, double s, int idx)
{
  if (s < b.s || (idx < b.idx && s <= b.shi)) ro_merge(b, s, sqrt(s), idx);
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
struct RoSearch {
  const double *x, *y, *z;       /* the converted points of the whole grid */
  const RoPoint *pts;            /* [ntiles * RO_TILE] compacted ocean points in row-major order, the tail padded with NaN */
  const RoBall *ball;            /* [ntiles] */
  const RoBall *gball;           /* [ngroups] */
  const int *orank;              /* [n + 1] ocean points before each grid index */
  const int *qindex;             /* [nq] grid index of each query */
  int *iout, *jout;              /* [nq] */
  int *visited;                  /* [nq] tiles visited per query */
  int n, nlon, nq, ntiles, ngroups;
  double r0;
};
void fgd_ro_xyz(long n, const double *lon, const double *lat, double *x, double *y, double *z, hipStream_t st);
/* the tiles and groups of npoints compacted points: pts holds ntiles * RO_TILE records, ball ntiles, gball ngroups */
struct RoTiles { int ntiles, ngroups; };
static inline RoTiles ro_tiles_of(int npoints)
{
  RoTiles t;
  t.ntiles = (npoints + RO_TILE - 1) / RO_TILE; t.ngroups = (t.ntiles + RO_GROUP - 1) / RO_GROUP;
  return t;
}
/* the tile build: the points oidx[0 .. npoints) of x, y, z into pts in that order, then the tile balls and the group balls */
void fgd_ro_tiles(int npoints, const int *oidx, const double *x, const double *y, const double *z, RoPoint *pts, RoBall *ball,
                  RoBall *gball, hipStream_t st);
void fgd_ro_nearest(const RoSearch &p, int prune, hipStream_t st);
struct RoApply {
  const int *rowptr, *src; const double *xarea;      /* exchange list by destination cell, list order within a cell */
  const int *tptr, *tsrc;                            /* land sources by ocean target, ascending */
  const unsigned char *land;                         /* [ncell] mask_out == 0 and mapped */
  const double *area_out, *area_in, *mask_in;
  int ncell_out, ncell_in;
};
void fgd_ro_apply(const RoApply &a, const double *in, double *tmp, double *out, double *totals, hipStream_t st);
#endif
