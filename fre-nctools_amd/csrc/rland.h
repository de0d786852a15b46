// rland.h -- what rland_kernels.hip (device), rland.hip (host orchestration) and tests/hostcheck/rland_check.cpp (a host build)
// share of remap_land's nearest-point search (tools/remap_land/remap_land.c:2520-2607, full_search_nearest and
// search_nearest_sface).  The reference's answer for a query is the lexicographic minimum of (d, l) over the unmasked source
// points, l = face * npts_src + i the flat index and d = great_circle_distance (mosaic_util.c:747) with the host libm.
// The device never forms d.  It finds, with runoff.h's point triples and chords, the set of points whose COMPUTED chord to the
// query is within RL_M of the smallest one; every other point has a strictly larger computed d, so the host
// evaluates the reference's own expression on that set alone, usually one point.  Queries the argument does not cover take
// the reference's loop, restated here, on the host.
#pragma once
#include "runoff.h"

#define RL_TILE RO_TILE            /* compacted unmasked points per tile (fg_rland_tile); fgd_ro_tiles is reused */
#define RL_GROUP RO_GROUP          /* tiles per group: one ballot step */
#define RL_WAVES RO_WAVES          /* queries (waves) per block: ball_walk.hip.h's launch shape */
#define RL_K 4                     /* survivor slots per query; a query with more goes to the exact-size overflow pass */
/* Two points whose computed chords differ by more than RL_M have computed d that differ strictly the same way (DESIGN.md 3.10:
 * the argument needs 2^-45.3; the rest is room). */
#define RL_M 0x1p-40
/* c_min above this: the query takes the host loop.  The survivors of every other query have h <= 1/2 + 2^-39, far from h > 1,
 * where the reference's d is NaN. */
#define RL_CMIN_LIMIT 1.4142135623730951
/* chord to the first unmasked point in scan order at or above this: the reference may accept a NaN d there (d_cur < 0) */
#define RL_ANTIPODE (2.0 - 0x1p-20)
/* The error bound of the haversine is derived for |lon| <= RL_LON_MAX and |lat| <= RL_LAT_MAX; anything else takes the host loop.
 * RL_LAT_MAX is the double nearest to pi/2, just below it: up to there cos(lat) >= 0, so both terms of the haversine are
 * non-negative and cannot cancel.  Beyond it h can come out negative and d NaN for a point that is nowhere near the antipode. */
#define RL_LON_MAX 8.0
#define RL_LAT_MAX 1.5707963267948966
#define RL_RADIUS 6371000.         /* constant.h:24 */

/* host only.  great_circle_distance (mosaic_util.c:754-756), every operation rounded on its own, libm's sin / cos / asin / sqrt */
static inline double rl_haversine(double lon1, double lat1, double lon2, double lat2)
{
  const double s1 = sin((lat1 - lat2) / 2.), s2 = sin((lon1 - lon2) / 2.);
  const double c1 = cos(lat1), c2 = cos(lat2);
  const double beta = 2. * asin(sqrt(s1 * s1 + c1 * c2 * (s2 * s2)));
  return RL_RADIUS * beta;
}

static inline int rl_in_range(double lon, double lat)
{
  return fabs(lon) <= RL_LON_MAX && fabs(lat) <= RL_LAT_MAX;       /* false for NaN */
}

/* The reference's loop for one query (remap_land.c:2534-2551) over the faces m0 .. m1-1: the flat index of its answer, -1 if no
 * point is unmasked.  d_cur = -1 accepts the first unmasked point whatever its d, NaN included; after a NaN nothing is smaller. */
static inline long rl_scan(int m0, int m1, int npts_src, const double *lon_src, const double *lat_src, const int *mask_src,
                           double lon, double lat)
{
  double d_cur = -1;
  long best = -1;
  for (int m = m0; m < m1; m++)
    for (int i = 0; i < npts_src; i++) {
      const long l = (long)m * npts_src + i;
      if (mask_src[l] == 0) continue;
      const double d = rl_haversine(lon, lat, lon_src[l], lat_src[l]);
      if (d_cur < 0 || d < d_cur) { best = l; d_cur = d; }
    }
  return best;
}

/* The survivor rule's other half: the minimum of (d, l) over a query's survivors, in any order.  No survivor's d is NaN. */
static inline long rl_finish(int n, const int *surv, const double *lon_src, const double *lat_src, double lon, double lat)
{
  long best = -1;
  double d_best = 0;
  for (int k = 0; k < n; k++) {
    const long l = surv[k];
    const double d = rl_haversine(lon, lat, lon_src[l], lat_src[l]);
    if (best < 0 || d < d_best || (d == d_best && l < best)) { best = l; d_best = d; }
  }
  return best;
}

/* true: the survivor argument does not cover this query.  c_first: the computed chord to the first unmasked point in scan order. */
static inline int rl_needs_scan(double c_min, double c_first, double lon, double lat)
{
  return !(c_min <= RL_CMIN_LIMIT) || !(c_first < RL_ANTIPODE) || !rl_in_range(lon, lat);
}

/* a point survives when its computed chord is at most c_min + RL_M; a NaN chord never does */
FG_HD bool rl_survives(double chord, double thr) { return chord <= thr; }

#ifdef __HIPCC__
struct RlSearch {
  const RoPoint *pts;            /* [ntiles * RL_TILE] the unmasked points in the space-filling order, idx = flat index, tail NaN */
  const RoBall *ball;            /* [ntiles] */
  const RoBall *gball;           /* [ngroups] */
  const double *qx, *qy, *qz;    /* the converted destination points */
  const int *qlist;              /* [nq] destination index of each query */
  const double *sx, *sy, *sz;    /* the converted source points by flat index */
  int first;                     /* flat index of the first unmasked point in scan order */
  double *cmin, *cfirst;         /* [nq] phase 1 */
  int *count, *slots;            /* [nq], [nq * RL_K] phase 2 */
  int *visited;                  /* [2 * nq] tiles visited per query in phase 1, phase 2 */
  int nq, ntiles, ngroups;
};
void fgd_rl_cmin(const RlSearch &p, int prune, hipStream_t st);
void fgd_rl_survivors(const RlSearch &p, int prune, hipStream_t st);
/* the queries with count > RL_K again: ovq[k] their position in qlist, ovptr[k] where their survivors go in ovout (exact size) */
void fgd_rl_overflow(const RlSearch &p, int nov, const int *ovq, const int *ovptr, int *ovout, int prune, hipStream_t st);
#endif
