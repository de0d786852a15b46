// ball_walk.hip.h -- the one walk over runoff.h's tiles and balls that the nearest searches share: k_ro_nearest
// (runoff_kernels.hip), k_rl_cmin and k_rl_survivors (rland_kernels.hip).  Device code: include it from .hip files only; the
// host checks under tests/hostcheck include runoff.h / rland.h with g++ and never see it.  The exactness argument: DESIGN.md 3.9.
//
// One wave serves one query.  The compacted points lie in tiles of RO_TILE, the tiles in groups of RO_GROUP = 64, each with a
// bounding ball.  A lane tests one ball per ballot; a visit takes BW_NSUB tiles, one per lane group of RO_TILE lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "runoff.h"

constexpr int BW_NSUB = 64 / RO_TILE;      // tiles per visit

// the kernels' preamble: which query (wave) of the grid this is, and the lane's place in a visit: tile `sub`, element `e`
struct BwLane { int wave, lane, sub, e; };
__device__ __forceinline__ BwLane bw_lane()
{
  BwLane l;
  l.wave = (blockIdx.x * (64 * RO_WAVES) + threadIdx.x) >> 6;
  l.lane = threadIdx.x & 63;
  l.sub = l.lane / RO_TILE;
  l.e = l.lane % RO_TILE;
  return l;
}

// true: every member of the ball has a computed chord > thr.  d - rad is a lower bound of every member's computed chord up to
// 2^-47 in all (the roundings of d, of the difference and of the member's own chord); RO_MARGIN makes the comparison strict
// with room to spare, so a member whose chord equals thr is never discarded.  NaN anywhere gives false.
__device__ __forceinline__ bool bw_skip(const RoBall &b, double qx, double qy, double qz, double thr)
{
  const double d = sqrt(ro_sumsq(qx, qy, qz, b.x, b.y, b.z));
  return (d - b.rad) - RO_MARGIN > thr;
}

// Calls visit(t) for every tile whose ball, and whose group's ball, bw_skip does not exclude at the threshold of the moment;
// returns the number of tiles visited (uniform).  Called by whole waves.
//   thr()     the current threshold, the same in every lane
//   visit(t)  tile t for this lane's group, t < 0: the group idles.  Always called by the whole wave: it may ballot.
//   settle()  makes the lanes agree on the threshold again; returns, the same in every lane, whether it went down
// PRUNE: groups are popped in ascending order; a popped group is tested again only when settle() has returned true since
// the group ballot it came from; the tile ballot uses thr() as it stands then; tiles are dealt lowest bit first, BW_NSUB per
// visit, one count each; settle() follows every popped group that had a tile to visit (after none it would change nothing).
// A lane beyond the last ball loads ball 0 (a clamped index, so the load does not hang on the range test) and votes no.
// !PRUNE: every tile, t0 + sub for t0 = 0, BW_NSUB, ..., then one settle(); the count is ntiles.
// Pass BwLane by value: by reference the deal loop loses its early exits (the compiler flattens it into selects).
template <bool PRUNE, typename Thr, typename Visit, typename Settle>
__device__ __forceinline__ int bw_walk(const RoBall *__restrict__ gball, const RoBall *__restrict__ ball, int ngroups, int ntiles,
                                       double qx, double qy, double qz, BwLane l, Thr thr, Visit visit, Settle settle)
{
  if (!PRUNE) {
    for (int t0 = 0; t0 < ntiles; t0 += BW_NSUB) visit(t0 + l.sub < ntiles ? t0 + l.sub : -1);
    settle();
    return ntiles;
  }
  int nvis = 0;
  for (int g0 = 0; g0 < ngroups; g0 += 64) {
    const int g = g0 + l.lane;
    unsigned long long gm = __ballot(g < ngroups && !bw_skip(gball[g < ngroups ? g : 0], qx, qy, qz, thr()));
    bool improved = false;                                            // since this ballot (uniform)
    while (gm) {
      const int gg = g0 + __builtin_ctzll(gm);
      gm &= gm - 1;
      if (improved && bw_skip(gball[gg], qx, qy, qz, thr())) continue;
      const int t = gg * RO_GROUP + l.lane;
      unsigned long long tm = __ballot(t < ntiles && !bw_skip(ball[t < ntiles ? t : 0], qx, qy, qz, thr()));
      if (!tm) continue;
      while (tm) {
        int mine = -1;
#pragma unroll
        for (int k = 0; k < BW_NSUB; k++)
          if (tm) { const int bit = __builtin_ctzll(tm); tm &= tm - 1; nvis++; if (l.sub == k) mine = gg * RO_GROUP + bit; }
        visit(mine);
      }
      if (settle()) improved = true;                                  // the lanes agree again before the next bound test
    }
  }
  return nvis;
}

// one wave per query, RO_WAVES per block; the pruned or the brute-force instance of a kernel
template <typename... K, typename... A>
static inline void bw_launch(void (*pruned)(K...), void (*brute)(K...), int prune, int nwaves, hipStream_t st, A... args)
{
  if (nwaves < 1) return;
  hipLaunchKernelGGL((prune ? pruned : brute), dim3((nwaves + RO_WAVES - 1) / RO_WAVES), dim3(64 * RO_WAVES), 0, st, args...);
}
