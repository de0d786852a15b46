// rland_kernels.hip -- remap_land's nearest-point search on the device (tools/remap_land/remap_land.c:2520-2607).
// Host orchestration: rland.hip; the rule shared with the host and the host check: rland.h; the design and the proof: DESIGN.md 3.10.
// The points, tiles and balls are runoff.h's (fgd_ro_xyz, fgd_ro_tiles); the tiles hold the unmasked points in a space-filling
// order, so a tile and a group are compact patches of the sphere.  Both kernels walk the balls with ball_walk.hip.h's bw_walk,
// the walk of runoff_kernels.hip's k_ro_nearest; they differ in the threshold, the visit and how the lanes settle.
//
// k_rl_cmin        one wave per query: the smallest computed chord c_min over the unmasked points, and the chord to the first
//                  unmasked point in scan order
// k_rl_survivors   one wave per query: every point with a computed chord <= c_min + RL_M; the count and the first RL_K flat
//                  indices, or (OVERFLOW) all of them into storage of exact size
// No distance is formed here: the host decides among the survivors with the reference's own expression.
#include <hip/hip_runtime.h>
#include <math.h>
#include "rland.h"
#include "ball_walk.hip.h"

__device__ __forceinline__ double rl_wave_min(double v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const double w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
  return v;
}
// all lanes leave with the index of the smallest d, the lowest index among equals; a NaN d is never chosen
__device__ __forceinline__ int rl_wave_argmin(double d, int i)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double w = __shfl_xor(d, o, 64);
    const int j = __shfl_xor(i, o, 64);
    if (w < d || (w == d && j < i)) { d = w; i = j; }
  }
  return i;
}

template <bool PRUNE>
__global__ void __launch_bounds__(64 * RL_WAVES) k_rl_cmin(RlSearch p)
{
  const BwLane l = bw_lane();
  const int q = l.wave, lane = l.lane;
  if (q >= p.nq) return;                                   // whole waves leave: no block-wide barrier below
  const int qi = p.qlist[q];
  const double qx = p.qx[qi], qy = p.qy[qi], qz = p.qz[qi];
  double s = (double)INFINITY;                             // this lane's smallest sum of squares; a NaN sum never replaces it
  double sbest = (double)INFINITY, cbest = (double)INFINITY;   // the wave's, and its root: sqrt is monotone, so cbest is the smallest chord
  int nvis = 0;
  auto visit = [&](int t) {                                // t < 0: this lane group idles
    if (t >= 0) {
      const RoPoint pt = p.pts[(size_t)t * RL_TILE + l.e];
      const double v = ro_sumsq(qx, qy, qz, pt.x, pt.y, pt.z);
      if (v < s) s = v;
    }
  };
  auto settle = [&]() {                                    // the lanes agree again: true if the minimum went down
    if (!__any(s < sbest)) return false;
    sbest = rl_wave_min(s); s = sbest; cbest = sqrt(sbest);
    return true;
  };
  if (PRUNE) {
    // Seed: a query is no member of the source grid, so it has no rank there.  The group whose centre is nearest, in it the
    // tile whose centre is nearest, and that tile's neighbours in the order.  The walk visits every tile the bound does not
    // exclude, these again if need be, so the seed only makes the bound tight from the start.
    double bd = (double)INFINITY;
    int bg = 0;
    for (int g = lane; g < p.ngroups; g += 64) {
      const RoBall b = p.gball[g];
      const double d = ro_sumsq(qx, qy, qz, b.x, b.y, b.z);
      if (d < bd) { bd = d; bg = g; }
    }
    bg = rl_wave_argmin(bd, bg);
    int bt = bg * RL_GROUP + lane;
    bd = (double)INFINITY;
    if (bt < p.ntiles) { const RoBall b = p.ball[bt]; bd = ro_sumsq(qx, qy, qz, b.x, b.y, b.z); }
    bt = rl_wave_argmin(bd, bt);
    bt = min(bt, p.ntiles - 1) - 1 + l.sub;
    visit(bt >= 0 && bt < p.ntiles ? bt : -1);
    nvis += BW_NSUB;
    settle();
  }
  nvis += bw_walk<PRUNE>(p.gball, p.ball, p.ngroups, p.ntiles, qx, qy, qz, l, [&]() { return cbest + RL_M; }, visit, settle);
  if (lane == 0) {
    p.cmin[q] = cbest;
    p.cfirst[q] = sqrt(ro_sumsq(qx, qy, qz, p.sx[p.first], p.sy[p.first], p.sz[p.first]));
    p.visited[q] = nvis;
  }
}

// The threshold is final here, so the bound is as tight as it gets from the first ballot on and no group is tested twice.
// OVERFLOW: wave w (four per block) takes the query ovq[w] and writes all its survivors to ovout[ovptr[w] .. ovptr[w + 1]).
template <bool PRUNE, bool OVERFLOW>
__global__ void __launch_bounds__(64 * RL_WAVES) k_rl_survivors(RlSearch p, int nov, const int *__restrict__ ovq,
                                                                 const int *__restrict__ ovptr, int *__restrict__ ovout)
{
  const BwLane l = bw_lane();
  const int w = l.wave, lane = l.lane;
  if (w >= (OVERFLOW ? nov : p.nq)) return;
  const int q = OVERFLOW ? ovq[w] : w;
  const int base = OVERFLOW ? ovptr[w] : q * RL_K, cap = OVERFLOW ? ovptr[w + 1] - ovptr[w] : RL_K;
  int *out = OVERFLOW ? ovout : p.slots;
  const int qi = p.qlist[q];
  const double qx = p.qx[qi], qy = p.qy[qi], qz = p.qz[qi];
  const double thr = p.cmin[q] + RL_M;
  int cnt = 0;                                             // uniform
  auto visit = [&](int t) {                                // called by the whole wave; t < 0: this lane group idles
    bool hit = false;
    int idx = 0;
    if (t >= 0) {
      const RoPoint pt = p.pts[(size_t)t * RL_TILE + l.e];
      hit = rl_survives(sqrt(ro_sumsq(qx, qy, qz, pt.x, pt.y, pt.z)), thr);
      idx = pt.idx;
    }
    const unsigned long long m = __ballot(hit);
    const int pos = cnt + __popcll(m & ((1ull << lane) - 1));
    if (hit && pos < cap) out[base + pos] = idx;          // never past the query's own storage
    cnt += __popcll(m);
  };
  const int nvis = bw_walk<PRUNE>(p.gball, p.ball, p.ngroups, p.ntiles, qx, qy, qz, l, [&]() { return thr; }, visit, []() { return false; });
  if (!OVERFLOW && lane == 0) { p.count[q] = cnt; p.visited[p.nq + q] = nvis; }
}

void fgd_rl_cmin(const RlSearch &p, int prune, hipStream_t st)
{
  bw_launch(k_rl_cmin<true>, k_rl_cmin<false>, prune, p.nq, st, p);
}
void fgd_rl_survivors(const RlSearch &p, int prune, hipStream_t st)
{
  bw_launch(k_rl_survivors<true, false>, k_rl_survivors<false, false>, prune, p.nq, st, p, 0, nullptr, nullptr, nullptr);
}
void fgd_rl_overflow(const RlSearch &p, int nov, const int *ovq, const int *ovptr, int *ovout, int prune, hipStream_t st)
{
  bw_launch(k_rl_survivors<true, true>, k_rl_survivors<false, true>, prune, nov, st, p, nov, ovq, ovptr, ovout);
}
