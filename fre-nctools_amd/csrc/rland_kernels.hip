// rland_kernels.hip -- remap_land's nearest-point search on the device (tools/remap_land/remap_land.c:2520-2607).
// Host orchestration: rland.hip; the rule shared with the host and the host check: rland.h; the design and the proof: DESIGN.md 3.10.
// The points, tiles and balls are runoff.h's (fgd_ro_xyz, fgd_ro_compact, fgd_ro_balls); the tiles hold the unmasked points in a
// space-filling order, so a tile and a group are compact patches of the sphere.
//
// k_rl_cmin        one wave per query: the smallest computed chord c_min over the unmasked points, and the chord to the first
//                  unmasked point in scan order
// k_rl_survivors   one wave per query: every point with a computed chord <= c_min + RL_M; the count and the first RL_K flat
//                  indices, or (OVERFLOW) all of them into storage of exact size
// No distance is formed here: the host decides among the survivors with the reference's own expression.
#include <hip/hip_runtime.h>
#include <math.h>
#include "rland.h"

// true: every member of the ball has a computed chord > thr.  d - rad is a lower bound of every member's computed chord up to
// 2^-47 in all; RO_MARGIN covers that with room.  NaN anywhere gives false.
__device__ __forceinline__ bool rl_skip(const RoBall &b, double qx, double qy, double qz, double thr)
{
  const double d = sqrt(ro_sumsq(qx, qy, qz, b.x, b.y, b.z));
  return (d - b.rad) - RO_MARGIN > thr;
}

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
  const int q = (blockIdx.x * (64 * RL_WAVES) + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (q >= p.nq) return;                                   // whole waves leave: no block-wide barrier below
  const int qi = p.qlist[q];
  const double qx = p.qx[qi], qy = p.qy[qi], qz = p.qz[qi];
  const int sub = lane / RL_TILE, e = lane % RL_TILE;      // a visit takes 64 / RL_TILE tiles, one per lane group
  constexpr int NSUB = 64 / RL_TILE;
  double s = (double)INFINITY;                             // this lane's smallest sum of squares; a NaN sum never replaces it
  double sbest = (double)INFINITY, cbest = (double)INFINITY;   // the wave's, and its root: sqrt is monotone, so cbest is the smallest chord
  int nvis = 0;
  auto visit = [&](int t) {                                // t < 0: this lane group idles
    if (t >= 0) {
      const RoPoint pt = p.pts[(size_t)t * RL_TILE + e];
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
    // tile whose centre is nearest, and that tile's neighbours in the order.  The scan below visits every tile the bound does
    // not exclude, these again if need be, so the seed only makes the bound tight from the start.
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
    bt = min(bt, p.ntiles - 1) - 1 + sub;
    visit(bt >= 0 && bt < p.ntiles ? bt : -1);
    nvis += NSUB;
    settle();
    for (int g0 = 0; g0 < p.ngroups; g0 += 64) {
      const int g = g0 + lane;
      unsigned long long gm = __ballot(g < p.ngroups && !rl_skip(p.gball[g < p.ngroups ? g : 0], qx, qy, qz, cbest + RL_M));
      bool improved = false;                                          // since this ballot (uniform)
      while (gm) {
        const int gg = g0 + __builtin_ctzll(gm);
        gm &= gm - 1;
        if (improved && rl_skip(p.gball[gg], qx, qy, qz, cbest + RL_M)) continue;
        const int t = gg * RL_GROUP + lane;
        unsigned long long tm = __ballot(t < p.ntiles && !rl_skip(p.ball[t < p.ntiles ? t : 0], qx, qy, qz, cbest + RL_M));
        while (tm) {
          int mine = -1;
#pragma unroll
          for (int k = 0; k < NSUB; k++)
            if (tm) { const int bit = __builtin_ctzll(tm); tm &= tm - 1; nvis++; if (sub == k) mine = gg * RL_GROUP + bit; }
          visit(mine);
        }
        if (settle()) improved = true;
      }
    }
  } else {
    for (int t0 = 0; t0 < p.ntiles; t0 += NSUB) visit(t0 + sub < p.ntiles ? t0 + sub : -1);
    nvis = p.ntiles;
    settle();
  }
  if (lane == 0) {
    p.cmin[q] = cbest;
    p.cfirst[q] = sqrt(ro_sumsq(qx, qy, qz, p.sx[p.first], p.sy[p.first], p.sz[p.first]));
    p.visited[q] = nvis;
  }
}

// The threshold is final here, so the bound is as tight as it gets from the first ballot on.  OVERFLOW: wave w (four per block)
// takes the query ovq[w] and writes all its survivors to ovout[ovptr[w] .. ovptr[w + 1]).
template <bool PRUNE, bool OVERFLOW>
__global__ void __launch_bounds__(64 * RL_WAVES) k_rl_survivors(RlSearch p, int nov, const int *__restrict__ ovq,
                                                                 const int *__restrict__ ovptr, int *__restrict__ ovout)
{
  const int w = (blockIdx.x * (64 * RL_WAVES) + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (w >= (OVERFLOW ? nov : p.nq)) return;
  const int q = OVERFLOW ? ovq[w] : w;
  const int base = OVERFLOW ? ovptr[w] : q * RL_K, cap = OVERFLOW ? ovptr[w + 1] - ovptr[w] : RL_K;
  int *out = OVERFLOW ? ovout : p.slots;
  const int qi = p.qlist[q];
  const double qx = p.qx[qi], qy = p.qy[qi], qz = p.qz[qi];
  const double thr = p.cmin[q] + RL_M;
  const int sub = lane / RL_TILE, e = lane % RL_TILE;
  constexpr int NSUB = 64 / RL_TILE;
  int cnt = 0, nvis = 0;                                   // uniform
  auto visit = [&](int t) {                                // called by the whole wave; t < 0: this lane group idles
    bool hit = false;
    int idx = 0;
    if (t >= 0) {
      const RoPoint pt = p.pts[(size_t)t * RL_TILE + e];
      hit = rl_survives(sqrt(ro_sumsq(qx, qy, qz, pt.x, pt.y, pt.z)), thr);
      idx = pt.idx;
    }
    const unsigned long long m = __ballot(hit);
    const int pos = cnt + __popcll(m & ((1ull << lane) - 1));
    if (hit && pos < cap) out[base + pos] = idx;          // never past the query's own storage
    cnt += __popcll(m);
  };
  if (PRUNE) {
    for (int g0 = 0; g0 < p.ngroups; g0 += 64) {
      const int g = g0 + lane;
      unsigned long long gm = __ballot(g < p.ngroups && !rl_skip(p.gball[g < p.ngroups ? g : 0], qx, qy, qz, thr));
      while (gm) {
        const int gg = g0 + __builtin_ctzll(gm);
        gm &= gm - 1;
        const int t = gg * RL_GROUP + lane;
        unsigned long long tm = __ballot(t < p.ntiles && !rl_skip(p.ball[t < p.ntiles ? t : 0], qx, qy, qz, thr));
        while (tm) {
          int mine = -1;
#pragma unroll
          for (int k = 0; k < NSUB; k++)
            if (tm) { const int bit = __builtin_ctzll(tm); tm &= tm - 1; nvis++; if (sub == k) mine = gg * RL_GROUP + bit; }
          visit(mine);
        }
      }
    }
  } else {
    for (int t0 = 0; t0 < p.ntiles; t0 += NSUB) visit(t0 + sub < p.ntiles ? t0 + sub : -1);
    nvis = p.ntiles;
  }
  if (!OVERFLOW && lane == 0) { p.count[q] = cnt; p.visited[p.nq + q] = nvis; }
}

void fgd_rl_cmin(const RlSearch &p, int prune, hipStream_t st)
{
  if (p.nq < 1) return;
  const dim3 grid((p.nq + RL_WAVES - 1) / RL_WAVES), block(64 * RL_WAVES);
  if (prune) hipLaunchKernelGGL(k_rl_cmin<true>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(k_rl_cmin<false>, grid, block, 0, st, p);
}
void fgd_rl_survivors(const RlSearch &p, int prune, hipStream_t st)
{
  if (p.nq < 1) return;
  const dim3 grid((p.nq + RL_WAVES - 1) / RL_WAVES), block(64 * RL_WAVES);
  if (prune) hipLaunchKernelGGL((k_rl_survivors<true, false>), grid, block, 0, st, p, 0, nullptr, nullptr, nullptr);
  else hipLaunchKernelGGL((k_rl_survivors<false, false>), grid, block, 0, st, p, 0, nullptr, nullptr, nullptr);
}
void fgd_rl_overflow(const RlSearch &p, int nov, const int *ovq, const int *ovptr, int *ovout, int prune, hipStream_t st)
{
  if (nov < 1) return;
  const dim3 grid((nov + RL_WAVES - 1) / RL_WAVES), block(64 * RL_WAVES);
  if (prune) hipLaunchKernelGGL((k_rl_survivors<true, true>), grid, block, 0, st, p, nov, ovq, ovptr, ovout);
  else hipLaunchKernelGGL((k_rl_survivors<false, true>), grid, block, 0, st, p, nov, ovq, ovptr, ovout);
}
