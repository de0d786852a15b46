// runoff_kernels.hip -- runoff_regrid's nearest-ocean step and runoff move on the device (tools/runoff_regrid/runoff_regrid.c).
// Host orchestration: runoff.hip; the arithmetic shared with the host check: runoff.h; the design and the exactness argument
// of the pruning: DESIGN.md 3.9.
//
// k_ro_xyz       lon, lat -> the point triple of distance(), once per point (the reference forms it once per PAIR)
// k_ro_compact   the ocean points' triples and indices, gathered in row-major order into tiles of RO_TILE
// k_ro_tile_balls / k_ro_group_balls   a bounding ball per tile and per group of RO_GROUP tiles
// k_ro_nearest   one wave per land query: the lexicographic minimum of (r, index) over the ocean points with r < r0; the
//                walk over the balls is ball_walk.hip.h's, shared with rland_kernels.hip
// k_ro_remap / k_ro_move / k_ro_totals   process_data's three loops and its two sums
#include <hip/hip_runtime.h>
#include <math.h>
#include "runoff.h"
#include "ball_walk.hip.h"

__global__ void __launch_bounds__(256) k_ro_xyz(long n, const double *__restrict__ lon, const double *__restrict__ lat,
                                                 double *__restrict__ x, double *__restrict__ y, double *__restrict__ z)
{
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  ro_xyz(lon[i], lat[i], &x[i], &y[i], &z[i]);
}

__global__ void __launch_bounds__(256) k_ro_compact(int nocean, int npad, const int *__restrict__ oidx, const double *__restrict__ x,
                                                     const double *__restrict__ y, const double *__restrict__ z, RoPoint *__restrict__ pts)
{
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= npad) return;
  RoPoint p;
  if (k < nocean) { const int i = oidx[k]; p.x = x[i]; p.y = y[i]; p.z = z[i]; p.idx = i; }
  else { p.x = p.y = p.z = (double)NAN; p.idx = 0x7fffffff; }       // padding: a NaN sum of squares never wins
  p.pad = 0;
  pts[k] = p;
}

// The centre is the mean of the members (any centre is valid); the radius is the largest computed distance to it plus the
// margin that covers the computation's own rounding, so it is never below the true radius.  Padding entries are left out.  A
// NaN member makes the centre, and with it every bound, NaN: such a ball is never skipped.
__device__ __forceinline__ RoBall ro_ball_of_points(const RoPoint *p, int n)
{
  double cx = 0, cy = 0, cz = 0;
  int m = 0;
  for (int k = 0; k < n; k++) if (p[k].idx != 0x7fffffff) { cx += p[k].x; cy += p[k].y; cz += p[k].z; m++; }
  RoBall b;
  b.x = cx / m; b.y = cy / m; b.z = cz / m;
  double rad = 0;
  for (int k = 0; k < n; k++) if (p[k].idx != 0x7fffffff) rad = fmax(rad, sqrt(ro_sumsq(p[k].x, p[k].y, p[k].z, b.x, b.y, b.z)));
  b.rad = rad + RO_MARGIN;
  return b;
}
__global__ void __launch_bounds__(256) k_ro_tile_balls(int ntiles, const RoPoint *__restrict__ pts, RoBall *__restrict__ ball)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < ntiles) ball[t] = ro_ball_of_points(pts + (size_t)t * RO_TILE, RO_TILE);
}
// a group's ball from its tiles' balls: |p - c| <= |p - ct| + |ct - c| <= rad_t + |ct - c|
__global__ void __launch_bounds__(256) k_ro_group_balls(int ntiles, int ngroups, const RoBall *__restrict__ ball, RoBall *__restrict__ gball)
{
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= ngroups) return;
  const int t0 = g * RO_GROUP, t1 = min(t0 + RO_GROUP, ntiles);
  double cx = 0, cy = 0, cz = 0;
  for (int t = t0; t < t1; t++) { cx += ball[t].x; cy += ball[t].y; cz += ball[t].z; }
  RoBall b;
  b.x = cx / (t1 - t0); b.y = cy / (t1 - t0); b.z = cz / (t1 - t0);
  double rad = 0;
  for (int t = t0; t < t1; t++) rad = fmax(rad, sqrt(ro_sumsq(ball[t].x, ball[t].y, ball[t].z, b.x, b.y, b.z)) + ball[t].rad);
  b.rad = rad + RO_MARGIN;
  gball[g] = b;
}

// all lanes leave with the wave's minimum of (r, idx)
__device__ __forceinline__ void ro_wave_min(RoBest &b)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double s = __shfl_xor(b.s, o, 64), r = __shfl_xor(b.r, o, 64);
    const int idx = __shfl_xor(b.idx, o, 64);
    ro_merge(b, s, r, idx);
  }
}

template <bool PRUNE>
__global__ void __launch_bounds__(64 * RO_WAVES) k_ro_nearest(RoSearch p)
{
  const BwLane l = bw_lane();
  const int q = l.wave;
  if (q >= p.nq) return;                                   // whole waves leave: no block-wide barrier below
  const int qi = p.qindex[q];
  const double qx = p.x[qi], qy = p.y[qi], qz = p.z[qi];
  RoBest b = ro_best_init(p.r0);
  int nvis = 0;
  bool dirty = false;                                      // this lane's minimum changed since the last ro_wave_min
  auto visit = [&](int t) {                                // t < 0: this lane group idles
    if (t >= 0) {
      const RoPoint pt = p.pts[(size_t)t * RO_TILE + l.e];
      const int was = b.idx;
      ro_consider(b, ro_sumsq(qx, qy, qz, pt.x, pt.y, pt.z), pt.idx);
      dirty |= b.idx != was;                               // a new minimum is another point
    }
  };
  auto settle = [&]() {                                    // the lanes agree again: true if some lane's minimum had changed
    if (!__any(dirty)) return false;
    ro_wave_min(b);
    dirty = false;
    return true;
  };
  if (PRUNE) {
    // Seed: the tiles around the query's own rank in the compacted list, and around the ranks of its northern and southern
    // neighbours' indices.  The walk visits every tile the bound does not exclude, these again if need be, so the seed only
    // makes the bound tight from the start.
    for (int k = -1; k <= 1; k++) {
      long g = (long)qi + (long)k * p.nlon;
      g = g < 0 ? 0 : (g > p.n ? p.n : g);
      const int t = min(p.orank[g] / RO_TILE, p.ntiles - 1) - 1 + l.sub;
      visit(l.sub < 3 && t >= 0 && t < p.ntiles ? t : -1);
      nvis += 3;
    }
    ro_wave_min(b);
    dirty = false;
  }
  nvis += bw_walk<PRUNE>(p.gball, p.ball, p.ngroups, p.ntiles, qx, qy, qz, l, [&]() { return b.r; }, visit, settle);
  if (l.lane == 0) {
    p.iout[q] = b.idx < 0 ? -1 : b.idx % p.nlon;
    p.jout[q] = b.idx < 0 ? -1 : b.idx / p.nlon;
    p.visited[q] = nvis;
  }
}

// process_data :626-637: out[cell] = sum over the cell's exchange entries, in list order, of in[src] * xarea
__global__ void __launch_bounds__(256) k_ro_remap(RoApply a, const double *__restrict__ in, double *__restrict__ tmp)
{
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.ncell_out) return;
  double v = 0;
  for (int k = a.rowptr[c]; k < a.rowptr[c + 1]; k++) v += in[a.src[k]] * a.xarea[k];
  tmp[c] = v;
}
// :640-653: an ocean target takes its land sources' positive values in ascending order onto its own; a mapped land cell with a
// positive value becomes 0; then the division by the cell area.  Reads tmp, writes out: no cell reads what another writes.
__global__ void __launch_bounds__(256) k_ro_move(RoApply a, const double *__restrict__ tmp, double *__restrict__ out)
{
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.ncell_out) return;
  double v = tmp[c];
  if (a.land[c]) { if (v > 0) v = 0; }
  else for (int k = a.tptr[c]; k < a.tptr[c + 1]; k++) { const double s = tmp[a.tsrc[k]]; if (s > 0) v += s; }
  out[c] = v / a.area_out[c];
}
// :666-671.  Block 0: sum of in * area_in over mask_in > 0; block 1: sum of out * area_out.  Order: thread t adds elements
// t, t + 1024, ... in ascending order, then a binary tree over the 1024 partial sums (stride 512, 256, ..., 1).
__global__ void __launch_bounds__(1024) k_ro_totals(RoApply a, const double *__restrict__ in, const double *__restrict__ out, double *__restrict__ totals)
{
  __shared__ double sh[1024];
  const int t = threadIdx.x;
  double v = 0;
  if (blockIdx.x == 0) { for (int i = t; i < a.ncell_in; i += 1024) if (a.mask_in[i] > 0) v += in[i] * a.area_in[i]; }
  else for (int i = t; i < a.ncell_out; i += 1024) v += out[i] * a.area_out[i];
  sh[t] = v;
  __syncthreads();
  for (int o = 512; o >= 1; o >>= 1) { if (t < o) sh[t] += sh[t + o]; __syncthreads(); }
  if (t == 0) totals[blockIdx.x] = sh[0];
}

void fgd_ro_xyz(long n, const double *lon, const double *lat, double *x, double *y, double *z, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_ro_xyz, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, lon, lat, x, y, z);
}
void fgd_ro_tiles(int npoints, const int *oidx, const double *x, const double *y, const double *z, RoPoint *pts, RoBall *ball,
                  RoBall *gball, hipStream_t st)
{
  const RoTiles t = ro_tiles_of(npoints);
  const int npad = t.ntiles * RO_TILE;
  hipLaunchKernelGGL(k_ro_compact, dim3((npad + 255) / 256), dim3(256), 0, st, npoints, npad, oidx, x, y, z, pts);
  hipLaunchKernelGGL(k_ro_tile_balls, dim3((t.ntiles + 255) / 256), dim3(256), 0, st, t.ntiles, pts, ball);
  hipLaunchKernelGGL(k_ro_group_balls, dim3((t.ngroups + 255) / 256), dim3(256), 0, st, t.ntiles, t.ngroups, ball, gball);
}
void fgd_ro_nearest(const RoSearch &p, int prune, hipStream_t st)
{
  bw_launch(k_ro_nearest<true>, k_ro_nearest<false>, prune, p.nq, st, p);
}
void fgd_ro_apply(const RoApply &a, const double *in, double *tmp, double *out, double *totals, hipStream_t st)
{
  const dim3 grid((a.ncell_out + 255) / 256), block(256);
  hipLaunchKernelGGL(k_ro_remap, grid, block, 0, st, a, in, tmp);
  hipLaunchKernelGGL(k_ro_move, grid, block, 0, st, a, tmp, out);
  hipLaunchKernelGGL(k_ro_totals, dim3(2), dim3(1024), 0, st, a, in, out, totals);
}
