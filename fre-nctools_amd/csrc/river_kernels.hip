// river_kernels.hip -- river_regrid's stages on gfx950 (tools/river_regrid/river_regrid.c; arithmetic: river.h):
//   k_rv_max_suba  calc_max_subA's search (:737-761), one wave per full-land cell.  Every lane carries the cell's four
//                  longitudes through the replay of adjust_lon (uniform work, no communication); the candidates between two
//                  changes of the longitudes are dealt one per lane, each a box clip and a poly_area; one wave maximum at the end.
//   k_rv_tocell    calc_tocell's 3 x 3 stencil (:900-976), one lane per cell
//   k_rv_outlets   cellarea, celllength (:1035-1063), the outlets (:1068-1086) and the successor of every other cell
//   k_rv_jump      one round of pointer jumping; k_rv_finish: travel and basin from the root (:1094-1117)
//   k_rv_level     the accumulated subA of one travel level (:1131-1164)
// Every field lives on the interior cells alone, tiles one after another; a neighbour is read through RvGrid::hmap, which is
// update_halo_double (:776) resolved to the interior cell a haloed index holds, so there is no halo pass between the stages.
#include "river.h"

#define RV_WAVES 4

__device__ __forceinline__ double rv_wave_max(double v)
{
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o, 64); if (w > v) v = w; }
  return v;
}
__device__ __forceinline__ long rv_wave_sum(long v)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((long long)v, o, 64);
  return v;
}

__global__ __launch_bounds__(64 * RV_WAVES) void k_rv_max_suba(RvSource s, RvGrid g, int nland, const int *land, double *maxsub,
                                                                unsigned long long *visited, int prune)
{
  const int lane = threadIdx.x & 63, q = blockIdx.x * RV_WAVES + (threadIdx.x >> 6);
  if (q >= nland) return;
  const int c = land[q], per = g.nx * g.ny, n = c / per, r = c - n * per, j = r / g.nx, i = r - j * g.nx, nxp = g.nx + 1;
  const double *xb = g.xb + (long)n * nxp * (g.ny + 1), *yb = g.yb + (long)n * nxp * (g.ny + 1);
  const int n0 = j * nxp + i, n1 = n0 + 1, n3 = n0 + nxp, n2 = n3 + 1;
  double x[4] = {xb[n0], xb[n1], xb[n2], xb[n3]};
  const double y[4] = {yb[n0], yb[n1], yb[n2], yb[n3]};
  long seen = 0;
  double best = prune ? rv_cell_pruned(s, x, y, g.area[c], lane, 64, &seen) : rv_cell_literal(s, x, y, g.area[c], lane, 64, &seen);
  /* the maximum of values that are > missing, or missing itself: the order of the comparisons does not matter */
  best = rv_wave_max(best);
  seen = rv_wave_sum(seen);
  if (lane == 0) { maxsub[c] = best; atomicAdd(visited, (unsigned long long)seen); }
}

/* haloed index of cell c's neighbour (joff, ioff in 0..2; 1, 1 is the cell) */
__device__ __forceinline__ long rv_halo_index(const RvGrid &g, int n, int j, int i, int joff, int ioff)
{
  return ((long)n * (g.ny + 2) + (j + joff)) * (g.nx + 2) + (i + ioff);
}
struct RvCell { int n, j, i; };           /* j, i: 0-based interior */
__device__ __forceinline__ RvCell rv_cell(const RvGrid &g, long c)
{
  const int per = g.nx * g.ny;
  RvCell k;
  k.n = (int)(c / per);
  const int r = (int)(c - (long)k.n * per);
  k.j = r / g.nx; k.i = r - k.j * g.nx;
  return k;
}

__constant__ int c_out_flow[9] = {8, 4, 2, 16, -1, 1, 32, 64, 128};
__constant__ int c_out_dir[9] = {3, 2, 1, 4, -1, 0, 5, 6, 7};
__constant__ int c_di[8] = {1, 1, 0, -1, -1, -1, 0, 1};
__constant__ int c_dj[8] = {0, -1, -1, -1, 0, 1, 1, 1};

__global__ __launch_bounds__(256) void k_rv_tocell(RvGrid g, const double *maxsub, double suba_cutoff, double subA_missing, int tocell_missing,
                                                    int *tocell, int *dir)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (long)g.ntiles * g.nx * g.ny) return;
  const double lf = g.landfrac[c];
  int t = tocell_missing, d = -1;
  if (lf == 0) { /* ocean: untouched */ }
  else if (lf < 1) t = 0;
  else {
    const RvCell k = rv_cell(g, c);
    double sub[9];
    for (int joff = 0; joff < 3; joff++) for (int ioff = 0; ioff < 3; ioff++) {
      const int h = g.hmap[rv_halo_index(g, k.n, k.j, k.i, joff, ioff)];
      sub[joff * 3 + ioff] = h >= 0 ? maxsub[h] : subA_missing;
    }
    const int slot = rv_tocell_slot(sub, suba_cutoff, subA_missing);
    if (slot >= 0) { t = c_out_flow[slot]; d = c_out_dir[slot]; } else t = 0;
  }
  tocell[c] = t; dir[c] = d;
}

__global__ __launch_bounds__(256) void k_rv_outlets(RvGrid g, const int *tocell, const int *dir, int tocell_missing, double cellarea_missing,
                                                     double celllength_missing, int *flag, int *trav0, int *succ, int *hops,
                                                     double *cellarea, double *celllength)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (long)g.ntiles * g.nx * g.ny) return;
  const RvCell k = rv_cell(g, c);
  const int t = tocell[c], d = dir[c];
  const long me = rv_halo_index(g, k.n, k.j, k.i, 1, 1);
  long dest = -1;
  int hd = -1;
  if (d >= 0) { dest = rv_halo_index(g, k.n, k.j, k.i, 1 + c_dj[d], 1 + c_di[d]); hd = g.hmap[dest]; }
  const double lf = g.landfrac[c];
  double ca = cellarea_missing, cl = celllength_missing;
  if (lf > 0) {
    ca = g.area[c] * lf;
    cl = d >= 0 ? rv_distance(g.xt[me], g.yt[me], g.xt[dest], g.yt[dest]) : 0;
  }
  cellarea[c] = ca; celllength[c] = cl;
  int f = 0, t0 = 0, s = (int)c, h = 0;
  if (t == 0) f = 1;
  else if (t > 0) {
    const int tdest = hd >= 0 ? tocell[hd] : tocell_missing;
    if (tdest == tocell_missing) { f = 1; t0 = 1; }
    else { s = hd; h = 1; }
  }
  flag[c] = f; trav0[c] = t0; succ[c] = s; hops[c] = h;
}

__global__ __launch_bounds__(256) void k_rv_jump(long n, const int *succ, const int *hops, int *succ2, int *hops2, int *changed)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const int s = succ[c], ss = succ[s];
  if (ss != s) { succ2[c] = ss; hops2[c] = hops[c] + hops[s]; *changed = 1; }
  else { succ2[c] = s; hops2[c] = hops[c]; }
}

__global__ __launch_bounds__(256) void k_rv_finish(long n, const int *tocell, int tocell_missing, const int *succ, const int *hops, const int *trav0,
                                                    const int *prefix, int travel_missing, int basin_missing, int *travel, int *basin)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  if (tocell[c] == tocell_missing) { travel[c] = travel_missing; basin[c] = basin_missing; return; }
  const int r = succ[c];
  travel[c] = hops[c] + trav0[r];
  basin[c] = prefix[r] + 1;
}

__global__ __launch_bounds__(256) void k_rv_level(RvGrid g, int level, int count, const int *cells, const int *dir, const int *travel,
                                                   const double *cellarea, double subA_missing, double *subA)
{
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= count) return;
  const int c = cells[q];
  const RvCell k = rv_cell(g, c);
  double sum = cellarea[c];
  for (int joff = 0; joff < 3; joff++) for (int ioff = 0; ioff < 3; ioff++) {
    if (ioff == 1 && joff == 1) continue;
    const int h = g.hmap[rv_halo_index(g, k.n, k.j, k.i, joff, ioff)];
    if (h < 0) continue;                                     /* a corner that no update fills: dir stays -1 */
    int d = dir[h];
    if (d < 0) continue;
    if (g.opcode & RV_CUBIC_GRID) {                          /* the receiver's rotation of a flow that arrives over a tile edge */
      const int ii = k.i + ioff, jj = k.j + joff;            /* haloed coordinates */
      if (ii == 0) { if (k.n % 2 == 0) d = (d + 2) % 8; }
      else if (ii == g.nx + 1) { if (k.n % 2 == 1) d = (d + 2) % 8; }
      else if (jj == 0) { if (k.n % 2 == 1) d = (d + 6) % 8; }
      else if (jj == g.ny + 1) { if (k.n % 2 == 0) d = (d + 6) % 8; }
    }
    if (ioff + c_di[d] == 1 && joff + c_dj[d] == 1)
      sum += travel[h] > level ? subA[h] : subA_missing;     /* what the reference's array holds at this level */
  }
  subA[c] = sum;
}

static inline int rv_nblk(long n, int t) { return (int)((n + t - 1) / t); }

void fgd_rv_max_suba(const RvSource &s, const RvGrid &g, int nland, const int *land, double *maxsub, unsigned long long *visited, int prune, hipStream_t st)
{
  if (nland > 0) k_rv_max_suba<<<rv_nblk(nland, RV_WAVES), 64 * RV_WAVES, 0, st>>>(s, g, nland, land, maxsub, visited, prune);
}
void fgd_rv_tocell(const RvGrid &g, const double *maxsub, double suba_cutoff, double subA_missing, int tocell_missing, int *tocell, int *dir, hipStream_t st)
{
  const long n = (long)g.ntiles * g.nx * g.ny;
  k_rv_tocell<<<rv_nblk(n, 256), 256, 0, st>>>(g, maxsub, suba_cutoff, subA_missing, tocell_missing, tocell, dir);
}
void fgd_rv_outlets(const RvGrid &g, const int *tocell, const int *dir, int tocell_missing, double cellarea_missing, double celllength_missing,
                    int *flag, int *trav0, int *succ, int *hops, double *cellarea, double *celllength, hipStream_t st)
{
  const long n = (long)g.ntiles * g.nx * g.ny;
  k_rv_outlets<<<rv_nblk(n, 256), 256, 0, st>>>(g, tocell, dir, tocell_missing, cellarea_missing, celllength_missing, flag, trav0, succ, hops, cellarea, celllength);
}
void fgd_rv_jump(long n, const int *succ, const int *hops, int *succ2, int *hops2, int *changed, hipStream_t st)
{
  k_rv_jump<<<rv_nblk(n, 256), 256, 0, st>>>(n, succ, hops, succ2, hops2, changed);
}
void fgd_rv_finish(long n, const int *tocell, int tocell_missing, const int *succ, const int *hops, const int *trav0, const int *prefix,
                   int travel_missing, int basin_missing, int *travel, int *basin, hipStream_t st)
{
  k_rv_finish<<<rv_nblk(n, 256), 256, 0, st>>>(n, tocell, tocell_missing, succ, hops, trav0, prefix, travel_missing, basin_missing, travel, basin);
}
void fgd_rv_level(const RvGrid &g, int level, int count, const int *cells, const int *dir, const int *travel, const double *cellarea,
                  double subA_missing, double *subA, hipStream_t st)
{
  if (count > 0) k_rv_level<<<rv_nblk(count, 256), 256, 0, st>>>(g, level, count, cells, dir, travel, cellarea, subA_missing, subA);
}
