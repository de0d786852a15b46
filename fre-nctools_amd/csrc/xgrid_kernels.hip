// xgrid_kernels.hip -- exchange-grid search kernels for gfx950 (MI355X).
//
// Pipeline for one destination tile against all source tiles:
//
//   k_cell_struct2     per cell (source tiles and destination tile in one launch): lat min/max, fix_lon, lon
//                      min/max/avg, <=8 vertices, area [get_grid_cell_struct semantics, create_xgrid.c:991-1016;
//                      get_grid_area :66-88]; destination cells are counted into their bins on the way
//   k_scan1            single-pass exclusive scan (decoupled look-back) of the bin counts / row counts
//   k_bin_fill         destination cells -> uniform (lat x lon mod 2pi) bins, one 48-byte record per
//                      cell stored in bin order (single insertion; wide cells in per-row lists); the same launch lists
//                      the source cells whose query is large (poles: huge longitude range)
//   k_candidates1      per source cell: scan the <= 2 contiguous record ranges per bin row, apply the reference's
//                      exact bounding-box rejects (create_xgrid.c:1055-1079) -> candidate pairs
//                      [get_upbound_nxcells_2dx2d semantics], appended to the pair list in ONE pass (a wave reserves
//                      its range with one atomic on a region counter); listed cells get a whole wave, same launch
//   k_clip_quad        one lane per candidate pair, quad x quad fast path: Sutherland-Hodgman
//                      clip (create_xgrid.c:1266-1341) with the polygon staged in LDS
//                      [vertex][lane], then area / centroid integrals and the 1e-6 area test
//   k_clip_general     same for pairs with pole-fixed cells (5..8 vertices) or fast-path overflow
//   k_compact(+_big)   compaction into the reference's canonical order (source cell ascending, destination cell index
//                      ascending): a block owns 256 consecutive source cells, counts their accepted pairs, takes its
//                      offset by look-back, ranks, writes the exchange cells coalesced, takes the destination-row slots
//                      and adds up the per-source-cell sums in exchange-cell order (conserve_interp.c:216-221)
//   k_centroids, k_distances     order-2 centroid pass (conserve_interp.c:319-358)
//
// No MFMA: this is FP64 VALU + irregular gather work.  Every floating-point operation uses the reference's expression
// trees, sin/cos included (geom.hip.h, sincos_glibc.h): lists, areas and centroid integrals are the reference's bits.
// Launched either for exact sizes or for fixed capacities with the true counts read from device memory (np_dev, cap).
#include <algorithm>
#include "xgrid_device.h"
#ifndef FG_EXP
#define FG_EXP 0      // timing experiments (scripts/exp_build.sh): 1 = no integrals, 2 = no clip loop
#endif
// The 3.5 KB sin/cos table of sincos_glibc.h is copied into LDS by every kernel of this file that takes sines: the lookups
// are per-lane gathers (index = latitude * 128), and from LDS they cost the clip kernel 0.42 ms instead of 0.48 ms from global
// memory, although the extra LDS and registers lower its occupancy from 5 to 4 waves per SIMD.
static __shared__ double fgs_lds_tab[112 * 4];
#define FGS_TAB(k, j) fgs_lds_tab[(k) * 4 + (j)]
#include "geom.hip.h"
__device__ __forceinline__ void d_load_trig_table()
{
  for (int i = threadIdx.x; i < 112 * 4; i += blockDim.x) fgs_lds_tab[i] = FG_SINCOS_TAB[i >> 2][i & 3];
  __syncthreads();
}

// ---------------------------------------------------------------------------------------
// single-pass exclusive scan (decoupled look-back) and the look-back itself
// ---------------------------------------------------------------------------------------
// A tile publishes its aggregate in one 64-bit word {flag:2, value:62} and walks back over its predecessors until it meets
// one whose inclusive prefix is known.  Tiles are numbered by a ticket taken when the block starts, so every predecessor a
// block waits for is already running: the wait ends whatever order the hardware dispatches blocks in.  The spin is bounded
// all the same (G_ERRBIT_LOOKBACK).  Value and flag share the word, so relaxed agent-scope accesses are all the protocol needs.
#define SCAN_THREADS 256
#define SCAN_ITEMS   8
#define SCAN_CHUNK   (SCAN_THREADS * SCAN_ITEMS)
#define LB_AGG   (1ull << 62)
#define LB_INC   (2ull << 62)
#define LB_MASK  ((1ull << 62) - 1ull)
#define LB_SPIN_LIMIT (1u << 22)

__device__ __forceinline__ unsigned wave_incl_scan(unsigned v, int lane)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    unsigned t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// inclusive scan across a 256-thread block; returns this thread's inclusive value and the block total
__device__ __forceinline__ unsigned block_incl_scan(unsigned v, unsigned *total)
{
  __shared__ unsigned wsum[4];
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = wave_incl_scan(v, lane);
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { if (k < w) base += wsum[k]; tot += wsum[k]; }
  __syncthreads();
  *total = tot;
  return inc + base;
}

__device__ __forceinline__ unsigned long long lb_load(const unsigned long long *p)
{
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lb_store(unsigned long long *p, unsigned long long v)
{
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Called by all 64 lanes of ONE wave of the block owning `tile`; returns the sum of the aggregates of tiles 0..tile-1 and
// publishes this tile's inclusive prefix.  Each round inspects 64 predecessors at once.
__device__ inline unsigned long long d_lookback_wave(unsigned long long *status, int tile, unsigned long long agg, unsigned *err)
{
  const int lane = threadIdx.x & 63;
  if (tile == 0) { if (lane == 0) lb_store(&status[0], LB_INC | (agg & LB_MASK)); return 0ull; }
  if (lane == 0) lb_store(&status[tile], LB_AGG | (agg & LB_MASK));
  unsigned long long excl = 0ull;
  int base = tile - 1;
  unsigned spins = 0;
  for (;;) {
    const int t = base - lane;
    const unsigned long long v = (t >= 0) ? lb_load(&status[t]) : LB_INC;      // "tiles" before the first: prefix 0, known
    const unsigned flag = (unsigned)(v >> 62);
    const unsigned long long inc = __ballot(flag == 2u), zero = __ballot(flag == 0u);
    const int first_inc = inc ? (__ffsll((long long)inc) - 1) : 63;
    const unsigned long long need = (first_inc >= 63) ? ~0ull : ((2ull << first_inc) - 1ull);   // lanes 0..first_inc
    if (zero & need) {                                  // a predecessor this round depends on has not published yet
      if (++spins > LB_SPIN_LIMIT) { if (lane == 0) atomicOr(err, G_ERRBIT_LOOKBACK); break; }
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    unsigned long long val = ((need >> lane) & 1ull) ? (v & LB_MASK) : 0ull;
#pragma unroll
    for (int o = 32; o; o >>= 1) val += __shfl_xor(val, o);
    excl += val;
    if (inc) break;
    base -= 64;
  }
  if (lane == 0) lb_store(&status[tile], LB_INC | ((excl + agg) & LB_MASK));
  return excl;
}

// out[i] = exclusive prefix for i in [0, n] (n inputs, n+1 outputs; 32-bit offsets, 64-bit total for the host's checks)
__global__ __launch_bounds__(SCAN_THREADS) void k_scan1(const int *in, long n, int *out, unsigned long long *status, unsigned *ticket,
                                                        unsigned long long *total_out, unsigned *err)
{
  __shared__ unsigned tile[SCAN_CHUNK];
  __shared__ int sh_t;
  __shared__ unsigned long long sh_excl;
  // ticket == null: the grid is small enough to be resident all at once, so no tile can wait for one that has not started
  if (ticket) { if (threadIdx.x == 0) sh_t = (int)atomicAdd(ticket, 1u); __syncthreads(); }
  const int t = ticket ? sh_t : (int)blockIdx.x;
  const long base = (long)t * SCAN_CHUNK;
  // thread k owns items k*SCAN_ITEMS .. +SCAN_ITEMS-1 of the chunk (blocked arrangement via LDS, coalesced global accesses)
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    const int li = k * SCAN_THREADS + threadIdx.x;
    const long idx = base + li;
    tile[li] = (idx < n) ? (unsigned)in[idx] : 0u;
  }
  __syncthreads();
  unsigned loc[SCAN_ITEMS];
  unsigned s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) { loc[k] = tile[threadIdx.x * SCAN_ITEMS + k]; s += loc[k]; }
  unsigned tot;
  const unsigned inc = block_incl_scan(s, &tot);
  if (threadIdx.x < 64) {
    const unsigned long long e = d_lookback_wave(status, t, (unsigned long long)tot, err);
    if (threadIdx.x == 0) sh_excl = e;
  }
  __syncthreads();
  const unsigned long long excl = sh_excl;
  unsigned run = (unsigned)excl + inc - s;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) { tile[threadIdx.x * SCAN_ITEMS + k] = run; run += loc[k]; }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    const int li = k * SCAN_THREADS + threadIdx.x;
    const long idx = base + li;
    if (idx <= n) out[idx] = (int)tile[li];
  }
  if (threadIdx.x == 0 && n >= base && n < base + SCAN_CHUNK) *total_out = excl + tot;      // the tile holding out[n]
}

// two independent scans in one launch (blockIdx.y picks the job): the accept-count scan and the destination-row scan of a search
// depend on the same kernel and feed the same one -- a launch boundary less on a path that is launch bound for small bands
struct FgScanJob { const int *in; long n; int *out; unsigned long long *status; unsigned *ticket; unsigned long long *total; };
__global__ __launch_bounds__(SCAN_THREADS) void k_scan2(FgScanJob a, FgScanJob b, unsigned *err, int by_ticket)
{
  const FgScanJob j = blockIdx.y ? b : a;
  const long nt = (j.n + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK;
  if ((long)blockIdx.x >= nt) return;
  __shared__ unsigned tile[SCAN_CHUNK];
  __shared__ int sh_t;
  __shared__ unsigned long long sh_excl;
  // by_ticket == 0: the whole grid is resident at once, no tile can wait for one that has not started
  if (by_ticket) { if (threadIdx.x == 0) sh_t = (int)atomicAdd(j.ticket, 1u); __syncthreads(); }
  const int t = by_ticket ? sh_t : (int)blockIdx.x;
  const long base = (long)t * SCAN_CHUNK;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    const int li = k * SCAN_THREADS + threadIdx.x;
    const long idx = base + li;
    tile[li] = (idx < j.n) ? (unsigned)j.in[idx] : 0u;
  }
  __syncthreads();
  unsigned loc[SCAN_ITEMS];
  unsigned s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) { loc[k] = tile[threadIdx.x * SCAN_ITEMS + k]; s += loc[k]; }
  unsigned tot;
  const unsigned inc = block_incl_scan(s, &tot);
  if (threadIdx.x < 64) {
    const unsigned long long e = d_lookback_wave(j.status, t, (unsigned long long)tot, err);
    if (threadIdx.x == 0) sh_excl = e;
  }
  __syncthreads();
  const unsigned long long excl = sh_excl;
  unsigned run = (unsigned)excl + inc - s;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) { tile[threadIdx.x * SCAN_ITEMS + k] = run; run += loc[k]; }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    const int li = k * SCAN_THREADS + threadIdx.x;
    const long idx = base + li;
    if (idx <= j.n) j.out[idx] = (int)tile[li];
  }
  if (threadIdx.x == 0 && j.n >= base && j.n < base + SCAN_CHUNK) *j.total = excl + tot;
}

long fgd_scan_tiles(long n) { if (n < 0) n = 0; return (n + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK; }
void fgd_exclusive_scan2(const int *in_a, long n_a, int *out_a, unsigned long long *status_a, unsigned *ticket_a, unsigned long long *total_a,
                         const int *in_b, long n_b, int *out_b, unsigned long long *status_b, unsigned *ticket_b, unsigned long long *total_b,
                         unsigned *err, hipStream_t st)
{
  if (n_a < 0) n_a = 0;
  if (n_b < 0) n_b = 0;
  const long nt = std::max(fgd_scan_tiles(n_a), fgd_scan_tiles(n_b));
  k_scan2<<<dim3((unsigned)nt, 2), SCAN_THREADS, 0, st>>>(FgScanJob{in_a, n_a, out_a, status_a, ticket_a, total_a},
                                                         FgScanJob{in_b, n_b, out_b, status_b, ticket_b, total_b}, err, 2 * nt > 1024 ? 1 : 0);
}

void fgd_exclusive_scan1(const int *in, long n, int *out, unsigned long long *status, unsigned *ticket,
                         unsigned long long *total_dev, unsigned *err, hipStream_t st)
{
  if (n < 0) n = 0;
  const int nt = (int)fgd_scan_tiles(n);
  k_scan1<<<nt, SCAN_THREADS, 0, st>>>(in, n, out, status, nt <= 1024 ? nullptr : ticket, total_dev, err);
}

// ---------------------------------------------------------------------------------------
// per-cell records
// ---------------------------------------------------------------------------------------
// (d_ord_key / d_ord_val: xgrid_device.h)

// body shared by the two kernels below: record of cell s0 + threadIdx.x of `ncells` cells described by `tiles`; the 16 vertex
// doubles are staged so that the block stores its 256 records as one contiguous run (a lane writing its own 128-byte
// record makes sixteen 8-byte stores at a 128-byte stride).  Returns the vertex count (0: no record) and the box.
// cull != null: {max key of lat_max, max of ~key of lat_min} over the destination cells (this rank's band): a cell whose
// latitude range cannot meet the band -- the reference's strict test, create_xgrid.c:1055, would reject every pair -- gets
// nv = 0 and area 0 and nothing else; a block without a live cell skips its vertex records altogether.
// QUADS_ONLY (k_cell_struct2r): a cell that needs the general fix_lon -- a pole vertex, an edge of |dlon| = pi: eight of the
// 884 736 cells of C384 -- gets its latitude box, its corners as read (in its vertex record) and *rare = true; the caller lists it and a wave of k_candidates_rect
// finishes its record (d_finish_rare_cell).  Everything else is then a quadrilateral: four vertices in registers instead of
// the general routine's two 12-element arrays (32 VGPRs of every wave), a four-edge area, and a staging tile of the eight live
// coordinates per cell (vtile is [256 * 9] then, [256 * 17] otherwise), which ARE the cell's record: c is compact (FgCells,
// xgrid_device.h) -- 64 bytes per cell, no lon_min / lon_max.
template <bool QUADS_ONLY = false>
__device__ __forceinline__ int d_cell_record(const FgTile *tiles, int ntiles, int ncells, const FgCells &c, unsigned *err, int s0,
                                             double *vtile, double *box /* lat_min, lat_max, lon_min, lon_max */, int *tile_of,
                                             const unsigned long long *cull = nullptr, double tlon = G_PI, bool *rare = nullptr)
{
  constexpr int VS = QUADS_ONLY ? 9 : 17, NLIVE = QUADS_ONLY ? 8 : 16, CAP = QUADS_ONLY ? 4 : G_FIXCAP;
  const int s = s0 + threadIdx.x;
  double *row = vtile + threadIdx.x * VS;
#pragma unroll
  for (int k = 0; k < NLIVE; k++) row[k] = 0.0;
  int nvert = 0;
  bool listed = false;
  if (s < ncells) {
    int t = 0;
    while (t + 1 < ntiles && s >= tiles[t + 1].cell_off) t++;
    *tile_of = t;
    const FgTile T = tiles[t];
    int loc = s - T.cell_off;
    int i = loc % T.nx, j = loc / T.nx;
    int nxp = T.nx + 1;
    int n0 = j * nxp + i, n1 = n0 + 1, n3 = n0 + nxp, n2 = n3 + 1;
    double x[CAP], y[CAP];
    x[0] = T.lon[n0]; y[0] = T.lat[n0];
    x[1] = T.lon[n1]; y[1] = T.lat[n1];
    x[2] = T.lon[n2]; y[2] = T.lat[n2];
    x[3] = T.lon[n3]; y[3] = T.lat[n3];
    double lmin = y[0], lmax = y[0];
#pragma unroll
    for (int k = 1; k < 4; k++) { if (y[k] < lmin) lmin = y[k]; if (y[k] > lmax) lmax = y[k]; }
    c.lat_min[s] = lmin; c.lat_max[s] = lmax;
    box[0] = lmin; box[1] = lmax;
    if (!(lmin >= -G_HPI - 1.e-6) || !(lmax <= G_HPI + 1.e-6)) atomicOr(err, G_ERRBIT_BADLAT);   // also catches NaN
    bool out_of_band = false;
    if (cull && cull[0]) {
      const double bmax = d_ord_val(cull[0]), bmin = d_ord_val(~cull[1]);
      out_of_band = (lmax <= bmin) || (lmin >= bmax);
    }
    int n = out_of_band ? 0 : d_fix_lon_quad_fast(x, y, tlon);
    if constexpr (!QUADS_ONLY) {
      if (n < 0) n = d_fix_lon(x, y, 4, tlon);           // cells with a pole vertex / a half-turn edge: the general routine
    }
    if (out_of_band) { c.nv[s] = 0; c.area[s] = 0; }
    else if (QUADS_ONLY && n < 0) {                      // (the caller's list: the rest of the record comes from k_candidates_rect,
      listed = true;                                     //  which finds the cell's corners, untouched, where its vertices will be)
#pragma unroll
      for (int k = 0; k < 4; k++) { row[k] = x[k]; row[4 + k] = y[k]; }
    }
    else if (n < 0 || n > G_MAXV) {
      atomicOr(err, G_ERRBIT_MAXV);
      c.nv[s] = 0; c.lon_avg[s] = 0; c.area[s] = 0;
      if constexpr (!QUADS_ONLY) { c.lon_min[s] = 0; c.lon_max[s] = 0; }
    } else if constexpr (QUADS_ONLY) {                   // n = 4: the same operations in the same order as below
      double xmin = x[0], xmax = x[0], xs = 0;
#pragma unroll
      for (int k = 1; k < 4; k++) { if (x[k] < xmin) xmin = x[k]; if (x[k] > xmax) xmax = x[k]; }
#pragma unroll
      for (int k = 0; k < 4; k++) xs += x[k];
      xs /= 4;
      c.lon_avg[s] = xs;                                 // (lon_min / lon_max: not kept for compact cells)
      box[2] = xmin; box[3] = xmax; box[4] = xs;
      c.nv[s] = 4;
      nvert = 4;
#pragma unroll
      for (int k = 0; k < 4; k++) { row[k] = x[k]; row[4 + k] = y[k]; }
      c.area[s] = d_poly_area<1>(x, y, 4);
    } else {
      double xmin = x[0], xmax = x[0], xs = 0;
      for (int k = 1; k < n; k++) { if (x[k] < xmin) xmin = x[k]; if (x[k] > xmax) xmax = x[k]; }
      for (int k = 0; k < n; k++) xs += x[k];
      xs /= n;
      c.lon_min[s] = xmin; c.lon_max[s] = xmax; c.lon_avg[s] = xs;
      box[2] = xmin; box[3] = xmax; box[4] = xs;
      c.nv[s] = n;
      nvert = n;
      for (int k = 0; k < G_MAXV; k++) {
        row[k] = (k < n) ? x[k] : 0.0;
        row[8 + k] = (k < n) ? y[k] : 0.0;
      }
      c.area[s] = d_poly_area<1>(x, y, n);
    }
  }
  if (QUADS_ONLY) *rare = listed;
  // no live cell in this block: no vertex records to store (a listed cell is live: its block stores, as it did before)
  if (!__syncthreads_or(nvert != 0 || listed) && cull) return 0;
  const long cnt = (long)min(256, ncells - s0) * NLIVE;
  double *out = QUADS_ONLY ? d_cell_quad(c, s0) : c.verts + (size_t)s0 * 16;
#pragma unroll
  for (int q = 0; q < NLIVE; q++) {
    const long e = (long)q * 256 + threadIdx.x;
    if (e < cnt) out[e] = vtile[(e / NLIVE) * VS + (e % NLIVE)];
  }
  return nvert;
}

// The rest of the record of a cell k_cell_struct2r listed (d_cell_record<true>): the general fix_lon and, from its vertices, what
// d_cell_record stores -- the same routines on the same inputs.  Every lane of the wave computes the same values, lane 0 stores.
// c is compact: a cell that ends with at most four vertices keeps its own 64-byte record (zeros beyond the last vertex); one with
// more gets slot h of c.wide -- h = its place in rare_list -- and h in the first word of its record.  No slot left (more such
// cells than c.wide_cap: no grid has them): the cell gets no record (nv = 0, so no pairs: the attempt runs to its end like any
// other, every kernel on what its predecessors wrote) and G_ERRBIT_WIDECAP, at which the host repeats the search on the generic path.
// Returns the vertex count (0: no record) and the box.
__device__ __forceinline__ int d_finish_rare_cell(const FgCells &c, unsigned *err, int s, int h, int lane, double *box)
{
  double *v = d_cell_quad(c, s);
  double x[G_FIXCAP], y[G_FIXCAP];
#pragma unroll
  for (int k = 0; k < 4; k++) { x[k] = v[k]; y[k] = v[4 + k]; }      // the corners as the record kernel read them: one round of loads
  double lmin = y[0], lmax = y[0];
#pragma unroll
  for (int k = 1; k < 4; k++) { if (y[k] < lmin) lmin = y[k]; if (y[k] > lmax) lmax = y[k]; }
  box[0] = lmin; box[1] = lmax;                          // (stored, and checked for G_ERRBIT_BADLAT, by the record kernel)
  const int n = d_fix_lon(x, y, 4, G_PI);
  if (n < 0 || n > G_MAXV || (n > 4 && h >= c.wide_cap)) {
    if (lane == 0) {
      atomicOr(err, (n < 0 || n > G_MAXV) ? G_ERRBIT_MAXV : G_ERRBIT_WIDECAP);
      c.nv[s] = 0; c.lon_avg[s] = 0; c.area[s] = 0;
      for (int k = 0; k < FG_VSTRIDE_QUAD; k++) v[k] = 0.0;
    }
    return 0;
  }
  double xmin = x[0], xmax = x[0], xs = 0;
  for (int k = 1; k < n; k++) { if (x[k] < xmin) xmin = x[k]; if (x[k] > xmax) xmax = x[k]; }
  for (int k = 0; k < n; k++) xs += x[k];
  xs /= n;
  box[2] = xmin; box[3] = xmax; box[4] = xs;
  const double area = d_poly_area<1>(x, y, n);
  if (lane == 0) {
    c.lon_avg[s] = xs;
    c.nv[s] = n;
    if (n > 4) {
      double *w = c.wide + (size_t)h * 16;
      for (int k = 0; k < G_MAXV; k++) {
        w[k] = (k < n) ? x[k] : 0.0;
        w[8 + k] = (k < n) ? y[k] : 0.0;
      }
      *(int *)v = h;                                     // (nothing else reads the record of a cell with nv > 4)
    } else
      for (int k = 0; k < 4; k++) {
        v[k] = (k < n) ? x[k] : 0.0;
        v[4 + k] = (k < n) ? y[k] : 0.0;
      }
    c.area[s] = area;
  }
  return n;
}

__global__ __launch_bounds__(256) void k_cell_struct(const FgTile *tiles, int ntiles, int ncells, FgCells c, unsigned *err)
{
  __shared__ double vtile[256 * 17];
  d_load_trig_table();
  double box[5]; int tl = 0;
  (void)d_cell_record(tiles, ntiles, ncells, c, err, blockIdx.x * 256, vtile, box, &tl);
}

// ---------------------------------------------------------------------------------------
// binning of destination cells
// ---------------------------------------------------------------------------------------
// Uniform bins over latitude x (longitude mod 2pi), sized ~1.5x the mean destination cell.
// A destination cell whose bounding box covers at most 2x2 bins ("regular") is stored ONCE, in
// the bin of its (lat_min, lon_min) corner; a source cell therefore finds every regular cell
// that can overlap it by scanning rows [r0-1, r1] x columns [c0-1, c1] of its own box -- and
// because bins of one row are adjacent in the table, that is at most two contiguous entry
// ranges per row.  Cells with a larger footprint (pole caps of a cubed-sphere target, ...) go to
// a per-latitude-row "wide" list that every source cell of that row tests.
// Margins of 1e-9 rad make the scan a superset of the pairs that pass the reference's tests,
// including its +-2pi shifts (create_xgrid.c:1064-1074); see DESIGN.md §3.2.
__device__ __forceinline__ void d_cell_box(double lat_min, double lat_max, double lon_min, double lon_max, FgBins b,
                                           int *r0, int *r1, long long *l0, long long *l1)
{
  const double eps = 1.e-9;
  int a0 = (int)floor((lat_min - eps + G_HPI) * b.inv_wlat);
  int a1 = (int)floor((lat_max + eps + G_HPI) * b.inv_wlat);
  *r0 = max(0, min(b.nblat - 1, a0));
  *r1 = max(0, min(b.nblat - 1, a1));
  *l0 = (long long)floor((lon_min - eps) * b.inv_wlon);
  *l1 = (long long)floor((lon_max + eps) * b.inv_wlon);
}
__device__ __forceinline__ int d_colmod(long long l, int nb) { return (int)(((l % nb) + nb) % nb); }

// one atomic per run of consecutive lanes that target the same slot (key >= 0; lanes with key < 0 sit out): returns this
// lane's position in the slot.  Consecutive cells of a regular grid share a bin (2.25 cells per bin), and same-address
// atomics that return a value are the expensive part of the fill pass.
__device__ __forceinline__ int d_slot_position(int *slot_cnt, int key)
{
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(key, 1);
  const bool head = (lane == 0) || (key != prev);
  const unsigned long long heads = __ballot(head);
  const int start = 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));
  const unsigned long long above = (start == 63) ? 0ull : (heads & ~((2ull << start) - 1ull));
  const int end = above ? (__ffsll((long long)above) - 1) : 64;
  int base = 0;
  if (lane == start && key >= 0) base = atomicAdd(&slot_cnt[key], end - start);
  base = __shfl(base, start);
  return base + (lane - start);
}

#define BIN_COPIES 16      // columns a cell may cover and still live in the bins (one copy per column but the last)
#define BIN_ROW_COPIES 4   // rows, likewise
static_assert(BIN_COPIES >= 1 && BIN_COPIES <= 16, "a bin record keeps the copy number and copies - 1 in four bits each");

// Is this bin record the first copy of its cell inside the query's window of rows [ra, rb] x columns [c_start, c_start + count)?
// Columns: p = the record's place in the window taken round the ring of nblon columns, o = the copy's number, flen = copies of the
// cell.  A copy o >= 1 has its predecessor one column earlier -- inside the window unless p == 0; copy 0 is preceded by a later
// copy only if the cell's run of columns passes the window's start going round the ring (p + flen > nblon).  Rows do not wrap: a
// copy that is not its cell's first has its predecessor one row earlier, inside the window unless this is the window's first row.
// Single-copy records always pass.
__device__ __forceinline__ bool d_copy_first(int word, int c_start, int nblon, bool first_row)
{
  const int col = word & 0xffff, o = (word >> 16) & 15, flen = ((word >> 20) & 15) + 1;
  if (((word >> 24) & 1) && !first_row) return false;
  int p = col - c_start;
  if (p < 0) p += nblon;
  return p == 0 || (o == 0 && p + flen <= nblon);
}

// Count (FILL = false) or store (FILL = true) destination cell d in its bin / wide lists.  Wave-wide: every lane of the
// wave must call it (live = false for lanes without a cell).
template <bool FILL>
__device__ __forceinline__ void d_bin_insert(bool live, int d, double lat_min, double lat_max, double lon_min, double lon_max, double lon_avg,
                                             FgBins b, int *slot_cnt, const int *slot_start, FgBinEntry *entries, int cap)
{
  FgBinEntry E;
  int r0 = 0, r1 = 0; long long l0 = 0, l1 = 0;
  if (live) {
    E.lat_min = lat_min; E.lat_max = lat_max; E.lon_min = lon_min; E.lon_max = lon_max; E.lon_avg = lon_avg;
    E.d = d;
    d_cell_box(lat_min, lat_max, lon_min, lon_max, b, &r0, &r1, &l0, &l1);
    E.row0 = r0;
  }
  const int nbins = b.nblat * b.nblon;
  // A cell whose box covers rows r0..r1 and columns l0..l1 is stored at rows r0 .. r1 - 1 x columns l0 .. l1 - 1 (at least one of
  // each): with r1 - r0 <= 1 and l1 - l0 <= 1 that is the single record described above; cells that are "long" -- the rings of a
  // cubed-sphere tile around its pole (up to BIN_COPIES columns), its cells along the diagonals, which lie at 45 degrees to the bin rows
  // (up to BIN_ROW_COPIES + 1 rows) -- get one copy per row and column, and a query takes the FIRST copy its window meets (d_copy_first).  Before round 3
  // such cells went to the wide lists, which every source cell of the row scans whatever its longitude (0.25 deg -> C384 polar tile:
  // 21 k wide cells, 188 k source cells listed for the wave-per-cell path, 2.1 ms against 0.7 ms for an equatorial tile).
  const int maxcopies = (b.nblon <= 0xffff) ? min(BIN_COPIES, b.nblon) : 1, maxrows_c = (b.nblon <= 0xffff) ? BIN_ROW_COPIES : 1;
  const bool regular = live && r1 - r0 <= maxrows_c && l1 - l0 <= maxcopies;
  const int ccopies = regular ? max(1, (int)(l1 - l0)) : 0, rcopies = regular ? max(1, r1 - r0) : 0;
  const int ncopies = ccopies * rcopies;
  int maxc = ncopies;
#pragma unroll
  for (int o = 32; o; o >>= 1) maxc = max(maxc, __shfl_xor(maxc, o));
  for (int k = 0; k < maxc; k++) {
    const bool on = k < ncopies;
    const int kr = on ? k / ccopies : 0, kc = on ? k - kr * ccopies : 0;
    const int col = on ? d_colmod(l0 + kc, b.nblon) : 0;
    const int slot = on ? (r0 + kr) * b.nblon + col : -1;
    if (FILL) {
      const int pos = d_slot_position(slot_cnt, slot);
      if (on) {
        const int at = slot_start[slot] + pos;
        // bin records: column, column-copy number, column copies - 1, "not the first row copy" (wide records: first row)
        E.row0 = (col & 0xffff) | (kc << 16) | ((ccopies - 1) << 20) | ((kr > 0) << 24);
        if ((unsigned)at < (unsigned)cap) entries[at] = E;
      }
    } else if (on)
      atomicAdd(&slot_cnt[slot], 1);
  }
  E.row0 = r0;
  // wide cells go into the per-row lists of every row they span.  Neighbouring cells of a grid row span the same rows, so a
  // whole wave often targets one list: the rows are walked in lockstep and each step takes one atomic per run of equal lists
  // (the great-circle search, whose cap-derived boxes are wide near the poles, spent 0.45 ms here on same-address atomics).
  const int nrows = (live && !regular) ? (r1 - r0 + 1) : 0;
  int maxrows = nrows;
#pragma unroll
  for (int o = 32; o; o >>= 1) maxrows = max(maxrows, __shfl_xor(maxrows, o));
  for (int it = 0; it < maxrows; it++) {
    const int key = (it < nrows) ? nbins + r0 + it : -1;
    const int pos = d_slot_position(slot_cnt, key);
    if (FILL && key >= 0) { const int at = slot_start[key] + pos; if ((unsigned)at < (unsigned)cap) entries[at] = E; }
  }
}

// Source tiles (blocks [0, nbS)) and the destination tile (the rest) in one launch.  Source blocks also store the index of
// each cell inside one level of the field array (order 1: no halo, index == s; order 2: 1-cell halo per tile,
// fregrid_util.c:2137-2145); destination blocks count their cells into the bins; block 0 stores the tile descriptors.
__global__ __launch_bounds__(256) void k_cell_struct2(FgTileSet ts, const FgTile *tiles_in, FgTile *tiles_out, int ntiles, int nsrc, int ndst,
                                                       int nbS, FgCells S, FgCells D, FgBins b, int *slot_cnt, int order, int *src_idx_f,
                                                       double *sums, unsigned *err, unsigned long long *band_keys, int cull, double dst_tlon)
{
  __shared__ double vtile[256 * 17];
  __shared__ FgTile sh_tiles[FG_TILESET_MAX];
  if (ts.n && (int)threadIdx.x < ts.n) sh_tiles[threadIdx.x] = ts.t[threadIdx.x];
  const bool isD = (int)blockIdx.x >= nbS;
  if (cull && !isD && band_keys[0]) {
    // a rank of a banded job: most source blocks lie wholly outside the band -- find that out from the corner latitudes alone
    // and leave before the trig table is loaded (nv = 0 is all the later kernels look at)
    __syncthreads();
    const FgTile *tl0 = ts.n ? sh_tiles : tiles_in;
    const int s = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    int idx_f = s;                                        // the cell's place in the field arrays: the sweep's record merge reads it for EVERY cell
    if (s < nsrc) {
      int t = 0;
      while (t + 1 < ntiles && s >= tl0[t + 1].cell_off) t++;
      const int loc = s - tl0[t].cell_off, i = loc % tl0[t].nx, j = loc / tl0[t].nx, nxp = tl0[t].nx + 1;
      if (order == 2) {
        int foff = 0;
        for (int m = 0; m < t; m++) foff += (tl0[m].nx + 2) * (tl0[m].ny + 2);
        idx_f = foff + (j + 1) * (tl0[t].nx + 2) + i + 1;
      }
      const int n0 = j * nxp + i;
      const double y0 = tl0[t].lat[n0], y1 = tl0[t].lat[n0 + 1], y2 = tl0[t].lat[n0 + nxp + 1], y3 = tl0[t].lat[n0 + nxp];
      const double lmin = fmin(fmin(y0, y1), fmin(y2, y3)), lmax = fmax(fmax(y0, y1), fmax(y2, y3));
      const double bmax = d_ord_val(band_keys[0]), bmin = d_ord_val(~band_keys[1]);
      keep = !((lmax <= bmin) || (lmin >= bmax)) || !(lmin == lmin);        // NaN goes on to the full path (it reports the error)
    }
    if (!__syncthreads_or(keep)) {
      if (s < nsrc) {
        S.nv[s] = 0; S.area[s] = 0;
        if (src_idx_f) src_idx_f[s] = idx_f;
        if (sums) { sums[s] = 0.0; sums[nsrc + s] = 0.0; sums[2 * (size_t)nsrc + s] = 0.0; }
      }
      if (ts.n && blockIdx.x == 0 && (int)threadIdx.x < ts.n) tiles_out[threadIdx.x] = sh_tiles[threadIdx.x];
      return;
    }
  }
  d_load_trig_table();                                   // (barrier inside)
  const FgTile *tiles = ts.n ? sh_tiles : tiles_in;
  if (ts.n && blockIdx.x == 0 && (int)threadIdx.x < ts.n) tiles_out[threadIdx.x] = sh_tiles[threadIdx.x];
  double box[5] = {0, 0, 0, 0, 0};
  int tl = 0;
  if (!isD) {
    const int s0 = blockIdx.x * 256, s = s0 + threadIdx.x;
    (void)d_cell_record(tiles, ntiles, nsrc, S, err, s0, vtile, box, &tl, cull ? band_keys : nullptr);
    if (s < nsrc && sums) { sums[s] = 0.0; sums[nsrc + s] = 0.0; sums[2 * (size_t)nsrc + s] = 0.0; }   // k_compact visits cells with exchange cells only
    if (s < nsrc && src_idx_f) {
      if (order != 2) src_idx_f[s] = s;
      else {
        int foff = 0;
        for (int t = 0; t < tl; t++) foff += (tiles[t].nx + 2) * (tiles[t].ny + 2);
        const int loc = s - tiles[tl].cell_off, i = loc % tiles[tl].nx, j = loc / tiles[tl].nx;
        src_idx_f[s] = foff + (j + 1) * (tiles[tl].nx + 2) + i + 1;
      }
    }
  } else {
    const int d0 = ((int)blockIdx.x - nbS) * 256, d = d0 + threadIdx.x;
    const int nv = d_cell_record(tiles + ntiles, 1, ndst, D, err, d0, vtile, box, &tl, nullptr, dst_tlon);
    d_bin_insert<false>(d < ndst && nv != 0, d, box[0], box[1], box[2], box[3], box[4], b, slot_cnt, nullptr, nullptr, 0);
    if (band_keys && cull != 2) {                       // latitude range of the destination cells, for the culling of a later launch
      // one pair of atomics per BLOCK, and only when it would change the value: thousands of same-address atomics serialise
      // at ~12 ns each (a wave-level version of this cost the kernel 0.37 ms)
      __shared__ unsigned long long sh_k[2][4];
      unsigned long long kmax = (d < ndst && nv != 0) ? d_ord_key(box[1]) : 0ull, kmin = (d < ndst && nv != 0) ? ~d_ord_key(box[0]) : 0ull;
#pragma unroll
      for (int o = 32; o; o >>= 1) { kmax = max(kmax, __shfl_xor(kmax, o)); kmin = max(kmin, __shfl_xor(kmin, o)); }
      if ((threadIdx.x & 63) == 0) { sh_k[0][threadIdx.x >> 6] = kmax; sh_k[1][threadIdx.x >> 6] = kmin; }
      __syncthreads();
      if (threadIdx.x == 0) {
        kmax = max(max(sh_k[0][0], sh_k[0][1]), max(sh_k[0][2], sh_k[0][3]));
        kmin = max(max(sh_k[1][0], sh_k[1][1]), max(sh_k[1][2], sh_k[1][3]));
        if (kmax > __hip_atomic_load(&band_keys[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&band_keys[0], kmax);
        if (kmin > __hip_atomic_load(&band_keys[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&band_keys[1], kmin);
      }
    }
  }
}

// latitude range of the destination grid from its corner array alone (= the range over its cells' lat_min / lat_max): lets the
// culling search keep the ONE fused record launch instead of a destination launch followed by a source launch
__global__ __launch_bounds__(256) void k_band_keys(const double *lat, long n, unsigned long long *band_keys)
{
  __shared__ unsigned long long sh_k[2][4];
  unsigned long long kmax = 0ull, kmin = 0ull;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const unsigned long long k = d_ord_key(lat[i]);
    kmax = max(kmax, k); kmin = max(kmin, ~k);
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) { kmax = max(kmax, __shfl_xor(kmax, o)); kmin = max(kmin, __shfl_xor(kmin, o)); }
  if ((threadIdx.x & 63) == 0) { sh_k[0][threadIdx.x >> 6] = kmax; sh_k[1][threadIdx.x >> 6] = kmin; }
  __syncthreads();
  if (threadIdx.x == 0) {
    kmax = max(max(sh_k[0][0], sh_k[0][1]), max(sh_k[0][2], sh_k[0][3]));
    kmin = max(max(sh_k[1][0], sh_k[1][1]), max(sh_k[1][2], sh_k[1][3]));
    atomicMax(&band_keys[0], kmax);
    atomicMax(&band_keys[1], kmin);
  }
}
void fgd_band_keys(const double *lat, long n, unsigned long long *band_keys, hipStream_t st)
{
  if (n > 0) k_band_keys<<<(int)min(64L, (n + 2047) / 2048), 256, 0, st>>>(lat, n, band_keys);
}

// stand-alone bin count for searches whose cell records come from another kernel (great circle)
__global__ __launch_bounds__(256) void k_bin_count(int ncells, FgCells c, FgBins b, int *slot_cnt)
{
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = d < ncells && c.nv[d] != 0;      // (no early return: the slot positions are a wave-wide operation)
  double v[5] = {0, 0, 0, 0, 0};
  if (live) { v[0] = c.lat_min[d]; v[1] = c.lat_max[d]; v[2] = c.lon_min[d]; v[3] = c.lon_max[d]; v[4] = c.lon_avg[d]; }
  d_bin_insert<false>(live, d, v[0], v[1], v[2], v[3], v[4], b, slot_cnt, nullptr, nullptr, 0);
}

// ---------------------------------------------------------------------------------------
// candidate pairs
// ---------------------------------------------------------------------------------------
struct SrcQuery {
  int ra, rb;          // rows holding regular cells that may overlap: [max(0, r0-1), r1]
  int r0, r1;          // the source cell's own rows (wide lists)
  int c_start, n0, n1; // columns [c_start, c_start+n0) and, wrapped, [0, n1)
};

__device__ __forceinline__ SrcQuery d_src_query(double lat_min, double lat_max, double lon_min, double lon_max, FgBins b)
{
  SrcQuery q;
  long long l0, l1;
  d_cell_box(lat_min, lat_max, lon_min, lon_max, b, &q.r0, &q.r1, &l0, &l1);
  q.ra = max(0, q.r0 - 1); q.rb = q.r1;
  long long count = (l1 - l0 + 1) + 1;
  if (count >= b.nblon) { q.c_start = 0; q.n0 = b.nblon; q.n1 = 0; }
  else {
    q.c_start = d_colmod(l0 - 1, b.nblon);
    q.n0 = (int)min((long long)(b.nblon - q.c_start), count);
    q.n1 = (int)count - q.n0;
  }
  return q;
}

// size of the query: bins scanned (a bin holds ~2 cells: bins are 1.25x the mean cell) plus the entries of
// the wide lists of its rows (two table loads).  Only used to route huge queries to the wave-per-cell path.
__device__ __forceinline__ int d_query_size(const SrcQuery &q, FgBins b, const int *slot_start)
{
  const int nbins = b.nblat * b.nblon;
  return (q.rb - q.ra + 1) * (q.n0 + q.n1) + (slot_start[nbins + q.r1 + 1] - slot_start[nbins + q.r0]);
}

// the reference's two bounding-box rejects, create_xgrid.c:1055 and :1062-1079
__device__ __forceinline__ bool d_box_pass(const FgBinEntry &E, double lat_in_min, double lat_in_max,
                                           double lon_in_min, double lon_in_max, double lon_in_avg)
{
  if (E.lat_min >= lat_in_max || E.lat_max <= lat_in_min) return false;
  double lon_out_min = E.lon_min, lon_out_max = E.lon_max;
  double dx = E.lon_avg - lon_in_avg;
  if (dx < -G_PI)     { lon_out_min += G_TPI; lon_out_max += G_TPI; }
  else if (dx > G_PI) { lon_out_min -= G_TPI; lon_out_max -= G_TPI; }
  if (lon_out_min >= lon_in_max || lon_out_max <= lon_in_min) return false;
  return true;
}

#define HEAVY_ENTRIES 32      // scanned bins + wide entries above which a source cell gets a whole wave (measured: 16 / 24 / 32 / 64 / 128
                              // give 0.31 / 0.27 / 0.28 / 0.305 / 0.38 ms for the candidate phase at C384 -> 0.25 deg; the lanes with the
                              // longest scans set the duration of the four-lanes-per-cell path)
#define CAND_G 4          // lanes per source cell in the candidate scan (one bin row each)
#define CP_SMALL 128      // pairs per cell up to which the lanes of k_compact rank by comparison; cells with more are "big"
                          // (32 until round 3: every cell of a coarse -> fine remap -- ~100 pairs at C48 -> 0.25 deg -- then took a whole
                          // block of the big-cell role: compaction 0.31 ms of a 0.83 ms search; 128: 0.17 of 0.67; 256: 0.14, but the
                          // 256 halo lanes of every lane-per-pair block then cost the similar-resolution case 2 %)
#define CAND_CHUNK 1     // consecutive waves (of 16 cells) that append to the same region: 1 = round robin, the best balance
                          // (16 was tried for the locality of the clip: no faster, and the great-circle search, whose pairs
                          // pile up around the poles, then overflowed a region and had to be repeated)
#define HEAVY_BLOCKS 2048 // waves serving the listed cells, appended to the grid of the four-lanes-per-cell blocks

__device__ __forceinline__ bool d_src_active(const FgCells &S, const double *mask, int s)
{
  bool active = S.nv[s] > 0;
  if (active && mask) active = mask[s] > 0.5;          // MASK_THRESH, create_xgrid.c:1030
  return active;
}

// Bin fill (blocks [0, nbD): destination cells -> their bin records) and, in the same launch, the list of the source cells
// whose query touches more than HEAVY_ENTRIES table entries (blocks [nbD, ...): one atomic per wave that has any).
__global__ __launch_bounds__(256) void k_bin_fill(int ndst, int nbD, FgCells D, FgBins b, int *slot_fill, const int *slot_start,
                                                   FgBinEntry *entries, int cap, int nsrc, FgCells S, const double *mask,
                                                   int *heavy_list, int *heavy_cnt)
{
  if ((int)blockIdx.x < nbD) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    const bool live = d < ndst && D.nv[d] != 0;
    double v[5] = {0, 0, 0, 0, 0};
    if (live) { v[0] = D.lat_min[d]; v[1] = D.lat_max[d]; v[2] = D.lon_min[d]; v[3] = D.lon_max[d]; v[4] = D.lon_avg[d]; }
    d_bin_insert<true>(live, d, v[0], v[1], v[2], v[3], v[4], b, slot_fill, slot_start, entries, cap);
    return;
  }
  const int s = ((int)blockIdx.x - nbD) * 256 + threadIdx.x, lane = threadIdx.x & 63;
  bool heavy = false;
  if (s < nsrc && d_src_active(S, mask, s)) {
    const SrcQuery q = d_src_query(S.lat_min[s], S.lat_max[s], S.lon_min[s], S.lon_max[s], b);
    heavy = d_query_size(q, b, slot_start) > HEAVY_ENTRIES;
  }
  const unsigned long long m = __ballot(heavy);
  if (m) {
    int base = 0;
    if (lane == 0) base = atomicAdd(heavy_cnt, __popcll(m));
    base = __shfl(base, 0);
    if (heavy) heavy_list[base + __popcll(m & ((1ull << lane) - 1ull))] = s;
  }
}

// One wave per listed source cell (pole caps of the source grid: their longitude range covers hundreds of bins); lanes
// stride the contiguous entry ranges, ballot + popcount compacts.  FILL = false counts, FILL = true writes at most `limit`
// pairs from position wbase on.
template <bool FILL>
__device__ __forceinline__ int d_heavy_scan(const SrcQuery &q, FgBins b, const int *slot_start, const FgBinEntry *entries, int ecap,
                                            double lat_in_min, double lat_in_max, double lon_in_min, double lon_in_max, double lon_in_avg,
                                            int s, int *pair_src, int *pair_dst, int wbase, int limit)
{
  const int lane = threadIdx.x & 63;
  const int nbins = b.nblat * b.nblon;
  int cnt = 0;
  const int nrows_reg = q.rb - q.ra + 1, nrows_wide = q.r1 - q.r0 + 1;
  for (int it = 0; it < 2 * nrows_reg + nrows_wide; it++) {
    int e0, e1, wide_row = -1;
    const bool first_row = it < 2;
    if (it < 2 * nrows_reg) {
      int r = q.ra + (it >> 1), seg = it & 1, base = r * b.nblon;
      if (seg && !q.n1) continue;
      e0 = seg ? slot_start[base] : slot_start[base + q.c_start];
      e1 = seg ? slot_start[base + q.n1] : slot_start[base + q.c_start + q.n0];
    } else {
      wide_row = q.r0 + (it - 2 * nrows_reg);
      e0 = slot_start[nbins + wide_row]; e1 = slot_start[nbins + wide_row + 1];
    }
    e1 = min(e1, ecap);
    for (int eb = e0; eb < e1; eb += 64) {
      int e = eb + lane;
      bool pass = false;
      int dcell = 0;
      if (e < e1) {
        const FgBinEntry E = entries[e];
        dcell = E.d;
        pass = d_box_pass(E, lat_in_min, lat_in_max, lon_in_min, lon_in_max, lon_in_avg);
        if (wide_row >= 0 ? wide_row != max(q.r0, E.row0) : !d_copy_first(E.row0, q.c_start, b.nblon, first_row)) pass = false;
      }
      unsigned long long m = __ballot(pass);
      if (FILL && pass) {
        const int k = cnt + __popcll(m & ((1ull << lane) - 1ull));
        if (k < limit) { pair_src[wbase + k] = s; pair_dst[wbase + k] = dcell; }
      }
      cnt += __popcll(m);
    }
  }
  return cnt;
}

// One lane's share of a source cell's query: every CAND_G-th bin row, the <= 2 contiguous record ranges of each row, then the
// wide lists of its rows.  Records are loaded four at a time ahead of their tests: the loop is a chain of L2 round trips
// otherwise (one per record).  FILL = false counts and keeps the first four hits in ids[]; FILL = true writes the pairs
// (same order) at psrc/pdst[wloc ...] while inside the region.
template <bool FILL>
__device__ __forceinline__ int d_lane_scan(const SrcQuery &q, int sub, FgBins b, const int *slot_start, const FgBinEntry *entries, int ecap,
                                           double lat_in_min, double lat_in_max, double lon_in_min, double lon_in_max, double lon_in_avg,
                                           int *ids, int s, int *psrc, int *pdst, unsigned wloc, unsigned regcap)
{
  const int nbins = b.nblat * b.nblon;
  int cnt = 0;
  auto visit = [&](const FgBinEntry &E, bool ok) {
    if (!ok || !d_box_pass(E, lat_in_min, lat_in_max, lon_in_min, lon_in_max, lon_in_avg)) return;
    if (FILL) { if (wloc + cnt < regcap) { psrc[wloc + cnt] = s; pdst[wloc + cnt] = E.d; } }
    else { ids[0] = cnt == 0 ? E.d : ids[0]; ids[1] = cnt == 1 ? E.d : ids[1]; ids[2] = cnt == 2 ? E.d : ids[2]; ids[3] = cnt == 3 ? E.d : ids[3]; }
    cnt++;
  };
  auto range = [&](int e0, int e1, int wide_row, bool first_row) {
    for (int eb = e0; eb < e1; eb += 4) {
      FgBinEntry E[4];
#pragma unroll
      for (int k = 0; k < 4; k++) E[k] = entries[min(eb + k, e1 - 1)];
#pragma unroll
      for (int k = 0; k < 4; k++)            // a wide cell sits in every row it spans, a long one in every column but its last
        visit(E[k], eb + k < e1 && (wide_row < 0 ? d_copy_first(E[k].row0, q.c_start, b.nblon, first_row) : wide_row == max(q.r0, E[k].row0)));
    }
  };
  for (int r = q.ra + sub; r <= q.rb; r += CAND_G) {
    const int base = r * b.nblon;
    const int a0 = slot_start[base + q.c_start], a1 = slot_start[base + q.c_start + q.n0];
    const int b0 = q.n1 ? slot_start[base] : 0, b1 = q.n1 ? slot_start[base + q.n1] : 0;
    range(a0, min(a1, ecap), -1, r == q.ra);             // a search may have outgrown its record buffer (it is then repeated)
    range(b0, min(b1, ecap), -1, r == q.ra);
  }
  for (int r = q.r0 + sub; r <= q.r1; r += CAND_G) range(slot_start[nbins + r], min(slot_start[nbins + r + 1], ecap), r, false);
  return cnt;
}

// Blocks [0, nbR): CAND_G lanes per source cell, each scanning every CAND_G-th bin row of the cell's query.  A lane keeps
// the first four destination cells it finds (the common case: 5.2 pairs per source cell over four lanes); the wave then adds
// up its lanes' counts, reserves that many entries of its region of the pair list with ONE atomic, and every lane writes its
// pairs -- from registers, or, with more than four, by scanning its rows again (same order).  The pairs of a source cell
// are contiguous: pair_beg / pair_cnt.  Blocks [nbR, nbR + HEAVY_BLOCKS): a wave per listed cell (count, reserve, fill).
// (one wave per block: a block gives its slots back when its slowest wave is done, and the scan lengths vary a lot --
// measured 256 / 128 / 64 threads: 0.240 / 0.230 / 0.224 ms for the old count pass)
// The listed cells come FIRST in the grid: their waves run long and should start with the others, not after them.
__global__ __launch_bounds__(64) void k_candidates1(int nsrc, int H, FgCells S, const double *mask, FgBins b, const int *slot_start,
                                                     const FgBinEntry *entries, int ecap, FgPairSpace ps, int *pair_beg, int *pair_cnt,
                                                     const int *heavy_list, const int *heavy_cnt, int *big_list, int *big_cnt)
{
  const int lane = threadIdx.x;
  if ((int)blockIdx.x < H) {
    const int nheavy = *heavy_cnt;
    for (int h = blockIdx.x; h < nheavy; h += H) {
      const int s = heavy_list[h];
      const double lat_in_min = S.lat_min[s], lat_in_max = S.lat_max[s];
      const double lon_in_min = S.lon_min[s], lon_in_max = S.lon_max[s], lon_in_avg = S.lon_avg[s];
      const SrcQuery q = d_src_query(lat_in_min, lat_in_max, lon_in_min, lon_in_max, b);
      const int cnt = d_heavy_scan<false>(q, b, slot_start, entries, ecap, lat_in_min, lat_in_max, lon_in_min, lon_in_max, lon_in_avg,
                                          s, nullptr, nullptr, 0, 0);
      // region by a hash of the cell number -- not by list position (the list order varies from run to run), and not s % nreg
      // (the cells around a pole share a few residues when the tile width is a multiple of nreg: 20 regions took all their pairs)
      const int r = (int)(((unsigned)s * 2654435761u >> 12) % (unsigned)ps.nreg);
      unsigned base = 0;
      if (lane == 0 && cnt) base = atomicAdd(&ps.fill[r * FG_FILL_STRIDE], (unsigned)cnt);
      base = __shfl(base, 0);
      const int loc0 = (int)min(base, (unsigned)ps.regcap), n_ok = min(cnt, ps.regcap - loc0);
      const int wbase = r * ps.regcap + loc0;
      if (n_ok > 0)
        (void)d_heavy_scan<true>(q, b, slot_start, entries, ecap, lat_in_min, lat_in_max, lon_in_min, lon_in_max, lon_in_avg,
                                 s, ps.src, ps.dst, wbase, n_ok);
      if (lane == 0) { pair_beg[s] = wbase; pair_cnt[s] = n_ok; if (n_ok > CP_SMALL) big_list[atomicAdd(big_cnt, 1)] = s; }
    }
    return;
  }
  const int bR = (int)blockIdx.x - H;                  // block among the four-lanes-per-cell blocks
  const long t = (long)bR * 64 + lane;
  const int s = (int)(t / CAND_G), sub = (int)(t % CAND_G);
  int cnt = 0;
  int ids[4] = {-1, -1, -1, -1};
  bool heavy = false;
  double lat_in_min = 0, lat_in_max = 0, lon_in_min = 0, lon_in_max = 0, lon_in_avg = 0;
  SrcQuery q{};
  // (Issuing the loads of each link of the chain -- cell box, slot offsets, first records of every range -- together, ahead of
  // the branches that may not need them, was measured: 223 us against 165.  The kernel is bound by the number of 48-byte record
  // requests its lanes make, not by their latency, and speculation adds requests.  Staging the UNION of the 16 cells' bin records
  // of a wave in LDS with coalesced loads and testing every cell against all of them there: 195 us -- 2.4x fewer record loads, but
  // 16 x 80 box tests per wave instead of 16 x 12.)
  if (s < nsrc && d_src_active(S, mask, s)) {
    lat_in_min = S.lat_min[s]; lat_in_max = S.lat_max[s];
    lon_in_min = S.lon_min[s]; lon_in_max = S.lon_max[s]; lon_in_avg = S.lon_avg[s];
    q = d_src_query(lat_in_min, lat_in_max, lon_in_min, lon_in_max, b);
    heavy = d_query_size(q, b, slot_start) > HEAVY_ENTRIES;       // listed by k_bin_fill; a whole wave writes its pairs
    if (!heavy)
      cnt = d_lane_scan<false>(q, sub, b, slot_start, entries, ecap, lat_in_min, lat_in_max, lon_in_min, lon_in_max, lon_in_avg,
                               ids, s, nullptr, nullptr, 0u, 0u);
  }
  // the wave's range in its region of the pair list
  const unsigned incl = wave_incl_scan((unsigned)cnt, lane);
  const unsigned total = __shfl(incl, 63);
  const unsigned excl = incl - (unsigned)cnt;
  // region by a hash of the wave's number: plain round robin leaves whole residue classes to the dense cells around a pole when
  // the tile width is a multiple of the region count (the great-circle search then overflowed a region and was repeated)
  const int r = (int)((((unsigned)(bR / CAND_CHUNK)) * 2654435761u >> 12) % (unsigned)ps.nreg);
  unsigned base = 0;
  if (lane == 0 && total) base = atomicAdd(&ps.fill[r * FG_FILL_STRIDE], total);
  base = __shfl(base, 0);
  // per source cell: first pair and number of pairs (entries beyond the region are dropped; the search is then repeated)
  int c4 = cnt;
  c4 += __shfl_xor(c4, 1); c4 += __shfl_xor(c4, 2);
  const unsigned excl0 = __shfl(excl, lane & ~(CAND_G - 1));
  if (sub == 0 && s < nsrc && !heavy) {
    const unsigned first = base + excl0;
    const int loc0 = (int)min(first, (unsigned)ps.regcap);
    pair_beg[s] = r * ps.regcap + loc0;
    pair_cnt[s] = min(c4, ps.regcap - loc0);
  }
  {                                                     // cells for the big-cell blocks of the compaction (rare here)
    const bool bigc = sub == 0 && s < nsrc && !heavy && min(c4, ps.regcap - (int)min(base + excl0, (unsigned)ps.regcap)) > CP_SMALL;
    const unsigned long long bm = __ballot(bigc);
    if (bm) {
      int q = 0;
      if (lane == 0) q = atomicAdd(big_cnt, __popcll(bm));
      q = __shfl(q, 0);
      if (bigc) big_list[q + __popcll(bm & ((1ull << lane) - 1ull))] = s;
    }
  }
  if (cnt == 0) return;
  const unsigned wloc = base + excl;                    // this lane's first entry within the region
  int *psrc = ps.src + (size_t)r * ps.regcap, *pdst = ps.dst + (size_t)r * ps.regcap;
  if (cnt <= 4) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < cnt && wloc + k < (unsigned)ps.regcap) { psrc[wloc + k] = s; pdst[wloc + k] = ids[k]; }
    return;
  }
  (void)d_lane_scan<true>(q, sub, b, slot_start, entries, ecap, lat_in_min, lat_in_max, lon_in_min, lon_in_max, lon_in_avg,
                          ids, s, psrc, pdst, wloc, (unsigned)ps.regcap);
}


// ---------------------------------------------------------------------------------------
// rectilinear destination grid
// ---------------------------------------------------------------------------------------
// lon_out depends on the column only and lat_out on the row only, bit for bit: what get_output_grid_by_size
// (fregrid_util.c:588-654) makes for every --nlon/--nlat target, global or regional, whole or a rank's band.  Then
//   * fix_lon's result for a cell depends on its column only (no lone pole vertex, no |dlon| = pi edge: checked), so a cell is
//     four values of a per-column record + two values of the latitude axis -- no 128-byte vertex record, no per-cell boxes;
//   * the reference's latitude reject (create_xgrid.c:1055) depends on the row only and its longitude reject (:1062-1079) on the
//     column only: the candidates of a source cell are (rows found on the latitude axis) x (columns that pass the exact
//     longitude test), found by index arithmetic -- no bins, no 48-byte record scans -- and come out in ascending destination
//     index, the reference's order.
// k_rect_tables VERIFIES the property on the device (every corner against its axis value, bitwise) in the same stream; every
// later kernel of the rectilinear path leaves at once when the check failed, and the host repeats the search with the generic
// path (plan.hip).  Results are the generic path's, bit for bit (tests/test_gpu_rect.py, scripts/legacy_fuzz.py).
// (RECT_COLW = 8 doubles per column record, xgrid_device.h: x'[0..3] after fix_lon (SW, SE, NE, NW), lon_min, lon_max, lon_avg, width)
#define RECT_HDR 8            // header of the tables: lon[0], nx / (lon[nx] - lon[0]), lat[0], ny / (lat[ny] - lat[0])
#define RECT_EPS 1.e-9
#define RECT_VERIFY_BLOCKS 8192   // blocks of k_rect_tables that verify the corners (2M corners in one round of loads)
#define RECT_HEAVY 48         // rows x window columns above which a source cell's candidates are made by a whole wave

__global__ __launch_bounds__(256) void k_rect_tables(const double *lon, const double *lat, int nx, int ny, double *hdr, double *lat_ax,
                                                      double *lon_ax, double *col, double *col_min, double *col_max, double *col_avg, double *row,
                                                      unsigned *bad, unsigned *err, double dst_tlon)
{
  // Blocks [0, nbT) make the tables, the others verify the corners: the table lanes' sines and fix_lon run beside the pass over the
  // two corner arrays instead of behind their share of it, and that pass is one round of loads per lane where 1024 blocks walked
  // the arrays in four (the launch took 13.8 us for 16.6 MB at 1440 x 720, whatever the table lanes did)
  const int nbT = (max(nx, ny) + 1 + 255) / 256;
  const long np = (long)(nx + 1) * (ny + 1);
  bool b = false;
  if ((int)blockIdx.x >= nbT) {
    // (row, column) of corner e by one 32-bit division per lane, then carried along: a stride of gsz corners is dj rows and di columns
    const long gid = (long)((int)blockIdx.x - nbT) * 256 + threadIdx.x, gsz = (long)((int)gridDim.x - nbT) * 256;
    const int nxp = nx + 1;
    const int dj = (int)(gsz / nxp), di = (int)(gsz - (long)dj * nxp);
    long j = 0; int i = 0;
    if (gid < np) { j = (long)((unsigned)gid / (unsigned)nxp); i = (int)(gid - j * nxp); }   // (gid < RECT_VERIFY_BLOCKS * 256)
    for (long e = gid; e < np; e += gsz) {
      if (__double_as_longlong(lon[e]) != __double_as_longlong(lon[i]) ||
          __double_as_longlong(lat[e]) != __double_as_longlong(lat[j * nxp])) b = true;
      j += dj; i += di;
      if (i >= nxp) { i -= nxp; j++; }
    }
    if (__ballot(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
    return;
  }
  d_load_trig_table();                                   // (barrier inside)
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid <= ny) {
    const double y = lat[gid * (nx + 1)];
    lat_ax[gid] = y;
    if (!(y >= -G_HPI - 1.e-6) || !(y <= G_HPI + 1.e-6)) atomicOr(err, G_ERRBIT_BADLAT);       // (also NaN)
    if (gid < ny && !(lat[(gid + 1) * (nx + 1)] > y)) b = true;                                 // strictly ascending rows
    if (gid > 0 && gid < ny && d_is_pole(y)) b = true;                                          // a pole only as the outer edge of an outer row
    // what d_poly_area evaluates on the cells of row gid (d_rect_area below): the sines of its two flat edges (lat1 == lat2: the
    // mid latitude 0.5 * (y + y) is y) and of its two meridian edges (mid latitude 0.5 * (yb + y), half height 0.5 * (yb - y))
    double *r = row + (size_t)gid * 4;
    r[0] = d_sin_lat(0.5 * (y + y));
    if (gid < ny) {
      const double yb = lat[(gid + 1) * (nx + 1)];
      const bool flat = fabs(yb - y) < G_SMALL;
      const double dy = 0.5 * (yb - y);
      r[1] = d_sin_lat(0.5 * (yb + y)); r[2] = flat ? 1.0 : d_sin_lat(dy) / dy; r[3] = flat ? 1.0 : 0.0;
    } else { r[1] = 0.0; r[2] = 1.0; r[3] = 1.0; }
  }
  if (gid <= nx) lon_ax[gid] = lon[gid];                                                        // (a copy: the caller's array may go away)
  if (gid < nx) {
    const double x0 = lon[gid], x1 = lon[gid + 1];
    if (!(x1 > x0) || !(x1 - x0 < G_PI - 1.e-6)) b = true;                                      // ascending columns narrower than pi
    double x[G_FIXCAP], y[G_FIXCAP];
    x[0] = x0; x[1] = x1; x[2] = x1; x[3] = x0;
    y[0] = 0.0; y[1] = 0.0; y[2] = 0.1; y[3] = 0.1;
    // the quadrilateral routine: same operations in the same order; it declines (-1, nothing modified) only for an edge of
    // |dlon| = pi -- these latitudes are no poles -- and such a column has failed the width check above
    int n = d_fix_lon_quad_fast(x, y, dst_tlon);
    if (n < 0) n = d_fix_lon(x, y, 4, dst_tlon);
    double *c = col + (size_t)gid * RECT_COLW;
    if (n != 4) { b = true; for (int k = 0; k < RECT_COLW; k++) c[k] = 0.0; col_min[gid] = 0.0; col_max[gid] = 0.0; col_avg[gid] = 0.0; }
    else {
      double xmin = x[0], xmax = x[0], xs = 0;                                                  // as in d_cell_record
      for (int k = 1; k < 4; k++) { if (x[k] < xmin) xmin = x[k]; if (x[k] > xmax) xmax = x[k]; }
      for (int k = 0; k < 4; k++) xs += x[k];
      xs /= 4;
      c[0] = x[0]; c[1] = x[1]; c[2] = x[2]; c[3] = x[3]; c[4] = xmin; c[5] = xmax; c[6] = xs; c[7] = x1 - x0;
      col_min[gid] = xmin; col_max[gid] = xmax; col_avg[gid] = xs;                              // c[4..6] again, laid out for d_rect_col_pass
    }
  }
  if (gid == 0) {
    if (!(lon[nx] - lon[0] <= G_TPI + 1.e-9)) b = true;                                         // one turn at most
    hdr[0] = lon[0]; hdr[1] = nx / (lon[nx] - lon[0]); hdr[2] = lat[0]; hdr[3] = ny / (lat[(long)ny * (nx + 1)] - lat[0]);
  }
  if (__ballot(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

// smallest k in [0, n] with ax[k] > v (STRICT) / ax[k] >= v (!STRICT); ax ascending.  (x0, inv): the uniform-axis guess that
// is right for the regular grids this path mostly sees (two loads); a binary search otherwise.
template <bool STRICT>
__device__ __forceinline__ int d_axis_first(const double *ax, int n, double v, double x0, double inv)
{
  const double t = fmin(fmax(floor((v - x0) * inv), -1.0), (double)(n - 1));
  const int g = (int)t;
  auto above = [&](double a) { return STRICT ? a > v : a >= v; };
  const bool lo_ok = (g < 0) || !above(ax[g]);
  const bool hi_ok = (g + 1 >= n) || above(ax[g + 1]);
  if (lo_ok && hi_ok) return g + 1;
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (above(ax[mid])) hi = mid; else lo = mid + 1; }
  return lo;
}

struct RectQuery { int j0, j1; int nw; int wa[3], wb[3]; };   // rows [j0, j1]; nw column windows [wa, wb], disjoint, ascending

__device__ __forceinline__ RectQuery d_rect_query(const FgRect &R, double lat_in_min, double lat_in_max, double lon_in_min, double lon_in_max)
{
  RectQuery q{};
  const double lon0 = R.hdr[0], inv_lon = R.hdr[1], lat0 = R.hdr[2], inv_lat = R.hdr[3];
  // rows that pass create_xgrid.c:1055: lat[j+1] > lat_in_min && lat[j] < lat_in_max
  q.j0 = max(d_axis_first<true>(R.lat_ax, R.ny + 1, lat_in_min, lat0, inv_lat) - 1, 0);
  q.j1 = min(d_axis_first<false>(R.lat_ax, R.ny + 1, lat_in_max, lat0, inv_lat) - 1, R.ny - 1);
  q.nw = 0;
  if (lon_in_max - lon_in_min > G_PI) { q.nw = 1; q.wa[0] = 0; q.wb[0] = R.nx - 1; return q; }   // pole caps: every column is tested
  // a column passes only if its raw interval, moved by a whole number of turns, meets (lon_in_min, lon_in_max): fix_lon moves the
  // cell by 0 / +-2pi, the reference's test by another 0 / +-2pi.  The windows for different turns are disjoint (columns are
  // narrower than pi, the source range is at most pi, the axis spans one turn at most); the exact test decides inside them.
  const double axl = R.lon_ax[0], axh = R.lon_ax[R.nx];
#pragma unroll
  for (int t = 2; t >= -2; t--) {                      // descending shift = ascending columns
    const double T = t * G_TPI;
    const double lo = lon_in_min - RECT_EPS - T, hi = lon_in_max + RECT_EPS - T;
    if (!(axh > lo) || !(axl < hi)) continue;
    const int a = max(d_axis_first<true>(R.lon_ax, R.nx + 1, lo, lon0, inv_lon) - 1, 0);
    const int b = min(d_axis_first<false>(R.lon_ax, R.nx + 1, hi, lon0, inv_lon) - 1, R.nx - 1);
    if (a <= b && q.nw < 3) {                          // (no indexing by q.nw: the windows stay in registers)
      if (q.nw == 0) { q.wa[0] = a; q.wb[0] = b; } else if (q.nw == 1) { q.wa[1] = a; q.wb[1] = b; } else { q.wa[2] = a; q.wb[2] = b; }
      q.nw++;
    }
  }
  return q;
}
__device__ __forceinline__ int d_rect_ncols(const RectQuery &q)
{
  int n = 0;
#pragma unroll
  for (int w = 0; w < 3; w++) if (w < q.nw) n += q.wb[w] - q.wa[w] + 1;
  return n;
}
// "Heavy" = the candidates are made by a whole wave instead of one lane.  Decided from the cell's box and the MEAN axis spacings
// alone (no axis search), by the record kernel that lists such cells and by the candidate kernel that skips them: the two must
// agree, nothing else depends on the estimate (the lane path handles any count, only slowly).
__device__ __forceinline__ bool d_rect_heavy(const FgRect &R, double lat_in_min, double lat_in_max, double lon_in_min, double lon_in_max)
{
  const double nr = (lat_in_max - lat_in_min) * R.hdr[3] + 2.0;
  const double nc = (lon_in_max - lon_in_min > G_PI) ? (double)R.nx : (lon_in_max - lon_in_min) * R.hdr[1] + 2.0;
  return nr * nc > (double)RECT_HEAVY;
}
// column k of the query's concatenated windows
__device__ __forceinline__ int d_rect_col(const RectQuery &q, int k)
{
  int i = q.wa[0] + k;
  const int l0 = q.wb[0] - q.wa[0] + 1;
  if (q.nw > 1 && k >= l0) { i = q.wa[1] + (k - l0); const int l1 = q.wb[1] - q.wa[1] + 1; if (q.nw > 2 && k - l0 >= l1) i = q.wa[2] + (k - l0 - l1); }
  return i;
}
// the reference's longitude reject for column i (create_xgrid.c:1062-1079), from the three plain arrays: lanes that test neighbouring
// columns read neighbouring doubles (the 64-byte column records gave every lane of a load a cache line of its own)
__device__ __forceinline__ bool d_rect_col_pass(const FgRect &R, int i, double lon_in_min, double lon_in_max, double lon_in_avg)
{
  double lon_out_min = R.col_min[i], lon_out_max = R.col_max[i];
  const double dx = R.col_avg[i] - lon_in_avg;
  if (dx < -G_PI)     { lon_out_min += G_TPI; lon_out_max += G_TPI; }
  else if (dx > G_PI) { lon_out_min -= G_TPI; lon_out_max -= G_TPI; }
  return !(lon_out_min >= lon_in_max || lon_out_max <= lon_in_min);
}

// poly_area (mosaic_util.c:417-459, d_poly_area) of the cell in column record c and row record r: the same terms in the same
// order -- edge 0 flat at the row's lower latitude, edge 1 a meridian (lat1 = upper, lat2 = lower), edge 2 flat at the upper
// latitude, edge 3 the other meridian (lat1 = lower, lat2 = upper: dy and sin(dy) change sign together, the mid latitude is the
// same sum) -- with the four sines and the quotient taken from the row table instead of evaluated per cell.
__device__ __forceinline__ double d_rect_area(const double *c, const double *r)
{
  const double s_lo = r[0], s_hi = r[4], s_mid = r[1], dat = r[2];
  const bool flat_m = r[3] != 0.0;
  double area = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    double dx = c[(k + 1) & 3] - c[k];
    if (dx > G_PI)  dx = dx - 2.0 * G_PI;
    if (dx < -G_PI) dx = dx + 2.0 * G_PI;
    if (fabs(dx + G_PI) < G_SMALL || fabs(dx - G_PI) < G_SMALL) { area += G_PI; continue; }
    if (k == 0) area -= dx * s_lo;
    else if (k == 2) area -= dx * s_hi;
    else if (flat_m) area -= dx * s_mid;
    else area -= dx * s_mid * dat;
  }
  if (area < 0) return -area * G_RADIUS * G_RADIUS;
  return area * G_RADIUS * G_RADIUS;
}

// position of the k-th (from 0) set bit of m; k < popcount(m)
__device__ __forceinline__ int d_kth_set_bit(unsigned long long m, unsigned k)
{
  int pos = 0;
#pragma unroll
  for (int w = 32; w; w >>= 1) {
    const unsigned c = (unsigned)__popcll(m & ((1ull << w) - 1ull));
    if (k >= c) { k -= c; m >>= w; pos += w; }
  }
  return pos;
}

// The candidates of one wave of source cells, a lane per cell: called by every thread of the block (barriers inside), by the
// record kernel with the box it has just made and by k_candidates_rect with the stored one.  Per lane: the query, the exact
// column test into a bit mask (cmask, nc), cnt = rows x columns; then the wave scan, ONE atomic on the region counter (the
// region is a hash of the wave's number), pair_beg / pair_cnt, the big-cell list.  The pairs are then written by the whole
// wave: output slot o of the wave's `total` finds its owner lane in the exclusive scan (kept in LDS with the owner's mask and
// windows), t = o - excl[owner] gives the row t / nc and the (t % nc)-th set bit of the owner's mask the column -- two stores
// of 64 consecutive ints per 64 pairs, where a lane writing its own ~5 pairs one by one spread every store over ten lines.
// A cell's pairs stay contiguous, row-major, in ascending destination index.  A lane whose windows hold more than 64 columns
// without being listed as heavy (a stretched axis: d_rect_heavy goes by the MEAN spacing) re-tests and writes its own pairs,
// as every lane did before; its slots are skipped by the others (nc = 0 in LDS).
// Returns whether the cell is heavy (its candidates are made by a wave of k_candidates_rect instead).
// ONE: the wave has a single cell, lane 0's (every lane passes the same s, only lane 0 is active): a cell whose record
// k_candidates_rect has just finished.
#define RECT_WL_WORDS 10             // LDS words per lane: excl, nc, cmask lo / hi, j0, wa0, l0, wa1 - l0, l0 + l1, wa2 - l0 - l1
template <bool ONE = false>
__device__ __forceinline__ bool d_rect_wave_candidates(const FgRect &R, const FgPairSpace &ps, bool active, int s, int nsrc, unsigned wave_no,
                                                       double lat_in_min, double lat_in_max, double lon_in_min, double lon_in_max,
                                                       double lon_in_avg, int *pair_beg, int *pair_cnt, int *big_list, int *big_cnt,
                                                       unsigned *wl /* [64 * RECT_WL_WORDS], this wave's; in other use until the first barrier */,
                                                       int *n_pairs = nullptr /* the lane's pair_cnt (0 for a cell that is heavy or not active) */)
{
  const int lane = threadIdx.x & 63;
  int cnt = 0, nr = 0, nwc = 0, nc = 0;
  unsigned long long cmask = 0ull;
  RectQuery q{};
  bool heavy = false;
  if (active) {
    heavy = d_rect_heavy(R, lat_in_min, lat_in_max, lon_in_min, lon_in_max);   // listed: a whole wave of k_candidates_rect writes its pairs
    if (!heavy) {
      q = d_rect_query(R, lat_in_min, lat_in_max, lon_in_min, lon_in_max);
      nr = max(q.j1 - q.j0 + 1, 0);
      nwc = d_rect_ncols(q);
      if (nr > 0) {
        // the columns that pass, as a bit mask when the windows are narrow enough (the usual case), else only counted here
        for (int k = 0; k < nwc; k++)
          if (d_rect_col_pass(R, d_rect_col(q, k), lon_in_min, lon_in_max, lon_in_avg)) { nc++; if (k < 64) cmask |= 1ull << k; }
      }
      cnt = (int)min((long)nr * nc, 0x3fffffffL);
    }
  }
  const unsigned incl = wave_incl_scan((unsigned)cnt, lane);
  const unsigned total = __shfl(incl, 63);
  const unsigned excl = incl - (unsigned)cnt;
  const int r = (int)((wave_no * 2654435761u >> 12) % (unsigned)ps.nreg);
  unsigned base = 0;
  if (lane == 0 && total) base = atomicAdd(&ps.fill[r * FG_FILL_STRIDE], total);
  base = __shfl(base, 0);
  int n_ok = 0;
  const unsigned first = base + excl;
  if (s < nsrc && !heavy && (!ONE || lane == 0)) {
    const int loc0 = (int)min(first, (unsigned)ps.regcap);
    n_ok = min(cnt, ps.regcap - loc0);
    pair_beg[s] = r * ps.regcap + loc0;
    pair_cnt[s] = n_ok;
  }
  if (n_pairs) *n_pairs = n_ok;
  {
    const bool bigc = n_ok > CP_SMALL;
    const unsigned long long bm = __ballot(bigc);
    if (bm) {
      int qq = 0;
      if (lane == 0) qq = atomicAdd(big_cnt, __popcll(bm));
      qq = __shfl(qq, 0);
      if (bigc) big_list[qq + __popcll(bm & ((1ull << lane) - 1ull))] = s;
    }
  }
  const bool wide = nwc > 64;
  const int l0 = q.nw > 1 ? q.wb[0] - q.wa[0] + 1 : 64, l1 = q.nw > 2 ? q.wb[1] - q.wa[1] + 1 : 64;    // (mask bits are below 64)
  __syncthreads();                                           // the caller's use of the LDS behind wl ends here
  wl[lane] = excl;
  wl[64 + lane] = wide ? 0u : (unsigned)nc;
  wl[2 * 64 + lane] = (unsigned)cmask; wl[3 * 64 + lane] = (unsigned)(cmask >> 32);
  wl[4 * 64 + lane] = (unsigned)q.j0;
  wl[5 * 64 + lane] = (unsigned)q.wa[0]; wl[6 * 64 + lane] = (unsigned)l0;
  wl[7 * 64 + lane] = (unsigned)(q.wa[1] - l0); wl[8 * 64 + lane] = (unsigned)(l0 + l1);
  wl[9 * 64 + lane] = (unsigned)(q.wa[2] - l0 - l1);
  __syncthreads();
  // the wave's slots that lie inside the region: o < lim is the owner's clamp t = o - excl < n_ok
  const unsigned lim = min(total, (unsigned)ps.regcap - min(base, (unsigned)ps.regcap));
  int *wsrc = ps.src + (size_t)r * ps.regcap + base, *wdst = ps.dst + (size_t)r * ps.regcap + base;
  const int s_first = ONE ? s : s - lane;                    // (ONE: the owner L is always lane 0)
  for (unsigned ob = 0; ob < lim; ob += 64) {
    const unsigned o = ob + lane;
    if (o >= lim || base + o >= (unsigned)ps.regcap) continue;   // (the second test repeats, at the store, what lim holds: an attempt with
                                                                 //  regcap = 0, the exactly sized search's first, must not write at all)
    int L = 0;                                               // the last lane whose exclusive prefix is <= o: the one with excl <= o < incl
#pragma unroll
    for (int st = 32; st; st >>= 1) if (wl[L + st] <= o) L += st;
    const unsigned ncL = wl[64 + L];
    if (!ncL) continue;                                      // (a lane that writes its own pairs, below)
    const unsigned t = o - wl[L], jr = t / ncL, kc = t - jr * ncL;
    const int k = d_kth_set_bit((unsigned long long)wl[2 * 64 + L] | ((unsigned long long)wl[3 * 64 + L] << 32), kc);
    const int i = k + (k < (int)wl[6 * 64 + L] ? (int)wl[5 * 64 + L] : k < (int)wl[8 * 64 + L] ? (int)wl[7 * 64 + L] : (int)wl[9 * 64 + L]);
    wsrc[o] = s_first + L;
    wdst[o] = ((int)wl[4 * 64 + L] + (int)jr) * R.nx + i;
  }
  if (wide && n_ok > 0) {
    int *psrc = ps.src + (size_t)r * ps.regcap + first, *pdst = ps.dst + (size_t)r * ps.regcap + first;
    int w = 0;
    for (int j = q.j0; j <= q.j1 && w < n_ok; j++)
      for (int k = 0; k < nwc && w < n_ok; k++) {
        const int i = d_rect_col(q, k);
        if (d_rect_col_pass(R, i, lon_in_min, lon_in_max, lon_in_avg)) { psrc[w] = s; pdst[w] = j * R.nx + i; w++; }
      }
  }
  return heavy;
}

// Rectilinear twin of k_cell_struct2: source blocks make the full records AND, from the box still in registers, the candidates of
// their cells (d_rect_wave_candidates; the cells whose candidates a whole wave will make are listed for k_candidates_rect);
// destination blocks store the cell AREA only.
// The source role is latency-bound (its predecessor: two thirds of its wave cycles not issuing), so its occupancy matters, and
// that was set by code for cells it hardly ever meets: the general fix_lon (127 VGPRs) and a staging tile of all 16 doubles of
// a record (38.9 KB with the tables: four blocks per CU).  The cells that need the general routine are listed (rare_list) and
// finished by k_candidates_rect<true>; the tile holds the eight live coordinates of a quadrilateral.
#define RECORD_WAVES 7      // waves per SIMD: 59 VGPRs; 22.5 KB of LDS per block give seven blocks per CU
__global__ __launch_bounds__(256, RECORD_WAVES) void k_cell_struct2r(FgTileSet ts, const FgTile *tiles_in, FgTile *tiles_out, int ntiles, int nsrc, int ndst,
                                                        int nbS, FgCells S, double *area_out, FgRect R, const double *mask, int order, int *src_idx_f,
                                                        double *sums, unsigned *err, unsigned long long *band_keys, int cull,
                                                        int *heavy_list, int *heavy_cnt, int *rare_list, int *rare_cnt, FgPairSpace ps,
                                                        int *pair_beg, int *pair_cnt, int *big_list, int *big_cnt)
{
  __shared__ double vtile[256 * 9];
  __shared__ FgTile sh_tiles[FG_TILESET_MAX];
  static_assert(64 * RECT_WL_WORDS * sizeof(unsigned) <= 64 * 9 * sizeof(double), "a wave's share of vtile holds its candidate words");
  if (*R.bad) return;
  if (ts.n && (int)threadIdx.x < ts.n) sh_tiles[threadIdx.x] = ts.t[threadIdx.x];
  const bool isD = (int)blockIdx.x >= nbS;
  // the band of a culling search: the latitude axis gives it (rows ascend) -- no reduction over the corner array, no launch for it
  __shared__ unsigned long long sh_band[2];
  if (cull) {
    if (threadIdx.x == 0) { sh_band[0] = d_ord_key(R.lat_ax[R.ny]); sh_band[1] = ~d_ord_key(R.lat_ax[0]); }
    __syncthreads();
    band_keys = sh_band;
  }
  if (cull && !isD && band_keys[0]) {                      // (as in k_cell_struct2: blocks wholly outside the band leave early)
    __syncthreads();
    const FgTile *tl0 = ts.n ? sh_tiles : tiles_in;
    const int s = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    int idx_f = s;
    if (s < nsrc) {
      int t = 0;
      while (t + 1 < ntiles && s >= tl0[t + 1].cell_off) t++;
      const int loc = s - tl0[t].cell_off, i = loc % tl0[t].nx, j = loc / tl0[t].nx, nxp = tl0[t].nx + 1;
      if (order == 2) {
        int foff = 0;
        for (int m = 0; m < t; m++) foff += (tl0[m].nx + 2) * (tl0[m].ny + 2);
        idx_f = foff + (j + 1) * (tl0[t].nx + 2) + i + 1;
      }
      const int n0 = j * nxp + i;
      const double y0 = tl0[t].lat[n0], y1 = tl0[t].lat[n0 + 1], y2 = tl0[t].lat[n0 + nxp + 1], y3 = tl0[t].lat[n0 + nxp];
      const double lmin = fmin(fmin(y0, y1), fmin(y2, y3)), lmax = fmax(fmax(y0, y1), fmax(y2, y3));
      const double bmax = d_ord_val(band_keys[0]), bmin = d_ord_val(~band_keys[1]);
      keep = !((lmax <= bmin) || (lmin >= bmax)) || !(lmin == lmin);
    }
    if (!__syncthreads_or(keep)) {
      if (s < nsrc) {
        S.nv[s] = 0; S.area[s] = 0;
        pair_beg[s] = 0; pair_cnt[s] = 0;                // (no candidates: what the candidate kernel stored for a cell without a record)
        if (src_idx_f) src_idx_f[s] = idx_f;
        if (sums) { sums[s] = 0.0; sums[nsrc + s] = 0.0; sums[2 * (size_t)nsrc + s] = 0.0; }
      }
      if (ts.n && blockIdx.x == 0 && (int)threadIdx.x < ts.n) tiles_out[threadIdx.x] = sh_tiles[threadIdx.x];
      return;
    }
  }
  d_load_trig_table();                                   // (barrier inside)
  const FgTile *tiles = ts.n ? sh_tiles : tiles_in;
  if (ts.n && blockIdx.x == 0 && (int)threadIdx.x < ts.n) tiles_out[threadIdx.x] = sh_tiles[threadIdx.x];
  if (!isD) {
    double box[5] = {0, 0, 0, 0, 0};
    int tl = 0;
    const int s0 = blockIdx.x * 256, s = s0 + threadIdx.x, lane = threadIdx.x & 63;
    bool rare = false;
    const int nv = d_cell_record<true>(tiles, ntiles, nsrc, S, err, s0, vtile, box, &tl, cull ? band_keys : nullptr, G_PI, &rare);
    {
      const unsigned long long m = __ballot(rare);         // the cells whose records k_candidates_rect finishes (hardly ever any)
      if (m) {
        int base = 0;
        if (lane == 0) base = atomicAdd(rare_cnt, __popcll(m));
        base = __shfl(base, 0);
        if (rare) rare_list[base + __popcll(m & ((1ull << lane) - 1ull))] = s;
      }
    }
    if (s < nsrc && src_idx_f) {
      if (order != 2) src_idx_f[s] = s;
      else {
        int foff = 0;
        for (int t = 0; t < tl; t++) foff += (tiles[t].nx + 2) * (tiles[t].ny + 2);
        const int loc = s - tiles[tl].cell_off, i = loc % tiles[tl].nx, j = loc / tiles[tl].nx;
        src_idx_f[s] = foff + (j + 1) * (tiles[tl].nx + 2) + i + 1;
      }
    }
    // the candidates, in the wave's share of vtile (d_cell_record is through with it); wave blockIdx.x * 4 + wave holds the cells
    // [64 * that, + 64), so the region hash is the one of the stand-alone kernel's block numbers
    // (lon_avg stays in a register: while the record code held the general routine's arrays it had to come back from the
    //  record this lane had just stored, a dependent round trip, or cost the kernel a block per CU)
    const bool active = s < nsrc && nv > 0 && (!mask || mask[s] > 0.5);
    int npair = 0;
    const bool heavy = d_rect_wave_candidates(R, ps, active, s, nsrc, (unsigned)(s >> 6), box[0], box[1], box[2], box[3], box[4], pair_beg, pair_cnt,
                                              big_list, big_cnt, (unsigned *)(vtile + (threadIdx.x >> 6) * (64 * 9)), &npair);
    // the sums of a cell that ends here without a pair: every other cell's are stored by k_compact (the lane of its first pair, or
    // the block of a big cell), those of a heavy or listed cell that ends without one by k_candidates_rect
    if (s < nsrc && sums && npair == 0 && !heavy && !rare) { sums[s] = 0.0; sums[nsrc + s] = 0.0; sums[2 * (size_t)nsrc + s] = 0.0; }
    const unsigned long long m = __ballot(heavy);
    if (m) {
      int base = 0;
      if (lane == 0) base = atomicAdd(heavy_cnt, __popcll(m));
      base = __shfl(base, 0);
      if (heavy) heavy_list[base + __popcll(m & ((1ull << lane) - 1ull))] = s;
    }
  } else {
    const int d = ((int)blockIdx.x - nbS) * 256 + threadIdx.x;
    if (d < ndst) {
      const int j = d / R.nx, i = d - j * R.nx;
      area_out[d] = d_rect_area(R.col + (size_t)i * RECT_COLW, R.row + (size_t)j * 4);
    }
  }
}

__global__ __launch_bounds__(256) void k_polylist_records(FgPolyList P, FgCells S, int *src_idx_f, double *sums, FgRect R, int rect,
                                                           int *heavy_list, int *heavy_cnt, unsigned *err)
{
  if (rect && *R.bad) return;
  const int s = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  bool heavy = false;
  if (s < P.npoly) {
    const int n = P.n[s];
    double *v = S.verts + (size_t)s * 16;
    if (n < 3 || n > G_MAXV) {
      if (n > G_MAXV) atomicOr(err, G_ERRBIT_MAXV);
      S.nv[s] = 0; S.area[s] = 0; S.lat_min[s] = 0; S.lat_max[s] = 0; S.lon_min[s] = 0; S.lon_max[s] = 0; S.lon_avg[s] = 0;
      for (int k = 0; k < 16; k++) v[k] = 0.0;
    } else {
      double xmin = 0, xmax = 0, ymin = 0, ymax = 0;
      for (int k = 0; k < G_MAXV; k++) {
        const double x = (k < n) ? P.lon[(size_t)s * G_MAXV + k] : 0.0, y = (k < n) ? P.lat[(size_t)s * G_MAXV + k] : 0.0;
        v[k] = x; v[8 + k] = y;
        if (k == 0) { xmin = xmax = x; ymin = ymax = y; }
        else if (k < n) { xmin = fmin(xmin, x); xmax = fmax(xmax, x); ymin = fmin(ymin, y); ymax = fmax(ymax, y); }
      }
      if (!(ymin >= -G_HPI - 1.e-6) || !(ymax <= G_HPI + 1.e-6)) atomicOr(err, G_ERRBIT_BADLAT);
      S.nv[s] = n; S.area[s] = P.area[s]; S.lon_avg[s] = P.lon_avg[s];
      S.lat_min[s] = ymin; S.lat_max[s] = ymax; S.lon_min[s] = xmin; S.lon_max[s] = xmax;
      if (rect) heavy = d_rect_heavy(R, ymin, ymax, xmin, xmax);
    }
    if (src_idx_f) src_idx_f[s] = s;
    if (sums) { sums[s] = 0.0; sums[P.npoly + s] = 0.0; sums[2 * (size_t)P.npoly + s] = 0.0; }
  }
  if (rect) {
    const unsigned long long m = __ballot(heavy);
    if (m) {
      int base = 0;
      if (lane == 0) base = atomicAdd(heavy_cnt, __popcll(m));
      base = __shfl(base, 0);
      if (heavy) heavy_list[base + __popcll(m & ((1ull << lane) - 1ull))] = s;
    }
  }
}

// the full destination records of a rectilinear plan, for fg_plan_get_cell_struct (tests): what k_cell_struct2 would have stored
__global__ __launch_bounds__(256) void k_rect_materialize(int ndst, FgRect R, FgCells D)
{
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= ndst) return;
  const int j = d / R.nx, i = d - j * R.nx;
  const double *c = R.col + (size_t)i * RECT_COLW;
  const double ya = R.lat_ax[j], yb = R.lat_ax[j + 1];
  D.lat_min[d] = ya; D.lat_max[d] = yb; D.lon_min[d] = c[4]; D.lon_max[d] = c[5]; D.lon_avg[d] = c[6]; D.nv[d] = 4;
  double *v = D.verts + (size_t)d * 16;
  for (int k = 0; k < 16; k++) v[k] = 0.0;
  v[0] = c[0]; v[1] = c[1]; v[2] = c[2]; v[3] = c[3];
  v[8] = ya; v[9] = ya; v[10] = yb; v[11] = yb;
}

// compact source cells spelled out for fg_plan_get_cell_struct (tests): the longitudes of the boxes and the 128-byte records that
// d_cell_record<false> would have stored; zeros beyond nv and for a cell without a record
__global__ __launch_bounds__(256) void k_quad_materialize(int nsrc, FgCells S, double *lon_min, double *lon_max, double *verts)
{
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nsrc) return;
  const int n = min(S.nv[s], G_MAXV);
  double *o = verts + (size_t)s * 16;
  double xmin = 0.0, xmax = 0.0;
  if (n > 0) {
    const FgVerts v = d_cell_verts(S, s, n);
    xmin = v.x[0]; xmax = v.x[0];
    for (int k = 0; k < G_MAXV; k++) {
      const double x = k < n ? v.x[k] : 0.0, y = k < n ? v.y[k] : 0.0;
      if (k > 0 && k < n) { if (x < xmin) xmin = x; if (x > xmax) xmax = x; }
      o[k] = x; o[8 + k] = y;
    }
  } else
    for (int k = 0; k < 16; k++) o[k] = 0.0;
  lon_min[s] = xmin; lon_max[s] = xmax;
}

// The candidates of ONE source cell made by a whole wave (a cell listed as heavy: pole caps, every column): count, reserve, fill.
// zero_sums != null (behind k_cell_struct2r, which left this cell's sums alone): [3][nsrc], zeroed here if the cell ends without a pair
__device__ __forceinline__ void d_rect_cell_candidates(const FgRect &R, const FgPairSpace &ps, int s, int lane, double lat_in_min, double lat_in_max,
                                                       double lon_in_min, double lon_in_max, double lon_in_avg, int *pair_beg, int *pair_cnt,
                                                       int *big_list, int *big_cnt, double *zero_sums = nullptr, int nsrc = 0)
{
  const RectQuery q = d_rect_query(R, lat_in_min, lat_in_max, lon_in_min, lon_in_max);
  const int nwc = d_rect_ncols(q), nr = q.j1 - q.j0 + 1;
  // pass 1: the columns that pass (the same set for every row of the query); pass 2 writes row after row -- the flags are
  // recomputed per 64-column chunk instead of listed (a list in LDS would cost every block of the launch its occupancy)
  int nc = 0;
  for (int kb = 0; kb < nwc; kb += 64) {
    const int k = kb + lane;
    const bool pass = k < nwc && d_rect_col_pass(R, d_rect_col(q, k), lon_in_min, lon_in_max, lon_in_avg);
    nc += __popcll(__ballot(pass));
  }
  const long cnt_l = (long)nr * nc;
  const int cnt = (int)min(cnt_l, 0x7fffffffL);
  const int r = (int)(((unsigned)s * 2654435761u >> 12) % (unsigned)ps.nreg);
  unsigned base = 0;
  if (lane == 0 && cnt) base = atomicAdd(&ps.fill[r * FG_FILL_STRIDE], (unsigned)cnt);
  base = __shfl(base, 0);
  const int loc0 = (int)min(base, (unsigned)ps.regcap), n_ok = min(cnt, ps.regcap - loc0);
  const int wbase = r * ps.regcap + loc0;
  int cbase = 0;
  for (int kb = 0; kb < nwc && n_ok > 0; kb += 64) {
    const int k = kb + lane;
    int i = 0; bool pass = false;
    if (k < nwc) { i = d_rect_col(q, k); pass = d_rect_col_pass(R, i, lon_in_min, lon_in_max, lon_in_avg); }
    const unsigned long long m = __ballot(pass);
    const int at = cbase + __popcll(m & ((1ull << lane) - 1ull));
    if (pass)
      for (int jr = 0; jr < nr; jr++) {
        const long kk = (long)jr * nc + at;
        if (kk < n_ok) { ps.src[wbase + kk] = s; ps.dst[wbase + kk] = (q.j0 + jr) * R.nx + i; }
      }
    cbase += __popcll(m);
  }
  if (lane == 0) { pair_beg[s] = wbase; pair_cnt[s] = n_ok; if (n_ok > CP_SMALL) big_list[atomicAdd(big_cnt, 1)] = s; }
  if (zero_sums && n_ok == 0 && lane < 3) zero_sums[(size_t)lane * nsrc + s] = 0.0;
}

// Candidates on a rectilinear destination grid.  Blocks [0, H): a wave per listed source cell (pole caps: every column);
// blocks [H, ...): one lane per source cell (d_rect_wave_candidates) -- none when the record kernel has made those candidates
// itself (k_cell_struct2r), all of them for a polygon-list source.  Pairs of a cell are contiguous and in ascending destination index.
// FINISH (behind k_cell_struct2r only, which launches no lane-per-cell blocks): the waves also take the cells that kernel
// listed in rare_list, those that need the general fix_lon: a wave finishes the cell's record (d_finish_rare_cell; this needs
// the sine table) and then makes its candidates, as a heavy cell's where d_rect_heavy says so (a pole cell over a fine target)
// and by the lane form with one live lane otherwise (the same cell over a 10-degree target).  A polygon-list plan keeps the
// small kernel without that code.
#define RARE_BLOCKS 64       // one-wave blocks for the cells of rare_list, in front of the H blocks of the heavy list
template <bool FINISH>
__global__ __launch_bounds__(64) void k_candidates_rect(int nsrc, int H, FgCells S, const double *mask, FgRect R, FgPairSpace ps,
                                                         int *pair_beg, int *pair_cnt, const int *heavy_list, const int *heavy_cnt,
                                                         int *big_list, int *big_cnt, const int *rare_list, const int *rare_cnt, unsigned *err,
                                                         double *sums /* FINISH: [3][nsrc] or null; zeroed for a cell of this launch that ends without a pair */)
{
  const int lane = threadIdx.x;
  __shared__ unsigned wl[64 * RECT_WL_WORDS];
  if (FINISH && (int)blockIdx.x < RARE_BLOCKS) d_load_trig_table();   // (barrier inside; ahead of everything the wave waits for)
  const unsigned bad = *R.bad;
  const int nrare = FINISH ? *rare_cnt : 0;
  if (bad) return;
  // FINISH: blocks [0, RARE_BLOCKS) come first and take the cells of rare_list, waves of their own, so that a listed cell -- a
  // chain of dependent loads, the general routine, then as a rule a pole cap's candidates -- does not wait behind the two or
  // three heavy cells of a wave of the other role (it did at first: the launch took 35 us instead of 15 at C384 -> 0.25 deg)
  const int hb = FINISH ? (int)blockIdx.x - RARE_BLOCKS : (int)blockIdx.x;
  if (hb >= 0 && hb < H) {
    const int nheavy = *heavy_cnt;
    for (int h = hb; h < nheavy; h += H) {
      const int s = heavy_list[h];
      double xmin, xmax;
      if constexpr (FINISH) {                              // compact cells: the box's longitudes from the record, as d_cell_record made them
        const double *q = d_cell_quad(S, s);
        const int n = S.nv[s];
        double x[G_MAXV];
#pragma unroll
        for (int k = 0; k < G_MAXV; k++) x[k] = k < 4 ? q[k] : 0.0;     // (asked for with the count: hardly any cell has more than four)
        if (n > 4) {
          const FgVerts v = d_cell_verts(S, s, n);
#pragma unroll
          for (int k = 0; k < G_MAXV; k++) x[k] = v.x[k];
        }
        xmin = x[0]; xmax = x[0];
#pragma unroll
        for (int k = 1; k < G_MAXV; k++) if (k < n) { if (x[k] < xmin) xmin = x[k]; if (x[k] > xmax) xmax = x[k]; }
      } else { xmin = S.lon_min[s]; xmax = S.lon_max[s]; }
      d_rect_cell_candidates(R, ps, s, lane, S.lat_min[s], S.lat_max[s], xmin, xmax, S.lon_avg[s], pair_beg, pair_cnt, big_list, big_cnt,
                             FINISH ? sums : nullptr, nsrc);
    }
    return;
  }
  if constexpr (FINISH) {
    for (int h = blockIdx.x; h < nrare; h += RARE_BLOCKS) {
      const int s = rare_list[h];
      const double mk = mask ? mask[s] : 1.0;              // (with the corners, not behind the record)
      double b[5] = {0, 0, 0, 0, 0};
      const int nv = d_finish_rare_cell(S, err, s, h, lane, b);
      if (!(nv > 0 && mk > 0.5)) {                         // (d_src_active; pair_cnt[s] = 0 from the record kernel)
        if (sums && lane < 3) sums[(size_t)lane * nsrc + s] = 0.0;
        continue;
      }
      if (d_rect_heavy(R, b[0], b[1], b[2], b[3])) d_rect_cell_candidates(R, ps, s, lane, b[0], b[1], b[2], b[3], b[4], pair_beg, pair_cnt, big_list, big_cnt, sums, nsrc);
      else {
        int npair = 0;
        (void)d_rect_wave_candidates<true>(R, ps, lane == 0, s, nsrc, (unsigned)(s >> 6), b[0], b[1], b[2], b[3], b[4], pair_beg, pair_cnt, big_list, big_cnt, wl, &npair);
        npair = __shfl(npair, 0);
        if (sums && npair == 0 && lane < 3) sums[(size_t)lane * nsrc + s] = 0.0;
      }
    }
  } else {
    const int bR = (int)blockIdx.x - H;
    const int s = bR * 64 + lane;
    const bool active = s < nsrc && d_src_active(S, mask, s);
    double b[5] = {0, 0, 0, 0, 0};
    if (active) { b[0] = S.lat_min[s]; b[1] = S.lat_max[s]; b[2] = S.lon_min[s]; b[3] = S.lon_max[s]; b[4] = S.lon_avg[s]; }
    (void)d_rect_wave_candidates(R, ps, active, s, nsrc, (unsigned)bR, b[0], b[1], b[2], b[3], b[4], pair_beg, pair_cnt, big_list, big_cnt, wl);
  }
}

// ---------------------------------------------------------------------------------------
// clip + area (+ centroid integrals)
// ---------------------------------------------------------------------------------------
struct ClipOut { double area, clon, clat; };

// area test and integrals on the clipped polygon held at px/py (stride S); returns area or -1
template <int ORDER, int S>
__device__ __forceinline__ void d_finish_pair(const double *px, const double *py, int n_out, double maskv,
                                              double area_in, double area_out, double lon_in_avg,
                                              ClipOut *o, unsigned long long *stats)
{
  double pa, clon = 0, clat = 0;
  if (ORDER == 2) d_poly_area_ctr<S>(px, py, n_out, lon_in_avg, &pa, &clon, &clat);
  else pa = d_poly_area<S>(px, py, n_out);
  double xarea = pa * maskv;                                   // create_xgrid.c:1083
  double min_area = (area_in < area_out) ? area_in : area_out; // :1084
  double ratio = xarea / min_area;
  if (fabs(ratio - 1.e-6) < 1.e-15) atomicAdd(&stats[FG_STAT_BORDERLINE], 1ull);
  if (ratio > 1.e-6) { o->area = xarea; o->clon = clon; o->clat = clat; }
  else o->area = -2.0;                                         // non-empty clip, below the area threshold
}

#ifndef CLIP_THREADS
#define CLIP_THREADS 256
#endif
#ifndef CLIP_SLOTS
#define CLIP_SLOTS 8        // vertices a polygon of the quad kernel may have (more: general kernel)
#endif
#ifndef CLIP_WAVES
#define CLIP_WAVES 4        // waves per SIMD the quad kernel is compiled for
#endif
#ifndef CLIP_PAD_LDS
#define CLIP_PAD_LDS 0      // timing experiment: extra LDS bytes per clip block (occupancy sensitivity)
#endif

// Quad x quad fast path, first half: the Sutherland-Hodgman pass.  LDS: polygon [8][T] double2 (32 KiB per 256 lanes); the
// cutting quad lives in registers.  Returns -1 if the pair must go to the general kernel (more than 4 vertices on a side, or
// more than 8 in an intermediate polygon; RECT: a column that is not exactly vertical); otherwise the vertex count of the clipped polygon left in column tid (0: empty).
// RECT: the destination cell is four values of its column record and two of the latitude axis (FgRect) -- D holds areas only.
// The pass runs at four waves per SIMD and is bound by instruction issue, with a third of its wave cycles spent waiting: what
// was measured on its round trips to memory and LDS and on its exec-masked regions, kept or not, is in
// profiles/clip_edges_summary.md (kept: the pair's loads asked for in one round; the cutting edges unrolled together with the
// polygon's slots read in one round, neither of which pays alone).
// QSRC (with RECT): the source cells are compact (FgCells, xgrid_device.h) -- four vertices in the one round, and the sixteen
// doubles of the side table under n1 > 4 (whole waves as a rule: a cell's pairs are contiguous).
template <bool RECT, int T, bool QSRC = false>
__device__ __forceinline__ int d_clip_quad_sh(double2 (*sh_poly)[T], const int tid, const int s, const int d,
                                              const FgCells &S, const FgCells &D, const FgRect &R, unsigned *err)
{
  // RECT: the cutting cell is always a quad, so source cells of up to 8 vertices (the pole-fixed ones) fit this kernel too --
  // the general kernel then only sees the rare pair whose intermediate polygon outgrows 8 vertices
  constexpr int NV1 = RECT ? CLIP_SLOTS : 4;
  // Everything the pair needs from memory is asked for here in one round, ahead of the vertex-count test: the counts, the source
  // cell's sixteen coordinates whatever its count (a cell record always has them; those from n1 on are not used) and the cutting
  // quad.  Asked for one after the other -- the count, then the quad, then the vertices beyond the fourth under k < n1 -- each
  // was a round trip of its own that a wave sat out.
  // (The empty asm statements keep the compiler from moving the loads back below the test.)
  double x1[NV1], y1[NV1], x2[4], y2[4];
  double lon_out_avg;
  int n1 = S.nv[s], n2 = RECT ? 4 : D.nv[d];
  double lon_in_avg = S.lon_avg[s];
  if constexpr (QSRC) {
    const double *sq = d_cell_quad(S, s);
#pragma unroll
    for (int k = 0; k < NV1; k++) { x1[k] = k < 4 ? sq[k] : 0.0; y1[k] = k < 4 ? sq[4 + k] : 0.0; }
  } else {
    const FgVerts sv = d_cell_verts(S, s, 0);            // (a 128-byte record: the place does not depend on the count)
#pragma unroll
    for (int k = 0; k < NV1; k++) { x1[k] = sv.x[k]; y1[k] = sv.y[k]; }
  }
  if (RECT) {
    const int j = d / R.nx, i = d - j * R.nx;
    const double *c = R.col + (size_t)i * RECT_COLW;
    double ya = R.lat_ax[j], yb = R.lat_ax[j + 1];
    x2[0] = c[0]; x2[1] = c[1]; x2[2] = c[2]; x2[3] = c[3]; lon_out_avg = c[6];
    asm volatile("" : "+v"(ya), "+v"(yb));
    y2[0] = ya; y2[1] = ya; y2[2] = yb; y2[3] = yb;
  } else {
    const FgVerts dv = d_cell_verts(D, d, 0);          // (a 128-byte record, as above)
#pragma unroll
    for (int k = 0; k < 4; k++) { x2[k] = dv.x[k]; y2[k] = dv.y[k]; }
    lon_out_avg = D.lon_avg[d];
#pragma unroll
    for (int k = 0; k < 4; k++) asm volatile("" : "+v"(y2[k]));
    asm volatile("" : "+v"(n2));
  }
#pragma unroll
  for (int k = 0; k < NV1; k++) asm volatile("" : "+v"(x1[k]), "+v"(y1[k]));
#pragma unroll
  for (int k = 0; k < 4; k++) asm volatile("" : "+v"(x2[k]));
  asm volatile("" : "+v"(n1), "+v"(lon_in_avg), "+v"(lon_out_avg));
  if (n1 > NV1 || n2 > 4) return -1;
  // RECT: the inside tests below drop the product that is an exact zero along an axis-aligned edge.  Edges 1 and 3 are
  // horizontal by construction (y2[0] and y2[1], y2[2] and y2[3] are one value each); edges 0 and 2 are vertical where the
  // column record's corners are equal -- the shift and d_pimod1 below give equal values for equal values, so they are equal
  // where the edge code sees them.  A column that fix_lon left not exactly vertical (the longitude axis changes sign inside it)
  // goes to the general kernel, which has the full formula.
  if (RECT && !(x2[3] == x2[0] && x2[1] == x2[2])) return -1;
  if constexpr (QSRC) {
    if (n1 > 4) {
      const FgVerts sv = d_cell_verts(S, s, n1);
#pragma unroll
      for (int k = 0; k < NV1; k++) { x1[k] = sv.x[k]; y1[k] = sv.y[k]; }
    }
  }
  double shift = 0.0;
  {
    double dx = lon_out_avg - lon_in_avg;            // create_xgrid.c:1064-1074
    if (dx < -G_PI) shift = G_TPI; else if (dx > G_PI) shift = -G_TPI;
  }
  bool wrap = false;
#pragma unroll
  for (int k = 0; k < NV1; k++) {
    if (!(k < 4 || k < n1)) { x1[k] = 0.0; y1[k] = 0.0; }
    if (k < n1 && (x1[k] > G_TPI || x1[k] < 0.0)) wrap = true;  // create_xgrid.c:1282
  }
#pragma unroll
  for (int k = 0; k < 4; k++) if (shift != 0.0) x2[k] += shift;
  if (wrap) {                                          // :1290
#pragma unroll
    for (int k = 0; k < NV1; k++) x1[k] = d_pimod1(x1[k]);
#pragma unroll
    for (int k = 0; k < 4; k++) x2[k] = d_pimod1(x2[k]);
  }
#pragma unroll
  for (int k = 0; k < NV1; k++) if (k < 4 || k < n1) sh_poly[k][tid] = make_double2(x1[k], y1[k]);
  // the cutting quad stays in registers; its vertex e is picked with selects (n2 <= 4)
  // vertex e of the cutting quad, picked with bit masks (a ?: chain on e is turned into a scratch-memory
  // table by the optimizer).  Where e is a constant -- every copy of the unrolled loop below, and n2 - 1 in the rectilinear
  // kernel -- the masks fold and the pick costs nothing.
  const long long b0x = __double_as_longlong(x2[0]), b1x = __double_as_longlong(x2[1]);
  const long long b2x = __double_as_longlong(x2[2]), b3x = __double_as_longlong(x2[3]);
  const long long b0y = __double_as_longlong(y2[0]), b1y = __double_as_longlong(y2[1]);
  const long long b2y = __double_as_longlong(y2[2]), b3y = __double_as_longlong(y2[3]);
  auto cut = [=](int e) -> double2 {
    const long long m0 = -(long long)(e == 0), m1 = -(long long)(e == 1), m2 = -(long long)(e == 2), m3 = -(long long)(e == 3);
    return make_double2(__longlong_as_double((b0x & m0) | (b1x & m1) | (b2x & m2) | (b3x & m3)),
                        __longlong_as_double((b0y & m0) | (b1y & m1) | (b2y & m2) | (b3y & m3)));
  };
  // Sutherland-Hodgman against one cutting edge at a time, restructured so that the expensive part -- the intersection (two
  // FP64 divisions) -- is not inside the per-vertex loop: a convex polygon crosses the line of a cutting edge at most twice, so
  // (1) the inside flags of all vertices are collected into bit masks (cheap, every lane busy), (2) the at most two crossings
  // are computed by code that runs twice per cutting edge instead of once per vertex slot with a third of the lanes active
  // (PMC, profiles/r03_summary.md: the old per-vertex loop kept 32.6 of 64 lanes busy), (3) the new polygon is written at
  // positions counted from the masks.  Same intersection formulas on the same operands, same output order as the reference's
  // loop (for every k: the crossing of edge (k-1, k) if there is one, then vertex k if it is inside, create_xgrid.c:1301-1333).
  // A polygon with more than two crossings of one line (non-convex source cell) goes to the general kernel.
  int n_cur = n1;
  bool overflow = false, parallel = false;
  double2 e0 = cut(n2 - 1);
  // The loop over the cutting edges is unrolled (a quad has at most four; the generic instantiation leaves at e == n2), so
  // that e is a constant in every copy and cut(e) is a pick of registers, not sixteen selects.  All CLIP_SLOTS columns of the
  // polygon are read in one round at the head of an edge -- slots from n_cur on hold stale vertices or nothing, and only their
  // contribution to inmask is predicated -- instead of one read, wait and test per slot, each behind its own k < n_cur.
#if FG_EXP == 2
  for (int e = 0; e < 0; e++) {
#else
#pragma unroll
  for (int e = 0; e < 4; e++) {
    if ((!RECT && e >= n2) || n_cur <= 0) break;
#endif
    double2 e1 = cut(e);
    const double x2_0 = e0.x, y2_0 = e0.y, x2_1 = e1.x, y2_1 = e1.y;
    double2 c[CLIP_SLOTS];
    unsigned inmask = 0u;
#pragma unroll
    for (int k = 0; k < CLIP_SLOTS; k++) c[k] = sh_poly[k][tid];
    // RECT: of d_inside_edge's two products one has the factor y2_1 - y2_0 (odd e) or x2_0 - x2_1 (even e, by the guard above),
    // an exact zero; adding +-0 to the other product cannot move it across 1e-12, so that one alone is formed, with its
    // vertex-independent factor taken once per edge.  (The crossings below keep their full formulas: there the sign of a zero
    // numerator reaches the result.)
    const double axis = (e & 1) ? x2_0 - x2_1 : y2_1 - y2_0;
#pragma unroll
    for (int k = 0; k < CLIP_SLOTS; k++)
      if (k < n_cur) {
        int in;
        if (RECT) in = (((e & 1) ? axis * (c[k].y - y2_0) : (c[k].x - x2_0) * axis) <= 1.e-12) ? 1 : 0;
        else in = d_inside_edge(x2_0, y2_0, x2_1, y2_1, c[k].x, c[k].y);
        inmask |= (unsigned)in << k;
      }
    const unsigned full = (1u << n_cur) - 1u;
    const unsigned prevmask = ((inmask << 1) | (inmask >> (n_cur - 1))) & full;     // bit k: vertex k-1 (cyclic) is inside
    const unsigned tmask = inmask ^ prevmask;                                        // bit k: edge (k-1, k) crosses the line
    const int ncross = __popc(tmask);
    if (ncross > 2 || ncross + __popc(inmask) > CLIP_SLOTS) { overflow = true; break; }
    if (tmask) {
      const int ka = __ffs((int)tmask) - 1, kb = 31 - __clz((int)tmask);
      double2 I[2];
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int k = j ? kb : ka;
        const double2 p0 = sh_poly[k ? k - 1 : n_cur - 1][tid], p1 = sh_poly[k][tid];
        const double x1_0 = p0.x, y1_0 = p0.y, x1_1 = p1.x, y1_1 = p1.y;
        double dy1 = y1_1 - y1_0;
        double dy2 = y2_1 - y2_0;
        double dx1 = x1_1 - x1_0;
        double dx2 = x2_1 - x2_0;
        double ds1 = y1_0 * x1_1 - y1_1 * x1_0;
        double ds2 = y2_0 * x2_1 - y2_1 * x2_0;
        double determ = dy2 * dx1 - dy1 * dx2;
        if (fabs(determ) < 1.0e-30) parallel = true;
        I[j] = make_double2((dx2 * ds1 - dx1 * ds2) / determ, (dy2 * ds1 - dy1 * ds2) / determ);
      }
      // (all reads of the old polygon are done: c[] and I[] are registers)
#pragma unroll
      for (int k = 0; k < CLIP_SLOTS; k++)
        if (k < n_cur && ((inmask >> k) & 1u))
          sh_poly[__popc(inmask & ((1u << k) - 1u)) + __popc(tmask & ((2u << k) - 1u))][tid] = c[k];
      sh_poly[__popc(inmask & ((1u << ka) - 1u))][tid] = I[0];                       // no crossing before the first one
      sh_poly[__popc(inmask & ((1u << kb) - 1u)) + 1][tid] = I[1];
    }
    // (no crossing: every vertex inside -> the polygon stays as it is; every vertex outside -> it is empty)
    n_cur = ncross + __popc(inmask);
    e0 = e1;
  }
  if (overflow) return -1;
  if (parallel) atomicOr(err, G_ERRBIT_PARALLEL);
  return n_cur;
}

// Result encoding shared by the clip kernels and the compaction: an accepted pair keeps pair_dst[p] = d and
// gets tmp_area/clon/clat[p]; a rejected pair gets pair_dst[p] = -1.
// (The integrals loop over the polygon's edges and a wave runs as many iterations as its largest polygon has.  Re-binning the
// block's 256 polygons by vertex count through LDS before the integrals, so that a wave sees polygons of equal size, was
// measured in round 1: 502 us against 482 -- the extra barriers and the scattered LDS columns cost more than the divergence.
// CLIP_COMPACT=1, round 3: the block's non-empty polygons moved to its first lanes before the integrals, order kept.  On the
// rectilinear path 4.16 M of 4.59 M candidate pairs are accepted, so there is next to nothing to move: 0.444 ms against 0.433.)
// row_cnt / tmp_rowpos (may be null): an accepted pair takes its slot in its destination row HERE -- a value-returning atomic whose
// latency hides behind the clip arithmetic -- instead of in the compaction, a kernel that does little else than wait on memory; the
// destination-row scan can then run before the compaction, which stores the row lists (perm) itself.
#ifndef CLIP_COMPACT
#define CLIP_COMPACT 0
#endif
__device__ __forceinline__ int d_row_slot(int *row_cnt, bool take, int d, int lane);   // (below, with the compaction)
template <int ORDER, bool RECT, bool QSRC = false>
__global__ __launch_bounds__(CLIP_THREADS) __attribute__((amdgpu_waves_per_eu(CLIP_WAVES, CLIP_WAVES))) void k_clip_quad(FgPairSpace ps, FgCells S, const double *mask, FgCells D, FgRect R,
                                                 double *tmp_area, double *tmp_clon, double *tmp_clat, int *nacc,
                                                 int *defer_list, int *defer_cnt,
                                                 unsigned long long *stats, unsigned *err, int *row_cnt, int *tmp_rowpos)
{
  constexpr int T = CLIP_THREADS;
  __shared__ double2 sh_poly[CLIP_SLOTS][T];
#if CLIP_PAD_LDS
  __shared__ char sh_pad[CLIP_PAD_LDS];
  if (nacc == (int *)16) sh_pad[threadIdx.x * 7 % CLIP_PAD_LDS] = 1;
#endif
#if CLIP_COMPACT
  __shared__ unsigned short sh_perm[T];
  __shared__ unsigned char sh_n[T];
  __shared__ int sh_wtot[T / 64];
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int p0 = blockIdx.x * T;
  // The head of a block in three steps, not a chain of ten loads each waited for on its own (profiles/clip_edges_summary.md
  // counts them in the ISA).  Step 1, two scalar loads and one test: the rectilinear check's verdict and the region's fill
  // -- the launch covers the regions' CAPACITY, and under culling and bands most of its blocks lie beyond their region's
  // fill and leave here, at the cost they always had.  Round 2, for a block that stays:
  // its lanes' pairs and its share of the trig table, asked for together (the empty asm keeps the compiler from moving the
  // pair's loads below the barrier).  Round 3 is the pair's cells, in d_clip_quad_sh.  Read where they are used -- verdict,
  // test, fill, test, table, table, barrier, fill again, src, count, ... -- each was a round trip that the wave sat out.
  // The fill is kept for the lane test below, and src / dst for the second half of the kernel.
  const unsigned first = blockIdx.x * T, reg = first / (unsigned)ps.regcap;
  const unsigned fill = ps.fill[reg * FG_FILL_STRIDE];
  const unsigned bad = RECT ? *R.bad : 0u;
  if ((RECT && bad != 0u) | (first - reg * (unsigned)ps.regcap >= fill)) return;
  static_assert(2 * T >= 112 * 4, "at most two table values per lane");
  const int t0 = min(tid, 112 * 4 - 1), t1 = min(tid + T, 112 * 4 - 1);       // (a lane past the end repeats the last value)
  int s_in = ps.src[p0 + tid], d_in = ps.dst[p0 + tid];
  double tab0 = FG_SINCOS_TAB[t0 >> 2][t0 & 3], tab1 = FG_SINCOS_TAB[t1 >> 2][t1 & 3];
  asm volatile("" : "+v"(s_in), "+v"(d_in), "+v"(tab0), "+v"(tab1));
  fgs_lds_tab[t0] = tab0; fgs_lds_tab[t1] = tab1;
  __syncthreads();
  // ---- first half: clip.  Lane = candidate pair; 4 of 10 pairs of a cubed-sphere x lat-lon job come out empty.
  bool defer = false;
  int n_cur = 0;
  if ((unsigned)(p0 + tid) - reg * (unsigned)ps.regcap < min(fill, (unsigned)ps.regcap)) {      // d_pair_live
    n_cur = d_clip_quad_sh<RECT, T, QSRC>(sh_poly, tid, s_in, d_in, S, D, R, err);
    if (n_cur < 0) { defer = true; n_cur = 0; }        // rare; the general kernel finishes this pair
    else if (n_cur == 0) ps.dst[p0 + tid] = -1;
  }
  // ---- the block's non-empty polygons move to its first lanes (order kept): the integrals below cost 2/3 of this kernel's
  // arithmetic, and a wave of them costs the same with 38 live lanes as with 64.  The polygons stay where they are in LDS:
  // lane l works on column sh_perm[l].
  int src = tid;
#if CLIP_COMPACT
  {
    const int wave = tid >> 6;
    const unsigned long long hm = __ballot(n_cur > 0);
    if (lane == 0) sh_wtot[wave] = __popcll(hm);
    sh_n[tid] = (unsigned char)n_cur;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < T / 64; w++) { const int c = sh_wtot[w]; if (w < wave) base += c; total += c; }
    if (n_cur > 0) sh_perm[base + __popcll(hm & ((1ull << lane) - 1ull))] = (unsigned short)tid;
    __syncthreads();
    if (tid < total) { src = sh_perm[tid]; n_cur = sh_n[src]; } else n_cur = 0;
  }
#endif
  // ---- second half: area (+ centroid integrals) of polygon `src`
  bool below = false, acc = false;
  int s = -1, d_acc = -1;
  if (n_cur > 0) {
    const int p = p0 + src;
    s = CLIP_COMPACT ? ps.src[p] : s_in;               // (a pair that reaches this point still has the dst it came with)
    const int d = CLIP_COMPACT ? ps.dst[p] : d_in;
    ClipOut o; o.area = -1.0; o.clon = 0; o.clat = 0;
    const double *px = (const double *)&sh_poly[0][src];
#if FG_EXP == 1
    o.area = n_cur + px[0] + px[1];
#else
    d_finish_pair<ORDER, 2 * T>(px, px + 1, n_cur, mask ? mask[s] : 1.0, S.area[s], D.area[d], S.lon_avg[s], &o, stats);
#endif
    if (o.area >= 0) {
      acc = true;
      tmp_area[p] = o.area;
      if (ORDER == 2) { tmp_clon[p] = o.clon; tmp_clat[p] = o.clat; }
      d_acc = d;
    } else {
      ps.dst[p] = -1;
      below = (o.area == -2.0);                                  // rare (slivers below the 1e-6 ratio)
    }
  }
  // the destination-row slot of an accepted pair.  Over a coarse target the pairs of a wave belong to a few destination cells
  // (C384 -> 10 deg: 1 450 exchange cells per row) and value-returning atomics on one address queue up behind each other (that
  // clip ran SEVEN times slower per pair than the headline's, with or without its arithmetic): one atomic per run of lanes with
  // the same destination cell (a lane that was not accepted ends a run).
  if (row_cnt) {
    const int slot = d_row_slot(row_cnt, acc, d_acc, lane);
    if (acc) tmp_rowpos[p0 + src] = slot;
  }
  // nacc[s]: accepted pairs of source cell s.  Lanes are pair-ordered (before and after the move), so one atomic per
  // (wave, source cell) run does it.
  if (__ballot(s >= 0)) {
    const int s_prev = __shfl_up(s, 1, 64);
    const bool head = (lane == 0) || (s != s_prev);
    const unsigned long long hm = __ballot(head), am = __ballot(acc);
    if (head && s >= 0) {
      const unsigned long long above = (lane == 63) ? 0ull : (hm >> (lane + 1)) << (lane + 1);
      const int end = above ? (__ffsll((long long)above) - 1) : 64;
      const unsigned long long upto = (end == 64) ? ~0ull : ((1ull << end) - 1ull);
      const int cnt = __popcll(am & upto & ~((1ull << lane) - 1ull));
      if (cnt) atomicAdd(&nacc[s], cnt);
    }
  }
  // one atomic per wave that has deferred pairs / slivers (value-returning same-address atomics serialise at ~12 ns each)
  const unsigned long long dm = __ballot(defer), bm = __ballot(below);
  if (dm) {
    int q = 0;
    if (lane == 0) q = atomicAdd(defer_cnt, __popcll(dm));
    q = __shfl(q, 0);
    if (defer) defer_list[q + __popcll(dm & ((1ull << lane) - 1ull))] = p0 + tid;
  }
  if (bm && lane == 0) atomicAdd(&stats[FG_STAT_BELOW], (unsigned long long)__popcll(bm));
}

// General path: up to 8 x 8 vertices, intermediate polygons up to 16.  One wave per block,
// LDS: two [16][64] double2 ping-pong buffers + cutter [8][64] double2 = 40 KiB.
#define GEN_THREADS 64
#define GEN_CAP 16
template <int ORDER, bool RECT>
__global__ __launch_bounds__(GEN_THREADS) void k_clip_general(const int *defer_list, const int *defer_cnt,
                                                              const int *pair_src, int *pair_dst,
                                                              FgCells S, const double *mask, FgCells D, FgRect R,
                                                              double *tmp_area, double *tmp_clon, double *tmp_clat, int *nacc,
                                                              unsigned long long *stats, unsigned *err, int *row_cnt, int *tmp_rowpos)
{
  __shared__ double2 sh_a[GEN_CAP][GEN_THREADS];
  __shared__ double2 sh_b[GEN_CAP][GEN_THREADS];
  __shared__ double2 sh_cut[G_MAXV][GEN_THREADS];
  if (RECT && *R.bad) return;
  d_load_trig_table();
  const int tid = threadIdx.x;
  const int ndefer = *defer_cnt;
  for (int q = blockIdx.x * GEN_THREADS + tid; q < ndefer; q += gridDim.x * GEN_THREADS) {
    const int p = defer_list[q];
    const int s = pair_src[p], d = pair_dst[p];
    const int n1 = S.nv[s], n2 = RECT ? 4 : D.nv[d];
    const FgVerts sv = d_cell_verts(S, s, n1);
    const double lon_in_avg = S.lon_avg[s];
    double dvx[G_MAXV], dvy[G_MAXV], lon_out_avg;
    if (RECT) {
      const int j = d / R.nx, i = d - j * R.nx;
      const double *c = R.col + (size_t)i * RECT_COLW;
      const double ya = R.lat_ax[j], yb = R.lat_ax[j + 1];
      dvx[0] = c[0]; dvx[1] = c[1]; dvx[2] = c[2]; dvx[3] = c[3]; lon_out_avg = c[6];
      dvy[0] = ya; dvy[1] = ya; dvy[2] = yb; dvy[3] = yb;
#pragma unroll
      for (int k = 4; k < G_MAXV; k++) { dvx[k] = 0.0; dvy[k] = 0.0; }
    } else {
      const FgVerts dv = d_cell_verts(D, d, n2);
#pragma unroll
      for (int k = 0; k < G_MAXV; k++) { dvx[k] = dv.x[k]; dvy[k] = dv.y[k]; }
      lon_out_avg = D.lon_avg[d];
    }
    double shift = 0.0;
    {
      double dx = lon_out_avg - lon_in_avg;
      if (dx < -G_PI) shift = G_TPI; else if (dx > G_PI) shift = -G_TPI;
    }
    bool wrap = false;
    for (int k = 0; k < n1; k++) { double xv = sv.x[k]; if (xv > G_TPI || xv < 0.0) wrap = true; }
    for (int k = 0; k < n1; k++) {
      double xv = sv.x[k]; if (wrap) xv = d_pimod1(xv);
      sh_a[k][tid] = make_double2(xv, sv.y[k]);
    }
#pragma unroll
    for (int k = 0; k < G_MAXV; k++)
      if (k < n2) {
        double xv = dvx[k]; if (shift != 0.0) xv += shift; if (wrap) xv = d_pimod1(xv);
        sh_cut[k][tid] = make_double2(xv, dvy[k]);
      }
    double2 (*cur)[GEN_THREADS] = sh_a;
    double2 (*nxt)[GEN_THREADS] = sh_b;
    int n_cur = n1;
    bool overflow = false, parallel = false;
    double2 e0 = sh_cut[n2 - 1][tid];
    for (int e = 0; e < n2 && n_cur > 0 && !overflow; e++) {
      double2 e1 = sh_cut[e][tid];
      const double x2_0 = e0.x, y2_0 = e0.y, x2_1 = e1.x, y2_1 = e1.y;
      double2 lastv = cur[n_cur - 1][tid];
      double x1_0 = lastv.x, y1_0 = lastv.y;
      int inside_last = d_inside_edge(x2_0, y2_0, x2_1, y2_1, x1_0, y1_0);
      int n_new = 0;
      for (int k = 0; k < n_cur; k++) {
        double2 cv = cur[k][tid];
        double x1_1 = cv.x, y1_1 = cv.y;
        int inside = d_inside_edge(x2_0, y2_0, x2_1, y2_1, x1_1, y1_1);
        if (inside != inside_last) {
          double dy1 = y1_1 - y1_0;
          double dy2 = y2_1 - y2_0;
          double dx1 = x1_1 - x1_0;
          double dx2 = x2_1 - x2_0;
          double ds1 = y1_0 * x1_1 - y1_1 * x1_0;
          double ds2 = y2_0 * x2_1 - y2_1 * x2_0;
          double determ = dy2 * dx1 - dy1 * dx2;
          if (fabs(determ) < 1.0e-30) parallel = true;
          if (n_new < GEN_CAP) nxt[n_new][tid] = make_double2((dx2 * ds1 - dx1 * ds2) / determ,
                                                              (dy2 * ds1 - dy1 * ds2) / determ);
          else overflow = true;
          n_new++;
        }
        if (inside) {
          if (n_new < GEN_CAP) nxt[n_new][tid] = make_double2(x1_1, y1_1);
          else overflow = true;
          n_new++;
        }
        x1_0 = x1_1; y1_0 = y1_1; inside_last = inside;
      }
      n_cur = n_new;
      double2 (*t)[GEN_THREADS] = cur; cur = nxt; nxt = t;
      e0 = e1;
    }
    if (overflow) { atomicOr(err, G_ERRBIT_OVERFLOW); pair_dst[p] = -1; continue; }
    if (parallel) atomicOr(err, G_ERRBIT_PARALLEL);
    ClipOut o; o.area = -1.0; o.clon = 0; o.clat = 0;
    if (n_cur > 0) {
      const double *px = (const double *)&cur[0][tid];
      d_finish_pair<ORDER, 2 * GEN_THREADS>(px, px + 1, n_cur, mask ? mask[s] : 1.0, S.area[s], D.area[d],
                                            lon_in_avg, &o, stats);
    }
    if (o.area >= 0) {
      tmp_area[p] = o.area;
      if (ORDER == 2) { tmp_clon[p] = o.clon; tmp_clat[p] = o.clat; }
      atomicAdd(&nacc[s], 1);
      if (row_cnt) tmp_rowpos[p] = atomicAdd(&row_cnt[d], 1);
    } else {
      pair_dst[p] = -1;
      if (o.area == -2.0) atomicAdd(&stats[FG_STAT_BELOW], 1ull);
    }
  }
}

// ---------------------------------------------------------------------------------------
// compaction into canonical order + per-source-cell sums
// ---------------------------------------------------------------------------------------
// The clip kernels count the accepted pairs of every source cell (nacc, one atomic per run of equal cells in a wave, hidden
// behind the clip arithmetic); a scan of nacc gives xoff[s], the reference's running nxgrid.  k_compact then works with ONE
// LANE PER PAIR, so that every array of the pair list is read once, fully coalesced:
//   * a block takes the source cells whose FIRST pair lies among its 256 pairs; such a cell (at most CP_SMALL pairs) ends
//     within the next CP_SMALL pairs, which the first lanes of the block handle as well ("halo");
//   * the destination indices of those 256 + CP_SMALL pairs are staged in LDS; a pair's rank among the accepted pairs of its
//     source cell by destination index (the reference's ij loop) is a handful of LDS reads;
//   * the exchange cell is stored at xoff[s] + rank (neighbouring lanes store neighbouring cells) and takes its slot in its
//     destination row (x_rowpos), which also counts the CSR row sizes;
//   * order 2: the values go to LDS at the cell's first pair + rank, and the lane holding the cell's first pair adds them up
//     in that order = exchange-cell order (conserve_interp.c:216-221).
// Cells with more than CP_SMALL pairs ("big": the cells around a pole of the target grid, every cell of a coarse -> fine
// remap; listed by the candidate kernel) are done by the big-cell blocks of the same launch.  Nothing depends on the order in which the candidate kernel filled the pair list.
// (Measured at C384 -> 0.25 deg: 109 us.  A first version gave each block 256 source cells and found xoff by look-back inside the
// kernel: 320-430 us -- its per-cell loads of the pair list are strided, and a chain of dependent round trips per block does not
// hide behind five blocks per CU; a lane-per-pair version that left the cells cut by a block boundary to one lane: 245 us.)
#define CP_SPAN (256 + CP_SMALL)
static_assert(CP_SMALL % 64 == 0 && CP_SMALL <= 256, "the halo lanes of k_compact are whole waves of its 256-lane block");

struct CpPair { int s, d, beg, cnt, row; long x0; int na; double a, l, t; bool mine; };    // row: the cell's place in perm (early row slots)

// Slot of an exchange cell in its destination row: atomicAdd(&row_cnt[d], 1) for every lane with take -- or, where many lanes of
// the wave share a destination cell (a coarse target: value-returning atomics on one address queue up), one atomic per group of
// lanes with the same d.  Every lane of the wave must call it.
__device__ __forceinline__ int d_row_slot(int *row_cnt, bool take, int d, int lane)
{
  const int key = take ? d : -1 - lane;                    // (distinct for the lanes that take no slot)
  const int prev = __shfl_up(key, 1, 64);
  const bool head = (lane == 0) || (key != prev);
  const unsigned long long hm = __ballot(head), am = __ballot(take);
  int slot = 0;
  if (!am) return 0;
  // similar resolutions: neighbouring lanes hardly ever share a cell -- a lane an atomic.  (Adjacent equal keys are the cheap sign
  // of sharing; with rejected pairs in between -- the great-circle search -- a third of the takers still have an equal neighbour.)
  if (4 * __popcll(hm & am) > 3 * __popcll(am)) {          // (wave-uniform)
    if (take) slot = atomicAdd(&row_cnt[d], 1);
    return slot;
  }
  unsigned long long rem = am;
  for (int it = 0; rem && it < 8; it++) {                  // groups by VALUE (not only runs), the first eight distinct cells
    const int lead = __ffsll((long long)rem) - 1;
    const int d0 = __shfl(d, lead);
    const unsigned long long grp = __ballot(take && d == d0) & rem;
    int base = 0;
    if (lane == lead) base = atomicAdd(&row_cnt[d0], __popcll(grp));
    base = __shfl(base, lead);
    if ((grp >> lane) & 1ull) slot = base + __popcll(grp & ((1ull << lane) - 1ull));
    rem &= ~grp;
  }
  if ((rem >> lane) & 1ull) slot = atomicAdd(&row_cnt[d], 1);       // (more than eight distinct cells in the wave: the rest one by one)
  return slot;
}

// A lane's pair of the block's 256 (c) and, for the first CP_SMALL lanes (HALO), its pair of the halo (h): everything the ranking
// and the stores need, in rounds of loads that are each issued together -- (A) what the pair index alone addresses, (B) what needs
// the pair's source and destination cell (xoff too: it waits for no answer about whose cell it is), (C) the area and centroid
// integrals of a halo pair once it is known to be this block's (with (A) they were reads for other blocks' pairs: FETCH_SIZE
// 179 MB against 154 MB, and 4 us slower).  Loads go out ahead of their guards, from clamped indices (pair p0 is live; row 0 for a
// rejected pair), and a value loaded for nothing is dropped: a pair beyond the region's end keeps d = -1 and mine = false,
// and d_cp_place reads the values of its own accepted pairs only.
// (A lane used to finish the main pair, four dependent rounds, before it began the same four for the halo pair.)
template <int ORDER, bool HALO>
__device__ __forceinline__ void d_cp_load(const FgPairSpace &ps, const FgCompactIo &io, int p0, int tid, unsigned live_end, CpPair &c, CpPair &h)
{
  constexpr int N = HALO ? 2 : 1;
  const int *const rowpos = io.tmp_rowpos ? io.tmp_rowpos : ps.dst;   // (no slots from the clip kernels: row is not used)
  int p[N], pc[N], s[N], d[N], rp[N], beg[N], cnt[N], rb[N], x0[N], x1[N];
  bool ok[N];
  double a[N], l[N], t[N];
#pragma unroll
  for (int k = 0; k < N; k++) { p[k] = p0 + 256 * k + tid; ok[k] = (unsigned)p[k] < live_end; pc[k] = ok[k] ? p[k] : p0; }
#pragma unroll
  for (int k = 0; k < N; k++) {                            // round A
    s[k] = ps.src[pc[k]]; d[k] = ps.dst[pc[k]]; rp[k] = rowpos[pc[k]];
    if (k == 0) { a[k] = io.tmp_area[pc[k]]; if (ORDER == 2) { l[k] = io.tmp_clon[pc[k]]; t[k] = io.tmp_clat[pc[k]]; } }
  }
#pragma unroll
  for (int k = 0; k < N; k++) {                            // round B
    beg[k] = io.pair_beg[s[k]]; cnt[k] = io.pair_cnt[s[k]]; rb[k] = io.row_ptr[max(d[k], 0)];
    x0[k] = io.xoff[s[k]]; x1[k] = io.xoff[s[k] + 1];
  }
#pragma unroll
  for (int k = 0; k < N; k++) {
    // this block's cell: its first pair is one of the block's 256 (halo lanes: ... and it is not a big cell's)
    const bool mine = ok[k] && cnt[k] <= CP_SMALL && beg[k] >= p0 && beg[k] < p0 + 256;
    if (k == 1) {                                          // round C, the halo pair's values: few halo pairs are this block's
      a[k] = 0; l[k] = 0; t[k] = 0;
      if (mine && d[k] >= 0) { a[k] = io.tmp_area[p[k]]; if (ORDER == 2) { l[k] = io.tmp_clon[p[k]]; t[k] = io.tmp_clat[p[k]]; } }
    }
    CpPair &o = k ? h : c;
    o.s = ok[k] ? s[k] : 0; o.d = ok[k] ? d[k] : -1; o.beg = ok[k] ? beg[k] : 0; o.cnt = ok[k] ? cnt[k] : 0;
    o.mine = mine; o.x0 = mine ? x0[k] : 0; o.na = mine ? x1[k] - x0[k] : 0; o.row = (int)((unsigned)rb[k] + (unsigned)rp[k]);
    o.a = a[k]; o.l = (ORDER == 2) ? l[k] : 0.0; o.t = (ORDER == 2) ? t[k] : 0.0;
  }
}

// returns the exchange cell's position if its row slot is still to be taken (no slots from the clip kernels), else -1
template <int ORDER>
__device__ __forceinline__ long d_cp_place(const FgCompactIo &io, const CpPair &c, int p0, const int *sh_d, double (*sh_v)[CP_SPAN])
{
  if (!c.mine || c.d < 0 || c.x0 + c.na > io.xcap) return -1;
  int rank = 0;
  const int lb = c.beg - p0;
  for (int j = 0; j < c.cnt; j++) rank += ((unsigned)sh_d[lb + j] < (unsigned)c.d) ? 1 : 0;       // rejected entries are 0xffffffff
  const long pos = c.x0 + rank;
  io.x_src[pos] = c.s; io.x_dst[pos] = c.d; io.x_area[pos] = c.a;
  if (ORDER == 2) { io.x_c1[pos] = c.l; io.x_c2[pos] = c.t; sh_v[0][lb + rank] = c.a; sh_v[1][lb + rank] = c.l; sh_v[2][lb + rank] = c.t; }
  if (io.tmp_rowpos) io.perm[c.row] = FgRowEnt{(int)pos, c.s};   // the row slot was taken by the clip kernel: row_ptr[d] + tmp_rowpos[p]
  else return pos;
  return -1;
}

#define RANK_WORDS 1024      // 65536 destination indices: 45 rows of a 1440-column grid
#define BIG_BLOCKS 512       // blocks of the big-cell role, in front of the lane-per-pair blocks
// The block's LDS: just under 20 KB, so that eight blocks share a CU (8 waves per SIMD, what the launch bound holds the
// registers to).  The lane-per-pair role, which does nearly all the work of similar grids, uses 10.6 KB of it.  The big-cell
// role divides it per cell: the bitmap over the cell's span of destination indices (at most RANK_WORDS words), half as much
// for the prefix, and what is left in three equal parts for the staged values (d_big_stage): 336 ranks per stage under a
// bitmap of full size, 512 for a cell of C24 over a 0.25-degree grid (30 rows: 675 words), 848 without a bitmap.  (Fixed
// sizes -- 1024 words and 3 x 512 values, 24 KB -- held the launch at six blocks per CU; 3 x 256 values made eight fit and
// cost the coarse -> fine plans, whose cells then took two stages and lost the loads issued ahead of the rank: compaction of
// C24 -> 0.25 deg 0.30 -> 0.44 ms, C48 0.154 -> 0.189 ms.)
#define CP_LDS_DOUBLES 2552
static_assert(CP_LDS_DOUBLES >= CP_SPAN / 2 + 8 + 3 * CP_SPAN, "the lane-per-pair role's sh_d and sh_v fit the block's LDS");
static_assert(CP_LDS_DOUBLES >= RANK_WORDS + RANK_WORDS / 2 + 3 * 8, "a bitmap of full size leaves room for a stage");
static_assert(8 * (CP_LDS_DOUBLES * 8 + 64) <= 160 * 1024, "eight blocks of k_compact per CU");
// ranks per stage of the big-cell role's ordered sums, for a cell whose bitmap has nw words (0: ranked by comparison)
__device__ __forceinline__ int d_big_stage(int nw) { const int w8 = (nw + 7) & ~7; return ((CP_LDS_DOUBLES - w8 - w8 / 2) / 3) & ~7; }

// The big cells: a block per cell.  Ranking a pair by comparing it with all the others of its cell is quadratic (great-circle
// search: ~3000 pairs in each of ~600 cells); here the block marks the cell's destination indices in an LDS bitmap over their
// span and reads each rank off as a prefix population count: linear.  Spans that do not fit fall back to the comparison.
template <int ORDER>
__device__ __forceinline__ void d_compact_big(int nsrc, const FgPairSpace &ps, const FgCompactIo &io, double *lds)
{
  unsigned long long *bits = (unsigned long long *)lds;              // [nw], nw <= RANK_WORDS: the cell's bitmap
  __shared__ int smin, smax;
  if (blockIdx.x == 0 && threadIdx.x < 64) {                  // candidate totals for the host's capacity checks
    unsigned long long f = 0; unsigned mx = 0;
    for (int r = threadIdx.x; r < ps.nreg; r += 64) { const unsigned v = ps.fill[r * FG_FILL_STRIDE]; f += v; mx = max(mx, v); }
#pragma unroll
    for (int o = 32; o; o >>= 1) { f += __shfl_xor(f, o); mx = max(mx, (unsigned)__shfl_xor((int)mx, o)); }
    if (threadIdx.x == 0) { io.dc->total[1] = f; io.dc->total[3] = mx; }
  }
  const int nb = *io.big_cnt;
  for (int h = blockIdx.x; h < nb; h += BIG_BLOCKS) {
    const int s = io.big_list[h];
    const int o = io.pair_beg[s], c = io.pair_cnt[s];
    const long x0 = io.xoff[s];
    const int na = io.xoff[s + 1] - (int)x0;
    if (threadIdx.x == 0) { smin = 0x7fffffff; smax = -1; }
    __syncthreads();
    int lmin = 0x7fffffff, lmax = -1;
    for (int k = threadIdx.x; k < c; k += 256) { const int d = ps.dst[o + k]; if (d >= 0) { lmin = min(lmin, d); lmax = max(lmax, d); } }
    if (lmax >= 0) { atomicMin(&smin, lmin); atomicMax(&smax, lmax); }
    __syncthreads();
    const int dmin = smin, dmax = smax;
    const long span = (long)dmax - dmin + 1;
    const bool bitmap = dmax >= 0 && span <= (long)RANK_WORDS * 64;
    const int nw = bitmap ? (int)((span + 63) >> 6) : 0, w8 = (nw + 7) & ~7;
    int *pref = (int *)(lds + w8);                           // [nw]
    const int stage = d_big_stage(nw);                       // ranks per stage: what the bitmap and the prefix leave, in three parts
    double *sval = lds + w8 + w8 / 2;                        // [3][stage]
    if (bitmap) {
      for (int w = threadIdx.x; w < nw; w += 256) bits[w] = 0ull;
      __syncthreads();
      for (int k = threadIdx.x; k < c; k += 256) {
        const int d = ps.dst[o + k];
        if (d >= 0) atomicOr(&bits[(d - dmin) >> 6], 1ull << ((d - dmin) & 63));
      }
      __syncthreads();
      // exclusive prefix of the word populations: each thread owns a contiguous chunk of words
      const int per = (nw + 255) / 256, w0 = threadIdx.x * per, w1 = min(nw, w0 + per);
      int mine = 0;
      for (int w = w0; w < w1; w++) mine += __popcll(bits[w]);
      unsigned tot;
      const int before = (int)block_incl_scan((unsigned)mine, &tot) - mine;
      int run = before;
      for (int w = w0; w < w1; w++) { pref[w] = run; run += __popcll(bits[w]); }
      __syncthreads();
    }
    // exchange cells to their places; order 2: the values also go to LDS in rank order, `stage` ranks at a time, where three
    // lanes (one array each) add them up in exchange-cell order -- hundreds to thousands of ordered additions per cell, which
    // from global memory (even with the loads 16 ahead) set the duration of the whole compaction
    // A cell that fits one stage (every cell of a coarse -> fine remap) takes a pair's values and row slot along with its
    // destination index, and row_ptr as soon as that is back, ahead of the rank: two rounds of loads per pair instead of
    // four.  A cell of several stages (great-circle search) passes over its pairs once per stage and loads only what the
    // stage stores.
    const bool ahead = na <= stage;                        // (block-uniform)
    const int *const rowpos = io.tmp_rowpos ? io.tmp_rowpos : ps.dst;
    double acc = 0;
    for (int c0 = 0; c0 < max(na, 1); c0 += stage) {
      for (int k = threadIdx.x; k < c; k += 256) {
        const int p = o + k;
        const int d = ps.dst[p];
        double a = 0, l = 0, t = 0;
        int row = 0;
        if (ahead) {
          a = io.tmp_area[p]; if (ORDER == 2) { l = io.tmp_clon[p]; t = io.tmp_clat[p]; }
          row = (int)((unsigned)rowpos[p] + (unsigned)io.row_ptr[max(d, 0)]);
        }
        if (d < 0) continue;
        int rank;
        if (bitmap) { const int w = (d - dmin) >> 6, b = (d - dmin) & 63; rank = pref[w] + __popcll(bits[w] & ((1ull << b) - 1ull)); }
        else { rank = 0; for (int j = 0; j < c; j++) rank += ((unsigned)ps.dst[o + j] < (unsigned)d) ? 1 : 0; }
        if (rank < c0 || rank >= c0 + stage) continue;
        const long pos = x0 + rank;
        if (pos >= io.xcap) continue;
        if (!ahead) {
          a = io.tmp_area[p]; if (ORDER == 2) { l = io.tmp_clon[p]; t = io.tmp_clat[p]; }
          if (io.tmp_rowpos) row = io.row_ptr[d] + io.tmp_rowpos[p];
        }
        io.x_src[pos] = s; io.x_dst[pos] = d; io.x_area[pos] = a;
        if (ORDER == 2) {
          io.x_c1[pos] = l; io.x_c2[pos] = t;
          sval[rank - c0] = a; sval[stage + rank - c0] = l; sval[2 * stage + rank - c0] = t;
        }
        if (io.tmp_rowpos) io.perm[row] = FgRowEnt{(int)pos, s};
        else io.x_rowpos[pos] = atomicAdd(&io.row_cnt[d], 1);
      }
      __syncthreads();
      if (ORDER == 2 && threadIdx.x < 3 && x0 + na <= io.xcap) {
        const double *v = sval + threadIdx.x * stage;
        const int n = min(stage, na - c0);
        int k = 0;
        for (; k + 8 <= n; k += 8) {
          double t[8];
#pragma unroll
          for (int u = 0; u < 8; u++) t[u] = v[k + u];
#pragma unroll
          for (int u = 0; u < 8; u++) acc += t[u];
        }
        for (; k < n; k++) acc += v[k];
      }
      __syncthreads();
    }
    if (ORDER == 2 && io.sums && threadIdx.x < 3) io.sums[(size_t)threadIdx.x * nsrc + s] = acc;
  }
}

// Blocks [0, BIG_BLOCKS): the big cells (listed by the candidate kernel); the rest: one lane per pair.  One launch, so that the
// few long-running big-cell blocks start first and run beside the others instead of after them.
template <int ORDER>
__global__ __launch_bounds__(256, 8) void k_compact(int nsrc, FgPairSpace ps, FgCompactIo io)
{
  __shared__ double lds[CP_LDS_DOUBLES];
  if ((int)blockIdx.x < BIG_BLOCKS) { d_compact_big<ORDER>(nsrc, ps, io, lds); return; }
  int *sh_d = (int *)lds;                                            // [CP_SPAN]
  double (*sh_v)[CP_SPAN] = (double (*)[CP_SPAN])(lds + CP_SPAN / 2 + 8);   // [3][CP_SPAN]
  const int tid = threadIdx.x;
  const int p0 = ((int)blockIdx.x - BIG_BLOCKS) * 256;
  const unsigned r = (unsigned)p0 / (unsigned)ps.regcap;          // block-uniform
  const unsigned rfill = ps.fill[r * FG_FILL_STRIDE];
  const unsigned live_end = r * (unsigned)ps.regcap + (rfill < (unsigned)ps.regcap ? rfill : (unsigned)ps.regcap);   // end of the region's pairs
  if ((unsigned)p0 >= live_end) return;
  CpPair c, h; h.mine = false; h.d = -1;
  if (tid < CP_SMALL) { d_cp_load<ORDER, true>(ps, io, p0, tid, live_end, c, h); sh_d[256 + tid] = h.d; }   // (whole waves)
  else d_cp_load<ORDER, false>(ps, io, p0, tid, live_end, c, h);
  sh_d[tid] = c.d;
  __syncthreads();
  const bool first = (unsigned)(p0 + tid) < live_end && p0 + tid == c.beg;
  {
    const long pos = d_cp_place<ORDER>(io, c, p0, sh_d, sh_v);
    if (!io.tmp_rowpos) { const int slot = d_row_slot(io.row_cnt, pos >= 0, c.d, tid & 63); if (pos >= 0) io.x_rowpos[pos] = slot; }
  }
  if (tid < CP_SMALL) {                                    // (whole waves: CP_SMALL is a multiple of 64)
    const long pos = d_cp_place<ORDER>(io, h, p0, sh_d, sh_v);
    if (!io.tmp_rowpos) { const int slot = d_row_slot(io.row_cnt, pos >= 0, h.d, tid & 63); if (pos >= 0) io.x_rowpos[pos] = slot; }
  }
  if (ORDER != 2 || !io.sums) return;
  __syncthreads();
  if (!first || !c.mine || c.x0 + c.na > io.xcap) return;
  double sa = 0, sl = 0, st = 0;
  const int lb = c.beg - p0;
  for (int k = 0; k < c.na; k++) { sa += sh_v[0][lb + k]; sl += sh_v[1][lb + k]; st += sh_v[2][lb + k]; }
  io.sums[c.s] = sa; io.sums[nsrc + c.s] = sl; io.sums[2 * (size_t)nsrc + c.s] = st;
}

// ---------------------------------------------------------------------------------------
// order-2 centroid pass
// ---------------------------------------------------------------------------------------
// cen[s] = centroid lon/lat of source cell s (conserve_interp.c:327-348), one 16-byte record: the record kernel of the finalize
// (k_csr_sortgather) and k_distances fetch both coordinates with one gather
__global__ __launch_bounds__(256) void k_centroids(int nsrc, FgCells S, const double *sums, FgSrcRec *cen)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  double a = 0, ca = 1, cl = 0, ct = 0;
  int nv = 0;
  bool whole = false;                                      // the cell's own integrals are needed (covered area off by >= 1e-3)
  // (a source cell a culling search left out -- nv = 0 -- has no exchange cell on this rank: its centroid is never read, though
  // the totals handed over by the other ranks are there)
  // A cell without exchange cells (most cells of a rank's band) costs one load; for the others the vertex count, the cell's
  // area and the two integrals go out together (they were two more dependent round trips)
  if (s < nsrc && (a = sums[s]) > 0) {
    const double sl = sums[nsrc + s], st = sums[2 * (size_t)nsrc + s], sa = S.area[s];
    nv = S.nv[s];
    if (nv > 0) {
      ca = sa;
      if (fabs(a - ca) / ca < 1.e-3) {
        cl = sl / a;
        ct = st / a;
      } else whole = true;
    }
  }
  // the sine table (3.5 KB into LDS, a barrier) only for blocks that hold such a cell: none in a global remap of similar grids
  if (__syncthreads_or(whole)) {
    d_load_trig_table();
    if (whole) {
      double x[G_MAXV], y[G_MAXV];
      int n = nv;
      const FgVerts vp = d_cell_verts(S, s, n);
      for (int k = 0; k < G_MAXV; k++) { x[k] = k < n ? vp.x[k] : 0.0; y[k] = k < n ? vp.y[k] : 0.0; }   // (zeros beyond n, as a 128-byte record has them)
      cl = d_poly_ctrlon<1>(x, y, n, S.lon_avg[s]) / ca;
      ct = d_poly_ctrlat<1>(x, y, n) / ca;
    }
  }
  if (s < nsrc) cen[s] = FgSrcRec{cl, ct};
}

// di = clon/area - cen_lon, dj = clat/area - cen_lat (conserve_interp.c:256-257,355-356)
__global__ __launch_bounds__(256) void k_distances(long nx, const int *x_src, const double *x_area, const FgSrcRec *cen, double *x_c1,
                                                    double *x_c2)
{
  long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= nx) return;
  int s = x_src[n];
  double a = x_area[n];
  double di = x_c1[n] / a, dj = x_c2[n] / a;
  di -= cen[s].cen_lon; dj -= cen[s].cen_lat;
  x_c1[n] = di; x_c2[n] = dj;
}

// ---------------------------------------------------------------------------------------
// host-callable launchers
// ---------------------------------------------------------------------------------------
static inline int nblk(long n, int t) { return (int)((n + t - 1) / t); }

void fgd_cell_struct(const FgTile *tiles_dev, int ntiles, int ncells, FgCells c, unsigned *err, hipStream_t st)
{
  if (ncells > 0) k_cell_struct<<<nblk(ncells, 256), 256, 0, st>>>(tiles_dev, ntiles, ncells, c, err);
}

void fgd_cell_struct2(const FgTileSet &ts, const FgTile *tiles_in, FgTile *tiles_out, int ntiles, int nsrc, int ndst, FgCells S, FgCells D,
                      FgBins b, int *slot_cnt, int order, int *src_idx_f, double *sums, unsigned *err, hipStream_t st,
                      unsigned long long *band_keys, int cull, double dst_tlon)
{
  const int nbS = nblk(nsrc, 256), nbD = nblk(ndst, 256);
  if (nbS + nbD > 0)
    k_cell_struct2<<<nbS + nbD, 256, 0, st>>>(ts, tiles_in, tiles_out, ntiles, nsrc, ndst, nbS, S, D, b, slot_cnt, order, src_idx_f, sums, err,
                                              band_keys, cull, dst_tlon);
}

void fgd_bin_count(int ncells, FgCells c, FgBins b, int *slot_cnt, hipStream_t st)
{
  if (ncells > 0) k_bin_count<<<nblk(ncells, 256), 256, 0, st>>>(ncells, c, b, slot_cnt);
}

void fgd_bin_fill(int ndst, FgCells D, FgBins b, int *slot_fill, const int *slot_start, FgBinEntry *entries, int cap,
                  int nsrc, FgCells S, const double *mask, int *heavy_list, int *heavy_cnt, hipStream_t st)
{
  const int nbD = nblk(ndst, 256), nbS = nblk(nsrc, 256);
  if (nbD + nbS > 0)
    k_bin_fill<<<nbD + nbS, 256, 0, st>>>(ndst, nbD, D, b, slot_fill, slot_start, entries, cap, nsrc, S, mask, heavy_list, heavy_cnt);
}

void fgd_candidates1(int nsrc, FgCells S, const double *mask, FgBins b, const int *slot_start, const FgBinEntry *entries, int ecap,
                     FgPairSpace ps, int *pair_beg, int *pair_cnt, const int *heavy_list, const int *heavy_cnt, int *big_list, int *big_cnt,
                     hipStream_t st)
{
  if (nsrc <= 0) return;
  const int nbR = nblk((long)nsrc * CAND_G, 64);
  // (as in fgd_candidates_rect, but up to eight times the waves: a curvilinear target that contains a pole -- a polar tile of a cubed
  // sphere -- lists a fifth of a lat-lon source grid's cells; 0.25 deg -> C384 tile 3: tile 2.8 -> 2.07 ms; 8192 waves: 2.20)
  const int H = min(8 * HEAVY_BLOCKS, max(64, nblk(nsrc, 8)));
  k_candidates1<<<nbR + H, 64, 0, st>>>(nsrc, H, S, mask, b, slot_start, entries, ecap, ps, pair_beg, pair_cnt, heavy_list, heavy_cnt, big_list, big_cnt);
}

void fgd_clip_quad(int order, FgPairSpace ps, FgCells S, const double *mask, FgCells D,
                   double *tmp_area, double *tmp_clon, double *tmp_clat, int *nacc, int *defer_list, int *defer_cnt,
                   unsigned long long *stats, unsigned *err, hipStream_t st, const FgRect *rect, int *row_cnt, int *tmp_rowpos)
{
  const long np = fgd_pairs_total(ps);
  if (np <= 0) return;
  const FgRect R = rect ? *rect : FgRect{};
  const int g = nblk(np, CLIP_THREADS);
#define FG_LAUNCH_QUAD(O, RC, QS) k_clip_quad<O, RC, QS><<<g, CLIP_THREADS, 0, st>>>(ps, S, mask, D, R, tmp_area, tmp_clon, tmp_clat, nacc, defer_list, defer_cnt, stats, err, row_cnt, tmp_rowpos)
  const bool qsrc = rect && S.vstride == FG_VSTRIDE_QUAD;    // compact source cells: a grid on the rectilinear path
  if (order == 2) { if (qsrc) FG_LAUNCH_QUAD(2, true, true); else if (rect) FG_LAUNCH_QUAD(2, true, false); else FG_LAUNCH_QUAD(2, false, false); }
  else            { if (qsrc) FG_LAUNCH_QUAD(1, true, true); else if (rect) FG_LAUNCH_QUAD(1, true, false); else FG_LAUNCH_QUAD(1, false, false); }
#undef FG_LAUNCH_QUAD
}

void fgd_clip_general(int order, FgPairSpace ps, FgCells S, const double *mask, FgCells D,
                      double *tmp_area, double *tmp_clon, double *tmp_clat, int *nacc, int *defer_list, int *defer_cnt,
                      unsigned long long *stats, unsigned *err, hipStream_t st, const FgRect *rect, int *row_cnt, int *tmp_rowpos)
{
  const long np = fgd_pairs_total(ps);
  if (np <= 0) return;
  int grid = nblk(np, GEN_THREADS); if (grid > 1024) grid = 1024;
  const FgRect R = rect ? *rect : FgRect{};
#define FG_LAUNCH_GEN(O, RC) k_clip_general<O, RC><<<grid, GEN_THREADS, 0, st>>>(defer_list, defer_cnt, ps.src, ps.dst, S, mask, D, R, tmp_area, tmp_clon, tmp_clat, nacc, stats, err, row_cnt, tmp_rowpos)
  if (order == 2) { if (rect) FG_LAUNCH_GEN(2, true); else FG_LAUNCH_GEN(2, false); }
  else            { if (rect) FG_LAUNCH_GEN(1, true); else FG_LAUNCH_GEN(1, false); }
#undef FG_LAUNCH_GEN
}

// ---- rectilinear destination grid
void fgd_rect_tables(const double *lon, const double *lat, int nx, int ny, double *hdr, double *lat_ax, double *lon_ax, double *col,
                     double *col_min, double *col_max, double *col_avg, double *row, unsigned *bad, unsigned *err, hipStream_t st, double dst_tlon)
{
  const long np = (long)(nx + 1) * (ny + 1);
  const int nbT = (std::max(nx, ny) + 1 + 255) / 256;      // (as the kernel counts them)
  const int nbV = (int)std::min<long>(RECT_VERIFY_BLOCKS, std::max<long>((np + 255) / 256, 1));
  k_rect_tables<<<nbT + nbV, 256, 0, st>>>(lon, lat, nx, ny, hdr, lat_ax, lon_ax, col, col_min, col_max, col_avg, row, bad, err, dst_tlon);
}
void fgd_cell_struct2r(const FgTileSet &ts, const FgTile *tiles_in, FgTile *tiles_out, int ntiles, int nsrc, int ndst, FgCells S, double *area_out,
                       FgRect R, const double *mask, int order, int *src_idx_f, double *sums, unsigned *err, hipStream_t st,
                       unsigned long long *band_keys, int cull, int *heavy_list, int *heavy_cnt, int *rare_list, int *rare_cnt, FgPairSpace ps,
                       int *pair_beg, int *pair_cnt, int *big_list, int *big_cnt)
{
  const int nbS = nblk(nsrc, 256), nbD = nblk(ndst, 256);
  if (nbS + nbD > 0)
    k_cell_struct2r<<<nbS + nbD, 256, 0, st>>>(ts, tiles_in, tiles_out, ntiles, nsrc, ndst, nbS, S, area_out, R, mask, order, src_idx_f, sums, err,
                                               band_keys, cull, heavy_list, heavy_cnt, rare_list, rare_cnt, ps, pair_beg, pair_cnt, big_list, big_cnt);
}
void fgd_polylist_records(FgPolyList P, FgCells S, int *src_idx_f, double *sums, const FgRect *rect, int *heavy_list, int *heavy_cnt,
                          unsigned *err, hipStream_t st)
{
  if (P.npoly > 0)
    k_polylist_records<<<nblk(P.npoly, 256), 256, 0, st>>>(P, S, src_idx_f, sums, rect ? *rect : FgRect{}, rect ? 1 : 0, heavy_list, heavy_cnt, err);
}
void fgd_rect_materialize(int ndst, FgRect R, FgCells D, hipStream_t st)
{
  if (ndst > 0) k_rect_materialize<<<nblk(ndst, 256), 256, 0, st>>>(ndst, R, D);
}
void fgd_quad_materialize(int nsrc, FgCells S, double *lon_min, double *lon_max, double *verts, hipStream_t st)
{
  if (nsrc > 0) k_quad_materialize<<<nblk(nsrc, 256), 256, 0, st>>>(nsrc, S, lon_min, lon_max, verts);
}
void fgd_candidates_rect(int nsrc, FgCells S, const double *mask, FgRect R, FgPairSpace ps, int *pair_beg, int *pair_cnt,
                         const int *heavy_list, const int *heavy_cnt, int *big_list, int *big_cnt, hipStream_t st, int listed_only,
                         const int *rare_list, const int *rare_cnt, unsigned *err, double *sums)
{
  if (nsrc <= 0) return;
  const int nbR = listed_only ? 0 : nblk(nsrc, 64);       // listed_only: the record kernel made the candidates of the other cells
  // waves for the listed cells: on a coarse source grid over a fine target EVERY cell is listed (C48 -> 0.25 deg: 13 824 cells; with
  // nsrc / 64 = 216 waves the candidates took 0.24 ms, with nsrc / 8 0.064 -- dealing a cell's (row, column) pairs to all 64 lanes
  // through LDS instead of a lane per column made no difference on top of that)
  const int H = min(HEAVY_BLOCKS, max(64, nblk(nsrc, 8)));
  // listed_only = behind k_cell_struct2r: the instantiation that also finishes the cells of rare_list
  // (its 174 VGPRs let two waves share a SIMD, 2048 on the chip: the rare-cell blocks come out of H, not on top of it)
  const int Hf = max(H - RARE_BLOCKS, RARE_BLOCKS);
  if (listed_only) k_candidates_rect<true><<<Hf + RARE_BLOCKS, 64, 0, st>>>(nsrc, Hf, S, mask, R, ps, pair_beg, pair_cnt, heavy_list, heavy_cnt, big_list, big_cnt,
                                                          rare_list, rare_cnt, err, sums);
  else k_candidates_rect<false><<<nbR + H, 64, 0, st>>>(nsrc, H, S, mask, R, ps, pair_beg, pair_cnt, heavy_list, heavy_cnt, big_list, big_cnt,
                                                       nullptr, nullptr, nullptr, nullptr);
}

void fgd_compact(int order, int nsrc, FgPairSpace ps, const FgCompactIo &io, hipStream_t st)
{
  if (nsrc <= 0) return;
  const long np = fgd_pairs_total(ps);
  if (order == 2) k_compact<2><<<BIG_BLOCKS + nblk(np, 256), 256, 0, st>>>(nsrc, ps, io);
  else            k_compact<1><<<BIG_BLOCKS + nblk(np, 256), 256, 0, st>>>(nsrc, ps, io);
}

void fgd_centroids(int nsrc, FgCells S, const double *sums, FgSrcRec *cen, hipStream_t st)
{
  if (nsrc > 0) k_centroids<<<nblk(nsrc, 256), 256, 0, st>>>(nsrc, S, sums, cen);
}

void fgd_distances(long nx, const int *x_src, const double *x_area, const FgSrcRec *cen, double *x_c1, double *x_c2, hipStream_t st)
{
  if (nx > 0) k_distances<<<nblk(nx, 256), 256, 0, st>>>(nx, x_src, x_area, cen, x_c1, x_c2);
}

// total[3][nsrc] += this plan's exchange cells, cell by cell in exchange-cell order, CONTINUING from the value already there:
// conserve_interp.c:203-221 adds the gathered exchange cells of all ranks (and of one output tile after the other) one by one
// "for the purpose of bitwise reproducing"; a running total handed from plan to plan (and from rank to rank for the cells cut by a
// band boundary) performs the same additions in the same order.  cells == null: all source cells.
__global__ __launch_bounds__(256) void k_accumulate_cell_sums(int n, const int *cells, int nsrc, const int *xoff, const double *xa,
                                                               const double *c1, const double *c2, double *total)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = cells ? cells[i] : i;
  if (s < 0 || s >= nsrc) return;
  const int b = xoff[s], e = xoff[s + 1];
  if (b >= e) return;
  double a0 = total[s], a1 = total[(size_t)nsrc + s], a2 = total[2 * (size_t)nsrc + s];
  for (int q = b; q < e; q++) { a0 += xa[q]; a1 += c1[q]; a2 += c2[q]; }
  total[s] = a0; total[(size_t)nsrc + s] = a1; total[2 * (size_t)nsrc + s] = a2;
}
void fgd_accumulate_cell_sums(int n, const int *cells, int nsrc, const int *xoff, const double *xa, const double *c1, const double *c2,
                              double *total, hipStream_t st)
{
  if (n > 0) k_accumulate_cell_sums<<<(n + 255) / 256, 256, 0, st>>>(n, cells, nsrc, xoff, xa, c1, c2, total);
}
