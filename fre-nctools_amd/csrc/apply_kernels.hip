// apply_kernels.hip -- the weight-apply sweep (do_scalar_conserve_interp) as a CSR
// SpMV-style gather on gfx950, plus the kernels that build the CSR layout.
//
// The reference scatters  out[dst] += (f[src] + gx*di + gy*dj) * area  sequentially over
// the exchange cells (tools/fregrid/conserve_interp.c:593-614, :785-811) and then divides
// by the accumulated area (:831-839).  Sorting the exchange cells by destination cell with
// a STABLE order (ascending exchange-cell index inside a row) turns that into one private
// sum per destination cell that adds in exactly the reference's order -- no FP atomics and
// bitwise the same result as the serial reference for the same weights.
//
// HBM-bound: per level the kernel streams the CSR entries (32 B each for order 2) and
// gathers 8..24 B per entry from the source fields (L2/Infinity-Cache resident).
#include "xgrid_device.h"
#include <type_traits>

static inline int nblk(long n, int t) { return (int)((n + t - 1) / t); }

__global__ __launch_bounds__(256) void k_csr_count(long nx, const int *x_dst, int *row_cnt)
{
  long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n < nx) atomicAdd(&row_cnt[x_dst[n]], 1);
}

// Slot of every exchange cell in its destination row.  Exchange cells are ordered by source cell, so in a fine -> coarse remap
// long runs of consecutive cells fall into the same row (C768 -> 1 deg: ~8): one atomic per run of equal rows within a wave
// instead of one per cell (the per-cell version spent 0.4 ms there on same-address atomics); the cells of a run take
// consecutive slots in ascending order.  The entry stored is the pair {exchange cell, its source cell} (x_src[n], read here
// beside x_dst[n]: coalesced).
__global__ __launch_bounds__(256) void k_csr_fill(long nx, const int *x_src, const int *x_dst, const int *row_ptr, int *row_fill, FgRowEnt *perm)
{
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int d = (n < nx) ? x_dst[n] : -1;
  const int s = (n < nx) ? x_src[n] : 0;
  const int prev = __shfl_up(d, 1);
  const bool head = (lane == 0) || (d != prev);
  const unsigned long long heads = __ballot(head);
  const int start = 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));     // head of this lane's run
  const unsigned long long above = (start == 63) ? 0ull : (heads & ~((2ull << start) - 1ull));
  const int end = above ? (__ffsll((long long)above) - 1) : 64;
  int base = 0;
  if (lane == start && d >= 0) base = atomicAdd(&row_fill[d], end - start);
  base = __shfl(base, start);
  if (d >= 0) perm[row_ptr[d] + base + (lane - start)] = FgRowEnt{(int)n, s};
}

// the same with slots already taken while the search compacted its exchange cells (k_compact): no atomics.  Launched for
// the capacity of the exchange-cell arrays when the host does not know the count yet (nx_dev)
__global__ __launch_bounds__(256) void k_csr_fill_pos(long nx, const unsigned long long *nx_dev, const int *x_src, const int *x_dst,
                                                       const int *row_ptr, const int *x_rowpos, FgRowEnt *perm)
{
  if (nx_dev) { const unsigned long long nd = *nx_dev; if (nd < (unsigned long long)nx) nx = (long)nd; }
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n < nx) { const int s = x_src[n]; perm[row_ptr[x_dst[n]] + x_rowpos[n]] = FgRowEnt{(int)n, s}; }
}

// Rows of `perm` into ascending exchange-cell order, then the packed CSR records -- one kernel.  An entry of perm is the pair
// {exchange cell n, its source cell s}: the rows are ordered by n and s moves with it, so that the record loop knows both
// addresses of an entry at once.  A block owns RPW consecutive rows, i.e. one contiguous run of perm: it is staged in LDS (the
// exchange cells in sh, the source cells in shs), every lane sorts its own row there by insertion (rows are short when the grids
// are of similar resolution, ~4 entries); rows longer than SHORT (fine -> coarse remaps: 50-1000 entries) are sorted by the whole
// wave, every lane placing its elements at their rank (the exchange-cell numbers are distinct).  The lanes hold their elements
// in registers while the ranks are counted, so after a barrier the placement goes back into sh / shs themselves: no landing
// buffer, and the LDS a block needs is what it was when the lists held the exchange cell alone.  The records then leave in one
// coalesced sweep over the run.  RPW = 64 when rows are short, 16 when the mean row is long, so that four times as many waves
// are in flight.  Runs beyond the staging capacity are sorted in place in global memory.
// DIST (order 2): x_c1/x_c2 still hold the centroid integrals; di = clon/area - cen_lon, dj = clat/area - cen_lat
// (conserve_interp.c:256-257,355-356) are formed here, the operations k_distances applies to the arrays themselves.
// rank[k] += number of keys[0..n) below v[k]: one walk over the keys (LDS) for N values -- a walk per value waits for LDS once
// per comparison
template <int N>
__device__ __forceinline__ void d_rank_count(const int *keys, int n, const int (&v)[N], int (&rank)[N])
{
  int j = 0;
  for (; j + 4 <= n; j += 4) {
    const int x0 = keys[j], x1 = keys[j + 1], x2 = keys[j + 2], x3 = keys[j + 3];
#pragma unroll
    for (int k = 0; k < N; k++) rank[k] += ((x0 < v[k]) ? 1 : 0) + ((x1 < v[k]) ? 1 : 0) + ((x2 < v[k]) ? 1 : 0) + ((x3 < v[k]) ? 1 : 0);
  }
  for (; j < n; j++) {
    const int x = keys[j];
#pragma unroll
    for (int k = 0; k < N; k++) rank[k] += (x < v[k]) ? 1 : 0;
  }
}

// A packed CSR record to its place with non-temporal 16-byte stores.  The finalize writes every record once and reads none, while
// the lines of x_area / x_c1 / x_c2 are shared by the gathers of neighbouring rows: at C384 -> 0.25 deg (133 MB of records)
// k_csr_sortgather takes 103.4 us with ordinary stores and 96.7 us with these (profiles/csr_row_pairs_summary.md).
template <typename E>
__device__ __forceinline__ void d_store_stream(E *dst, const E &e)
{
  typedef int v4i __attribute__((ext_vector_type(4)));
  static_assert(sizeof(E) % 16 == 0 && alignof(E) >= 8, "records are whole 16-byte words");
  v4i w[sizeof(E) / 16];
  __builtin_memcpy(w, &e, sizeof(E));
#pragma unroll
  for (unsigned k = 0; k < sizeof(E) / 16; k++) __builtin_nontemporal_store(w[k], (v4i *)dst + k);
}

// The records of a block's run of perm (nq entries from q0; STAGED: sorted in LDS, else in perm itself): G entries per lane and
// pass.  An entry names its exchange cell and its source cell, so all its loads go out in ONE round: area (order 2: and the two
// integrals) by exchange cell; the field index and (DIST) the centroid record of k_centroids by source cell.  Entries past the
// run's end repeat the pass's first one and store nothing.  Per entry the operations are those of a one-entry loop, in the same
// order.  (STAGED is a template constant: chosen per load, LDS or global memory, the index reads become flat loads, which are
// waited for one by one.)
template <int ORDER, bool DIST, int BT, int G, bool STAGED>
__device__ __forceinline__ void d_csr_records(const int *sh, const int *shs, const FgRowEnt *perm, int q0, int nq, const double *x_area,
                                              const double *x_c1, const double *x_c2, const int *src_idx_f, const FgSrcRec *cen,
                                              const FgCsr &csr)
{
  for (int i0 = threadIdx.x; i0 < nq; i0 += BT * G) {
    int n[G], s[G], idx[G];
    double ar[G], c1[G], c2[G], cl[G], ct[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const int i = i0 + BT * g, ic = (i < nq) ? i : i0;
      if (STAGED) { n[g] = sh[ic]; s[g] = shs[ic]; }
      else { const FgRowEnt p = perm[q0 + ic]; n[g] = p.n; s[g] = p.s; }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
      ar[g] = x_area[n[g]];
      if (ORDER == 2) { c1[g] = x_c1[n[g]]; c2[g] = x_c2[n[g]]; }
      idx[g] = src_idx_f[s[g]];
      if (ORDER == 2 && DIST) { const FgSrcRec r = cen[s[g]]; cl[g] = r.cen_lon; ct[g] = r.cen_lat; }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
      const int i = i0 + BT * g;
      if (ORDER == 2) {
        FgCsrEntry2 E;
        E.idx_f = idx[g]; E.idx_g = s[g]; E.area = ar[g];
        if (DIST) {
          double di = c1[g] / E.area, dj = c2[g] / E.area;
          di -= cl[g]; dj -= ct[g];
          E.di = di; E.dj = dj;
        } else { E.di = c1[g]; E.dj = c2[g]; }
        if (i < nq) d_store_stream(&csr.e2[q0 + i], E);
      } else {
        FgCsrEntry1 E;
        E.idx_f = idx[g]; E.pad = 0; E.area = ar[g];
        if (i < nq) d_store_stream(&csr.e1[q0 + i], E);
      }
    }
  }
}

// lane-serial insertion of the row [b, e) of perm (global memory), ordered by exchange cell
__device__ __forceinline__ void d_row_insertion(FgRowEnt *perm, int b, int e)
{
  for (int i = b + 1; i < e; i++) {
    const FgRowEnt v = perm[i];
    int j = i - 1;
    while (j >= b && perm[j].n > v.n) { perm[j + 1] = perm[j]; j--; }
    perm[j + 1] = v;
  }
}

// entries per lane and pass of the record loop.  2 and 4 take the same time on C384 -> 0.25 deg, with an entry's loads in two
// dependent rounds (113.4 / 113.1 us, 117.9 with one: profiles/compact_finalize_loads_summary.md) and in one (101.3 / 102.1 us:
// profiles/csr_row_pairs_summary.md); 4 costs the DIST kernels registers and cost the finalize of a coarse -> fine plan 4-7 us
// (C96 -> 0.25 deg: 54 us with 2, 62 with 4, 59 with one)
#define SG_GROUP 2
template <int ORDER, int RPW, bool DIST, int BT, int G>
__global__ __launch_bounds__(BT) void k_csr_sortgather(int ndst, FgRowEnt *perm, const double *x_area, const double *x_c1, const double *x_c2,
                                                        const int *src_idx_f, const FgSrcRec *cen, FgCsr csr, int *tmp, long ntmp)
{
  constexpr int SHORT = 12, CAP = (RPW >= 64) ? 512 : 2048;                // 4 KB of LDS per wave in the short-row case
  // (BT: 64 lanes for 64 short rows; 256 for 16 long rows -- their ~1000 records leave through gathers, and with one wave that
  // was 18 rounds of them per block: C384 -> 2 deg finalize 0.186 ms)
  __shared__ int sh[CAP], shs[CAP];                        // exchange cells (the sort key) and their source cells
  __shared__ int long_b[RPW], long_n[RPW];
  __shared__ int nlong;
  if (threadIdx.x == 0) nlong = 0;
  __syncthreads();
  const int d0 = blockIdx.x * RPW, d1 = min(d0 + RPW, ndst);
  const int q0 = csr.row_ptr[d0], q1 = csr.row_ptr[d1], nq = q1 - q0;
  const bool staged = nq <= CAP;
  const int d = d0 + threadIdx.x;
  int b = 0, e = 0;
  if ((int)threadIdx.x < RPW && d < ndst) { b = csr.row_ptr[d]; e = csr.row_ptr[d + 1]; }
  if (staged) {
    for (int i = threadIdx.x; i < nq; i += BT) { const FgRowEnt p = perm[q0 + i]; sh[i] = p.n; shs[i] = p.s; }
    __syncthreads();
    if (e - b > SHORT) { const int q = atomicAdd(&nlong, 1); long_b[q] = b - q0; long_n[q] = e - b; }
    else
      for (int i = b - q0 + 1; i < e - q0; i++) {
        const int v = sh[i], w = shs[i];
        int j = i - 1;
        while (j >= b - q0 && sh[j] > v) { sh[j + 1] = sh[j]; shs[j + 1] = shs[j]; j--; }
        sh[j + 1] = v; shs[j + 1] = w;
      }
    __syncthreads();
    const int nl = nlong;
    for (int q = 0; q < nl; q++) {
      const int rb = long_b[q], n = long_n[q];
      // every lane ranks up to CAP / BT = 8 elements of the row in ONE walk over its keys (a walk per element waits for LDS
      // once per comparison: 0.82 ms for the 1 850-entry rows of C384 -> 10 deg).  The elements stay in registers over the
      // barrier that ends every lane's walk; then they go to their ranks in the row itself.
      constexpr int OWN = CAP / BT;
      if (n <= BT) {                                       // (block-uniform) one element per lane at most
        const bool own = (int)threadIdx.x < n;
        int v = 0, w = 0, rank = 0;
        if (own) {
          v = sh[rb + threadIdx.x]; w = shs[rb + threadIdx.x];
          for (int j = 0; j < n; j++) rank += (sh[rb + j] < v) ? 1 : 0;
        }
        __syncthreads();
        if (own) { sh[rb + rank] = v; shs[rb + rank] = w; }
      } else {
        int v[OWN], w[OWN], rank[OWN];
#pragma unroll
        for (int k = 0; k < OWN; k++) {
          const int i = threadIdx.x + BT * k;
          v[k] = (i < n) ? sh[rb + i] : 0x7fffffff; w[k] = (i < n) ? shs[rb + i] : 0; rank[k] = 0;
        }
        d_rank_count<OWN>(sh + rb, n, v, rank);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < OWN; k++) if ((int)threadIdx.x + BT * k < n) { sh[rb + rank[k]] = v[k]; shs[rb + rank[k]] = w[k]; }
      }
      __syncthreads();
    }
  } else {
    // beyond the staging capacity: per row in global memory (lane-serial insertion, or the wave through LDS for long rows)
    if (e - b > SHORT) { const int q = atomicAdd(&nlong, 1); long_b[q] = b; long_n[q] = e - b; }
    else d_row_insertion(perm, b, e);
    __syncthreads();
    const int nl = nlong;
    for (int q = 0; q < nl; q++) {
      const int rb = long_b[q], n = long_n[q];
      if (n <= CAP) {
        for (int i = threadIdx.x; i < n; i += BT) { const FgRowEnt p = perm[rb + i]; sh[i] = p.n; shs[i] = p.s; }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += BT) {
          const int v = sh[i];
          int rank = 0;
          for (int j = 0; j < n; j++) rank += (sh[j] < v) ? 1 : 0;
          perm[rb + rank] = FgRowEnt{v, shs[i]};
        }
        __syncthreads();
      } else if (tmp) {
        // a row longer than the staging buffer (C384 -> 10 deg: 1 850 exchange cells): its keys pass through LDS a buffer-full at
        // a time, every element counts the smaller keys of each tile into its rank (kept in the last third of tmp), then the
        // row's pairs are written out in rank order (first two thirds of tmp) and copied back.  (Until round 3 one lane sorted
        // such a row by insertion, in global memory: 1.9 SECONDS for that remap's finalize.)
        FgRowEnt *srt = (FgRowEnt *)tmp + rb;
        int *rk = tmp + 2 * ntmp + rb;
        for (int t0 = 0; t0 < n; t0 += CAP) {
          const int m = min(CAP, n - t0);
          for (int j = threadIdx.x; j < m; j += BT) sh[j] = perm[rb + t0 + j].n;
          __syncthreads();
          for (int i0 = threadIdx.x; i0 < n; i0 += 8 * BT) {           // eight elements per lane and walk over the tile
            int v[8], r[8];
#pragma unroll
            for (int k = 0; k < 8; k++) { const int i = i0 + BT * k; v[k] = (i < n) ? perm[rb + i].n : 0x7fffffff; r[k] = (i < n && t0) ? rk[i] : 0; }
            d_rank_count<8>(sh, m, v, r);
#pragma unroll
            for (int k = 0; k < 8; k++) { const int i = i0 + BT * k; if (i < n) rk[i] = r[k]; }
          }
          __syncthreads();
        }
        for (int i = threadIdx.x; i < n; i += BT) srt[rk[i]] = perm[rb + i];
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += BT) perm[rb + i] = srt[i];
        __syncthreads();
      } else if (threadIdx.x == 0) d_row_insertion(perm, rb, rb + n);   // serial, as a last resort (no scratch: the plan's mean row is short)
    }
    __syncthreads();
  }
  if (staged) d_csr_records<ORDER, DIST, BT, G, true>(sh, shs, perm, q0, nq, x_area, x_c1, x_c2, src_idx_f, cen, csr);
  else        d_csr_records<ORDER, DIST, BT, G, false>(sh, shs, perm, q0, nq, x_area, x_c1, x_c2, src_idx_f, cen, csr);
}

// index of source cell s inside one level of the field array: order 1 fields have no halo
// (index == s); order 2 fields carry a 1-cell halo per tile (fregrid_util.c:2137-2145)
__global__ __launch_bounds__(256) void k_src_field_index(int order, const FgTile *tiles, int ntiles, int nsrc, int *src_idx_f)
{
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsrc) return;
  if (order != 2) { src_idx_f[s] = s; return; }
  int t = 0, foff = 0;
  while (t + 1 < ntiles && s >= tiles[t + 1].cell_off) { foff += (tiles[t].nx + 2) * (tiles[t].ny + 2); t++; }
  int loc = s - tiles[t].cell_off;
  int i = loc % tiles[t].nx, j = loc / tiles[t].nx;
  src_idx_f[s] = foff + (j + 1) * (tiles[t].nx + 2) + i + 1;
}

// Block -> destination-row mapping.  The hardware deals blocks round-robin over the 8 XCDs (block b runs on XCD b % 8), each
// with its own 4 MiB L2.  With the identity mapping the blocks resident on one XCD hold every 8th run of 64 rows, so two
// destination rows that are neighbours in latitude -- they gather the same source records -- never share an L2.  g_xcd_band:
// XCD x sweeps ONE contiguous band of rows (tile = start_x + b / 8), so that its ~160 resident blocks cover ~7 adjacent grid
// rows and the second use of a source record is an L2 hit.  (PMC, round 2: the identity mapping reads 538 MB per launch through
// the fabric where the algorithm needs 303 MB; TCC hit rate 41 %.)  Measured (scripts/apply_ab.py, same box, 8 levels on records):
// identity 0.096 ms, banded 0.110 ms -- slower although it re-reads less: the second and third XCD that need a record find it in
// the Infinity Cache (the fabric counters count those hits, HBM does not see them), and eight bands stream eight separate windows
// of the CSR.  The identity mapping stays the default; fg_set_apply_xcd(1) selects the banded one.  Non-temporal stores of the
// output changed nothing.
__device__ __forceinline__ int d_xcd_block(int b, int nb, int band)
{
  if (!band) return b;
  if (band == 1) {
    const int x = b & 7, k = b >> 3, q = nb >> 3, r = nb & 7;
    return x * q + min(x, r) + k;                     // XCD x owns q + (x < r) consecutive tiles
  }
  // band = C >= 2: chunks of C consecutive tiles go to one XCD, chunks round-robin over the XCDs: neighbouring rows share an L2
  // (a chunk spans several grid rows) while all eight XCDs still sweep the same window of the arrays at any time
  const int C = band, per = 8 * C, full = nb / per * per;
  if (b >= full) return b;
  const int x = b & 7, k = b >> 3;
  return ((k / C) * 8 + x) * C + (k % C);
}

// ------------------------------------------------------------------- the pieces every entry-parallel sweep kernel is made of
// A tile of ROWS destination rows owns one contiguous run [q0, q1) of CSR records and walks it in chunks of CAP: a chunk is staged
// in LDS (ep_stage_*), every lane takes its exchange cells' records into registers and issues their gathers in one round, the
// buffer becomes the table of products, and the lane of each row -- or of each (row, level) -- adds its part of the chunk in CSR
// order (ep_row_add), carrying its sums from chunk to chunk; apply_finish turns the sums into the output value.
template <int ORDER> using CsrEntry = typename std::conditional<ORDER == 2, FgCsrEntry2, FgCsrEntry1>::type;
template <int ORDER> __device__ __forceinline__ const CsrEntry<ORDER> *csr_entries(const FgCsr &csr)
{
  if constexpr (ORDER == 2) return csr.e2; else return csr.e1;
}
typedef unsigned int u4v __attribute__((ext_vector_type(4)));

// The tile's run of records and this lane's row [b, e): LPR lanes per row, lane t serves row d0 + t / LPR at level t % LPR
// (LPR = 1: a lane per row); lanes past ROWS * LPR serve none (lane == false, b == e == 0).
struct EpTile { int q0, q1, d, lev, b, e; bool lane; };
template <int ROWS, int LPR>
__device__ __forceinline__ EpTile ep_tile(const FgCsr &csr, int ndst, int tile)
{
  EpTile T;
  const int t = threadIdx.x;
  const int d0 = tile * ROWS, dl = min(d0 + ROWS, ndst);
  T.q0 = csr.row_ptr[d0]; T.q1 = csr.row_ptr[dl];
  T.lane = t < ROWS * LPR;
  T.d = d0 + t / LPR; T.lev = t % LPR;
  const int dc = min(T.d, ndst - 1);
  T.b = 0; T.e = 0;
  if (T.lane) { T.b = csr.row_ptr[dc]; T.e = csr.row_ptr[dc + 1]; }
  return T;
}

// n <= CAP records src[0 .. n) -> sh_e with coalesced 16-byte loads, non-temporal as in k_apply_il (the CSR records are used once
// per launch).
// Unrolled form (the one-level kernels): every 16-byte word of the chunk in flight at once (a loop would wait for each load before
// it issues the next), no branches around the loads.
template <int TPB, int CAP, typename Entry>
__device__ __forceinline__ void ep_stage_unrolled(Entry *sh_e, const Entry *src, int n)
{
  constexpr int W = sizeof(Entry) / 16, WPL = CAP * W / TPB;
  const int t = threadIdx.x, nw = n * W;
  const u4v *g = reinterpret_cast<const u4v *>(src);
  u4v *l = reinterpret_cast<u4v *>(sh_e);
  u4v w[WPL];
#pragma unroll
  for (int j = 0; j < WPL; j++) w[j] = __builtin_nontemporal_load(g + min(t + TPB * j, nw - 1));
#pragma unroll
  for (int j = 0; j < WPL; j++) if (t + TPB * j < nw) l[t + TPB * j] = w[j];
}
// Loop form (the 8-level kernels).
template <int TPB, typename Entry>
__device__ __forceinline__ void ep_stage_loop(Entry *sh_e, const Entry *src, int n)
{
  constexpr int W = sizeof(Entry) / 16;
  const u4v *g = reinterpret_cast<const u4v *>(src);
  u4v *l = reinterpret_cast<u4v *>(sh_e);
  for (int i = threadIdx.x; i < n * W; i += TPB) l[i] = __builtin_nontemporal_load(g + i);
}

// What one staged exchange cell adds to a row: the product value * area, the area, and whether it counts as touched.  A cell the
// reference skips with `continue` holds +0.0, +0.0, 0: x + 0.0 == x bit for bit here (no sum is ever -0.0: they start at +0.0).
struct EpTerm { double p, a; unsigned ok; };
// The row lane's part of the chunk [c0, c0 + n): the cells of row [b, e) in it, added in CSR order; term(q) reads cell q of the
// chunk from LDS.
template <typename F>
__device__ __forceinline__ void ep_row_add(int b, int e, int c0, int n, double &acc, double &asum, unsigned &touched, F term)
{
  const int qa = max(b, c0) - c0, qb = min(e, c0 + n) - c0;
  int q = qa;
  for (; q + 8 <= qb; q += 8) {                            // (long rows: eight LDS reads in flight, then the adds in CSR order)
    EpTerm c[8];
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = term(q + k);
#pragma unroll
    for (int k = 0; k < 8; k++) { acc += c[k].p; asum += c[k].a; touched |= c[k].ok; }
  }
  for (; q < qb; q++) { const EpTerm c = term(q); acc += c.p; asum += c.a; touched |= c.ok; }
}

// conserve_interp.c:815-839: the row's sums -> its global-sum term (rs) and its output value
__device__ __forceinline__ double apply_finish(double acc, double asum, bool touched, double missing, double &rs)
{
  rs = (asum > 0) ? acc : 0.0;                                 // :815-819
  if (asum > 0) return acc / asum;                             // :831-839
  return touched ? 0.0 : missing;
}
// the same with cell_methods = sum (:821-830) and --target_grid (asum_t: the plain exchange-cell areas of row d)
__device__ __forceinline__ double apply_finish_ex(const FgApplyEx &o, int d, double acc, double asum, double asum_t, bool touched, double &rs)
{
  if (o.sum) {
    rs = (asum > 0) ? acc : 0.0;
    return (asum == 0) ? (touched ? 0.0 : o.missing) : acc;
  }
  double r = apply_finish(acc, asum, touched, o.missing, rs);
  if (o.cell_area_out && r != o.missing) r *= (asum_t / o.cell_area_out[d]);
  return r;
}

// Single level, level-major fields (also the has_missing path): one thread per destination cell.
template <int ORDER, bool MISSING>
__global__ __launch_bounds__(256) void k_apply1(int ndst, FgCsr csr, const double *f, const double *px, const double *py,
                                                 const int *gmask, double missing, double *out, double *row_sum)
{
  int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= ndst) return;
  int b = csr.row_ptr[d], e = csr.row_ptr[d + 1];
  double acc = 0.0, asum = 0.0;
  int touched = 0;
  for (int q = b; q < e; q++) {
    double a, v;
    if (ORDER == 2) {
      const FgCsrEntry2 E = csr.e2[q];
      a = E.area; v = f[E.idx_f];
      if (MISSING) { if (v == missing) continue; }
      bool flatgrad = false;
      if (MISSING) flatgrad = gmask[E.idx_g] != 0;
      if (!flatgrad) v = (v + px[E.idx_g] * E.di + py[E.idx_g] * E.dj);
    } else {
      const FgCsrEntry1 E = csr.e1[q];
      a = E.area; v = f[E.idx_f];
      if (MISSING) { if (v == missing) continue; }
    }
    acc += v * a;
    asum += a;
    touched = 1;
  }
  double rs;
  const double r = apply_finish(acc, asum, touched != 0, missing, rs);
  if (row_sum) row_sum[d] = rs;
  out[d] = r;
}

// The single-level sweep as fregrid's level loop calls it (fregrid.c:1045-1061: get_input_data, do_scalar_conserve_interp(..., 1),
// write_field_data per level; also every field with missing values), entry-parallel like k_apply_ep8: a tile of ROWS rows walks
// its run of CSR records in chunks of CAP: the chunk is staged with coalesced loads, a lane per exchange cell issues the chunk's
// gathers (field, two gradients, the gradient mask) in one round, the products area * (f + gx di + gy dj) go to LDS and the lane
// of each row adds its part of the chunk in CSR order, carrying its sums from chunk to chunk -- so a row may be as long as it
// likes (fine -> coarse remaps: ROWS shrinks with the mean row length, a row of thousands of exchange cells is one tile walking
// many chunks).  An exchange cell whose source value is missing adds +0.0 to both sums (x + 0.0 == x bit for bit) and does not
// count as touched: k_apply1's `continue`.  k_apply1 (a lane walking its row: a record load and a gather round per exchange cell)
// took 0.137 ms for one level of C384 -> 0.25 deg second order -- more than two levels together -- and 0.142 ms for C384 -> 2 deg.
template <int ORDER, bool MISSING, int TPB, int CAP, int ROWS>
__global__ __launch_bounds__(TPB) void k_apply_ep1(int ndst, FgCsr csr, const double *f, const double *px, const double *py, const int *gmask,
                                                    double missing, double *out, double *row_sum, int xcd_band)
{
  typedef CsrEntry<ORDER> Entry;
  constexpr int PASS = CAP / TPB;
  static_assert(ROWS <= TPB && CAP % TPB == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) Entry sh_e[CAP];
  double *sh_p = reinterpret_cast<double *>(sh_e), *sh_a = sh_p + CAP;       // the products take the records' place (2 * 8 <= sizeof(Entry))
  __shared__ unsigned char sh_fl[CAP];
  const int t = threadIdx.x;
  const EpTile T = ep_tile<ROWS, 1>(csr, ndst, d_xcd_block(blockIdx.x, gridDim.x, xcd_band));
  double acc = 0.0, asum = 0.0;
  unsigned touched = 0;
  for (int c0 = T.q0; c0 < T.q1; c0 += CAP) {              // (block-uniform)
    const int n = min(CAP, T.q1 - c0);
    if (c0 > T.q0) __syncthreads();                        // the previous chunk's products have been added
    ep_stage_unrolled<TPB, CAP>(sh_e, csr_entries<ORDER>(csr) + c0, n);
    __syncthreads();
    Entry E[PASS];
    double v[PASS], gxv[PASS], gyv[PASS];
    int gm[PASS];
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      const int i = min(t + TPB * j, n - 1);
      E[j] = sh_e[i]; v[j] = 0.0; gxv[j] = 0.0; gyv[j] = 0.0; gm[j] = 0;
      if (TPB * j < n) {                                    // (block-uniform)
        v[j] = f[E[j].idx_f];
        if constexpr (ORDER == 2) {
          gxv[j] = px[E[j].idx_g]; gyv[j] = py[E[j].idx_g];
          if (MISSING) gm[j] = gmask[E[j].idx_g];
        }
      }
    }
    __syncthreads();                                       // the records are in registers: the buffer becomes the product table
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      const int i = t + TPB * j;
      if (i < n) {
        double val = v[j], a = E[j].area, p;
        unsigned char fl = 1;
        if (MISSING && val == missing) { p = 0.0; a = 0.0; fl = 0; }
        else {
          if constexpr (ORDER == 2) { if (!(MISSING && gm[j] != 0)) val = (val + gxv[j] * E[j].di + gyv[j] * E[j].dj); }
          p = val * a;
        }
        sh_p[i] = p; sh_a[i] = a; sh_fl[i] = fl;
      }
    }
    __syncthreads();
    if (T.lane) ep_row_add(T.b, T.e, c0, n, acc, asum, touched, [&](int q) { return EpTerm{sh_p[q], sh_a[q], sh_fl[q]}; });
  }
  if (!T.lane || T.d >= ndst) return;
  double rs;
  const double r = apply_finish(acc, asum, touched != 0, missing, rs);
  if (row_sum) row_sum[T.d] = rs;
  out[T.d] = r;
}

// NB levels at once, fields interleaved [cell][NB]: every CSR entry is read once for NB levels and
// each gather is NB*8 contiguous bytes (a full 64-byte sector for NB = 8).  A row is served by NB/V
// adjacent lanes, each owning V consecutive levels (V = 2: one 16-byte load per field and entry):
// the lanes of a row read one CSR record (same address, one request) and then one contiguous
// NB*8-byte segment per field, so a wave instruction touches 64*V/NB full segments instead of 64
// scattered lines.  Every (row, level) sum adds in ascending exchange-cell order, exactly the
// reference's order.  No missing values (has_missing requires nz == 1, conserve_interp.c:544).
// Every option of do_scalar_conserve_interp on one level; the per-entry operation order is the reference's
// (weight, then the missing test, then sum / cell_measures scaling) so sums are bit-identical.
// MONO: values come limited from xdata[] (the monotone branch never sets out_miss, :720-739).
template <int ORDER, bool MONO>
__global__ __launch_bounds__(256) void k_apply_ex(int ndst, FgCsr csr, const double *f, const double *px, const double *py,
                                                   FgApplyEx o, double *out, double *row_sum, int *err)
{
  int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= ndst) return;
  int b = csr.row_ptr[d], e = csr.row_ptr[d + 1];
  double acc = 0.0, asum = 0.0, asum_t = 0.0;
  int touched = 0;
  for (int q = b; q < e; q++) {
    double a, v, di = 0, dj = 0;
    int s, jf;
    if (ORDER == 2) { const FgCsrEntry2 E = csr.e2[q]; a = E.area; jf = E.idx_f; s = E.idx_g; di = E.di; dj = E.dj; }
    else            { const FgCsrEntry1 E = csr.e1[q]; a = E.area; jf = E.idx_f; s = E.idx_f; }
    if (o.cell_area_out) {                                       // :845-860 (plain exchange-cell area, no weight)
      if (o.field_area) asum_t += (a * o.field_area[s] / o.cell_area[s]);
      else asum_t += a;
    }
    if (MONO) {
      v = o.xdata[q];
      if (v == o.missing) continue;
      if (o.weight) a *= o.weight[s];
    } else {
      if (o.weight) a *= o.weight[s];
      v = f[jf];
      if (o.has_missing && v == o.missing) continue;
    }
    if (o.sum) a /= o.cell_area[s];
    else if (o.field_area) {
      const double fa = o.field_area[s];
      if (!MONO && o.has_missing && fa == o.area_missing) { atomicOr(err, FG_XERR_AREA_MISSING); continue; }
      a *= (fa / o.cell_area[s]);
    }
    if (ORDER == 2 && !MONO) {
      bool flat = o.has_missing && o.gmask && o.gmask[s] != 0;
      if (!flat) v = (v + px[s] * di + py[s] * dj);
    }
    acc += v * a;
    asum += a;
    if (!MONO) touched = 1;
  }
  double rs;
  const double r = apply_finish_ex(o, d, acc, asum, asum_t, touched != 0, rs);
  if (row_sum) row_sum[d] = rs;
  out[d] = r;
}

// k_apply_ex entry-parallel, the way k_apply_ep1 is k_apply1: per exchange cell the three numbers the row's sums take -- its term of
// the --target_grid area sum (taken before the missing test, as above), the product value * area' and area' (weight, cell_methods /
// cell_measures scaling applied in the reference's order) -- go through LDS, a cell the loop above leaves with `continue` adds +0.0
// to the last two and does not count as touched.  Rows of any length (chunks of CAP records, ROWS rows per tile).
template <int ORDER, bool MONO, int TPB, int CAP, int ROWS>
__global__ __launch_bounds__(TPB) void k_apply_epx(int ndst, FgCsr csr, const double *f, const double *px, const double *py,
                                                    FgApplyEx o, double *out, double *row_sum, int *err, int xcd_band)
{
  typedef CsrEntry<ORDER> Entry;
  constexpr int PASS = CAP / TPB;
  static_assert(ROWS <= TPB && CAP % TPB == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) double sh_raw[CAP * 4];     // CSR records (<= 32 B each), then [3][CAP] products
  Entry *sh_e = reinterpret_cast<Entry *>(sh_raw);
  double *sh_t = sh_raw, *sh_p = sh_raw + CAP, *sh_a = sh_raw + 2 * CAP;
  __shared__ unsigned char sh_fl[CAP];
  const int t = threadIdx.x;
  const EpTile T = ep_tile<ROWS, 1>(csr, ndst, d_xcd_block(blockIdx.x, gridDim.x, xcd_band));
  double acc = 0.0, asum = 0.0, asum_t = 0.0;
  int touched = 0;
  for (int c0 = T.q0; c0 < T.q1; c0 += CAP) {              // (block-uniform)
    const int n = min(CAP, T.q1 - c0);
    if (c0 > T.q0) __syncthreads();
    ep_stage_unrolled<TPB, CAP>(sh_e, csr_entries<ORDER>(csr) + c0, n);
    __syncthreads();
    double tq[PASS], pp[PASS], aa[PASS];
    unsigned char fl[PASS];
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      const int i = min(t + TPB * j, n - 1);
      double a, v, di = 0, dj = 0;
      int s, jf;
      if constexpr (ORDER == 2) { const FgCsrEntry2 E = ((const FgCsrEntry2 *)sh_e)[i]; a = E.area; jf = E.idx_f; s = E.idx_g; di = E.di; dj = E.dj; }
      else                      { const FgCsrEntry1 E = ((const FgCsrEntry1 *)sh_e)[i]; a = E.area; jf = E.idx_f; s = E.idx_f; }
      // every value the cell may need, in one round
      const double wgt = o.weight ? o.weight[s] : 1.0;
      const double ca = (o.sum || o.field_area) ? o.cell_area[s] : 1.0;
      const double fa = o.field_area ? o.field_area[s] : 0.0;
      const double gxv = (ORDER == 2 && !MONO) ? px[s] : 0.0, gyv = (ORDER == 2 && !MONO) ? py[s] : 0.0;
      const int gm = (ORDER == 2 && !MONO && o.has_missing && o.gmask) ? o.gmask[s] : 0;
      v = MONO ? o.xdata[c0 + i] : f[jf];
      double tt = 0.0;
      if (o.cell_area_out) tt = o.field_area ? (a * fa / ca) : a;            // :845-860 (plain exchange-cell area, no weight)
      bool skip = false;
      if (MONO) { if (v == o.missing) skip = true; else if (o.weight) a *= wgt; }
      else { if (o.weight) a *= wgt; if (o.has_missing && v == o.missing) skip = true; }
      if (!skip) {
        if (o.sum) a /= ca;
        else if (o.field_area) {
          if (!MONO && o.has_missing && fa == o.area_missing) { if (t + TPB * j < n) atomicOr(err, FG_XERR_AREA_MISSING); skip = true; }
          else a *= (fa / ca);
        }
      }
      if (!skip && ORDER == 2 && !MONO) { if (gm == 0) v = (v + gxv * di + gyv * dj); }
      tq[j] = tt; pp[j] = skip ? 0.0 : v * a; aa[j] = skip ? 0.0 : a; fl[j] = (skip || MONO) ? 0 : 1;
    }
    __syncthreads();                                       // the records have been read: the buffer becomes the product table
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      const int i = t + TPB * j;
      if (i < n) { sh_t[i] = tq[j]; sh_p[i] = pp[j]; sh_a[i] = aa[j]; sh_fl[i] = fl[j]; }
    }
    __syncthreads();
    if (T.lane) {   // three sums, a plain loop: on ep_row_add (8 reads, then 8 adds) the kernel takes 15-20 VGPRs more, ORDER 2 drops to 6 waves
      const int qa = max(T.b, c0) - c0, qb = min(T.e, c0 + n) - c0;
      for (int q = qa; q < qb; q++) { asum_t += sh_t[q]; acc += sh_p[q]; asum += sh_a[q]; touched |= sh_fl[q]; }
    }
  }
  if (!T.lane || T.d >= ndst) return;
  double rs;
  const double r = apply_finish_ex(o, T.d, acc, asum, asum_t, touched != 0, rs);
  if (row_sum) row_sum[T.d] = rs;
  out[T.d] = r;
}

// :622-645: bounds of the 3x3 halo'd neighbourhood, ignoring missing values
__global__ __launch_bounds__(256) void k_mono_bounds(const FgTile *tiles, int ntiles, int nsrc, const int *src_idx_f, const double *f,
                                                      double missing, double *fbmax, double *fbmin, double *fmax, double *fmin)
{
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsrc) return;
  int t = 0;
  while (t + 1 < ntiles && s >= tiles[t + 1].cell_off) t++;
  const int ld = tiles[t].nx + 2, c = src_idx_f[s];
  double mx = -1.e20, mn = 1.e20;
  for (int jj = -1; jj <= 1; jj++)
    for (int ii = -1; ii <= 1; ii++) {
      double v = f[c + jj * ld + ii];
      if (v != missing) { if (v > mx) mx = v; if (v < mn) mn = v; }
    }
  fbmax[s] = mx; fbmin[s] = mn; fmax[s] = -1.e20; fmin[s] = 1.e20;
}

// :647-669: second-order value of every exchange cell (CSR order) and its extremes per source cell
__global__ __launch_bounds__(256) void k_mono_xdata(long nx, FgCsr csr, const double *f, const double *px, const double *py,
                                                     const int *gmask, double missing, double *xdata, double *fmax, double *fmin)
{
  long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nx) return;
  const FgCsrEntry2 E = csr.e2[q];
  double v = f[E.idx_f], x;
  if (v != missing) {
    if (gmask && gmask[E.idx_g]) x = v;
    else x = v + px[E.idx_g] * E.di + py[E.idx_g] * E.dj;
    // (the hardware's own FP64 max / min, no value returned: a compare-and-swap loop per value -- a read, then a CAS round, twice per
    // exchange cell -- made this kernel 0.415 of the 0.485 ms of a monotone sweep)
    (void)atomicMax(fmax + E.idx_g, x);
    (void)atomicMin(fmin + E.idx_g, x);
  } else
    x = missing;
  xdata[q] = x;
}

// :679-716
__global__ __launch_bounds__(256) void k_mono_limit(long nx, FgCsr csr, const double *f, double missing, const double *fbmax,
                                                     const double *fbmin, const double *fmax, const double *fmin, double *xdata, int *err)
{
  long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nx) return;
  double x = xdata[q];
  if (x == missing) return;
  const FgCsrEntry2 E = csr.e2[q];
  const int s = E.idx_g;
  const double f_bar = f[E.idx_f];
  if (fmax[s] > fbmax[s]) {
    x = f_bar + ((x - f_bar) / (fmax[s] - f_bar)) * (fbmax[s] - f_bar);
    if (x > fbmax[s]) {
      if (x - fbmax[s] < 1.e-10) x = fbmax[s];
      if (x > fbmax[s]) atomicOr(err, FG_XERR_ABOVE);
    }
  } else if (fmin[s] < fbmin[s]) {
    x = f_bar + ((x - f_bar) / (fmin[s] - f_bar)) * (fbmin[s] - f_bar);
    if (x < fbmin[s]) {
      if (fbmin[s] - x < 1.e-10) x = fbmin[s];
      if (x < fbmin[s]) atomicOr(err, FG_XERR_BELOW);
    }
  }
  xdata[q] = x;
}

template <int V> struct VecD;
template <> struct VecD<1> { double v[1]; };
template <> struct __attribute__((aligned(16))) VecD<2> { double v[2]; };
template <> struct __attribute__((aligned(16))) VecD<4> { double v[4]; };
template <> struct __attribute__((aligned(16))) VecD<8> { double v[8]; };


// MERGED (order 2): f points at records [source cell][3][NB] = {field, grad_x, grad_y} of the interior cell idx_g
// (k_merge3): one contiguous 3*NB*8-byte segment per entry instead of three NB*8-byte ones in three arrays -- 13 % (NB = 8)
// to 23 % (NB = 4) faster on MI355X; px, py unused.
template <int ORDER, int NB, int V, bool MERGED = false, int UNR = 1>
__global__ __launch_bounds__(256) void k_apply_il(int ndst, FgCsr csr, const double *f, const double *px, const double *py,
                                                   double missing, double *out, double *row_sum, long out_ld, int nb_valid, int xcd_band)
{
  constexpr int LPR = NB / V;                        // lanes per row
  constexpr int ROWS = 256 / LPR;                    // rows per block
  constexpr int APPLY_STAGE = ROWS * 6;              // CSR records staged in LDS (mean row has ~4)
  typedef typename std::conditional<ORDER == 2, FgCsrEntry2, FgCsrEntry1>::type Entry;
  __shared__ Entry sh_e[APPLY_STAGE];
  const int lev = (threadIdx.x % LPR) * V;
  const int d0 = d_xcd_block(blockIdx.x, gridDim.x, xcd_band) * ROWS;
  const int d = d0 + threadIdx.x / LPR;
  // the block's rows own one contiguous run of CSR records: stage it with coalesced 16-byte loads
  const int dl = min(d0 + ROWS, ndst);
  const int q0 = csr.row_ptr[d0], q1 = csr.row_ptr[dl];
  const int dc = min(d, ndst - 1);
  const int b = csr.row_ptr[dc], e = csr.row_ptr[dc + 1];   // (issued with q0, q1: one memory round trip less per wave)
  {
    const Entry *src = (ORDER == 2) ? (const Entry *)csr.e2 : (const Entry *)csr.e1;
    const int nstage = min(q1 - q0, APPLY_STAGE);
    constexpr int W = sizeof(Entry) / 16;            // 16-byte words per record
    const uint4 *g = reinterpret_cast<const uint4 *>(src + q0);
    uint4 *l = reinterpret_cast<uint4 *>(sh_e);
    // the CSR records are used once per launch: non-temporal loads keep them from evicting the gathered source records
    // (measured on MI355X, 8 levels: 0.1071 -> 0.0963 ms on records, 0.1162 -> 0.1049 ms on interleaved arrays)
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    for (int i = threadIdx.x; i < nstage * W; i += 256) ((u4v *)l)[i] = __builtin_nontemporal_load((const u4v *)g + i);
  }
  __syncthreads();
  if (d >= ndst) return;
  double acc[V], asum = 0.0;
#pragma unroll
  for (int k = 0; k < V; k++) acc[k] = 0.0;
  if (MERGED && UNR > 1) {
    // UNR entries of the row in flight per lane: all their gathers are issued before the first is consumed (a row has ~4
    // entries; the sums keep the CSR order).  Entries past the row's end repeat its last one (same lines, no new traffic).
    for (int q = b; q < e; q += UNR) {
      FgCsrEntry2 E[UNR];
      VecD<V> fv[UNR], gxv[UNR], gyv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; u++) {
        const int qq = min(q + u, e - 1), ql = qq - q0;
        E[u] = (ql < APPLY_STAGE) ? ((const FgCsrEntry2 *)sh_e)[ql] : csr.e2[qq];
      }
#pragma unroll
      for (int u = 0; u < UNR; u++) {
        const double *pf = f + (size_t)E[u].idx_g * (3 * NB) + lev;
        fv[u] = *reinterpret_cast<const VecD<V> *>(pf);
        gxv[u] = *reinterpret_cast<const VecD<V> *>(pf + NB);
        gyv[u] = *reinterpret_cast<const VecD<V> *>(pf + 2 * NB);
      }
#pragma unroll
      for (int u = 0; u < UNR; u++) {
        if (q + u < e) {
#pragma unroll
          for (int k = 0; k < V; k++) {
            double v = (fv[u].v[k] + gxv[u].v[k] * E[u].di + gyv[u].v[k] * E[u].dj);
            acc[k] += v * E[u].area;
          }
          asum += E[u].area;
        }
      }
    }
  } else
  for (int q = b; q < e; q++) {
    const int ql = q - q0;
    if (ORDER == 2) {
      const FgCsrEntry2 E = (ql < APPLY_STAGE) ? ((const FgCsrEntry2 *)sh_e)[ql] : csr.e2[q];
      const double *pf = MERGED ? f + (size_t)E.idx_g * (3 * NB) + lev : f + (size_t)E.idx_f * NB + lev;
      const double *pgx = MERGED ? pf + NB : px + (size_t)E.idx_g * NB + lev;
      const double *pgy = MERGED ? pf + 2 * NB : py + (size_t)E.idx_g * NB + lev;
      const VecD<V> fv = *reinterpret_cast<const VecD<V> *>(pf);
      const VecD<V> gxv = *reinterpret_cast<const VecD<V> *>(pgx);
      const VecD<V> gyv = *reinterpret_cast<const VecD<V> *>(pgy);
#pragma unroll
      for (int k = 0; k < V; k++) {
        double v = (fv.v[k] + gxv.v[k] * E.di + gyv.v[k] * E.dj);
        acc[k] += v * E.area;
      }
      asum += E.area;
    } else {
      const FgCsrEntry1 E = (ql < APPLY_STAGE) ? ((const FgCsrEntry1 *)sh_e)[ql] : csr.e1[q];
      const VecD<V> fv = *reinterpret_cast<const VecD<V> *>(f + (size_t)E.idx_f * NB + lev);
#pragma unroll
      for (int k = 0; k < V; k++) acc[k] += fv.v[k] * E.area;
      asum += E.area;
    }
  }
  VecD<V> r, rs;
#pragma unroll
  for (int k = 0; k < V; k++) {
    rs.v[k] = (asum > 0) ? acc[k] : 0.0;
    if (asum > 0) r.v[k] = acc[k] / asum;
    else if (e > b) r.v[k] = 0.0;
    else r.v[k] = missing;
  }
  if (row_sum) *reinterpret_cast<VecD<V> *>(row_sum + (size_t)d * NB + lev) = rs;
  if (out_ld > 0) {
    // level-major output out[level][d] (fg_plan_apply): lanes of one level group hold consecutive rows, so each store
    // instruction writes 16 consecutive doubles per level -- the separate de-interleave pass is not needed
#pragma unroll
    for (int k = 0; k < V; k++) if (lev + k < nb_valid) out[(size_t)(lev + k) * out_ld + d] = r.v[k];
  } else
    *reinterpret_cast<VecD<V> *>(out + (size_t)d * NB + lev) = r;
}

// Entry-parallel order-2 sweep on merged records, 8 levels: the gathers of ALL of a tile's exchange cells are issued in one go
// (a lane pair per exchange cell, up to three per lane pair), the products area * (f + gx di + gy dj) go to LDS, and a lane group
// per destination row adds them in CSR order -- the same operations in the same order as k_apply_il, so the same bits, but a
// wave's dependent chain is row pointers -> CSR staging -> ONE round of gathers -> LDS sums instead of ~7 gather rounds.
// A tile whose rows hold more than EP_CAP exchange cells (fine -> coarse remaps) takes the row-serial loop.
// (A persistent version -- blocks walking over tiles, the next tile's row pointers and records prefetched into registers while
//  the current tile's gathers fly, no LDS staging -- was measured: 0.119 ms against 0.0833.  Its 108 VGPRs halve the occupancy
//  (4 waves per SIMD against 7), and the occupancy is what hides the gather latency.)
#ifndef EP_ROWS
#define EP_ROWS 32
#endif
template <int TPB, int CAP>
__global__ __launch_bounds__(TPB) void k_apply_ep8(int ndst, FgCsr csr, const double *rec, double missing, double *out, double *row_sum,
                                                    long out_ld, int nb_valid, int xcd_band)
{
  constexpr int NB = 8;                                    // sum phase: a lane per (row, level); EP_ROWS * NB <= TPB lanes take part
  static_assert(EP_ROWS * NB <= TPB, "rows per tile");
  constexpr int EPP = TPB / 2, PASS = CAP / EPP;          // gather phase: a lane pair per exchange cell, EPP cells per pass
  // one buffer: the staged CSR records first, then (once every lane holds its records in registers) the products and areas
  __shared__ __attribute__((aligned(16))) double sh_raw[CAP * (NB + 1)];
  FgCsrEntry2 *sh_e = reinterpret_cast<FgCsrEntry2 *>(sh_raw);
  double *sh_p = sh_raw, *sh_a = sh_raw + CAP * NB;
  const int t = threadIdx.x;
  const EpTile T = ep_tile<EP_ROWS, NB>(csr, ndst, d_xcd_block(blockIdx.x, gridDim.x, xcd_band));
  const int q0 = T.q0, n = T.q1 - T.q0, lev = T.lev;
  ep_stage_loop<TPB>(sh_e, csr.e2 + q0, min(n, CAP));
  __syncthreads();
  double acc = 0.0, asum = 0.0;
  if (n <= CAP) {
    const int h = (t & 1) * 4;                             // four levels per lane of the pair
    VecD<4> fv[PASS], gxv[PASS], gyv[PASS];
    FgCsrEntry2 E[PASS];
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      if (EPP * j < n) {                                   // (block-uniform)
        const int i = min(t / 2 + EPP * j, n - 1);
        E[j] = sh_e[i];
        const double *pf = rec + (size_t)E[j].idx_g * (3 * NB) + h;
        fv[j] = *reinterpret_cast<const VecD<4> *>(pf);
        gxv[j] = *reinterpret_cast<const VecD<4> *>(pf + NB);
        gyv[j] = *reinterpret_cast<const VecD<4> *>(pf + 2 * NB);
      }
    }
    __syncthreads();                                       // the records are in registers: the buffer becomes the product table
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      const int i = t / 2 + EPP * j;
      if (EPP * j < n && i < n) {
        VecD<4> pv;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          double v = (fv[j].v[k] + gxv[j].v[k] * E[j].di + gyv[j].v[k] * E[j].dj);
          pv.v[k] = v * E[j].area;
        }
        *reinterpret_cast<VecD<4> *>(sh_p + i * NB + h) = pv;
        if (h == 0) sh_a[i] = E[j].area;
      }
    }
    __syncthreads();
    if (T.d >= ndst || !T.lane) return;
    for (int q = T.b - q0; q < T.e - q0; q++) { acc += sh_p[q * NB + lev]; asum += sh_a[q]; }
  } else {
    if (T.d >= ndst || !T.lane) return;
    for (int q = T.b; q < T.e; q++) {
      const int ql = q - q0;
      const FgCsrEntry2 E = (ql < CAP) ? sh_e[ql] : csr.e2[q];
      const double *pf = rec + (size_t)E.idx_g * (3 * NB) + lev;
      double v = (pf[0] + pf[NB] * E.di + pf[2 * NB] * E.dj);
      acc += v * E.area;
      asum += E.area;
    }
  }
  double rs;
  const double r = apply_finish(acc, asum, T.e > T.b, missing, rs);
  if (row_sum) row_sum[(size_t)T.d * NB + lev] = rs;
  if (out_ld > 0) { if (lev < nb_valid) out[(size_t)lev * out_ld + T.d] = r; }
  else out[(size_t)T.d * NB + lev] = r;
}

// The same for plans with longer rows (fine -> coarse remaps; k_apply_ep8 above is for rows of a few exchange cells): ROWS rows per
// tile, fewer the longer the mean row, and the tile's run of CSR records walked in chunks of CAP, the (row, level) lanes carrying
// their sums from chunk to chunk: any row length, every gather of a chunk in one round.  (Such plans took the row-serial
// k_apply_il before: C384 -> 2 deg 0.117 ms per 8 levels on records, now 0.037.)  As a loop the kernel needs more registers than
// k_apply_ep8 -- with 32 rows per tile on C384 -> 0.25 deg it runs in 0.117 ms against 0.083 -- so short rows keep the kernel above.
// (ORDER 1: `rec` is the interleaved field [cell][8], a 16-byte CSR record and one 64-byte gather per exchange cell.)
//
// MASKED: eight levels that each carry their own missing values (fg_plan_apply_levels, fg_plan_apply_records_levels,
// fg_sweep_run_levels).  The reference takes such a field one level per call (fregrid.c:1045-1083; conserve_interp.c:544 forbids
// has_missing with nz > 1): level k of the output is do_scalar_conserve_interp(nz = 1, has_missing = 1) on level k alone -- per
// destination cell the exchange cells whose source value differs from `missing` IN THAT LEVEL are summed in CSR order, the result is
// acc / asum where asum > 0, 0.0 where an exchange cell counted but asum == 0, else `missing` (:562-591, :744-783, :815-839).
// Here every CSR record is still read once and every gather is a full 64-byte sector; only the validity differs from level to
// level: the product table keeps ONE area and an 8-bit validity mask per exchange cell, an invalid (exchange cell, level) holds the
// product +0.0, and the (row, level) lane carries a touched flag beside its two sums.
//   gbits (ORDER 2): per source cell, bit k set = level k takes the flat value (fregrid_util.c:2203-2215); k_gmask_bits makes them.
//   out, row_sum: level-major [level][out_ld], levels < nb_valid only.  The tile mapping is the identity (xcd_band is not read).
// (Weight field, cell_measures, cell_methods = sum and --target_grid on eight levels: k_apply_ep8x below.  This kernel is the
// bandwidth path and carries none of their gathers.)
template <int ORDER, bool MASKED, int TPB, int CAP, int ROWS>
__global__ __launch_bounds__(TPB) void k_apply_ep8g(int ndst, FgCsr csr, const double *rec, const unsigned char *gbits, double missing,
                                                    double *out, double *row_sum, long out_ld, int nb_valid, int xcd_band)
{
  constexpr int NB = 8;
  constexpr int EPP = TPB / 2, PASS = CAP / EPP;          // gather phase: a lane pair per exchange cell, EPP cells per pass
  static_assert(ROWS * NB <= TPB && (!MASKED || CAP % EPP == 0), "a lane per (row, level)");
  // one buffer: the staged CSR records first, then (once every lane holds its records in registers) the products and areas
  __shared__ __attribute__((aligned(16))) double sh_raw[CAP * (NB + 1)];
  __shared__ unsigned char sh_vm[MASKED ? CAP * 2 : 1];    // MASKED: validity of levels 0-3 and 4-7 of every staged exchange cell
  typedef CsrEntry<ORDER> Entry;
  Entry *sh_e = reinterpret_cast<Entry *>(sh_raw);
  double *sh_p = sh_raw, *sh_a = sh_raw + CAP * NB;
  const int t = threadIdx.x;
  const EpTile T = ep_tile<ROWS, NB>(csr, ndst, MASKED ? (int)blockIdx.x : d_xcd_block(blockIdx.x, gridDim.x, xcd_band));
  const int lev = T.lev, vsel = lev >> 2, vbit = lev & 3;
  double acc = 0.0, asum = 0.0;
  unsigned touched = 0;
  for (int c0 = T.q0; c0 < T.q1; c0 += CAP) {              // (block-uniform)
    const int n = min(CAP, T.q1 - c0);
    if (c0 > T.q0) __syncthreads();                        // the previous chunk's products have been added
    ep_stage_loop<TPB>(sh_e, csr_entries<ORDER>(csr) + c0, n);
    __syncthreads();
    const int h = (t & 1) * 4;                             // four levels per lane of the pair
    VecD<4> fv[PASS], gxv[PASS], gyv[PASS];
    Entry E[PASS];
    unsigned gb[PASS];
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      gb[j] = 0;
      if (EPP * j < n) {                                   // (block-uniform)
        const int i = min(t / 2 + EPP * j, n - 1);
        E[j] = sh_e[i];
        if constexpr (ORDER == 2) {
          const double *pf = rec + (size_t)E[j].idx_g * (3 * NB) + h;
          fv[j] = *reinterpret_cast<const VecD<4> *>(pf);
          gxv[j] = *reinterpret_cast<const VecD<4> *>(pf + NB);
          gyv[j] = *reinterpret_cast<const VecD<4> *>(pf + 2 * NB);
          if constexpr (MASKED) gb[j] = gbits[E[j].idx_g];
        } else
          fv[j] = *reinterpret_cast<const VecD<4> *>(rec + (size_t)E[j].idx_f * NB + h);
      }
    }
    __syncthreads();                                       // the records are in registers: the buffer becomes the product table
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      const int i = t / 2 + EPP * j;
      if (EPP * j < n && i < n) {
        VecD<4> pv;
        unsigned vm = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          double v = fv[j].v[k];
          bool ok = true;
          if constexpr (MASKED) ok = !(v == missing);      // `if (data == missing) continue`
          if constexpr (ORDER == 2) { if (!((gb[j] >> (h + k)) & 1u)) v = (v + gxv[j].v[k] * E[j].di + gyv[j].v[k] * E[j].dj); }
          pv.v[k] = ok ? v * E[j].area : 0.0;
          vm |= (ok ? 1u : 0u) << k;
        }
        *reinterpret_cast<VecD<4> *>(sh_p + i * NB + h) = pv;
        if constexpr (MASKED) sh_vm[i * 2 + (t & 1)] = (unsigned char)vm;
        if (h == 0) sh_a[i] = E[j].area;
      }
    }
    __syncthreads();
    if (T.lane)
      ep_row_add(T.b, T.e, c0, n, acc, asum, touched, [&](int q) {
        if constexpr (MASKED) {
          const unsigned ok = (sh_vm[q * 2 + vsel] >> vbit) & 1u;
          return EpTerm{sh_p[q * NB + lev], ok ? sh_a[q] : 0.0, ok};
        } else
          return EpTerm{sh_p[q * NB + lev], sh_a[q], 0u};
      });
  }
  if (!T.lane || T.d >= ndst || (MASKED && lev >= nb_valid)) return;
  double rs;
  const double r = apply_finish(acc, asum, MASKED ? touched != 0 : T.e > T.b, missing, rs);
  if (row_sum) row_sum[MASKED ? (size_t)lev * out_ld + T.d : (size_t)T.d * NB + lev] = rs;
  if (MASKED || out_ld > 0) { if (lev < nb_valid) out[(size_t)lev * out_ld + T.d] = r; }
  else out[(size_t)T.d * NB + lev] = r;
}

// The sum phase of k_apply_ep8x and k_apply_ep8m below: the (row, level) lane's part of the chunk [c0, c0 + n) from the product table
// (APL: scaled area and target term per level) -- three sums and the flag, four LDS reads of each in flight, adds in CSR order.
template <bool APL>
__device__ __forceinline__ void ep8x_row_add(const EpTile &T, int c0, int n, const double *sh_p, const double *sh_a, const double *sh_t,
                                             const unsigned char *sh_vm, double &acc, double &asum, double &asum_t, unsigned &touched)
{
  constexpr int NB = 8;
  const int lev = T.lev, vsel = lev >> 2, vbit = lev & 3;
  const int qa = max(T.b, c0) - c0, qb = min(T.e, c0 + n) - c0;
  auto term = [&](int q, double &p, double &a, double &tt, unsigned &ok) {
    ok = (sh_vm[q * 2 + vsel] >> vbit) & 1u;
    p = sh_p[q * NB + lev];
    if constexpr (APL) { a = sh_a[q * NB + lev]; tt = sh_t[q * NB + lev]; }
    else { a = ok ? sh_a[q] : 0.0; tt = sh_t[q]; }
  };
  int q = qa;
  for (; q + 4 <= qb; q += 4) {
    double p[4], a[4], tt[4];
    unsigned ok[4];
#pragma unroll
    for (int k = 0; k < 4; k++) term(q + k, p[k], a[k], tt[k], ok[k]);
#pragma unroll
    for (int k = 0; k < 4; k++) { asum_t += tt[k]; acc += p[k]; asum += a[k]; touched |= ok[k]; }
  }
  for (; q < qb; q++) {
    double p, a, tt;
    unsigned ok;
    term(q, p, a, tt, ok);
    asum_t += tt; acc += p; asum += a; touched |= ok;
  }
}

// Eight levels with every option of do_scalar_conserve_interp but the monotone limiter (fg_plan_apply_levels_ex,
// fg_plan_apply_records_levels_ex, fg_sweep_run_levels_ex): the sibling of k_apply_ep8g<MASKED> with k_apply_epx's per-cell
// arithmetic.  Level k of the output is do_scalar_conserve_interp(nz = 1) on level k alone with the same options (the reference
// refuses nz > 1 for them, conserve_interp.c:544-546, so fregrid.c:1045-1083 loops over the levels); per (exchange cell, level) the
// operations come in the reference's order -- area *= weight, the missing test, area /= cell_area (sum) or the area_missing check
// and area *= (field_area / cell_area) (cell_measures), value * area -- and a cell left by `continue` adds +0.0 and is not counted.
// The --target_grid term (:842-858) is taken from every exchange cell, missing or not: area * field_area / cell_area, left to
// right, or the plain area without cell_measures.
//   APL false: weight, cell_area and field_area are per source cell and the same for the eight levels: the product table keeps ONE
//     scaled area and ONE target term per exchange cell beside the 8-bit validity mask, as k_apply_ep8g keeps one area.
//   APL true:  field_area has a level axis (area_has_zaxis, fregrid_util.c:2156-2162; e.g. volcello); fa8 holds it interleaved
//     [source cell][8] (zero beyond nb_valid), one 64-byte gather like the field's.  Scaled area and target term are per (exchange
//     cell, level): the table is 24 doubles per cell, so CAP is half the other form's.
// The (row, level) lane adds three sums in CSR order and carries them from chunk to chunk.  Tile mapping: the identity.
template <int ORDER, bool APL, int TPB, int CAP, int ROWS>
__global__ __launch_bounds__(TPB) void k_apply_ep8x(int ndst, FgCsr csr, const double *rec, const unsigned char *gbits, FgApplyEx o,
                                                    const double *fa8, double *out, double *row_sum, long out_ld, int nb_valid, int *err)
{
  constexpr int NB = 8;
  constexpr int EPP = TPB / 2, PASS = CAP / EPP;          // gather phase: a lane pair per exchange cell, EPP cells per pass
  constexpr int AW = APL ? NB : 1;                        // scaled areas / target terms per exchange cell
  static_assert(ROWS * NB <= TPB && CAP % EPP == 0, "a lane per (row, level)");
  // one buffer: the staged CSR records first (<= 32 B each), then the products, the scaled areas and the target terms
  __shared__ __attribute__((aligned(16))) double sh_raw[CAP * (NB + 2 * AW)];
  __shared__ unsigned char sh_vm[CAP * 2];                 // validity of levels 0-3 and 4-7 of every staged exchange cell
  typedef CsrEntry<ORDER> Entry;
  Entry *sh_e = reinterpret_cast<Entry *>(sh_raw);
  double *sh_p = sh_raw, *sh_a = sh_raw + CAP * NB, *sh_t = sh_a + CAP * AW;
  const int t = threadIdx.x;
  const EpTile T = ep_tile<ROWS, NB>(csr, ndst, (int)blockIdx.x);
  const int lev = T.lev;
  const bool scaled = o.sum || o.field_area;              // (block-uniform, as every test of `o` below)
  double acc = 0.0, asum = 0.0, asum_t = 0.0;
  unsigned touched = 0;
  for (int c0 = T.q0; c0 < T.q1; c0 += CAP) {              // (block-uniform)
    const int n = min(CAP, T.q1 - c0);
    if (c0 > T.q0) __syncthreads();                        // the previous chunk's products have been added
    ep_stage_loop<TPB>(sh_e, csr_entries<ORDER>(csr) + c0, n);
    __syncthreads();
    const int h = (t & 1) * 4;                             // four levels per lane of the pair
    VecD<4> fv[PASS], gxv[PASS], gyv[PASS], fav[PASS];
    Entry E[PASS];
    double wgt[PASS], ca[PASS], fa[PASS];
    unsigned gb[PASS];
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      gb[j] = 0; wgt[j] = 1.0; ca[j] = 1.0; fa[j] = 0.0;
      if (EPP * j < n) {                                   // (block-uniform)
        const int i = min(t / 2 + EPP * j, n - 1);
        E[j] = sh_e[i];
        int s;
        if constexpr (ORDER == 2) {
          s = E[j].idx_g;
          const double *pf = rec + (size_t)s * (3 * NB) + h;
          fv[j] = *reinterpret_cast<const VecD<4> *>(pf);
          gxv[j] = *reinterpret_cast<const VecD<4> *>(pf + NB);
          gyv[j] = *reinterpret_cast<const VecD<4> *>(pf + 2 * NB);
          if (gbits) gb[j] = gbits[s];
        } else {
          s = E[j].idx_f;
          fv[j] = *reinterpret_cast<const VecD<4> *>(rec + (size_t)s * NB + h);
        }
        // every value the cell may need, in the same round
        if (o.weight) wgt[j] = o.weight[s];
        if (scaled) ca[j] = o.cell_area[s];
        if constexpr (APL) fav[j] = *reinterpret_cast<const VecD<4> *>(fa8 + (size_t)s * NB + h);
        else if (o.field_area) fa[j] = o.field_area[s];
      }
    }
    __syncthreads();                                       // the records are in registers: the buffer becomes the product table
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      const int i = t / 2 + EPP * j;
      if (EPP * j < n && i < n) {
        const double a0 = E[j].area;
        double aw = a0;
        if (o.weight) aw *= wgt[j];                        // :574 ...: the weight comes before the missing test
        VecD<4> pv;
        unsigned vm = 0;
        if constexpr (!APL) {
          double tt = 0.0, as = aw;
          bool bad = false;
          if (o.cell_area_out) tt = o.field_area ? (a0 * fa[j] / ca[j]) : a0;    // :845-860 (plain exchange-cell area, no weight)
          if (o.sum) as = aw / ca[j];
          else if (o.field_area) { bad = o.has_missing && fa[j] == o.area_missing; as = aw * (fa[j] / ca[j]); }
#pragma unroll
          for (int k = 0; k < 4; k++) {
            double v = fv[j].v[k];
            bool ok = !(o.has_missing && v == o.missing);  // `if (data == missing) continue`
            if (ok && bad) { if (h + k < nb_valid) atomicOr(err, FG_XERR_AREA_MISSING); ok = false; }
            if constexpr (ORDER == 2) { if (!((gb[j] >> (h + k)) & 1u)) v = (v + gxv[j].v[k] * E[j].di + gyv[j].v[k] * E[j].dj); }
            pv.v[k] = ok ? v * as : 0.0;
            vm |= (ok ? 1u : 0u) << k;
          }
          if (h == 0) { sh_a[i] = as; sh_t[i] = tt; }
        } else {
          VecD<4> av, tv;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            double v = fv[j].v[k];
            const double f = fav[j].v[k];
            bool ok = !(o.has_missing && v == o.missing);
            if (ok && o.has_missing && f == o.area_missing) { if (h + k < nb_valid) atomicOr(err, FG_XERR_AREA_MISSING); ok = false; }
            const double as = aw * (f / ca[j]);
            if constexpr (ORDER == 2) { if (!((gb[j] >> (h + k)) & 1u)) v = (v + gxv[j].v[k] * E[j].di + gyv[j].v[k] * E[j].dj); }
            pv.v[k] = ok ? v * as : 0.0;
            av.v[k] = ok ? as : 0.0;
            tv.v[k] = o.cell_area_out ? (a0 * f / ca[j]) : 0.0;
            vm |= (ok ? 1u : 0u) << k;
          }
          *reinterpret_cast<VecD<4> *>(sh_a + i * NB + h) = av;
          *reinterpret_cast<VecD<4> *>(sh_t + i * NB + h) = tv;
        }
        *reinterpret_cast<VecD<4> *>(sh_p + i * NB + h) = pv;
        sh_vm[i * 2 + (t & 1)] = (unsigned char)vm;
      }
    }
    __syncthreads();
    if (T.lane) ep8x_row_add<APL>(T, c0, n, sh_p, sh_a, sh_t, sh_vm, acc, asum, asum_t, touched);
  }
  if (!T.lane || T.d >= ndst || lev >= nb_valid) return;
  double rs;
  const double r = apply_finish_ex(o, T.d, acc, asum, asum_t, touched != 0, rs);
  if (row_sum) row_sum[(size_t)lev * out_ld + T.d] = rs;
  out[(size_t)lev * out_ld + T.d] = r;
}

// ------------------------------------------------------------------- the monotone limiter, eight levels per launch
// conserve_order2_monotonic (conserve_interp.c:617-742) on the chunks of fg_plan_apply_levels_mono / fg_plan_mono_levels_*: level k
// is the one-level chain k_mono_bounds, k_mono_xdata, k_mono_limit, k_apply_epx<2, MONO> on level k alone, bit for bit.  The
// per-source-cell numbers of a chunk live in b8 [source cell][4][8] = f_bar_max | f_bar_min | f_max | f_min, one 256-byte gather
// per exchange cell for the eight levels; no per-exchange-cell value is stored: the sweep recomputes f + gx di + gy dj from the
// operands the extremes kernel used.
#define MB8 32                                             // doubles per source cell in b8
// :622-645 per (source cell, level): CB cells per block, a wave reads consecutive cells of ONE level (the nine loads of a
// neighbourhood are contiguous along i), the records leave through LDS in one coalesced sweep.  Levels >= nb get the initial
// values in all four rows, so no branch of the limiter is taken for them.
template <int CB>
__global__ __launch_bounds__(256) void k_mono_bounds8(const FgTile *tiles, int ntiles, int nsrc, const int *src_idx_f, const double *f,
                                                       long ld_f, int nb, double missing, double *b8)
{
  constexpr int NB = 8;
  static_assert(256 % CB == 0 && NB % (256 / CB) == 0, "a thread keeps its cell");
  __shared__ double tile[CB * (MB8 + 1)];
  const int t = threadIdx.x % CB;
  const long s0 = (long)blockIdx.x * CB, s = s0 + t;
  int c = 0, ld = 0;
  if (s < nsrc) {
    int m = 0;
    while (m + 1 < ntiles && s >= tiles[m + 1].cell_off) m++;
    ld = tiles[m].nx + 2; c = src_idx_f[s];
  }
  for (int k = threadIdx.x / CB; k < NB; k += 256 / CB) {
    double mx = -1.e20, mn = 1.e20;
    if (k < nb && s < nsrc) {
      const double *fk = f + (size_t)k * ld_f + c;
      for (int jj = -1; jj <= 1; jj++)
        for (int ii = -1; ii <= 1; ii++) {
          const double v = fk[jj * ld + ii];
          if (v != missing) { if (v > mx) mx = v; if (v < mn) mn = v; }
        }
    }
    double *r = tile + t * (MB8 + 1) + k;
    r[0] = mx; r[NB] = mn; r[2 * NB] = -1.e20; r[3 * NB] = 1.e20;
  }
  __syncthreads();
  const long cnt = ((nsrc - s0) < CB ? (nsrc - s0) : CB) * MB8;  // doubles this block writes
  for (long e = threadIdx.x; e < cnt; e += 256) b8[(size_t)s0 * MB8 + e] = tile[(e / MB8) * (MB8 + 1) + (e % MB8)];
}

// :647-669: a lane per (exchange cell, level).  The eight lanes of a cell read one CSR record (one request) and one 64-byte
// segment of each of f, gx, gy; the value is k_mono_xdata's expression on the same operands.  The hardware's FP64 max / min, no
// value returned.  Missing values and the levels >= nb of a partial chunk issue no atomic.
__global__ __launch_bounds__(256) void k_mono_extremes8(long nx, FgCsr csr, const double *rec, const unsigned char *gbits, double missing,
                                                         int nb, double *b8)
{
  constexpr int NB = 8;
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x, q = g / NB;
  const int k = (int)(g % NB);
  if (q >= nx || k >= nb) return;
  const FgCsrEntry2 E = csr.e2[q];
  const double *pf = rec + (size_t)E.idx_g * (3 * NB) + k;
  const double v = pf[0];
  if (v == missing) return;
  double x = v;
  if (!(gbits && ((gbits[E.idx_g] >> k) & 1u))) x = v + pf[NB] * E.di + pf[2 * NB] * E.dj;
  double *b = b8 + (size_t)E.idx_g * MB8 + k;
  (void)atomicMax(b + 2 * NB, x);
  (void)atomicMin(b + 3 * NB, x);
}

// f_max / f_min of nz levels between b8 and the caller's level-major buffers [nz][nsrc] (fg_plan_mono_levels_copy_minmax)
__global__ __launch_bounds__(256) void k_mono_minmax8(int nsrc, int nz, int to_b8, double *b8, double *f_min, double *f_max)
{
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long)nsrc * nz) return;
  const long s = g % nsrc;
  const int k = (int)(g / nsrc);
  constexpr int NB = 8;
  double *b = b8 + (size_t)s * MB8 + k;
  if (to_b8) { b[2 * NB] = f_max[g]; b[3 * NB] = f_min[g]; }
  else { f_max[g] = b[2 * NB]; f_min[g] = b[3 * NB]; }
}

// rows 2 and 3 of every b8 record back to the start values k_mono_bounds8 gives them: a lane per double, 16 consecutive doubles
// (128 B) per source cell.  Between two plans over one source grid, instead of a second bounds pass (fg_plan_mono_records_reset).
__global__ __launch_bounds__(256) void k_mono_reset8(int nsrc, double *b8)
{
  constexpr int NB = 8;
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long)nsrc * (2 * NB)) return;
  const int q = (int)(g % (2 * NB));
  b8[(size_t)(g / (2 * NB)) * MB8 + 2 * NB + q] = q < NB ? -1.e20 : 1.e20;
}

// The limited sweep: k_apply_ep8x<2, false> whose gather round also takes the source cell's bounds record.  Per (exchange cell,
// level): the second-order value as in k_mono_extremes8 (same operations on the same operands: same bits), :689-713 with the
// 1e-10 snap and the fatal checks (an error bit only for a level < nb_valid), then area *= weight, the sum / cell_measures scaling
// and the product, in k_apply_epx<2, MONO>'s order.  A value equal to `missing` -- the field's, the second-order value's or the
// limited one's, as the one-level chain tests its stored xdata -- adds +0.0; the branch never counts a cell as touched (:720-739),
// so a row without area becomes `missing`.  No area_missing check.  The --target_grid term is taken from every exchange cell.
template <int TPB, int CAP, int ROWS>
__global__ __launch_bounds__(TPB) void k_apply_ep8m(int ndst, FgCsr csr, const double *rec, const unsigned char *gbits, const double *b8,
                                                    FgApplyEx o, double *out, double *row_sum, long out_ld, int nb_valid, int *err)
{
  constexpr int NB = 8;
  constexpr int EPP = TPB / 2, PASS = CAP / EPP;          // gather phase: a lane pair per exchange cell, EPP cells per pass
  static_assert(ROWS * NB <= TPB && CAP % EPP == 0, "a lane per (row, level)");
  __shared__ __attribute__((aligned(16))) double sh_raw[CAP * (NB + 2)];   // the staged CSR records, then products, areas, target terms
  __shared__ unsigned char sh_vm[CAP * 2];
  FgCsrEntry2 *sh_e = reinterpret_cast<FgCsrEntry2 *>(sh_raw);
  double *sh_p = sh_raw, *sh_a = sh_raw + CAP * NB, *sh_t = sh_a + CAP;
  const int t = threadIdx.x;
  const EpTile T = ep_tile<ROWS, NB>(csr, ndst, (int)blockIdx.x);
  const int lev = T.lev;
  const bool scaled = o.sum || o.field_area;              // (block-uniform, as every test of `o` below)
  double acc = 0.0, asum = 0.0, asum_t = 0.0;
  unsigned touched = 0;
  for (int c0 = T.q0; c0 < T.q1; c0 += CAP) {              // (block-uniform)
    const int n = min(CAP, T.q1 - c0);
    if (c0 > T.q0) __syncthreads();                        // the previous chunk's products have been added
    ep_stage_loop<TPB>(sh_e, csr.e2 + c0, n);
    __syncthreads();
    const int h = (t & 1) * 4;                             // four levels per lane of the pair
    VecD<4> fv[PASS], gxv[PASS], gyv[PASS], bmx[PASS], bmn[PASS], xmx[PASS], xmn[PASS];
    FgCsrEntry2 E[PASS];
    double wgt[PASS], ca[PASS], fa[PASS];
    unsigned gb[PASS];
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      gb[j] = 0; wgt[j] = 1.0; ca[j] = 1.0; fa[j] = 0.0;
      if (EPP * j < n) {                                   // (block-uniform)
        const int i = min(t / 2 + EPP * j, n - 1);
        E[j] = sh_e[i];
        const int s = E[j].idx_g;
        const double *pf = rec + (size_t)s * (3 * NB) + h, *pb = b8 + (size_t)s * MB8 + h;
        fv[j] = *reinterpret_cast<const VecD<4> *>(pf);
        gxv[j] = *reinterpret_cast<const VecD<4> *>(pf + NB);
        gyv[j] = *reinterpret_cast<const VecD<4> *>(pf + 2 * NB);
        bmx[j] = *reinterpret_cast<const VecD<4> *>(pb);
        bmn[j] = *reinterpret_cast<const VecD<4> *>(pb + NB);
        xmx[j] = *reinterpret_cast<const VecD<4> *>(pb + 2 * NB);
        xmn[j] = *reinterpret_cast<const VecD<4> *>(pb + 3 * NB);
        if (gbits) gb[j] = gbits[s];
        if (o.weight) wgt[j] = o.weight[s];
        if (scaled) ca[j] = o.cell_area[s];
        if (o.field_area) fa[j] = o.field_area[s];
      }
    }
    __syncthreads();                                       // the records are in registers: the buffer becomes the product table
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      const int i = t / 2 + EPP * j;
      if (EPP * j < n && i < n) {
        const double a0 = E[j].area;
        double as = a0, tt = 0.0;
        if (o.weight) as *= wgt[j];
        if (o.cell_area_out) tt = o.field_area ? (a0 * fa[j] / ca[j]) : a0;      // :845-860 (plain exchange-cell area, no weight)
        if (o.sum) as /= ca[j];
        else if (o.field_area) as *= (fa[j] / ca[j]);
        VecD<4> pv;
        unsigned vm = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const double f_bar = fv[j].v[k];
          double x = f_bar;
          bool ok = !(f_bar == o.missing);
          if (!((gb[j] >> (h + k)) & 1u)) x = f_bar + gxv[j].v[k] * E[j].di + gyv[j].v[k] * E[j].dj;
          if (ok && !(x == o.missing)) {                   // k_mono_limit passes over a stored value equal to `missing`
            const double fbmax = bmx[j].v[k], fbmin = bmn[j].v[k], fmax = xmx[j].v[k], fmin = xmn[j].v[k];
            if (fmax > fbmax) {
              x = f_bar + ((x - f_bar) / (fmax - f_bar)) * (fbmax - f_bar);
              if (x > fbmax) {
                if (x - fbmax < 1.e-10) x = fbmax;
                if (x > fbmax && h + k < nb_valid) atomicOr(err, FG_XERR_ABOVE);
              }
            } else if (fmin < fbmin) {
              x = f_bar + ((x - f_bar) / (fmin - f_bar)) * (fbmin - f_bar);
              if (x < fbmin) {
                if (fbmin - x < 1.e-10) x = fbmin;
                if (x < fbmin && h + k < nb_valid) atomicOr(err, FG_XERR_BELOW);
              }
            }
          }
          ok = ok && !(x == o.missing);                    // `if (xdata == missing) continue` of the sweep
          pv.v[k] = ok ? x * as : 0.0;
          vm |= (ok ? 1u : 0u) << k;
        }
        if (h == 0) { sh_a[i] = as; sh_t[i] = tt; }
        *reinterpret_cast<VecD<4> *>(sh_p + i * NB + h) = pv;
        sh_vm[i * 2 + (t & 1)] = (unsigned char)vm;
      }
    }
    __syncthreads();
    if (T.lane) ep8x_row_add<false>(T, c0, n, sh_p, sh_a, sh_t, sh_vm, acc, asum, asum_t, touched);
  }
  if (!T.lane || T.d >= ndst || lev >= nb_valid) return;
  double rs;
  const double r = apply_finish_ex(o, T.d, acc, asum, asum_t, false, rs);
  if (row_sum) row_sum[(size_t)lev * out_ld + T.d] = rs;
  out[(size_t)lev * out_ld + T.d] = r;
}

// grad_mask int [nb][ncells] (fg_c2l_gradient) -> one byte per source cell, bit k = level k
__global__ __launch_bounds__(256) void k_gmask_bits(long n, const int *gmask, long ld, int nb, unsigned char *bits)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  unsigned m = 0;
  for (int k = 0; k < nb; k++) m |= (gmask[(size_t)k * ld + c] != 0 ? 1u : 0u) << k;
  bits[c] = (unsigned char)m;
}

// [nb][n] (level-major, row stride ld) <-> [n][NB] interleaved
template <int NB>
__global__ __launch_bounds__(256) void k_interleave(long n, const double *in, long ld, int nb, double *out)
{
  long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double v[NB];
#pragma unroll
  for (int k = 0; k < NB; k++) v[k] = (k < nb) ? in[(size_t)k * ld + c] : 0.0;
#pragma unroll
  for (int k = 0; k < NB; k++) out[(size_t)c * NB + k] = v[k];
}
template <int NB>
__global__ __launch_bounds__(256) void k_deinterleave(long n, const double *in, long ld, int nb, double *out)
{
  long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double v[NB];
#pragma unroll
  for (int k = 0; k < NB; k++) v[k] = in[(size_t)c * NB + k];
#pragma unroll
  for (int k = 0; k < NB; k++) if (k < nb) out[(size_t)k * ld + c] = v[k];
}

// Up to three level-major arrays -> interleaved in one launch (blockIdx.y picks the array), transposed through LDS so
// both the global reads ([level][cell], consecutive cells per level) and the global writes ([cell][NB], consecutive
// addresses across the block) are fully coalesced.  The per-thread version above wrote 64-byte strided chunks and reached
// only ~0.5 TB/s.
struct FgIl3 { const double *in[3]; double *out[3]; long n[3]; long ld[3]; };
template <int NB>
__global__ __launch_bounds__(256) void k_interleave3(FgIl3 a, int nb)
{
  __shared__ double tile[256 * (NB + 1)];
  const int w = blockIdx.y;
  const long n = a.n[w];
  const long c0 = (long)blockIdx.x * 256;
  if (c0 >= n) return;
  const double *in = a.in[w];
  double *out = a.out[w];
  const long ld = a.ld[w];
  const long c = c0 + threadIdx.x;
#pragma unroll
  for (int k = 0; k < NB; k++) tile[threadIdx.x * (NB + 1) + k] = (k < nb && c < n) ? in[(size_t)k * ld + c] : 0.0;
  __syncthreads();
  const long cnt = ((n - c0) < 256 ? (n - c0) : 256) * NB;       // doubles this block writes
#pragma unroll
  for (int i = 0; i < NB; i++) {
    const long e = (long)i * 256 + threadIdx.x;                  // consecutive threads -> consecutive addresses
    if (e < cnt) out[(size_t)c0 * NB + e] = tile[(e / NB) * (NB + 1) + (e % NB)];
  }
}

// Level-major field (with halo, gathered through src_idx_f) and gradients of one chunk of levels -> records
// out[source cell][3][NB] for the MERGED sweep; zero padded beyond nb levels.  CB cells per block through LDS so that both the
// loads (consecutive cells of one level) and the stores (consecutive doubles of the records) are coalesced.
template <int NB, int CB>
__global__ __launch_bounds__(256) void k_merge3(long n, const int *src_idx_f, const double *f, long ld_f, const double *gx,
                                                const double *gy, long ld_g, int nb, double *out)
{
  constexpr int R = 3 * NB;                                      // doubles per record
  __shared__ double tile[CB * (R + 1)];
  const long c0 = (long)blockIdx.x * CB;
  const int t = threadIdx.x % CB;                                // 256 is a multiple of CB: a thread keeps its cell
  const long c = c0 + t;
  const long cf = (c < n) ? (long)src_idx_f[c] : 0;
  for (int e = threadIdx.x; e < CB * R; e += 256) {
    const int wk = e / CB, w = wk / NB, k = wk % NB;             // array, level; cell fastest
    double v = 0.0;
    if (k < nb && c < n) v = (w == 0) ? f[(size_t)k * ld_f + cf] : ((w == 1) ? gx[(size_t)k * ld_g + c] : gy[(size_t)k * ld_g + c]);
    tile[t * (R + 1) + wk] = v;
  }
  __syncthreads();
  const long cnt = ((n - c0) < CB ? (n - c0) : CB) * R;          // doubles this block writes
  for (long e = threadIdx.x; e < cnt; e += 256) out[(size_t)c0 * R + e] = tile[(e / R) * (R + 1) + (e % R)];
}

// flattened source / destination cell numbers -> (tile, i, j) and (i, j) for fg_plan_get_xgrid
__global__ __launch_bounds__(256) void k_xgrid_indices(long nx, const int *x_src, const int *x_dst, const FgTile *tiles, int ntiles,
                                                        int nx_out, int *t_in, int *i_in, int *j_in, int *i_out, int *j_out)
{
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nx) return;
  const int s = x_src[k], d = x_dst[k];
  int m = 0;
  while (m + 1 < ntiles && s >= tiles[m + 1].cell_off) m++;
  const int loc = s - tiles[m].cell_off, nxt = tiles[m].nx;
  t_in[k] = m; i_in[k] = loc % nxt; j_in[k] = loc / nxt;
  i_out[k] = d % nx_out; j_out[k] = d / nx_out;
}
void fgd_xgrid_indices(long nx, const int *x_src, const int *x_dst, const FgTile *tiles_dev, int ntiles, int nx_out,
                       int *t_in, int *i_in, int *j_in, int *i_out, int *j_out, hipStream_t st)
{
  if (nx > 0) k_xgrid_indices<<<nblk(nx, 256), 256, 0, st>>>(nx, x_src, x_dst, tiles_dev, ntiles, nx_out, t_in, i_in, j_in, i_out, j_out);
}

// interp.c:262-305 (conserve_interp): weights are xarea / (sum of xarea in the destination cell)
__global__ __launch_bounds__(256) void k_apply_frac(int ndst, FgCsr csr, const double *data, double *out)
{
  int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= ndst) return;
  int b = csr.row_ptr[d], e = csr.row_ptr[d + 1];
  double asum = 0.0, acc = 0.0;
  for (int q = b; q < e; q++) asum += csr.e1[q].area;
  for (int q = b; q < e; q++) {
    double frac = csr.e1[q].area / asum;
    acc += data[csr.e1[q].idx_f] * frac;
  }
  out[d] = acc;
}

// deterministic two-stage sum
__global__ __launch_bounds__(256) void k_reduce_partial(const double *v, long n, double *partial)
{
  __shared__ double sh[256];
  double s = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) s += v[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(256) void k_reduce_final(const double *partial, int np, double *result)
{
  __shared__ double sh[256];
  double s = 0;
  for (int i = threadIdx.x; i < np; i += 256) s += partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) *result = sh[0];
}

#define REDUCE_BLOCKS 512

void fgd_csr_count(long nx, const int *x_dst, int *row_cnt, hipStream_t st)
{
  if (nx > 0) k_csr_count<<<nblk(nx, 256), 256, 0, st>>>(nx, x_dst, row_cnt);
}
void fgd_csr_fill(long nx, const int *x_src, const int *x_dst, const int *row_ptr, int *row_fill, FgRowEnt *perm, hipStream_t st)
{
  if (nx > 0) k_csr_fill<<<nblk(nx, 256), 256, 0, st>>>(nx, x_src, x_dst, row_ptr, row_fill, perm);
}
void fgd_csr_fill_pos(long nx_cap, const unsigned long long *nx_dev, const int *x_src, const int *x_dst, const int *row_ptr, const int *x_rowpos, FgRowEnt *perm,
                      hipStream_t st)
{
  if (nx_cap > 0) k_csr_fill_pos<<<nblk(nx_cap, 256), 256, 0, st>>>(nx_cap, nx_dev, x_src, x_dst, row_ptr, x_rowpos, perm);
}
void fgd_csr_sortgather(int order, int ndst, long nx, const FgRowEnt *perm, const double *x_area, const double *x_c1, const double *x_c2,
                        const int *src_idx_f, const FgSrcRec *cen, FgCsr csr, hipStream_t st, int *tmp, long ntmp,
                        int long_rows)
{
  if (ndst <= 0) return;
  FgRowEnt *pm = const_cast<FgRowEnt *>(perm);                     // sorted in place only for runs beyond the LDS staging capacity
  // rows per block: 64 short rows for one wave; 16 long ones, or a single very long one (fine -> very coarse), for four waves
  // (long_rows: the caller knows of a region of long rows under a short mean -- the cells round the pole of a curvilinear target)
  const int mode = nx > 256 * (long)ndst ? 2 : ((nx > 8 * (long)ndst || long_rows) ? 1 : 0);
#define SG(O_, R_, D_) k_csr_sortgather<O_, R_, D_, (R_ >= 64 ? 64 : 256), SG_GROUP><<<nblk(ndst, R_), (R_ >= 64 ? 64 : 256), 0, st>>>(ndst, pm, x_area, x_c1, x_c2, src_idx_f, cen, csr, tmp, ntmp)
#define SGM(O_, D_) do { if (mode == 2) SG(O_, 1, D_); else if (mode == 1) SG(O_, 16, D_); else SG(O_, 64, D_); } while (0)
  if (order == 2) { if (cen) SGM(2, true); else SGM(2, false); }
  else SGM(1, false);
#undef SGM
#undef SG
}
void fgd_src_field_index(int order, const FgTile *tiles_dev, int ntiles, int nsrc, int *src_idx_f, hipStream_t st)
{
  if (nsrc > 0) k_src_field_index<<<nblk(nsrc, 256), 256, 0, st>>>(order, tiles_dev, ntiles, nsrc, src_idx_f);
}
extern int g_apply_xcd, g_apply_ep;
// Rows per tile of the chunked entry-parallel kernels by the mean row length m = nx / ndst: R0 rows for rows of a few exchange
// cells (a tile's cells mostly fit one chunk), fewer rows the longer they are; a single row of any length walks its chunks alone.
// launch(R) gets the choice as a std::integral_constant.
template <int V> using Int = std::integral_constant<int, V>;
template <int R0, int R1, int R2, int R3, typename F>
static void by_row_length(long m, F launch)
{
  if (m <= 6) launch(Int<R0>()); else if (m <= 24) launch(Int<R1>()); else if (m <= 96) launch(Int<R2>()); else launch(Int<R3>());
}
// d_xcd_block's mode for the 8-level entry-parallel kernels: the XCD chunks are twice as many tiles as k_apply_il's
static int xcd_chunk8() { return g_apply_xcd >= 2 ? 2 * g_apply_xcd : g_apply_xcd; }

void fgd_apply1(int order, int ndst, FgCsr csr, const double *f, const double *gx, const double *gy, const int *gmask,
                int has_missing, double missing, double *out, double *row_sum, hipStream_t st, long nx)
{
  if (ndst <= 0) return;
  if (g_apply_ep && nx >= 0) {                             // the entry-parallel single-level kernel; rows per tile by the mean row length
    auto ep1 = [&](auto O, auto M) {
      by_row_length<64, 16, 4, 1>(nx / ndst, [&](auto R) {
        k_apply_ep1<decltype(O)::value, decltype(M)::value, 256, 512, decltype(R)::value><<<nblk(ndst, decltype(R)::value), 256, 0, st>>>(
            ndst, csr, f, gx, gy, gmask, missing, out, row_sum, g_apply_xcd);
      });
    };
    if (order == 2) { if (has_missing) ep1(Int<2>(), std::true_type()); else ep1(Int<2>(), std::false_type()); }
    else            { if (has_missing) ep1(Int<1>(), std::true_type()); else ep1(Int<1>(), std::false_type()); }
    return;
  }
  int grid = nblk(ndst, 256);
  if (order == 2) {
    if (has_missing) k_apply1<2, true><<<grid, 256, 0, st>>>(ndst, csr, f, gx, gy, gmask, missing, out, row_sum);
    else             k_apply1<2, false><<<grid, 256, 0, st>>>(ndst, csr, f, gx, gy, gmask, missing, out, row_sum);
  } else {
    if (has_missing) k_apply1<1, true><<<grid, 256, 0, st>>>(ndst, csr, f, gx, gy, gmask, missing, out, row_sum);
    else             k_apply1<1, false><<<grid, 256, 0, st>>>(ndst, csr, f, gx, gy, gmask, missing, out, row_sum);
  }
}

// k_apply_ep8g with R0 / R1 / R2 / R3 rows per tile (the unmasked callers come here with rows longer than 6 only)
template <int ORDER, bool MASKED, int CAP, int R0, int R1, int R2, int R3>
static void apply_ep8g(int ndst, long nx, FgCsr csr, const double *rec, const unsigned char *gbits, double missing, double *out,
                       double *row_sum, long out_ld, int nb_valid, int xb, hipStream_t st)
{
  by_row_length<R0, R1, R2, R3>(nx / ndst, [&](auto R) {
    k_apply_ep8g<ORDER, MASKED, 256, CAP, decltype(R)::value><<<nblk(ndst, decltype(R)::value), 256, 0, st>>>(
        ndst, csr, rec, gbits, missing, out, row_sum, out_ld, nb_valid, xb);
  });
}

template <int NB, int V>
static void apply_il_nb(int order, int ndst, FgCsr csr, const double *f, const double *gx, const double *gy, double missing,
                        double *out, double *row_sum, long out_ld, int nb_valid, hipStream_t st)
{
  int grid = nblk(ndst, 256 / (NB / V));
  if (order == 2) k_apply_il<2, NB, V><<<grid, 256, 0, st>>>(ndst, csr, f, gx, gy, missing, out, row_sum, out_ld, nb_valid, g_apply_xcd);
  else            k_apply_il<1, NB, V><<<grid, 256, 0, st>>>(ndst, csr, f, gx, gy, missing, out, row_sum, out_ld, nb_valid, g_apply_xcd);
}
// nb in {2, 4, 8, 16}: interleaved fields [cell][nb]; out_ld > 0: write out level-major, out[level][cell] with row stride
// out_ld for the first nb_valid levels (else interleaved [cell][nb])
int g_apply_xcd = 64;  // d_xcd_block: 0 identity, 1 one band per XCD, C >= 2 chunks of C tiles per XCD (measured on the 1440x720 sweep,
                       // 8 levels merged records: 0.0936 ms with C = 32..256, 0.0966 identity, 0.1105 banded)
int g_apply_ep = 1;    // entry-parallel kernel for 8-level sweeps on records (k_apply_ep8): 0.0832 against 0.0872 ms (1440x720 x 8 levels)
int g_apply_vec = 0;   // levels per lane: 0 = auto (4 for nb >= 8, else 2: with chunked tiles 0.0986 against 0.1010 ms on interleaved arrays,
                       // 0.0875 against 0.0937 on records, 1440x720 x 8 levels), or force 1 / 2 / 4
void fgd_apply_il(int order, int nb, int ndst, FgCsr csr, const double *f, const double *gx, const double *gy, double missing,
                  double *out, double *row_sum, long out_ld, int nb_valid, hipStream_t st, long nx)
{
  if (ndst <= 0) return;
  if (order == 1 && nb == 8 && g_apply_ep && nx > 6L * ndst) {   // first order, long rows (fine -> coarse): chunked entry-parallel tiles
    apply_ep8g<1, false, 256, 8, 8, 2, 1>(ndst, nx, csr, f, nullptr, missing, out, row_sum, out_ld, nb_valid, xcd_chunk8(), st);
    return;
  }
  const int v = g_apply_vec ? g_apply_vec : (nb >= 8 ? 4 : 2);
#define AP(NB_) do { if (v >= 4 && NB_ >= 4) apply_il_nb<NB_, (NB_ >= 4 ? 4 : 2)>(order, ndst, csr, f, gx, gy, missing, out, row_sum, out_ld, nb_valid, st); \
                     else if (v >= 2) apply_il_nb<NB_, 2>(order, ndst, csr, f, gx, gy, missing, out, row_sum, out_ld, nb_valid, st); \
                     else apply_il_nb<NB_, 1>(order, ndst, csr, f, gx, gy, missing, out, row_sum, out_ld, nb_valid, st); } while (0)
  if (nb == 16) AP(16);
  else if (nb == 8) AP(8);
  else if (nb == 4) AP(4);
  else AP(2);
#undef AP
}
// order-2 sweep on merged records (k_merge3); same arguments otherwise
void fgd_apply_il_merged(int nb, int ndst, long nx, FgCsr csr, const double *rec, double missing, double *out, double *row_sum, long out_ld,
                         int nb_valid, hipStream_t st)
{
  if (ndst <= 0) return;
#define APM(NB_, V_) k_apply_il<2, NB_, V_, true><<<nblk(ndst, 256 / (NB_ / V_)), 256, 0, st>>>(ndst, csr, rec, nullptr, nullptr, missing, out, row_sum, out_ld, nb_valid, g_apply_xcd)
  if (nb == 16) APM(16, 4);
  else if (nb == 8 && g_apply_ep && nx <= 6L * ndst)       // rows of ~4 exchange cells: a tile's cells fit the product table
    k_apply_ep8<256, 256><<<nblk(ndst, EP_ROWS), 256, 0, st>>>(ndst, csr, rec, missing, out, row_sum, out_ld, nb_valid, xcd_chunk8());
  else if (nb == 8 && g_apply_ep)                          // longer rows: chunked tiles, rows per tile by the mean row length
    apply_ep8g<2, false, 256, 8, 8, 2, 1>(ndst, nx, csr, rec, nullptr, missing, out, row_sum, out_ld, nb_valid, xcd_chunk8(), st);
  else if (nb == 8) { if (g_apply_vec == 2) APM(8, 2); else APM(8, 4); }   // 4 levels per lane: 0.0875 ms against 0.0936 with 2 (1440x720, 8 levels, chunked tiles)
  else if (nb == 4) APM(4, 2);
  else APM(2, 2);
#undef APM
}
// eight levels with missing values of their own, fields and output as k_apply_ep8g's MASKED form takes them
void fgd_apply_levels8(int order, int ndst, long nx, FgCsr csr, const double *rec, const unsigned char *gbits, double missing, double *out,
                       double *row_sum, long ld, int nb_valid, hipStream_t st)
{
  if (ndst <= 0) return;
  if (order == 2) apply_ep8g<2, true, FG_LEVELS_CAP, 32, 8, 2, 1>(ndst, nx, csr, rec, gbits, missing, out, row_sum, ld, nb_valid, 0, st);
  else            apply_ep8g<1, true, FG_LEVELS_CAP, 32, 8, 2, 1>(ndst, nx, csr, rec, gbits, missing, out, row_sum, ld, nb_valid, 0, st);
}
// the same with the options of FgApplyEx (k_apply_ep8x); fa8 != null: the per-level area, interleaved [source cell][8].  Rows per
// tile by the mean row length, so that a tile's exchange cells about fill one chunk: 32 / 16 / 2 / 1 rows on chunks of
// FG_LEVELS_EX_CAP, 16 / 8 / 2 / 1 on the chunks of half that size the per-level table leaves room for.
void fgd_apply_levels8x(int order, int ndst, long nx, FgCsr csr, const double *rec, const unsigned char *gbits, FgApplyEx o, const double *fa8,
                        double *out, double *row_sum, long ld, int nb_valid, int *err, hipStream_t st)
{
  if (ndst <= 0) return;
  auto go = [&](auto O) {
    constexpr int ORD = decltype(O)::value;
    if (fa8)
      by_row_length<16, 8, 2, 1>(nx / ndst, [&](auto R) {
        k_apply_ep8x<ORD, true, 256, FG_LEVELS_EX_CAP_Z, decltype(R)::value><<<nblk(ndst, decltype(R)::value), 256, 0, st>>>(
            ndst, csr, rec, gbits, o, fa8, out, row_sum, ld, nb_valid, err);
      });
    else
      by_row_length<32, 16, 2, 1>(nx / ndst, [&](auto R) {
        k_apply_ep8x<ORD, false, 256, FG_LEVELS_EX_CAP, decltype(R)::value><<<nblk(ndst, decltype(R)::value), 256, 0, st>>>(
            ndst, csr, rec, gbits, o, nullptr, out, row_sum, ld, nb_valid, err);
      });
  };
  if (order == 2) go(Int<2>()); else go(Int<1>());
}
void fgd_gmask_bits(long n, const int *gmask, long ld, int nb, unsigned char *bits, hipStream_t st)
{
  if (n > 0) k_gmask_bits<<<nblk(n, 256), 256, 0, st>>>(n, gmask, ld, nb, bits);
}
void fgd_merge3(int nb_pad, long n, const int *src_idx_f, const double *f, long ld_f, const double *gx, const double *gy, long ld_g,
                int nb_valid, double *out, hipStream_t st)
{
  if (n <= 0) return;
  if (nb_pad == 16) k_merge3<16, 64><<<nblk(n, 64), 256, 0, st>>>(n, src_idx_f, f, ld_f, gx, gy, ld_g, nb_valid, out);
  else if (nb_pad == 8) k_merge3<8, 64><<<nblk(n, 64), 256, 0, st>>>(n, src_idx_f, f, ld_f, gx, gy, ld_g, nb_valid, out);
  else if (nb_pad == 4) k_merge3<4, 128><<<nblk(n, 128), 256, 0, st>>>(n, src_idx_f, f, ld_f, gx, gy, ld_g, nb_valid, out);
  else k_merge3<2, 128><<<nblk(n, 128), 256, 0, st>>>(n, src_idx_f, f, ld_f, gx, gy, ld_g, nb_valid, out);
}
// level-major [nb_valid][n] (row stride ld) -> interleaved [n][nb_pad] (zero padded), and back
void fgd_interleave(int nb_pad, long n, const double *in, long ld, int nb_valid, double *out, hipStream_t st)
{
  if (n <= 0) return;
  if (nb_pad == 16) k_interleave<16><<<nblk(n, 256), 256, 0, st>>>(n, in, ld, nb_valid, out);
  else if (nb_pad == 8) k_interleave<8><<<nblk(n, 256), 256, 0, st>>>(n, in, ld, nb_valid, out);
  else if (nb_pad == 4) k_interleave<4><<<nblk(n, 256), 256, 0, st>>>(n, in, ld, nb_valid, out);
  else k_interleave<2><<<nblk(n, 256), 256, 0, st>>>(n, in, ld, nb_valid, out);
}
// three arrays at once (f, grad_x, grad_y of one chunk of levels); narr = 1 or 3
void fgd_interleave3(int nb_pad, int narr, const double *const *in, const long *ld, const long *n, double *const *out, int nb_valid,
                     hipStream_t st)
{
  FgIl3 a;
  long nmax = 0;
  for (int w = 0; w < 3; w++) {
    a.in[w] = (w < narr) ? in[w] : nullptr; a.out[w] = (w < narr) ? out[w] : nullptr;
    a.n[w] = (w < narr) ? n[w] : 0; a.ld[w] = (w < narr) ? ld[w] : 0;
    if (a.n[w] > nmax) nmax = a.n[w];
  }
  if (nmax <= 0) return;
  dim3 grid(nblk(nmax, 256), narr);
  if (nb_pad == 16) k_interleave3<16><<<grid, 256, 0, st>>>(a, nb_valid);
  else if (nb_pad == 8) k_interleave3<8><<<grid, 256, 0, st>>>(a, nb_valid);
  else if (nb_pad == 4) k_interleave3<4><<<grid, 256, 0, st>>>(a, nb_valid);
  else k_interleave3<2><<<grid, 256, 0, st>>>(a, nb_valid);
}
void fgd_deinterleave(int nb_pad, long n, const double *in, long ld, int nb_valid, double *out, hipStream_t st)
{
  if (n <= 0) return;
  if (nb_pad == 16) k_deinterleave<16><<<nblk(n, 256), 256, 0, st>>>(n, in, ld, nb_valid, out);
  else if (nb_pad == 8) k_deinterleave<8><<<nblk(n, 256), 256, 0, st>>>(n, in, ld, nb_valid, out);
  else if (nb_pad == 4) k_deinterleave<4><<<nblk(n, 256), 256, 0, st>>>(n, in, ld, nb_valid, out);
  else k_deinterleave<2><<<nblk(n, 256), 256, 0, st>>>(n, in, ld, nb_valid, out);
}
void fgd_apply_ex(int order, int ndst, FgCsr csr, const double *f, const double *gx, const double *gy, FgApplyEx o,
                  double *out, double *row_sum, int *err, hipStream_t st, long nx)
{
  if (ndst <= 0) return;
  if (g_apply_ep && nx >= 0) {                             // entry-parallel; rows per tile by the mean row length
    auto epx = [&](auto O, auto M) {
      by_row_length<64, 16, 4, 1>(nx / ndst, [&](auto R) {
        k_apply_epx<decltype(O)::value, decltype(M)::value, 256, 512, decltype(R)::value><<<nblk(ndst, decltype(R)::value), 256, 0, st>>>(
            ndst, csr, f, gx, gy, o, out, row_sum, err, g_apply_xcd);
      });
    };
    if (order == 2) { if (o.xdata) epx(Int<2>(), std::true_type()); else epx(Int<2>(), std::false_type()); }
    else epx(Int<1>(), std::false_type());
    return;
  }
  int grid = nblk(ndst, 256);
  if (order == 2) {
    if (o.xdata) k_apply_ex<2, true><<<grid, 256, 0, st>>>(ndst, csr, f, gx, gy, o, out, row_sum, err);
    else         k_apply_ex<2, false><<<grid, 256, 0, st>>>(ndst, csr, f, gx, gy, o, out, row_sum, err);
  } else
    k_apply_ex<1, false><<<grid, 256, 0, st>>>(ndst, csr, f, gx, gy, o, out, row_sum, err);
}
void fgd_mono_bounds(const FgTile *tiles_dev, int ntiles, int nsrc, const int *src_idx_f, const double *f, double missing,
                     double *fbmax, double *fbmin, double *fmax, double *fmin, hipStream_t st)
{
  if (nsrc > 0) k_mono_bounds<<<nblk(nsrc, 256), 256, 0, st>>>(tiles_dev, ntiles, nsrc, src_idx_f, f, missing, fbmax, fbmin, fmax, fmin);
}
void fgd_mono_xdata(long nx, FgCsr csr, const double *f, const double *gx, const double *gy, const int *gmask, double missing,
                    double *xdata, double *fmax, double *fmin, hipStream_t st)
{
  if (nx > 0) k_mono_xdata<<<nblk(nx, 256), 256, 0, st>>>(nx, csr, f, gx, gy, gmask, missing, xdata, fmax, fmin);
}
void fgd_mono_limit(long nx, FgCsr csr, const double *f, double missing, const double *fbmax, const double *fbmin,
                    const double *fmax, const double *fmin, double *xdata, int *err, hipStream_t st)
{
  if (nx > 0) k_mono_limit<<<nblk(nx, 256), 256, 0, st>>>(nx, csr, f, missing, fbmax, fbmin, fmax, fmin, xdata, err);
}
void fgd_mono_bounds8(const FgTile *tiles_dev, int ntiles, int nsrc, const int *src_idx_f, const double *f, long ld_f, int nb,
                      double missing, double *b8, hipStream_t st)
{
  if (nsrc > 0) k_mono_bounds8<64><<<nblk(nsrc, 64), 256, 0, st>>>(tiles_dev, ntiles, nsrc, src_idx_f, f, ld_f, nb, missing, b8);
}
void fgd_mono_extremes8(long nx, FgCsr csr, const double *rec, const unsigned char *gbits, double missing, int nb, double *b8,
                        hipStream_t st)
{
  if (nx > 0) k_mono_extremes8<<<nblk(nx * 8, 256), 256, 0, st>>>(nx, csr, rec, gbits, missing, nb, b8);
}
void fgd_mono_reset8(int nsrc, double *b8, hipStream_t st)
{
  if (nsrc > 0) k_mono_reset8<<<nblk((long)nsrc * 16, 256), 256, 0, st>>>(nsrc, b8);
}
void fgd_mono_minmax8(int nsrc, int nz, int to_b8, double *b8, double *f_min, double *f_max, hipStream_t st)
{
  if (nsrc > 0 && nz > 0) k_mono_minmax8<<<nblk((long)nsrc * nz, 256), 256, 0, st>>>(nsrc, nz, to_b8, b8, f_min, f_max);
}
// rows per tile by the mean row length, so that a tile's exchange cells about fill one chunk of FG_LEVELS_MONO_CAP
void fgd_apply_levels8m(int ndst, long nx, FgCsr csr, const double *rec, const unsigned char *gbits, const double *b8, FgApplyEx o,
                        double *out, double *row_sum, long ld, int nb_valid, int *err, hipStream_t st)
{
  if (ndst <= 0) return;
  by_row_length<16, 8, 2, 1>(nx / ndst, [&](auto R) {
    k_apply_ep8m<256, FG_LEVELS_MONO_CAP, decltype(R)::value><<<nblk(ndst, decltype(R)::value), 256, 0, st>>>(
        ndst, csr, rec, gbits, b8, o, out, row_sum, ld, nb_valid, err);
  });
}

void fgd_apply_frac(int ndst, FgCsr csr, const double *data, double *out, hipStream_t st)
{
  if (ndst > 0) k_apply_frac<<<nblk(ndst, 256), 256, 0, st>>>(ndst, csr, data, out);
}
void fgd_reduce_sum(const double *v, long n, double *partial, double *result, hipStream_t st)
{
  k_reduce_partial<<<REDUCE_BLOCKS, 256, 0, st>>>(v, n, partial);
  k_reduce_final<<<1, 256, 0, st>>>(partial, REDUCE_BLOCKS, result);
}
