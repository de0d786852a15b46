// bilinear_kernels.hip -- fregrid's bilinear cubed-sphere -> lat-lon path on the device
// (tools/fregrid/bilinear_interp.c: setup_bilinear_interp :72-434, do_c2l_interp :562-616,
// do_vector_bilinear_interp :476-560, do_latlon_coarsening / redu2x :994-1155).
//
//   k_bl_window     per cubed-sphere cell and sweep `iter`: the reference's lat-lon window (:150-169) -> pair count
//   k_scan_*        exclusive scan of the pair counts (three plain kernels, no inter-block waiting)
//   k_bl_pairs      one lane per (cell, window point) pair: nearest of the <= 4 centres, get_closest_index (:648-818);
//                   a success does a 64-bit atomicMin of the packed (tile, jc, ic) key of the cell, followed by the lower-left
//                   corner it found
//   k_bl_finalize   per point: the minimum key is the reference's first success in loop order -> index, found;
//                   counts the points still unfound (the next sweep's kernels return at once when that count is 0)
//   k_bl_weight_*   per point: the three cube-corner cases and the general case (:260-406), around a host pass
//   k_bl_gather_*   the 4-point gather with the reference's missing-value test, nz levels per lane; the vector form
//                   projects (u, v) onto x, y, z at each corner and rotates back in the same pass
//   k_redu2x_*      the coarsening of finer_step > 0, its missing-value quirk included
//   k_bl_stream_*   the field loop (fg_bilin_sweep): the gathers on a chunk of eight levels in the file's type, widened at the
//                   corner and narrowed at the point; k_redu2x_y_typed narrows behind the last coarsening step
//
// Comparisons: get_closest_index compares spherical angles (acosl in the reference).  They are taken with the fast acos and
// redone with fp80.h's fg_acosl when the two sides are within 1e-13 (relative) of each other.  The nearest-centre choice
// compares normalize_great_circle_distance values the same way with acos_dd.h's correctly rounded fg_acos_cr as the exact side;
// where the two correctly rounded distances are equal or one ulp apart -- the only comparisons libm's own rounding could
// decide otherwise -- a counter is raised (fg_bilin_ambiguous_ties).  The libm acos / sin / asin of the search windows and of
// the weights (with the acosl of the weights' spherical angles) are evaluated on the host (bilinear_host.c).  Every double expression keeps the reference's tree
// (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#define FG_HDN __host__ __device__ static      // gc_kernels.hip holds the library's external copies of fp80.h's functions
#include "fp80.h"
#include "acos_dd.h"
#include "bilinear.h"
#include "fregrid_hip.h"                       // FG_NC_*: the file types of the field loop's kernels

#define BL_PI 3.14159265358979323846
#define BL_EPSLN30 (1.e-30)
#define BL_MAXKEY 0xffffffffffffffffULL
#define BL_IBITS 13                   // key = cell << 26 | ic << 13 | jc of the result: N <= 8191 (fg_bilin_create checks)
#define BL_IMASK ((1ULL << BL_IBITS) - 1)


__device__ __forceinline__ double bl_max(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double bl_min(double a, double b) { return a < b ? a : b; }

// spherical_angle, mosaic_util.c:800-836 (double branch); EXACT: acosl as the reference's x87 build rounds it.  arg (may be
// null): the argument handed to acosl, NaN where the angle comes from another branch
template <bool EXACT>
__device__ double bl_angle(const double *v1, const double *v2, const double *v3, double *arg = nullptr)
{
  double angle, px, py, pz, qx, qy, qz, ddd;
  if (arg) *arg = __builtin_nan("");
  px = v1[1] * v2[2] - v1[2] * v2[1];
  py = v1[2] * v2[0] - v1[0] * v2[2];
  pz = v1[0] * v2[1] - v1[1] * v2[0];
  qx = v1[1] * v3[2] - v1[2] * v3[1];
  qy = v1[2] * v3[0] - v1[0] * v3[2];
  qz = v1[0] * v3[1] - v1[1] * v3[0];
  ddd = (px * px + py * py + pz * pz) * (qx * qx + qy * qy + qz * qz);
  if (ddd <= 0.0) angle = 0.;
  else {
    ddd = (px * qx + py * qy + pz * qz) / sqrt(ddd);
    if (fabs(ddd - 1) < BL_EPSLN30) ddd = 1;
    if (fabs(ddd + 1) < BL_EPSLN30) ddd = -1;
    if (ddd > 1. || ddd < -1.) angle = (ddd < 0.) ? BL_PI : 0.;
    else {
      angle = EXACT ? fg_acosl(ddd) : acos(ddd);
      if (arg) *arg = ddd;
    }
  }
  return angle;
}

// the cosine normalize_great_circle_distance hands to acos (:746-752)
__device__ __forceinline__ double bl_gcd_cos(const double *v1, const double *v2)
{
  double dist = (v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]) /
                sqrt((v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]) * (v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2]));
  const double m = bl_min(1., fabs(dist));
  return dist < 0 ? -fabs(m) : fabs(m);
}

// max(angle(a), angle(b)) <= angle(c), each angle at its own vertex o: fast first, exact when the sides are close
struct BlTri { const double *o, *p, *q; };
__device__ bool bl_le(BlTri a, BlTri b, BlTri c)
{
  double A = bl_angle<false>(a.o, a.p, a.q), B = bl_angle<false>(b.o, b.p, b.q), Cc = bl_angle<false>(c.o, c.p, c.q);
  double m = bl_max(A, B);
  if (fabs(m - Cc) > 1.e-13 * fmax(fabs(m), fabs(Cc))) return m <= Cc;
  A = bl_angle<true>(a.o, a.p, a.q); B = bl_angle<true>(b.o, b.p, b.q); Cc = bl_angle<true>(c.o, c.p, c.q);
  return bl_max(A, B) <= Cc;
}

__device__ __forceinline__ void bl_ld(const BlGeom &g, long off, int n, double *v)
{
  v[0] = g.xt[off + n]; v[1] = g.yt[off + n]; v[2] = g.zt[off + n];
}

// get_closest_index (:648-818) for cell (i_in, j_in) of tile l and point v0.  Returns the quadrant of the lower-left
// corner (0: (i, j), 1: (i-1, j), 2: (i-1, j-1), 3: (i, j-1)) or -1.
__device__ int bl_closest(const BlGeom &g, long off, int i_in, int j_in, const double *v0)
{
  const int nx_in = g.N, ny_in = g.N, nxd = g.N + 2;
  double v1[3], v2[3], v3[3], v4[3], v5[3], v6[3], v7[3], v8[3];
  bl_ld(g, off, j_in * nxd + i_in, v1);
  bl_ld(g, off, j_in * nxd + i_in + 1, v2);
  bl_ld(g, off, (j_in + 1) * nxd + i_in, v3);
  if (bl_le({v1, v2, v0}, {v1, v3, v0}, {v1, v2, v3})) {
    bool ok;
    if (i_in == nx_in && j_in == ny_in) ok = bl_le({v2, v1, v0}, {v2, v3, v0}, {v2, v3, v1});
    else {
      bl_ld(g, off, (j_in + 1) * nxd + i_in + 1, v4);
      ok = bl_le({v4, v2, v0}, {v4, v3, v0}, {v4, v3, v2});
    }
    return ok ? 0 : -1;
  }
  bl_ld(g, off, j_in * nxd + i_in - 1, v4);
  if (bl_le({v1, v3, v0}, {v1, v4, v0}, {v1, v3, v4})) {
    bool ok;
    if (i_in == 1 && j_in == ny_in) ok = bl_le({v3, v4, v0}, {v3, v1, v0}, {v3, v1, v4});
    else {
      bl_ld(g, off, (j_in + 1) * nxd + i_in - 1, v5);
      bl_ld(g, off, j_in * nxd + i_in - 1, v6);
      ok = bl_le({v5, v6, v0}, {v5, v3, v0}, {v5, v3, v6});
    }
    return ok ? 1 : -1;
  }
  bl_ld(g, off, j_in * nxd + i_in - 1, v5);
  bl_ld(g, off, (j_in - 1) * nxd + i_in, v6);
  if (bl_le({v1, v4, v0}, {v1, v6, v0}, {v1, v5, v6}) && i_in > 1 && j_in > 1) {
    bl_ld(g, off, (j_in - 1) * nxd + i_in - 1, v7);
    return bl_le({v7, v5, v0}, {v7, v6, v0}, {v7, v6, v5}) ? 2 : -1;
  }
  if (bl_le({v1, v6, v0}, {v1, v2, v0}, {v1, v6, v2})) {
    bool ok;
    if (i_in == nx_in && j_in == 1) ok = bl_le({v2, v6, v0}, {v2, v1, v0}, {v2, v1, v6});
    else {
      bl_ld(g, off, (j_in - 1) * nxd + i_in + 1, v8);
      ok = bl_le({v8, v6, v0}, {v8, v2, v0}, {v8, v2, v6});
    }
    return ok ? 3 : -1;
  }
  return -1;
}


// the search window of cell c in sweep iter (:150-169)
__global__ __launch_bounds__(256) void k_bl_window(BlGeom g, int iter, double dlon, double dlat, double lonbegin, double latbegin,
                                                   const unsigned *unfound, BlWin *win, unsigned long long *cnt)
{
  if (iter > 1 && unfound[iter - 1] == 0) return;
  const long ncell = 6L * g.N * g.N;
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell) return;
  const int N = g.N, nxd = N + 2;
  const int l = (int)(c / ((long)N * N));
  const int rem = (int)(c - (long)l * N * N);
  const int jc = rem / N + 1, ic = rem % N + 1;
  const long off = (long)l * nxd * nxd;
  const int n1 = jc * nxd + ic, n2 = (jc + 1) * nxd + ic + 1;
  (void)n2;                                      // (jc+1, ic+1): its distance is g.cell_dist[c], host libm acos
  const double dcub = iter * g.cell_dist[c];
  const double lat = g.latt[off + n1], lon = g.lont[off + n1];
  const int j_min = (int)bl_max(1, floor((lat - dcub - latbegin) / dlat) - iter + 1);
  const int j_max = (int)bl_min(g.nyo, ceil((lat + dcub - latbegin) / dlat) + iter - 1);
  int i_min, i_max;
  if (j_min == 1 || j_max == g.nyo) { i_min = 1; i_max = g.nxo; }
  else {
    i_min = (int)bl_max(1, floor((lon - dcub - lonbegin) / dlon - iter + 1));
    i_max = (int)bl_min(g.nxo, ceil((lon + dcub - lonbegin) / dlon + iter - 1));
  }
  BlWin w = {i_min - 1, i_max - 1, j_min - 1, j_max - 1};
  win[c] = w;
  const long ni = (long)i_max - i_min + 1, nj = (long)j_max - j_min + 1;
  cnt[c] = (ni > 0 && nj > 0) ? (unsigned long long)(ni * nj) : 0ULL;
}

// ---- exclusive scan of n counts (block of 256 lanes x 4 elements), block sums scanned by one block
#define BL_SCAN_B 256
#define BL_SCAN_E 4
__device__ unsigned long long bl_block_scan(unsigned long long v, unsigned long long *sh)
{
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < BL_SCAN_B; d <<= 1) {
    unsigned long long a = (t >= d) ? sh[t - d] : 0ULL;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const unsigned long long incl = sh[t];
  __syncthreads();
  return incl - v;                               // exclusive
}

__global__ __launch_bounds__(BL_SCAN_B) void k_scan_local(int iter, const unsigned *unfound, const unsigned long long *in, long n,
                                                          unsigned long long *out, unsigned long long *bsum)
{
  if (iter > 1 && unfound[iter - 1] == 0) return;
  __shared__ unsigned long long sh[BL_SCAN_B];
  const long base = (long)blockIdx.x * BL_SCAN_B * BL_SCAN_E + (long)threadIdx.x * BL_SCAN_E;
  unsigned long long e[BL_SCAN_E], s = 0;
  for (int k = 0; k < BL_SCAN_E; k++) { e[k] = (base + k < n) ? in[base + k] : 0ULL; s += e[k]; }
  unsigned long long ex = bl_block_scan(s, sh);
  for (int k = 0; k < BL_SCAN_E; k++) { if (base + k < n) out[base + k] = ex; ex += e[k]; }
  if (threadIdx.x == BL_SCAN_B - 1) bsum[blockIdx.x] = ex;
}

__global__ __launch_bounds__(BL_SCAN_B) void k_scan_sums(int iter, const unsigned *unfound, unsigned long long *bsum, long nb,
                                                         unsigned long long *total)
{
  if (iter > 1 && unfound[iter - 1] == 0) return;
  __shared__ unsigned long long sh[BL_SCAN_B];
  unsigned long long carry = 0;
  for (long b0 = 0; b0 < nb; b0 += BL_SCAN_B) {
    const long b = b0 + threadIdx.x;
    const unsigned long long v = (b < nb) ? bsum[b] : 0ULL;
    const unsigned long long ex = bl_block_scan(v, sh);
    if (b < nb) bsum[b] = carry + ex;
    if (threadIdx.x == BL_SCAN_B - 1) sh[0] = ex + v;
    __syncthreads();
    carry += sh[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(BL_SCAN_B) void k_scan_add(int iter, const unsigned *unfound, unsigned long long *out, long n,
                                                        const unsigned long long *bsum)
{
  if (iter > 1 && unfound[iter - 1] == 0) return;
  const long base = (long)blockIdx.x * BL_SCAN_B * BL_SCAN_E + (long)threadIdx.x * BL_SCAN_E;
  const unsigned long long add = bsum[blockIdx.x];
  for (int k = 0; k < BL_SCAN_E; k++) if (base + k < n) out[base + k] += add;
}

// one lane per (cell, window point) pair, grid-stride over the device-side total
__global__ __launch_bounds__(256) void k_bl_pairs(BlGeom g, int iter, const unsigned *unfound, const BlWin *win,
                                                  const unsigned long long *off, const unsigned long long *total,
                                                  const int *found, unsigned long long *key, unsigned *ties)
{
  if (iter > 1 && unfound[iter - 1] == 0) return;
  const long ncell = 6L * g.N * g.N;
  const unsigned long long tot = *total;
  const int N = g.N, nxd = N + 2;
  for (unsigned long long p = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; p < tot;
       p += (unsigned long long)gridDim.x * blockDim.x) {
    long lo = 0, hi = ncell - 1;                 // last cell with off <= p
    while (lo < hi) {
      const long mid = (lo + hi + 1) >> 1;
      if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const long c = lo;
    const BlWin w = win[c];
    const long ni = (long)w.i1 - w.i0 + 1;
    const long q = (long)(p - off[c]);
    const int j = w.j0 + (int)(q / ni), i = w.i0 + (int)(q % ni);
    const long n0 = (long)j * g.nxo + i;
    if (found[n0]) continue;
    const int l = (int)(c / ((long)N * N));
    const int rem = (int)(c - (long)l * N * N);
    const int jc = rem / N + 1, ic = rem % N + 1;
    const long toff = (long)l * nxd * nxd;
    const double v0[3] = {g.xo[n0], g.yo[n0], g.zo[n0]};
    // nearest centre among (ic..ic+1, jc..jc+1) clipped to the tile (:175-194): strict <, first wins
    int bi = ic, bj = jc;
    double bc = 0.0, bf = 0.0;
    bool have = false;
    for (int jcc = jc; jcc <= min(N, jc + 1); jcc++)
      for (int icc = ic; icc <= min(N, ic + 1); icc++) {
        double v1[3];
        bl_ld(g, toff, jcc * nxd + icc, v1);
        const double cs = bl_gcd_cos(v1, v0), f = acos(cs);
        bool less;
        if (!have) less = true;                  // shortest starts at 2*pi
        else if (fabs(f - bf) > 1.e-13 * fmax(f, bf)) less = f < bf;
        else {
          const double a = fg_acos_cr(cs), b = fg_acos_cr(bc);
          less = a < b;
          // different arguments whose correctly rounded distances are equal or adjacent: libm's rounding could order them
          // otherwise (equal arguments give equal results in any acos)
          if (cs != bc && (a == b || nextafter(a, b) == b)) atomicAdd(ties, 1u);
        }
        if (less) { bi = icc; bj = jcc; bc = cs; bf = f; have = true; }
      }
    const int quad = bl_closest(g, toff, bi, bj, v0);
    if (quad >= 0) {                             // the lower-left corner is relative to the nearest centre (bi, bj)
      const unsigned long long ri = (quad == 0 || quad == 3) ? bi : bi - 1, rj = (quad == 0 || quad == 1) ? bj : bj - 1;
      const unsigned long long k = ((unsigned long long)c << (2 * BL_IBITS)) | (ri << BL_IBITS) | rj;
      if (k < key[n0]) atomicMin(&key[n0], k);
    }
  }
}

// per point: the first success of the sweep in the reference's loop order -> index; count what is still missing
__global__ __launch_bounds__(256) void k_bl_finalize(int N, long npts, int iter, unsigned *unfound, int *found,
                                                     const unsigned long long *key, int *index)
{
  if (iter > 1 && unfound[iter - 1] == 0) { if (blockIdx.x == 0 && threadIdx.x == 0) unfound[iter] = 0; return; }
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  bool miss = false;
  if (n < npts && !found[n]) {
    const unsigned long long k = key[n];
    if (k != BL_MAXKEY) {
      const long c = (long)(k >> (2 * BL_IBITS));
      index[3 * n] = (int)((k >> BL_IBITS) & BL_IMASK);
      index[3 * n + 1] = (int)(k & BL_IMASK);
      index[3 * n + 2] = (int)(c / ((long)N * N));
      found[n] = 1;
    } else miss = true;
  }
  const unsigned long long b = __ballot(miss);
  if ((threadIdx.x & (warpSize - 1)) == 0 && b) atomicAdd(&unfound[iter], (unsigned)__popcll(b));
}

// weights (:260-406) in two device passes around the host: k_bl_weight_sides writes, for each dist2side call of the point's
// case (at most 4, in the reference's order), the spherical angle, the argument spherical_angle hands to acosl (NaN where
// the angle comes from another branch) and the cosine normalize_great_circle_distance hands to acos; the host then takes
// acosl of the argument and evaluates asin(sin(acos(cos)) * sin(angle)) with its own libm (bilinear_host.c:
// fg_bilin_dist2side_tail), and k_bl_weight_final combines the distances.  Unused slots: angle 0, argument NaN, cos 1.
// fg_acosl rounds correctly; the reference rounds x87 acosl's long double to double, which differs in the last place at a
// few arguments, so the weights take acosl from the host like the other libm calls.
__device__ __forceinline__ void bl_side(const double *v1, const double *v2, const double *point, double *angle, double *arg,
                                        double *cs)
{
  *angle = bl_angle<true>(v1, v2, point, arg);
  *cs = bl_gcd_cos(v1, point);
}

__global__ __launch_bounds__(256) void k_bl_weight_sides(BlGeom g, long npts, const int *index, double *angle, double *acos_arg,
                                                         double *side_cos)
{
  const long n0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n0 >= npts) return;
  const int N = g.N, nxd = N + 2;
  const int ic = index[3 * n0], jc = index[3 * n0 + 1], l = index[3 * n0 + 2];
  const long off = (long)l * nxd * nxd;
  const double v0[3] = {g.xo[n0], g.yo[n0], g.zo[n0]};
  const double nan = __builtin_nan("");
  double v1[3], v2[3], v3[3], v4[3], a[4] = {0., 0., 0., 0.}, x[4] = {nan, nan, nan, nan}, c[4] = {1., 1., 1., 1.};
  if (ic == N && jc == N) {
    bl_ld(g, off, jc * nxd + ic, v1); bl_ld(g, off, jc * nxd + ic + 1, v2); bl_ld(g, off, (jc + 1) * nxd + ic, v3);
    bl_side(v2, v3, v0, &a[0], &x[0], &c[0]); bl_side(v2, v1, v0, &a[1], &x[1], &c[1]); bl_side(v1, v3, v0, &a[2], &x[2], &c[2]);
  } else if (ic == 0 && jc == N) {
    bl_ld(g, off, jc * nxd + ic, v1); bl_ld(g, off, jc * nxd + ic + 1, v2); bl_ld(g, off, (jc + 1) * nxd + ic + 1, v3);
    bl_side(v3, v2, v0, &a[0], &x[0], &c[0]); bl_side(v2, v1, v0, &a[1], &x[1], &c[1]); bl_side(v3, v1, v0, &a[2], &x[2], &c[2]);
  } else if (jc == 0 && ic == N) {
    bl_ld(g, off, jc * nxd + ic, v1); bl_ld(g, off, (jc + 1) * nxd + ic, v2); bl_ld(g, off, (jc + 1) * nxd + ic + 1, v3);
    bl_side(v2, v3, v0, &a[0], &x[0], &c[0]); bl_side(v1, v3, v0, &a[1], &x[1], &c[1]); bl_side(v1, v2, v0, &a[2], &x[2], &c[2]);
  } else {
    bl_ld(g, off, jc * nxd + ic, v1); bl_ld(g, off, jc * nxd + ic + 1, v2);
    bl_ld(g, off, (jc + 1) * nxd + ic, v3); bl_ld(g, off, (jc + 1) * nxd + ic + 1, v4);
    bl_side(v1, v3, v0, &a[0], &x[0], &c[0]); bl_side(v3, v4, v0, &a[1], &x[1], &c[1]); bl_side(v4, v2, v0, &a[2], &x[2], &c[2]);
    bl_side(v2, v1, v0, &a[3], &x[3], &c[3]);
  }
  for (int k = 0; k < 4; k++) { angle[4 * n0 + k] = a[k]; acos_arg[4 * n0 + k] = x[k]; side_cos[4 * n0 + k] = c[k]; }
}

__global__ __launch_bounds__(256) void k_bl_weight_final(long npts, int N, const int *index, const double *dist, double *weight)
{
  const long n0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n0 >= npts) return;
  const int ic = index[3 * n0], jc = index[3 * n0 + 1];
  const double d1 = dist[4 * n0], d2 = dist[4 * n0 + 1], d3 = dist[4 * n0 + 2], d4 = dist[4 * n0 + 3];
  double w[4];
  if (ic == N && jc == N) {
    w[0] = d1; w[1] = d2; w[2] = 0.; w[3] = d3;
    const double sum = w[0] + w[1] + w[3];
    w[0] /= sum; w[1] /= sum; w[3] /= sum;
  } else if (ic == 0 && jc == N) {
    w[0] = d1; w[1] = 0.; w[2] = d2; w[3] = d3;
    const double sum = w[0] + w[2] + w[3];
    w[0] /= sum; w[2] /= sum; w[3] /= sum;
  } else if (jc == 0 && ic == N) {
    w[0] = d1; w[1] = d2; w[2] = d3; w[3] = 0.;
    const double sum = w[0] + w[1] + w[2];
    w[0] /= sum; w[1] /= sum; w[2] /= sum;
  } else {
    w[0] = d2 * d3; w[1] = d3 * d4; w[2] = d4 * d1; w[3] = d1 * d2;
    const double sum = w[0] + w[1] + w[2] + w[3];
    w[0] /= sum; w[1] /= sum; w[2] /= sum; w[3] /= sum;
  }
  for (int k = 0; k < 4; k++) weight[4 * n0 + k] = w[k];
}

// per point: the halo'd elements of the four corners in do_c2l_interp's order (:579-582) -> the unpadded cell each holds
// after the halo update (-1: a halo corner, init_halo's zero)
__global__ __launch_bounds__(256) void k_bl_corners(int N, long npts, const int *index, const int *cell_of, int *elem, int *cell)
{
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= npts) return;
  const int nxd = N + 2;
  const int ic = index[3 * n], jc = index[3 * n + 1], l = index[3 * n + 2];
  const int base = l * nxd * nxd;
  const int e[4] = {base + jc * nxd + ic, base + (jc + 1) * nxd + ic, base + (jc + 1) * nxd + ic + 1, base + jc * nxd + ic + 1};
  for (int k = 0; k < 4; k++) { elem[4 * n + k] = e[k]; cell[4 * n + k] = cell_of[e[k]]; }
}

__device__ __forceinline__ int bl_max_weight_index(const double *w)
{
  int ind = 0;
  for (int i = 1; i < 4; i++) if (w[i] > w[ind]) ind = i;
  return ind;
}

// the interpolation of one point from its four corner values (:571-607)
__device__ __forceinline__ double bl_interp(const double *d, const double *w, int has_missing, double missing, int fill_missing)
{
  if (has_missing && (d[0] == missing || d[1] == missing || d[2] == missing || d[3] == missing))
    return fill_missing ? d[bl_max_weight_index(w)] : missing;
  return d[0] * w[0] + d[1] * w[1] + d[2] * w[2] + d[3] * w[3];
}

// scalar: src [nz][ncells] (no halo) -> out [nz][npts]; the corner indices and weights are read once for all levels
__global__ __launch_bounds__(256) void k_bl_gather_scalar(long npts, long ncells, int nz, const int *cell, const double *weight,
                                                          const double *src, int has_missing, double missing, int fill_missing,
                                                          double *out)
{
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= npts) return;
  const int4 c = *(const int4 *)(cell + 4 * n);
  const double w[4] = {weight[4 * n], weight[4 * n + 1], weight[4 * n + 2], weight[4 * n + 3]};
  const int cc[4] = {c.x, c.y, c.z, c.w};
  for (int k = 0; k < nz; k++) {
    const double *lev = src + (size_t)k * ncells;
    double d[4];
    for (int m = 0; m < 4; m++) d[m] = cc[m] >= 0 ? lev[cc[m]] : 0.0;
    out[(size_t)k * npts + n] = bl_interp(d, w, has_missing, missing, fill_missing);
  }
}

// vector (:476-560): at each corner e the three projections u*vlon_t[3e+a] + v*vlat_t[3e+a] of the halo'd cube, interpolated
// like scalars (missing tested on the projected values), then rotated onto the lat-lon point's vlon_t / vlat_t
__global__ __launch_bounds__(256) void k_bl_gather_vector(long npts, long ncells, int nz, const int *elem, const int *cell,
                                                          const double *weight, const double *vlon_in, const double *vlat_in,
                                                          const double *vlon_out, const double *vlat_out, const double *u,
                                                          const double *v, int has_missing, double missing, int fill_missing,
                                                          double *u_out, double *v_out)
{
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= npts) return;
  const int4 c = *(const int4 *)(cell + 4 * n);
  const int4 e = *(const int4 *)(elem + 4 * n);
  const int cc[4] = {c.x, c.y, c.z, c.w}, ee[4] = {e.x, e.y, e.z, e.w};
  const double w[4] = {weight[4 * n], weight[4 * n + 1], weight[4 * n + 2], weight[4 * n + 3]};
  double lo[4][3], la[4][3];
  for (int m = 0; m < 4; m++)
    for (int a = 0; a < 3; a++) { lo[m][a] = vlon_in[3L * ee[m] + a]; la[m][a] = vlat_in[3L * ee[m] + a]; }
  const double ol[3] = {vlon_out[3 * n], vlon_out[3 * n + 1], vlon_out[3 * n + 2]};
  const double oa[3] = {vlat_out[3 * n], vlat_out[3 * n + 1], vlat_out[3 * n + 2]};
  for (int k = 0; k < nz; k++) {
    const double *ul = u + (size_t)k * ncells, *vl = v + (size_t)k * ncells;
    double uu[4], vv[4], r[3];
    for (int m = 0; m < 4; m++) { uu[m] = cc[m] >= 0 ? ul[cc[m]] : 0.0; vv[m] = cc[m] >= 0 ? vl[cc[m]] : 0.0; }
    for (int a = 0; a < 3; a++) {
      double d[4];
      for (int m = 0; m < 4; m++) d[m] = uu[m] * lo[m][a] + vv[m] * la[m][a];
      r[a] = bl_interp(d, w, has_missing, missing, fill_missing);
    }
    u_out[(size_t)k * npts + n] = r[0] * ol[0] + r[1] * ol[1] + r[2] * ol[2];
    v_out[(size_t)k * npts + n] = r[0] * oa[0] + r[1] * oa[1] + r[2] * oa[2];
  }
}

// redu2x (:1065-1155), nz levels, each level as the reference's one-level call treats it.
// x-sweep: tmp [nz][nyf][nxc], rows 1..nyf-2 (the cosp scaling of the y-sweep folded in, with the has_missing quirk of :1121:
// `if (vartmp[n1] /= missvalue)` divides by the missing value and tests the quotient)
__global__ __launch_bounds__(256) void k_redu2x_x(const double *fin, int nxf, int nyf, int nxc, int nz, const double *cosp,
                                                  int has_missing, double missvalue, double *tmp)
{
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)(nyf - 2) * nxc;
  if (t >= per * nz) return;
  const int k = (int)(t / per);
  const long r = t - (long)k * per;
  const int j = 1 + (int)(r / nxc), i2 = (int)(r % nxc);
  const double *row = fin + (size_t)k * nxf * nyf + (size_t)j * nxf;
  const double a = (i2 == 0) ? row[nxf - 1] : row[2 * i2 - 1], b = row[2 * i2], c = row[2 * i2 + 1];
  double val;
  if (has_missing && (a == missvalue || b == missvalue || c == missvalue)) val = missvalue;
  else val = 0.25 * (a + 2. * b + c);
  if (has_missing) {
    val /= missvalue;
    if (val != 0.0) val *= cosp[j];
  } else val *= cosp[j];
  tmp[(size_t)k * nxc * nyf + (size_t)j * nxc + i2] = val;
}

// y-sweep and poles of coarse point (j2, i) of level k
__device__ __forceinline__ double bl_redu2x_y_val(const double *fin, const double *tmp, int nxf, int nyf, int nxc, int nyc,
                                                  const double *acosp, int has_missing, double missvalue, int k, int j2, int i)
{
  const double *f = fin + (size_t)k * nxf * nyf;
  const double *tp = tmp + (size_t)k * nxc * nyf + i;
  double val;
  if (j2 == 0) val = f[2 * i];
  else if (j2 == nyc - 1) val = f[(size_t)(nyf - 1) * nxf + 2 * i];
  else {
    const int j = 2 * j2;
    const double a = tp[(size_t)j * nxc], b = tp[(size_t)(j - 1) * nxc], c = tp[(size_t)(j + 1) * nxc];
    if (has_missing && (a == missvalue || b == missvalue || c == missvalue)) val = missvalue;
    else val = acosp[j] * (a + 0.5 * (b + c));
  }
  return val;
}

// y-sweep and poles: crs [nz][nyc][nxc]
__global__ __launch_bounds__(256) void k_redu2x_y(const double *fin, const double *tmp, int nxf, int nyf, int nxc, int nyc, int nz,
                                                  const double *acosp, int has_missing, double missvalue, double *crs)
{
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)nyc * nxc;
  if (t >= per * nz) return;
  const int k = (int)(t / per);
  const long r = t - (long)k * per;
  const int j2 = (int)(r / nxc), i = (int)(r % nxc);
  crs[(size_t)k * nxc * nyc + (size_t)j2 * nxc + i] = bl_redu2x_y_val(fin, tmp, nxf, nyf, nxc, nyc, acosp, has_missing, missvalue, k, j2, i);
}

// ----------------------------------------------------------------------------- the field loop (fg_bilin_sweep, bilinear.hip)
// The gathers above on one chunk of up to BL_CHUNK levels in the FILE type (fregrid.c:1013-1112 around do_scalar / do_vector_
// bilinear_interp): a corner value is widened where it is gathered -- get_input_data's conversion (fregrid_util.c:2097-2123) is a
// pure function of one value, so this gives the bits of widening the level first and no double copy of the source exists -- and
// the result leaves in the file type with write_field_data's conversion (:2376-2406).  A halo corner is init_halo's 0.0, neither
// scaled nor offset: the reference converts the unpadded nx * ny block only (:2117-2124).  The level loop is unrolled over the
// chunk with the raw corner loads of LB levels issued before the first use, so the independent gathers are in flight together;
// `k < nl` (the partial last chunk) is uniform over the wave.
template <typename T> __device__ __forceinline__ double bl_widen(T raw, const BlConv &c)
{
  double v = (double)raw;
  if (c.scale != 0 && v != c.missing) v *= c.scale;
  if (c.offset != 0 && v != c.missing) v += c.offset;
  return v;
}
// (a conversion of zeros with T = double changes nothing: what finer_step > 0 stores into the fine workspace)
template <typename T> __device__ __forceinline__ T bl_narrow(double v, const BlConv &c)
{
  if (c.offset != 0 && v != c.missing) v -= c.offset;
  if (c.scale != 0 && v != c.missing) v /= c.scale;
  return (T)v;
}

// scalar: src [nl][ncells] of Tin -> out [nl][npts] of Tout; the interpolation's missing value is the field's own (cin.missing)
template <typename Tin, typename Tout>
__global__ __launch_bounds__(256) void k_bl_stream_scalar(BlStream a, const Tin *src, BlConv cin, BlConv cout, Tout *out)
{
  constexpr int LB = BL_CHUNK;
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.npts) return;
  const int4 c = *(const int4 *)(a.cell + 4 * n);
  const double w[4] = {a.weight[4 * n], a.weight[4 * n + 1], a.weight[4 * n + 2], a.weight[4 * n + 3]};
  const int cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int k0 = 0; k0 < BL_CHUNK; k0 += LB) {
    Tin raw[LB][4];
#pragma unroll
    for (int k = 0; k < LB; k++)
#pragma unroll
      for (int m = 0; m < 4; m++) raw[k][m] = (k0 + k < a.nl && cc[m] >= 0) ? src[(size_t)(k0 + k) * a.ncells + cc[m]] : (Tin)0;
#pragma unroll
    for (int k = 0; k < LB; k++) {
      if (k0 + k >= a.nl) break;
      double d[4];
#pragma unroll
      for (int m = 0; m < 4; m++) d[m] = cc[m] >= 0 ? bl_widen(raw[k][m], cin) : 0.0;
      out[(size_t)(k0 + k) * a.npts + n] = bl_narrow<Tout>(bl_interp(d, w, a.has_missing, cin.missing, a.fill_missing), cout);
    }
  }
}

// vector: u and v carry their own conversions; the interpolation's missing value is u's (bilinear_interp.c:494-495)
template <typename Tin, typename Tout>
__global__ __launch_bounds__(256) void k_bl_stream_vector(BlStream a, const Tin *u, const Tin *v, BlConv cu, BlConv cv, BlConv cu_out,
                                                          BlConv cv_out, Tout *u_out, Tout *v_out)
{
  constexpr int LB = BL_CHUNK / 2;               // 2 * 4 * LB raw values beside the 36 doubles of unit vectors and weights
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.npts) return;
  const int4 c = *(const int4 *)(a.cell + 4 * n);
  const int4 e = *(const int4 *)(a.elem + 4 * n);
  const int cc[4] = {c.x, c.y, c.z, c.w}, ee[4] = {e.x, e.y, e.z, e.w};
  const double w[4] = {a.weight[4 * n], a.weight[4 * n + 1], a.weight[4 * n + 2], a.weight[4 * n + 3]};
  double lo[4][3], la[4][3];
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int x = 0; x < 3; x++) { lo[m][x] = a.vlon_in[3L * ee[m] + x]; la[m][x] = a.vlat_in[3L * ee[m] + x]; }
  const double ol[3] = {a.vlon_out[3 * n], a.vlon_out[3 * n + 1], a.vlon_out[3 * n + 2]};
  const double oa[3] = {a.vlat_out[3 * n], a.vlat_out[3 * n + 1], a.vlat_out[3 * n + 2]};
#pragma unroll
  for (int k0 = 0; k0 < BL_CHUNK; k0 += LB) {
    Tin ru[LB][4], rv[LB][4];
#pragma unroll
    for (int k = 0; k < LB; k++)
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const bool ld = k0 + k < a.nl && cc[m] >= 0;
        const size_t at = (size_t)(k0 + k) * a.ncells + (ld ? cc[m] : 0);
        ru[k][m] = ld ? u[at] : (Tin)0;
        rv[k][m] = ld ? v[at] : (Tin)0;
      }
#pragma unroll
    for (int k = 0; k < LB; k++) {
      if (k0 + k >= a.nl) break;
      double uu[4], vv[4], r[3];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        uu[m] = cc[m] >= 0 ? bl_widen(ru[k][m], cu) : 0.0;
        vv[m] = cc[m] >= 0 ? bl_widen(rv[k][m], cv) : 0.0;
      }
#pragma unroll
      for (int x = 0; x < 3; x++) {
        double d[4];
#pragma unroll
        for (int m = 0; m < 4; m++) d[m] = uu[m] * lo[m][x] + vv[m] * la[m][x];
        r[x] = bl_interp(d, w, a.has_missing, cu.missing, a.fill_missing);
      }
      u_out[(size_t)(k0 + k) * a.npts + n] = bl_narrow<Tout>(r[0] * ol[0] + r[1] * ol[1] + r[2] * ol[2], cu_out);
      v_out[(size_t)(k0 + k) * a.npts + n] = bl_narrow<Tout>(r[0] * oa[0] + r[1] * oa[1] + r[2] * oa[2], cv_out);
    }
  }
}

// the last y-sweep of finer_step > 0 with the narrowing folded in: crs [nz][nyc][nxc] of Tout
template <typename Tout>
__global__ __launch_bounds__(256) void k_redu2x_y_typed(const double *fin, const double *tmp, int nxf, int nyf, int nxc, int nyc, int nz,
                                                        const double *acosp, int has_missing, double missvalue, BlConv cout, Tout *crs)
{
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)nyc * nxc;
  if (t >= per * nz) return;
  const int k = (int)(t / per);
  const long r = t - (long)k * per;
  const int j2 = (int)(r / nxc), i = (int)(r % nxc);
  const double val = bl_redu2x_y_val(fin, tmp, nxf, nyf, nxc, nyc, acosp, has_missing, missvalue, k, j2, i);
  crs[(size_t)k * nxc * nyc + (size_t)j2 * nxc + i] = bl_narrow<Tout>(val, cout);
}

// ----------------------------------------------------------------------------- launchers (bilinear.hip)
static inline unsigned bl_nblk(long n, int b) { return (unsigned)((n + b - 1) / b); }

void fgd_bl_search_iter(const BlGeom &g, int iter, double dlon, double dlat, double lonbegin, double latbegin, unsigned *unfound,
                        BlWin *win, unsigned long long *cnt, unsigned long long *off, unsigned long long *bsum,
                        unsigned long long *total, int *found, unsigned long long *key, int *index, unsigned *ties,
                        int pair_blocks, hipStream_t st)
{
  const long ncell = 6L * g.N * g.N, npts = (long)g.nxo * g.nyo;
  const long nb = (ncell + BL_SCAN_B * BL_SCAN_E - 1) / (BL_SCAN_B * BL_SCAN_E);
  k_bl_window<<<bl_nblk(ncell, 256), 256, 0, st>>>(g, iter, dlon, dlat, lonbegin, latbegin, unfound, win, cnt);
  k_scan_local<<<(unsigned)nb, BL_SCAN_B, 0, st>>>(iter, unfound, cnt, ncell, off, bsum);
  k_scan_sums<<<1, BL_SCAN_B, 0, st>>>(iter, unfound, bsum, nb, total);
  k_scan_add<<<(unsigned)nb, BL_SCAN_B, 0, st>>>(iter, unfound, off, ncell, bsum);
  k_bl_pairs<<<pair_blocks, 256, 0, st>>>(g, iter, unfound, win, off, total, found, key, ties);
  k_bl_finalize<<<bl_nblk(npts, 256), 256, 0, st>>>(g.N, npts, iter, unfound, found, key, index);
}

long fgd_bl_scan_blocks(long ncell) { return (ncell + BL_SCAN_B * BL_SCAN_E - 1) / (BL_SCAN_B * BL_SCAN_E); }

void fgd_bl_weight_sides(const BlGeom &g, const int *index, double *angle, double *acos_arg, double *side_cos, hipStream_t st)
{
  const long npts = (long)g.nxo * g.nyo;
  k_bl_weight_sides<<<bl_nblk(npts, 256), 256, 0, st>>>(g, npts, index, angle, acos_arg, side_cos);
}

void fgd_bl_weight_final(long npts, int N, const int *index, const double *dist, double *weight, hipStream_t st)
{
  k_bl_weight_final<<<bl_nblk(npts, 256), 256, 0, st>>>(npts, N, index, dist, weight);
}

void fgd_bl_corners(const BlGeom &g, const int *index, const int *cell_of, int *elem, int *cell, hipStream_t st)
{
  const long npts = (long)g.nxo * g.nyo;
  k_bl_corners<<<bl_nblk(npts, 256), 256, 0, st>>>(g.N, npts, index, cell_of, elem, cell);
}

void fgd_bl_gather_scalar(long npts, long ncells, int nz, const int *cell, const double *weight, const double *src, int has_missing,
                          double missing, int fill_missing, double *out, hipStream_t st)
{
  k_bl_gather_scalar<<<bl_nblk(npts, 256), 256, 0, st>>>(npts, ncells, nz, cell, weight, src, has_missing, missing, fill_missing, out);
}

void fgd_bl_gather_vector(long npts, long ncells, int nz, const int *elem, const int *cell, const double *weight, const double *vlon_in,
                          const double *vlat_in, const double *vlon_out, const double *vlat_out, const double *u, const double *v,
                          int has_missing, double missing, int fill_missing, double *u_out, double *v_out, hipStream_t st)
{
  k_bl_gather_vector<<<bl_nblk(npts, 256), 256, 0, st>>>(npts, ncells, nz, elem, cell, weight, vlon_in, vlat_in, vlon_out, vlat_out,
                                                        u, v, has_missing, missing, fill_missing, u_out, v_out);
}

void fgd_bl_redu2x(const double *fin, int nxf, int nyf, int nz, const double *cosp, const double *acosp, int has_missing,
                   double missvalue, double *tmp, double *crs, hipStream_t st)
{
  const int nxc = nxf / 2, nyc = (nyf - 1) / 2 + 1;
  const long nx_work = (long)(nyf - 2) * nxc * nz, ny_work = (long)nyc * nxc * nz;
  if (nx_work > 0) k_redu2x_x<<<bl_nblk(nx_work, 256), 256, 0, st>>>(fin, nxf, nyf, nxc, nz, cosp, has_missing, missvalue, tmp);
  k_redu2x_y<<<bl_nblk(ny_work, 256), 256, 0, st>>>(fin, tmp, nxf, nyf, nxc, nyc, nz, acosp, has_missing, missvalue, crs);
}

// ---- the field loop's launchers: the kernel instance of a pair of file types (FG_NC_SHORT / _INT / _FLOAT / _DOUBLE)
template <typename F> static void bl_with_type(int nc_type, F f)
{
  switch (nc_type) {
    case FG_NC_SHORT: f((int16_t)0); break;
    case FG_NC_INT: f((int32_t)0); break;
    case FG_NC_FLOAT: f(0.0f); break;
    default: f(0.0); break;
  }
}

void fgd_bl_stream_scalar(int in_type, int out_type, const BlStream &a, const void *src, BlConv cin, BlConv cout, void *out,
                          hipStream_t st)
{
  bl_with_type(in_type, [&](auto ti) {
    bl_with_type(out_type, [&](auto to) {
      using Tin = decltype(ti); using Tout = decltype(to);
      k_bl_stream_scalar<Tin, Tout><<<bl_nblk(a.npts, 256), 256, 0, st>>>(a, (const Tin *)src, cin, cout, (Tout *)out);
    });
  });
}

void fgd_bl_stream_vector(int in_type, int out_type, const BlStream &a, const void *u, const void *v, BlConv cu, BlConv cv,
                          BlConv cu_out, BlConv cv_out, void *u_out, void *v_out, hipStream_t st)
{
  bl_with_type(in_type, [&](auto ti) {
    bl_with_type(out_type, [&](auto to) {
      using Tin = decltype(ti); using Tout = decltype(to);
      k_bl_stream_vector<Tin, Tout><<<bl_nblk(a.npts, 256), 256, 0, st>>>(a, (const Tin *)u, (const Tin *)v, cu, cv, cu_out, cv_out,
                                                                          (Tout *)u_out, (Tout *)v_out);
    });
  });
}

// fgd_bl_redu2x whose y-sweep narrows to out_type: the last coarsening step of a streamed chunk
void fgd_bl_redu2x_typed(int out_type, const double *fin, int nxf, int nyf, int nz, const double *cosp, const double *acosp,
                         int has_missing, double missvalue, double *tmp, BlConv cout, void *crs, hipStream_t st)
{
  const int nxc = nxf / 2, nyc = (nyf - 1) / 2 + 1;
  const long nx_work = (long)(nyf - 2) * nxc * nz, ny_work = (long)nyc * nxc * nz;
  if (nx_work > 0) k_redu2x_x<<<bl_nblk(nx_work, 256), 256, 0, st>>>(fin, nxf, nyf, nxc, nz, cosp, has_missing, missvalue, tmp);
  bl_with_type(out_type, [&](auto to) {
    using Tout = decltype(to);
    k_redu2x_y_typed<Tout><<<bl_nblk(ny_work, 256), 256, 0, st>>>(fin, tmp, nxf, nyf, nxc, nyc, nz, acosp, has_missing, missvalue, cout,
                                                                  (Tout *)crs);
  });
}
