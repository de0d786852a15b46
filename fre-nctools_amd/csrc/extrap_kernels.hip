// extrap_kernels.hip -- device kernels of fregrid's --extrapolate fill (do_extrapolate, tools/fregrid/fregrid_util.c:2662-2812) and
// of the --dst_vgrid level interpolation (linear_vertical_interp, tools/libfrencutils/interp.c:360-396).
//
// The fill is a relaxed Jacobi iteration: every residual of an iteration is formed from the old array (:2752-2760) before any
// point is updated (:2761-2767), so one launch per iteration over ping-pong arrays performs exactly the reference's operations on
// the reference's operands.  The padded array of the reference is not materialised: a neighbour beyond the north / south edge
// reads 0, one beyond the east / west edge reads the wrapped current value (cyclic: fill_boundaries runs after every update,
// :2780, :2802-2812) or 0.  The library is built with -ffp-contract=off: `cfw*W + cfe*E + cfs*S + cfn*N - C` stays four
// multiplications, three additions and a subtraction in that order.
//
// Stop without the host: every block reduces max |res| and adds it with one 64-bit atomicMax to the slot of its iteration (the
// bit patterns of non-negative doubles order like the numbers).  Launch n looks at slot n-1 first and leaves when that maximum
// is already <= stop_crit, so the launches queued behind the stopping iteration change nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "extrap.h"
#include "fregrid_hip.h"

// Iteration kernel geometry, measured on the MI355X at 1440 x 720: the launch time follows the number of
// blocks, each of which ends in one atomic on the same address -- 256-thread blocks of 1 / 4 cells per thread 30.5 / 16.6 us,
// 1024-thread blocks of 1 / 2 / 4 cells 15.2 / 12.8 / 13.0 us.  Small grids want every CU busy instead: one cell per thread.
#define EX_BLOCK 1024
#define EX_SMALL_GRID (512L * EX_BLOCK)   // up to this many cells one cell per thread, beyond it two
#define EX_PREP_BLOCK 256

__global__ __launch_bounds__(EX_PREP_BLOCK) void ex_prepare_kernel(long ncell, const double *in, double missing, const double *prev,
                                                              double *dst, unsigned long long *sorbits)
{
  const long n = (long)blockIdx.x * EX_PREP_BLOCK + threadIdx.x;
  bool miss = false;
  if (n < ncell) {
    const double v = in[n];
    miss = fabs(v - missing) <= EX_EPSLN10;                       // :2731, :2739
    dst[n] = miss ? (prev ? prev[n] : 0.0) : v;                    // the first level starts from initial_guess = 0 (:2726-2732)
  }
  const unsigned long long word = __ballot(miss);
  if ((threadIdx.x & 63) == 0 && n < ncell) sorbits[n >> 6] = word;
}

// One iteration of one record: the body of the single-record kernel and of the batched one (there the record is blockIdx.y and
// the five pointers are that record's).
template <bool STORED, int EX_CELLS_PER_THREAD>
__device__ __forceinline__ void ex_iterate_body(const ExGrid &g, const double *__restrict__ src, double *__restrict__ dst,
                                                const unsigned long long *__restrict__ sorbits, double stop_crit,
                                                const unsigned long long *prev_slot, unsigned long long *slot)
{
  if (prev_slot && __longlong_as_double((long long)*prev_slot) <= stop_crit) return;   // the level has stopped (:2769)
  const unsigned ncell = (unsigned)g.ni * (unsigned)g.nj;          // < 2^29 (fg_extrap_create): 32-bit index arithmetic
  const unsigned ni = (unsigned)g.ni;
  __shared__ unsigned long long wave_max[EX_BLOCK / 64];
  double v = 0.0;
  unsigned long long any = 0;                                      // wave-uniform: a wave covers one 64-cell word per step
  // Every load is unconditional (an edge cell reads a valid address and the value is replaced afterwards): a branch around a
  // load would make the wave wait for memory once per neighbour instead of once per cell.
#pragma unroll
  for (int q = 0; q < EX_CELLS_PER_THREAD; q++) {
    const unsigned n0 = (blockIdx.x * EX_CELLS_PER_THREAD + q) * EX_BLOCK + threadIdx.x;
    const bool live = n0 < ncell;
    const unsigned n = live ? n0 : ncell - 1;
    const unsigned long long word = sorbits[n >> 6];
    any |= live ? word : 0ull;
    const unsigned j = n / ni, i = n - j * ni;
    const bool west = i > 0, east = i < ni - 1, south = j > 0, north = j < (unsigned)g.nj - 1;
    const double c = src[n];
    double w = src[west ? n - 1 : n + ni - 1];
    double e = src[east ? n + 1 : n + 1 - ni];
    double s = src[south ? n - ni : n];
    double nn = src[north ? n + ni : n];
    w = (west || g.is_cyclic) ? w : 0.0;
    e = (east || g.is_cyclic) ? e : 0.0;
    s = south ? s : 0.0;
    nn = north ? nn : 0.0;
    double cfw, cfe, cfs, cfn;
    if (STORED) {
      const double2 a = ((const double2 *)g.coef)[2 * n], b = ((const double2 *)g.coef)[2 * n + 1];
      cfw = a.x; cfe = a.y; cfs = b.x; cfn = b.y;
    } else
      ex_cell_coef(g.f.rn[j], g.f.rs[j], g.f.rc[j], g.f.ce[i], g.f.cw[i], cfw, cfe, cfs, cfn);
    double res = cfw * w + cfe * e + cfs * s + cfn * nn - c;       // :2759
    res *= ((word >> (n & 63)) & 1ull) ? EX_REL_COEF : 0.0;        // :2764 -- valid points too: 0 * res keeps the reference's -0 / NaN
    if (live) dst[n] = c + res;                                    // :2765
    const double a = live ? fabs(res) : 0.0;
    v = a > v ? a : v;                                             // max(fabs(res), resmax) is (a>b ? a:b): a NaN never raises it (:2766)
  }
  // block maximum as a bit pattern (v >= +0, never NaN); a wave without missing points has every |res| = 0 and skips the shuffles
  unsigned long long m = (unsigned long long)__double_as_longlong(v);
  if (__ballot(any != 0) != 0) {
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(m, off);
      m = o > m ? o : m;
    }
  }
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < EX_BLOCK / 64; w++) m = wave_max[w] > m ? wave_max[w] : m;
    if (m) atomicMax(slot, m);                                     // slots start at 0: a zero maximum needs no atomic
  }
}

template <bool STORED, int EX_CELLS_PER_THREAD>
__global__ __launch_bounds__(EX_BLOCK) void ex_iterate_kernel(ExGrid g, const double *__restrict__ src, double *__restrict__ dst,
                                                              const unsigned long long *__restrict__ sorbits, double stop_crit,
                                                              const unsigned long long *prev_slot, unsigned long long *slot)
{
  ex_iterate_body<STORED, EX_CELLS_PER_THREAD>(g, src, dst, sorbits, stop_crit, prev_slot, slot);
}

// ---- several records per launch (fg_extrap_run_batch_dev): the record is blockIdx.y.  State [nrec][ncell] in two buffers, mask
// bits [nrec][nwords] (a record's bits start on a word of its own), slots [iteration][nrec].  Every record is the single-record
// problem on its own pointers: a record that has stopped leaves at the guard, whatever the others do.
__global__ __launch_bounds__(EX_PREP_BLOCK) void ex_prepare_batch_kernel(long ncell, long nwords, const double *in, long rec_stride,
                                                                    double missing, const double *buf0, const double *buf1,
                                                                    const int *parity, double *dst, unsigned long long *sorbits)
{
  const long r = blockIdx.y, n = (long)blockIdx.x * EX_PREP_BLOCK + threadIdx.x;
  const double *prev = parity ? (parity[r] ? buf1 : buf0) + r * ncell : nullptr;   // parity == NULL: the first level
  bool miss = false;
  if (n < ncell) {
    const double v = in[r * rec_stride + n];
    miss = fabs(v - missing) <= EX_EPSLN10;
    dst[r * ncell + n] = miss ? (prev ? prev[n] : 0.0) : v;
  }
  const unsigned long long word = __ballot(miss);
  if ((threadIdx.x & 63) == 0 && n < ncell) sorbits[r * nwords + (n >> 6)] = word;
}

template <bool STORED, int EX_CELLS_PER_THREAD>
__global__ __launch_bounds__(EX_BLOCK) void ex_iterate_batch_kernel(ExGrid g, long nwords, const double *__restrict__ src,
                                                                    double *__restrict__ dst,
                                                                    const unsigned long long *__restrict__ sorbits, double stop_crit,
                                                                    const unsigned long long *prev_slots, unsigned long long *slots)
{
  const long r = blockIdx.y, ncell = (long)g.ni * g.nj;
  ex_iterate_body<STORED, EX_CELLS_PER_THREAD>(g, src + r * ncell, dst + r * ncell, sorbits + r * nwords, stop_crit,
                                               prev_slots ? prev_slots + r : nullptr, slots + r);
}

// the level's answer of every record, from the buffer its own last iteration wrote
__global__ __launch_bounds__(EX_PREP_BLOCK) void ex_copy_out_batch_kernel(long ncell, const double *buf0, const double *buf1,
                                                                     const int *parity, double *out, long rec_stride)
{
  const long r = blockIdx.y, n = (long)blockIdx.x * EX_PREP_BLOCK + threadIdx.x;
  if (n < ncell) out[r * rec_stride + n] = (parity[r] ? buf1 : buf0)[r * ncell + n];
}

__global__ __launch_bounds__(EX_PREP_BLOCK) void ex_vertical_kernel(long nxy, const ExVLevel *lev, const double *__restrict__ in,
                                                               double *__restrict__ out)
{
  const long l = (long)blockIdx.x * EX_PREP_BLOCK + threadIdx.x;
  if (l >= nxy) return;
  const ExVLevel L = lev[blockIdx.y];
  const double a = in[(long)L.a * nxy + l];
  double r = a;
  if (L.interp) r = (1. - L.w) * a + L.w * in[(long)L.b * nxy + l];   // interp.c:381, :390
  out[(long)blockIdx.y * nxy + l] = r;
}

// do_vertical_interp and write_field_data's conversion in one pass (the column pipeline): per record the one or two source
// planes a destination level needs, (1.-w)*a + w*b in double, then `-= offset`, `/= scale` where != missing and the C cast to the
// file type (sweep.hip's k_narrow) -- the double never goes to memory.  grid (cells, nk2, records).
template <typename T>
__global__ __launch_bounds__(EX_PREP_BLOCK) void ex_vertical_narrow_kernel(long nxy, int nk1, int nk2, const ExVLevel *lev,
                                                                      const double *__restrict__ in, double scale, double offset,
                                                                      double missing, T *__restrict__ out)
{
  const long l = (long)blockIdx.x * EX_PREP_BLOCK + threadIdx.x;
  if (l >= nxy) return;
  const ExVLevel L = lev[blockIdx.y];
  const double *p = in + (long)blockIdx.z * nk1 * nxy;
  double v = p[(long)L.a * nxy + l];
  if (L.interp) v = (1. - L.w) * v + L.w * p[(long)L.b * nxy + l];
  if (offset != 0 && v != missing) v -= offset;
  if (scale != 0 && v != missing) v /= scale;
  out[((long)blockIdx.z * nk2 + blockIdx.y) * nxy + l] = (T)v;
}

void fgd_ex_prepare(const ExGrid &g, const double *in, double missing, const double *prev, double *dst,
                    unsigned long long *sorbits, hipStream_t st)
{
  const long ncell = (long)g.ni * g.nj;
  ex_prepare_kernel<<<dim3((unsigned)((ncell + EX_PREP_BLOCK - 1) / EX_PREP_BLOCK)), dim3(EX_PREP_BLOCK), 0, st>>>(ncell, in, missing, prev, dst, sorbits);
}

void fgd_ex_iterate(const ExGrid &g, const double *src, double *dst, const unsigned long long *sorbits, double stop_crit,
                    const unsigned long long *prev_slot, unsigned long long *slot, hipStream_t st)
{
  const long ncell = (long)g.ni * g.nj;
  const int cpt = ncell <= EX_SMALL_GRID ? 1 : 2;
  const long per_block = (long)EX_BLOCK * cpt;
  const dim3 grid((unsigned)((ncell + per_block - 1) / per_block)), block(EX_BLOCK);
  if (g.coef) {
    if (cpt == 1) ex_iterate_kernel<true, 1><<<grid, block, 0, st>>>(g, src, dst, sorbits, stop_crit, prev_slot, slot);
    else ex_iterate_kernel<true, 2><<<grid, block, 0, st>>>(g, src, dst, sorbits, stop_crit, prev_slot, slot);
  } else {
    if (cpt == 1) ex_iterate_kernel<false, 1><<<grid, block, 0, st>>>(g, src, dst, sorbits, stop_crit, prev_slot, slot);
    else ex_iterate_kernel<false, 2><<<grid, block, 0, st>>>(g, src, dst, sorbits, stop_crit, prev_slot, slot);
  }
}

void fgd_ex_vertical(long nxy, int nk2, const ExVLevel *lev, const double *in, double *out, hipStream_t st)
{
  ex_vertical_kernel<<<dim3((unsigned)((nxy + EX_PREP_BLOCK - 1) / EX_PREP_BLOCK), (unsigned)nk2), dim3(EX_PREP_BLOCK), 0, st>>>(nxy, lev, in, out);
}

void fgd_ex_vertical_narrow(int nc_type, long nxy, int nrec, int nk1, int nk2, const ExVLevel *lev, const double *in, double scale,
                            double offset, double missing, void *out, hipStream_t st)
{
  const dim3 grid((unsigned)((nxy + EX_PREP_BLOCK - 1) / EX_PREP_BLOCK), (unsigned)nk2, (unsigned)nrec), block(EX_PREP_BLOCK);
  switch (nc_type) {
    case FG_NC_SHORT: ex_vertical_narrow_kernel<int16_t><<<grid, block, 0, st>>>(nxy, nk1, nk2, lev, in, scale, offset, missing, (int16_t *)out); break;
    case FG_NC_INT: ex_vertical_narrow_kernel<int32_t><<<grid, block, 0, st>>>(nxy, nk1, nk2, lev, in, scale, offset, missing, (int32_t *)out); break;
    case FG_NC_FLOAT: ex_vertical_narrow_kernel<float><<<grid, block, 0, st>>>(nxy, nk1, nk2, lev, in, scale, offset, missing, (float *)out); break;
    default: ex_vertical_narrow_kernel<double><<<grid, block, 0, st>>>(nxy, nk1, nk2, lev, in, scale, offset, missing, (double *)out); break;
  }
}

void fgd_ex_prepare_batch(const ExGrid &g, int nrec, const double *in, long rec_stride, double missing, const double *buf0,
                          const double *buf1, const int *parity, double *dst, unsigned long long *sorbits, hipStream_t st)
{
  const long ncell = (long)g.ni * g.nj;
  const dim3 grid((unsigned)((ncell + EX_PREP_BLOCK - 1) / EX_PREP_BLOCK), (unsigned)nrec);
  ex_prepare_batch_kernel<<<grid, dim3(EX_PREP_BLOCK), 0, st>>>(ncell, (ncell + 63) / 64, in, rec_stride, missing, buf0, buf1, parity, dst, sorbits);
}

void fgd_ex_iterate_batch(const ExGrid &g, int nrec, const double *src, double *dst, const unsigned long long *sorbits, double stop_crit,
                          const unsigned long long *prev_slots, unsigned long long *slots, hipStream_t st)
{
  const long ncell = (long)g.ni * g.nj, nwords = (ncell + 63) / 64;
  const int cpt = ncell <= EX_SMALL_GRID ? 1 : 2;
  const long per_block = (long)EX_BLOCK * cpt;
  const dim3 grid((unsigned)((ncell + per_block - 1) / per_block), (unsigned)nrec), block(EX_BLOCK);
  if (g.coef) {
    if (cpt == 1) ex_iterate_batch_kernel<true, 1><<<grid, block, 0, st>>>(g, nwords, src, dst, sorbits, stop_crit, prev_slots, slots);
    else ex_iterate_batch_kernel<true, 2><<<grid, block, 0, st>>>(g, nwords, src, dst, sorbits, stop_crit, prev_slots, slots);
  } else {
    if (cpt == 1) ex_iterate_batch_kernel<false, 1><<<grid, block, 0, st>>>(g, nwords, src, dst, sorbits, stop_crit, prev_slots, slots);
    else ex_iterate_batch_kernel<false, 2><<<grid, block, 0, st>>>(g, nwords, src, dst, sorbits, stop_crit, prev_slots, slots);
  }
}

void fgd_ex_copy_out_batch(const ExGrid &g, int nrec, const double *buf0, const double *buf1, const int *parity, double *out,
                           long rec_stride, hipStream_t st)
{
  const long ncell = (long)g.ni * g.nj;
  const dim3 grid((unsigned)((ncell + EX_PREP_BLOCK - 1) / EX_PREP_BLOCK), (unsigned)nrec);
  ex_copy_out_batch_kernel<<<grid, dim3(EX_PREP_BLOCK), 0, st>>>(ncell, buf0, buf1, parity, out, rec_stride);
}
