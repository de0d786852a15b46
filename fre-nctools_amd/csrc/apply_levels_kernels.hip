// apply_levels_kernels.hip -- the sweep of up to eight levels that each carry their own missing values (fg_plan_apply_levels,
// fg_plan_apply_records_levels, fg_sweep_run_levels).
//
// The reference takes such a field one level per call (fregrid.c:1045-1083; conserve_interp.c:544 forbids has_missing with
// nz > 1): level k of the output is do_scalar_conserve_interp(nz = 1, has_missing = 1) on level k alone -- per destination
// cell the exchange cells whose source value differs from `missing` IN THAT LEVEL are summed in CSR order, the result is
// acc / asum where asum > 0, 0.0 where an exchange cell counted but asum == 0, else `missing` (:562-591, :744-783, :815-839).
// k_apply_ep8m does that for eight interleaved levels in one launch: every CSR record is read once, every gather is a full
// 64-byte sector, and only the validity -- area sum and "touched" flag -- differs from level to level.
//
//   k_apply_ep8m   entry-parallel like k_apply_ep8g (apply_kernels.hip): a tile of ROWS destination rows walks its run of CSR
//                  records in chunks of CAP; a chunk is staged in LDS, a lane pair per exchange cell issues the chunk's gathers
//                  in one round, the products go to LDS with ONE area and an 8-bit validity mask per exchange cell, and the
//                  lane of each (row, level) adds its part in CSR order, carrying sum, area sum and touched flag from chunk
//                  to chunk.  An invalid (exchange cell, level) holds the product +0.0: x + 0.0 == x bit for bit here (no sum
//                  is ever -0.0: they start at +0.0), which is the `continue` of the reference, as in k_apply_ep1.
//   k_gmask_bits   grad_mask int [nb][ncells] (fg_c2l_gradient) -> one byte per source cell, bit k = level k
#include "xgrid_device.h"
#include <type_traits>

namespace {
struct __attribute__((aligned(16))) Vec4 { double v[4]; };
inline int nblk(long n, int t) { return (int)((n + t - 1) / t); }
}

// rec: ORDER 2 the merged records [source cell][3][8] = {f, gx, gy} x levels (k_merge3 / k_c2l_records_m), indexed by idx_g;
//      ORDER 1 the interleaved field [F][8], indexed by idx_f.
// gbits (ORDER 2): per source cell, bit k set = level k takes the flat value (fregrid_util.c:2203-2215).
// out, row_sum: level-major [level][ld], levels < nb_valid only.
template <int ORDER, int TPB, int CAP, int ROWS>
__global__ __launch_bounds__(TPB) void k_apply_ep8m(int ndst, FgCsr csr, const double *rec, const unsigned char *gbits, double missing,
                                                    double *out, double *row_sum, long ld, int nb_valid)
{
  constexpr int NB = 8;
  constexpr int EPP = TPB / 2, PASS = CAP / EPP;          // gather phase: a lane pair per exchange cell, EPP cells per pass
  static_assert(ROWS * NB <= TPB && CAP % EPP == 0, "a lane per (row, level)");
  // one buffer: the staged CSR records first, then (once every lane holds its records in registers) the products and areas
  __shared__ __attribute__((aligned(16))) double sh_raw[CAP * (NB + 1)];
  __shared__ unsigned char sh_vm[CAP * 2];                 // validity of levels 0-3 and 4-7 of every staged exchange cell
  typedef typename std::conditional<ORDER == 2, FgCsrEntry2, FgCsrEntry1>::type Entry;
  constexpr int W = sizeof(Entry) / 16;
  Entry *sh_e = reinterpret_cast<Entry *>(sh_raw);
  double *sh_p = sh_raw, *sh_a = sh_raw + CAP * NB;
  const int t = threadIdx.x;
  const int d0 = blockIdx.x * ROWS;
  const int dl = min(d0 + ROWS, ndst);
  const int q0 = csr.row_ptr[d0], q1 = csr.row_ptr[dl];
  const bool sumlane = t < ROWS * NB;                      // lane (row, level) of the sum phase
  const int d = d0 + t / NB, lev = t % NB;
  const int dc = min(d, ndst - 1);
  int b = 0, e = 0;
  if (sumlane) { b = csr.row_ptr[dc]; e = csr.row_ptr[dc + 1]; }
  const int vsel = lev >> 2, vbit = lev & 3;
  double acc = 0.0, asum = 0.0;
  unsigned touched = 0;
  for (int c0 = q0; c0 < q1; c0 += CAP) {                  // (block-uniform)
    const int n = min(CAP, q1 - c0);
    if (c0 > q0) __syncthreads();                          // the previous chunk's products have been added
    {
      typedef unsigned int u4v __attribute__((ext_vector_type(4)));
      const Entry *src = (ORDER == 2) ? (const Entry *)csr.e2 : (const Entry *)csr.e1;
      const u4v *g = reinterpret_cast<const u4v *>(src + c0);
      u4v *l = reinterpret_cast<u4v *>(sh_e);
      for (int i = t; i < n * W; i += TPB) l[i] = __builtin_nontemporal_load(g + i);
    }
    __syncthreads();
    const int h = (t & 1) * 4;                             // four levels per lane of the pair
    Vec4 fv[PASS], gxv[PASS], gyv[PASS];
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
          fv[j] = *reinterpret_cast<const Vec4 *>(pf);
          gxv[j] = *reinterpret_cast<const Vec4 *>(pf + NB);
          gyv[j] = *reinterpret_cast<const Vec4 *>(pf + 2 * NB);
          gb[j] = gbits[E[j].idx_g];
        } else
          fv[j] = *reinterpret_cast<const Vec4 *>(rec + (size_t)E[j].idx_f * NB + h);
      }
    }
    __syncthreads();                                       // the records are in registers: the buffer becomes the product table
#pragma unroll
    for (int j = 0; j < PASS; j++) {
      const int i = t / 2 + EPP * j;
      if (EPP * j < n && i < n) {
        Vec4 pv;
        unsigned vm = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          double v = fv[j].v[k];
          const bool ok = !(v == missing);                 // `if (data == missing) continue`
          if constexpr (ORDER == 2) { if (!((gb[j] >> (h + k)) & 1u)) v = (v + gxv[j].v[k] * E[j].di + gyv[j].v[k] * E[j].dj); }
          pv.v[k] = ok ? v * E[j].area : 0.0;
          vm |= (ok ? 1u : 0u) << k;
        }
        *reinterpret_cast<Vec4 *>(sh_p + i * NB + h) = pv;
        sh_vm[i * 2 + (t & 1)] = (unsigned char)vm;
        if (h == 0) sh_a[i] = E[j].area;
      }
    }
    __syncthreads();
    if (sumlane) {
      const int qa = max(b, c0) - c0, qb = min(e, c0 + n) - c0;
      int q = qa;
      for (; q + 8 <= qb; q += 8) {                        // (long rows: eight LDS reads in flight, then the adds in CSR order)
        double pp[8], aa[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const unsigned ok = (sh_vm[(q + k) * 2 + vsel] >> vbit) & 1u;
          pp[k] = sh_p[(q + k) * NB + lev]; aa[k] = ok ? sh_a[q + k] : 0.0; touched |= ok;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) { acc += pp[k]; asum += aa[k]; }
      }
      for (; q < qb; q++) {
        const unsigned ok = (sh_vm[q * 2 + vsel] >> vbit) & 1u;
        acc += sh_p[q * NB + lev]; asum += ok ? sh_a[q] : 0.0; touched |= ok;
      }
    }
  }
  if (!sumlane || d >= ndst || lev >= nb_valid) return;
  if (row_sum) row_sum[(size_t)lev * ld + d] = (asum > 0) ? acc : 0.0;      // conserve_interp.c:815-819
  double r;                                                                 // :831-839
  if (asum > 0) r = acc / asum;
  else if (touched) r = 0.0;
  else r = missing;
  out[(size_t)lev * ld + d] = r;
}

__global__ __launch_bounds__(256) void k_gmask_bits(long n, const int *gmask, long ld, int nb, unsigned char *bits)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  unsigned m = 0;
  for (int k = 0; k < nb; k++) m |= (gmask[(size_t)k * ld + c] != 0 ? 1u : 0u) << k;
  bits[c] = (unsigned char)m;
}

// rows per tile by the mean row length, as fgd_apply_il_merged picks them: EP_ROWS-sized tiles for rows of a few exchange cells
// (a tile's cells mostly fit one chunk), fewer rows the longer they are; a single row of any length walks its chunks alone
void fgd_apply_levels8(int order, int ndst, long nx, FgCsr csr, const double *rec, const unsigned char *gbits, double missing, double *out,
                       double *row_sum, long ld, int nb_valid, hipStream_t st)
{
  if (ndst <= 0) return;
  const long m = nx / ndst;
#define EP8M(O_, R_) k_apply_ep8m<O_, 256, FG_LEVELS_CAP, R_><<<nblk(ndst, R_), 256, 0, st>>>(ndst, csr, rec, gbits, missing, out, row_sum, ld, nb_valid)
#define EP8MR(O_) do { if (m <= 6) EP8M(O_, 32); else if (m <= 24) EP8M(O_, 8); else if (m <= 96) EP8M(O_, 2); else EP8M(O_, 1); } while (0)
  if (order == 2) EP8MR(2); else EP8MR(1);
#undef EP8MR
#undef EP8M
}

void fgd_gmask_bits(long n, const int *gmask, long ld, int nb, unsigned char *bits, hipStream_t st)
{
  if (n > 0) k_gmask_bits<<<nblk(n, 256), 256, 0, st>>>(n, gmask, ld, nb, bits);
}
