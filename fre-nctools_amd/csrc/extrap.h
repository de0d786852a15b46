// extrap.h -- what extrap.hip (host orchestration) and extrap_kernels.hip (kernels) share: the grid factors of do_extrapolate
// (tools/fregrid/fregrid_util.c:2676-2720), the cell formula that turns them into the four coefficients, and the launchers.
#pragma once
#include <hip/hip_runtime.h>

#define EX_MAX_ITER 4000                 // MAX_ITER (fregrid_util.c:39)
#define EX_REL_COEF 0.9                  // REL_COEF (:38)
#define EX_EPSLN10  1.e-10               // EPSLN10  (:37)

// The coefficients depend on the row through three numbers and on the column through two:
//   rn[j] = csj*cstr/(dyt[j]*dyu[j])   rs[j] = csm*cstr/(dyt[j]*dyu[max(j-1,0)])   rc[j] = cstr*cstr          (:2710-2713)
//   ce[i] = dxu[i]*dxt[i]              cw[i] = dxu[max(i-1,0)]*dxt[i]
struct ExFactors {
  const double *rn, *rs, *rc;           // [nj]
  const double *ce, *cw;                // [ni]
};

// One cell's cfw, cfe, cfs, cfn with the reference's operations in the reference's order (:2710-2718).  Division, addition and
// multiplication are IEEE on the host and on the device (the library is built without contraction and without fast-math), so
// the host table and the device's own evaluation agree bit for bit.
__host__ __device__ __forceinline__ void ex_cell_coef(double rn, double rs, double rc, double ce, double cw,
                                                      double &cfw, double &cfe, double &cfs, double &cfn)
{
  const double n0 = rn, s0 = rs, e0 = rc / ce, w0 = rc / cw;
  const double cfc = 1.0 / (n0 + s0 + e0 + w0);
  cfn = n0 * cfc;
  cfs = s0 * cfc;
  cfe = e0 * cfc;
  cfw = w0 * cfc;
}

struct ExGrid {
  int ni, nj, is_cyclic;
  ExFactors f;
  const double *coef;                   // stored coefficients [nj*ni][4] = cfw, cfe, cfs, cfn, or NULL: evaluate ex_cell_coef per use
};

// level preparation (:2728-2745): dst = valid ? in : (prev ? prev : 0); sor bit = missing.  prev may equal dst.
void fgd_ex_prepare(const ExGrid &g, const double *in, double missing, const double *prev, double *dst,
                    unsigned long long *sorbits, hipStream_t st);
// one Jacobi iteration (:2752-2767): src -> dst, slot = max |res| as the bit pattern of a non-negative double.  prev_slot (NULL for
// the first iteration of a level): the launch leaves at once when that maximum is already <= stop_crit.
void fgd_ex_iterate(const ExGrid &g, const double *src, double *dst, const unsigned long long *sorbits, double stop_crit,
                    const unsigned long long *prev_slot, unsigned long long *slot, hipStream_t st);
// vertical interpolation: out[k][l] = interp[k] ? (1.-w[k])*in[a[k]][l] + w[k]*in[b[k]][l] : in[a[k]][l]
struct ExVLevel { int a, b, interp; double w; };
void fgd_ex_vertical(long nxy, int nk2, const ExVLevel *lev, const double *in, double *out, hipStream_t st);
// the same for nrec records in [nrec][nk1][nxy] with write_field_data's conversion to nc_type fused: out [nrec][nk2][nxy] of that type
void fgd_ex_vertical_narrow(int nc_type, long nxy, int nrec, int nk1, int nk2, const ExVLevel *lev, const double *in, double scale,
                            double offset, double missing, void *out, hipStream_t st);

// Several records per launch (fg_extrap_run_batch_dev).  State buf0 / buf1 [nrec][ncell], sorbits [nrec][(ncell+63)/64], slots
// [iteration][nrec]; parity[r] names the buffer that holds record r's state (NULL in prepare: the first level, nothing to carry).
// prepare: `in` is this level of record 0, record r lies r*rec_stride doubles on; it always writes buf0.  iterate: src -> dst for
// every record whose prev_slots[r] (NULL for iteration 0) is still > stop_crit.  copy_out: `out` as `in`.
void fgd_ex_prepare_batch(const ExGrid &g, int nrec, const double *in, long rec_stride, double missing, const double *buf0,
                          const double *buf1, const int *parity, double *dst, unsigned long long *sorbits, hipStream_t st);
void fgd_ex_iterate_batch(const ExGrid &g, int nrec, const double *src, double *dst, const unsigned long long *sorbits, double stop_crit,
                          const unsigned long long *prev_slots, unsigned long long *slots, hipStream_t st);
void fgd_ex_copy_out_batch(const ExGrid &g, int nrec, const double *buf0, const double *buf1, const int *parity, double *out,
                           long rec_stride, hipStream_t st);

// host side, for the column pipeline (column.hip).  ex_vertical_levels: the bracket table of do_vertical_interp for nk2 destination
// levels after linear_vertical_interp's fatal checks (FG_ERR_DATA with its message); *need = 0: the field is left alone (lev untouched).
#include <vector>
int ex_vertical_levels(int nk1, const double *z1, int nk2, const double *z2, std::vector<ExVLevel> &lev, int *need);
struct fg_extrap;
int fg_extrap_borrow_stream(fg_extrap *h, void *stream, void **saved, int *saved_own);   // as fg_plan_borrow_stream
void fg_extrap_return_stream(fg_extrap *h, void *saved, int saved_own);
void fg_extrap_dims(const fg_extrap *h, int *ni, int *nj, int *device);
