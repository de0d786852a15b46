// extrap.hip -- host orchestration of fregrid's --extrapolate fill (fg_extrap_*: do_extrapolate, tools/fregrid/fregrid_util.c:2662-2812)
// and of the --dst_vgrid levels (fg_setup_vertical_interp / fg_dev_vertical_interp: setup_vertical_interp / do_vertical_interp,
// :756-819, linear_vertical_interp, tools/libfrencutils/interp.c:360-396).  Kernels: extrap_kernels.hip.
//
// The grid factors are O(ni + nj) host work, once per source grid.  Their cosines are csrc/sincos_glibc.h's fgs_cos -- the
// operation sequence the reference's cos() call resolves to on its build host -- so they do not depend on this host's libm.
//
// A level is iterated without the host in the loop: `batch` launches are queued, each guarded by the maximum of the one before
// it (see extrap_kernels.hip), then the batch's slots are read back once.  The first slot <= stop_crit is the reference's
// stopping iteration; the launches behind it were no-ops, so the buffer iteration n wrote holds the answer.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <vector>
#include "extrap.h"
#include "fg_host.h"
#include "sincos_glibc.h"

#define EX_DEFAULT_BATCH 64
static std::atomic<int> g_batch{EX_DEFAULT_BATCH};
static std::atomic<int> g_coef_mode{0};          // 0: evaluate the coefficients per use from the row / column factors, 1: stored

extern "C" void fg_set_extrap_batch(int n) { g_batch = (n < 1) ? EX_DEFAULT_BATCH : (n > EX_MAX_ITER ? EX_MAX_ITER : n); }
extern "C" void fg_set_extrap_coef(int stored) { g_coef_mode = stored ? 1 : 0; }

// :2676-2713 up to the per-cell part: rn, rs, rc [nj], ce, cw [ni]
static void ex_factors(int ni, int nj, const double *lon, const double *lat, double *rn, double *rs, double *rc, double *ce, double *cw)
{
  std::vector<double> dyu(nj), dyt(nj), dxu(ni), dxt(ni);
  for (int j = 0; j < nj - 1; j++) dyu[j] = lat[j + 1] - lat[j];
  dyu[nj - 1] = dyu[nj - 2];
  for (int j = 1; j < nj; j++) dyt[j] = 0.5 * (dyu[j] + dyu[j - 1]);
  dyt[0] = dyt[1];
  for (int i = 0; i < ni - 1; i++) dxu[i] = lon[i + 1] - lon[i];
  dxu[ni - 1] = dxu[ni - 2];
  for (int i = 1; i < ni; i++) dxt[i] = 0.5 * (dxu[i] + dxu[i - 1]);
  dxt[0] = dxt[1];
  for (int j = 0; j < nj; j++) {
    const double latp = (j == nj - 1) ? lat[j] + 0.5 * (lat[j] - lat[j - 1]) : 0.5 * (lat[j] + lat[j + 1]);
    const double latm = (j == 0) ? lat[j] - 0.5 * (lat[j + 1] - lat[j]) : 0.5 * (lat[j] + lat[j - 1]);
    const double csj = fgs_cos(latp), csm = fgs_cos(latm), cstr = 1.0 / fgs_cos(lat[j]);
    rn[j] = csj * cstr / (dyt[j] * dyu[j]);
    rs[j] = csm * cstr / (dyt[j] * dyu[j > 0 ? j - 1 : 0]);
    rc[j] = cstr * cstr;
  }
  for (int i = 0; i < ni; i++) {
    ce[i] = dxu[i] * dxt[i];
    cw[i] = dxu[i > 0 ? i - 1 : 0] * dxt[i];
  }
}

static int ex_check_grid(int ni, int nj, const double *lon, const double *lat)
{
  if (ni < 2 || nj < 2) return fg_fail(FG_ERR_ARG, "fg_extrap: the grid must be at least 2 x 2 (ni = %d, nj = %d)", ni, nj);
  if ((long)ni * nj > 0x7fffffffL / 4) return fg_fail(FG_ERR_ARG, "fg_extrap: grid too large");
  if (!lon || !lat) return fg_fail(FG_ERR_ARG, "fg_extrap: null axis");
  for (int j = 0; j < nj; j++)
    if (!(fabs(lat[j]) < 2.4)) return fg_fail(FG_ERR_ARG, "fg_extrap: latitude %d (%g) is not in radians", j, lat[j]);
  return 0;
}

extern "C" int fg_extrap_coef_host(int ni, int nj, const double *lon, const double *lat, double *cfw, double *cfe, double *cfs, double *cfn)
{
  int rc_ = ex_check_grid(ni, nj, lon, lat);
  if (rc_) return rc_;
  if (!cfw || !cfe || !cfs || !cfn) return fg_fail(FG_ERR_ARG, "fg_extrap_coef_host: null output");
  std::vector<double> rn(nj), rs(nj), rc(nj), ce(ni), cw(ni);
  ex_factors(ni, nj, lon, lat, rn.data(), rs.data(), rc.data(), ce.data(), cw.data());
  for (int j = 0; j < nj; j++) for (int i = 0; i < ni; i++) {
    const long n = (long)j * ni + i;
    ex_cell_coef(rn[j], rs[j], rc[j], ce[i], cw[i], cfw[n], cfe[n], cfs[n], cfn[n]);
  }
  return 0;
}

struct fg_extrap {
  int device = 0, ni = 0, nj = 0, is_cyclic = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  double *fac = nullptr;                     // rn | rs | rc | ce | cw
  double *coef = nullptr;                    // [ncell][4], stored mode only (built on first use)
  double *buf[2] = {nullptr, nullptr};       // ping-pong state [nj][ni]
  unsigned long long *sorbits = nullptr;     // one bit per cell: missing at this level
  unsigned long long *slots = nullptr;       // [EX_MAX_ITER] maxima of the level's iterations
  unsigned long long *h_slots = nullptr;     // pinned
  std::vector<double> h_fac;
  long syncs = 0;                            // host synchronisations of the last run's iteration loops
  // fg_extrap_run_batch_dev: the same state for b_cap records, grown on demand
  int b_cap = 0;
  double *b_buf[2] = {nullptr, nullptr};     // [b_cap][ncell]
  unsigned long long *b_bits = nullptr;      // [b_cap][(ncell + 63) / 64]: a record's bits start on a word of their own
  unsigned long long *b_slots = nullptr;     // [EX_MAX_ITER][nrec] of the running call
  unsigned long long *b_h_slots = nullptr;   // pinned
  int *b_par = nullptr, *b_h_par = nullptr;  // [b_cap] buffer that holds record r's state; device / pinned
};

static void ex_batch_free(fg_extrap *h)
{
  (void)hipFree(h->b_buf[0]); (void)hipFree(h->b_buf[1]); (void)hipFree(h->b_bits); (void)hipFree(h->b_slots); (void)hipFree(h->b_par);
  if (h->b_h_slots) (void)hipHostFree(h->b_h_slots);
  if (h->b_h_par) (void)hipHostFree(h->b_h_par);
  h->b_buf[0] = h->b_buf[1] = nullptr; h->b_bits = h->b_slots = h->b_h_slots = nullptr; h->b_par = h->b_h_par = nullptr;
  h->b_cap = 0;
}

extern "C" void fg_extrap_destroy(fg_extrap *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->own_stream) (void)hipStreamDestroy(h->stream);
  (void)hipFree(h->fac); (void)hipFree(h->coef); (void)hipFree(h->buf[0]); (void)hipFree(h->buf[1]);
  (void)hipFree(h->sorbits); (void)hipFree(h->slots);
  if (h->h_slots) (void)hipHostFree(h->h_slots);
  ex_batch_free(h);
  delete h;
}

static int ex_create(int ni, int nj, const double *lon, const double *lat, int is_cyclic, int device, fg_extrap *h)
{
  const long ncell = (long)ni * nj;
  FGCHK(hipSetDevice(device));
  h->device = device; h->ni = ni; h->nj = nj; h->is_cyclic = is_cyclic ? 1 : 0;
  h->h_fac.resize(3 * (size_t)nj + 2 * (size_t)ni);
  double *f = h->h_fac.data();
  ex_factors(ni, nj, lon, lat, f, f + nj, f + 2 * nj, f + 3 * nj, f + 3 * nj + ni);
  FGCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  h->own_stream = true;
  FGCHK(hipMalloc((void **)&h->fac, h->h_fac.size() * sizeof(double)));
  FGCHK(hipMemcpy(h->fac, f, h->h_fac.size() * sizeof(double), hipMemcpyHostToDevice));
  FGCHK(hipMalloc((void **)&h->buf[0], ncell * sizeof(double)));
  FGCHK(hipMalloc((void **)&h->buf[1], ncell * sizeof(double)));
  FGCHK(hipMalloc((void **)&h->sorbits, ((ncell + 63) / 64) * sizeof(unsigned long long)));
  FGCHK(hipMalloc((void **)&h->slots, EX_MAX_ITER * sizeof(unsigned long long)));
  FGCHK(hipHostMalloc((void **)&h->h_slots, EX_MAX_ITER * sizeof(unsigned long long)));
  return 0;
}

extern "C" int fg_extrap_create(int ni, int nj, const double *lon, const double *lat, int is_cyclic, int device, fg_extrap **out)
{
  if (!out) return fg_fail(FG_ERR_ARG, "fg_extrap_create: null output handle");
  *out = nullptr;
  int rc = ex_check_grid(ni, nj, lon, lat);
  if (rc) return rc;
  rc = fg_use_device("fg_extrap_create", device);
  if (rc) return rc;
  fg_extrap *h = new fg_extrap;
  rc = ex_create(ni, nj, lon, lat, is_cyclic, device, h);
  if (rc) { fg_extrap_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" int fg_extrap_set_stream(fg_extrap *h, void *stream)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_extrap_set_stream: null handle");
  (void)hipSetDevice(h->device);
  if (h->stream) FGCHK(hipStreamSynchronize(h->stream));
  if (h->own_stream) (void)hipStreamDestroy(h->stream);
  h->stream = (hipStream_t)stream;
  h->own_stream = false;
  return 0;
}
extern "C" void *fg_extrap_stream(fg_extrap *h) { return h ? (void *)h->stream : nullptr; }
// Internal (column.hip): queue on `stream` for the duration of one call, then take the previous stream back (the caller has
// synchronised `stream` by then).  The handle never owns a borrowed stream.
int fg_extrap_borrow_stream(fg_extrap *h, void *stream, void **saved, int *saved_own)
{
  if (!h) return fg_fail(FG_ERR_ARG, "null extrapolation handle");
  FGCHK(hipSetDevice(h->device));
  if (h->stream) FGCHK(hipStreamSynchronize(h->stream));
  *saved = (void *)h->stream; *saved_own = h->own_stream ? 1 : 0;
  h->stream = (hipStream_t)stream; h->own_stream = false;
  return 0;
}
void fg_extrap_return_stream(fg_extrap *h, void *saved, int saved_own)
{
  if (!h) return;
  h->stream = (hipStream_t)saved; h->own_stream = saved_own != 0;
}
void fg_extrap_dims(const fg_extrap *h, int *ni, int *nj, int *device) { *ni = h->ni; *nj = h->nj; *device = h->device; }
extern "C" long fg_extrap_last_syncs(const fg_extrap *h) { return h ? h->syncs : 0; }

extern "C" int fg_extrap_get_coef(fg_extrap *h, double *cfw, double *cfe, double *cfs, double *cfn)
{
  if (!h || !cfw || !cfe || !cfs || !cfn) return fg_fail(FG_ERR_ARG, "fg_extrap_get_coef: null argument");
  const double *f = h->h_fac.data();
  const int ni = h->ni, nj = h->nj;
  for (int j = 0; j < nj; j++) for (int i = 0; i < ni; i++) {
    const long n = (long)j * ni + i;
    ex_cell_coef(f[j], f[nj + j], f[2 * nj + j], f[3 * nj + i], f[3 * nj + ni + i], cfw[n], cfe[n], cfs[n], cfn[n]);
  }
  return 0;
}

static int ex_stored_coef(fg_extrap *h)
{
  if (h->coef) return 0;
  const long ncell = (long)h->ni * h->nj;
  std::vector<double> c(4 * (size_t)ncell);
  const double *f = h->h_fac.data();
  const int ni = h->ni, nj = h->nj;
  for (int j = 0; j < nj; j++) for (int i = 0; i < ni; i++) {
    double *q = &c[4 * ((size_t)j * ni + i)];
    ex_cell_coef(f[j], f[nj + j], f[2 * nj + j], f[3 * nj + i], f[3 * nj + ni + i], q[0], q[1], q[2], q[3]);
  }
  FGCHK(hipMalloc((void **)&h->coef, c.size() * sizeof(double)));
  FGCHK(hipMemcpy(h->coef, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

extern "C" int fg_extrap_run_dev(fg_extrap *h, const double *d_in, double *d_out, int nk, long level_stride, double missing,
                                 double stop_crit, int *iters_out, double *resmax_out)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_extrap_run_dev: null handle");
  if (nk < 1 || !d_in || !d_out) return fg_fail(FG_ERR_ARG, "fg_extrap_run_dev: bad argument");
  const long ncell = (long)h->ni * h->nj;
  if (level_stride == 0) level_stride = ncell;
  if (level_stride < ncell) return fg_fail(FG_ERR_ARG, "fg_extrap_run_dev: level_stride smaller than a level");
  FGCHK(hipSetDevice(h->device));
  const int batch = g_batch;
  ExGrid g;
  g.ni = h->ni; g.nj = h->nj; g.is_cyclic = h->is_cyclic;
  g.f.rn = h->fac; g.f.rs = h->fac + h->nj; g.f.rc = h->fac + 2 * h->nj; g.f.ce = h->fac + 3 * h->nj; g.f.cw = h->fac + 3 * h->nj + h->ni;
  g.coef = nullptr;
  if (g_coef_mode) {
    int rc = ex_stored_coef(h);
    if (rc) return rc;
    g.coef = h->coef;
  }
  hipStream_t st = h->stream;
  h->syncs = 0;
  int cur = 0;                                                        // buffer that holds the state
  for (int k = 0; k < nk; k++) {
    // valid points take this level's data, missing ones keep the level above's solution (:2734-2745)
    fgd_ex_prepare(g, d_in + (long)k * level_stride, missing, k ? h->buf[cur] : nullptr, h->buf[0], h->sorbits, st);
    cur = 0;
    FGCHK(hipMemsetAsync(h->slots, 0, EX_MAX_ITER * sizeof(unsigned long long), st));
    int stop = -1;
    for (int n0 = 0; n0 < EX_MAX_ITER && stop < 0; n0 += batch) {
      const int n1 = n0 + batch < EX_MAX_ITER ? n0 + batch : EX_MAX_ITER;
      for (int n = n0; n < n1; n++)                                   // iteration n: buf[n & 1] -> buf[(n + 1) & 1]
        fgd_ex_iterate(g, h->buf[n & 1], h->buf[(n + 1) & 1], h->sorbits, stop_crit, n ? h->slots + n - 1 : nullptr, h->slots + n, st);
      FGCHK(hipGetLastError());
      FGCHK(hipMemcpyAsync(h->h_slots + n0, h->slots + n0, (size_t)(n1 - n0) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      FGCHK(hipStreamSynchronize(st));
      h->syncs++;
      for (int n = n0; n < n1; n++) {
        double r;
        memcpy(&r, &h->h_slots[n], sizeof r);
        if (r <= stop_crit || n == EX_MAX_ITER - 1) { stop = n; break; }   // :2769
      }
    }
    cur = (stop + 1) & 1;
    if (iters_out) iters_out[k] = stop;
    if (resmax_out) memcpy(&resmax_out[k], &h->h_slots[stop], sizeof(double));
    FGCHK(hipMemcpyAsync(d_out + (long)k * level_stride, h->buf[cur], ncell * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  FGCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int fg_extrap_run(fg_extrap *h, const double *in, double *out, int nk, double missing, double stop_crit,
                             int *iters_out, double *resmax_out)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_extrap_run: null handle");
  if (nk < 1 || !in || !out) return fg_fail(FG_ERR_ARG, "fg_extrap_run: bad argument");
  FGCHK(hipSetDevice(h->device));
  const size_t bytes = (size_t)h->ni * h->nj * (size_t)nk * sizeof(double);
  double *d = nullptr;
  FGCHK(hipMalloc((void **)&d, bytes));
  int rc = 0;
  hipError_t e = hipMemcpy(d, in, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    rc = fg_extrap_run_dev(h, d, d, nk, 0, missing, stop_crit, iters_out, resmax_out);   // in place: a level is read before it is written
    if (!rc) e = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
  }
  (void)hipFree(d);
  if (e != hipSuccess) return fg_fail(FG_ERR_HIP, "fg_extrap_run: copy failed: %s", hipGetErrorString(e));
  return rc;
}

// ------------------------------------------------------------------------------------------------ several records per launch
static int ex_batch_reserve(fg_extrap *h, int nrec)
{
  if (nrec <= h->b_cap) return 0;
  FGCHK(hipStreamSynchronize(h->stream));
  ex_batch_free(h);
  const size_t ncell = (size_t)h->ni * h->nj, nwords = (ncell + 63) / 64, n = (size_t)nrec;
  FGCHK(hipMalloc((void **)&h->b_buf[0], n * ncell * sizeof(double)));
  FGCHK(hipMalloc((void **)&h->b_buf[1], n * ncell * sizeof(double)));
  FGCHK(hipMalloc((void **)&h->b_bits, n * nwords * sizeof(unsigned long long)));
  FGCHK(hipMalloc((void **)&h->b_slots, n * EX_MAX_ITER * sizeof(unsigned long long)));
  FGCHK(hipMalloc((void **)&h->b_par, n * sizeof(int)));
  FGCHK(hipHostMalloc((void **)&h->b_h_slots, n * EX_MAX_ITER * sizeof(unsigned long long)));
  FGCHK(hipHostMalloc((void **)&h->b_h_par, n * sizeof(int)));
  h->b_cap = nrec;
  return 0;
}

// fg_extrap_run_dev for nrec records that advance through the levels in lockstep: one prepare launch per level and one launch per
// iteration for all of them.  A record is its own problem -- its own slots (laid out [iteration][record], so a batch of launches
// is one contiguous region: one memset per level, one copy per synchronisation), stop, ping-pong parity and mask words -- and the
// next level starts when every record has stopped on this one.
extern "C" int fg_extrap_run_batch_dev(fg_extrap *h, int nrec, const double *d_in, double *d_out, int nk, long level_stride,
                                       long rec_stride, double missing, double stop_crit, int *iters_out, double *resmax_out)
{
  if (!h) return fg_fail(FG_ERR_ARG, "fg_extrap_run_batch_dev: null handle");
  if (nrec < 1 || nrec > 65535 || nk < 1 || !d_in || !d_out) return fg_fail(FG_ERR_ARG, "fg_extrap_run_batch_dev: bad argument");
  const long ncell = (long)h->ni * h->nj;
  if (level_stride == 0) level_stride = ncell;
  if (level_stride < ncell) return fg_fail(FG_ERR_ARG, "fg_extrap_run_batch_dev: level_stride smaller than a level");
  if (rec_stride == 0) rec_stride = (long)nk * level_stride;
  if (rec_stride < (long)(nk - 1) * level_stride + ncell) return fg_fail(FG_ERR_ARG, "fg_extrap_run_batch_dev: rec_stride smaller than a record");
  FGCHK(hipSetDevice(h->device));
  int rc = ex_batch_reserve(h, nrec);
  if (rc) return rc;
  const int batch = g_batch;
  ExGrid g;
  g.ni = h->ni; g.nj = h->nj; g.is_cyclic = h->is_cyclic;
  g.f.rn = h->fac; g.f.rs = h->fac + h->nj; g.f.rc = h->fac + 2 * h->nj; g.f.ce = h->fac + 3 * h->nj; g.f.cw = h->fac + 3 * h->nj + h->ni;
  g.coef = nullptr;
  if (g_coef_mode) {
    rc = ex_stored_coef(h);
    if (rc) return rc;
    g.coef = h->coef;
  }
  hipStream_t st = h->stream;
  h->syncs = 0;
  std::vector<int> stop(nrec);
  for (int k = 0; k < nk; k++) {
    fgd_ex_prepare_batch(g, nrec, d_in + (long)k * level_stride, rec_stride, missing, h->b_buf[0], h->b_buf[1], k ? h->b_par : nullptr,
                         h->b_buf[0], h->b_bits, st);
    FGCHK(hipMemsetAsync(h->b_slots, 0, (size_t)nrec * EX_MAX_ITER * sizeof(unsigned long long), st));
    int running = nrec;
    for (int r = 0; r < nrec; r++) stop[r] = -1;
    for (int n0 = 0; n0 < EX_MAX_ITER && running > 0; n0 += batch) {
      const int n1 = n0 + batch < EX_MAX_ITER ? n0 + batch : EX_MAX_ITER;
      for (int n = n0; n < n1; n++)                                   // iteration n: buf[n & 1] -> buf[(n + 1) & 1], every record
        fgd_ex_iterate_batch(g, nrec, h->b_buf[n & 1], h->b_buf[(n + 1) & 1], h->b_bits, stop_crit,
                             n ? h->b_slots + (size_t)(n - 1) * nrec : nullptr, h->b_slots + (size_t)n * nrec, st);
      FGCHK(hipGetLastError());
      FGCHK(hipMemcpyAsync(h->b_h_slots + (size_t)n0 * nrec, h->b_slots + (size_t)n0 * nrec,
                           (size_t)(n1 - n0) * nrec * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      FGCHK(hipStreamSynchronize(st));
      h->syncs++;
      for (int r = 0; r < nrec; r++) {
        if (stop[r] >= 0) continue;
        for (int n = n0; n < n1; n++) {
          double v;
          memcpy(&v, &h->b_h_slots[(size_t)n * nrec + r], sizeof v);
          if (v <= stop_crit || n == EX_MAX_ITER - 1) { stop[r] = n; running--; break; }   // :2769
        }
      }
    }
    for (int r = 0; r < nrec; r++) {
      h->b_h_par[r] = (stop[r] + 1) & 1;
      if (iters_out) iters_out[(size_t)r * nk + k] = stop[r];
      if (resmax_out) memcpy(&resmax_out[(size_t)r * nk + k], &h->b_h_slots[(size_t)stop[r] * nrec + r], sizeof(double));
    }
    // (the stream is idle here, and the next write of b_h_par comes after the next synchronisation: the copy has run by then)
    FGCHK(hipMemcpyAsync(h->b_par, h->b_h_par, (size_t)nrec * sizeof(int), hipMemcpyHostToDevice, st));
    fgd_ex_copy_out_batch(g, nrec, h->b_buf[0], h->b_buf[1], h->b_par, d_out + (long)k * level_stride, rec_stride, st);
  }
  FGCHK(hipGetLastError());
  FGCHK(hipStreamSynchronize(st));
  return 0;
}

// ------------------------------------------------------------------------------------------------ vertical interpolation
extern "C" int fg_setup_vertical_interp(int nk1, const double *z1, int nk2, const double *z2, int *kstart_out, int *kend_out,
                                        int *need_interp_out)
{
  if (nk1 < 1 || nk2 < 1 || !z1 || !z2) return fg_fail(FG_ERR_ARG, "fg_setup_vertical_interp: bad argument");
  int kstart, kend, need = 1;
  for (kstart = 0; kstart < nk2; kstart++) if (z2[kstart] >= z1[0]) break;            // fregrid_util.c:764-769
  for (kend = nk2 - 1; kend >= 0; kend--) if (z2[kend] <= z1[nk1 - 1]) break;
  if (nk1 == nk2) {
    int k;
    for (k = 0; k < nk1; k++) if (fabs(z2[k] - z1[k]) > EX_EPSLN10) break;            // :781-786
    if (k == nk1) need = 0;
  }
  if (kstart_out) *kstart_out = kstart;
  if (kend_out) *kend_out = kend;
  if (need_interp_out) *need_interp_out = need;
  return 0;
}

static int ex_nearest_index(double value, const double *array, int ia)              // mosaic_util.c:81-109
{
  if (value < array[0]) return 0;
  if (value > array[ia - 1]) return ia - 1;
  for (int i = 1; i < ia; i++)
    if (value <= array[i]) return (array[i] - value > value - array[i - 1]) ? i - 1 : i;
  return ia - 1;
}

extern "C" int fg_dev_vertical_interp(long nxy, int nk1, const double *z1, int nk2, const double *z2, const double *d_in, double *d_out)
{
  if (nxy < 1 || !d_in || !d_out) return fg_fail(FG_ERR_ARG, "fg_dev_vertical_interp: bad argument");
  if (nk2 > 65535) return fg_fail(FG_ERR_ARG, "fg_dev_vertical_interp: more than 65535 destination levels");
  int kstart, kend, need;
  int rc = fg_setup_vertical_interp(nk1, z1, nk2, z2, &kstart, &kend, &need);
  if (rc) return rc;
  if (!need) {                                                                        // do_vertical_interp leaves the field alone (:794)
    if (d_in != d_out) FGCHK(hipMemcpy(d_out, d_in, (size_t)nxy * nk1 * sizeof(double), hipMemcpyDeviceToDevice));
    return 0;
  }
  if (d_in == d_out) return fg_fail(FG_ERR_ARG, "fg_dev_vertical_interp: in and out must be different arrays");
  std::vector<ExVLevel> lev;
  rc = ex_vertical_levels(nk1, z1, nk2, z2, lev, &need);                              // (the fatal checks come after the argument check)
  if (rc) return rc;
  ExVLevel *d_lev = nullptr;
  FGCHK(hipMalloc((void **)&d_lev, lev.size() * sizeof(ExVLevel)));
  hipError_t e = hipMemcpy(d_lev, lev.data(), lev.size() * sizeof(ExVLevel), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    fgd_ex_vertical(nxy, nk2, d_lev, d_in, d_out, nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  }
  (void)hipFree(d_lev);
  if (e != hipSuccess) return fg_fail(FG_ERR_HIP, "fg_dev_vertical_interp: %s", hipGetErrorString(e));
  return 0;
}

int ex_vertical_levels(int nk1, const double *z1, int nk2, const double *z2, std::vector<ExVLevel> &lev, int *need_out)
{
  int kstart, kend, need;
  int rc = fg_setup_vertical_interp(nk1, z1, nk2, z2, &kstart, &kend, &need);
  if (rc) return rc;
  *need_out = need;
  if (!need) return 0;
  const int nk = kend - kstart + 1;
  if (nk < 1) return fg_fail(FG_ERR_DATA, "interp.c: grid2 lies outside grid1");
  const double *g1 = z1, *g2 = z2 + kstart;
  // linear_vertical_interp's fatal checks (interp.c:366-374), nearest_index's (mosaic_util.c:86-89)
  for (int k = 1; k < nk1; k++) if (g1[k] <= g1[k - 1]) return fg_fail(FG_ERR_DATA, "interp.c: grid1 not monotonic");
  for (int k = 1; k < nk; k++) if (g2[k] <= g2[k - 1]) return fg_fail(FG_ERR_DATA, "interp.c: grid2 not monotonic");
  if (g1[0] > g2[0]) return fg_fail(FG_ERR_DATA, "interp.c: grid2 lies outside grid1");
  if (g1[nk1 - 1] < g2[nk - 1]) return fg_fail(FG_ERR_DATA, "interp.c: grid2 lies outside grid1");
  lev.assign(nk2, ExVLevel());
  for (int k = 0; k < nk2; k++) {
    ExVLevel &L = lev[k];
    L.a = L.b = 0; L.interp = 0; L.w = 0.0;
    if (k < kstart) continue;                                                         // the shallowest source level (:808-810)
    if (k > kend) { L.a = nk1 - 1; continue; }                                        // the deepest one (:811-813; level kend is overwritten below)
    const double v = z2[k];
    const int n = ex_nearest_index(v, g1, nk1);
    if (g1[n] < v) { L.interp = 1; L.a = n; L.b = n + 1; L.w = (v - g1[n]) / (g1[n + 1] - g1[n]); }
    else if (n == 0) L.a = 0;
    else { L.interp = 1; L.a = n - 1; L.b = n; L.w = (v - g1[n - 1]) / (g1[n] - g1[n - 1]); }
  }
  return 0;
}
