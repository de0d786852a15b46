// column.hip -- fg_column: fregrid's ocean column loop, `--extrapolate --dst_vgrid`, streamed (include/fregrid_hip.h, "column loop").
//
// Per variable and record the reference reads the whole column and fills its missing points (get_input_data with level_z = -1,
// fregrid_util.c:2126-2135; the fill clears has_missing), remaps all nz levels in the plain branch of do_scalar_conserve_interp
// (conserve_interp.c:592-615), puts them on the --dst_vgrid levels (do_vertical_interp) and writes them in the file's type
// (fregrid.c:1026-1043).  Here a chunk of records takes that path together: typed upload -> k_widen -> the batched fill
// (fg_extrap_run_batch_dev: one launch per iteration for all records of the chunk) -> fg_plan_apply on records x nk1 planes per
// plan -> one kernel for the vertical interpolation and the narrowing -> typed download.  Slots, streams and events are the
// conservative sweep's (stream_slots.h).  The fill waits on the host for its slots, so the upload of chunk c+1 is queued BEFORE
// chunk c is computed: while the host sits in the fill, the copy-in stream carries c+1 and the copy-out stream c-1.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <vector>
#include "extrap.h"
#include "fg_host.h"
#include "stream_slots.h"

extern "C" int fg_plan_order(const fg_plan *pl);
extern "C" long fg_plan_ncells_out(const fg_plan *pl);
extern "C" int fg_plan_device(const fg_plan *pl);
int fg_plan_borrow_stream(fg_plan *pl, void *stream, void **saved, int *saved_own);
void fg_plan_return_stream(fg_plan *pl, void *saved, int saved_own);
int fg_plan_is_finalized(const fg_plan *pl);

using namespace fg_stream;

// Records per chunk: as many as fit, with every buffer of the pipeline, in COL_MEM_SHARE of the free device memory, at most
// COL_MAX_RECORDS, and never more planes than one fg_plan_apply takes (2048).
#define COL_MAX_RECORDS 8
#define COL_MEM_SHARE 0.25
#define COL_MAX_PLANES 2048
static std::atomic<int> g_col_records{0};
extern "C" int fg_set_column_records(int n) { g_col_records = n < 1 ? 0 : n; return g_col_records; }

struct fg_column {
  fg_extrap *ex = nullptr;
  int device = 0, in_type = FG_NC_DOUBLE, out_type = FG_NC_DOUBLE, nk1 = 0, nk2 = 0;
  size_t in_sz = 8, out_sz = 8;
  std::vector<fg_plan *> plans;
  std::vector<long> ndst, pre;             // cells per plan; cells of the plans before it
  long ncin = 0, ndst_total = 0;
  ExVLevel *d_lev = nullptr;               // [nk2] (the identity without --dst_vgrid and with need_interp = 0)
  hipStream_t s_in = nullptr, s_comp = nullptr, s_out = nullptr;
  int cap = 0;                             // records the buffers below hold
  double *d_f64 = nullptr, *d_tmp = nullptr;   // filled columns [cap][nk1][ncin]; remapped ones [plan][cap][nk1][ndst_p]
  struct Slot {
    void *d_raw = nullptr, *d_fin = nullptr;     // [cap][nk1][ncin] of in_type; [plan][cap][nk2][ndst_p] of out_type
    void *pin_in = nullptr, *pin_out = nullptr;  // staging for pageable user memory (allocated on first need)
    hipEvent_t e_in = nullptr, e_comp = nullptr, e_out = nullptr;
    bool busy = false, staged_out = false;
    long r0 = 0; int nr = 0;
  } slot[NSLOT];
};

static void col_free_buffers(fg_column *c)
{
  for (auto &sl : c->slot) {
    (void)hipFree(sl.d_raw); (void)hipFree(sl.d_fin);
    if (sl.pin_in) (void)hipHostFree(sl.pin_in);
    if (sl.pin_out) (void)hipHostFree(sl.pin_out);
    sl.d_raw = sl.d_fin = sl.pin_in = sl.pin_out = nullptr;
  }
  (void)hipFree(c->d_f64); (void)hipFree(c->d_tmp);
  c->d_f64 = c->d_tmp = nullptr;
  c->cap = 0;
}

extern "C" void fg_column_destroy(fg_column *c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (hipStream_t s : {c->s_in, c->s_comp, c->s_out}) if (s) (void)hipStreamSynchronize(s);
  col_free_buffers(c);
  for (auto &sl : c->slot) for (hipEvent_t e : {sl.e_in, sl.e_comp, sl.e_out}) if (e) (void)hipEventDestroy(e);
  (void)hipFree(c->d_lev);
  for (hipStream_t s : {c->s_in, c->s_comp, c->s_out}) if (s) (void)hipStreamDestroy(s);
  delete c;
}

extern "C" int fg_column_create(fg_extrap *ex, int nplans, fg_plan *const *plans, int in_type, int out_type, int nk1, const double *z1,
                                int nk2, const double *z2, fg_column **out)
{
  if (!ex || nplans < 1 || !plans || !out) return fg_fail(FG_ERR_ARG, "fg_column_create: null argument");
  *out = nullptr;
  if (!type_size(in_type) || !type_size(out_type)) return fg_fail(FG_ERR_ARG, "fg_column_create: types must be FG_NC_SHORT, FG_NC_INT, FG_NC_FLOAT or FG_NC_DOUBLE");
  if (nk1 < 1 || nk1 > COL_MAX_PLANES || (z2 && (nk2 < 1 || nk2 > 65535 || !z1))) return fg_fail(FG_ERR_ARG, "fg_column_create: bad number of levels");
  int ni, nj, device;
  fg_extrap_dims(ex, &ni, &nj, &device);
  for (int p = 0; p < nplans; p++)
    if (!plans[p] || fg_plan_order(plans[p]) != 1 || !fg_plan_is_finalized(plans[p]) || fg_plan_ncells_in(plans[p]) != (long)ni * nj ||
        fg_plan_device(plans[p]) != device)
      return fg_fail(FG_ERR_ARG, "fg_column_create: the plans must be finalized conserve_order1 plans on the extrapolator's %d x %d grid and device", ni, nj);
  // the bracket table; linear_vertical_interp's fatal checks are raised here, before any field is touched
  std::vector<ExVLevel> lev;
  int need = 0;
  if (z2) { int rc = ex_vertical_levels(nk1, z1, nk2, z2, lev, &need); if (rc) return rc; }
  if (!need) {                                          // no --dst_vgrid, or do_vertical_interp leaves the field alone (:794)
    nk2 = nk1;
    lev.assign(nk1, ExVLevel());
    for (int k = 0; k < nk1; k++) { lev[k].a = lev[k].b = k; lev[k].interp = 0; lev[k].w = 0.0; }
  }
  fg_column *c = new fg_column();
  c->ex = ex; c->device = device; c->in_type = in_type; c->out_type = out_type; c->in_sz = type_size(in_type); c->out_sz = type_size(out_type);
  c->nk1 = nk1; c->nk2 = nk2; c->ncin = (long)ni * nj;
  for (int p = 0; p < nplans; p++) {
    c->plans.push_back(plans[p]);
    c->pre.push_back(c->ndst_total);
    c->ndst.push_back(fg_plan_ncells_out(plans[p]));
    c->ndst_total += c->ndst.back();
  }
  bool ok = hipSetDevice(device) == hipSuccess;
  ok = ok && hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking) == hipSuccess &&
       hipStreamCreateWithFlags(&c->s_comp, hipStreamNonBlocking) == hipSuccess &&
       hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking) == hipSuccess;
  for (auto &sl : c->slot)
    ok = ok && hipEventCreateWithFlags(&sl.e_in, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&sl.e_comp, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&sl.e_out, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipMalloc((void **)&c->d_lev, lev.size() * sizeof(ExVLevel)) == hipSuccess &&
       hipMemcpy(c->d_lev, lev.data(), lev.size() * sizeof(ExVLevel), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); fg_column_destroy(c); return fg_fail(FG_ERR_HIP, "fg_column_create: out of device memory (or stream / event creation failed)"); }
  *out = c;
  return 0;
}

// device bytes one record of a chunk costs: its raw and finished copies in every slot, the filled and the remapped columns, and
// the fill's own state (two arrays, mask bits, slots)
static size_t col_bytes_per_record(const fg_column *c)
{
  const size_t in = (size_t)c->nk1 * c->ncin, mid = (size_t)c->nk1 * c->ndst_total, fin = (size_t)c->nk2 * c->ndst_total;
  return NSLOT * (in * c->in_sz + fin * c->out_sz) + (in + mid) * 8 + (size_t)c->ncin * 17 + EX_MAX_ITER * 8;
}

static int col_reserve(fg_column *c, int R)
{
  if (R <= c->cap) return 0;
  for (hipStream_t s : {c->s_in, c->s_comp, c->s_out}) FGCHK(hipStreamSynchronize(s));
  col_free_buffers(c);
  const size_t in = (size_t)R * c->nk1 * c->ncin, mid = (size_t)R * c->nk1 * c->ndst_total, fin = (size_t)R * c->nk2 * c->ndst_total;
  for (auto &sl : c->slot) {
    FGCHK(hipMalloc(&sl.d_raw, in * c->in_sz));
    FGCHK(hipMalloc(&sl.d_fin, fin * c->out_sz));
  }
  FGCHK(hipMalloc((void **)&c->d_f64, in * 8));
  FGCHK(hipMalloc((void **)&c->d_tmp, mid * 8));
  c->cap = R;
  return 0;
}

// wait for a slot's chunk to be back on the host, then hand staged outputs to the user's pageable arrays
static int col_retire(fg_column *c, fg_column::Slot &sl, void *const *host_out)
{
  if (!sl.busy) return 0;
  FGCHK(hipEventSynchronize(sl.e_out));
  if (sl.staged_out)
    for (size_t p = 0; p < c->plans.size(); p++) {
      const size_t rec = (size_t)c->nk2 * c->ndst[p] * c->out_sz;
      memcpy((char *)host_out[p] + (size_t)sl.r0 * rec, (char *)sl.pin_out + (size_t)c->pre[p] * c->cap * c->nk2 * c->out_sz, (size_t)sl.nr * rec);
    }
  sl.busy = false;
  return 0;
}

extern "C" int fg_column_run(fg_column *c, const void *host_in, long nrec, double scale, double offset, double missing, double stop_crit,
                             void *const *host_out, int *iters_out, double *resmax_out)
{
  if (!c || !host_in || !host_out || nrec < 1) return fg_fail(FG_ERR_ARG, "fg_column_run: null argument");
  const size_t nplans = c->plans.size();
  for (size_t p = 0; p < nplans; p++) if (!host_out[p]) return fg_fail(FG_ERR_ARG, "fg_column_run: null output array");
  FGCHK(hipSetDevice(c->device));
  int R = g_col_records;
  if (R < 1) {
    size_t free_b = 0, total_b = 0;
    FGCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t fit = (size_t)(COL_MEM_SHARE * (double)free_b) / col_bytes_per_record(c);
    R = fit < 1 ? 1 : fit > COL_MAX_RECORDS ? COL_MAX_RECORDS : (int)fit;
    if (R < c->cap && c->cap <= COL_MAX_RECORDS) R = c->cap;           // an earlier run's buffers are part of what is no longer free
  }
  if (R > nrec) R = (int)nrec;
  if ((long)R * c->nk1 > COL_MAX_PLANES) R = COL_MAX_PLANES / c->nk1;
  { int rc = col_reserve(c, R); if (rc) return rc; }
  // The plans and the extrapolator launch on OUR compute stream for the duration of this call only (fg_sweep_run's rule): on
  // every way out the three streams are drained, the borrowed streams handed back and the slots cleared.
  struct Borrow {
    fg_column *c; std::vector<void *> saved; std::vector<int> own; void *x_saved = nullptr; int x_own = 0; bool x_on = false;
    ~Borrow()
    {
      for (hipStream_t s : {c->s_in, c->s_comp, c->s_out}) (void)hipStreamSynchronize(s);
      for (size_t p = 0; p < saved.size(); p++) fg_plan_return_stream(c->plans[p], saved[p], own[p]);
      if (x_on) fg_extrap_return_stream(c->ex, x_saved, x_own);
      for (auto &sl : c->slot) { sl.busy = false; sl.staged_out = false; }
    }
  } borrow{c};
  for (fg_plan *p : c->plans) {
    void *sv = nullptr; int ow = 0;
    if (fg_plan_borrow_stream(p, c->s_comp, &sv, &ow)) return FG_ERR_HIP;
    borrow.saved.push_back(sv); borrow.own.push_back(ow);
  }
  if (fg_extrap_borrow_stream(c->ex, c->s_comp, &borrow.x_saved, &borrow.x_own)) return FG_ERR_HIP;
  borrow.x_on = true;
  const bool in_pinned = is_pinned(host_in);
  bool out_pinned = true;
  for (size_t p = 0; p < nplans; p++) out_pinned = out_pinned && is_pinned(host_out[p]);
  const size_t rec_in = (size_t)c->nk1 * c->ncin;                      // elements of one record on the way in
  const bool widen_pass = c->in_type != FG_NC_DOUBLE || scale != 0 || offset != 0;
  const long nchunk = (nrec + R - 1) / R;
  const long cap = c->cap;                                             // the buffers' record stride between the plans' blocks

  auto upload = [&](long ch) -> int {
    fg_column::Slot &sl = c->slot[ch % NSLOT];
    int rc = col_retire(c, sl, host_out);
    if (rc) return rc;
    const long r0 = ch * R;
    const int nr = (int)(nrec - r0 < R ? nrec - r0 : R);
    const size_t bytes = (size_t)nr * rec_in * c->in_sz;
    const char *src = (const char *)host_in + (size_t)r0 * rec_in * c->in_sz;
    if (!in_pinned) {
      if (!sl.pin_in) FGCHK(hipHostMalloc(&sl.pin_in, (size_t)cap * rec_in * c->in_sz, hipHostMallocDefault));
      memcpy(sl.pin_in, src, bytes);
      src = (const char *)sl.pin_in;
    }
    FGCHK(hipMemcpyAsync(sl.d_raw, src, bytes, hipMemcpyHostToDevice, c->s_in));
    FGCHK(hipEventRecord(sl.e_in, c->s_in));
    sl.r0 = r0; sl.nr = nr;
    return 0;
  };

  { int rc = upload(0); if (rc) return rc; }
  for (long ch = 0; ch < nchunk; ch++) {
    if (ch + 1 < nchunk) { int rc = upload(ch + 1); if (rc) return rc; }
    fg_column::Slot &sl = c->slot[ch % NSLOT];
    const long r0 = sl.r0;
    const int nr = sl.nr;
    // --- widen, fill, remap, vertical + narrow (compute stream)
    FGCHK(hipStreamWaitEvent(c->s_comp, sl.e_in, 0));
    const double *f64 = (const double *)sl.d_raw;
    if (widen_pass) {
      widen(c->in_type, (long)((size_t)nr * rec_in), sl.d_raw, scale, offset, missing, c->d_f64, c->s_comp);
      f64 = c->d_f64;
    }
    int rc = fg_extrap_run_batch_dev(c->ex, nr, f64, c->d_f64, c->nk1, 0, 0, missing, stop_crit,
                                     iters_out ? iters_out + (size_t)r0 * c->nk1 : nullptr,
                                     resmax_out ? resmax_out + (size_t)r0 * c->nk1 : nullptr);
    if (rc) return rc;
    for (size_t p = 0; p < nplans; p++) {
      // has_missing is 0 after the fill: the plain branch, all nr x nk1 planes in one call (conserve_interp.c:592-615)
      double *mid = c->d_tmp + (size_t)c->pre[p] * cap * c->nk1;
      rc = fg_plan_apply(c->plans[p], c->d_f64, nullptr, nullptr, nullptr, 0, 0.0, nr * c->nk1, mid, nullptr);
      if (rc) return rc;
      fgd_ex_vertical_narrow(c->out_type, c->ndst[p], nr, c->nk1, c->nk2, c->d_lev, mid, scale, offset, missing,
                             (char *)sl.d_fin + (size_t)c->pre[p] * cap * c->nk2 * c->out_sz, c->s_comp);
    }
    FGCHK(hipGetLastError());
    FGCHK(hipEventRecord(sl.e_comp, c->s_comp));
    // --- download (copy-out stream)
    FGCHK(hipStreamWaitEvent(c->s_out, sl.e_comp, 0));
    if (!out_pinned && !sl.pin_out) FGCHK(hipHostMalloc(&sl.pin_out, (size_t)cap * c->nk2 * c->ndst_total * c->out_sz, hipHostMallocDefault));
    for (size_t p = 0; p < nplans; p++) {
      const size_t rec = (size_t)c->nk2 * c->ndst[p] * c->out_sz, off = (size_t)c->pre[p] * cap * c->nk2 * c->out_sz;
      char *dst = out_pinned ? (char *)host_out[p] + (size_t)r0 * rec : (char *)sl.pin_out + off;
      FGCHK(hipMemcpyAsync(dst, (const char *)sl.d_fin + off, (size_t)nr * rec, hipMemcpyDeviceToHost, c->s_out));
    }
    FGCHK(hipEventRecord(sl.e_out, c->s_out));
    sl.busy = true; sl.staged_out = !out_pinned;
  }
  // drain in chunk order
  for (long ch = (nchunk > NSLOT ? nchunk - NSLOT : 0); ch < nchunk; ch++) { int rc = col_retire(c, c->slot[ch % NSLOT], host_out); if (rc) return rc; }
  return 0;
}
