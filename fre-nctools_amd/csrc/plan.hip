// plan.hip -- host orchestration and the C ABI of libfregrid_hip.so (see include/fregrid_hip.h).
//
// A plan owns, in HBM, everything one destination tile needs: per-cell records of the
// source tiles and of the destination tile, the exchange cells in canonical order and the
// destination-row CSR layout for the sweep.  Device memory comes from a small caching pool
// so that repeated plan creation (one per destination tile / per benchmark step) does not
// pay hipMalloc/hipFree.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include "fg_host.h"
#include "plan_internal.h"
#include "xgrid_device.h"

// ----------------------------------------------------------------------------- errors
static thread_local std::string g_err;
extern "C" const char *fg_last_error(void) { return g_err.c_str(); }
void fg_set_last_error(const char *msg) { g_err = msg ? msg : ""; }      // what fg_host.h's fg_fail writes, in every translation unit

extern "C" int fg_device_count(void)
{
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { fg_fail(FG_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); return FG_ERR_HIP; }
  return n;
}

// Streams and events are cached per process: creating and destroying a stream costs ~0.1 ms each on this runtime, which
// was a quarter of a millisecond per plan (scripts/host_time.py).
struct HandleCache {
  std::mutex mu;
  std::map<int, std::vector<hipStream_t>> streams;
  std::map<int, std::vector<hipEvent_t>> events;        // per device, like the streams: an event belongs to its device
  static int current_device() { int d = 0; (void)hipGetDevice(&d); return d; }
  hipStream_t get_stream(int dev)
  {
    {
      std::lock_guard<std::mutex> lk(mu);
      auto &v = streams[dev];
      if (!v.empty()) { hipStream_t s = v.back(); v.pop_back(); return s; }
    }
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    return s;
  }
  void put_stream(int dev, hipStream_t s)
  {
    if (!s) return;
    std::lock_guard<std::mutex> lk(mu);
    streams[dev].push_back(s);
  }
  hipEvent_t get_event()
  {
    {
      std::lock_guard<std::mutex> lk(mu);
      auto &v = events[current_device()];
      if (!v.empty()) { hipEvent_t e = v.back(); v.pop_back(); return e; }
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  void put_event(hipEvent_t e)
  {
    if (!e) return;
    std::lock_guard<std::mutex> lk(mu);
    events[current_device()].push_back(e);
  }
  // ordering-only events (the plan's stream <-> its second stream in the great-circle clip, the readback of a fused search, a
  // plan's `done` mark, the pool's tagged blocks).  dev < 0: the current device (where a new event is created in any case).
  std::map<int, std::vector<hipEvent_t>> sync_events;
  hipEvent_t get_sync_event(int dev = -1)
  {
    {
      std::lock_guard<std::mutex> lk(mu);
      auto &v = sync_events[dev >= 0 ? dev : current_device()];
      if (!v.empty()) { hipEvent_t e = v.back(); v.pop_back(); return e; }
    }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return e;
  }
  void put_sync_event(hipEvent_t e, int dev = -1)
  {
    if (!e) return;
    std::lock_guard<std::mutex> lk(mu);
    sync_events[dev >= 0 ? dev : current_device()].push_back(e);
  }
};
static HandleCache g_handles;

// ----------------------------------------------------------------------------- memory pool
// The bookkeeping is dev_pool.h's; this is the policy that makes its device calls.  Events come from g_handles' ordering-only
// cache.  Without an event (creation failed), or when the record fails, the batch's device is synchronised instead.
#include "dev_pool.h"
namespace {
struct HipPoolPolicy {
  typedef hipStream_t Stream;
  typedef hipEvent_t Event;
  static void *dev_malloc(size_t c) { void *p = nullptr; if (hipMalloc(&p, c) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
  static void dev_free(void *p) { (void)hipFree(p); }
  struct OnDevice {                                    // an event belongs to the device it was created on, a record to the stream's
    int old = -1, dev;
    explicit OnDevice(int d) : dev(d) { if (hipGetDevice(&old) != hipSuccess) old = -1; if (old != dev) (void)hipSetDevice(dev); }
    ~OnDevice() { if (old >= 0 && old != dev) (void)hipSetDevice(old); }
  };
  static Event event_get(int dev) { OnDevice on(dev); return g_handles.get_sync_event(dev); }
  static void event_put(int dev, Event e) { g_handles.put_sync_event(e, dev); }
  static void event_record(int dev, Event e, Stream s)
  {
    OnDevice on(dev);
    if (!e || hipEventRecord(e, s) != hipSuccess) { (void)hipGetLastError(); (void)hipDeviceSynchronize(); }
  }
  static bool event_passed(Event e) { return !e || hipEventQuery(e) != hipErrorNotReady; }
  static void stream_wait(Stream s, Event e) { if (e && hipStreamWaitEvent(s, e, 0) != hipSuccess) (void)hipEventSynchronize(e); }
  static void event_wait_host(Event e) { if (e) (void)hipEventSynchronize(e); }
  static bool poison_on()
  {
    static const bool on = getenv("FREGRID_HIP_POISON") && atoi(getenv("FREGRID_HIP_POISON")) != 0;
    return on;
  }
  // (the first synchronise: a tagged block may still be in use by queued work, and the fill runs on the null stream)
  static void poison(void *p, size_t c) { (void)hipDeviceSynchronize(); (void)hipMemset(p, 0x7f, c); (void)hipDeviceSynchronize(); }
};
typedef DevPool<HipPoolPolicy> Pool;
Pool g_pool;
}  // namespace

extern "C" void fg_pool_release(void) { g_pool.release_all(); }
// plan_internal.h: before a synchronised stream that plans ran on is destroyed; and the events the pool holds (tests)
void fg_pool_retire_stream(void *stream) { g_pool.retire((hipStream_t)stream); }
extern "C" long fg_pool_live_events(void) { return g_pool.live_events(); }

// Device memory for C callers that do not include the HIP headers (the fregrid replacement objects, integration/): blocks come
// from the plans' caching pool; copies are synchronous.
extern "C" void *fg_dev_alloc(size_t bytes, int device)
{
  if (hipSetDevice(device) != hipSuccess) { fg_fail(FG_ERR_HIP, "fg_dev_alloc: no such HIP device %d", device); return nullptr; }
  void *p = g_pool.get(device, bytes);
  if (!p) fg_fail(FG_ERR_HIP, "fg_dev_alloc: out of device memory (%zu bytes)", bytes);
  return p;
}
extern "C" void fg_dev_free(void *p) { g_pool.put(p); }
extern "C" int fg_dev_upload(void *dst_dev, const void *src_host, size_t bytes)
{
  if (bytes && (!dst_dev || !src_host)) return fg_fail(FG_ERR_ARG, "fg_dev_upload: null pointer");
  if (bytes) FGCHK(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
  return 0;
}
extern "C" int fg_dev_download(void *dst_host, const void *src_dev, size_t bytes)
{
  if (bytes && (!dst_host || !src_dev)) return fg_fail(FG_ERR_ARG, "fg_dev_download: null pointer");
  if (bytes) FGCHK(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
  return 0;
}
// dst_dev[i] = src_dev[idx_dev[i]] / dst_dev[idx_dev[i]] = src_dev[i], i < n: moving a short list of source cells in and out of the
// [3][ncells] sum arrays (integration/conserve_interp_hip.c hands the shared cells' running sums from rank to rank with them)
__global__ __launch_bounds__(256) void k_gather_f64(long n, double *dst, const double *src, const int *idx, int scatter)
{
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (scatter) dst[idx[i]] = src[i]; else dst[i] = src[idx[i]];
}
static int dev_gather(double *dst_dev, const double *src_dev, const int *idx_dev, long n, int scatter)
{
  if (n < 0 || (n > 0 && (!dst_dev || !src_dev || !idx_dev))) return fg_fail(FG_ERR_ARG, "fg_dev_gather_f64 / fg_dev_scatter_f64: bad argument");
  if (n == 0) return 0;
  k_gather_f64<<<(unsigned)((n + 255) / 256), 256>>>(n, dst_dev, src_dev, idx_dev, scatter);
  FGCHK(hipGetLastError());
  FGCHK(hipDeviceSynchronize());
  return 0;
}
extern "C" int fg_dev_gather_f64(double *dst_dev, const double *src_dev, const int *idx_dev, long n) { return dev_gather(dst_dev, src_dev, idx_dev, n, 0); }
extern "C" int fg_dev_scatter_f64(double *dst_dev, const double *src_dev, const int *idx_dev, long n) { return dev_gather(dst_dev, src_dev, idx_dev, n, 1); }

// ----------------------------------------------------------------------------- host <-> device transfers of large arrays
// The host-pointer entry points (B1: create_xgrid_*, B2: fg_plan_create / fg_plan_get_xgrid) move corner arrays up and 166 MB of
// exchange cells (C384 -> 0.25 deg) down, to and from the caller's PAGEABLE memory (the reference's malloc'ed Interp_config
// arrays).  A plain hipMemcpy does that at ~14 GB/s -- one thread staging through a bounce buffer and taking the page faults of
// freshly allocated destination arrays -- which was 12 of the 14 ms of the whole call.  XferPool splits a batch of copies into
// 2 MB chunks taken by a few persistent worker threads; each has a stream and two page-locked slots, so that the DMA of one chunk
// runs beside the host memcpy (and page faults) of another and the workers add up to the link's rate.
#include <atomic>
#include <condition_variable>
#include <thread>
namespace {
struct XferJob { void *host; void *dev; size_t bytes; bool d2h; };
class XferPool {
  const size_t CHUNK = [] { const char *e = getenv("FREGRID_HIP_XFER_CHUNK_MB"); const int m = e ? atoi(e) : 0; return (size_t)(m > 0 && m <= 64 ? m : 2) << 20; }();   // 2 MB x 8 workers measured best (scripts/pcie_time.py)
  std::mutex batch_mu;                        // one batch at a time
  std::mutex mu; std::condition_variable cv_work, cv_done;
  std::vector<std::thread> threads;
  const std::vector<XferJob> *jobs = nullptr;
  std::vector<std::pair<int, size_t>> chunks; // (job, offset)
  std::atomic<size_t> next{0};
  std::atomic<int> failed{0};
  int device = 0, active = 0;
  unsigned long long gen = 0;
  struct Slot { void *pin = nullptr; hipEvent_t ev = nullptr; int pending = 0; void *host = nullptr; size_t bytes = 0; };   // pending: 1 h2d, 2 d2h
  struct Worker { int dev = -1; hipStream_t st = nullptr; Slot slot[2]; };

  bool retire(Slot &sl)
  {
    if (!sl.pending) return true;
    const bool ok = hipEventSynchronize(sl.ev) == hipSuccess;
    if (ok && sl.pending == 2) memcpy(sl.host, sl.pin, sl.bytes);
    sl.pending = 0;
    return ok;
  }
  bool prepare(Worker &w)
  {
    if (w.dev == device && w.st) return true;
    if (hipSetDevice(device) != hipSuccess) return false;
    if (w.st) {                                            // another device than last time: start over
      for (Slot &sl : w.slot) { if (sl.pin) (void)hipHostFree(sl.pin); if (sl.ev) (void)hipEventDestroy(sl.ev); sl = Slot{}; }
      (void)hipStreamDestroy(w.st); w.st = nullptr;
    }
    if (hipStreamCreateWithFlags(&w.st, hipStreamNonBlocking) != hipSuccess) return false;
    for (Slot &sl : w.slot)
      if (hipHostMalloc(&sl.pin, CHUNK, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) != hipSuccess) return false;
    w.dev = device;
    return true;
  }
  void work(Worker &w)
  {
    bool ok = prepare(w);
    int s = 0;
    for (;;) {
      const size_t c = next.fetch_add(1);
      if (c >= chunks.size() || !ok) break;
      const XferJob &j = (*jobs)[chunks[c].first];
      const size_t off = chunks[c].second, n = std::min(CHUNK, j.bytes - off);
      Slot &sl = w.slot[s]; s ^= 1;
      ok = retire(sl);
      if (!ok) break;
      if (j.d2h) {
        ok = hipMemcpyAsync(sl.pin, (const char *)j.dev + off, n, hipMemcpyDeviceToHost, w.st) == hipSuccess && hipEventRecord(sl.ev, w.st) == hipSuccess;
        sl.pending = 2; sl.host = (char *)j.host + off; sl.bytes = n;
      } else {
        memcpy(sl.pin, (const char *)j.host + off, n);
        ok = hipMemcpyAsync((char *)j.dev + off, sl.pin, n, hipMemcpyHostToDevice, w.st) == hipSuccess && hipEventRecord(sl.ev, w.st) == hipSuccess;
        sl.pending = 1;
      }
    }
    for (Slot &sl : w.slot) ok = retire(sl) && ok;
    if (!ok) { (void)hipGetLastError(); failed.store(1); }
  }
  void loop()
  {
    Worker w;
    unsigned long long seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_work.wait(lk, [&] { return gen != seen; });
        seen = gen;
      }
      work(w);
      std::lock_guard<std::mutex> lk(mu);
      if (--active == 0) cv_done.notify_all();
    }
  }

 public:
  // false: a copy failed (the caller reports it)
  bool run(int dev, const std::vector<XferJob> &batch)
  {
    size_t total = 0;
    for (const XferJob &j : batch) total += j.bytes;
    if (total == 0) return true;
    static const int nthreads = [] {
      const char *e = getenv("FREGRID_HIP_XFER_THREADS");
      int n = e ? atoi(e) : 0;
      if (n <= 0) { const unsigned hc = std::thread::hardware_concurrency(); n = hc >= 16 ? 8 : (hc >= 8 ? 4 : 2); }
      return std::min(n, 16);
    }();
    if (total < 2 * CHUNK) {                               // small: not worth waking anybody
      if (hipSetDevice(dev) != hipSuccess) return false;
      for (const XferJob &j : batch)
        if (j.bytes && hipMemcpy(j.d2h ? j.host : j.dev, j.d2h ? j.dev : j.host, j.bytes, j.d2h ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice) != hipSuccess) return false;
      return true;
    }
    std::lock_guard<std::mutex> bl(batch_mu);
    {
      std::lock_guard<std::mutex> lk(mu);
      if (threads.empty())
        for (int t = 0; t < nthreads; t++) { threads.emplace_back([this] { loop(); }); threads.back().detach(); }
      jobs = &batch; chunks.clear();
      for (size_t k = 0; k < batch.size(); k++)
        for (size_t off = 0; off < batch[k].bytes; off += CHUNK) chunks.push_back({(int)k, off});
      next.store(0); failed.store(0); device = dev; active = (int)threads.size(); gen++;
    }
    cv_work.notify_all();
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return active == 0; });
    jobs = nullptr;
    return failed.load() == 0;
  }
};
XferPool &xfer_pool() { static XferPool *p = new XferPool(); return *p; }     // (never destroyed: its threads outlive main's statics)
}  // namespace

// ----------------------------------------------------------------------------- phase timing
// Optional HIP-event timing of the phases of a search / sweep, recorded on the plan's own
// stream (bench.py reads these for the roofline object; torch.cuda.Event would only see
// PyTorch's current stream).
static int g_profiling = 0;
extern "C" void fg_set_profiling(int on) { g_profiling = on ? 1 : 0; }
enum { PH_CELL_STRUCT = 0, PH_BINS, PH_CANDIDATES, PH_CLIP_QUAD, PH_CLIP_GENERAL, PH_COMPACT, PH_ROWS,
       PH_SEARCH_TOTAL, PH_FINALIZE, PH_APPLY, PH_COUNT };

struct PhaseTimer {
  bool on = false;
  hipStream_t st = nullptr;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> spans;
  hipEvent_t open_ev = nullptr; int open_ph = -1;
  void start(bool enable, hipStream_t s) { on = enable; st = s; }
  void begin(int ph)
  {
    if (!on) return;
    open_ev = g_handles.get_event(); (void)hipEventRecord(open_ev, st); open_ph = ph;
  }
  void end()
  {
    if (!on || open_ph < 0) return;
    hipEvent_t e = g_handles.get_event(); (void)hipEventRecord(e, st);
    spans.push_back({open_ph, {open_ev, e}}); open_ph = -1;
  }
  // call after the stream has been synchronised; accumulates into ms[]
  void collect(float *ms)
  {
    for (auto &sp : spans) {
      float t = 0; (void)hipEventElapsedTime(&t, sp.second.first, sp.second.second);
      ms[sp.first] += t;
      g_handles.put_event(sp.second.first); g_handles.put_event(sp.second.second);
    }
    spans.clear();
  }
};

// ----------------------------------------------------------------------------- plan
struct fg_plan {
  float phase_ms[PH_COUNT] = {0};
  PhaseTimer apply_pt;
  int apply_spans = 0;
  int order = 0, device = 0;
  bool great_circle = false;   // exchange cells from create_xgrid_great_circle semantics (order 1 only)
  hipStream_t stream = nullptr;
  hipStream_t stream_b = nullptr;   // second stream of the three-pass great-circle clip (always ours)
  bool own_stream = true;
  int ntiles = 0;
  std::vector<int> nx_in, ny_in, cell_off;
  std::vector<FgTile> tiles_host;   // staging for the async descriptor upload
  int nsrc = 0;                 // flattened source cells
  int nx_out = 0, ny_out = 0, ndst = 0;
  long f_stride = 0;            // elements in one level of the source field array
  bool searched = false, finalized = false, have_geom = false;
  bool fused = false;            // finalized by its own search (fg_set_search_finalize): centroids from the plan's own per-cell sums

  std::vector<void *> owned;    // every pool block of this plan
  FgTile *tiles_dev = nullptr;
  double *mask_dev = nullptr;
  FgCells S{}, D{};
  bool rect = false;            // searched on the rectilinear path: D holds areas only, the cells are in rect_tab (FgRect)
  FgRect rect_tab{};
  FgPolyList polys{};           // npoly > 0: the source "cells" are this list of polygons (fg_plan_create_polylist)
  FgGcPolyList gcpolys{};       // npoly > 0: ... this list of great-circle polygons (fg_plan_create_polylist_gc)
  double *gc_prec = nullptr;    // their records, [npoly][FG_GC_PREC] (k_gc_poly_records)
  // exchange cells
  long nx = 0;
  int *x_src = nullptr, *x_dst = nullptr;
  double *x_area = nullptr, *x_c1 = nullptr, *x_c2 = nullptr;
  int *xoff = nullptr;
  FgRowEnt *perm = nullptr;      // {exchange cell, its source cell} grouped by destination row (unsorted inside a row) until fg_plan_finalize
  bool rows_built = false;       // csr.row_ptr and perm come from the search
  bool dist_pending = false;     // order 2: x_c1/x_c2 still hold the centroid integrals after finalize (fg_plan_get_xgrid applies di/dj)
  double *sums = nullptr;
  FgSrcRec *cen = nullptr;       // order 2, from the finalize on: the centroid of every source cell
  // sweep
  FgCsr csr{};
  int *src_idx_f = nullptr;
  double *row_sum = nullptr, *red_partial = nullptr, *red_result = nullptr;
  long row_sum_cap = 0;
  double *il_f = nullptr, *il_out = nullptr, *il_rs = nullptr;   // [cell][8] scratch (order 1 field, output, row sums)
  double *il_m = nullptr;                                        // order 2: merged records [source cell][3][8] (k_merge3)
  unsigned char *lv_bits = nullptr;                              // order 2, fg_plan_apply_levels: gradient-mask bits per source cell
  double *lx_fa = nullptr;                                       // fg_plan_apply_levels_ex: a chunk's per-level field_area [source cell][8]
  long stats[FG_NSTATS] = {0};
  long search_d2h = 0;           // bytes the search read back: one counter block per attempt
  // monotone limiter scratch (fg_plan_mono_*): limited values per CSR entry, per-source-cell bounds, error word
  double *mono_x = nullptr, *mono_b = nullptr;     // mono_b: [4][nsrc] = f_bar_max | f_bar_min | f_max | f_min
  int *xerr = nullptr;
  bool mono_open = false;
  // the limiter on eight levels (fg_plan_mono_levels_*): one chunk's bounds [nsrc][4][8] = f_bar_max | f_bar_min | f_max | f_min
  double *mono8_b = nullptr;
  int mono8_nz = 0;              // levels of the open chunk, 0 = none open
  // ... on the gradient object's records (fg_plan_mono_records_*): the open chunk's bounds are the CALLER's buffer
  double *mono8r_b = nullptr;
  int mono8r_nz = 0;
  unsigned *ll_err = nullptr;    // error word of a latlon2xyz conversion queued ahead of the search (great-circle plans from lon / lat)

  // Stream-ordered plans (fg_set_search_async).
  // async: the plan's search ran with the switch on; its blocks go back to the pool tagged with its stream, and fg_plan_destroy
  //   does not drain the stream.
  // on_stream: set while plan_search / the finalize allocate -- every block taken then is first touched by work queued on `stream`
  //   (or on stream_b behind an event of `stream`), so the pool may hand out one that earlier work of the stream still uses.
  //   Everywhere else alloc() takes blocks nothing uses: host copies and the transfer pool's streams write into them.
  // INVARIANT -- when a fused search (or a finalize on a caller's stream) has returned, everything in the plan is complete
  //   except `cen` and the CSR records (csr.e1 / csr.e2); those two are complete in stream order on `stream`.  Whoever reads them
  //   from the host or from another stream, or moves the plan to another stream, synchronises `stream` first -- every entry that
  //   does either did so before this invariant existed and still does; entries that only queue work on `stream` need not.
  bool async = false, on_stream = false;

  template <typename T> T *alloc(size_t count)
  {
    void *p = on_stream ? g_pool.get(device, count * sizeof(T), stream) : g_pool.get(device, count * sizeof(T));
    if (p) owned.push_back(p);
    return (T *)p;
  }
  void disown(void *p) { for (size_t k = 0; k < owned.size(); k++) if (owned[k] == p) { owned.erase(owned.begin() + k); break; } }
  void release(void *p)
  {
    if (!p) return;
    disown(p);
    g_pool.put(p);
  }
  // blocks that work queued on the plan's stream may still be using: one batch of the pool, left without an event of its own
  // (the plan vouches for its stream; fg_plan_destroy or a change of stream seals the batch)
  void release_on_stream(const std::vector<void *> &ps)
  {
    for (void *p : ps) disown(p);
    g_pool.put(ps, stream, false);
  }
  // Before a search is repeated (plan_search): every block beyond the first `keep` -- those the caller staged -- goes back to the
  // pool, and so must every pointer into them.  A field that plan_search_core allocates or sets is added HERE as well.
  void drop_search(size_t keep)
  {
    while (owned.size() > keep) { g_pool.put(owned.back()); owned.pop_back(); }
    tiles_dev = nullptr; mask_dev = nullptr; S = FgCells{}; D = FgCells{};
    x_src = x_dst = nullptr; x_area = x_c1 = x_c2 = nullptr; xoff = nullptr;
    perm = nullptr; csr.row_ptr = nullptr; csr.e1 = nullptr; csr.e2 = nullptr; cen = nullptr; src_idx_f = nullptr; sums = nullptr; gc_prec = nullptr;
    have_geom = false; rect = false; rect_tab = FgRect{};
  }
};

// Slots of the side table of compact source cells (FgCells, xgrid_device.h): cells that fix_lon leaves with more than four
// vertices.  A cubed sphere has eight, a lat-lon grid none; a search that meets more than the table holds is repeated on the
// generic path.  fg_set_search_wide_cap(n >= 0) lowers the capacity to n (tests of that route), n < 0 = the default.
static int g_wide_cap = -1;
extern "C" void fg_set_search_wide_cap(int n) { g_wide_cap = n < 0 ? -1 : n; }
static bool alloc_cells(fg_plan *pl, FgCells *c, size_t n, bool compact = false)
{
  *c = FgCells{};
  c->lat_min = pl->alloc<double>(n); c->lat_max = pl->alloc<double>(n);
  if (!compact) { c->lon_min = pl->alloc<double>(n); c->lon_max = pl->alloc<double>(n); }
  c->lon_avg = pl->alloc<double>(n); c->area = pl->alloc<double>(n);
  c->nv = pl->alloc<int>(n);
  c->verts = pl->alloc<double>(n * (compact ? FG_VSTRIDE_QUAD : 16));
  if (compact) {
    const size_t cap = n / 16 + 64;
    c->vstride = FG_VSTRIDE_QUAD;
    c->wide_cap = (int)(g_wide_cap >= 0 ? std::min<size_t>((size_t)g_wide_cap, cap) : cap);
    c->wide = pl->alloc<double>(16 * (size_t)std::max(c->wide_cap, 1));
    if (!c->wide) return false;
  }
  return c->lat_min && c->lat_max && (compact || (c->lon_min && c->lon_max)) && c->lon_avg && c->area && c->nv && c->verts;
}

static int plan_base(int order, int ntiles_in, const int *nx_in, const int *ny_in, int nx_out, int ny_out,
                     int device, fg_plan **out)
{
  if (order != FG_CONSERVE_ORDER1 && order != FG_CONSERVE_ORDER2) return fg_fail(FG_ERR_ARG, "order must be 1 or 2");
  if (ntiles_in < 1 || !nx_in || !ny_in || nx_out < 1 || ny_out < 1 || !out) return fg_fail(FG_ERR_ARG, "bad grid sizes");
  if (int rc = fg_use_device("fg_plan", device)) return rc;
  fg_plan *pl = new fg_plan();
  pl->order = order; pl->device = device; pl->ntiles = ntiles_in;
  long off = 0, foff = 0;
  for (int m = 0; m < ntiles_in; m++) {
    if (nx_in[m] < 1 || ny_in[m] < 1) { delete pl; return fg_fail(FG_ERR_ARG, "bad source tile size"); }
    pl->nx_in.push_back(nx_in[m]); pl->ny_in.push_back(ny_in[m]); pl->cell_off.push_back((int)off);
    off += (long)nx_in[m] * ny_in[m];
    foff += (order == 2) ? (long)(nx_in[m] + 2) * (ny_in[m] + 2) : (long)nx_in[m] * ny_in[m];
  }
  if (off > 2000000000L || (long)nx_out * ny_out > 2000000000L) { delete pl; return fg_fail(FG_ERR_ARG, "grid too large for 32-bit cell indices"); }
  pl->nsrc = (int)off; pl->f_stride = foff;
  pl->nx_out = nx_out; pl->ny_out = ny_out; pl->ndst = nx_out * ny_out;
  pl->stream = g_handles.get_stream(device);
  if (!pl->stream) { delete pl; return fg_fail(FG_ERR_HIP, "hipStreamCreate failed"); }
  *out = pl;
  return 0;
}

// A plan whose search ran stream-ordered (fg_plan::async) does not drain its stream here: its blocks go back to the pool tagged
// with the stream, in one batch, and its streams to the cache as they are (whoever gets them next queues behind what is left).
// What may still be queued reads plan-owned memory only -- k_centroids and k_csr_sortgather read S, sums, cen, perm, the
// exchange cells, src_idx_f and their scratch, never the caller's corner arrays, which nothing behind the search's readback
// touches -- and later work of the caller (an apply) is ordered on the caller's stream like the caller's own buffers.
// On a caller's stream the batch is sealed here: one event, recorded now, also for what the search and the finalize gave back
// earlier, so that the pool never touches the stream after this call and the caller may destroy it.  A plan-owned stream goes
// back to the cache, which never destroys one: its batch gets an event only if a taker on another stream needs it.
// stream_b is idle whenever a search has returned: only the great-circle clip uses it, and joins it into `stream` ahead of the
// readback.
extern "C" void fg_plan_destroy(fg_plan *pl)
{
  if (!pl) return;
  (void)hipSetDevice(pl->device);
  const bool drain = !pl->async || !pl->apply_pt.spans.empty();      // (timing events of sweeps are read after a synchronisation)
  if (drain && (pl->stream || !pl->own_stream)) (void)hipStreamSynchronize(pl->stream);
  if (pl->stream_b) { if (drain) (void)hipStreamSynchronize(pl->stream_b); g_handles.put_stream(pl->device, pl->stream_b); }
  { float junk[PH_COUNT] = {0}; pl->apply_pt.collect(junk); }
  if (pl->async) g_pool.put(pl->owned, pl->stream, !pl->own_stream);
  else for (void *p : pl->owned) g_pool.put(p);
  if (pl->stream && pl->own_stream) g_handles.put_stream(pl->device, pl->stream);
  delete pl;
}

static void choose_bins(const fg_plan *pl, double mean_dlat, double mean_dlon, FgBins *b)
{
  const double PI = 3.14159265358979323846;
  // a typical cell covers at most 2x2 bins.  Measured on C384 -> 0.25 deg: factors 1.1 / 1.25 / 1.5 / 2.0 give 0.247 / 0.257 /
  // 0.271 / 0.334 ms for the candidate phase (fewer records per scanned bin); 1.25 keeps a margin for cells larger than the mean
  double h = 1.25 * mean_dlat, w = 1.25 * mean_dlon;
  int nblat = (h > 0) ? (int)ceil(PI / h) : 1;
  int nblon = (w > 0) ? (int)ceil(2.0 * PI / w) : 1;
  if (nblat < 1) nblat = 1; if (nblat > 8192) nblat = 8192;
  if (nblon < 1) nblon = 1; if (nblon > 16384) nblon = 16384;
  (void)pl;
  b->nblat = nblat; b->nblon = nblon;
  b->inv_wlat = nblat / PI;
  b->inv_wlon = nblon / (2.0 * PI);
}

// Device-side counters of one search (FgCounters, xgrid_device.h): one block, zeroed by the search's one memset, read back with
// one copy into pinned host memory when the search has been queued.
// Behind the counters, in the same page-locked block, one 64-bit word: the arrival mark of a stream-ordered search, which its
// counter kernel stores after the counters and the host polls (k_counters_out).
struct PinnedCounters { FgCounters c; unsigned long long mark; };
static FgCounters *pinned_counters()
{
  static thread_local PinnedCounters *h = nullptr;
  if (!h) { if (hipHostMalloc((void **)&h, sizeof(PinnedCounters), hipHostMallocCoherent) != hipSuccess) h = nullptr; else h->mark = 0; }
  return h ? &h->c : nullptr;
}

// the search proper; all grid pointers are device pointers
// Great-circle plans pass the corner unit vectors instead (gc_in[m] = {x, y, z} device pointers of source tile m,
// gc_out likewise); d_lon/d_lat are then unused.
struct GcXyz { const double *x, *y, *z; };
// 1-D x 2-D variants: the "source" tile of the search is the box grid expanded to corner arrays (d_lon_in[0]/d_lat_in[0]),
// the "destination" the quads; box holds the 1-D bounds the pair kernel clips against.
struct BoxMode { FgBox box; const double *mask_quad; int no_adjust; };
// What one search works on; every pointer is a device pointer, and a caller names the fields it has.  A legacy search takes
// lon_in / lat_in [ntiles] and lon_out / lat_out, a great-circle search gc_in [ntiles] and gc_out instead.  mask_in: null, or
// [ntiles] with null entries for unmasked tiles.  mean_dlat / mean_dlon size the bins (choose_bins).  rect_hint 0: the caller has
// seen that the destination is not rectilinear, so no attempt is spent on finding that out.
struct SearchIn {
  const double *const *lon_in = nullptr, *const *lat_in = nullptr, *const *mask_in = nullptr;
  const double *lon_out = nullptr, *lat_out = nullptr;
  const GcXyz *gc_in = nullptr, *gc_out = nullptr;
  const BoxMode *boxm = nullptr;
  double mean_dlat = 0, mean_dlon = 0;
  int rect_hint = 1;
};
// What steers a search: the values of the process-wide setters (fg_set_search_*, fg_set_gc_split, fg_set_profiling) as
// plan_search found them when the plan-creating call started.  Every attempt of that search gets the same ones.
struct SearchOpts { bool exact, cull, finalize, rect, dst_frame; int gc_split; bool profile, async; };
// The counter block of a fused, stream-ordered search into the page-locked host block: one wave, queued behind the compaction
// (the last kernel that writes a counter), so that the host has the counters while the centroid pass and the CSR records still
// run.  Plain stores, 4 bytes a lane and round; then, when every lane's stores are out, the arrival mark the host polls for.
__global__ __launch_bounds__(64) void k_counters_out(const unsigned *src, unsigned *dst, int nwords, unsigned long long *mark, unsigned long long seq)
{
  for (int k = threadIdx.x; k < nwords; k += 64) dst[k] = src[k];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(mark, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
static_assert(sizeof(FgCounters) % sizeof(unsigned) == 0 && offsetof(PinnedCounters, mark) == sizeof(FgCounters), "FgCounters travels as 32-bit words, the mark behind them");
// The host side: polls the mark, looking at the stream now and then so that a failed launch or a fault ends the wait.
static hipError_t wait_counters(const FgCounters *hc, unsigned long long seq, hipStream_t st)
{
  const unsigned long long *mark = &((const PinnedCounters *)hc)->mark;
  for (unsigned spin = 1;; spin++) {
    if (__atomic_load_n(mark, __ATOMIC_ACQUIRE) == seq) return hipSuccess;
    __builtin_ia32_pause();
    if (spin % 65536 == 0) {
      const hipError_t e = hipStreamQuery(st);
      if (e == hipErrorNotReady) (void)hipGetLastError();       // (not an error; the caller has checked the launches already)
      if (e == hipSuccess) return __atomic_load_n(mark, __ATOMIC_ACQUIRE) == seq ? hipSuccess : hipErrorUnknown;   // drained: it is there, or never will be
      if (e != hipErrorNotReady) return e;
    }
  }
}
static const char *gc_clip_error(int code)
{
  switch (code) {
    case 3: return "firstIntersect is not in the grid1List";
    case 4: return " not found the next intersection ";
    case 5: return "not return back to the first intersection";
    case 6: return "After clipping, nintersect should be 0";
    case 7: return "inserAfter: point (x,y,z) is not found in the list";
    case 8: return "Error from create_xgrid.c: temp is not in list1";
    // the device's own (GC_ENDLESS, gc_kernels.hip): the reference does not end on such a pair and has no message for it
    case 11: return "clip_2dx2d_great_circle: insertIntersect finds no node that is not an intersection (the reference's loop over "
                    "the list, mosaic_util.c:1352, does not end on this pair of cells)";
    // 9, the device's own as well: its node lists hold what two convex polygons can produce (gc_kernels.hip: GC_NCAP, GC_ICAP,
    // GC_PCAP), the reference's pool holds more (MAXNODELIST, mosaic_util.c:1046)
    default: return "clip_2dx2d_great_circle: more intersections than two convex polygons can have (the list capacity of the device "
                    "clip, not a check of the reference)";
  }
}

// Capacities of one attempt: bin-table records and entries per region of the pair list.  The default capacities (bin records
// 3*ndst, pairs 8*max(nsrc, ndst)) fit every remap between grids of comparable resolution; every kernel clamps its writes
// AND reads to them, the counters keep counting, and an attempt that outgrew one is repeated with the counted sizes.
static int g_search_cull = 0;
static int g_search_finalize = 0;     // fg_set_search_finalize: a search that can also queues the finalize work before its one synchronisation
// great-circle clip: 1 = three passes (k_gc_screen / k_gc_solve / k_gc_walk) with the one-kernel clip for the unusual pairs,
// 0 = the one-kernel clip for every pair (fg_set_gc_split; the tests compare the two)
static int g_gc_split = 1;
extern "C" void fg_set_gc_split(int on) { g_gc_split = on < 0 ? 0 : on; }      // 2: a task space 64 times too small (tests of the overflow path)
struct SearchCaps { unsigned long long entries; int regcap, nreg; bool rect; };
// Rectilinear destination grids (k_rect_tables, xgrid_kernels.hip): 1 = try the index-arithmetic path first and verify the grid on
// the device in the same stream (default), 0 = always the generic bins path.  A target that fails the check costs the attempt's
// launches (every kernel leaves at once) and one more synchronisation, ~0.1 ms; callers with host arrays are spared even that by
// a look at a few corners (host_says_not_rect).
static int g_search_rect = 1;
extern "C" void fg_set_search_rect(int on) { g_search_rect = on ? 1 : 0; }
// Longitude frame of the DESTINATION cells of a legacy search.  0 (default) = create_xgrid's: fix_lon(cell, pi), then per pair a
// shift of +-2pi towards the source cell's mean longitude (create_xgrid.c:1004,1062-1079).  1 = make_coupler_mosaic's: the cell is
// only unwrapped and then moved ONCE per pair, fix_lon(cell, mean longitude of the other cell) (make_coupler_mosaic.c:1452,1598).
// The two agree unless the first recentring moved the cell and the second moved it back -- (x + 2pi) - 2pi is not x in floating
// point -- as for an ocean grid given on -280..80 degrees.  Implementation: the recentring target of the destination records is
// NaN (every comparison of fix_lon's last step is then false), the per-pair shift is the same code.
static int g_dst_frame = 0;
extern "C" void fg_set_search_frame(int coupler) { g_dst_frame = coupler ? 1 : 0; }
static thread_local int tl_dst_frame = -1;  // >= 0: the frame of the searches this thread starts, whatever fg_set_search_frame says (fg_search_frame_override)
static bool host_says_not_rect(int nx, int ny, const double *lon, const double *lat)
{
  const long nxp = nx + 1;
  const int js[3] = {ny, ny / 2, 1}, is[3] = {nx, nx / 2, 1};
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      const long e = (long)js[a] * nxp + is[b];
      if (memcmp(&lon[e], &lon[is[b]], sizeof(double)) || memcmp(&lat[e], &lat[(long)js[a] * nxp], sizeof(double))) return true;
    }
  return false;
}
#define FG_RETRY (-1000L)
// Offsets of the parts of one block, handed out in order: the one walk gives every part's place and, at its end, the block's size.
struct Carve {
  size_t n = 0;
  size_t operator()(size_t size) { const size_t at = n; n += size; return at; }
};
// Device blocks of one attempt.  keep: stays with the plan; get: scratch of the search, handed back by release().  A block that
// could not be had clears ok, which the search tests once, before its first launch.
struct SearchBlocks {
  fg_plan *pl;
  bool ok = true;
  std::vector<void *> scratch;
  template <typename T> T *keep(size_t count) { T *p = pl->alloc<T>(count); ok = ok && p; return p; }
  template <typename T> T *get(size_t count) { T *p = keep<T>(count); if (p) scratch.push_back(p); return p; }
  void release() { for (void *p : scratch) pl->release(p); scratch.clear(); }
};
static long plan_search_core(fg_plan *pl, const SearchIn &in, const SearchOpts &opt, SearchCaps *caps)
{
  // Queue order (legacy search, 11 launches + 1 readback; the host synchronises ONCE, at the end):
  //   memset | cell records + bin counts | bin scan | bin fill + heavy list | candidates | quad clip | general clip |
  //   compaction (+ big cells) | row scan | row slots -> perm | counters -> host
  // Rectilinear target (8 launches): memset | axis tables + check | source records + candidates + destination areas | candidates of
  //   the listed (heavy) cells | quad clip | general clip | the two scans | compaction | counters -> host
  //   (no launch fewer than before the record kernel made the candidates: the listed cells keep theirs, now min(2048, nsrc / 8)
  //   one-wave blocks instead of those + nsrc / 64)
  //   phase_ms: "cell_struct" covers the tables and the record kernel, candidates included; "candidates" the listed cells' launch
  const bool gc = in.gc_in != nullptr;
  const BoxMode *const boxm = in.boxm;
  pl->great_circle = gc;
  hipStream_t st = pl->stream;
  const int nsrc = pl->nsrc, ndst = pl->ndst, order = pl->order;
  FgCounters *hc = pinned_counters();
  if (!hc) return fg_fail(FG_ERR_HIP, "hipHostMalloc failed");

  // tile descriptors: source tiles + the destination tile as entry [ntiles]
  std::vector<FgTile> &th = pl->tiles_host;  // owned by the plan: an async upload needs no sync
  th.resize(pl->ntiles + 1);
  for (int m = 0; m < pl->ntiles; m++) th[m] = FgTile{gc ? nullptr : in.lon_in[m], gc ? nullptr : in.lat_in[m], pl->nx_in[m], pl->ny_in[m], pl->cell_off[m]};
  th[pl->ntiles] = FgTile{in.lon_out, in.lat_out, pl->nx_out, pl->ny_out, 0};
  pl->tiles_dev = pl->alloc<FgTile>(pl->ntiles + 1);
  if (!pl->tiles_dev) return fg_fail(FG_ERR_HIP, "out of device memory");
  FgTileSet ts; ts.n = 0;
  const bool by_value = !gc && pl->ntiles + 1 <= FG_TILESET_MAX;        // descriptors travel as a kernel argument
  if (by_value) { ts.n = pl->ntiles + 1; for (int m = 0; m <= pl->ntiles; m++) ts.t[m] = th[m]; }
  else FGCHK(hipMemcpyAsync(pl->tiles_dev, th.data(), sizeof(FgTile) * th.size(), hipMemcpyHostToDevice, st));
  FgTileXyz *gct_dev = nullptr;
  std::vector<FgTileXyz> gct;                       // must outlive the async upload: synchronised at the readback
  if (gc) {
    gct.resize(pl->ntiles + 1);
    for (int m = 0; m < pl->ntiles; m++) gct[m] = FgTileXyz{in.gc_in[m].x, in.gc_in[m].y, in.gc_in[m].z, pl->nx_in[m], pl->ny_in[m], pl->cell_off[m]};
    gct[pl->ntiles] = FgTileXyz{in.gc_out->x, in.gc_out->y, in.gc_out->z, pl->nx_out, pl->ny_out, 0};
    gct_dev = pl->alloc<FgTileXyz>(pl->ntiles + 1);
    if (!gct_dev) return fg_fail(FG_ERR_HIP, "out of device memory");
    FGCHK(hipMemcpyAsync(gct_dev, gct.data(), sizeof(FgTileXyz) * gct.size(), hipMemcpyHostToDevice, st));
  }

  bool any_mask = false;
  if (in.mask_in) for (int m = 0; m < pl->ntiles; m++) if (in.mask_in[m]) any_mask = true;
  if (any_mask) {
    pl->mask_dev = pl->alloc<double>(nsrc);
    if (!pl->mask_dev) return fg_fail(FG_ERR_HIP, "out of device memory");
    std::vector<double> ones;
    for (int m = 0; m < pl->ntiles; m++) {
      size_t nc = (size_t)pl->nx_in[m] * pl->ny_in[m];
      if (in.mask_in[m]) FGCHK(hipMemcpyAsync(pl->mask_dev + pl->cell_off[m], in.mask_in[m], nc * sizeof(double), hipMemcpyDeviceToDevice, st));
      else {
        ones.assign(nc, 1.0);
        FGCHK(hipMemcpyAsync(pl->mask_dev + pl->cell_off[m], ones.data(), nc * sizeof(double), hipMemcpyHostToDevice, st));
        FGCHK(hipStreamSynchronize(st));
      }
    }
  }

  // --- sizes known up front
  const bool rect = caps->rect && !gc && !boxm;
  pl->rect = rect;
  const double dst_tlon = opt.dst_frame ? (double)NAN : 3.14159265358979323846;
  FgBins bins;
  choose_bins(pl, in.mean_dlat, in.mean_dlon, &bins);
  if (rect) { bins.nblat = 0; bins.nblon = 0; }       // no bins on the rectilinear path
  const long nbins = (long)bins.nblat * bins.nblon;
  const long nslots = nbins + bins.nblat;             // regular bins + one wide list per bin row
  const unsigned long long nentries = rect ? 0ull : caps->entries;
  const int ecap = (int)std::min<unsigned long long>(nentries, 2147483647ull);     // records the buffer holds: writes and reads stop there
  FgPairSpace ps{};
  ps.nreg = caps->nreg; ps.regcap = caps->regcap;
  const long npairs = fgd_pairs_total(ps);            // capacity of the pair list
  const long nx_alloc = npairs;                       // nxgrid <= candidate pairs <= capacity

  // (a grid on the rectilinear path: compact source cells, written by k_cell_struct2r and k_candidates_rect<true>)
  if (!alloc_cells(pl, &pl->S, nsrc, rect && !pl->polys.npoly)) return fg_fail(FG_ERR_HIP, "out of device memory");
  SearchBlocks blk{pl};
  const bool gc_poly = gc && pl->gcpolys.npoly > 0;   // great-circle polygon list: records of its own, the general clip for every pair
  if (gc_poly) pl->gc_prec = blk.keep<double>((size_t)nsrc * FG_GC_PREC);
  struct { double *hdr, *lat_ax, *lon_ax, *col, *row, *col_min, *col_max, *col_avg; } rt{};   // the rectilinear tables, one block (FgRect, xgrid_device.h)
  if (rect) {
    pl->D = FgCells{};
    pl->D.area = blk.keep<double>(ndst);
    Carve at;                                         // (in doubles)
    const size_t o_hdr = at(8), o_lat = at((size_t)pl->ny_out + 1), o_lon = at((size_t)pl->nx_out + 1), o_col = at(8 * (size_t)pl->nx_out),
                 o_row = at(4 * ((size_t)pl->ny_out + 1)), o_cmin = at((size_t)pl->nx_out), o_cmax = at((size_t)pl->nx_out), o_cavg = at((size_t)pl->nx_out);
    double *rect_blk = blk.keep<double>(at.n);
    if (!blk.ok) return fg_fail(FG_ERR_HIP, "out of device memory");
    rt = {rect_blk + o_hdr, rect_blk + o_lat, rect_blk + o_lon, rect_blk + o_col, rect_blk + o_row, rect_blk + o_cmin, rect_blk + o_cmax, rect_blk + o_cavg};
  } else if (!alloc_cells(pl, &pl->D, ndst)) return fg_fail(FG_ERR_HIP, "out of device memory");
  // one zeroed block: [counters | region fill counters | tickets | look-back words of the three scans | bin counts |
  //                    bin fill cursors | destination-row counts | accepted pairs per source cell | great-circle task counters]
  const long t_bins = fgd_scan_tiles(nslots), t_rows = fgd_scan_tiles(ndst), t_comp = fgd_scan_tiles(nsrc);
  const size_t zreg = (size_t)FG_NREG * FG_FILL_STRIDE * sizeof(unsigned);        // a counter per region (nreg <= FG_NREG)
  Carve z;
  const size_t z_dc = z((sizeof(FgCounters) + 127) / 128 * 128), z_fill = z(zreg), z_tick = z(128);
  const size_t z_lb_bins = z(t_bins * sizeof(unsigned long long)), z_lb_rows = z(t_rows * sizeof(unsigned long long)),
               z_lb_comp = z(t_comp * sizeof(unsigned long long));
  const size_t z_bin_cnt = z((size_t)(nslots + 1) * sizeof(int)), z_bin_fill = z((size_t)(nslots + 1) * sizeof(int)),
               z_row_cnt = z((size_t)(ndst + 1) * sizeof(int)), z_nacc = z((size_t)(nsrc + 1) * sizeof(int));
  z((16 - (z.n - z_bin_cnt) % 16) % 16);              // (the four int arrays together are rounded up to 16 bytes)
  const size_t z_gc_ntask = z(gc ? zreg : 0), z_gc_ocnt = z(gc ? zreg : 0);   // great-circle clip: task counters, then the counters of the walk's pair lists
  const size_t zbytes = z.n;
  char *zero_blk = blk.get<char>(zbytes);
  int *bin_start = blk.get<int>(nslots + 1);
  int *heavy_list = blk.get<int>(nsrc + 1);
  int *rare_list = blk.get<int>(rect ? nsrc + 1 : 1);  // rectilinear path: the cells k_candidates_rect finishes (laid out like heavy_list)
  int *big_list = blk.get<int>(nsrc + 1);
  int *pair_beg = blk.get<int>(nsrc + 1), *pair_cnt = blk.get<int>(nsrc + 1);
  FgBinEntry *bin_entries = blk.get<FgBinEntry>(nentries ? nentries : 1);
  ps.src = blk.get<int>(npairs + 1); ps.dst = blk.get<int>(npairs + 1);
  double *tmp_area = blk.get<double>(npairs + 1);
  double *tmp_clon = (order == 2) ? blk.get<double>(npairs + 1) : nullptr;
  double *tmp_clat = (order == 2) ? blk.get<double>(npairs + 1) : nullptr;
  int *defer_list = blk.get<int>(npairs + 1);
  // legacy clip: the clip kernels take the destination-row slots, the row scan runs before the compaction and the compaction
  // stores the row lists itself (no k_csr_fill_pos, no returning atomics in the compaction)
  const bool early_rows = !gc && !boxm;
  int *tmp_rowpos = early_rows ? blk.get<int>(npairs + 1) : nullptr;
  // great-circle path, three-pass clip: per-pair words, and 3 tasks (edge pairs to solve) per pair of capacity -- 3.0 per LIVE
  // pair were counted at C384 -> 0.25 deg; pairs whose tasks do not fit go through the one-kernel clip instead
  const bool gc_split = gc && !gc_poly && opt.gc_split && npairs < (1L << 28);
  const long tcap_want = (opt.gc_split == 2) ? npairs / 64 : 3 * npairs;
  const long tcap_reg = gc_split ? std::min<long>((tcap_want / FG_NREG + 255) / 256 * 256, 0x7ffffff0L / FG_NREG) : 0;   // tasks per region
  const long tcap_all = tcap_reg * FG_NREG;
  unsigned *gc_meta = gc_split ? blk.get<unsigned>(npairs + 1) : nullptr;
  int *gc_tbase = gc_split ? blk.get<int>(npairs + 1) : nullptr;
  int *gc_order = gc_split ? blk.get<int>(npairs + 1) : nullptr;
  unsigned *gc_task = gc_split ? blk.get<unsigned>(tcap_all + 1) : nullptr;
  double *gc_res = gc_split ? blk.get<double>(2 * (size_t)tcap_all + 2) : nullptr;
  pl->xoff = blk.keep<int>(nsrc + 1);
  pl->x_src = blk.keep<int>(nx_alloc + 1); pl->x_dst = blk.keep<int>(nx_alloc + 1);
  pl->x_area = blk.keep<double>(nx_alloc + 1);
  if (order == 2) { pl->x_c1 = blk.keep<double>(nx_alloc + 1); pl->x_c2 = blk.keep<double>(nx_alloc + 1); pl->sums = blk.keep<double>(3 * (size_t)nsrc); }
  int *x_rowpos = blk.get<int>(nx_alloc + 1);          // slot of every exchange cell in its destination row, where the compaction takes it (!early_rows)
  pl->perm = blk.keep<FgRowEnt>(nx_alloc + 1);
  pl->csr.row_ptr = blk.keep<int>(ndst + 1);
  if (!pl->src_idx_f) pl->src_idx_f = blk.keep<int>(nsrc + 1);
  if (!blk.ok) return fg_fail(FG_ERR_HIP, "out of device memory");
  FgCounters *dc = (FgCounters *)(zero_blk + z_dc);
  ps.fill = (unsigned *)(zero_blk + z_fill);
  unsigned *tickets = (unsigned *)(zero_blk + z_tick);                     // [0] bins [1] rows [2] xoff scan
  unsigned long long *lb_bins = (unsigned long long *)(zero_blk + z_lb_bins), *lb_rows = (unsigned long long *)(zero_blk + z_lb_rows),
                     *lb_comp = (unsigned long long *)(zero_blk + z_lb_comp);
  int *bin_cnt = (int *)(zero_blk + z_bin_cnt), *bin_fill = (int *)(zero_blk + z_bin_fill), *row_cnt = (int *)(zero_blk + z_row_cnt);
  int *nacc = (int *)(zero_blk + z_nacc);
  FGCHK(hipMemsetAsync(zero_blk, 0, zbytes, st));
  if (pl->ll_err) FGCHK(hipMemcpyAsync(&dc->err[2], pl->ll_err, sizeof(unsigned), hipMemcpyDeviceToDevice, st));   // rides on the one readback

  PhaseTimer pt, ptot;
  pt.start(opt.profile, st); ptot.start(opt.profile, st);
  for (int k = 0; k < PH_COUNT; k++) pl->phase_ms[k] = 0;
  ptot.begin(PH_SEARCH_TOTAL);
  pt.begin(PH_CELL_STRUCT);
  if (gc) {
    // destination cells first: a culling search (a rank's band of the target) folds their latitude ranges into band_keys, and
    // the source launch drops the cells that cannot meet that range before their (expensive) spherical-excess area
    fgd_gc_cell_struct(gct_dev + pl->ntiles, 1, ndst, pl->D, st, opt.cull ? dc->band_keys : nullptr, 1);
    if (gc_poly) fgd_gc_poly_records(pl->gcpolys, pl->S, pl->gc_prec, dc->err, st);
    else fgd_gc_cell_struct(gct_dev, pl->ntiles, nsrc, pl->S, st, opt.cull ? dc->band_keys : nullptr, 2);
    fgd_src_field_index(order, pl->tiles_dev, pl->ntiles, nsrc, pl->src_idx_f, st);
  } else if (rect) {
    // tables + on-device verification of the grid, then the source records, the heavy list and the destination AREAS in one launch
    FgRect &R = pl->rect_tab;
    R.hdr = rt.hdr; R.lat_ax = rt.lat_ax; R.lon_ax = rt.lon_ax; R.col = rt.col; R.row = rt.row;
    R.col_min = rt.col_min; R.col_max = rt.col_max; R.col_avg = rt.col_avg;
    R.bad = &dc->rect_bad; R.nx = pl->nx_out; R.ny = pl->ny_out;
    fgd_rect_tables(in.lon_out, in.lat_out, pl->nx_out, pl->ny_out, rt.hdr, rt.lat_ax, rt.lon_ax, rt.col, rt.col_min, rt.col_max, rt.col_avg, rt.row,
                    &dc->rect_bad, dc->err, st, dst_tlon);
    if (pl->polys.npoly) fgd_polylist_records(pl->polys, pl->S, pl->src_idx_f, pl->sums, &R, heavy_list, &dc->heavy_cnt, dc->err, st);
    fgd_cell_struct2r(ts, pl->tiles_dev, pl->tiles_dev, pl->ntiles, pl->polys.npoly ? 0 : nsrc, ndst, pl->S, pl->D.area, R, pl->mask_dev, order,
                      pl->src_idx_f, pl->sums, dc->err, st, dc->band_keys, (opt.cull && !pl->polys.npoly) ? 2 : 0, heavy_list, &dc->heavy_cnt,
                      rare_list, &dc->rare_cnt, ps, pair_beg, pair_cnt, big_list, &dc->big_cnt);
  } else if (opt.cull && !boxm && !pl->polys.npoly) {
    // the destination grid's latitude range from its corners (a 5 us reduction), then ONE record launch in which the source
    // blocks that cannot meet it leave early (round 2 first ran a destination launch, then a source launch: two latency floors)
    fgd_band_keys(in.lat_out, (long)(pl->nx_out + 1) * (pl->ny_out + 1), dc->band_keys, st);
    fgd_cell_struct2(ts, pl->tiles_dev, pl->tiles_dev, pl->ntiles, nsrc, ndst, pl->S, pl->D, bins, bin_cnt, order, pl->src_idx_f, pl->sums, dc->err, st, dc->band_keys, 2, dst_tlon);
  } else if (pl->polys.npoly) {
    fgd_polylist_records(pl->polys, pl->S, pl->src_idx_f, pl->sums, nullptr, nullptr, nullptr, dc->err, st);
    fgd_cell_struct2(ts, pl->tiles_dev, pl->tiles_dev, pl->ntiles, 0, ndst, pl->S, pl->D, bins, bin_cnt, order, pl->src_idx_f, pl->sums, dc->err, st, nullptr, 0, dst_tlon);
  } else
    fgd_cell_struct2(ts, pl->tiles_dev, pl->tiles_dev, pl->ntiles, nsrc, ndst, pl->S, pl->D, bins, bin_cnt, order, pl->src_idx_f, pl->sums, dc->err, st, nullptr, 0, dst_tlon);
  if (boxm) fgd_box_cell_boxes(boxm->box, pl->S, st);
  if (boxm && boxm->no_adjust) fgd_box_area_no_adjust(boxm->box, pl->S.area, st);      // create_xgrid.c:239-242
  pt.end();
  pl->have_geom = true;

  if (!rect) {
    pt.begin(PH_BINS);
    if (gc) fgd_bin_count(ndst, pl->D, bins, bin_cnt, st);
    fgd_exclusive_scan1(bin_cnt, nslots, bin_start, lb_bins, &tickets[0], &dc->total[0], dc->err, st);
    fgd_bin_fill(ndst, pl->D, bins, bin_fill, bin_start, bin_entries, ecap, nsrc, pl->S, pl->mask_dev, heavy_list, &dc->heavy_cnt, st);
    pt.end();
  }

  pt.begin(PH_CANDIDATES);
  if (rect)
    fgd_candidates_rect(nsrc, pl->S, pl->mask_dev, pl->rect_tab, ps, pair_beg, pair_cnt, heavy_list, &dc->heavy_cnt, big_list, &dc->big_cnt, st,
                        pl->polys.npoly ? 0 : 1,          // (the record kernel made the candidates of every cell that is not listed)
                        rare_list, &dc->rare_cnt, dc->err, pl->polys.npoly ? nullptr : pl->sums);
  else
    fgd_candidates1(nsrc, pl->S, pl->mask_dev, bins, bin_start, bin_entries, ecap, ps, pair_beg, pair_cnt, heavy_list, &dc->heavy_cnt, big_list,
                    &dc->big_cnt, st);
  pt.end();
  // --- clip, area, centroid integrals
  hipEvent_t gc_e1 = nullptr, gc_e2 = nullptr;        // great-circle clip: the listed pairs run on stream B beside k_gc_walk
  struct EvReturn {                                   // back to the cache on every way out of this function (FGCHK / fg_fail returns too)
    hipEvent_t &a, &b;
    ~EvReturn() { g_handles.put_sync_event(a); g_handles.put_sync_event(b); a = b = nullptr; }
  } ev_return{gc_e1, gc_e2};
  if (boxm) {
    pt.begin(PH_CLIP_GENERAL);
    fgd_clip_box(order, ps, boxm->box, th[pl->ntiles], pl->S, pl->D, pl->mask_dev, boxm->mask_quad, tmp_area, tmp_clon, tmp_clat, nacc, dc->stats, dc->err, st);
    pt.end();
  } else if (gc) {
    pt.begin(PH_CLIP_GENERAL);
    if (gc_poly)
      fgd_gc_clip_poly(ps, pl->S, pl->gc_prec, pl->D, tmp_area, nacc, dc->stats, dc->err, st);
    else if (gc_split) {
      if (!pl->stream_b) pl->stream_b = g_handles.get_stream(pl->device);
      gc_e1 = g_handles.get_sync_event(); gc_e2 = g_handles.get_sync_event();
      GcSplit g{gc_meta, gc_tbase, gc_task, gc_res, (unsigned)tcap_reg, (unsigned *)(zero_blk + z_gc_ntask), defer_list, &dc->defer_cnt,
                &dc->gc_list2_cnt, npairs, gc_order, (unsigned *)(zero_blk + z_gc_ocnt)};
      fgd_gc_clip_split(ps, pl->S, pl->mask_dev, pl->D, tmp_area, nacc, g, dc->stats, dc->err, st, pl->stream_b, gc_e1, gc_e2);
    } else
      fgd_gc_clip(ps, pl->S, pl->mask_dev, pl->D, tmp_area, nacc, defer_list, &dc->defer_cnt, dc->stats, dc->err, st);
    pt.end();
  } else {
    pt.begin(PH_CLIP_QUAD);
    fgd_clip_quad(order, ps, pl->S, pl->mask_dev, pl->D, tmp_area, tmp_clon, tmp_clat, nacc, defer_list, &dc->defer_cnt, dc->stats, dc->err, st,
                  rect ? &pl->rect_tab : nullptr, row_cnt, tmp_rowpos);
    pt.end();
    pt.begin(PH_CLIP_GENERAL);
    fgd_clip_general(order, ps, pl->S, pl->mask_dev, pl->D, tmp_area, tmp_clon, tmp_clat, nacc, defer_list, &dc->defer_cnt, dc->stats, dc->err, st,
                     rect ? &pl->rect_tab : nullptr, row_cnt, tmp_rowpos);
    pt.end();
  }
  // --- compaction into canonical order, per-source-cell sums, destination-row slots
  pt.begin(PH_COMPACT);
  FgCompactIo io{};
  io.pair_beg = pair_beg; io.pair_cnt = pair_cnt;
  io.tmp_area = tmp_area; io.tmp_clon = tmp_clon; io.tmp_clat = tmp_clat;
  io.xoff = pl->xoff; io.x_src = pl->x_src; io.x_dst = pl->x_dst; io.x_area = pl->x_area; io.x_c1 = pl->x_c1; io.x_c2 = pl->x_c2;
  io.row_cnt = row_cnt; io.x_rowpos = x_rowpos; io.sums = pl->sums; io.big_list = big_list; io.big_cnt = &dc->big_cnt;
  io.tmp_rowpos = tmp_rowpos; io.row_ptr = pl->csr.row_ptr; io.perm = pl->perm;
  io.dc = dc; io.xcap = nx_alloc;
  if (early_rows)       // accepted pairs per source cell -> xoff, destination-row counts -> row_ptr: one launch
    fgd_exclusive_scan2(nacc, nsrc, pl->xoff, lb_comp, &tickets[2], &dc->xtot, row_cnt, ndst, pl->csr.row_ptr, lb_rows, &tickets[1], &dc->rows_total, dc->err, st);
  else
    fgd_exclusive_scan1(nacc, nsrc, pl->xoff, lb_comp, &tickets[2], &dc->xtot, dc->err, st);
  fgd_compact(order, nsrc, ps, io, st);
  pt.end();
  if (!early_rows) {
    pt.begin(PH_ROWS);
    fgd_exclusive_scan1(row_cnt, ndst, pl->csr.row_ptr, lb_rows, &tickets[1], &dc->rows_total, dc->err, st);
    fgd_csr_fill_pos(nx_alloc, &dc->xtot, pl->x_src, pl->x_dst, pl->csr.row_ptr, x_rowpos, pl->perm, st);
    pt.end();
  }
  ptot.end();
  // fg_set_search_finalize(1): the centroid pass and the CSR records of fg_plan_finalize queued HERE, behind the compaction and
  // before the one synchronisation -- a single-plan job (one destination tile, one rank: the plan's own per-cell sums are the
  // totals) then has no host round trip and no idle GPU between its search and its finalize (25-30 us of a 0.9 ms step; rocprofv3
  // kernel timeline, scripts/band_trace.sh).  The records are sized by the capacity of the exchange-cell arrays (the count is
  // not known yet); an attempt that has to be repeated drops them with everything else.
  const bool fuse = opt.finalize && early_rows && !pl->polys.npoly;
  // Stream-ordered (fg_set_search_async): every counter is final when the compaction ends -- k_centroids
  // and k_csr_sortgather write cen, the CSR records and their scratch only -- so the counters leave from HERE, and the host
  // waits for them alone; the two kernels below are still queued or running when the search returns.
  // A one-wave kernel on the plan's stream stores them, and behind them an arrival mark that the host polls: no event and no
  // second stream, so nothing holds k_centroids back but the kernel's own 4-5 us (the parent's readback copy took as long at the
  // end of the step).  The same kernel, or a copy, on the second stream between two events held k_centroids back by 7 us and
  // cost a host wake-up through an event.
  const bool stream_ordered = fuse && opt.async && !opt.profile;
  static thread_local unsigned long long rb_seq = 0;
  int *fused_tmp = nullptr;
  if (fuse) {            // the finalize's blocks first: no error return stands between the counter kernel's launch and the wait for it
    if (order == 2) { pl->cen = pl->alloc<FgSrcRec>((size_t)nsrc + 1); pl->csr.e2 = pl->alloc<FgCsrEntry2>(nx_alloc + 1); }
    else pl->csr.e1 = pl->alloc<FgCsrEntry1>(nx_alloc + 1);
    if ((order == 2 && !pl->cen) || (!pl->csr.e1 && !pl->csr.e2)) return fg_fail(FG_ERR_HIP, "out of device memory");
    fused_tmp = pl->alloc<int>(3 * (size_t)(nx_alloc + 1));     // (scratch for rows beyond the LDS staging; null = the serial last resort)
  }
  if (stream_ordered) {
    unsigned *hc_dev = nullptr;
    if (hipHostGetDevicePointer((void **)&hc_dev, hc, 0) != hipSuccess || !hc_dev) return fg_fail(FG_ERR_HIP, "the counters' host block is not mapped");
    const int nwords = (int)(sizeof(FgCounters) / sizeof(unsigned));
    k_counters_out<<<1, 64, 0, st>>>((const unsigned *)dc, hc_dev, nwords, (unsigned long long *)(hc_dev + nwords), ++rb_seq);
    FGCHK(hipGetLastError());
  }
  if (fuse) {
    pt.begin(PH_FINALIZE);
    if (order == 2) fgd_centroids(nsrc, pl->S, pl->sums, pl->cen, st);
    // (the row-length heuristic of the record kernel wants the exchange-cell count: nsrc + ndst is within a factor of it)
    fgd_csr_sortgather(order, ndst, (long)nsrc + ndst, pl->perm, pl->x_area, pl->x_c1, pl->x_c2, pl->src_idx_f,
                       order == 2 ? pl->cen : nullptr, pl->csr, st, fused_tmp, nx_alloc + 1);
    pt.end();
  }
  if (stream_ordered) {
    if (hipError_t e = hipGetLastError()) {                     // (the launches; the wait below may leave a "not ready" behind)
      (void)hipStreamSynchronize(st);                           // (the counter kernel must not write the host block behind a later search)
      return fg_fail(FG_ERR_HIP, "a launch of the search failed: %s", hipGetErrorString(e));
    }
    FGCHK(wait_counters(hc, rb_seq, st));                      // the one host wait of this search: up to the compaction, no further
  } else {
    FGCHK(hipMemcpyAsync(hc, dc, sizeof(FgCounters), hipMemcpyDeviceToHost, st));
    FGCHK(hipStreamSynchronize(st));                            // the one synchronisation of a search (stream B's work is ordered before it)
  }
  pt.collect(pl->phase_ms); ptot.collect(pl->phase_ms);          // (also hands the timing events back on every exit below)
  FGCHK(hipGetLastError());
  if (rect && hc->rect_bad) { caps->rect = false; return FG_RETRY; }   // not a rectilinear grid after all: every kernel of this attempt left at once
  if (rect && (hc->err[0] & G_ERRBIT_WIDECAP)) { caps->rect = false; return FG_RETRY; }   // the side table of the compact source cells is full
  if (hc->total[0] > nentries) { caps->entries = hc->total[0]; return FG_RETRY; }
  if (hc->total[0] > 2000000000ull) return fg_fail(FG_ERR_ARG, "bin table too large");
  if (hc->total[3] > (unsigned long long)ps.regcap) {
    if (hc->total[3] > 2000000000ull / (unsigned long long)ps.nreg) return fg_fail(FG_ERR_CAPACITY, "candidate pair list exceeds 2^31 entries");
    caps->regcap = (int)((hc->total[3] + FG_REG_ALIGN - 1) / FG_REG_ALIGN * FG_REG_ALIGN);
    return FG_RETRY;
  }
  if (hc->err[2] & G_ERRBIT_LL2X) return fg_fail(FG_ERR_ARG, "latlon2xyz: a grid corner is not finite, or its latitude (|lat| >= 2.4262) or longitude "
                                                          "(|lon| > 1024) lies outside the range of the device trig (radians expected)");
  if (hc->err[0] & 8u) return fg_fail(FG_ERR_ARG, "a grid corner latitude lies outside [-pi/2, pi/2] (radians expected)");
  if (hc->err[0] & 1u) return fg_fail(FG_ERR_MAXV, "create_xgrid.c: n2_in is greater than MAX_V");
  if (hc->err[0] & 2u) return fg_fail(FG_ERR_PARALLEL, "the line between <x1_0,y1_0> and  <x1_1,y1_1> should not parallel to "
                                                    "the line between <x2_0,y2_0> and  <x2_1,y2_1>");
  if (hc->err[0] & 4u) return fg_fail(FG_ERR_MAXV, "clipped polygon exceeds 16 vertices");
  if (hc->err[0] & G_ERRBIT_GC_CONVEX1) return fg_fail(FG_ERR_GEOM, "create_xgrid.c(clip_2dx2d_great_circle): grid box 1 is not convex");
  if (hc->err[0] & G_ERRBIT_GC_CONVEX2) return fg_fail(FG_ERR_GEOM, "create_xgrid.c(clip_2dx2d_great_circle): grid box 2 is not convex");
  if (hc->err[0] & G_ERRBIT_GC_POLYN) return fg_fail(FG_ERR_MAXV, "a polygon of the list has more than 8 vertices");
  if (hc->err[0] & G_ERRBIT_GC_CLIP) return fg_fail(FG_ERR_GEOM, "%s", gc_clip_error((int)hc->err[1]));
  if (hc->err[0] & G_ERRBIT_LOOKBACK) return fg_fail(FG_ERR_HIP, "single-pass scan: a tile waited too long for its predecessor");
  pl->nx = (long)hc->xtot;
  pl->stats[FG_STAT_PAIRS] = (long)hc->total[1];
  pl->stats[FG_STAT_NONEMPTY] = (long)(hc->xtot + hc->stats[FG_STAT_BELOW]);
  pl->stats[FG_STAT_NXGRID] = pl->nx;
  pl->stats[FG_STAT_BORDERLINE] = (long)hc->stats[FG_STAT_BORDERLINE];
  pl->stats[FG_STAT_BINS] = nbins;
  pl->stats[FG_STAT_BIN_ENTRIES] = (long)hc->total[0];
  pl->stats[FG_STAT_DEFERRED] = hc->defer_cnt + hc->gc_list2_cnt;
  pl->stats[FG_STAT_HEAVY] = hc->heavy_cnt;
  pl->stats[FG_STAT_RARE] = hc->rare_cnt;
  pl->stats[FG_STAT_BELOW] = (long)hc->stats[FG_STAT_BELOW];

  pl->rect_tab.bad = nullptr;                          // (lives in the scratch block released below; nothing reads it after the search)
  if (stream_ordered) {                                // k_csr_sortgather may still be reading perm and its scratch: one tagged batch
    blk.scratch.push_back(pl->perm); blk.scratch.push_back(fused_tmp);
    pl->release_on_stream(blk.scratch); blk.scratch.clear();
    pl->perm = nullptr; fused_tmp = nullptr;
  }
  blk.release();                                      // scratch no longer needed
  pl->rows_built = true;
  pl->searched = true;
  if (fuse) {
    pl->release(pl->perm); pl->perm = nullptr; pl->release(fused_tmp);
    if (!pl->red_partial) { pl->red_partial = pl->alloc<double>(1024); pl->red_result = pl->alloc<double>(260); }
    if (!pl->red_partial || !pl->red_result) return fg_fail(FG_ERR_HIP, "out of device memory");
    pl->dist_pending = (order == 2);
    pl->finalized = true; pl->fused = true;
  }
  return pl->nx;
}

// Default capacities first; an attempt that outgrew one (coarse -> very fine grids: a source cell with thousands of
// candidates) drops everything it allocated and is repeated with the sizes its counters report -- at most twice, since the
// candidate counts of an attempt whose bin table was cut short mean nothing.  fg_set_search_mode(1) /
// FREGRID_HIP_EXACT_SEARCH=1 starts from empty buffers, i.e. sizes everything by counting (tests; memory-tight callers).
static int g_search_exact = 0;
extern "C" void fg_set_search_mode(int exact) { g_search_exact = exact; }
// 1: source cells whose latitude range cannot meet the destination grid get no record (a rank of a banded multi-GPU job sees
// a fraction of the source cells); fg_plan_get_cell_area then returns 0 for them.  Results are unchanged.
extern "C" void fg_set_search_cull(int on) { g_search_cull = on ? 1 : 0; }
extern "C" void fg_set_search_finalize(int on) { g_search_finalize = on ? 1 : 0; }
// Stream-ordered plans.  1 (default): a fused search returns when its counters are back, with its centroid
// pass and CSR records still queued; plans take and return their device blocks tagged with their stream, and fg_plan_destroy
// does not drain the stream.  0: the search synchronises its stream at its end, fg_plan_destroy at its start, blocks travel
// untagged.  The tests compare the two bit for bit.
static int g_search_async = 1;
extern "C" void fg_set_search_async(int on) { g_search_async = on ? 1 : 0; }
static long plan_search(fg_plan *pl, const SearchIn &in)
{
  static const bool env_exact = getenv("FREGRID_HIP_EXACT_SEARCH") && atoi(getenv("FREGRID_HIP_EXACT_SEARCH")) != 0;
  // the setters' variables are read HERE and nowhere below: a repeated attempt runs under the options of the first
  const SearchOpts opt{.exact = g_search_exact || env_exact, .cull = g_search_cull != 0, .finalize = g_search_finalize != 0,
                       .rect = g_search_rect != 0, .dst_frame = (tl_dst_frame >= 0 ? tl_dst_frame : g_dst_frame) != 0, .gc_split = g_gc_split, .profile = g_profiling != 0, .async = g_search_async != 0};
  const long big = std::max((long)pl->nsrc, (long)pl->ndst);
  // 32-bit prefixes (bin starts, exchange-cell offsets, CSR rows): the bin table holds up to 3 records per destination cell
  // (+ the wide lists) and the pair list 8 per cell, so grids beyond 2^28 cells could wrap an int before the host sees a
  // counter -- refused up front rather than guarded in every kernel
  if (big > (1L << 28)) return fg_fail(FG_ERR_CAPACITY, "grid of %ld cells: more than 2^28 cells per search are not supported", big);
  SearchCaps caps;
  caps.entries = opt.exact ? 0ull : 3ull * (unsigned long long)pl->ndst + 4096ull;
  const unsigned long long cap_pairs = std::min<unsigned long long>(8ull * (unsigned long long)big + 65536ull, 2000000000ull);
  // regions of the pair list: a run of 256 source cells appends to one region; at least four such runs per region on average, so
  // that small grids do not pile their pairs into a few small regions
  caps.nreg = (int)std::max(1L, std::min((long)FG_NREG, ((long)pl->nsrc + 1023) / 1024));
  caps.regcap = opt.exact ? 0 : (int)((cap_pairs / caps.nreg + FG_REG_ALIGN - 1) / FG_REG_ALIGN * FG_REG_ALIGN);
  caps.rect = opt.rect && in.rect_hint && !in.gc_in && !in.boxm && pl->nx_out <= 8192 && pl->nx_out >= 2;
  const size_t keep = pl->owned.size();              // blocks the caller staged before the search stay
  long rc = FG_RETRY;
  int attempts = 0;
  pl->async = opt.async;
  pl->on_stream = pl->async;                         // (every block of the search is first touched on the plan's stream)
  for (; attempts < 4 && rc == FG_RETRY; attempts++) {
    if (attempts) {
      (void)hipStreamSynchronize(pl->stream);        // (a stream-ordered attempt left its last two kernels queued)
      pl->drop_search(keep);
    }
    rc = plan_search_core(pl, in, opt, &caps);
  }
  pl->on_stream = false;
  if (rc == FG_RETRY) return fg_fail(FG_ERR_CAPACITY, "exchange-grid search: capacities did not settle");
  if (rc >= 0) pl->stats[FG_STAT_EXACT] = (attempts > 1) ? 1 : 0;
  pl->search_d2h = (long)attempts * (long)sizeof(FgCounters);
  return rc;
}

// ----------------------------------------------------------------------------- mean cell extents of the destination grid
// A strided sample of at most ~4096 cells (sample k = cell k * step), their corners in a compact buffer
// q[array][sample][4] = SW, SE, NE, NW; the arrays are lon, lat or x, y, z.
struct CornerSample {
  int nsamp = 0;
  std::vector<double> q;
  const double *corners(int a, int k) const { return &q[((size_t)a * nsamp + k) * 4]; }
};
static long sample_step(int nx, int ny, int *nsamp)
{
  const long ncell = (long)nx * ny;
  long step = ncell / 4096; if (step < 1) step = 1;
  *nsamp = (int)((ncell + step - 1) / step);
  return step;
}
// the corner nodes of sample k in a corner array of nx + 1 columns, in the buffer's order
__host__ __device__ static inline void sample_nodes(int nx, long step, int k, long n[4])
{
  const long c = (long)k * step;
  const int i = (int)(c % nx), j = (int)(c / nx);
  n[0] = (long)j * (nx + 1) + i; n[1] = n[0] + 1; n[3] = n[0] + nx + 1; n[2] = n[3] + 1;
}
static CornerSample sample_corners_host(int nx, int ny, int narr, const double *const *arr)
{
  CornerSample s;
  const long step = sample_step(nx, ny, &s.nsamp);
  s.q.resize((size_t)s.nsamp * narr * 4);
  for (int k = 0; k < s.nsamp; k++) {
    long n[4];
    sample_nodes(nx, step, k, n);
    for (int a = 0; a < narr; a++)
      for (int v = 0; v < 4; v++) s.q[((size_t)a * s.nsamp + k) * 4 + v] = arr[a][n[v]];
  }
  return s;
}
// Corner arrays that live on the device: the sampled cells' corners are gathered there, and the compact buffer is copied -- a
// quarter of a megabyte instead of the whole grid (the whole 0.25-degree target copied into a fresh std::vector took 29 ms,
// thirty times the search it was preparing).
__global__ void k_sample_corners(int nx, long step, int nsamp, int narr, const double *a0, const double *a1, const double *a2, double *out)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nsamp) return;
  long n[4];
  sample_nodes(nx, step, k, n);
  const double *arr[3] = {a0, a1, a2};
  for (int a = 0; a < narr; a++) {
    double *o = out + ((size_t)a * nsamp + k) * 4;
    o[0] = arr[a][n[0]]; o[1] = arr[a][n[1]]; o[2] = arr[a][n[2]]; o[3] = arr[a][n[3]];
  }
}
static int sample_corners_dev(fg_plan *pl, int nx, int ny, int narr, const double *d_a0, const double *d_a1, const double *d_a2, CornerSample *s)
{
  const long step = sample_step(nx, ny, &s->nsamp);
  s->q.resize((size_t)s->nsamp * narr * 4);
  double *d_q = (double *)g_pool.get(pl->device, s->q.size() * sizeof(double));
  if (!d_q) return fg_fail(FG_ERR_HIP, "out of device memory");
  k_sample_corners<<<(s->nsamp + 255) / 256, 256, 0, pl->stream>>>(nx, step, s->nsamp, narr, d_a0, d_a1, d_a2, d_q);
  hipError_t e = hipMemcpyAsync(s->q.data(), d_q, s->q.size() * sizeof(double), hipMemcpyDeviceToHost, pl->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(pl->stream);
  g_pool.put(d_q);
  if (e != hipSuccess) return fg_fail(FG_ERR_HIP, "sampling the destination corners failed: %s", hipGetErrorString(e));
  return 0;
}
// sums over cnt representative cells -> the means choose_bins takes
static void mean_extents(double sl, double sw, long cnt, double *mdlat, double *mdlon)
{
  const double PI = 3.14159265358979323846;
  if (cnt == 0) { *mdlat = PI / 180; *mdlon = PI / 180; return; }
  *mdlat = sl / cnt; *mdlon = sw / cnt;
  if (*mdlat < 1e-7) *mdlat = 1e-7;
  if (*mdlon < 1e-7) *mdlon = 1e-7;
}
// lon / lat corners: latitude range and widest edge in longitude of every sampled cell.
// *curvilinear = 1 if a sampled cell's west / east corners differ in longitude or its south / north corners in latitude (bit
// patterns, the test k_rect_tables applies to the whole grid): such a target cannot take the rectilinear path, and the search does
// not spend an attempt on finding that out (a cubed-sphere tile as target: 0.2 ms of kernels and a read-back per plan)
static void extents_lonlat(const CornerSample &s, double *mdlat, double *mdlon, int *curvilinear)
{
  const double PI = 3.14159265358979323846;
  *curvilinear = 0;
  double sl = 0, sw = 0; long cnt = 0;
  for (int k = 0; k < s.nsamp; k++) {
    const double *x = s.corners(0, k), *y = s.corners(1, k);
    if (memcmp(&x[0], &x[3], 8) || memcmp(&x[1], &x[2], 8) || memcmp(&y[0], &y[1], 8) || memcmp(&y[3], &y[2], 8)) *curvilinear = 1;
    double ymin = y[0], ymax = y[0], w = 0;
    for (int m = 1; m < 4; m++) { if (y[m] < ymin) ymin = y[m]; if (y[m] > ymax) ymax = y[m]; }
    for (int m = 0; m < 4; m++) {
      double d = fabs(x[(m + 1) & 3] - x[m]);              // |remainder(dx, 2 pi)|: the subtraction is exact for pi <= |dx| <= 4 pi (Sterbenz),
      if (d > 3.0 * PI) d = fabs(remainder(d, 2.0 * PI)); else if (d > PI) d = fabs(2.0 * PI - d);   // so the same bits as the library call,
      if (d > w) w = d;                                    // which took 0.12 ms per plan for the 16 k differences of the sample
    }
    if (w > PI / 2) continue;      // polar caps: not representative
    sl += ymax - ymin; sw += w; cnt++;
  }
  mean_extents(sl, sw, cnt, mdlat, mdlon);
}
// unit-vector corners (great-circle plans): the diagonal SW - NE of every sampled cell as its cap-box extent
static void extents_xyz(const CornerSample &s, double *mdlat, double *mdlon)
{
  double sl = 0, sw = 0; long cnt = 0;
  for (int k = 0; k < s.nsamp; k++) {
    const double *x = s.corners(0, k), *y = s.corners(1, k), *z = s.corners(2, k);
    const double dx = x[0] - x[2], dy = y[0] - y[2], dz = z[0] - z[2];
    const double diag = sqrt(dx * dx + dy * dy + dz * dz);
    const double zc = 0.5 * (z[0] + z[2]);
    const double coslat = sqrt(fmax(0.0, 1.0 - zc * zc));
    if (coslat < 0.2) continue;
    sl += diag; sw += diag / coslat; cnt++;
  }
  mean_extents(sl, sw, cnt, mdlat, mdlon);
}
// What a search takes from the destination grid before it starts: the mean extents and the rectilinear hint (SearchIn).
struct DstExtents { double dlat = 0, dlon = 0; int rect_hint = 1; };
// host corner arrays: the sample for the extents, a look at a few corners for the hint
static DstExtents dst_extents_host(int nx, int ny, const double *lon, const double *lat)
{
  const double *arr[2] = {lon, lat};
  DstExtents x;
  int curvilinear;
  extents_lonlat(sample_corners_host(nx, ny, 2, arr), &x.dlat, &x.dlon, &curvilinear);
  x.rect_hint = host_says_not_rect(nx, ny, lon, lat) ? 0 : 1;
  return x;
}
// device corner arrays, lon / lat (d_a2 null) or x / y / z: a no-op when the caller gave positive extents, otherwise the sample
// is gathered on the plan's stream and read back (one synchronisation); the lon / lat form also gives the hint
static int dst_extents_dev(fg_plan *pl, const double *d_a0, const double *d_a1, const double *d_a2, DstExtents *x)
{
  if (x->dlat > 0 && x->dlon > 0) return 0;
  CornerSample s;
  FGCHK(hipSetDevice(pl->device));
  if (sample_corners_dev(pl, pl->nx_out, pl->ny_out, d_a2 ? 3 : 2, d_a0, d_a1, d_a2, &s)) return FG_ERR_HIP;
  int curvilinear = 0;
  if (d_a2) extents_xyz(s, &x->dlat, &x->dlon);
  else extents_lonlat(s, &x->dlat, &x->dlon, &curvilinear);
  x->rect_hint = !curvilinear;
  return 0;
}

// ----------------------------------------------------------------------------- plan creation: the steps the entries share
// Ownership: a static helper that fails returns the error and leaves the plan alone.  Every extern "C" entry holds the plan it
// got from plan_base in a PlanGuard, which destroys it on every way out but one: hand_over passes the entry's result through
// and gives the plan to the caller when that is no error, so *plan_out is written on success only.
struct PlanGuard {
  fg_plan *pl = nullptr;
  ~PlanGuard() { fg_plan_destroy(pl); }
  long hand_over(long rc, fg_plan **plan_out) { if (rc >= 0) { *plan_out = pl; pl = nullptr; } return rc; }
};
// The grid-pointer check of every entry, host or device arrays alike: the tables themselves, the destination arrays, and every
// tile's corner arrays (a tile's mask may be null).  ntiles is the plan's, i.e. plan_base has seen it.
static int check_grid_ptrs(int ntiles, std::initializer_list<const double *const *> tables, std::initializer_list<const double *> dst)
{
  bool ok = true;
  for (const double *const *t : tables) ok = ok && t;
  for (const double *p : dst) ok = ok && p;
  if (ok) for (const double *const *t : tables) for (int m = 0; m < ntiles; m++) ok = ok && t[m];
  return ok ? 0 : fg_fail(FG_ERR_ARG, "null grid pointer");
}
namespace {
// Host arrays into plan-owned blocks, all in one batch of the transfer pool; done() hands back the blocks, for a caller whose
// search has run and needs none of them any more.
struct HostUpload {
  fg_plan *pl = nullptr;
  bool ok = true;
  std::vector<XferJob> jobs;
  std::vector<void *> blocks;
  template <typename T> T *put(const T *h, size_t n)
  {
    T *d = pl->alloc<T>(n);
    ok = ok && d;
    if (d) { jobs.push_back(XferJob{(void *)h, d, n * sizeof(T), false}); blocks.push_back(d); }
    return d;
  }
  bool run() { return ok && xfer_pool().run(pl->device, jobs); }
  void done() { for (void *p : blocks) pl->release(p); blocks.clear(); }
};
// The staging of host lon / lat: every source tile's corner arrays and mask (where given) and the destination's corner arrays.
// lon / lat / mask are the device pointer tables a SearchIn takes.
struct StagedGrids {
  HostUpload up;
  std::vector<const double *> lon, lat, mask;
  const double *lon_out = nullptr, *lat_out = nullptr;
  bool has_masks = false;
  explicit StagedGrids(fg_plan *pl) : up{pl}, lon(pl->ntiles), lat(pl->ntiles), mask(pl->ntiles, nullptr) {}
  const double *const *masks() const { return has_masks ? mask.data() : nullptr; }
};
}  // namespace
static int stage_host_grids(fg_plan *pl, const double *const *lon_in, const double *const *lat_in, const double *const *mask_in,
                            const double *lon_out, const double *lat_out, StagedGrids *s)
{
  if (int rc = check_grid_ptrs(pl->ntiles, {lon_in, lat_in}, {lon_out, lat_out})) return rc;     // (before anything touches the device)
  HostUpload &up = s->up;
  s->has_masks = mask_in != nullptr;
  for (int m = 0; m < pl->ntiles && up.ok; m++) {
    const size_t np = (size_t)(pl->nx_in[m] + 1) * (pl->ny_in[m] + 1);
    s->lon[m] = up.put(lon_in[m], np); s->lat[m] = up.put(lat_in[m], np);
    if (mask_in && mask_in[m]) s->mask[m] = up.put(mask_in[m], (size_t)pl->nx_in[m] * pl->ny_in[m]);
  }
  const size_t npo = (size_t)(pl->nx_out + 1) * (pl->ny_out + 1);
  if (up.ok) { s->lon_out = up.put(lon_out, npo); s->lat_out = up.put(lat_out, npo); }
  if (!up.run()) return fg_fail(FG_ERR_HIP, "grid upload failed (out of device memory?)");
  return 0;
}
// The plan runs on the caller's stream from here on and never owns it; a stream of its own goes back to the cache.
static void adopt_stream(fg_plan *pl, void *stream)
{
  if (pl->own_stream && pl->stream) g_handles.put_stream(pl->device, pl->stream);
  else if (!pl->own_stream) g_pool.seal(pl->stream);      // (the plan stops vouching for the caller's previous stream)
  pl->stream = (hipStream_t)stream; pl->own_stream = false;
}

extern "C" long fg_plan_create(int order, int ntiles_in, const int *nx_in, const int *ny_in,
                               const double *const *lon_in, const double *const *lat_in,
                               const double *const *mask_in,
                               int nx_out, int ny_out, const double *lon_out, const double *lat_out,
                               int device, fg_plan **plan_out)
{
  PlanGuard g;
  if (int rc = plan_base(order, ntiles_in, nx_in, ny_in, nx_out, ny_out, device, &g.pl)) return rc;
  StagedGrids s(g.pl);
  if (int rc = stage_host_grids(g.pl, lon_in, lat_in, mask_in, lon_out, lat_out, &s)) return rc;
  const DstExtents x = dst_extents_host(nx_out, ny_out, lon_out, lat_out);
  const long nx = plan_search(g.pl, SearchIn{.lon_in = s.lon.data(), .lat_in = s.lat.data(), .mask_in = s.masks(), .lon_out = s.lon_out,
                                             .lat_out = s.lat_out, .mean_dlat = x.dlat, .mean_dlon = x.dlon, .rect_hint = x.rect_hint});
  if (nx >= 0) s.up.done();
  return g.hand_over(nx, plan_out);
}

// Same as fg_plan_create but every grid pointer is a DEVICE pointer (inputs already in HBM).
// mean_dlat/mean_dlon: typical destination cell extent in radians (<=0: derive by copying a
// strided sample of the destination corners to the host).
extern "C" long fg_plan_create_dev(int order, int ntiles_in, const int *nx_in, const int *ny_in,
                                   const double *const *d_lon_in, const double *const *d_lat_in,
                                   const double *const *d_mask_in,
                                   int nx_out, int ny_out, const double *d_lon_out, const double *d_lat_out,
                                   double mean_dlat, double mean_dlon, int device, void *stream,
                                   int use_caller_stream, fg_plan **plan_out)
{
  PlanGuard g;
  if (int rc = plan_base(order, ntiles_in, nx_in, ny_in, nx_out, ny_out, device, &g.pl)) return rc;
  if (int rc = check_grid_ptrs(ntiles_in, {d_lon_in, d_lat_in}, {d_lon_out, d_lat_out})) return rc;
  if (use_caller_stream) adopt_stream(g.pl, stream);
  DstExtents x{mean_dlat, mean_dlon};
  if (int rc = dst_extents_dev(g.pl, d_lon_out, d_lat_out, nullptr, &x)) return rc;
  const long nx = plan_search(g.pl, SearchIn{.lon_in = d_lon_in, .lat_in = d_lat_in, .mask_in = d_mask_in, .lon_out = d_lon_out,
                                             .lat_out = d_lat_out, .mean_dlat = x.dlat, .mean_dlon = x.dlon, .rect_hint = x.rect_hint});
  return g.hand_over(nx, plan_out);
}

// ------------------------------------------------------------------------------------- great-circle plans
// The tail of every great-circle entry.  gxyz: the corner unit vectors on the device, [ntiles] source tiles and the destination
// grid as entry [ntiles]; x: the caller's extents, derived from the destination's unit vectors where not positive.  After the
// search nothing reads the corner arrays any more (the cell records hold the corners; fg_plan_get_polygons works from those).
static long gc_search(fg_plan *pl, const GcXyz *gxyz, const double *const *d_mask_in, DstExtents x)
{
  const GcXyz *out = &gxyz[pl->ntiles];
  if (int rc = dst_extents_dev(pl, out->x, out->y, out->z, &x)) return rc;
  return plan_search(pl, SearchIn{.mask_in = d_mask_in, .gc_in = gxyz, .gc_out = out, .mean_dlat = x.dlat, .mean_dlon = x.dlon});
}

extern "C" long fg_plan_create_great_circle_dev(int ntiles_in, const int *nx_in, const int *ny_in,
                                                const double *const *d_x_in, const double *const *d_y_in, const double *const *d_z_in,
                                                const double *const *d_mask_in, int nx_out, int ny_out,
                                                const double *d_x_out, const double *d_y_out, const double *d_z_out,
                                                double mean_dlat, double mean_dlon, int device, void *stream, int use_caller_stream,
                                                fg_plan **plan_out)
{
  PlanGuard g;
  if (int rc = plan_base(FG_CONSERVE_ORDER1, ntiles_in, nx_in, ny_in, nx_out, ny_out, device, &g.pl)) return rc;
  if (int rc = check_grid_ptrs(ntiles_in, {d_x_in, d_y_in, d_z_in}, {d_x_out, d_y_out, d_z_out})) return rc;
  if (use_caller_stream) adopt_stream(g.pl, stream);
  std::vector<GcXyz> gxyz(ntiles_in + 1);
  for (int m = 0; m < ntiles_in; m++) gxyz[m] = GcXyz{d_x_in[m], d_y_in[m], d_z_in[m]};
  gxyz[ntiles_in] = GcXyz{d_x_out, d_y_out, d_z_out};
  const long nx = gc_search(g.pl, gxyz.data(), d_mask_in, DstExtents{mean_dlat, mean_dlon});
  return g.hand_over(nx, plan_out);
}

// host corner arrays, unit vectors on the host (libm, as the reference), then one synchronous upload per grid
extern "C" long fg_plan_create_great_circle(int ntiles_in, const int *nx_in, const int *ny_in,
                                            const double *const *lon_in, const double *const *lat_in, const double *const *mask_in,
                                            int nx_out, int ny_out, const double *lon_out, const double *lat_out,
                                            int device, fg_plan **plan_out)
{
  PlanGuard g;
  if (int rc = plan_base(FG_CONSERVE_ORDER1, ntiles_in, nx_in, ny_in, nx_out, ny_out, device, &g.pl)) return rc;
  if (int rc = check_grid_ptrs(ntiles_in, {lon_in, lat_in}, {lon_out, lat_out})) return rc;
  fg_plan *pl = g.pl;
  std::vector<GcXyz> gxyz(ntiles_in + 1);           // [ntiles_in] = the destination grid
  std::vector<const double *> dmask(ntiles_in, nullptr);
  std::vector<void *> blocks;
  std::vector<double> h;
  auto upload = [&](const double *src, size_t n) -> double * {
    double *d = pl->alloc<double>(n);
    if (d) blocks.push_back(d);
    return d && hipMemcpy(d, src, n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess ? d : nullptr;
  };
  for (int m = 0; m <= ntiles_in; m++) {
    const bool src = m < ntiles_in;
    const size_t np = src ? (size_t)(nx_in[m] + 1) * (ny_in[m] + 1) : (size_t)(nx_out + 1) * (ny_out + 1);
    h.resize(3 * np);                               // x | y | z
    fg_latlon2xyz((long)np, src ? lon_in[m] : lon_out, src ? lat_in[m] : lat_out, h.data(), h.data() + np, h.data() + 2 * np);
    const double *d = upload(h.data(), 3 * np);
    bool ok = d != nullptr;
    if (ok && src && mask_in && mask_in[m]) ok = (dmask[m] = upload(mask_in[m], (size_t)nx_in[m] * ny_in[m])) != nullptr;
    if (!ok) return fg_fail(FG_ERR_HIP, "grid upload failed (out of device memory?)");
    gxyz[m] = GcXyz{d, d + np, d + 2 * np};
  }
  const long nx = gc_search(pl, gxyz.data(), mask_in ? dmask.data() : nullptr, dst_extents_host(nx_out, ny_out, lon_out, lat_out));
  if (nx >= 0) for (void *p : blocks) pl->release(p);
  return g.hand_over(nx, plan_out);
}

// ------------------------------------------------------------------------------------- great-circle plans from lon / lat
// latlon2xyz on the device (latlon2xyz_kernels.hip): the unit vectors carry the bits of the reference's host libm, so nothing of
// the great-circle path is left to the host.

extern "C" int fg_dev_latlon2xyz(long n, const double *d_lon, const double *d_lat, double *d_x, double *d_y, double *d_z, int device, void *stream)
{
  if (n < 0 || (n > 0 && (!d_lon || !d_lat || !d_x || !d_y || !d_z))) return fg_fail(FG_ERR_ARG, "fg_dev_latlon2xyz: bad size or null pointer");
  if (n == 0) return 0;
  FGCHK(hipSetDevice(device));
  const FgLl2xGrid g{d_lon, d_lat, d_x, d_y, d_z, n};
  fgd_latlon2xyz(&g, 1, nullptr, (hipStream_t)stream);
  FGCHK(hipGetLastError());
  return 0;
}

// pl: from plan_base, its stream settled.  Takes the unit-vector buffers from the plan's pool, queues the conversion of every
// grid (one launch) and its error word ahead of the search on the plan's stream, runs gc_search and hands the buffers back.
static long gc_lonlat_search(fg_plan *pl, const double *const *d_lon_in, const double *const *d_lat_in, const double *const *d_mask_in,
                             const double *d_lon_out, const double *d_lat_out, DstExtents x)
{
  const int nt = pl->ntiles;
  std::vector<FgLl2xGrid> jobs(nt + 1);
  std::vector<GcXyz> gxyz(nt + 1);                  // [nt] = the destination grid
  std::vector<void *> blocks;
  for (int m = 0; m <= nt; m++) {
    const size_t np = m < nt ? (size_t)(pl->nx_in[m] + 1) * (pl->ny_in[m] + 1) : (size_t)(pl->nx_out + 1) * (pl->ny_out + 1);
    double *d = pl->alloc<double>(3 * np);          // x | y | z
    if (!d) return fg_fail(FG_ERR_HIP, "out of device memory");
    blocks.push_back(d);
    jobs[m] = FgLl2xGrid{m < nt ? d_lon_in[m] : d_lon_out, m < nt ? d_lat_in[m] : d_lat_out, d, d + np, d + 2 * np, (long)np};
    gxyz[m] = GcXyz{d, d + np, d + 2 * np};
  }
  pl->ll_err = pl->alloc<unsigned>(1);
  if (!pl->ll_err) return fg_fail(FG_ERR_HIP, "out of device memory");
  blocks.push_back(pl->ll_err);
  hipError_t e = hipSetDevice(pl->device);
  if (e == hipSuccess) e = hipMemsetAsync(pl->ll_err, 0, sizeof(unsigned), pl->stream);
  if (e == hipSuccess) { fgd_latlon2xyz(jobs.data(), nt + 1, pl->ll_err, pl->stream); e = hipGetLastError(); }
  if (e != hipSuccess) return fg_fail(FG_ERR_HIP, "latlon2xyz: %s", hipGetErrorString(e));
  const long nx = gc_search(pl, gxyz.data(), d_mask_in, x);
  if (nx < 0) return nx;
  for (void *p : blocks) pl->release(p);
  pl->ll_err = nullptr;
  return nx;
}

extern "C" long fg_plan_create_great_circle_lonlat_dev(int ntiles_in, const int *nx_in, const int *ny_in,
                                                       const double *const *d_lon_in, const double *const *d_lat_in,
                                                       const double *const *d_mask_in, int nx_out, int ny_out,
                                                       const double *d_lon_out, const double *d_lat_out,
                                                       double mean_dlat, double mean_dlon, int device, void *stream, int use_caller_stream,
                                                       fg_plan **plan_out)
{
  PlanGuard g;
  if (int rc = plan_base(FG_CONSERVE_ORDER1, ntiles_in, nx_in, ny_in, nx_out, ny_out, device, &g.pl)) return rc;
  if (int rc = check_grid_ptrs(ntiles_in, {d_lon_in, d_lat_in}, {d_lon_out, d_lat_out})) return rc;
  if (use_caller_stream) adopt_stream(g.pl, stream);
  const long nx = gc_lonlat_search(g.pl, d_lon_in, d_lat_in, d_mask_in, d_lon_out, d_lat_out, DstExtents{mean_dlat, mean_dlon});
  return g.hand_over(nx, plan_out);
}

// host corner arrays: lon / lat go up through the transfer pool (16 bytes per vertex), the rest is the entry above; the extents
// come from the host arrays, as in fg_plan_create_great_circle (no read-back)
extern "C" long fg_plan_create_great_circle_lonlat(int ntiles_in, const int *nx_in, const int *ny_in,
                                                   const double *const *lon_in, const double *const *lat_in, const double *const *mask_in,
                                                   int nx_out, int ny_out, const double *lon_out, const double *lat_out,
                                                   int device, fg_plan **plan_out)
{
  PlanGuard g;
  if (int rc = plan_base(FG_CONSERVE_ORDER1, ntiles_in, nx_in, ny_in, nx_out, ny_out, device, &g.pl)) return rc;
  StagedGrids s(g.pl);
  if (int rc = stage_host_grids(g.pl, lon_in, lat_in, mask_in, lon_out, lat_out, &s)) return rc;
  const long nx = gc_lonlat_search(g.pl, s.lon.data(), s.lat.data(), s.masks(), s.lon_out, s.lat_out,
                                   dst_extents_host(nx_out, ny_out, lon_out, lat_out));
  if (nx >= 0) s.up.done();
  return g.hand_over(nx, plan_out);
}

// A search whose SOURCE cells are a list of polygons (<= 8 vertices each), e.g. the atmosphere x land cells of a coupler mosaic
// against the ocean grid (make_coupler_mosaic.c:1659-1692: clip_2dx2d(atmxlnd polygon, ocean cell)).  Host arrays: n[npoly],
// lon / lat [npoly][8] in the longitude frame of the polygon's parent cell, lon_avg[npoly] = that cell's mean longitude (decides
// the +-2pi shift of a destination cell and is poly_ctrlon's reference longitude), area_ref[npoly] = the area the 1e-6 ratio
// test compares with (together with the destination cell's).  Exchange cells: i_in = polygon index, j_in = t_in = 0.
extern "C" long fg_plan_create_polylist(int order, int npoly, const int *n, const double *lon, const double *lat, const double *lon_avg,
                                        const double *area_ref, int nx_out, int ny_out, const double *lon_out, const double *lat_out,
                                        int device, fg_plan **plan_out)
{
  if (npoly < 1 || !n || !lon || !lat || !lon_avg || !area_ref || !lon_out || !lat_out) return fg_fail(FG_ERR_ARG, "null argument");
  PlanGuard g;
  const int one = 1;
  if (int rc = plan_base(order, 1, &npoly, &one, nx_out, ny_out, device, &g.pl)) return rc;
  fg_plan *pl = g.pl;
  if (order == 2) pl->f_stride = npoly;                  // (no halo: the "field" of a polygon list is one value per polygon)
  const size_t npo = (size_t)(nx_out + 1) * (ny_out + 1);
  HostUpload up{pl};
  pl->polys = FgPolyList{up.put(n, npoly), up.put(lon, (size_t)npoly * 8), up.put(lat, (size_t)npoly * 8), up.put(lon_avg, npoly),
                         up.put(area_ref, npoly), npoly};
  double *d_lo = up.put(lon_out, npo), *d_la = up.put(lat_out, npo);
  if (!up.run()) return fg_fail(FG_ERR_HIP, "polygon upload failed (out of device memory?)");
  const DstExtents x = dst_extents_host(nx_out, ny_out, lon_out, lat_out);
  const double *none[1] = {nullptr};
  const long nx = plan_search(pl, SearchIn{.lon_in = none, .lat_in = none, .lon_out = d_lo, .lat_out = d_la, .mean_dlat = x.dlat,
                                           .mean_dlon = x.dlon, .rect_hint = x.rect_hint});
  if (nx >= 0) { pl->release(d_lo); pl->release(d_la); }     // (the list stays with the plan)
  return g.hand_over(nx, plan_out);
}

// ------------------------------------------------------------------------------------- internal entries (plan_internal.h)
// What coupler.hip needs of a plan without a trip through the host: the exchange cells and source records where they lie, the
// clipped polygons into device arrays, a polygon-list search fed from device arrays, and a search whose destination extents
// and rectilinear hint the caller worked out once from its host copy of the grid.
int fg_plan_view(const fg_plan *pl, FgPlanView *v)
{
  if (!pl || !v) return fg_fail(FG_ERR_ARG, "null argument");
  if (!pl->searched || !pl->have_geom) return fg_fail(FG_ERR_STATE, "fg_plan_view: needs a plan from a search");
  *v = FgPlanView{pl->nx, pl->nsrc, pl->ndst, pl->x_src, pl->x_dst, pl->x_area, pl->order == 2 ? pl->x_c1 : nullptr,
                  pl->order == 2 ? pl->x_c2 : nullptr, pl->S.area, pl->S.lon_avg};
  return 0;
}
// queued on the plan's stream; n_out [nx], lon / lat [nx][8] (device).  A polygon of more than 8 vertices keeps its count.
int fg_plan_polygons_dev(const fg_plan *pl, int *n_out, double *lon, double *lat)
{
  if (!pl || !n_out || !lon || !lat) return fg_fail(FG_ERR_ARG, "null argument");
  if (!pl->searched || !pl->have_geom || !pl->x_src || pl->great_circle) return fg_fail(FG_ERR_STATE, "fg_plan_polygons_dev: needs a legacy plan from a search");
  FGCHK(hipSetDevice(pl->device));
  fgd_xgrid_polygons(pl->nx, pl->x_src, pl->x_dst, pl->S, pl->D, pl->rect ? &pl->rect_tab : nullptr, 8, n_out, lon, lat, pl->stream);
  FGCHK(hipGetLastError());
  return 0;
}
int fg_plan_polygons_gc_dev(const fg_plan *pl, int *n_out, double *x, double *y, double *z)
{
  if (!pl || !n_out || !x || !y || !z) return fg_fail(FG_ERR_ARG, "null argument");
  if (!pl->searched || !pl->have_geom || !pl->x_src || !pl->great_circle || pl->gc_prec)
    return fg_fail(FG_ERR_STATE, "fg_plan_polygons_gc_dev: needs a great-circle plan between grids from a search");
  FGCHK(hipSetDevice(pl->device));
  const long n = pl->nx;
  if (n == 0) return 0;
  const int dev = pl->device;
  double *a = (double *)g_pool.get(dev, (size_t)n * 12 * 8), *b = (double *)g_pool.get(dev, (size_t)n * 12 * 8);
  double *o = (double *)g_pool.get(dev, (size_t)n * FG_GC_POLY_CAP * 3 * 8), *ar = (double *)g_pool.get(dev, (size_t)n * 8);
  struct Put4 { void *p[4]; ~Put4() { for (void *q : p) g_pool.put(q); } } put4{{a, b, o, ar}};
  if (!a || !b || !o || !ar) return fg_fail(FG_ERR_HIP, "out of device memory");
  fgd_xgrid_gather_gc(n, pl->x_src, pl->x_dst, pl->S, pl->D, a, b, pl->stream);
  fgd_gc_clip_batch((int)n, a, b, o, n_out, ar, pl->stream);
  fgd_split_xyz(n, 8, o, x, y, z, pl->stream);
  FGCHK(hipGetLastError());
  FGCHK(hipStreamSynchronize(pl->stream));
  return 0;
}
long fg_plan_search_d2h(const fg_plan *pl) { return pl ? pl->search_d2h : 0; }
extern "C" long fg_plan_device_bytes(const fg_plan *pl, long *sizes, int nmax)
{
  if (!pl) return 0;
  long sum = 0;
  for (size_t k = 0; k < pl->owned.size(); k++) { const long b = (long)g_pool.block_bytes(pl->owned[k]); sum += b; if (sizes && (int)k < nmax) sizes[k] = b; }
  return sum;
}
void fg_dst_extents(int nx, int ny, const double *lon, const double *lat, double *dlat, double *dlon, int *rect_hint)
{
  const DstExtents x = dst_extents_host(nx, ny, lon, lat);
  *dlat = x.dlat; *dlon = x.dlon; *rect_hint = x.rect_hint;
}
int fg_search_frame_override(int frame) { const int old = tl_dst_frame; tl_dst_frame = frame; return old; }
long fg_plan_create_dev_hint(int order, int ntiles_in, const int *nx_in, const int *ny_in, const double *const *d_lon_in,
                             const double *const *d_lat_in, int nx_out, int ny_out, const double *d_lon_out, const double *d_lat_out,
                             double mean_dlat, double mean_dlon, int rect_hint, int device, void *stream, fg_plan **plan_out)
{
  PlanGuard g;
  if (int rc = plan_base(order, ntiles_in, nx_in, ny_in, nx_out, ny_out, device, &g.pl)) return rc;
  if (int rc = check_grid_ptrs(ntiles_in, {d_lon_in, d_lat_in}, {d_lon_out, d_lat_out})) return rc;
  if (!(mean_dlat > 0) || !(mean_dlon > 0)) return fg_fail(FG_ERR_ARG, "fg_plan_create_dev_hint: the extents must be positive");
  adopt_stream(g.pl, stream);
  const long nx = plan_search(g.pl, SearchIn{.lon_in = d_lon_in, .lat_in = d_lat_in, .lon_out = d_lon_out, .lat_out = d_lat_out,
                                             .mean_dlat = mean_dlat, .mean_dlon = mean_dlon, .rect_hint = rect_hint});
  return g.hand_over(nx, plan_out);
}
// fg_plan_create_polylist with every array on the device (n [npoly], lon / lat [npoly][8], lon_avg, area_ref [npoly]); the arrays
// stay the caller's and must outlive the search only.
long fg_plan_create_polylist_dev(int order, int npoly, const int *d_n, const double *d_lon, const double *d_lat, const double *d_lon_avg,
                                 const double *d_area_ref, int nx_out, int ny_out, const double *d_lon_out, const double *d_lat_out,
                                 double mean_dlat, double mean_dlon, int rect_hint, int device, void *stream, fg_plan **plan_out)
{
  if (npoly < 1 || !d_n || !d_lon || !d_lat || !d_lon_avg || !d_area_ref || !d_lon_out || !d_lat_out) return fg_fail(FG_ERR_ARG, "null argument");
  if (!(mean_dlat > 0) || !(mean_dlon > 0)) return fg_fail(FG_ERR_ARG, "fg_plan_create_polylist_dev: the extents must be positive");
  PlanGuard g;
  const int one = 1;
  if (int rc = plan_base(order, 1, &npoly, &one, nx_out, ny_out, device, &g.pl)) return rc;
  fg_plan *pl = g.pl;
  if (order == 2) pl->f_stride = npoly;
  adopt_stream(pl, stream);
  pl->polys = FgPolyList{d_n, d_lon, d_lat, d_lon_avg, d_area_ref, npoly};
  const double *none[1] = {nullptr};
  const long nx = plan_search(pl, SearchIn{.lon_in = none, .lat_in = none, .lon_out = d_lon_out, .lat_out = d_lat_out, .mean_dlat = mean_dlat,
                                           .mean_dlon = mean_dlon, .rect_hint = rect_hint});
  return g.hand_over(nx, plan_out);
}

// ------------------------------------------------------------------------------------- great-circle polygon lists
// The tail of both entries: the list and the destination's unit vectors are on the device.  The search is gc_search's with the
// list in place of the source tiles (one pseudo-tile of npoly x 1 "cells" without corner arrays).
static long polylist_gc_search(fg_plan *pl, FgGcPolyList P, GcXyz out, DstExtents x)
{
  pl->gcpolys = P;
  const GcXyz gxyz[2] = {GcXyz{nullptr, nullptr, nullptr}, out};
  const long nx = gc_search(pl, gxyz, nullptr, x);
  pl->gcpolys = FgGcPolyList{nullptr, nullptr, nullptr, nullptr, nullptr, P.npoly};      // (the records hold all of it from here on)
  return nx;
}

// fg_plan_create_polylist_gc with every array on the device: n [npoly], x / y / z [npoly][8], area_ref [npoly], the destination
// corners as unit vectors; the arrays stay the caller's and must outlive the search only.  Extents <= 0: derived from a sample.
// use_caller_stream 0: a stream of the plan's own (the caller has finished writing the arrays), as fg_plan_create_great_circle_dev.
long fg_plan_create_polylist_gc_dev(int npoly, const int *d_n, const double *d_x, const double *d_y, const double *d_z, const double *d_area_ref,
                                    int nx_out, int ny_out, const double *d_x_out, const double *d_y_out, const double *d_z_out,
                                    double mean_dlat, double mean_dlon, int device, void *stream, int use_caller_stream, fg_plan **plan_out)
{
  if (npoly < 1 || !d_n || !d_x || !d_y || !d_z || !d_area_ref || !d_x_out || !d_y_out || !d_z_out) return fg_fail(FG_ERR_ARG, "null argument");
  PlanGuard g;
  const int one = 1;
  if (int rc = plan_base(FG_CONSERVE_ORDER1, 1, &npoly, &one, nx_out, ny_out, device, &g.pl)) return rc;
  if (use_caller_stream) adopt_stream(g.pl, stream);
  const long nx = polylist_gc_search(g.pl, FgGcPolyList{d_n, d_x, d_y, d_z, d_area_ref, npoly}, GcXyz{d_x_out, d_y_out, d_z_out},
                                     DstExtents{mean_dlat, mean_dlon});
  return g.hand_over(nx, plan_out);
}

// Host arrays; lon_out / lat_out in radians, converted on the host like fg_plan_create_great_circle.  A list of no polygons is
// searched as one polygon without vertices (it has no candidates): the plan then has one source "cell" and no exchange cell.
extern "C" long fg_plan_create_polylist_gc(int npoly, const int *n, const double *x, const double *y, const double *z, const double *area_ref,
                                           int nx_out, int ny_out, const double *lon_out, const double *lat_out, int device, fg_plan **plan_out)
{
  if (npoly < 0 || !lon_out || !lat_out || (npoly > 0 && (!n || !x || !y || !z || !area_ref))) return fg_fail(FG_ERR_ARG, "null argument");
  for (int k = 0; k < npoly; k++)
    if (n[k] < 0 || n[k] > 8) return fg_fail(FG_ERR_ARG, "fg_plan_create_polylist_gc: polygon %d has %d vertices (at most 8)", k, n[k]);
  PlanGuard g;
  const int one = 1, np1 = npoly > 0 ? npoly : 1;
  if (int rc = plan_base(FG_CONSERVE_ORDER1, 1, &np1, &one, nx_out, ny_out, device, &g.pl)) return rc;
  fg_plan *pl = g.pl;
  static const int n_none[1] = {0};
  static const double v_none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (npoly == 0) { n = n_none; x = y = z = v_none; area_ref = v_none; }
  const size_t npo = (size_t)(nx_out + 1) * (ny_out + 1);
  std::vector<double> h(3 * npo);                       // x | y | z of the destination corners
  fg_latlon2xyz((long)npo, lon_out, lat_out, h.data(), h.data() + npo, h.data() + 2 * npo);
  HostUpload up{pl};
  const FgGcPolyList P{up.put(n, np1), up.put(x, (size_t)np1 * 8), up.put(y, (size_t)np1 * 8), up.put(z, (size_t)np1 * 8), up.put(area_ref, np1), np1};
  double *d_o = up.put(h.data(), 3 * npo);
  if (!up.run()) return fg_fail(FG_ERR_HIP, "polygon upload failed (out of device memory?)");
  const long nx = polylist_gc_search(pl, P, GcXyz{d_o, d_o + npo, d_o + 2 * npo}, dst_extents_host(nx_out, ny_out, lon_out, lat_out));
  if (nx >= 0) up.done();
  return g.hand_over(nx, plan_out);
}

extern "C" int fg_plan_set_stream(fg_plan *pl, void *stream)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null plan");
  FGCHK(hipSetDevice(pl->device));
  FGCHK(hipStreamSynchronize(pl->stream));
  adopt_stream(pl, stream);
  return 0;
}

// Internal (sweep.hip): run the plan's launches on `stream` for the duration of one call and hand the previous stream back
// afterwards.  borrow: waits for the plan's own stream, then points it at `stream`; *saved / *saved_own receive what it had.
// give back: the caller has synchronised `stream`.  The plan never owns a borrowed stream.
int fg_plan_borrow_stream(fg_plan *pl, void *stream, void **saved, int *saved_own)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null plan");
  FGCHK(hipSetDevice(pl->device));
  FGCHK(hipStreamSynchronize(pl->stream));
  *saved = (void *)pl->stream; *saved_own = pl->own_stream ? 1 : 0;
  pl->stream = (hipStream_t)stream; pl->own_stream = false;
  return 0;
}
void fg_plan_return_stream(fg_plan *pl, void *saved, int saved_own)
{
  if (!pl) return;
  pl->stream = (hipStream_t)saved; pl->own_stream = saved_own != 0;
}

// a plan without a search: exchange cells are supplied later by fg_plan_set_xgrid
extern "C" int fg_plan_create_empty(int order, int ntiles_in, const int *nx_in, const int *ny_in,
                                    int nx_out, int ny_out, int device, fg_plan **plan_out)
{
  PlanGuard g;
  if (int rc = plan_base(order, ntiles_in, nx_in, ny_in, nx_out, ny_out, device, &g.pl)) return rc;
  fg_plan *pl = g.pl;
  std::vector<FgTile> th(pl->ntiles);
  for (int m = 0; m < pl->ntiles; m++) th[m] = FgTile{nullptr, nullptr, pl->nx_in[m], pl->ny_in[m], pl->cell_off[m]};
  pl->tiles_dev = pl->alloc<FgTile>(pl->ntiles + 1);
  if (!pl->tiles_dev || hipMemcpy(pl->tiles_dev, th.data(), sizeof(FgTile) * th.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fg_fail(FG_ERR_HIP, "out of device memory");
  return (int)g.hand_over(0, plan_out);
}

// The search sizes the exchange-cell arrays by capacity (8*max(nsrc, ndst) entries), about twice what a remap between grids of
// similar resolution fills.  A caller that keeps many plans (one per output tile or variable set) can give the surplus back:
// the arrays are re-allocated at nxgrid entries (device-to-device copies, ~0.1 ms at C384 -> 0.25 deg).
extern "C" int fg_plan_trim(fg_plan *pl)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null plan");
  if (!pl->searched) return fg_fail(FG_ERR_STATE, "fg_plan_trim: plan holds no exchange cells");
  FGCHK(hipSetDevice(pl->device));
  FGCHK(hipStreamSynchronize(pl->stream));
  const size_t n = (size_t)pl->nx + 1;
  auto shrink = [&](auto *&ptr) -> int {
    if (!ptr) return 0;
    typedef typename std::remove_reference<decltype(*ptr)>::type T;
    T *q = pl->alloc<T>(n);
    if (!q) return fg_fail(FG_ERR_HIP, "out of device memory");
    if (hipMemcpyAsync(q, ptr, n * sizeof(T), hipMemcpyDeviceToDevice, pl->stream) != hipSuccess) return fg_fail(FG_ERR_HIP, "device copy failed");
    void *old = ptr; ptr = q;
    FGCHK(hipStreamSynchronize(pl->stream));
    pl->release(old);
    return 0;
  };
  int rc = 0;
  if ((rc = shrink(pl->x_src)) || (rc = shrink(pl->x_dst)) || (rc = shrink(pl->x_area)) || (rc = shrink(pl->x_c1)) || (rc = shrink(pl->x_c2))) return rc;
  if (pl->perm && (rc = shrink(pl->perm))) return rc;
  return 0;
}

extern "C" long fg_plan_nxgrid(const fg_plan *pl) { return pl ? pl->nx : FG_ERR_ARG; }
extern "C" long fg_plan_ncells_in(const fg_plan *pl) { return pl ? pl->nsrc : FG_ERR_ARG; }
extern "C" long fg_plan_ncells_out(const fg_plan *pl) { return pl ? pl->ndst : FG_ERR_ARG; }
extern "C" int fg_plan_order(const fg_plan *pl) { return pl ? pl->order : FG_ERR_ARG; }
extern "C" int fg_plan_device(const fg_plan *pl) { return pl ? pl->device : FG_ERR_ARG; }
extern "C" double *fg_plan_cell_sums_dev(fg_plan *pl) { return (pl && pl->order == 2) ? pl->sums : nullptr; }
extern "C" int fg_plan_copy_cell_sums(fg_plan *pl, double *dst_dev)
{
  if (!pl || !dst_dev) return fg_fail(FG_ERR_ARG, "null argument");
  if (pl->order != 2 || !pl->sums) return fg_fail(FG_ERR_STATE, "plan holds no order-2 cell sums");
  FGCHK(hipSetDevice(pl->device));
  FGCHK(hipMemcpyAsync(dst_dev, pl->sums, 3 * (size_t)pl->nsrc * sizeof(double), hipMemcpyDeviceToDevice, pl->stream));
  FGCHK(hipStreamSynchronize(pl->stream));
  return 0;
}
// total_dev[3][ncells_in] (sum of area, of the clon integral, of the clat integral per source cell) += this plan's exchange cells,
// added one by one in exchange-cell order onto what total_dev already holds; cells_dev (may be null = all) restricts it to a list
// of source cells.  Before fg_plan_finalize only.
static int accumulate_cell_sums(fg_plan *pl, double *total_dev, const int *cells_dev, int ncells, bool sync)
{
  if (!pl || !total_dev) return fg_fail(FG_ERR_ARG, "null argument");
  if (pl->order != 2 || !pl->searched || pl->finalized || !pl->xoff)
    return fg_fail(FG_ERR_STATE, "fg_plan_accumulate_cell_sums: needs a searched, not yet finalized order-2 plan");
  FGCHK(hipSetDevice(pl->device));
  if (pl->nx > 0)
    fgd_accumulate_cell_sums(cells_dev ? ncells : pl->nsrc, cells_dev, pl->nsrc, pl->xoff, pl->x_area, pl->x_c1, pl->x_c2, total_dev, pl->stream);
  if (sync) FGCHK(hipStreamSynchronize(pl->stream));
  FGCHK(hipGetLastError());
  return 0;
}
extern "C" int fg_plan_accumulate_cell_sums(fg_plan *pl, double *total_dev, const int *cells_dev, int ncells)
{
  return accumulate_cell_sums(pl, total_dev, cells_dev, ncells, true);
}
// the same, only queued on the plan's stream: for callers that put the plan on the stream their other device work is ordered on
// (fg_plan_set_stream / the stream argument of fg_plan_create_dev), so that a rank-to-rank hand-over needs no host round trip
extern "C" int fg_plan_accumulate_cell_sums_async(fg_plan *pl, double *total_dev, const int *cells_dev, int ncells)
{
  return accumulate_cell_sums(pl, total_dev, cells_dev, ncells, false);
}
extern "C" void *fg_plan_stream(fg_plan *pl) { return pl ? (void *)pl->stream : nullptr; }
extern "C" int fg_plan_sync(fg_plan *pl)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null plan");
  FGCHK(hipStreamSynchronize(pl->stream));
  return 0;
}
extern "C" int fg_plan_stats(const fg_plan *pl, long *stats, int n)
{
  if (!pl || !stats) return fg_fail(FG_ERR_ARG, "null argument");
  for (int k = 0; k < n && k < FG_NSTATS; k++) stats[k] = pl->stats[k];
  return 0;
}

// Destination-row CSR.  A searched plan arrives with row_ptr and perm (rows grouped, unsorted inside a row) already built on
// the device by the search; a plan loaded from a remap file (fg_plan_set_xgrid) counts and fills its rows here.
// cen != null: order 2, x_c1/x_c2 hold the centroid integrals and di/dj are formed while the records are packed.
// The two-call finalize without its host wait: a stream-ordered plan (fg_plan::async) on a stream the CALLER supplied, profiling
// off.  The caller orders its own buffers on that stream (total_cell_sums_dev must outlive k_centroids there, as the comment on
// fg_plan_accumulate_cell_sums_async says of the sums).  A plan-owned stream keeps the wait: the caller has no way to order
// total_cell_sums_dev behind it.  What is left in flight is what fg_plan's invariant names.
static bool finalize_stream_ordered(const fg_plan *pl) { return pl->async && !pl->own_stream && !g_profiling; }
static int build_csr(fg_plan *pl, const FgSrcRec *cen)
{
  struct OnStream {                                    // its blocks are first touched on the plan's stream (fg_plan::on_stream)
    fg_plan *pl; bool was;
    ~OnStream() { pl->on_stream = was; }
  } on_stream{pl, pl->on_stream};
  pl->on_stream = pl->async;
  hipStream_t st = pl->stream;
  const int ndst = pl->ndst;
  const long nx = pl->nx;
  FGCHK(hipSetDevice(pl->device));
  if (!pl->src_idx_f) {
    pl->src_idx_f = pl->alloc<int>(pl->nsrc + 1);
    if (!pl->src_idx_f) return fg_fail(FG_ERR_HIP, "out of device memory");
    fgd_src_field_index(pl->order, pl->tiles_dev, pl->ntiles, pl->nsrc, pl->src_idx_f, st);
  }
  void *scratch = nullptr;
  if (!pl->rows_built) {
    const long t_rows = fgd_scan_tiles(ndst);
    const size_t zb = 256 + (size_t)t_rows * sizeof(unsigned long long) + 2 * ((size_t)ndst + 1) * sizeof(int);
    char *z = pl->alloc<char>(zb);                                    // [ticket, total, err | look-back words | counts | fill cursors]
    pl->perm = pl->alloc<FgRowEnt>(nx + 1);
    pl->csr.row_ptr = pl->alloc<int>(ndst + 1);
    if (!z || !pl->perm || !pl->csr.row_ptr) return fg_fail(FG_ERR_HIP, "out of device memory");
    FGCHK(hipMemsetAsync(z, 0, zb, st));
    unsigned long long *lb = (unsigned long long *)(z + 256);
    int *row_cnt = (int *)(z + 256 + (size_t)t_rows * sizeof(unsigned long long));
    fgd_csr_count(nx, pl->x_dst, row_cnt, st);
    fgd_exclusive_scan1(row_cnt, ndst, pl->csr.row_ptr, lb, (unsigned *)z, (unsigned long long *)(z + 8), (unsigned *)(z + 16), st);
    fgd_csr_fill(nx, pl->x_src, pl->x_dst, pl->csr.row_ptr, row_cnt + ndst + 1, pl->perm, st);
    scratch = z;
  }
  if (pl->order == 2) pl->csr.e2 = pl->alloc<FgCsrEntry2>(nx + 1);
  else pl->csr.e1 = pl->alloc<FgCsrEntry1>(nx + 1);
  if (!pl->csr.e1 && !pl->csr.e2) return fg_fail(FG_ERR_HIP, "out of device memory");
  // rows longer than the kernel's LDS staging are sorted through this -- also in plans whose MEAN row is short: the cells around a
  // pole of a cubed-sphere target hold a whole row of a lat-lon source each (1 440 exchange cells: a lane sorting that by insertion
  // took 17 ms)
  int *sg_tmp = pl->alloc<int>(3 * (size_t)(nx + 1));
  // a curvilinear target with cells that went to the general clip (pole vertices): its rows round the pole are long -- hundreds of
  // exchange cells -- under a mean of 6.6, and the 64-rows-per-wave mode ranks them one after another (0.25 deg -> C384 tile 3:
  // 0.23 ms of the tile's 1.1); the 16-rows-per-block mode costs the short rows of such a tile little
  const int long_rows = !pl->rect && !pl->great_circle && pl->stats[FG_STAT_DEFERRED] > 0 && nx > 4 * (long)ndst;
  fgd_csr_sortgather(pl->order, ndst, nx, pl->perm, pl->x_area, pl->x_c1, pl->x_c2, pl->src_idx_f, cen, pl->csr, st, sg_tmp, nx + 1,
                     long_rows);
  if (finalize_stream_ordered(pl)) {                   // the wait was for these three blocks only: they go back tagged instead
    pl->release_on_stream({scratch, pl->perm, sg_tmp});
  } else {
    FGCHK(hipStreamSynchronize(st));
    pl->release(scratch); pl->release(pl->perm); pl->release(sg_tmp);
  }
  pl->perm = nullptr;
  FGCHK(hipGetLastError());
  if (!pl->red_partial) { pl->red_partial = pl->alloc<double>(1024); pl->red_result = pl->alloc<double>(260); }
  if (!pl->red_partial || !pl->red_result) return fg_fail(FG_ERR_HIP, "out of device memory");
  return 0;
}

extern "C" int fg_plan_finalize(fg_plan *pl, const double *total_cell_sums_dev)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null plan");
  if (!pl->searched) return fg_fail(FG_ERR_STATE, "fg_plan_finalize: plan holds no search result");
  if (pl->finalized && pl->fused && !total_cell_sums_dev) return 0;         // its search did it (fg_set_search_finalize)
  if (pl->finalized) return fg_fail(FG_ERR_STATE, pl->fused ? "fg_plan_finalize: the plan was finalized by its search (fg_set_search_finalize) from its own "
                                                          "per-cell sums; totals over several plans need the two-step sequence"
                                                         : "fg_plan_finalize: already finalized");
  FGCHK(hipSetDevice(pl->device));
  PhaseTimer pt; pt.start(g_profiling != 0, pl->stream);
  pt.begin(PH_FINALIZE);
  if (pl->order == 2) {
    // (first touched by k_centroids on the plan's stream: taken in stream order like build_csr's blocks -- a stream-less request
    // would wait on the host for the block the previous plan gave back tagged, with the GPU idle: 10-20 us per finalize)
    pl->on_stream = pl->async;
    pl->cen = pl->alloc<FgSrcRec>((size_t)pl->nsrc + 1);
    pl->on_stream = false;
    if (!pl->cen) return fg_fail(FG_ERR_HIP, "out of device memory");
    const double *tot = total_cell_sums_dev ? total_cell_sums_dev : pl->sums;
    fgd_centroids(pl->nsrc, pl->S, tot, pl->cen, pl->stream);
    pl->dist_pending = true;                 // the CSR records get di/dj now; the exchange-cell arrays when somebody asks for them
  }
  int rc = build_csr(pl, pl->order == 2 ? pl->cen : nullptr);
  if (rc) return rc;
  pt.end();
  if (!finalize_stream_ordered(pl)) FGCHK(hipStreamSynchronize(pl->stream));
  pl->phase_ms[PH_FINALIZE] = 0; pt.collect(pl->phase_ms);
  pl->finalized = true;
  return 0;
}

// phase times (ms) of the last search/finalize/apply when fg_set_profiling(1) was active:
// [0] cell records [1] binning [2] candidates [3] clip quad [4] clip general [5] compaction
// [6] destination rows [7] whole search (device span) [8] finalize [9] last apply
extern "C" int fg_plan_phase_ms(fg_plan *pl, float *ms, int n)
{
  if (!pl || !ms) return fg_fail(FG_ERR_ARG, "null argument");
  if (pl->apply_spans > 0) {               // sweeps are timed without a sync; average them now
    FGCHK(hipSetDevice(pl->device));
    FGCHK(hipStreamSynchronize(pl->stream));
    float acc[PH_COUNT] = {0};
    pl->apply_pt.collect(acc);
    pl->phase_ms[PH_APPLY] = acc[PH_APPLY] / pl->apply_spans;
    pl->apply_spans = 0;
  }
  for (int k = 0; k < n && k < PH_COUNT; k++) ms[k] = pl->phase_ms[k];
  return 0;
}

extern "C" int fg_plan_get_xgrid(const fg_plan *pl, int *t_in, int *i_in, int *j_in, int *i_out, int *j_out,
                                 double *area, double *c1, double *c2)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null plan");
  if (!pl->searched) return fg_fail(FG_ERR_STATE, "plan holds no exchange cells");
  FGCHK(hipSetDevice(pl->device));
  FGCHK(hipStreamSynchronize(pl->stream));
  const long nx = pl->nx;
  if (nx == 0) return 0;
  if (pl->dist_pending) {                     // di = clon/area - centroid (conserve_interp.c:256-257,355-356), on first use
    fg_plan *m = const_cast<fg_plan *>(pl);
    fgd_distances(nx, pl->x_src, pl->x_area, pl->cen, m->x_c1, m->x_c2, pl->stream);
    FGCHK(hipStreamSynchronize(pl->stream));
    m->dist_pending = false;
  }
  std::vector<XferJob> jobs;
  int *idx = nullptr;
  struct PutBack { int *&p; ~PutBack() { g_pool.put(p); } } put_back{idx};
  if (t_in || i_in || j_in || i_out || j_out) {
    // index decomposition on the device (the host loop with two divisions per exchange cell took longer than the transfer)
    idx = (int *)g_pool.get(pl->device, 5 * (size_t)nx * sizeof(int));
    if (!idx) return fg_fail(FG_ERR_HIP, "out of device memory");
    fgd_xgrid_indices(nx, pl->x_src, pl->x_dst, pl->tiles_dev, pl->ntiles, pl->nx_out, idx, idx + nx, idx + 2 * nx, idx + 3 * nx,
                      idx + 4 * nx, pl->stream);
    FGCHK(hipStreamSynchronize(pl->stream));
    int *dst[5] = {t_in, i_in, j_in, i_out, j_out};
    for (int q = 0; q < 5; q++) if (dst[q]) jobs.push_back(XferJob{dst[q], idx + (size_t)q * nx, (size_t)nx * sizeof(int), true});
  }
  if (area) jobs.push_back(XferJob{area, pl->x_area, (size_t)nx * sizeof(double), true});
  if (pl->order == 2) {
    if (c1) jobs.push_back(XferJob{c1, pl->x_c1, (size_t)nx * sizeof(double), true});
    if (c2) jobs.push_back(XferJob{c2, pl->x_c2, (size_t)nx * sizeof(double), true});
  }
  if (!xfer_pool().run(pl->device, jobs)) return fg_fail(FG_ERR_HIP, "fg_plan_get_xgrid: device -> host copy failed");
  return 0;
}

// The clipped polygon of every exchange cell (canonical order): n_out[nx] vertex counts and [nx][maxv] vertex arrays -- legacy
// plans: v0 = lon, v1 = lat (v2 unused, may be null); great-circle plans: v0, v1, v2 = x, y, z.  Host arrays.  What clip_2dx2d /
// clip_2dx2d_great_circle returned for the pair inside create_xgrid (make_coupler_mosaic.c:1560-1577 keeps exactly these).
extern "C" int fg_plan_get_polygons(const fg_plan *pl, int maxv, int *n_out, double *v0, double *v1, double *v2)
{
  if (!pl || !n_out || !v0 || !v1) return fg_fail(FG_ERR_ARG, "null argument");
  if (!pl->searched || !pl->have_geom || !pl->x_src) return fg_fail(FG_ERR_STATE, "fg_plan_get_polygons: needs a plan from a search (cell records)");
  if (pl->great_circle && !v2) return fg_fail(FG_ERR_ARG, "fg_plan_get_polygons: a great-circle plan returns x, y, z");
  if (maxv < 3 || maxv > 64) return fg_fail(FG_ERR_ARG, "fg_plan_get_polygons: maxv must be 3..64");
  FGCHK(hipSetDevice(pl->device));
  FGCHK(hipStreamSynchronize(pl->stream));
  const long nx = pl->nx, CH = 1L << 20;
  const int dev = pl->device;
  for (long k0 = 0; k0 < nx; k0 += CH) {
    const long n = std::min(CH, nx - k0);
    const size_t nv = (size_t)n * maxv;
    int *d_n = (int *)g_pool.get(dev, n * sizeof(int));
    double *d_v = (double *)g_pool.get(dev, 3 * nv * sizeof(double));
    struct Put { void *a, *b; ~Put() { g_pool.put(a); g_pool.put(b); } } put{d_n, d_v};
    if (!d_n || !d_v) return fg_fail(FG_ERR_HIP, "out of device memory");
    std::vector<XferJob> jobs;
    if (pl->great_circle && pl->gc_prec) {            // a polygon list: the n-gon clip on the plan's records
      double *o = (double *)g_pool.get(dev, (size_t)n * FG_GC_POLY_CAP * 3 * 8);
      struct Put1 { void *p; ~Put1() { g_pool.put(p); } } put1{o};
      if (!o) return fg_fail(FG_ERR_HIP, "out of device memory");
      fgd_gc_poly_polygons(n, pl->x_src + k0, pl->x_dst + k0, pl->S.nv, pl->gc_prec, pl->D, o, d_n, pl->stream);
      fgd_split_xyz(n, maxv, o, d_v, d_v + nv, d_v + 2 * nv, pl->stream);
      FGCHK(hipStreamSynchronize(pl->stream));
      jobs.push_back(XferJob{v2 + (size_t)k0 * maxv, d_v + 2 * nv, nv * sizeof(double), true});
    } else if (pl->great_circle) {
      double *a = (double *)g_pool.get(dev, (size_t)n * 12 * 8), *b = (double *)g_pool.get(dev, (size_t)n * 12 * 8);
      double *o = (double *)g_pool.get(dev, (size_t)n * FG_GC_POLY_CAP * 3 * 8), *ar = (double *)g_pool.get(dev, (size_t)n * 8);
      struct Put4 { void *p[4]; ~Put4() { for (void *q : p) g_pool.put(q); } } put4{{a, b, o, ar}};
      if (!a || !b || !o || !ar) return fg_fail(FG_ERR_HIP, "out of device memory");
      fgd_xgrid_gather_gc(n, pl->x_src + k0, pl->x_dst + k0, pl->S, pl->D, a, b, pl->stream);
      fgd_gc_clip_batch((int)n, a, b, o, d_n, ar, pl->stream);
      fgd_split_xyz(n, maxv, o, d_v, d_v + nv, d_v + 2 * nv, pl->stream);
      FGCHK(hipStreamSynchronize(pl->stream));
      jobs.push_back(XferJob{v2 + (size_t)k0 * maxv, d_v + 2 * nv, nv * sizeof(double), true});
    } else {
      fgd_xgrid_polygons(n, pl->x_src + k0, pl->x_dst + k0, pl->S, pl->D, pl->rect ? &pl->rect_tab : nullptr, maxv, d_n, d_v, d_v + nv, pl->stream);
      FGCHK(hipStreamSynchronize(pl->stream));
    }
    FGCHK(hipGetLastError());
    jobs.push_back(XferJob{n_out + k0, d_n, (size_t)n * sizeof(int), true});
    jobs.push_back(XferJob{v0 + (size_t)k0 * maxv, d_v, nv * sizeof(double), true});
    jobs.push_back(XferJob{v1 + (size_t)k0 * maxv, d_v + nv, nv * sizeof(double), true});
    if (!xfer_pool().run(dev, jobs)) return fg_fail(FG_ERR_HIP, "fg_plan_get_polygons: device -> host copy failed");
  }
  return 0;
}

extern "C" int fg_plan_get_cell_area(const fg_plan *pl, double *area_in, double *area_out)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null plan");
  if (!pl->have_geom) return fg_fail(FG_ERR_STATE, "plan holds no cell records");
  FGCHK(hipSetDevice(pl->device));
  FGCHK(hipStreamSynchronize(pl->stream));
  if (area_in) FGCHK(hipMemcpy(area_in, pl->S.area, (size_t)pl->nsrc * sizeof(double), hipMemcpyDeviceToHost));
  if (area_out) FGCHK(hipMemcpy(area_out, pl->D.area, (size_t)pl->ndst * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// per-cell records of the source (which = 0) or destination (which = 1) cells, for the
// get_grid_cell_struct parity test.  Host arrays; vlon/vlat are [ncells][8].
extern "C" int fg_plan_get_cell_struct(const fg_plan *pl, int which, double *lat_min, double *lat_max, double *lon_min,
                                       double *lon_max, double *lon_avg, int *nvert, double *vlon, double *vlat)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null plan");
  if (!pl->have_geom) return fg_fail(FG_ERR_STATE, "plan holds no cell records");
  FGCHK(hipSetDevice(pl->device));
  FGCHK(hipStreamSynchronize(pl->stream));
  FgCells tmp{};
  std::vector<void *> tmp_blocks;
  struct Free { std::vector<void *> &v; ~Free() { for (void *p : v) g_pool.put(p); } } free_tmp{tmp_blocks};
  if (which && pl->rect) {                       // a rectilinear plan keeps tables, not records: spell them out for the caller
    const size_t nd = (size_t)pl->ndst;
    auto get = [&](size_t bytes) { void *p = g_pool.get(pl->device, bytes); if (p) tmp_blocks.push_back(p); return p; };
    tmp.lat_min = (double *)get(nd * 8); tmp.lat_max = (double *)get(nd * 8); tmp.lon_min = (double *)get(nd * 8);
    tmp.lon_max = (double *)get(nd * 8); tmp.lon_avg = (double *)get(nd * 8); tmp.nv = (int *)get(nd * 4); tmp.verts = (double *)get(nd * 128);
    tmp.area = pl->D.area;
    if (tmp_blocks.size() != 7) return fg_fail(FG_ERR_HIP, "out of device memory");
    FgRect R = pl->rect_tab;
    fgd_rect_materialize(pl->ndst, R, tmp, pl->stream);
    FGCHK(hipStreamSynchronize(pl->stream));
  }
  if (!which && pl->S.vstride == FG_VSTRIDE_QUAD) {   // compact source cells: the boxes' longitudes and the 128-byte records likewise
    const size_t ns = (size_t)pl->nsrc;
    auto get = [&](size_t bytes) { void *p = g_pool.get(pl->device, bytes); if (p) tmp_blocks.push_back(p); return p; };
    tmp = pl->S;
    tmp.lon_min = (double *)get(ns * 8); tmp.lon_max = (double *)get(ns * 8); tmp.verts = (double *)get(ns * 128);
    tmp.vstride = 16; tmp.wide = nullptr; tmp.wide_cap = 0;
    if (tmp_blocks.size() != 3) return fg_fail(FG_ERR_HIP, "out of device memory");
    fgd_quad_materialize(pl->nsrc, pl->S, tmp.lon_min, tmp.lon_max, tmp.verts, pl->stream);
    FGCHK(hipStreamSynchronize(pl->stream));
  }
  const FgCells &c = which ? (pl->rect ? tmp : pl->D) : (pl->S.vstride == FG_VSTRIDE_QUAD ? tmp : pl->S);
  size_t n = which ? pl->ndst : pl->nsrc;
  if (lat_min) FGCHK(hipMemcpy(lat_min, c.lat_min, n * sizeof(double), hipMemcpyDeviceToHost));
  if (lat_max) FGCHK(hipMemcpy(lat_max, c.lat_max, n * sizeof(double), hipMemcpyDeviceToHost));
  if (lon_min) FGCHK(hipMemcpy(lon_min, c.lon_min, n * sizeof(double), hipMemcpyDeviceToHost));
  if (lon_max) FGCHK(hipMemcpy(lon_max, c.lon_max, n * sizeof(double), hipMemcpyDeviceToHost));
  if (lon_avg) FGCHK(hipMemcpy(lon_avg, c.lon_avg, n * sizeof(double), hipMemcpyDeviceToHost));
  if (nvert) FGCHK(hipMemcpy(nvert, c.nv, n * sizeof(int), hipMemcpyDeviceToHost));
  if (vlon || vlat) {
    std::vector<double> v(n * 16);
    FGCHK(hipMemcpy(v.data(), c.verts, n * 16 * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; k++)
      for (int l = 0; l < 8; l++) {
        if (vlon) vlon[k * 8 + l] = v[k * 16 + l];
        if (vlat) vlat[k * 8 + l] = v[k * 16 + 8 + l];
      }
  }
  return 0;
}

extern "C" int fg_plan_set_xgrid(fg_plan *pl, long nxgrid, const int *t_in, const int *i_in, const int *j_in,
                                 const int *i_out, const int *j_out, const double *area,
                                 const double *di_in, const double *dj_in)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null plan");
  if (nxgrid < 0 || (nxgrid > 0 && (!t_in || !i_in || !j_in || !i_out || !j_out || !area))) return fg_fail(FG_ERR_ARG, "null exchange-cell array");
  if (pl->order == 2 && nxgrid > 0 && (!di_in || !dj_in)) return fg_fail(FG_ERR_ARG, "order 2 needs di_in/dj_in");
  if (pl->finalized || pl->searched) return fg_fail(FG_ERR_STATE, "fg_plan_set_xgrid needs a plan from fg_plan_create_empty");
  FGCHK(hipSetDevice(pl->device));
  std::vector<int> s(nxgrid), d(nxgrid);
  for (long k = 0; k < nxgrid; k++) {
    int m = t_in[k];
    if (m < 0 || m >= pl->ntiles || i_in[k] < 0 || i_in[k] >= pl->nx_in[m] || j_in[k] < 0 || j_in[k] >= pl->ny_in[m] ||
        i_out[k] < 0 || i_out[k] >= pl->nx_out || j_out[k] < 0 || j_out[k] >= pl->ny_out)
      return fg_fail(FG_ERR_ARG, "exchange cell %ld has an index outside its grid", k);
    s[k] = pl->cell_off[m] + j_in[k] * pl->nx_in[m] + i_in[k];
    d[k] = j_out[k] * pl->nx_out + i_out[k];
  }
  pl->nx = nxgrid;
  pl->x_src = pl->alloc<int>(nxgrid + 1); pl->x_dst = pl->alloc<int>(nxgrid + 1);
  pl->x_area = pl->alloc<double>(nxgrid + 1);
  if (pl->order == 2) { pl->x_c1 = pl->alloc<double>(nxgrid + 1); pl->x_c2 = pl->alloc<double>(nxgrid + 1); }
  if (!pl->x_src || !pl->x_dst || !pl->x_area || (pl->order == 2 && (!pl->x_c1 || !pl->x_c2))) return fg_fail(FG_ERR_HIP, "out of device memory");
  if (nxgrid > 0) {
    FGCHK(hipMemcpy(pl->x_src, s.data(), nxgrid * sizeof(int), hipMemcpyHostToDevice));
    FGCHK(hipMemcpy(pl->x_dst, d.data(), nxgrid * sizeof(int), hipMemcpyHostToDevice));
    FGCHK(hipMemcpy(pl->x_area, area, nxgrid * sizeof(double), hipMemcpyHostToDevice));
    if (pl->order == 2) {
      FGCHK(hipMemcpy(pl->x_c1, di_in, nxgrid * sizeof(double), hipMemcpyHostToDevice));
      FGCHK(hipMemcpy(pl->x_c2, dj_in, nxgrid * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  pl->searched = true;
  int rc = build_csr(pl, nullptr);
  if (rc) return rc;
  pl->finalized = true;
  return 0;
}

extern int g_apply_vec, g_apply_ep;
extern "C" void fg_set_apply_ep(int on) { g_apply_ep = on ? 1 : 0; }     // tuning hook: entry-parallel 8-level sweep on records

extern int g_apply_xcd;
extern "C" void fg_set_apply_xcd(int on) { g_apply_xcd = on < 0 ? 0 : on; }       // tuning hook: tile -> XCD mapping of the sweep (0 identity, 1 banded, C >= 2 chunked)
extern "C" void fg_set_apply_vec(int v) { g_apply_vec = (v >= 4) ? 4 : (v >= 2 ? 2 : (v == 1 ? 1 : 0)); }   // tuning hook (scripts/)

// ------------------------------------------------------------------- what the apply entry points share
// the PH_APPLY span of one call's launches on stream st, for fg_plan_phase_ms
static void apply_span_begin(fg_plan *pl, hipStream_t st)
{
  pl->apply_pt.start(g_profiling != 0 && pl->apply_spans < 256, st);     // (a long sweep loop must not pile up timing events)
  pl->apply_pt.begin(PH_APPLY);
}
static void apply_span_end(fg_plan *pl)
{
  pl->apply_pt.end();
  if (pl->apply_pt.on) pl->apply_spans++;
}

// levels per source cell of the interleaved layouts that hold nz <= 8 levels
static int levels_pad(int nz) { return nz > 4 ? 8 : (nz > 2 ? 4 : 2); }

// Scratch of the sweeps.  A buffer is allocated by the first call that wants it and lives as long as the plan.
enum : unsigned {
  SC_IL = 1,            // il_out [cell][8] and the staged chunk: il_m (order 2, records) or il_f (order 1, [cell][8])
  SC_RS = 2,            // il_rs, the row sums of one launch: [cell][16] or [level <= 8][cell]
  SC_BITS = 4,          // lv_bits, order 2: a chunk's gradient-mask bits per source cell
  SC_XERR = 8,          // the error word
  SC_FA8 = 16,          // lx_fa: a chunk's per-level field_area [source cell][8]
  SC_MONO8 = 32,        // mono8_b: the limiter's bounds of a chunk
  SC_ROW_SUM = 64,      // row_sum [ndst], the one-level calls
  SC_MONO = 128         // mono_x, mono_b: the one-level limiter
};
template <typename T> static bool scratch_get(fg_plan *pl, T *&p, size_t n) { return p || (p = pl->alloc<T>(n)); }
static int apply_scratch(fg_plan *pl, unsigned want)
{
  const size_t ns = pl->nsrc, ns1 = pl->nsrc > 0 ? pl->nsrc : 1;
  bool ok = true;
  if (want & SC_IL)
    ok = scratch_get(pl, pl->il_out, (size_t)pl->ndst * 8) &&
         (pl->order == 2 ? scratch_get(pl, pl->il_m, ns * 24) : scratch_get(pl, pl->il_f, (size_t)pl->f_stride * 8));
  if (ok && (want & SC_BITS) && pl->order == 2) ok = scratch_get(pl, pl->lv_bits, ns1);
  if (ok && (want & SC_RS)) ok = scratch_get(pl, pl->il_rs, (size_t)pl->ndst * 16);
  if (ok && (want & SC_XERR)) ok = scratch_get(pl, pl->xerr, 4);
  if (ok && (want & SC_FA8)) ok = scratch_get(pl, pl->lx_fa, ns1 * 8);
  if (ok && (want & SC_MONO8)) ok = scratch_get(pl, pl->mono8_b, ns1 * 32);
  if (ok && (want & SC_ROW_SUM) && pl->row_sum_cap < pl->ndst) {
    pl->release(pl->row_sum);
    pl->row_sum = pl->alloc<double>(pl->ndst);
    pl->row_sum_cap = pl->row_sum ? pl->ndst : 0;
    ok = pl->row_sum != nullptr;
  }
  if (ok && (want & SC_MONO)) ok = scratch_get(pl, pl->mono_x, pl->nx > 0 ? pl->nx : 1) && scratch_get(pl, pl->mono_b, ns * 4);
  return ok ? 0 : fg_fail(FG_ERR_HIP, "out of device memory");
}

// levels [0, nbv) of the first-order field f (level-major, stride f_stride) -> il_f [f_stride][nbp]
static void interleave_field(fg_plan *pl, const double *f, int nbp, int nbv, hipStream_t st)
{
  const double *ins[3] = {f, nullptr, nullptr};
  double *outs[3] = {pl->il_f, nullptr, nullptr};
  const long lds[3] = {pl->f_stride, 0, 0}, ns[3] = {pl->f_stride, 0, 0};
  fgd_interleave3(nbp, 1, ins, lds, ns, outs, nbv, st);
}

// the error word of the sweeps that have one, read once the stream has drained
static int ex_error_word(fg_plan *pl)
{
  int e = 0;
  FGCHK(hipMemcpyAsync(&e, pl->xerr, sizeof(int), hipMemcpyDeviceToHost, pl->stream));
  FGCHK(hipStreamSynchronize(pl->stream));
  if (e & FG_XERR_AREA_MISSING) return fg_fail(FG_ERR_DATA, "conserve_interp: data is not missing but area is missing");
  if (e & FG_XERR_ABOVE) return fg_fail(FG_ERR_DATA, " xdata is greater than f_bar_max ");
  if (e & FG_XERR_BELOW) return fg_fail(FG_ERR_DATA, " xdata is less than f_bar_min ");
  return 0;
}

// the options as the kernels take them
static FgApplyEx ex_pack(fg_plan *pl, const fg_apply_opts *o, const int *gmask)
{
  FgApplyEx x{};
  x.weight = o->weight; x.field_area = o->field_area; x.cell_area_out = o->cell_methods_sum ? nullptr : o->cell_area_out;
  x.cell_area = o->cell_area_in ? o->cell_area_in : (pl->have_geom ? pl->S.area : nullptr);
  x.gmask = gmask; x.area_missing = o->area_missing;
  x.has_missing = o->has_missing; x.missing = o->has_missing ? o->missing : -1.e20;   // conserve_interp.c:541-542
  x.sum = o->cell_methods_sum;
  return x;
}

// cell_methods = sum and cell_measures need the source cells' areas
static int area_rule(const char *who, const fg_plan *pl, const fg_apply_opts *o)
{
  if ((o->cell_methods_sum || o->field_area) && !o->cell_area_in && !pl->have_geom)
    return fg_fail(FG_ERR_ARG, "%s: cell_area_in is required (this plan was loaded from a remap file and holds no cell areas)", who);
  return 0;
}

// The argument rules of the many-level entries.  An entry names those that apply to it; they are tested in the order written here,
// after the null pointers (null_arg) and the unfinalized plan.  null_late: a pointer the limiter's entries test after the area rule.
// o is read only by the rules that concern options.  Codes and texts are include/fregrid_hip.h's.
enum : unsigned {
  CK_NO_LIMITER = 1, CK_LIMITER = 2, CK_FA_LD = 4, CK_AREA = 8, CK_RECORDS = 16, CK_BITS = 32, CK_NLEV = 64, CK_NZ8 = 128, CK_NZ8_PAIR = 256,
  CK_BITS_IF_MISSING = 512, CK_GRADS = 1024, CK_GRADS_MASK = 2048
};
static int levels_check(const char *who, const fg_plan *pl, const fg_apply_opts *o, unsigned rules, bool null_arg, bool null_late, int nlev,
                        long fa_ld, bool grads, bool mask)
{
  const bool nz8 = nlev >= 1 && nlev <= 8;
  if (null_arg) return fg_fail(FG_ERR_ARG, "%s: null argument", who);
  if (!pl->finalized) return fg_fail(FG_ERR_ARG, "%s: the plan is not finalized (fg_plan_finalize)", who);
  if ((rules & CK_NO_LIMITER) && o->monotonic) return fg_fail(FG_ERR_ARG, "%s: the monotone limiter works on one level per call (fg_plan_apply_ex)", who);
  if ((rules & CK_LIMITER) && pl->order != 2) return fg_fail(FG_ERR_ARG, "%s: the monotone limiter belongs to conserve_order2 (conserve_interp.c:527-531)", who);
  if ((rules & CK_FA_LD) && fa_ld != 0 && fa_ld != pl->nsrc)
    return fg_fail(FG_ERR_ARG, "%s: field_area_ld must be 0 (one area for all levels) or ncells_in (an area per level)", who);
  if ((rules & CK_FA_LD) && fa_ld != 0 && !o->field_area) return fg_fail(FG_ERR_ARG, "%s: field_area_ld is set but opts->field_area is NULL", who);
  if (rules & CK_AREA) { if (int rc = area_rule(who, pl, o)) return rc; }
  if ((rules & CK_RECORDS) && pl->order != 2) return fg_fail(FG_ERR_ARG, "%s: records carry gradients, the plan is first order", who);
  if (null_late) return fg_fail(FG_ERR_ARG, "%s: null argument", who);
  if ((rules & CK_BITS) && !mask) return fg_fail(FG_ERR_ARG, "%s: order 2 needs the gradient-mask bits", who);
  if ((rules & CK_NLEV) && nlev < 1) return fg_fail(FG_ERR_ARG, "%s: nlev must be >= 1", who);
  if ((rules & CK_NZ8) && !nz8) return fg_fail(FG_ERR_ARG, "%s: 1 to 8 levels per call", who);
  if ((rules & CK_NZ8_PAIR) && !nz8) return fg_fail(FG_ERR_ARG, "%s: 1 to 8 levels per begin / end pair", who);
  if ((rules & CK_BITS_IF_MISSING) && o->has_missing && !mask) return fg_fail(FG_ERR_ARG, "%s: a field with missing values needs the gradient-mask bits", who);
  if ((rules & CK_GRADS) && pl->order == 2 && !grads) return fg_fail(FG_ERR_ARG, "%s: order 2 needs grad_x and grad_y [nlev][ncells_in]", who);
  if ((rules & CK_GRADS_MASK) && pl->order == 2 && !(grads && mask))
    return fg_fail(FG_ERR_ARG, "%s: order 2 needs grad_x, grad_y and grad_mask [nlev][ncells_in]", who);
  return 0;
}

extern "C" int fg_plan_apply(fg_plan *pl, const double *data, const double *grad_x, const double *grad_y,
                             const int *grad_mask, int has_missing, double missing, int nz,
                             double *out, double *gsum_out)
{
  if (!pl || !data || !out) return fg_fail(FG_ERR_ARG, "null argument");
  if (!pl->finalized) return fg_fail(FG_ERR_STATE, "fg_plan_apply: call fg_plan_finalize first");
  if (nz < 1) return fg_fail(FG_ERR_ARG, "nz must be >= 1");
  if (nz > 1 && has_missing) return fg_fail(FG_ERR_ARG, "conserve_interp: has_missing should be false when nz > 1");
  if (pl->order == 2 && (!grad_x || !grad_y)) return fg_fail(FG_ERR_ARG, "order 2 needs grad_x and grad_y");
  if (pl->order == 2 && has_missing && !grad_mask) return fg_fail(FG_ERR_ARG, "order 2 with missing values needs grad_mask");
  FGCHK(hipSetDevice(pl->device));
  hipStream_t st = pl->stream;
  const double miss = has_missing ? missing : -1.e20;            // conserve_interp.c:541-542
  const int ndst = pl->ndst;
  const int nchunk = (nz + 7) / 8;
  if (nchunk > 256) return fg_fail(FG_ERR_ARG, "nz too large for one call (max 2048 levels)");
  { int rc = apply_scratch(pl, (gsum_out ? SC_ROW_SUM : 0) | (nz > 1 ? SC_IL : 0) | (nz > 1 && gsum_out ? SC_RS : 0)); if (rc) return rc; }
  apply_span_begin(pl, st);
  int nred = 0;
  for (int k0 = 0; k0 < nz; k0 += 8) {
    const int nbv = (nz - k0 < 8) ? nz - k0 : 8;
    const double *f = data + (size_t)k0 * pl->f_stride;
    const double *gx = grad_x ? grad_x + (size_t)k0 * pl->nsrc : nullptr;
    const double *gy = grad_y ? grad_y + (size_t)k0 * pl->nsrc : nullptr;
    double *o = out + (size_t)k0 * ndst;
    if (nbv == 1) {
      fgd_apply1(pl->order, ndst, pl->csr, f, gx, gy, grad_mask, has_missing, miss, o, gsum_out ? pl->row_sum : nullptr, st, pl->nx);
      if (gsum_out) fgd_reduce_sum(pl->row_sum, ndst, pl->red_partial, pl->red_result + nred++, st);
    } else {
      const int nbp = levels_pad(nbv);
      double *rs = gsum_out ? pl->il_rs : nullptr;
      if (pl->order == 2) {
        // field + gradients of the chunk -> one record per source cell, then the sweep writes level-major directly
        fgd_merge3(nbp, pl->nsrc, pl->src_idx_f, f, pl->f_stride, gx, gy, pl->nsrc, nbv, pl->il_m, st);
        fgd_apply_il_merged(nbp, ndst, pl->nx, pl->csr, pl->il_m, miss, o, rs, (long)ndst, nbv, st);
      } else {
        interleave_field(pl, f, nbp, nbv, st);
        fgd_apply_il(1, nbp, ndst, pl->csr, pl->il_f, nullptr, nullptr, miss, o, rs, (long)ndst, nbv, st, pl->nx);
      }
      if (gsum_out) fgd_reduce_sum(pl->il_rs, (long)ndst * nbp, pl->red_partial, pl->red_result + nred++, st);
    }
  }
  apply_span_end(pl);
  if (gsum_out) {
    double parts[256];
    FGCHK(hipMemcpyAsync(parts, pl->red_result, nred * sizeof(double), hipMemcpyDeviceToHost, st));
    FGCHK(hipStreamSynchronize(st));
    double g = 0;
    for (int k = 0; k < nred; k++) g += parts[k];
    *gsum_out = g;
  }
  FGCHK(hipGetLastError());
  return 0;
}

// The order-2 sweep on records made by fg_c2l_gradient_records: no level-major detour, no merge pass.
extern "C" int fg_plan_apply_records(fg_plan *pl, int nz, const double *rec, double *out, double *gsum_out)
{
  if (!pl || !rec || !out) return fg_fail(FG_ERR_ARG, "null argument");
  if (!pl->finalized) return fg_fail(FG_ERR_STATE, "fg_plan_apply_records: call fg_plan_finalize first");
  if (pl->order != 2) return fg_fail(FG_ERR_ARG, "fg_plan_apply_records: records carry gradients, the plan is first order");
  if (nz < 1 || nz > 8) return fg_fail(FG_ERR_ARG, "fg_plan_apply_records: 1 to 8 levels per call");
  FGCHK(hipSetDevice(pl->device));
  hipStream_t st = pl->stream;
  const int ndst = pl->ndst, nbp = levels_pad(nz);
  { int rc = apply_scratch(pl, gsum_out ? SC_RS : 0); if (rc) return rc; }
  apply_span_begin(pl, st);
  fgd_apply_il_merged(nbp, ndst, pl->nx, pl->csr, rec, -1.e20, out, gsum_out ? pl->il_rs : nullptr, (long)ndst, nz, st);
  if (gsum_out) fgd_reduce_sum(pl->il_rs, (long)ndst * nbp, pl->red_partial, pl->red_result, st);
  apply_span_end(pl);
  if (gsum_out) {
    FGCHK(hipMemcpyAsync(gsum_out, pl->red_result, sizeof(double), hipMemcpyDeviceToHost, st));
    FGCHK(hipStreamSynchronize(st));
  }
  FGCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------- eight levels per launch: one chunk driver
// The reference sweeps a field whose levels have missing values, options or the limiter one level at a time (fregrid.c:1045-1083:
// do_scalar_conserve_interp(nz = 1) per level).  Here eight levels share a launch and level k keeps the bits of that one-level call,
// its sum included.  Three families of kernels do so, and every entry below is its argument rules and one call of run_levels:
//   masked  k_apply_ep8g<MASKED> (fgd_apply_levels8): levels with missing values of their own
//   ex      k_apply_ep8x (fgd_apply_levels8x): weight / sum / cell_measures / --target_grid, no limiter
//   mono    the limiter: k_mono_bounds8 and k_mono_extremes8 (the first half, conserve_interp.c:622-669), then k_apply_ep8m (the second,
//           :679-866); the split for ranks falls between the halves, at the reference's mpp_min_double / mpp_max_double (:672-677)
extern "C" int fg_plan_levels_capacity(void) { return FG_LEVELS_CAP; }
int fg_plan_is_finalized(const fg_plan *pl) { return pl && pl->finalized; }      // for sweep.hip
enum { FAM_MASKED, FAM_EX, FAM_MONO };
enum : unsigned {
  RUN_QUEUED = 1,                 // a chunk of a streamed run (sweep.hip): the error word is neither cleared nor read, so that the host
                                  // does not wait for the chunk -- fg_plan_levels_ex_begin clears it, fg_plan_levels_ex_end reads it
  RUN_FIRST = 2, RUN_SECOND = 4,  // the halves of the limiter; the other families run as RUN_BOTH
  RUN_BOTH = RUN_FIRST | RUN_SECOND
};

// The levels of a call: level-major arrays (rec null) or the caller's records of one chunk.
struct LevelSrc {
  const double *data, *grad_x, *grad_y;      // [nlev][f_stride], [nlev][nsrc], [nlev][nsrc]; order 1 reads data alone
  const int *grad_mask;                      // [nlev][nsrc]; null: no mask bits are staged and the kernels get none
  const double *rec;                         // [nsrc][3][8], as k_merge3 writes them
  const unsigned char *maskbits;             // [nsrc]
  double *b8;                                // the limiter's bounds [nsrc][4][8], rows 0 / 1 filled (fg_c2l_records_levels_mono)
  long field_area_ld;                        // != 0: the options' field_area is [nlev][field_area_ld]
};
static LevelSrc src_records(const double *rec, const unsigned char *maskbits, double *b8)    // (arrays: LevelSrc{data, gx, gy, gm})
{
  return LevelSrc{nullptr, nullptr, nullptr, nullptr, rec, maskbits, b8, 0};
}

// what the kernels of a chunk read
struct Chunk { const double *rec; const unsigned char *bits; const double *fa8; };

// levels [k0, k0 + nbv) of s, padded to eight: records stay the caller's; level-major arrays go through k_merge3 (and k_gmask_bits)
// into il_m (lv_bits), a first-order field into il_f; per-level areas into lx_fa
static Chunk stage_chunk(fg_plan *pl, const LevelSrc &s, const double *field_area, int k0, int nbv, hipStream_t st)
{
  Chunk c{s.rec, s.maskbits, nullptr};
  if (s.field_area_ld) {
    fgd_interleave(8, pl->nsrc, field_area + (size_t)k0 * s.field_area_ld, s.field_area_ld, nbv, pl->lx_fa, st);
    c.fa8 = pl->lx_fa;
  }
  if (s.rec) return c;
  const double *f = s.data + (size_t)k0 * pl->f_stride;
  const size_t g = (size_t)k0 * pl->nsrc;
  if (pl->order == 2) {
    fgd_merge3(8, pl->nsrc, pl->src_idx_f, f, pl->f_stride, s.grad_x + g, s.grad_y + g, pl->nsrc, nbv, pl->il_m, st);
    if (s.grad_mask) fgd_gmask_bits(pl->nsrc, s.grad_mask + g, pl->nsrc, nbv, pl->lv_bits, st);
    c.rec = pl->il_m; c.bits = s.grad_mask ? pl->lv_bits : nullptr;
  } else {
    interleave_field(pl, f, 8, nbv, st);
    c.rec = pl->il_f;
  }
  return c;
}

// per-level sums of one chunk (il_rs [level][ndst]) -> red_result, handed to the host whenever the 256 result slots are full
static int levels_gsum(fg_plan *pl, int nbv, int *nred, double **gsum_out, bool last)
{
  hipStream_t st = pl->stream;
  for (int k = 0; k < nbv; k++) fgd_reduce_sum(pl->il_rs + (size_t)k * pl->ndst, pl->ndst, pl->red_partial, pl->red_result + (*nred)++, st);
  if (*nred + 8 > 256 || last) {
    FGCHK(hipMemcpyAsync(*gsum_out, pl->red_result, *nred * sizeof(double), hipMemcpyDeviceToHost, st));
    FGCHK(hipStreamSynchronize(st));
    *gsum_out += *nred; *nred = 0;
  }
  return 0;
}

// A call: the device, the scratch it wants, the error word cleared (not queued, not the second half alone), then inside one PH_APPLY
// span every chunk of up to eight levels -- staged, swept by the family's kernels, its per-level row sums reduced with the reduction
// of the one-level calls -- and at the end the error word read (not queued, not the first half alone; the masked family has none,
// so without gsum_out it returns without waiting for the device).  The entries see to it that records come with nlev <= 8 (one chunk),
// that RUN_FIRST alone comes with out == gsum_out == nullptr, and that only the limiter is ever run by halves.
static int run_levels(fg_plan *pl, int fam, const LevelSrc &s, const FgApplyEx &x, int nlev, double *out, double *gsum_out, unsigned flags)
{
  FGCHK(hipSetDevice(pl->device));
  const bool arrays = !s.rec, queued = flags & RUN_QUEUED, first = flags & RUN_FIRST, second = flags & RUN_SECOND;
  int rc = apply_scratch(pl, (arrays ? SC_IL | SC_BITS : 0) | (gsum_out ? SC_RS : 0) | (fam != FAM_MASKED ? SC_XERR : 0) |
                               (s.field_area_ld ? SC_FA8 : 0) | (fam == FAM_MONO && arrays ? SC_MONO8 : 0));
  if (rc) return rc;
  hipStream_t st = pl->stream;
  const int ndst = pl->ndst;
  double *rs = gsum_out ? pl->il_rs : nullptr, *b8 = arrays ? pl->mono8_b : s.b8;
  if (fam != FAM_MASKED && first && !queued) FGCHK(hipMemsetAsync(pl->xerr, 0, sizeof(int), st));
  apply_span_begin(pl, st);
  int nred = 0;
  for (int k0 = 0; k0 < nlev && !rc; k0 += 8) {
    const int nbv = std::min(8, nlev - k0);
    const Chunk c = stage_chunk(pl, s, x.field_area, k0, nbv, st);
    double *o = out + (size_t)k0 * ndst;
    if (fam == FAM_MASKED)
      fgd_apply_levels8(pl->order, ndst, pl->nx, pl->csr, c.rec, c.bits, x.missing, o, rs, (long)ndst, nbv, st);
    else if (fam == FAM_EX)
      fgd_apply_levels8x(pl->order, ndst, pl->nx, pl->csr, c.rec, c.bits, x, c.fa8, o, rs, (long)ndst, nbv, pl->xerr, st);
    else {
      if (first && arrays)
        fgd_mono_bounds8(pl->tiles_dev, pl->ntiles, pl->nsrc, pl->src_idx_f, s.data + (size_t)k0 * pl->f_stride, pl->f_stride, nbv, x.missing,
                         b8, st);
      if (first) fgd_mono_extremes8(pl->nx, pl->csr, c.rec, c.bits, x.missing, nbv, b8, st);
      if (second) fgd_apply_levels8m(ndst, pl->nx, pl->csr, c.rec, c.bits, b8, x, o, rs, (long)ndst, nbv, pl->xerr, st);
    }
    if (gsum_out) rc = levels_gsum(pl, nbv, &nred, &gsum_out, k0 + 8 >= nlev);
  }
  apply_span_end(pl);                                      // on every path
  if (rc) return rc;
  FGCHK(hipGetLastError());
  return (fam == FAM_MASKED || queued || !second) ? 0 : ex_error_word(pl);
}

// levels with missing values of their own: gsum_out[k] carries the bits fg_plan_apply_ex returns for level k alone
extern "C" int fg_plan_apply_levels(fg_plan *pl, const double *data, const double *grad_x, const double *grad_y,
                                    const int *grad_mask, double missing, int nlev, double *out, double *gsum_out)
{
  if (int rc = levels_check("fg_plan_apply_levels", pl, nullptr, CK_NLEV | CK_GRADS_MASK, !pl || !data || !out, false, nlev, 0,
                            grad_x && grad_y, grad_mask))
    return rc;
  FgApplyEx x{};
  x.missing = missing;
  return run_levels(pl, FAM_MASKED, LevelSrc{data, grad_x, grad_y, grad_mask}, x, nlev, out, gsum_out, RUN_BOTH);
}

extern "C" int fg_plan_apply_records_levels(fg_plan *pl, int nz, const double *rec, const unsigned char *maskbits, double missing,
                                            double *out, double *gsum_out)
{
  if (int rc = levels_check("fg_plan_apply_records_levels", pl, nullptr, CK_RECORDS | CK_BITS | CK_NZ8, !pl || !rec || !out, false, nz, 0,
                            false, maskbits))
    return rc;
  FgApplyEx x{};
  x.missing = missing;
  return run_levels(pl, FAM_MASKED, src_records(rec, maskbits, nullptr), x, nz, out, gsum_out, RUN_BOTH);
}

// ------------------------------------------------------------------- the sweep with every option
static int ex_check(fg_plan *pl, const fg_apply_opts *o, const double *data, const double *gx, const double *gy, int nz, const char *who)
{
  if (!pl || !o || !data) return fg_fail(FG_ERR_ARG, "%s: null argument", who);
  if (!pl->finalized) return fg_fail(FG_ERR_STATE, "%s: call fg_plan_finalize first", who);
  if (nz < 1) return fg_fail(FG_ERR_ARG, "nz must be >= 1");
  if (nz > 1 && o->has_missing) return fg_fail(FG_ERR_ARG, "conserve_interp: has_missing should be false when nz > 1");
  if (nz > 1 && o->field_area) return fg_fail(FG_ERR_ARG, "conserve_interp: cell_measures should be false when nz > 1");
  if (nz > 1 && o->cell_methods_sum) return fg_fail(FG_ERR_ARG, "conserve_interp: cell_methods should not be sum when nz > 1");
  if (pl->order == 2 && (!gx || !gy)) return fg_fail(FG_ERR_ARG, "order 2 needs grad_x and grad_y");
  return area_rule(who, pl, o);
}

extern "C" int fg_plan_mono_begin(fg_plan *pl, const fg_apply_opts *o, const double *data, const double *grad_x,
                                  const double *grad_y, const int *grad_mask)
{
  int rc = ex_check(pl, o, data, grad_x, grad_y, 1, "fg_plan_mono_begin");
  if (rc) return rc;
  if (pl->order != 2) return fg_fail(FG_ERR_ARG, "the monotone limiter belongs to conserve_order2 (conserve_interp.c:527-531)");
  FGCHK(hipSetDevice(pl->device));
  if ((rc = apply_scratch(pl, SC_XERR | SC_ROW_SUM | SC_MONO))) return rc;
  const double miss = o->has_missing ? o->missing : -1.e20;
  double *b = pl->mono_b;
  const size_t n = pl->nsrc;
  FGCHK(hipMemsetAsync(pl->xerr, 0, sizeof(int), pl->stream));
  fgd_mono_bounds(pl->tiles_dev, pl->ntiles, pl->nsrc, pl->src_idx_f, data, miss, b, b + n, b + 2 * n, b + 3 * n, pl->stream);
  fgd_mono_xdata(pl->nx, pl->csr, data, grad_x, grad_y, grad_mask, miss, pl->mono_x, b + 2 * n, b + 3 * n, pl->stream);
  FGCHK(hipGetLastError());
  pl->mono_open = true;
  return 0;
}

extern "C" int fg_plan_mono_minmax_dev(fg_plan *pl, double **f_min, double **f_max)
{
  if (!pl || !pl->mono_open) return fg_fail(FG_ERR_STATE, "fg_plan_mono_minmax_dev: call fg_plan_mono_begin first");
  if (f_max) *f_max = pl->mono_b + 2 * (size_t)pl->nsrc;
  if (f_min) *f_min = pl->mono_b + 3 * (size_t)pl->nsrc;
  return 0;
}

extern "C" int fg_plan_mono_copy_minmax(fg_plan *pl, int to_plan, double *f_min, double *f_max)
{
  if (!pl || !pl->mono_open || !f_min || !f_max) return fg_fail(FG_ERR_STATE, "fg_plan_mono_copy_minmax: call fg_plan_mono_begin first");
  FGCHK(hipSetDevice(pl->device));
  double *mx = pl->mono_b + 2 * (size_t)pl->nsrc, *mn = pl->mono_b + 3 * (size_t)pl->nsrc;
  const size_t bytes = (size_t)pl->nsrc * sizeof(double);
  FGCHK(hipMemcpyAsync(to_plan ? mn : f_min, to_plan ? f_min : mn, bytes, hipMemcpyDeviceToDevice, pl->stream));
  FGCHK(hipMemcpyAsync(to_plan ? mx : f_max, to_plan ? f_max : mx, bytes, hipMemcpyDeviceToDevice, pl->stream));
  FGCHK(hipStreamSynchronize(pl->stream));
  return 0;
}

extern "C" int fg_plan_mono_end(fg_plan *pl, const fg_apply_opts *o, const double *data, double *out, double *gsum_out)
{
  if (!pl || !o || !data || !out) return fg_fail(FG_ERR_ARG, "null argument");
  if (!pl->mono_open) return fg_fail(FG_ERR_STATE, "fg_plan_mono_end: call fg_plan_mono_begin first");
  FGCHK(hipSetDevice(pl->device));
  pl->mono_open = false;
  const double miss = o->has_missing ? o->missing : -1.e20;
  double *b = pl->mono_b;
  const size_t n = pl->nsrc;
  fgd_mono_limit(pl->nx, pl->csr, data, miss, b, b + n, b + 2 * n, b + 3 * n, pl->mono_x, pl->xerr, pl->stream);
  FgApplyEx x = ex_pack(pl, o, nullptr);
  x.xdata = pl->mono_x;
  fgd_apply_ex(2, pl->ndst, pl->csr, data, nullptr, nullptr, x, out, gsum_out ? pl->row_sum : nullptr, pl->xerr, pl->stream, pl->nx);
  if (gsum_out) {
    fgd_reduce_sum(pl->row_sum, pl->ndst, pl->red_partial, pl->red_result, pl->stream);
    FGCHK(hipMemcpyAsync(gsum_out, pl->red_result, sizeof(double), hipMemcpyDeviceToHost, pl->stream));
  }
  FGCHK(hipGetLastError());
  return ex_error_word(pl);
}

extern "C" int fg_plan_apply_ex(fg_plan *pl, const fg_apply_opts *o, const double *data, const double *grad_x,
                                const double *grad_y, const int *grad_mask, int nz, double *out, double *gsum_out)
{
  int rc = ex_check(pl, o, data, grad_x, grad_y, nz, "fg_plan_apply_ex");
  if (rc) return rc;
  if (!out) return fg_fail(FG_ERR_ARG, "null argument");
  if (o->monotonic && pl->order == 2) {
    if (nz != 1) return fg_fail(FG_ERR_ARG, "the monotone limiter works on one level per call (conserve_interp.c:648-651 index level 0 only)");
    if ((rc = fg_plan_mono_begin(pl, o, data, grad_x, grad_y, grad_mask))) return rc;
    return fg_plan_mono_end(pl, o, data, out, gsum_out);
  }
  FGCHK(hipSetDevice(pl->device));
  if ((rc = apply_scratch(pl, SC_XERR | SC_ROW_SUM))) return rc;
  if (nz > 256) return fg_fail(FG_ERR_ARG, "nz too large for one call (max 256 levels)");
  hipStream_t st = pl->stream;
  FGCHK(hipMemsetAsync(pl->xerr, 0, sizeof(int), st));
  FgApplyEx x = ex_pack(pl, o, grad_mask);
  for (int k = 0; k < nz; k++) {
    fgd_apply_ex(pl->order, pl->ndst, pl->csr, data + (size_t)k * pl->f_stride, grad_x ? grad_x + (size_t)k * pl->nsrc : nullptr,
                 grad_y ? grad_y + (size_t)k * pl->nsrc : nullptr, x, out + (size_t)k * pl->ndst,
                 gsum_out ? pl->row_sum : nullptr, pl->xerr, st, pl->nx);
    if (gsum_out) fgd_reduce_sum(pl->row_sum, pl->ndst, pl->red_partial, pl->red_result + k, st);
  }
  FGCHK(hipGetLastError());
  if (gsum_out) {
    double parts[256];
    FGCHK(hipMemcpyAsync(parts, pl->red_result, nz * sizeof(double), hipMemcpyDeviceToHost, st));
    FGCHK(hipStreamSynchronize(st));
    double g = 0;
    for (int k = 0; k < nz; k++) g += parts[k];
    *gsum_out = g;
  }
  return ex_error_word(pl);
}

// ------------------------------------------------------------------- the level loop of these options (the ex family)
// fg_plan_apply_ex(nz = 1) per level is what the reference does for weight / sum / cell_measures / --target_grid fields
// (conserve_interp.c:544-546 refuse nz > 1).  Mask bits are staged and read only for an order-2 field with missing values.
extern "C" int fg_plan_levels_ex_capacity(int per_level_area) { return per_level_area ? FG_LEVELS_EX_CAP_Z : FG_LEVELS_EX_CAP; }

// the options as the many-level kernels take them; cell_methods = sum uses no field_area (:582-588 is the else branch)
static FgApplyEx levels_ex_pack(fg_plan *pl, const fg_apply_opts *o)
{
  FgApplyEx x = ex_pack(pl, o, nullptr);
  if (x.sum) x.field_area = nullptr;
  return x;
}

static int levels_ex_run(fg_plan *pl, const fg_apply_opts *o, bool records, LevelSrc s, int nlev, long field_area_ld, double *out,
                         double *gsum_out, unsigned queued)
{
  if (int rc = levels_check(records ? "fg_plan_apply_records_levels_ex" : "fg_plan_apply_levels_ex", pl, o,
                            CK_NO_LIMITER | CK_FA_LD | CK_AREA | (records ? CK_RECORDS | CK_NZ8 | CK_BITS_IF_MISSING : CK_NLEV | CK_GRADS),
                            !pl || !o || !(records ? s.rec : s.data) || !out, false, nlev, field_area_ld, s.grad_x && s.grad_y, s.maskbits))
    return rc;
  const FgApplyEx x = levels_ex_pack(pl, o);
  s.field_area_ld = x.field_area ? field_area_ld : 0;
  if (!o->has_missing || pl->order != 2) s.grad_mask = nullptr, s.maskbits = nullptr;
  return run_levels(pl, FAM_EX, s, x, nlev, out, gsum_out, RUN_BOTH | queued);
}

extern "C" int fg_plan_apply_levels_ex(fg_plan *pl, const fg_apply_opts *o, const double *data, const double *grad_x, const double *grad_y,
                                       const int *grad_mask, int nlev, long field_area_ld, double *out, double *gsum_out)
{
  return levels_ex_run(pl, o, false, LevelSrc{data, grad_x, grad_y, grad_mask}, nlev, field_area_ld, out, gsum_out, 0);
}
extern "C" int fg_plan_apply_records_levels_ex(fg_plan *pl, const fg_apply_opts *o, int nz, const double *rec, const unsigned char *maskbits,
                                               long field_area_ld, double *out, double *gsum_out)
{
  return levels_ex_run(pl, o, true, src_records(rec, maskbits, nullptr), nz, field_area_ld, out, gsum_out, 0);
}

// for sweep.hip: the chunks of one streamed run, queued on the plan's (borrowed) stream between _begin and _end
int fg_plan_levels_ex_begin(fg_plan *pl)
{
  if (!pl) return fg_fail(FG_ERR_ARG, "null argument");
  FGCHK(hipSetDevice(pl->device));
  if (int rc = apply_scratch(pl, SC_XERR)) return rc;
  FGCHK(hipMemsetAsync(pl->xerr, 0, sizeof(int), pl->stream));
  return 0;
}
int fg_plan_levels_ex_chunk(fg_plan *pl, const fg_apply_opts *o, int nz, const double *data, const double *rec, const unsigned char *maskbits,
                            double *out)
{
  return levels_ex_run(pl, o, rec != nullptr, rec ? src_records(rec, maskbits, nullptr) : LevelSrc{data}, nz, 0, out, nullptr, RUN_QUEUED);
}
int fg_plan_levels_ex_end(fg_plan *pl) { return ex_error_word(pl); }

// ------------------------------------------------------------------- the limiter on many levels (the mono family)
// fg_plan_apply_ex(monotonic = 1, nz = 1) per level is what the reference does (conserve_interp.c:648-651 index level 0 only):
// four launches, an xdata array written and read again and three reads of every CSR record per level.  Mask bits are staged when
// grad_mask is given.  mono8_nz: the levels of the chunk fg_plan_mono_levels_begin left open, 0 for none.  The records entries work
// on what fg_c2l_records_levels_mono wrote -- rec, maskbits and b8 with rows 0 / 1 filled, rows 2 / 3 at their start values -- so a
// chunk is k_mono_extremes8 and k_apply_ep8m straight on the caller's buffers; b8 is consumed: the extremes go into its rows 2 and 3.
// mono8r_nz / mono8r_b: the levels and the caller's bounds buffer of the chunk fg_plan_mono_records_begin left open.
// the rules all six entries share, with the entry's rule on the number of levels; level-major arrays come with mandatory gradients
static int mono_check(const char *who, const fg_plan *pl, const fg_apply_opts *o, bool records, const LevelSrc &s, unsigned nz_rule, bool null_late,
                      int nlev)
{
  const bool null_arg = !pl || !o || (records ? !s.rec : !s.data || !s.grad_x || !s.grad_y);
  return levels_check(who, pl, o, CK_LIMITER | CK_AREA | nz_rule, null_arg, null_late, nlev, 0, true, true);
}

extern "C" int fg_plan_apply_levels_mono(fg_plan *pl, const fg_apply_opts *o, const double *data, const double *grad_x, const double *grad_y,
                                         const int *grad_mask, int nlev, double *out, double *gsum_out)
{
  const LevelSrc s{data, grad_x, grad_y, grad_mask};
  if (int rc = mono_check("fg_plan_apply_levels_mono", pl, o, false, s, CK_NLEV, !out, nlev)) return rc;
  pl->mono8_nz = 0;                                        // an open chunk of the split entries is overwritten
  return run_levels(pl, FAM_MONO, s, levels_ex_pack(pl, o), nlev, out, gsum_out, RUN_BOTH);
}

extern "C" int fg_plan_mono_levels_begin(fg_plan *pl, const fg_apply_opts *o, const double *data, const double *grad_x,
                                         const double *grad_y, const int *grad_mask, int nz)
{
  const LevelSrc s{data, grad_x, grad_y, grad_mask};
  if (int rc = mono_check("fg_plan_mono_levels_begin", pl, o, false, s, CK_NZ8_PAIR, false, nz)) return rc;
  int rc = run_levels(pl, FAM_MONO, s, levels_ex_pack(pl, o), nz, nullptr, nullptr, RUN_FIRST);
  if (!rc) pl->mono8_nz = nz;
  return rc;
}

// f_max / f_min of the open chunk (nz levels, bounds b8) out of (to_plan = 0) or back into it; synchronises the plan's stream
static int mono8_copy_minmax(const char *who, const char *begin, fg_plan *pl, int nz, double *b8, int to_plan, double *f_min, double *f_max)
{
  if (!pl || !f_min || !f_max) return fg_fail(FG_ERR_ARG, "%s: null argument", who);
  if (!nz) return fg_fail(FG_ERR_STATE, "%s: call %s first", who, begin);
  FGCHK(hipSetDevice(pl->device));
  fgd_mono_minmax8(pl->nsrc, nz, to_plan ? 1 : 0, b8, f_min, f_max, pl->stream);
  FGCHK(hipGetLastError());
  FGCHK(hipStreamSynchronize(pl->stream));
  return 0;
}
extern "C" int fg_plan_mono_levels_copy_minmax(fg_plan *pl, int to_plan, double *f_min, double *f_max)
{
  return mono8_copy_minmax("fg_plan_mono_levels_copy_minmax", "fg_plan_mono_levels_begin", pl, pl ? pl->mono8_nz : 0, pl ? pl->mono8_b : nullptr,
                           to_plan, f_min, f_max);
}

// The records and bits are staged again from the caller's arrays: il_m and lv_bits are the scratch of every many-level entry, and
// the caller may have swept another field on this plan while its ranks exchanged the extremes.
extern "C" int fg_plan_mono_levels_end(fg_plan *pl, const fg_apply_opts *o, const double *data, const double *grad_x, const double *grad_y,
                                       const int *grad_mask, double *out, double *gsum_out)
{
  const LevelSrc s{data, grad_x, grad_y, grad_mask};
  if (int rc = mono_check("fg_plan_mono_levels_end", pl, o, false, s, 0, !out, 1)) return rc;
  if (!pl->mono8_nz) return fg_fail(FG_ERR_STATE, "fg_plan_mono_levels_end: call fg_plan_mono_levels_begin first");
  const int nz = pl->mono8_nz;
  pl->mono8_nz = 0;
  return run_levels(pl, FAM_MONO, s, levels_ex_pack(pl, o), nz, out, gsum_out, RUN_SECOND);
}

static int mono_records_run(fg_plan *pl, const fg_apply_opts *o, int nz, const double *rec, const unsigned char *maskbits, double *b8,
                            double *out, double *gsum_out, unsigned queued)
{
  const LevelSrc s = src_records(rec, maskbits, b8);
  if (int rc = mono_check("fg_plan_apply_records_levels_mono", pl, o, true, s, CK_NZ8, !b8 || !out, nz)) return rc;
  pl->mono8r_nz = 0;                                       // as fg_plan_apply_levels_mono closes an open chunk of its split
  return run_levels(pl, FAM_MONO, s, levels_ex_pack(pl, o), nz, out, gsum_out, RUN_BOTH | queued);
}
extern "C" int fg_plan_apply_records_levels_mono(fg_plan *pl, const fg_apply_opts *o, int nz, const double *rec, const unsigned char *maskbits,
                                                 double *b8, double *out, double *gsum_out)
{
  return mono_records_run(pl, o, nz, rec, maskbits, b8, out, gsum_out, 0);
}
// for sweep.hip: a chunk of one streamed run, between fg_plan_levels_ex_begin and _end
int fg_plan_mono_records_chunk(fg_plan *pl, const fg_apply_opts *o, int nz, const double *rec, const unsigned char *maskbits, double *b8,
                               double *out)
{
  return mono_records_run(pl, o, nz, rec, maskbits, b8, out, nullptr, RUN_QUEUED);
}

extern "C" int fg_plan_mono_records_reset(fg_plan *pl, double *b8)
{
  if (!pl || !b8) return fg_fail(FG_ERR_ARG, "fg_plan_mono_records_reset: null argument");
  FGCHK(hipSetDevice(pl->device));
  fgd_mono_reset8(pl->nsrc, b8, pl->stream);
  FGCHK(hipGetLastError());
  return 0;
}

extern "C" int fg_plan_mono_records_begin(fg_plan *pl, const fg_apply_opts *o, int nz, const double *rec, const unsigned char *maskbits,
                                          double *b8)
{
  const LevelSrc s = src_records(rec, maskbits, b8);
  if (int rc = mono_check("fg_plan_mono_records_begin", pl, o, true, s, CK_NZ8_PAIR, !b8, nz)) return rc;
  int rc = run_levels(pl, FAM_MONO, s, levels_ex_pack(pl, o), nz, nullptr, nullptr, RUN_FIRST);
  if (!rc) { pl->mono8r_nz = nz; pl->mono8r_b = b8; }
  return rc;
}
extern "C" int fg_plan_mono_records_copy_minmax(fg_plan *pl, int to_plan, double *f_min, double *f_max)
{
  return mono8_copy_minmax("fg_plan_mono_records_copy_minmax", "fg_plan_mono_records_begin", pl, pl ? pl->mono8r_nz : 0,
                           pl ? pl->mono8r_b : nullptr, to_plan, f_min, f_max);
}

// rec and maskbits are the caller's, unchanged since begin; the bounds are the buffer begin was given
extern "C" int fg_plan_mono_records_end(fg_plan *pl, const fg_apply_opts *o, const double *rec, const unsigned char *maskbits, double *out,
                                        double *gsum_out)
{
  if (int rc = mono_check("fg_plan_mono_records_end", pl, o, true, src_records(rec, maskbits, nullptr), 0, !out, 1)) return rc;
  if (!pl->mono8r_nz) return fg_fail(FG_ERR_STATE, "fg_plan_mono_records_end: call fg_plan_mono_records_begin first");
  const int nz = pl->mono8r_nz;
  pl->mono8r_nz = 0;
  return run_levels(pl, FAM_MONO, src_records(rec, maskbits, pl->mono8r_b), levels_ex_pack(pl, o), nz, out, gsum_out, RUN_SECOND);
}

// The sweep on fields the caller already keeps interleaved: data_il [F][nb], grad_x_il/grad_y_il [ncells_in][nb],
// out_il [ndst][nb]; nb in {2, 4, 8}; no missing values.  Skips the two transposes of fg_plan_apply.
extern "C" int fg_plan_apply_interleaved(fg_plan *pl, int nb, const double *data_il, const double *grad_x_il,
                                         const double *grad_y_il, double *out_il, double *gsum_out)
{
  if (!pl || !data_il || !out_il) return fg_fail(FG_ERR_ARG, "null argument");
  if (!pl->finalized) return fg_fail(FG_ERR_STATE, "fg_plan_apply_interleaved: call fg_plan_finalize first");
  if (nb != 2 && nb != 4 && nb != 8 && nb != 16) return fg_fail(FG_ERR_ARG, "nb must be 2, 4, 8 or 16");
  if (pl->order == 2 && (!grad_x_il || !grad_y_il)) return fg_fail(FG_ERR_ARG, "order 2 needs grad_x and grad_y");
  FGCHK(hipSetDevice(pl->device));
  { int rc = apply_scratch(pl, gsum_out ? SC_IL | SC_RS : 0); if (rc) return rc; }
  apply_span_begin(pl, pl->stream);
  fgd_apply_il(pl->order, nb, pl->ndst, pl->csr, data_il, grad_x_il, grad_y_il, -1.e20, out_il,
               gsum_out ? pl->il_rs : nullptr, 0, nb, pl->stream, pl->nx);
  apply_span_end(pl);
  if (gsum_out) {
    fgd_reduce_sum(pl->il_rs, (long)pl->ndst * nb, pl->red_partial, pl->red_result, pl->stream);
    FGCHK(hipMemcpyAsync(gsum_out, pl->red_result, sizeof(double), hipMemcpyDeviceToHost, pl->stream));
    FGCHK(hipStreamSynchronize(pl->stream));
  }
  FGCHK(hipGetLastError());
  return 0;
}

// ----------------------------------------------------------------------------- (B1)
// libfrencutils drop-ins.  Fatal errors follow mosaic_util.c:57-65.
static void fatal(const char *msg)
{
  fprintf(stderr, "FATAL Error: %s\n", msg);
  exit(1);
}

#ifndef MAXXGRID
#define MAXXGRID 5e6          /* create_xgrid.h:22-28, serial build */
#endif

extern "C" int get_maxxgrid(void) { return MAXXGRID; }
extern "C" int get_maxxgrid_(void) { return get_maxxgrid(); }

// get_grid_area / get_grid_great_circle_area: the source records of a plan against a 1x1 dummy destination, which keeps the plan
// machinery uniform
static void b1_grid_area(bool great_circle, const int *nlon, const int *nlat, const double *lon, const double *lat, double *area)
{
  int nx = *nlon, ny = *nlat, one = 1;
  const double dl[4] = {0, 0.01, 0, 0.01}, da[4] = {0, 0, 0.01, 0.01};
  const double *lons[1] = {lon}, *lats[1] = {lat};
  fg_plan *pl = nullptr;
  long rc = great_circle ? fg_plan_create_great_circle(1, &nx, &ny, lons, lats, nullptr, one, one, dl, da, fg_env_device(), &pl)
                         : fg_plan_create(FG_CONSERVE_ORDER1, 1, &nx, &ny, lons, lats, nullptr, one, one, dl, da, fg_env_device(), &pl);
  if (rc < 0) fatal(fg_last_error());
  if (fg_plan_get_cell_area(pl, area, nullptr)) fatal(fg_last_error());
  fg_plan_destroy(pl);
}
extern "C" void get_grid_area(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area)
{
  b1_grid_area(false, nlon, nlat, lon, lat, area);
}
extern "C" void get_grid_area_(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area)
{
  get_grid_area(nlon, nlat, lon, lat, area);
}

extern "C" int create_xgrid_great_circle(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out,
                                         const double *lon_in, const double *lat_in, const double *lon_out, const double *lat_out,
                                         const double *mask_in, int *i_in, int *j_in, int *i_out, int *j_out,
                                         double *xgrid_area, double *xgrid_clon, double *xgrid_clat)
{
  int nx1 = *nlon_in, ny1 = *nlat_in;
  const double *lons[1] = {lon_in}, *lats[1] = {lat_in}, *masks[1] = {mask_in};
  fg_plan *pl = nullptr;
  long nx = fg_plan_create_great_circle(1, &nx1, &ny1, lons, lats, masks, *nlon_out, *nlat_out, lon_out, lat_out, fg_env_device(), &pl);
  if (nx < 0) fatal(fg_last_error());
  if (nx > (long)MAXXGRID) fatal("nxgrid is greater than MAXXGRID, increase MAXXGRID");      // create_xgrid.c:1444
  if (fg_plan_get_xgrid(pl, nullptr, i_in, j_in, i_out, j_out, xgrid_area, nullptr, nullptr)) fatal(fg_last_error());
  for (long k = 0; k < nx; k++) { if (xgrid_clon) xgrid_clon[k] = 0; if (xgrid_clat) xgrid_clat[k] = 0; }   // :1446-1447
  fg_plan_destroy(pl);
  return (int)nx;
}
extern "C" int create_xgrid_great_circle_(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out,
                                          const double *lon_in, const double *lat_in, const double *lon_out, const double *lat_out,
                                          const double *mask_in, int *i_in, int *j_in, int *i_out, int *j_out,
                                          double *xgrid_area, double *xgrid_clon, double *xgrid_clat)
{
  return create_xgrid_great_circle(nlon_in, nlat_in, nlon_out, nlat_out, lon_in, lat_in, lon_out, lat_out, mask_in,
                                   i_in, j_in, i_out, j_out, xgrid_area, xgrid_clon, xgrid_clat);
}

extern "C" void get_grid_great_circle_area(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area)
{
  b1_grid_area(true, nlon, nlat, lon, lat, area);
}
extern "C" void get_grid_great_circle_area_(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area)
{
  get_grid_great_circle_area(nlon, nlat, lon, lat, area);
}

extern "C" int fg_gc_clip_batch(int npairs, const double *a, const double *b, double *out, int *n_out, double *area, int device)
{
  if (npairs < 0 || !a || !b || !out || !n_out || !area) return fg_fail(FG_ERR_ARG, "null argument");
  if (npairs == 0) return 0;
  if (int rc = fg_use_device("fg_gc_clip_batch", device)) return rc;
  const size_t na = (size_t)npairs * 12, no = (size_t)npairs * FG_GC_POLY_CAP * 3;
  double *d_a = (double *)g_pool.get(device, (2 * na + no + npairs) * sizeof(double));
  int *d_n = (int *)g_pool.get(device, (size_t)npairs * sizeof(int));
  if (!d_a || !d_n) { if (d_a) g_pool.put(d_a); if (d_n) g_pool.put(d_n); return fg_fail(FG_ERR_HIP, "out of device memory"); }
  double *d_b = d_a + na, *d_o = d_b + na, *d_ar = d_o + no;
  int rc = 0;
  if (hipMemcpy(d_a, a, na * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_b, b, na * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = FG_ERR_HIP;
  if (!rc) {
    fgd_gc_clip_batch(npairs, d_a, d_b, d_o, d_n, d_ar, nullptr);
    if (hipMemcpy(out, d_o, no * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(n_out, d_n, (size_t)npairs * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(area, d_ar, (size_t)npairs * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = FG_ERR_HIP;
  }
  g_pool.put(d_a); g_pool.put(d_n);
  if (rc) return fg_fail(rc, "fg_gc_clip_batch: HIP copy/launch failed: %s", hipGetErrorString(hipGetLastError()));
  return 0;
}

extern "C" double great_circle_area(int n, const double *x, const double *y, const double *z)
{
  if (n < 1 || n > 64) fatal("great_circle_area (HIP): 1 <= n <= 64");
  double h[64 * 3], area = 0;
  for (int k = 0; k < n; k++) { h[k * 3] = x[k]; h[k * 3 + 1] = y[k]; h[k * 3 + 2] = z[k]; }
  if (hipSetDevice(fg_env_device()) != hipSuccess) fatal("no HIP device visible: libfregrid_hip needs an MI355X-class GPU");
  double *d = (double *)g_pool.get(fg_env_device(), (64 * 3 + 2) * sizeof(double));
  if (!d) fatal("out of device memory");
  int *dn = (int *)(d + 64 * 3 + 1);
  bool ok = hipMemcpy(d, h, n * 3 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dn, &n, sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    fgd_gc_area_batch(1, 64, d, dn, d + 64 * 3, nullptr);
    ok = hipMemcpy(&area, d + 64 * 3, sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
  }
  g_pool.put(d);
  if (!ok) fatal("great_circle_area: HIP copy/launch failed");
  return area;
}

// sin / cos of n host values with the device's latitude trig (sincos_glibc.h): parity probe for the tests
extern "C" int fg_sincos_batch(long n, const double *x, double *s, double *c, int device)
{
  if (n < 0 || !x || !s || !c) return fg_fail(FG_ERR_ARG, "null argument");
  if (n == 0) return 0;
  if (int rc = fg_use_device("fg_sincos_batch", device)) return rc;
  double *d = (double *)g_pool.get(device, 3 * (size_t)n * sizeof(double));
  if (!d) return fg_fail(FG_ERR_HIP, "out of device memory");
  bool ok = hipMemcpy(d, x, n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    fgd_sincos_probe(n, d, d + n, d + 2 * n, nullptr);
    ok = hipMemcpy(s, d + n, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(c, d + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
  }
  g_pool.put(d);
  if (!ok) return fg_fail(FG_ERR_HIP, "fg_sincos_batch: HIP copy/launch failed");
  return 0;
}

// clip_2dx2d_great_circle / great_circle_area, one polygon pair per call (create_xgrid.h / mosaic_util.h prototypes)
extern "C" int clip_2dx2d_great_circle(const double x1_in[], const double y1_in[], const double z1_in[], int n1_in,
                                       const double x2_in[], const double y2_in[], const double z2_in[], int n2_in,
                                       double x_out[], double y_out[], double z_out[])
{
  if (n1_in != 4 || n2_in != 4) fatal("clip_2dx2d_great_circle (HIP): quadrilaterals only (n1_in == n2_in == 4, as every caller in the reference passes)");
  double a[12], b[12], out[FG_GC_POLY_CAP * 3], area;
  int n_out = 0;
  for (int k = 0; k < 4; k++) {
    a[k * 3] = x1_in[k]; a[k * 3 + 1] = y1_in[k]; a[k * 3 + 2] = z1_in[k];
    b[k * 3] = x2_in[k]; b[k * 3 + 1] = y2_in[k]; b[k * 3 + 2] = z2_in[k];
  }
  if (fg_gc_clip_batch(1, a, b, out, &n_out, &area, fg_env_device())) fatal(fg_last_error());
  if (n_out == -1) fatal("create_xgrid.c(clip_2dx2d_great_circle): grid box 1 is not convex");
  if (n_out == -2) fatal("create_xgrid.c(clip_2dx2d_great_circle): grid box 2 is not convex");
  if (n_out < 0) fatal(gc_clip_error(-n_out));
  for (int k = 0; k < n_out; k++) { x_out[k] = out[k * 3]; y_out[k] = out[k * 3 + 1]; z_out[k] = out[k * 3 + 2]; }
  return n_out;
}

// create_xgrid_1dx2d_order1/2 and create_xgrid_2dx1d_order1/2 (create_xgrid.c:208-591) through the shared search pipeline.
// fg_box_xgrid_lists is the part that can fail with a code (runoff.hip calls it on its own device); lists as (box i, box j, quad i, quad j).
long fg_box_xgrid_lists(int dev, int box_is_src, int order, int nxb, int nyb, const double *lon_b, const double *lat_b,
                        int nxq, int nyq, const double *lon_q, const double *lat_q, const double *mask,
                        std::vector<int> idx[4], std::vector<double> &area, std::vector<double> *clon, std::vector<double> *clat)
{
  if (nxb < 1 || nyb < 1 || nxq < 1 || nyq < 1) return fg_fail(FG_ERR_ARG, "create_xgrid: bad grid sizes");
  fg_plan *pl = nullptr;
  int rc = plan_base(order, 1, &nxb, &nyb, nxq, nyq, dev, &pl);
  if (rc) return rc;
  const size_t npb = (size_t)(nxb + 1) * (nyb + 1), npq = (size_t)(nxq + 1) * (nyq + 1);
  std::vector<double> tx(npb), ty(npb);                                  // the reference's tmpx/tmpy, :229-236
  for (int j = 0; j <= nyb; j++) for (int i = 0; i <= nxb; i++) { tx[(size_t)j * (nxb + 1) + i] = lon_b[i]; ty[(size_t)j * (nxb + 1) + i] = lat_b[j]; }
  const size_t nmask = box_is_src ? (size_t)nxb * nyb : (size_t)nxq * nyq;
  double *d = pl->alloc<double>(2 * npb + 2 * npq + (nxb + 1) + (nyb + 1) + nmask);
  if (!d) { fg_plan_destroy(pl); return fg_fail(FG_ERR_HIP, "out of device memory"); }
  double *d_tx = d, *d_ty = d_tx + npb, *d_lq = d_ty + npb, *d_aq = d_lq + npq, *d_lb = d_aq + npq, *d_ab = d_lb + (nxb + 1), *d_mask = d_ab + (nyb + 1);
  bool ok = hipMemcpy(d_tx, tx.data(), npb * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d_ty, ty.data(), npb * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d_lq, lon_q, npq * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d_aq, lat_q, npq * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d_lb, lon_b, (nxb + 1) * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d_ab, lat_b, (nyb + 1) * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d_mask, mask, nmask * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { fg_plan_destroy(pl); return fg_fail(FG_ERR_HIP, "grid upload failed"); }
  BoxMode bm;
  bm.box = FgBox{d_lb, d_ab, nxb, nyb};
  bm.mask_quad = box_is_src ? nullptr : d_mask;
  bm.no_adjust = (box_is_src && order == 1 && !(nxb > 1)) ? 1 : 0;
  const double *lons[1] = {d_tx}, *lats[1] = {d_ty}, *masks[1] = {box_is_src ? d_mask : nullptr};
  const DstExtents x = dst_extents_host(nxq, nyq, lon_q, lat_q);
  long nx = plan_search(pl, SearchIn{.lon_in = lons, .lat_in = lats, .mask_in = box_is_src ? masks : nullptr, .lon_out = d_lq, .lat_out = d_aq,
                                     .boxm = &bm, .mean_dlat = x.dlat, .mean_dlon = x.dlon});
  if (nx < 0) { fg_plan_destroy(pl); return nx; }
  if (nx > (long)MAXXGRID) { fg_plan_destroy(pl); return fg_fail(FG_ERR_CAPACITY, "nxgrid is greater than MAXXGRID, increase MAXXGRID"); }
  for (int k = 0; k < 4; k++) idx[k].resize(nx);
  area.resize(nx);
  if (order == 2) { clon->resize(nx); clat->resize(nx); }
  rc = fg_plan_get_xgrid(pl, nullptr, idx[0].data(), idx[1].data(), idx[2].data(), idx[3].data(), area.data(),
                         order == 2 ? clon->data() : nullptr, order == 2 ? clat->data() : nullptr);
  fg_plan_destroy(pl);
  return rc ? rc : nx;
}

static int b1_create_xgrid_box(int box_is_src, int order, int nxb, int nyb, const double *lon_b, const double *lat_b,
                               int nxq, int nyq, const double *lon_q, const double *lat_q, const double *mask,
                               int *i_in, int *j_in, int *i_out, int *j_out, double *xgrid_area, double *xgrid_clon, double *xgrid_clat)
{
  std::vector<int> idx[4];
  std::vector<double> area, clon, clat;
  const long nx = fg_box_xgrid_lists(fg_env_device(), box_is_src, order, nxb, nyb, lon_b, lat_b, nxq, nyq, lon_q, lat_q, mask, idx, area, &clon, &clat);
  if (nx < 0) fatal(fg_last_error());
  const size_t ni = (size_t)nx * sizeof(int), nd = (size_t)nx * sizeof(double);
  memcpy(box_is_src ? i_in : i_out, idx[0].data(), ni); memcpy(box_is_src ? j_in : j_out, idx[1].data(), ni);
  memcpy(box_is_src ? i_out : i_in, idx[2].data(), ni); memcpy(box_is_src ? j_out : j_in, idx[3].data(), ni);
  memcpy(xgrid_area, area.data(), nd);
  if (order == 2) { memcpy(xgrid_clon, clon.data(), nd); memcpy(xgrid_clat, clat.data(), nd); }
  return (int)nx;
}

// clip / box_ctrlat / box_ctrlon / get_grid_area_no_adjust (create_xgrid.h:37-45)
extern "C" int clip(const double lon_in[], const double lat_in[], int n_in, double ll_lon, double ll_lat, double ur_lon, double ur_lat,
                    double lon_out[], double lat_out[])
{
  if (n_in < 1 || n_in > 12) fatal("clip (HIP): 1 <= n_in <= 12");
  const int dev = fg_env_device();
  if (hipSetDevice(dev) != hipSuccess) fatal("no HIP device visible: libfregrid_hip needs an MI355X-class GPU");
  double *d = (double *)g_pool.get(dev, (4 * 16 + 2) * sizeof(double));
  if (!d) fatal("out of device memory");
  int *dn = (int *)(d + 64);
  int n = 0;
  bool ok = hipMemcpy(d, lon_in, n_in * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d + 16, lat_in, n_in * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    fgd_clip_single(d, d + 16, n_in, ll_lon, ll_lat, ur_lon, ur_lat, d + 32, d + 48, dn, nullptr);
    ok = hipMemcpy(&n, dn, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && n > 0) ok = hipMemcpy(lon_out, d + 32, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
                          hipMemcpy(lat_out, d + 48, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
  }
  g_pool.put(d);
  if (!ok) fatal("clip: HIP copy/launch failed");
  if (n < 0) fatal("clip (HIP): clipped polygon exceeds 16 vertices");
  return n;
}

static void b1_box_ctr(double ll_lon, double ll_lat, double ur_lon, double ur_lat, double clon, double out[2])
{
  const int dev = fg_env_device();
  if (hipSetDevice(dev) != hipSuccess) fatal("no HIP device visible: libfregrid_hip needs an MI355X-class GPU");
  double *d = (double *)g_pool.get(dev, 2 * sizeof(double));
  if (!d) fatal("out of device memory");
  fgd_box_ctr(ll_lon, ll_lat, ur_lon, ur_lat, clon, d, nullptr);
  bool ok = hipMemcpy(out, d, 2 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
  g_pool.put(d);
  if (!ok) fatal("box_ctr: HIP copy/launch failed");
}
extern "C" double box_ctrlat(double ll_lon, double ll_lat, double ur_lon, double ur_lat)
{
  double o[2]; b1_box_ctr(ll_lon, ll_lat, ur_lon, ur_lat, 0.0, o); return o[0];
}
extern "C" double box_ctrlon(double ll_lon, double ll_lat, double ur_lon, double ur_lat, double clon)
{
  double o[2]; b1_box_ctr(ll_lon, ll_lat, ur_lon, ur_lat, clon, o); return o[1];
}

extern "C" void get_grid_area_no_adjust(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area)
{
  const int nx = *nlon, ny = *nlat, dev = fg_env_device();
  if (nx < 1 || ny < 1) fatal("get_grid_area_no_adjust: bad grid sizes");
  if (hipSetDevice(dev) != hipSuccess) fatal("no HIP device visible: libfregrid_hip needs an MI355X-class GPU");
  const size_t np = (size_t)(nx + 1) * (ny + 1), nc = (size_t)nx * ny;
  double *d = (double *)g_pool.get(dev, (2 * np + nc) * sizeof(double));
  if (!d) fatal("out of device memory");
  bool ok = hipMemcpy(d, lon, np * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d + np, lat, np * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    fgd_grid_area_no_adjust(nx, ny, d, d + np, d + 2 * np, nullptr);
    ok = hipMemcpy(area, d + 2 * np, nc * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
  }
  g_pool.put(d);
  if (!ok) fatal("get_grid_area_no_adjust: HIP copy/launch failed");
}
extern "C" void get_grid_area_no_adjust_(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area)
{
  get_grid_area_no_adjust(nlon, nlat, lon, lat, area);
}

#define B1_BOX_FN(NAME, BOXSRC, ORDER)                                                                                          \
  extern "C" int NAME(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out, const double *lon_in, \
                      const double *lat_in, const double *lon_out, const double *lat_out, const double *mask_in, int *i_in,     \
                      int *j_in, int *i_out, int *j_out, double *xgrid_area B1_BOX_EXTRA_##ORDER)                              \
  {                                                                                                                             \
    return (BOXSRC) ? b1_create_xgrid_box(1, ORDER, *nlon_in, *nlat_in, lon_in, lat_in, *nlon_out, *nlat_out, lon_out, lat_out, \
                                          mask_in, i_in, j_in, i_out, j_out, xgrid_area, B1_BOX_ARGS_##ORDER)                   \
                    : b1_create_xgrid_box(0, ORDER, *nlon_out, *nlat_out, lon_out, lat_out, *nlon_in, *nlat_in, lon_in, lat_in, \
                                          mask_in, i_in, j_in, i_out, j_out, xgrid_area, B1_BOX_ARGS_##ORDER);                  \
  }
#define B1_BOX_EXTRA_1
#define B1_BOX_EXTRA_2 , double *xgrid_clon, double *xgrid_clat
#define B1_BOX_ARGS_1 nullptr, nullptr
#define B1_BOX_ARGS_2 xgrid_clon, xgrid_clat
B1_BOX_FN(create_xgrid_1dx2d_order1, 1, 1)
B1_BOX_FN(create_xgrid_1dx2d_order1_, 1, 1)
B1_BOX_FN(create_xgrid_1dx2d_order2, 1, 2)
B1_BOX_FN(create_xgrid_1dx2d_order2_, 1, 2)
B1_BOX_FN(create_xgrid_2dx1d_order1, 0, 1)
B1_BOX_FN(create_xgrid_2dx1d_order1_, 0, 1)
B1_BOX_FN(create_xgrid_2dx1d_order2, 0, 2)
B1_BOX_FN(create_xgrid_2dx1d_order2_, 0, 2)

static int b1_create_xgrid(int order, const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out,
                           const double *lon_in, const double *lat_in, const double *lon_out, const double *lat_out,
                           const double *mask_in, int *i_in, int *j_in, int *i_out, int *j_out,
                           double *xgrid_area, double *xgrid_clon, double *xgrid_clat)
{
  int nx1 = *nlon_in, ny1 = *nlat_in;
  const double *lons[1] = {lon_in}, *lats[1] = {lat_in}, *masks[1] = {mask_in};
  fg_plan *pl = nullptr;
  long nx = fg_plan_create(order, 1, &nx1, &ny1, lons, lats, masks, *nlon_out, *nlat_out, lon_out, lat_out, fg_env_device(), &pl);
  if (nx < 0) fatal(fg_last_error());
  if (nx >= (long)MAXXGRID)                                     // create_xgrid.c:1087-1088
    fatal("nxgrid is greater than MAXXGRID/nthreads, increase MAXXGRID, decrease nthreads, or increase number of MPI ranks");
  if (fg_plan_get_xgrid(pl, nullptr, i_in, j_in, i_out, j_out, xgrid_area, xgrid_clon, xgrid_clat)) fatal(fg_last_error());
  fg_plan_destroy(pl);
  return (int)nx;
}

extern "C" int create_xgrid_2dx2d_order1(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out,
                                         const double *lon_in, const double *lat_in, const double *lon_out, const double *lat_out,
                                         const double *mask_in, int *i_in, int *j_in, int *i_out, int *j_out, double *xgrid_area)
{
  return b1_create_xgrid(FG_CONSERVE_ORDER1, nlon_in, nlat_in, nlon_out, nlat_out, lon_in, lat_in, lon_out, lat_out, mask_in,
                         i_in, j_in, i_out, j_out, xgrid_area, nullptr, nullptr);
}
extern "C" int create_xgrid_2dx2d_order2(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out,
                                         const double *lon_in, const double *lat_in, const double *lon_out, const double *lat_out,
                                         const double *mask_in, int *i_in, int *j_in, int *i_out, int *j_out,
                                         double *xgrid_area, double *xgrid_clon, double *xgrid_clat)
{
  return b1_create_xgrid(FG_CONSERVE_ORDER2, nlon_in, nlat_in, nlon_out, nlat_out, lon_in, lat_in, lon_out, lat_out, mask_in,
                         i_in, j_in, i_out, j_out, xgrid_area, xgrid_clon, xgrid_clat);
}
extern "C" int create_xgrid_2dx2d_order1_(const int *a, const int *b, const int *c, const int *d, const double *e, const double *f,
                                          const double *g, const double *h, const double *m, int *i1, int *j1, int *i2, int *j2, double *xa)
{
  return create_xgrid_2dx2d_order1(a, b, c, d, e, f, g, h, m, i1, j1, i2, j2, xa);
}
extern "C" int create_xgrid_2dx2d_order2_(const int *a, const int *b, const int *c, const int *d, const double *e, const double *f,
                                          const double *g, const double *h, const double *m, int *i1, int *j1, int *i2, int *j2,
                                          double *xa, double *xl, double *xt)
{
  return create_xgrid_2dx2d_order2(a, b, c, d, e, f, g, h, m, i1, j1, i2, j2, xa, xl, xt);
}

static int plan_apply_frac(fg_plan *pl, const double *data, double *out)
{
  fgd_apply_frac(pl->ndst, pl->csr, data, out, pl->stream);
  FGCHK(hipStreamSynchronize(pl->stream));
  FGCHK(hipGetLastError());
  return 0;
}

extern "C" int fg_plan_apply_frac_dev(fg_plan *pl, const double *data_dev, double *out_dev)
{
  if (!pl || !data_dev || !out_dev) return fg_fail(FG_ERR_ARG, "fg_plan_apply_frac_dev: null argument");
  if (!pl->finalized || pl->order != 1) return fg_fail(FG_ERR_STATE, "fg_plan_apply_frac_dev: needs a finalized first-order plan");
  FGCHK(hipSetDevice(pl->device));
  return plan_apply_frac(pl, data_dev, out_dev);
}

// interp.c:262-305: first-order remap with weights xarea / (sum of xarea over the destination cell); interp.c:312: the same
// with the great-circle exchange grid
static void b1_conserve_interp(bool great_circle, int nx_src, int ny_src, int nx_dst, int ny_dst, const double *x_src,
                               const double *y_src, const double *x_dst, const double *y_dst,
                               const double *mask_src, const double *data_src, double *data_dst)
{
  const double *lons[1] = {x_src}, *lats[1] = {y_src}, *masks[1] = {mask_src};
  fg_plan *pl = nullptr;
  long nx = great_circle ? fg_plan_create_great_circle(1, &nx_src, &ny_src, lons, lats, masks, nx_dst, ny_dst, x_dst, y_dst, fg_env_device(), &pl)
                         : fg_plan_create(FG_CONSERVE_ORDER1, 1, &nx_src, &ny_src, lons, lats, masks, nx_dst, ny_dst, x_dst, y_dst, fg_env_device(), &pl);
  if (nx < 0) fatal(fg_last_error());
  if (great_circle && nx > (long)MAXXGRID) fatal("nxgrid is greater than MAXXGRID, increase MAXXGRID");
  if (!great_circle && nx >= (long)MAXXGRID)
    fatal("The xgrid size is too large for resources.\n nxgrid is greater than MAXXGRID/nthreads; increase MAXXGRID,\n"
          " decrease nthreads, or increase number of MPI ranks.");
  if (fg_plan_finalize(pl, nullptr)) fatal(fg_last_error());
  size_t ns = (size_t)nx_src * ny_src, nd = (size_t)nx_dst * ny_dst;
  double *dsrc = nullptr, *ddst = nullptr;
  if (hipMalloc(&dsrc, ns * sizeof(double)) != hipSuccess || hipMalloc(&ddst, nd * sizeof(double)) != hipSuccess) fatal("hipMalloc failed");
  if (hipMemcpy(dsrc, data_src, ns * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) fatal("hipMemcpy failed");
  if (plan_apply_frac(pl, dsrc, ddst)) fatal(fg_last_error());
  if (hipMemcpy(data_dst, ddst, nd * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) fatal("hipMemcpy failed");
  (void)hipFree(dsrc); (void)hipFree(ddst);
  fg_plan_destroy(pl);
}
extern "C" void conserve_interp(int nx_src, int ny_src, int nx_dst, int ny_dst, const double *x_src,
                                const double *y_src, const double *x_dst, const double *y_dst,
                                const double *mask_src, const double *data_src, double *data_dst)
{
  b1_conserve_interp(false, nx_src, ny_src, nx_dst, ny_dst, x_src, y_src, x_dst, y_dst, mask_src, data_src, data_dst);
}
extern "C" void conserve_interp_great_circle(int nx_src, int ny_src, int nx_dst, int ny_dst, const double *x_src,
                                             const double *y_src, const double *x_dst, const double *y_dst,
                                             const double *mask_src, const double *data_src, double *data_dst)
{
  b1_conserve_interp(true, nx_src, ny_src, nx_dst, ny_dst, x_src, y_src, x_dst, y_dst, mask_src, data_src, data_dst);
}

// ----------------------------------------------------------------------------- polygon primitives
// Batched device versions + the single-polygon libfrencutils symbols built on them.
namespace {
struct DevBuf {
  void *p = nullptr;
  DevBuf(size_t n) { if (hipMalloc(&p, n ? n : 1) != hipSuccess) p = nullptr; }
  ~DevBuf() { if (p) (void)hipFree(p); }
};
}

// lon/lat arrays are [npoly][FG_POLY_STRIDE] (= 24) host arrays; n1/n2 <= 12 vertices each.
// n_out[p] = vertex count, 0 (empty), -1 (parallel edges: the reference is fatal here) or -2 (too many vertices).
extern "C" int fg_clip_2dx2d_batch(int npoly, const double *lon1, const double *lat1, const int *n1,
                                   const double *lon2, const double *lat2, const int *n2,
                                   double *lon_out, double *lat_out, int *n_out)
{
  if (npoly < 0 || !lon1 || !lat1 || !n1 || !lon2 || !lat2 || !n2 || !lon_out || !lat_out || !n_out) return fg_fail(FG_ERR_ARG, "null argument");
  if (npoly == 0) return 0;
  FGCHK(hipSetDevice(fg_env_device()));
  size_t nb = (size_t)npoly * FG_POLY_STRIDE * sizeof(double), ni = (size_t)npoly * sizeof(int);
  DevBuf a(nb), b(nb), c(nb), d(nb), xo(nb), yo(nb), m1(ni), m2(ni), mo(ni);
  if (!a.p || !b.p || !c.p || !d.p || !xo.p || !yo.p || !m1.p || !m2.p || !mo.p) return fg_fail(FG_ERR_HIP, "out of device memory");
  FGCHK(hipMemcpy(a.p, lon1, nb, hipMemcpyHostToDevice)); FGCHK(hipMemcpy(b.p, lat1, nb, hipMemcpyHostToDevice));
  FGCHK(hipMemcpy(c.p, lon2, nb, hipMemcpyHostToDevice)); FGCHK(hipMemcpy(d.p, lat2, nb, hipMemcpyHostToDevice));
  FGCHK(hipMemcpy(m1.p, n1, ni, hipMemcpyHostToDevice)); FGCHK(hipMemcpy(m2.p, n2, ni, hipMemcpyHostToDevice));
  fgd_poly_clip(npoly, (double *)a.p, (double *)b.p, (int *)m1.p, (double *)c.p, (double *)d.p, (int *)m2.p,
                (double *)xo.p, (double *)yo.p, (int *)mo.p, 0);
  FGCHK(hipDeviceSynchronize());
  FGCHK(hipMemcpy(lon_out, xo.p, nb, hipMemcpyDeviceToHost)); FGCHK(hipMemcpy(lat_out, yo.p, nb, hipMemcpyDeviceToHost));
  FGCHK(hipMemcpy(n_out, mo.p, ni, hipMemcpyDeviceToHost));
  return 0;
}

// op 0 poly_area, 1 poly_ctrlon(clon), 2 poly_ctrlat, 3 fix_lon(tlon = clon) in place (lon/lat/n updated);
// 4, 5, 6: area, ctrlon(clon), ctrlat as the clip kernels' fused integrals routine computes them.
extern "C" int fg_poly_op_batch(int op, int npoly, double *lon, double *lat, int *n, const double *clon, double *result)
{
  if (op < 0 || op > 6 || npoly < 0 || !lon || !lat || !n) return fg_fail(FG_ERR_ARG, "bad argument");
  if ((op == 1 || op == 3 || op == 5) && !clon) return fg_fail(FG_ERR_ARG, "clon/tlon array required");
  if (op != 3 && !result) return fg_fail(FG_ERR_ARG, "result array required");
  if (npoly == 0) return 0;
  FGCHK(hipSetDevice(fg_env_device()));
  size_t nb = (size_t)npoly * FG_POLY_STRIDE * sizeof(double), ni = (size_t)npoly * sizeof(int), nd = (size_t)npoly * sizeof(double);
  DevBuf a(nb), b(nb), m(ni), cl(nd), r(nd);
  if (!a.p || !b.p || !m.p || !cl.p || !r.p) return fg_fail(FG_ERR_HIP, "out of device memory");
  FGCHK(hipMemcpy(a.p, lon, nb, hipMemcpyHostToDevice)); FGCHK(hipMemcpy(b.p, lat, nb, hipMemcpyHostToDevice));
  FGCHK(hipMemcpy(m.p, n, ni, hipMemcpyHostToDevice));
  if (clon) FGCHK(hipMemcpy(cl.p, clon, nd, hipMemcpyHostToDevice));
  fgd_poly_op(op, npoly, (double *)a.p, (double *)b.p, (int *)m.p, (double *)cl.p, (double *)r.p, 0);
  FGCHK(hipDeviceSynchronize());
  if (op == 3) {
    FGCHK(hipMemcpy(lon, a.p, nb, hipMemcpyDeviceToHost)); FGCHK(hipMemcpy(lat, b.p, nb, hipMemcpyDeviceToHost));
    FGCHK(hipMemcpy(n, m.p, ni, hipMemcpyDeviceToHost));
  } else FGCHK(hipMemcpy(result, r.p, nd, hipMemcpyDeviceToHost));
  return 0;
}

// single-polygon libfrencutils symbols (create_xgrid.h:35-46, mosaic_util.h:95-101)
extern "C" int clip_2dx2d(const double lon1_in[], const double lat1_in[], int n1_in, const double lon2_in[],
                          const double lat2_in[], int n2_in, double lon_out[], double lat_out[])
{
  double a[FG_POLY_STRIDE] = {0}, b[FG_POLY_STRIDE] = {0}, c[FG_POLY_STRIDE] = {0}, d[FG_POLY_STRIDE] = {0};
  double xo[FG_POLY_STRIDE], yo[FG_POLY_STRIDE];
  if (n1_in > 12 || n2_in > 12 || n1_in < 1 || n2_in < 1) fatal("clip_2dx2d: this build supports 1..12 vertices per polygon");
  for (int k = 0; k < n1_in; k++) { a[k] = lon1_in[k]; b[k] = lat1_in[k]; }
  for (int k = 0; k < n2_in; k++) { c[k] = lon2_in[k]; d[k] = lat2_in[k]; }
  int no = 0;
  if (fg_clip_2dx2d_batch(1, a, b, &n1_in, c, d, &n2_in, xo, yo, &no)) fatal(fg_last_error());
  if (no == -1) fatal("the line between <x1_0,y1_0> and  <x1_1,y1_1> should not parallel to "
                      "the line between <x2_0,y2_0> and  <x2_1,y2_1>");
  if (no < 0) fatal("clip_2dx2d: clipped polygon exceeds 24 vertices");
  for (int k = 0; k < no; k++) { lon_out[k] = xo[k]; lat_out[k] = yo[k]; }
  return no;
}
static double poly_single(int op, const double x[], const double y[], int n, double clon)
{
  double a[FG_POLY_STRIDE] = {0}, b[FG_POLY_STRIDE] = {0}, r = 0;
  if (n < 1 || n > FG_POLY_STRIDE) fatal("polygon primitive: this build supports 1..24 vertices");
  for (int k = 0; k < n; k++) { a[k] = x[k]; b[k] = y[k]; }
  if (fg_poly_op_batch(op, 1, a, b, &n, &clon, &r)) fatal(fg_last_error());
  return r;
}
extern "C" double poly_area(const double x[], const double y[], int n) { return poly_single(0, x, y, n, 0.0); }
extern "C" double poly_ctrlon(const double x[], const double y[], int n, double clon) { return poly_single(1, x, y, n, clon); }
extern "C" double poly_ctrlat(const double x[], const double y[], int n) { return poly_single(2, x, y, n, 0.0); }
extern "C" int fix_lon(double x[], double y[], int n, double tlon)
{
  double a[FG_POLY_STRIDE] = {0}, b[FG_POLY_STRIDE] = {0};
  if (n < 1 || n > 8) fatal("fix_lon: this build supports 1..8 vertices");
  for (int k = 0; k < n; k++) { a[k] = x[k]; b[k] = y[k]; }
  if (fg_poly_op_batch(3, 1, a, b, &n, &tlon, nullptr)) fatal(fg_last_error());
  if (n < 0) fatal("fix_lon: vertex capacity exceeded");
  for (int k = 0; k < n; k++) { x[k] = a[k]; y[k] = b[k]; }
  return n;
}
extern "C" void pimod(double x[], int nn)
{
  const double PI = 3.14159265358979323846;
  for (int i = 0; i < nn; i++) { if (x[i] < -PI) x[i] += 2.0 * PI; else if (x[i] > PI) x[i] -= 2.0 * PI; }
}

// ----------------------------------------------------------------------------- order-2 input preparation
// fg_c2l: per-mosaic state for get_input_data's order-2 branch on the device (fregrid_util.c:2137-2216):
// halo fill across tile contacts, grad_c2l, gradient mask.  Geometry (calc_c2l_grid_info) is computed once on
// the host in the reference's operation order (c2l_host.c) and kept in HBM.
extern "C" int fg_c2l_grid_info(int nx, int ny, const double *xt, const double *yt, const double *xc, const double *yc,
                                double *dx, double *dy, double *area, double *edge_w, double *edge_e, double *edge_s,
                                double *edge_n, double *en_n, double *en_e, double *vlon, double *vlat);
extern "C" int fg_halo_map(int ntiles, const int *nx, const int *ny, int ncontacts, const int *tile1, const int *tile2,
                           const int *istart1, const int *iend1, const int *jstart1, const int *jend1,
                           const int *istart2, const int *iend2, const int *jstart2, const int *jend2,
                           long *map_off, int *map);

struct fg_c2l {
  int device = 0, ntiles = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  long ncells = 0, F = 0;
  std::vector<int> nx, ny;
  std::vector<void *> owned;
  void *tiles_dev = nullptr;
  int *map_dev = nullptr;
  int *cell_of_dev = nullptr;                     // halo'd element -> unpadded cell whose value it holds after update_halo (-1: zero)
  double *geom_dev[11] = {nullptr};
  std::vector<double> lont_halo, latt_halo;       // host copies (tests / inspection)
  template <typename T> T *alloc(size_t n) { void *p = g_pool.get(device, n * sizeof(T)); if (p) owned.push_back(p); return (T *)p; }
};

extern "C" void fg_c2l_destroy(fg_c2l *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  if (h->own_stream) g_handles.put_stream(h->device, h->stream);
  for (void *p : h->owned) g_pool.put(p);
  delete h;
}

extern "C" int fg_c2l_create(int ntiles, const int *nx, const int *ny, const double *const *lonc, const double *const *latc,
                             const double *const *lont, const double *const *latt,
                             int ncontacts, const int *tile1, const int *tile2,
                             const int *istart1, const int *iend1, const int *jstart1, const int *jend1,
                             const int *istart2, const int *iend2, const int *jstart2, const int *jend2,
                             int device, fg_c2l **out)
{
  if (ntiles < 1 || !nx || !ny || !lonc || !latc || !lont || !latt || !out) return fg_fail(FG_ERR_ARG, "null argument");
  if (int rc = fg_use_device("fg_c2l_create", device)) return rc;
  fg_c2l *h = new fg_c2l();
  h->device = device; h->ntiles = ntiles;
  std::vector<long> cell_off(ntiles + 1), f_off(ntiles + 1), dx_off(ntiles + 1), dy_off(ntiles + 1), ew_off(ntiles + 1), es_off(ntiles + 1);
  long co = 0, fo = 0, xo = 0, yo = 0, wo = 0, so = 0;
  for (int t = 0; t < ntiles; t++) {
    if (nx[t] < 2 || ny[t] < 2) { delete h; return fg_fail(FG_ERR_ARG, "tiles need at least 2x2 cells for the gradient"); }
    h->nx.push_back(nx[t]); h->ny.push_back(ny[t]);
    cell_off[t] = co; f_off[t] = fo; dx_off[t] = xo; dy_off[t] = yo; ew_off[t] = wo; es_off[t] = so;
    co += (long)nx[t] * ny[t]; fo += (long)(nx[t] + 2) * (ny[t] + 2);
    xo += (long)nx[t] * (ny[t] + 1); yo += (long)(nx[t] + 1) * ny[t]; wo += ny[t] + 1; so += nx[t] + 1;
  }
  h->ncells = co; h->F = fo;
  // halo map (setup_boundary + update_halo semantics)
  std::vector<long> map_off(ntiles + 1);
  std::vector<int> map(fo);
  int rc = fg_halo_map(ntiles, nx, ny, ncontacts, tile1, tile2, istart1, iend1, jstart1, jend1, istart2, iend2, jstart2, jend2,
                       map_off.data(), map.data());
  if (rc) { delete h; return fg_fail(rc, "fregrid_util: inconsistent contact description (size mismatch between the boundary)"); }
  // halo'd cell centres: interior copy, zero halo (init_halo), then the same halo update as the data
  h->lont_halo.assign(fo, 0.0); h->latt_halo.assign(fo, 0.0);
  for (int t = 0; t < ntiles; t++)
    for (int j = 0; j < ny[t]; j++) for (int i = 0; i < nx[t]; i++) {
      h->lont_halo[f_off[t] + (long)(j + 1) * (nx[t] + 2) + i + 1] = lont[t][(long)j * nx[t] + i];
      h->latt_halo[f_off[t] + (long)(j + 1) * (nx[t] + 2) + i + 1] = latt[t][(long)j * nx[t] + i];
    }
  for (long e = 0; e < fo; e++) if (map[e] >= 0) { h->lont_halo[e] = h->lont_halo[map[e]]; h->latt_halo[e] = h->latt_halo[map[e]]; }
  // geometry per tile
  std::vector<double> dx(xo), dy(yo), area(co), ew(wo), ee(wo), es(so), en(so), enn(3 * xo), ene(3 * yo), vlon(3 * co), vlat(3 * co);
  {
    // a thread per tile: the tiles' outputs are disjoint, the arithmetic per cell is the host routine's (calc_c2l_grid_info,
    // gradient_c2l.c:368-454) either way -- 0.38 s for a C384 mosaic on one core
    std::vector<int> rcs(ntiles, 0);
    std::vector<std::thread> workers;
    auto one = [&](int t) {
      rcs[t] = fg_c2l_grid_info(nx[t], ny[t], h->lont_halo.data() + f_off[t], h->latt_halo.data() + f_off[t], lonc[t], latc[t],
                                dx.data() + dx_off[t], dy.data() + dy_off[t], area.data() + cell_off[t], ew.data() + ew_off[t],
                                ee.data() + ew_off[t], es.data() + es_off[t], en.data() + es_off[t], enn.data() + 3 * dx_off[t],
                                ene.data() + 3 * dy_off[t], vlon.data() + 3 * cell_off[t], vlat.data() + 3 * cell_off[t]);
    };
    for (int t = 1; t < ntiles; t++) workers.emplace_back(one, t);
    one(0);
    for (std::thread &w : workers) w.join();
    for (int t = 0; t < ntiles; t++) if (rcs[t]) { rc = rcs[t]; delete h; return fg_fail(rc, "fg_c2l_grid_info failed"); }
  }
  h->stream = g_handles.get_stream(device);
  if (!h->stream) { delete h; return fg_fail(FG_ERR_HIP, "hipStreamCreate failed"); }
  std::vector<char> th(fgd_c2l_tile_size() * ntiles);
  for (int t = 0; t < ntiles; t++) fgd_c2l_tile_fill(th.data(), t, nx[t], ny[t], cell_off[t], f_off[t], dx_off[t], dy_off[t], ew_off[t], es_off[t]);
  const std::vector<double> *src[11] = {&dx, &dy, &area, &ew, &ee, &es, &en, &enn, &ene, &vlon, &vlat};
  bool ok = true;
  h->tiles_dev = h->alloc<char>(th.size()); h->map_dev = h->alloc<int>(fo); h->cell_of_dev = h->alloc<int>(fo);
  ok = ok && h->tiles_dev && h->map_dev && h->cell_of_dev;
  // the gather map composed with the packing: which unpadded cell ends up in each halo'd element
  std::vector<int> cell_of(fo, -1);
  for (int t = 0; t < ntiles; t++)
    for (int j = 0; j < ny[t]; j++) for (int i = 0; i < nx[t]; i++)
      cell_of[f_off[t] + (long)(j + 1) * (nx[t] + 2) + i + 1] = (int)(cell_off[t] + (long)j * nx[t] + i);
  for (long e = 0; e < fo; e++) if (map[e] >= 0) cell_of[e] = cell_of[map[e]];     // sources are interior elements
  ok = ok && hipMemcpy(h->cell_of_dev, cell_of.data(), fo * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  for (int k = 0; k < 11 && ok; k++) { h->geom_dev[k] = h->alloc<double>(src[k]->size()); ok = ok && h->geom_dev[k]; }
  if (!ok) { fg_c2l_destroy(h); return fg_fail(FG_ERR_HIP, "out of device memory"); }
  ok = ok && hipMemcpy(h->tiles_dev, th.data(), th.size(), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(h->map_dev, map.data(), fo * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  for (int k = 0; k < 11 && ok; k++) ok = hipMemcpy(h->geom_dev[k], src[k]->data(), src[k]->size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { fg_c2l_destroy(h); return fg_fail(FG_ERR_HIP, "upload of the gradient geometry failed"); }
  *out = h;
  return 0;
}

extern "C" long fg_c2l_ncells(const fg_c2l *h) { return h ? h->ncells : FG_ERR_ARG; }
extern "C" long fg_c2l_halo_size(const fg_c2l *h) { return h ? h->F : FG_ERR_ARG; }
extern "C" int fg_c2l_set_stream(fg_c2l *h, void *stream)
{
  if (!h) return fg_fail(FG_ERR_ARG, "null handle");
  FGCHK(hipSetDevice(h->device));
  FGCHK(hipStreamSynchronize(h->stream));
  if (h->own_stream) g_handles.put_stream(h->device, h->stream);
  h->stream = (hipStream_t)stream; h->own_stream = false;
  return 0;
}
int fg_c2l_borrow_stream(fg_c2l *h, void *stream, void **saved, int *saved_own)      // (see fg_plan_borrow_stream)
{
  if (!h) return fg_fail(FG_ERR_ARG, "null handle");
  FGCHK(hipSetDevice(h->device));
  FGCHK(hipStreamSynchronize(h->stream));
  *saved = (void *)h->stream; *saved_own = h->own_stream ? 1 : 0;
  h->stream = (hipStream_t)stream; h->own_stream = false;
  return 0;
}
void fg_c2l_return_stream(fg_c2l *h, void *saved, int saved_own)
{
  if (!h) return;
  h->stream = (hipStream_t)saved; h->own_stream = saved_own != 0;
}
extern "C" int fg_c2l_sync(fg_c2l *h)
{
  if (!h) return fg_fail(FG_ERR_ARG, "null handle");
  FGCHK(hipStreamSynchronize(h->stream));
  return 0;
}
// host copies of the halo'd cell-centre arrays [F] (for tests)
extern "C" int fg_c2l_get_centres(const fg_c2l *h, double *lont_halo, double *latt_halo)
{
  if (!h) return fg_fail(FG_ERR_ARG, "null handle");
  if (lont_halo) memcpy(lont_halo, h->lont_halo.data(), h->F * sizeof(double));
  if (latt_halo) memcpy(latt_halo, h->latt_halo.data(), h->F * sizeof(double));
  return 0;
}

// src [nz][ncells] (tiles back to back, no halo) -> halo_data [nz][F] with the halo filled from the neighbours.
// src == NULL: halo_data already holds the interiors, only the halo is filled.  Device pointers.
extern "C" int fg_c2l_fill_halo(fg_c2l *h, const double *src, double *halo_data, int nz)
{
  if (!h || !halo_data || nz < 1) return fg_fail(FG_ERR_ARG, "bad argument");
  FGCHK(hipSetDevice(h->device));
  if (src) {
    FGCHK(hipMemsetAsync(halo_data, 0, (size_t)nz * h->F * sizeof(double), h->stream));   // init_halo (corners stay 0)
    fgd_pack_interior(h->tiles_dev, h->ntiles, h->ncells, h->F, nz, src, halo_data, h->stream);
  }
  fgd_halo_gather(h->F, nz, h->map_dev, halo_data, h->stream);
  FGCHK(hipGetLastError());
  return 0;
}

// grad_c2l for every tile and level: halo_data [nz][F] -> grad_x, grad_y [nz][ncells]; grad_mask (int [nz][ncells],
// may be NULL) is filled when has_missing (fregrid_util.c:2203-2216), zeroed otherwise.  Device pointers.
extern "C" int fg_c2l_gradient(fg_c2l *h, const double *halo_data, int nz, int has_missing, double missing,
                               double *grad_x, double *grad_y, int *grad_mask)
{
  if (!h || !halo_data || !grad_x || !grad_y || nz < 1) return fg_fail(FG_ERR_ARG, "bad argument");
  FGCHK(hipSetDevice(h->device));
  fgd_grad_c2l(h->tiles_dev, h->ntiles, h->ncells, h->F, nz, halo_data, (const double *const *)h->geom_dev, grad_x, grad_y, h->stream);
  if (grad_mask) {
    if (has_missing) fgd_grad_mask(h->tiles_dev, h->ntiles, h->ncells, h->F, nz, halo_data, missing, grad_mask, h->stream);
    else FGCHK(hipMemsetAsync(grad_mask, 0, (size_t)nz * h->ncells * sizeof(int), h->stream));
  }
  FGCHK(hipGetLastError());
  return 0;
}

extern "C" int fg_c2l_records(fg_c2l *h, const double *src, int nz, double *rec)
{
  if (!h || !src || !rec) return fg_fail(FG_ERR_ARG, "bad argument");
  if (nz < 1 || nz > 8) return fg_fail(FG_ERR_ARG, "fg_c2l_records: 1 to 8 levels per call");
  FGCHK(hipSetDevice(h->device));
  fgd_c2l_records(h->tiles_dev, h->ntiles, h->ncells, nz, levels_pad(nz), src, h->cell_of_dev, (const double *const *)h->geom_dev, rec, h->stream);
  FGCHK(hipGetLastError());
  return 0;
}

extern "C" int fg_c2l_records_levels(fg_c2l *h, const double *src, int nz, double missing, double *rec, unsigned char *maskbits)
{
  if (!h || !src || !rec || !maskbits) return fg_fail(FG_ERR_ARG, "fg_c2l_records_levels: null argument");
  if (nz < 1 || nz > 8) return fg_fail(FG_ERR_ARG, "fg_c2l_records_levels: 1 to 8 levels per call");
  FGCHK(hipSetDevice(h->device));
  fgd_c2l_records_levels(h->tiles_dev, h->ntiles, h->ncells, nz, src, h->cell_of_dev, (const double *const *)h->geom_dev, missing, rec,
                         maskbits, h->stream);
  FGCHK(hipGetLastError());
  return 0;
}

extern "C" int fg_c2l_records_levels_mono(fg_c2l *h, const double *src, int nz, double missing, double *rec, unsigned char *maskbits,
                                          double *b8)
{
  if (!h || !src || !rec || !maskbits || !b8) return fg_fail(FG_ERR_ARG, "fg_c2l_records_levels_mono: null argument");
  if (nz < 1 || nz > 8) return fg_fail(FG_ERR_ARG, "fg_c2l_records_levels_mono: 1 to 8 levels per call");
  FGCHK(hipSetDevice(h->device));
  fgd_c2l_records_levels_mono(h->tiles_dev, h->ntiles, h->ncells, nz, src, h->cell_of_dev, (const double *const *)h->geom_dev, missing, rec,
                              maskbits, b8, h->stream);
  FGCHK(hipGetLastError());
  return 0;
}

extern "C" int fg_c2l_gradient_records(fg_c2l *h, const double *halo_data, int nz, double *rec)
{
  if (!h || !halo_data || !rec) return fg_fail(FG_ERR_ARG, "bad argument");
  if (nz < 1 || nz > 8) return fg_fail(FG_ERR_ARG, "fg_c2l_gradient_records: 1 to 8 levels per call");
  FGCHK(hipSetDevice(h->device));
  fgd_grad_c2l_rec(h->tiles_dev, h->ntiles, h->ncells, h->F, nz, levels_pad(nz), halo_data, (const double *const *)h->geom_dev, rec, h->stream);
  FGCHK(hipGetLastError());
  return 0;
}
