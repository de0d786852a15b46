// rland.hip -- host orchestration of remap_land's nearest-point search on the device (fg_rland_*): full_search_nearest and
// search_nearest_sface (tools/remap_land/remap_land.c:2520-2607).  Kernels: rland_kernels.hip; the rule shared with the host
// check: rland.h; the proof: DESIGN.md 3.10.
//
// Create: the source points' triples on the device (fgd_ro_xyz) and, once, their order along a space-filling curve.
// Search: the unmasked points in that order into tiles with balls, the smallest computed chord per query (phase 1), the points
// within RL_M of it (phase 2, a second launch of exact size for the queries with more than RL_K), and on the host the
// reference's own expression on those few points.  Queries the proof does not cover take the reference's loop on the host.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <vector>
#include "rland.h"
#include "fg_host.h"

static std::atomic<int> g_prune{1};
extern "C" void fg_set_rland_prune(int on) { g_prune = on ? 1 : 0; }
extern "C" int fg_rland_tile(void) { return RL_TILE; }

enum { RL_ST_QUERIES, RL_ST_TILES, RL_ST_VISITED, RL_ST_VISITED2, RL_ST_SURVIVORS, RL_ST_HOST, RL_ST_FALLBACK, RL_ST_OVERFLOW, RL_NSTAT };
enum { RL_MS_CONVERT, RL_MS_ORDER, RL_MS_QUERIES, RL_MS_TILES, RL_MS_PHASE1, RL_MS_PHASE2, RL_MS_OVERFLOW, RL_MS_FINISH, RL_NMS };

// a device buffer of the handle that only grows: a search allocates nothing once the handle has seen its sizes
struct RlBuf {
  void *p = nullptr;
  size_t cap = 0;
  ~RlBuf() { if (p) (void)hipFree(p); }
  template <typename T> T *need(size_t n)
  {
    const size_t bytes = (n ? n : 1) * sizeof(T);
    if (bytes > cap) {
      if (p) (void)hipFree(p);
      p = nullptr; cap = 0;
      if (hipMalloc(&p, bytes + bytes / 4) != hipSuccess) { p = nullptr; return nullptr; }
      cap = bytes + bytes / 4;
    }
    return (T *)p;
  }
  template <typename T> T *put(const T *src, size_t n)
  {
    T *d = need<T>(n);
    if (d && n && hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
  }
};

struct fg_rland {
  int device = 0, nface = 0, npts = 0;
  long n = 0;
  hipStream_t stream = nullptr;
  double *d_xyz = nullptr;                   // [3][n] by flat index (b_xyz)
  std::vector<double> lon, lat;              // the host's copies: the finish evaluates the reference's expression on them
  std::vector<int> order;                    // the flat indices along the curve
  bool in_range = true;                      // every source point within the proof's domain
  RlBuf b_xyz, b_ll, b_qxyz, b_oidx, b_q, b_pts, b_ball, b_gball, b_c, b_i, b_ovq, b_ovptr, b_ovout;
  long stats[RL_NSTAT] = {0};
  float ms[RL_NMS] = {0};
};

// Cube face of the triple and the Morton code of its two other coordinates over the major one, 16 bits each: points that are
// close on the sphere are close in the order, except across the seams of the code.  Any order gives the same answers.
static uint64_t rl_key(double x, double y, double z)
{
  if (!(x == x) || !(y == y) || !(z == z)) return ~(uint64_t)0;
  const double ax = fabs(x), ay = fabs(y), az = fabs(z);
  int f; double m, u, v;
  if (ax >= ay && ax >= az) { f = x < 0; m = ax; u = y; v = z; }
  else if (ay >= az) { f = 2 + (y < 0); m = ay; u = x; v = z; }
  else { f = 4 + (z < 0); m = az; u = x; v = y; }
  if (!(m > 0)) return 0;
  auto quant = [](double t) { const double w = (t + 1.0) * 32767.5; return (uint32_t)(w < 0 ? 0 : (w > 65535.0 ? 65535.0 : w)); };
  auto spread = [](uint32_t a) {
    uint64_t b = a;
    b = (b | (b << 8)) & 0x00ff00ffu; b = (b | (b << 4)) & 0x0f0f0f0fu; b = (b | (b << 2)) & 0x33333333u; b = (b | (b << 1)) & 0x55555555u;
    return b;
  };
  return ((uint64_t)f << 32) | spread(quant(u / m)) | (spread(quant(v / m)) << 1);
}

extern "C" void fg_rland_destroy(fg_rland *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  delete h;
}

static int rl_create(fg_rland *h, const double *lon_src, const double *lat_src)
{
  const long n = h->n;
  FGCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  double t0 = fg_now_ms();
  h->lon.assign(lon_src, lon_src + n); h->lat.assign(lat_src, lat_src + n);
  for (long l = 0; l < n; l++) if (!rl_in_range(lon_src[l], lat_src[l])) { h->in_range = false; break; }
  h->d_xyz = h->b_xyz.need<double>(3 * (size_t)n);
  double *d_ll = h->b_ll.need<double>(2 * (size_t)n);      // the searches reuse it for the destination points
  if (!h->d_xyz || !d_ll) return fg_fail(FG_ERR_HIP, "fg_rland_create: out of device memory");
  std::vector<double> xyz(3 * (size_t)n);
  FGCHK(hipMemcpy(d_ll, lon_src, n * sizeof(double), hipMemcpyHostToDevice));
  FGCHK(hipMemcpy(d_ll + n, lat_src, n * sizeof(double), hipMemcpyHostToDevice));
  fgd_ro_xyz(n, d_ll, d_ll + n, h->d_xyz, h->d_xyz + n, h->d_xyz + 2 * n, h->stream);
  FGCHK(hipGetLastError());
  FGCHK(hipMemcpyAsync(xyz.data(), h->d_xyz, xyz.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  FGCHK(hipStreamSynchronize(h->stream));
  double t1 = fg_now_ms();
  h->ms[RL_MS_CONVERT] = (float)(t1 - t0);
  std::vector<std::pair<uint64_t, int>> keyed((size_t)n);
  for (long l = 0; l < n; l++) keyed[l] = {rl_key(xyz[l], xyz[n + l], xyz[2 * n + l]), (int)l};
  std::sort(keyed.begin(), keyed.end());
  h->order.resize((size_t)n);
  for (long k = 0; k < n; k++) h->order[k] = keyed[k].second;
  h->ms[RL_MS_ORDER] = (float)(fg_now_ms() - t1);
  return 0;
}

extern "C" int fg_rland_create(int nface_src, int npts_src, const double *lon_src, const double *lat_src, fg_rland **out)
{
  if (!out) return fg_fail(FG_ERR_ARG, "fg_rland_create: null output handle");
  *out = nullptr;
  if (nface_src < 1 || npts_src < 1 || (long)nface_src * npts_src > 0x7fffffffL / RL_TILE)
    return fg_fail(FG_ERR_ARG, "fg_rland_create: bad source size %d x %d", nface_src, npts_src);
  if (!lon_src || !lat_src) return fg_fail(FG_ERR_ARG, "fg_rland_create: null grid argument");
  const int device = fg_env_device();
  int rc = fg_use_device("fg_rland_create", device);
  if (rc) return rc;
  fg_rland *h = new fg_rland;
  h->device = device; h->nface = nface_src; h->npts = npts_src; h->n = (long)nface_src * npts_src;
  rc = rl_create(h, lon_src, lat_src);
  if (rc) { fg_rland_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" void *fg_rland_stream(fg_rland *h) { return h ? (void *)h->stream : nullptr; }

// the destination points on the host and, converted, on the device.  lon_dst / lat_dst: host or device memory.
struct RlQueries {
  std::vector<double> lon, lat;
  double *d_xyz = nullptr;
  int npts = 0;
};
static int rl_queries(fg_rland *h, int npts_dst, const void *lon_dst, const void *lat_dst, RlQueries &qs)
{
  const size_t n = (size_t)npts_dst;
  const double t0 = fg_now_ms();
  qs.npts = npts_dst;
  qs.lon.resize(n); qs.lat.resize(n);
  double *d_ll = h->b_ll.need<double>(2 * n);
  qs.d_xyz = h->b_qxyz.need<double>(3 * n);
  if (!d_ll || !qs.d_xyz) return fg_fail(FG_ERR_HIP, "fg_rland_search: out of device memory");
  FGCHK(hipMemcpy(qs.lon.data(), lon_dst, n * sizeof(double), hipMemcpyDefault));
  FGCHK(hipMemcpy(qs.lat.data(), lat_dst, n * sizeof(double), hipMemcpyDefault));
  FGCHK(hipMemcpy(d_ll, qs.lon.data(), n * sizeof(double), hipMemcpyHostToDevice));
  FGCHK(hipMemcpy(d_ll + n, qs.lat.data(), n * sizeof(double), hipMemcpyHostToDevice));
  fgd_ro_xyz((long)n, d_ll, d_ll + n, qs.d_xyz, qs.d_xyz + n, qs.d_xyz + 2 * n, h->stream);
  FGCHK(hipGetLastError());
  FGCHK(hipStreamSynchronize(h->stream));
  h->ms[RL_MS_QUERIES] += (float)(fg_now_ms() - t0);
  return 0;
}

// The nearest unmasked point of the faces m0 .. m1-1 for the listed destination points: answer[k] is its flat index.
static int rl_search(fg_rland *h, const int *mask_src, int m0, int m1, const RlQueries &qs, const std::vector<int> &qlist, std::vector<long> &answer)
{
  const int nq = (int)qlist.size(), npts = h->npts, prune = g_prune;
  answer.assign((size_t)nq, -1);
  h->stats[RL_ST_QUERIES] += nq;
  if (nq < 1) return 0;
  hipStream_t st = h->stream;
  double t0 = fg_now_ms();
  const long l0 = (long)m0 * npts, l1 = (long)m1 * npts;
  std::vector<int> oidx;
  for (long k = 0; k < h->n; k++) { const int l = h->order[k]; if (l >= l0 && l < l1 && mask_src[l] != 0) oidx.push_back(l); }
  const int nsrc = (int)oidx.size();
  if (nsrc == 0) return fg_fail(FG_ERR_ARG, "remap_land(full_search_nearest): no nearest point is found");
  long first = l0;
  while (mask_src[first] == 0) first++;
  const RoTiles tl = ro_tiles_of(nsrc);
  const int ntiles = tl.ntiles, ngroups = tl.ngroups;
  h->stats[RL_ST_TILES] = ntiles;
  int *d_oidx = h->b_oidx.put(oidx.data(), oidx.size()), *d_q = h->b_q.put(qlist.data(), (size_t)nq);
  RoPoint *d_pts = h->b_pts.need<RoPoint>((size_t)ntiles * RL_TILE);
  RoBall *d_ball = h->b_ball.need<RoBall>(ntiles), *d_gball = h->b_gball.need<RoBall>(ngroups);
  double *d_c = h->b_c.need<double>(2 * (size_t)nq);
  int *d_i = h->b_i.need<int>((size_t)nq * (3 + RL_K));
  if (!d_oidx || !d_q || !d_pts || !d_ball || !d_gball || !d_c || !d_i) return fg_fail(FG_ERR_HIP, "fg_rland_search: device allocation or upload failed");
  const long n = h->n;
  fgd_ro_tiles(nsrc, d_oidx, h->d_xyz, h->d_xyz + n, h->d_xyz + 2 * n, d_pts, d_ball, d_gball, st);
  FGCHK(hipGetLastError());
  FGCHK(hipStreamSynchronize(st));
  double t1 = fg_now_ms();
  h->ms[RL_MS_TILES] += (float)(t1 - t0);
  RlSearch p;
  p.pts = d_pts; p.ball = d_ball; p.gball = d_gball;
  p.qx = qs.d_xyz; p.qy = qs.d_xyz + qs.npts; p.qz = qs.d_xyz + 2 * (size_t)qs.npts; p.qlist = d_q;
  p.sx = h->d_xyz; p.sy = h->d_xyz + n; p.sz = h->d_xyz + 2 * n; p.first = (int)first;
  p.cmin = d_c; p.cfirst = d_c + nq;
  p.count = d_i; p.visited = d_i + nq; p.slots = d_i + 3 * (size_t)nq;
  p.nq = nq; p.ntiles = ntiles; p.ngroups = ngroups;
  struct Events { hipEvent_t e[3] = {nullptr, nullptr, nullptr}; ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } } evs;
  hipEvent_t *ev = evs.e;
  for (int k = 0; k < 3; k++) FGCHK(hipEventCreate(&ev[k]));
  FGCHK(hipEventRecord(ev[0], st));
  fgd_rl_cmin(p, prune, st);
  FGCHK(hipGetLastError());
  FGCHK(hipEventRecord(ev[1], st));
  fgd_rl_survivors(p, prune, st);
  FGCHK(hipGetLastError());
  FGCHK(hipEventRecord(ev[2], st));
  std::vector<double> c(2 * (size_t)nq);
  std::vector<int> iv((size_t)nq * (3 + RL_K));
  FGCHK(hipMemcpyAsync(c.data(), d_c, c.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  FGCHK(hipMemcpyAsync(iv.data(), d_i, iv.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  FGCHK(hipStreamSynchronize(st));
  float ms1 = 0, ms2 = 0;
  FGCHK(hipEventElapsedTime(&ms1, ev[0], ev[1]));
  FGCHK(hipEventElapsedTime(&ms2, ev[1], ev[2]));
  h->ms[RL_MS_PHASE1] += ms1; h->ms[RL_MS_PHASE2] += ms2;
  const int *count = iv.data(), *visited = iv.data() + nq, *slots = iv.data() + 3 * (size_t)nq;
  for (int q = 0; q < nq; q++) { h->stats[RL_ST_VISITED] += visited[q]; h->stats[RL_ST_VISITED2] += visited[nq + q]; }
  // which queries take the reference's loop, and which have more survivors than slots
  std::vector<char> scan((size_t)nq);
  std::vector<int> ovq, ovptr(1, 0);
  for (int q = 0; q < nq; q++) {
    const int i = qlist[q];
    scan[q] = !h->in_range || count[q] < 1 || rl_needs_scan(c[q], c[(size_t)nq + q], qs.lon[i], qs.lat[i]);
    if (!scan[q] && count[q] > RL_K) { ovq.push_back(q); ovptr.push_back(ovptr.back() + count[q]); }
  }
  t0 = fg_now_ms();
  std::vector<int> ovout((size_t)ovptr.back());
  const int nov = (int)ovq.size();
  if (nov > 0) {
    int *d_ovq = h->b_ovq.put(ovq.data(), ovq.size()), *d_ovptr = h->b_ovptr.put(ovptr.data(), ovptr.size());
    int *d_ovout = h->b_ovout.need<int>(ovout.size());
    if (!d_ovq || !d_ovptr || !d_ovout) return fg_fail(FG_ERR_HIP, "fg_rland_search: device allocation or upload failed");
    FGCHK(hipMemsetAsync(d_ovout, 0xff, ovout.size() * sizeof(int), st));
    fgd_rl_overflow(p, nov, d_ovq, d_ovptr, d_ovout, prune, st);
    FGCHK(hipGetLastError());
    FGCHK(hipMemcpyAsync(ovout.data(), d_ovout, ovout.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    FGCHK(hipStreamSynchronize(st));
    for (int v : ovout) if (v < 0 || v >= n) return fg_fail(FG_ERR_HIP, "fg_rland_search: the overflow pass did not reproduce the survivor counts");
  }
  t1 = fg_now_ms();
  h->ms[RL_MS_OVERFLOW] += (float)(t1 - t0);
  h->stats[RL_ST_OVERFLOW] += nov;
  const double *slon = h->lon.data(), *slat = h->lat.data();
  for (int q = 0, ko = 0; q < nq; q++) {
    const int i = qlist[q];
    if (scan[q]) {
      answer[q] = rl_scan(m0, m1, npts, slon, slat, mask_src, qs.lon[i], qs.lat[i]);
      h->stats[RL_ST_FALLBACK]++;
      continue;
    }
    h->stats[RL_ST_SURVIVORS] += count[q];
    if (count[q] == 1) { answer[q] = slots[(size_t)q * RL_K]; continue; }
    h->stats[RL_ST_HOST]++;
    if (count[q] <= RL_K) answer[q] = rl_finish(count[q], slots + (size_t)q * RL_K, slon, slat, qs.lon[i], qs.lat[i]);
    else { answer[q] = rl_finish(count[q], ovout.data() + ovptr[ko], slon, slat, qs.lon[i], qs.lat[i]); ko++; }
  }
  h->ms[RL_MS_FINISH] += (float)(fg_now_ms() - t1);
  return 0;
}

static int rl_check_search(const char *who, fg_rland *h, const int *mask_src, int npts_dst, const void *lon_dst, const void *lat_dst,
                           const int *mask_dst)
{
  if (!h) return fg_fail(FG_ERR_ARG, "%s: null handle", who);
  if (npts_dst < 0 || !mask_src || (npts_dst > 0 && (!lon_dst || !lat_dst || !mask_dst))) return fg_fail(FG_ERR_ARG, "%s: bad argument", who);
  FGCHK(hipSetDevice(h->device));
  memset(h->stats, 0, sizeof h->stats);
  for (int k = RL_MS_QUERIES; k < RL_NMS; k++) h->ms[k] = 0;
  return 0;
}

extern "C" int fg_rland_search(fg_rland *h, const int *mask_src, int face, int npts_dst, const void *lon_dst, const void *lat_dst,
                               const int *mask_dst, int *idx_map, int *face_map)
{
  int rc = rl_check_search("fg_rland_search", h, mask_src, npts_dst, lon_dst, lat_dst, mask_dst);
  if (rc) return rc;
  if (face < -1 || face >= h->nface) return fg_fail(FG_ERR_ARG, "fg_rland_search: face %d of %d", face, h->nface);
  if (npts_dst > 0 && (!idx_map || !face_map)) return fg_fail(FG_ERR_ARG, "fg_rland_search: null output");
  std::vector<int> qlist;
  for (int i = 0; i < npts_dst; i++) { idx_map[i] = face_map[i] = -1; if (mask_dst[i] != 0) qlist.push_back(i); }
  if (qlist.empty()) return 0;
  RlQueries qs;
  rc = rl_queries(h, npts_dst, lon_dst, lat_dst, qs);
  if (rc) return rc;
  std::vector<long> ans;
  rc = rl_search(h, mask_src, face < 0 ? 0 : face, face < 0 ? h->nface : face + 1, qs, qlist, ans);
  if (rc) return rc;
  for (size_t q = 0; q < qlist.size(); q++) { idx_map[qlist[q]] = (int)(ans[q] % h->npts); face_map[qlist[q]] = (int)(ans[q] / h->npts); }
  return 0;
}

extern "C" int fg_rland_search_sface(fg_rland *h, const int *mask_src, int npts_dst, const void *lon_dst, const void *lat_dst,
                                     const int *mask_dst, const int *idx_map, const int *face_map, int iface_dst, int *idx_map_sf)
{
  int rc = rl_check_search("fg_rland_search_sface", h, mask_src, npts_dst, lon_dst, lat_dst, mask_dst);
  if (rc) return rc;
  if (iface_dst < 0 || iface_dst >= h->nface) return fg_fail(FG_ERR_ARG, "fg_rland_search_sface: face %d of %d", iface_dst, h->nface);
  if (npts_dst > 0 && (!idx_map || !face_map || !idx_map_sf)) return fg_fail(FG_ERR_ARG, "fg_rland_search_sface: null map");
  std::vector<int> qlist;
  for (int i = 0; i < npts_dst; i++) {
    if (mask_dst[i] == 0) idx_map_sf[i] = -1;
    else if (face_map[i] == iface_dst) idx_map_sf[i] = idx_map[i];
    else { idx_map_sf[i] = -1; qlist.push_back(i); }
  }
  if (qlist.empty()) return 0;
  RlQueries qs;
  rc = rl_queries(h, npts_dst, lon_dst, lat_dst, qs);
  if (rc) return rc;
  std::vector<long> ans;
  rc = rl_search(h, mask_src, iface_dst, iface_dst + 1, qs, qlist, ans);
  if (rc) return rc;
  for (size_t q = 0; q < qlist.size(); q++) idx_map_sf[qlist[q]] = (int)(ans[q] % h->npts);
  return 0;
}

extern "C" int fg_rland_stats(const fg_rland *h, long *stats, int n)
{
  if (!h || !stats || n < 0) return fg_fail(FG_ERR_ARG, "fg_rland_stats: bad argument");
  for (int k = 0; k < n && k < RL_NSTAT; k++) stats[k] = h->stats[k];
  return 0;
}

extern "C" int fg_rland_phase_ms(const fg_rland *h, float *ms, int n)
{
  if (!h || !ms || n < 0) return fg_fail(FG_ERR_ARG, "fg_rland_phase_ms: bad argument");
  for (int k = 0; k < n && k < RL_NMS; k++) ms[k] = h->ms[k];
  return 0;
}
