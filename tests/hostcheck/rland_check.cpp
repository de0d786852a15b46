// Host build of what the device shares with the host of remap_land's nearest-point search (csrc/rland.h on csrc/runoff.h), as a
// stand-alone program (test infrastructure; built by tests/rland_cases.py; a plain build, no sanitizer).
//   rland_check IN OUT
//   IN:  int mode (ignored), nface_src, npts_src, npts_dst, iface_dst, 0; double lon_src[n], lat_src[n]; int mask_src[n];
//        double lon_dst[npts_dst], lat_dst[..]; int mask_dst[..]       (the input of tests/capi/rland_ref_driver.c)
//   OUT: int idx_map[npts_dst], face_map[..], idx_map_sf[..]; long fallback, several: queries that took the reference's loop,
//        queries decided among several survivors
// The survivors are found by brute force over the point triples: the smallest computed chord, then every point within RL_M of
// it; the finish is rland.h's, the same code the library runs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rland.h"

struct Src {
  int nface, npts;
  std::vector<double> lon, lat, x, y, z;
  std::vector<int> mask;
  bool in_range;
};
static long g_fallback = 0, g_several = 0;

// the flat index of the answer over the faces m0 .. m1-1, or -1
static long nearest(const Src &s, int m0, int m1, double lon, double lat)
{
  const long l0 = (long)m0 * s.npts, l1 = (long)m1 * s.npts;
  long first = l0;
  while (first < l1 && s.mask[first] == 0) first++;
  if (first == l1) return -1;
  double qx, qy, qz;
  ro_xyz(lon, lat, &qx, &qy, &qz);
  double smin = (double)INFINITY;
  for (long l = l0; l < l1; l++) if (s.mask[l] != 0) { const double v = ro_sumsq(qx, qy, qz, s.x[l], s.y[l], s.z[l]); if (v < smin) smin = v; }
  const double cmin = sqrt(smin), cfirst = sqrt(ro_sumsq(qx, qy, qz, s.x[first], s.y[first], s.z[first]));
  std::vector<int> surv;
  for (long l = l0; l < l1; l++)
    if (s.mask[l] != 0 && rl_survives(sqrt(ro_sumsq(qx, qy, qz, s.x[l], s.y[l], s.z[l])), cmin + RL_M)) surv.push_back((int)l);
  if (!s.in_range || surv.empty() || rl_needs_scan(cmin, cfirst, lon, lat)) {
    g_fallback++;
    return rl_scan(m0, m1, s.npts, s.lon.data(), s.lat.data(), s.mask.data(), lon, lat);
  }
  if (surv.size() == 1) return surv[0];
  g_several++;
  return rl_finish((int)surv.size(), surv.data(), s.lon.data(), s.lat.data(), lon, lat);
}

template <typename T> static bool rd(std::vector<T> &v, size_t n, FILE *f) { v.resize(n); return fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  int hdr[6];
  if (!f || fread(hdr, sizeof(int), 6, f) != 6) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  Src s;
  s.nface = hdr[1]; s.npts = hdr[2];
  const int nd = hdr[3], iface = hdr[4];
  const size_t n = (size_t)s.nface * s.npts;
  std::vector<double> lon_dst, lat_dst;
  std::vector<int> mask_dst;
  if (!rd(s.lon, n, f) || !rd(s.lat, n, f) || !rd(s.mask, n, f) || !rd(lon_dst, nd, f) || !rd(lat_dst, nd, f) || !rd(mask_dst, nd, f)) {
    fprintf(stderr, "short input\n");
    return 2;
  }
  fclose(f);
  s.x.resize(n); s.y.resize(n); s.z.resize(n);
  s.in_range = true;
  for (size_t l = 0; l < n; l++) {
    ro_xyz(s.lon[l], s.lat[l], &s.x[l], &s.y[l], &s.z[l]);
    if (!rl_in_range(s.lon[l], s.lat[l])) s.in_range = false;
  }
  std::vector<int> idx_map(nd, -1), face_map(nd, -1), idx_sf(nd, -1);
  for (int i = 0; i < nd; i++) {
    if (mask_dst[i] == 0) continue;
    const long l = nearest(s, 0, s.nface, lon_dst[i], lat_dst[i]);
    if (l < 0) { fprintf(stderr, "no nearest point is found\n"); return 3; }
    idx_map[i] = (int)(l % s.npts); face_map[i] = (int)(l / s.npts);
  }
  for (int i = 0; i < nd && iface >= 0 && iface < s.nface; i++) {
    if (mask_dst[i] == 0) continue;
    if (face_map[i] == iface) { idx_sf[i] = idx_map[i]; continue; }
    const long l = nearest(s, iface, iface + 1, lon_dst[i], lat_dst[i]);
    if (l < 0) { fprintf(stderr, "no nearest point is found\n"); return 3; }
    idx_sf[i] = (int)(l % s.npts);
  }
  f = fopen(argv[2], "wb");
  if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  fwrite(idx_map.data(), sizeof(int), nd, f); fwrite(face_map.data(), sizeof(int), nd, f); fwrite(idx_sf.data(), sizeof(int), nd, f);
  const long counts[2] = {g_fallback, g_several};
  fwrite(counts, sizeof(long), 2, f);
  fclose(f);
  return 0;
}
