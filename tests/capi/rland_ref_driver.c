/* rland_ref_driver.c -- TEST HARNESS ONLY (tests/golden/make_golden_rland.py, tests/test_rland_cpu.py, scripts/rland_time.py):
 * runs the reference's full_search_nearest and search_nearest_sface (tools/remap_land/remap_land.c:2520, :2569) with its
 * great_circle_distance (tools/libfrencutils/mosaic_util.c:747) on one case and dumps what they produce.  Linked with the
 * reference's remap_land.c (compiled with -Dmain=remap_land_main and -ffunction-sections and linked with --gc-sections, so that
 * none of its netCDF-bound functions is kept) and mosaic_util.c, mpp.c, mpp_domain.c, in a temporary directory outside the
 * repository.  Nothing of the reference is restated here.
 *
 *   rland_ref_driver IN OUTDIR
 *   IN: int mode, nface_src, npts_src, npts_dst, iface_dst, 0; then double lon_src[nface*npts], lat_src[..]; int mask_src[..];
 *       double lon_dst[npts_dst], lat_dst[..]; int mask_dst[..]
 *   mode 0 -> OUTDIR/idx_map.bin, face_map.bin, idx_map_sf.bin int [npts_dst]: the all-faces search, then the same-face search
 *             for face iface_dst with mask_src
 *   mode 1 -> the all-faces search alone: idx_map.bin, face_map.bin, seconds.txt
 *   mode 2 -> nface_src * npts_src must equal npts_dst: d.bin double [npts_dst], great_circle_distance(dst k, src k) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

void full_search_nearest(int nface_src, int npts_src, const double *lon_src, const double *lat_src, const int *mask_src, int npts_dst,
                         const double *lon_dst, const double *lat_dst, const int *mask_dst, int *idx_map, int *face_map);
void search_nearest_sface(const int npts_src, const double *lon_src, const double *lat_src, const int *mask_src, int npts_dst,
                          const double *lon_dst, const double *lat_dst, const int *mask_dst, const int *idx_map, const int *face_map,
                          const int iface_dst, int *idx_map_sf);
double great_circle_distance(double *p1, double *p2);

static void *rd(size_t sz, size_t n, FILE *f)
{
  void *p = malloc((n ? n : 1) * sz);
  if (!p || fread(p, sz, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return p;
}
static void dump(const char *dir, const char *name, const void *p, size_t bytes)
{
  char path[4096];
  FILE *f;
  snprintf(path, sizeof path, "%s/%s", dir, name);
  f = fopen(path, "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}

int main(int argc, char **argv)
{
  FILE *f;
  int *hdr;
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUTDIR\n", argv[0]); return 2; }
  f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  hdr = (int *)rd(sizeof(int), 6, f);
  {
    const int mode = hdr[0], nface = hdr[1], npts = hdr[2], nd = hdr[3], iface = hdr[4];
    const size_t n = (size_t)nface * npts;
    double *lon_src = (double *)rd(sizeof(double), n, f), *lat_src = (double *)rd(sizeof(double), n, f);
    int *mask_src = (int *)rd(sizeof(int), n, f);
    double *lon_dst = (double *)rd(sizeof(double), nd, f), *lat_dst = (double *)rd(sizeof(double), nd, f);
    int *mask_dst = (int *)rd(sizeof(int), nd, f);
    int *idx_map = (int *)malloc((nd ? nd : 1) * sizeof(int)), *face_map = (int *)malloc((nd ? nd : 1) * sizeof(int));
    int *idx_sf = (int *)malloc((nd ? nd : 1) * sizeof(int));
    fclose(f);
    if (mode == 2) {
      double *d = (double *)malloc((nd ? nd : 1) * sizeof(double));
      int k;
      if (n != (size_t)nd) { fprintf(stderr, "mode 2 needs as many source as destination points\n"); return 2; }
      for (k = 0; k < nd; k++) {
        double p1[2], p2[2];
        p1[0] = lon_dst[k]; p1[1] = lat_dst[k]; p2[0] = lon_src[k]; p2[1] = lat_src[k];
        d[k] = great_circle_distance(p1, p2);
      }
      dump(argv[2], "d.bin", d, nd * sizeof(double));
      return 0;
    }
    {
      struct timespec t0, t1;
      char txt[64];
      clock_gettime(CLOCK_MONOTONIC, &t0);
      full_search_nearest(nface, npts, lon_src, lat_src, mask_src, nd, lon_dst, lat_dst, mask_dst, idx_map, face_map);
      clock_gettime(CLOCK_MONOTONIC, &t1);
      snprintf(txt, sizeof txt, "%.6f\n", (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
      dump(argv[2], "seconds.txt", txt, strlen(txt));
    }
    dump(argv[2], "idx_map.bin", idx_map, nd * sizeof(int));
    dump(argv[2], "face_map.bin", face_map, nd * sizeof(int));
    if (mode == 0) {
      search_nearest_sface(npts, lon_src, lat_src, mask_src, nd, lon_dst, lat_dst, mask_dst, idx_map, face_map, iface, idx_sf);
      dump(argv[2], "idx_map_sf.bin", idx_sf, nd * sizeof(int));
    }
  }
  return 0;
}
