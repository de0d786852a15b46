// bilinear.h -- what bilinear.hip (host orchestration) and bilinear_kernels.hip (kernels) share: the device view of a plan
// and the launchers.
#pragma once
#include <hip/hip_runtime.h>

struct BlGeom {                       // device pointers of one handle
  int N;                              // cube tile size (nx == ny)
  int nxo, nyo;                       // fine lat-lon grid
  const double *xt, *yt, *zt;         // halo'd input centres, [6][N+2][N+2]
  const double *lont, *latt;
  const double *xo, *yo, *zo;         // lat-lon points [nyo][nxo]
  const double *cell_dist;            // normalize_great_circle_distance of each cell's (jc, ic) -> (jc+1, ic+1) centres [6*N*N]
};
struct BlWin { int i0, i1, j0, j1; };   // 0-based inclusive ranges of the window loops (bilinear_interp.c:170)

void fgd_bl_search_iter(const BlGeom &g, int iter, double dlon, double dlat, double lonbegin, double latbegin, unsigned *unfound,
                        BlWin *win, unsigned long long *cnt, unsigned long long *off, unsigned long long *bsum,
                        unsigned long long *total, int *found, unsigned long long *key, int *index, unsigned *ties,
                        int pair_blocks, hipStream_t st);
long fgd_bl_scan_blocks(long ncell);
void fgd_bl_weight_sides(const BlGeom &g, const int *index, double *angle, double *acos_arg, double *side_cos, hipStream_t st);
void fgd_bl_weight_final(long npts, int N, const int *index, const double *dist, double *weight, hipStream_t st);
void fgd_bl_corners(const BlGeom &g, const int *index, const int *cell_of, int *elem, int *cell, hipStream_t st);
void fgd_bl_gather_scalar(long npts, long ncells, int nz, const int *cell, const double *weight, const double *src, int has_missing,
                          double missing, int fill_missing, double *out, hipStream_t st);
void fgd_bl_gather_vector(long npts, long ncells, int nz, const int *elem, const int *cell, const double *weight, const double *vlon_in,
                          const double *vlat_in, const double *vlon_out, const double *vlat_out, const double *u, const double *v,
                          int has_missing, double missing, int fill_missing, double *u_out, double *v_out, hipStream_t st);
void fgd_bl_redu2x(const double *fin, int nxf, int nyf, int nz, const double *cosp, const double *acosp, int has_missing,
                   double missvalue, double *tmp, double *crs, hipStream_t st);
