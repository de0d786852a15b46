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

// the field loop (fg_bilin_sweep): one chunk of levels in the file's type
#define BL_CHUNK 8                      // levels per launch, the unroll of k_bl_stream_*
struct BlConv { double scale, offset, missing; };   // a variable's scale_factor / add_offset (0 = absent) and missing value
struct BlStream {                       // what a chunk's gather reads beside the levels: device pointers of the plan
  long npts, ncells;
  int nl;                               // levels in this chunk, 1..BL_CHUNK
  const int *elem, *cell;               // [npts][4]: halo'd element and unpadded cell (-1: a halo corner) of the four corners
  const double *weight;                 // [npts][4]
  const double *vlon_in, *vlat_in;      // [6][N+2][N+2][3] (vector only, like vlon_out / vlat_out [npts][3])
  const double *vlon_out, *vlat_out;
  int has_missing, fill_missing;
};

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
// in_type / out_type: FG_NC_SHORT, FG_NC_INT, FG_NC_FLOAT or FG_NC_DOUBLE (the caller has checked them)
void fgd_bl_stream_scalar(int in_type, int out_type, const BlStream &a, const void *src, BlConv cin, BlConv cout, void *out,
                          hipStream_t st);
void fgd_bl_stream_vector(int in_type, int out_type, const BlStream &a, const void *u, const void *v, BlConv cu, BlConv cv,
                          BlConv cu_out, BlConv cv_out, void *u_out, void *v_out, hipStream_t st);
void fgd_bl_redu2x_typed(int out_type, const double *fin, int nxf, int nyf, int nz, const double *cosp, const double *acosp,
                         int has_missing, double missvalue, double *tmp, BlConv cout, void *crs, hipStream_t st);
