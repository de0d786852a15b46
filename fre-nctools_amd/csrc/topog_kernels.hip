// topog_kernels.hip -- make_topog's realistic topography on gfx950 (tools/make_topog/topog.c; arithmetic: topog.h):
//   k_tp_scale, k_tp_expand   the destination corners in radians (:431-434); the source's 2-D corner arrays from its two axes (:456-460)
//   k_tp_prepare              the field widened from its file type, masked and scaled in one pass (:482, :492-502)
//   k_tp_ongrid               the copy of the on_grid branch (:505-510)
//   k_tp_rmask, k_tp_filter   filter_topo (:719-748): one launch per pass, the caller swaps the buffers
//   k_tp_kmt                  kmt and ht on the haloed arrays (:582-619); k_tp_halo_y, k_tp_halo_x: the boundary condition (:623-645)
//   k_tp_isolated             one anti-diagonal t = 2j + i of remove_isolated_cells' in-place sweep (:851-862)
//                             (the literal route; the other one evaluates every cell at once inside k_tp_finish)
//   k_tp_finish               the copy back (:652-655), restrict_partial_cells, enforce_min_depth and num_levels = kmt + 1 (:666)
//   k_tp_max_partial, _final  the deepest non-zero depth (show_deepest :960-962), two stages
// All of it is bound by memory or by launch latency: one lane per cell, coalesced along i.
#include "topog.h"

static inline int tp_nblk(long n, int t) { return (int)((n + t - 1) / t); }

__global__ __launch_bounds__(256) void k_tp_scale(long n, const double *x_deg, const double *y_deg, double *x_r, double *y_r)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  x_r[c] = x_deg[c] * TP_D2R;
  y_r[c] = y_deg[c] * TP_D2R;
}

__global__ __launch_bounds__(256) void k_tp_expand(int nxp, int nyp, const double *xc, const double *yc, double *x2, double *y2)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (long)nxp * nyp) return;
  const int j = (int)(c / nxp), i = (int)(c - (long)j * nxp);
  x2[c] = xc[i];
  y2[c] = yc[j];
}

__global__ __launch_bounds__(256) void k_tp_prepare(long n, const void *raw, int dtype, double missing, double scale, double *depth_src, double *mask_src)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double d = dtype == TP_NC_FLOAT ? (double)((const float *)raw)[c] : dtype == TP_NC_INT ? (double)((const int *)raw)[c] : ((const double *)raw)[c];
  double m;
  d = tp_prepare_cell(d, missing, scale, &m);
  depth_src[c] = d;
  mask_src[c] = m;
}

/* the second test against `missing` is made on the scaled values, as written there */
__global__ __launch_bounds__(256) void k_tp_ongrid(long n, const double *depth_src, double missing, double *depth)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double d = depth_src[c];
  depth[c] = d == missing ? 0.0 : d;
}

__global__ __launch_bounds__(256) void k_tp_rmask(long n, const double *depth, double *rmask)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  rmask[c] = depth[c] == 0.0 ? 0.0 : 1.0;
}

/* one pass; the outermost rows and columns are copied */
__global__ __launch_bounds__(256) void k_tp_filter(int nx, int ny, const double *in, const double *rmask, int allow_deepening, double *out)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (long)nx * ny) return;
  const int j = (int)(c / nx), i = (int)(c - (long)j * nx);
  if (i < 1 || i >= nx - 1 || j < 1 || j >= ny - 1) { out[c] = in[c]; return; }
  out[c] = tp_filter_cell(nx, in, rmask, i, j, allow_deepening);
}

__global__ __launch_bounds__(256) void k_tp_zero_row(int nx, double *depth)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nx) depth[i] = 0.0;
}

/* ht, kmt: (ni+2) x (nj+2), the caller has set them to 0 and -1; this writes the interior */
__global__ __launch_bounds__(256) void k_tp_kmt(int ni, int nj, int nk, const double *zw, const double *depth, double min_thickness, int full_cell,
                                                 int flat_bottom, double *ht, int *kmt)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (long)ni * nj) return;
  const int j = (int)(c / ni), i = (int)(c - (long)j * ni);
  double h = depth[c];
  const int k = tp_kmt_cell(&h, zw, nk, min_thickness, full_cell, flat_bottom);
  const long q = (long)(j + 1) * (ni + 2) + i + 1;
  ht[q] = h;
  kmt[q] = k;
}

/* :623-636, i = 1 .. ni.  tripolar: the fold of the last row into the north halo; else (1 here = cyclic_y) both halo rows. */
__global__ __launch_bounds__(256) void k_tp_halo_y(int ni, int nj, int tripolar, double *ht, int *kmt)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
  if (i > ni) return;
  tp_halo_y_cell(ni, nj, tripolar, ht, kmt, i);
}

/* :638-645, j = 0 .. nj+1: after the rows above, so the halo rows are wrapped too */
__global__ __launch_bounds__(256) void k_tp_halo_x(int ni, int nj, double *ht, int *kmt)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > nj + 1) return;
  tp_halo_x_cell(ni, ht, kmt, j);
}

/* The cells with 2j + i = t, j = jlo .. jhi.  Cell (i, j) reads (i-1, j) [t-1] and row j-1 at i-1, i, i+1 [t-3, t-2, t-1], all
 * from earlier launches, and (i+1, j) [t+1] and row j+1 [t+1 .. t+3], which later launches write: the values of the sequential
 * sweep.  Two cells of one launch are (i, j) and (i-2, j+1): neither is among the other's eight neighbours.  The halo is never
 * written. */
__global__ __launch_bounds__(256) void k_tp_isolated(int ni, int t, int jlo, int jhi, int dont_change_landmask, double *ht, int *kmt, TpCounts *cnt)
{
  const int j = jlo + blockIdx.x * blockDim.x + threadIdx.x;
  int changed = 0;
  if (j <= jhi) changed = tp_isolated_cell(ni, ht, kmt, t - 2 * j, j, dont_change_landmask);
  const unsigned long long b = __ballot(changed);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&cnt->isolated, (unsigned)__popcll(b));
}

/* fused_nj_max > 0: remove_isolated_cells for the rows 1 .. fused_nj_max is evaluated here, every cell on the arrays as process_topo
 * left them, instead of by the sweep before this kernel.  The sweep's result does not depend on its order (a reset
 * leaves the minimum of each of the four 2 x 2 blocks round the cell as it was), so this is the sequential sweep's result too. */
__global__ __launch_bounds__(256) void k_tp_finish(int ni, int nj, int nk, const double *zw, const double *p_cell_min, const double *ht, const int *kmt,
                                                    int fused_nj_max, int dont_change_landmask, int adjust_topo, int open_very_this_cell, int kmt_min, int round_shallow, int deepen_shallow,
                                                    int fill_shallow, double *depth, int *num_levels, TpCounts *cnt)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int partial = 0, shallow = 0, isolated = 0;
  if (c < (long)ni * nj) {
    const int j = (int)(c / ni), i = (int)(c - (long)j * ni);
    const long q = (long)(j + 1) * (ni + 2) + i + 1;
    double h = ht[q];
    int k = kmt[q];
    if (j < fused_nj_max) isolated = tp_isolated_eval(ni, ht, kmt, i + 1, j + 1, dont_change_landmask, &k, &h);
    if (adjust_topo) {
      partial = tp_restrict_cell(&h, &k, zw, p_cell_min, open_very_this_cell);
      shallow = tp_enforce_cell(&h, &k, zw, kmt_min, round_shallow, deepen_shallow, fill_shallow);
    }
    depth[c] = h;
    num_levels[c] = k + 1;
  }
  const unsigned long long bp = __ballot(partial), bs = __ballot(shallow), bi = __ballot(isolated);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&cnt->isolated, (unsigned)__popcll(bi));
    if (bp) atomicAdd(&cnt->partial, (unsigned)__popcll(bp));
    if (bs) atomicAdd(&cnt->shallow, (unsigned)__popcll(bs));
  }
}

/* deepest = 0; if (ht != 0) deepest = max(ht, deepest): the result does not depend on the order */
__global__ __launch_bounds__(256) void k_tp_max_partial(long n, const double *v, double *partial)
{
  __shared__ double sh[256];
  double s = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const double h = v[i];
    if (h != 0) s = TP_MAX(h, s);
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if (threadIdx.x < w) sh[threadIdx.x] = TP_MAX(sh[threadIdx.x + w], sh[threadIdx.x]); __syncthreads(); }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(256) void k_tp_max_final(const double *partial, int np, double *result)
{
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < np; i += 256) s = TP_MAX(partial[i], s);
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if (threadIdx.x < w) sh[threadIdx.x] = TP_MAX(sh[threadIdx.x + w], sh[threadIdx.x]); __syncthreads(); }
  if (threadIdx.x == 0) *result = sh[0];
}

void fgd_tp_scale(long n, const double *x_deg, const double *y_deg, double *x_r, double *y_r, hipStream_t st)
{
  if (n > 0) k_tp_scale<<<tp_nblk(n, 256), 256, 0, st>>>(n, x_deg, y_deg, x_r, y_r);
}
void fgd_tp_expand(int nxp, int nyp, const double *xc, const double *yc, double *x2, double *y2, hipStream_t st)
{
  const long n = (long)nxp * nyp;
  if (n > 0) k_tp_expand<<<tp_nblk(n, 256), 256, 0, st>>>(nxp, nyp, xc, yc, x2, y2);
}
void fgd_tp_prepare(long n, const void *raw, int dtype, double missing, double scale, double *depth_src, double *mask_src, hipStream_t st)
{
  if (n > 0) k_tp_prepare<<<tp_nblk(n, 256), 256, 0, st>>>(n, raw, dtype, missing, scale, depth_src, mask_src);
}
void fgd_tp_ongrid(long n, const double *depth_src, double missing, double *depth, hipStream_t st)
{
  if (n > 0) k_tp_ongrid<<<tp_nblk(n, 256), 256, 0, st>>>(n, depth_src, missing, depth);
}
void fgd_tp_rmask(long n, const double *depth, double *rmask, hipStream_t st)
{
  if (n > 0) k_tp_rmask<<<tp_nblk(n, 256), 256, 0, st>>>(n, depth, rmask);
}
void fgd_tp_filter(int nx, int ny, const double *in, const double *rmask, int allow_deepening, double *out, hipStream_t st)
{
  const long n = (long)nx * ny;
  if (n > 0) k_tp_filter<<<tp_nblk(n, 256), 256, 0, st>>>(nx, ny, in, rmask, allow_deepening, out);
}
void fgd_tp_zero_row(int nx, double *depth, hipStream_t st)
{
  if (nx > 0) k_tp_zero_row<<<tp_nblk(nx, 256), 256, 0, st>>>(nx, depth);
}
void fgd_tp_kmt(int ni, int nj, int nk, const double *zw, const double *depth, double min_thickness, int full_cell, int flat_bottom,
                double *ht, int *kmt, hipStream_t st)
{
  const long n = (long)ni * nj;
  if (n > 0) k_tp_kmt<<<tp_nblk(n, 256), 256, 0, st>>>(ni, nj, nk, zw, depth, min_thickness, full_cell, flat_bottom, ht, kmt);
}
void fgd_tp_halo_y(int ni, int nj, int tripolar, double *ht, int *kmt, hipStream_t st)
{
  k_tp_halo_y<<<tp_nblk(ni, 256), 256, 0, st>>>(ni, nj, tripolar, ht, kmt);
}
void fgd_tp_halo_x(int ni, int nj, double *ht, int *kmt, hipStream_t st)
{
  k_tp_halo_x<<<tp_nblk(nj + 2, 256), 256, 0, st>>>(ni, nj, ht, kmt);
}
int fgd_tp_isolated(int ni, int nj_max, int dont_change_landmask, double *ht, int *kmt, TpCounts *cnt, hipStream_t st)
{
  int launches = 0;
  for (int t = 3; t <= 2 * nj_max + ni; t++) {
    int jlo, jhi;
    if (!tp_diagonal(ni, nj_max, t, &jlo, &jhi)) continue;
    k_tp_isolated<<<tp_nblk(jhi - jlo + 1, 256), 256, 0, st>>>(ni, t, jlo, jhi, dont_change_landmask, ht, kmt, cnt);
    launches++;
  }
  return launches;
}
void fgd_tp_finish(int ni, int nj, int nk, const double *zw, const double *p_cell_min, const double *ht, const int *kmt, int fused_nj_max,
                   int dont_change_landmask, int adjust_topo, int open_very_this_cell, int kmt_min, int round_shallow, int deepen_shallow, int fill_shallow, double *depth, int *num_levels,
                   TpCounts *cnt, hipStream_t st)
{
  const long n = (long)ni * nj;
  if (n > 0) k_tp_finish<<<tp_nblk(n, 256), 256, 0, st>>>(ni, nj, nk, zw, p_cell_min, ht, kmt, fused_nj_max, dont_change_landmask, adjust_topo, open_very_this_cell,
                                                          kmt_min, round_shallow, deepen_shallow, fill_shallow, depth, num_levels, cnt);
}
void fgd_tp_deepest(long n, const double *depth, double *partial, double *result, hipStream_t st)
{
  k_tp_max_partial<<<TP_REDUCE_BLOCKS, 256, 0, st>>>(n, depth, partial);
  k_tp_max_final<<<1, 256, 0, st>>>(partial, TP_REDUCE_BLOCKS, result);
}
