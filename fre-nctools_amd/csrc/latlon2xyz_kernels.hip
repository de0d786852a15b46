// latlon2xyz_kernels.hip -- latlon2xyz (mosaic_util.c:212-222) on the device: corner longitudes / latitudes -> unit vectors with
// the bits of the host libm the reference calls (sincos_glibc.h), so a great-circle plan can start from lon / lat arrays that
// live on the device.
//
// One lane per vertex; one launch converts every source tile and the destination grid (descriptors as a kernel argument).
// Per vertex: one fgs_trig of the latitude (sin and cos), one fused wide sin/cos of the longitude, two multiplies; 16 bytes in,
// three coalesced 8-byte stores out (SoA x | y | z).  A few hundred FP64 operations per 40 bytes: arithmetic-bound, so the
// block is 256 lanes -- one wave per SIMD of a CU, nothing shared between lanes, and more waves per block would only coarsen
// the tail of the last grid.  42 VGPRs, no scratch.
// The 3.5 KB table of the trig is read from global memory, where it stays L1/L2-hot.  A copy in LDS per block, as the clip
// kernels have it, makes no difference here -- with the copy 85.4 and 90.9 us in two sessions against 85.7 and 87.2 us without
// for the 7.7 M corners of C768 -> 0.125 deg, 18.7 and 18.7 against 18.7 and 19.1 us for C384 -> 0.25 deg, the two builds
// alternating launch by launch (profiles/gc_lonlat_summary.md): two lookups per vertex under ~250 FP64 operations, against five
// to seven per clipped edge there -- so the kernel does without it.
// -DFG_LL2X_TAB_LDS=1 builds the LDS variant (scripts/exp_build.sh, scripts/gc_lonlat_time.py --ab-lib).
#include "xgrid_device.h"
#ifndef FG_LL2X_TAB_LDS
#define FG_LL2X_TAB_LDS 0
#endif
#if FG_LL2X_TAB_LDS
static __shared__ double fgs_lds_tab[112 * 4];
#define FGS_TAB(k, j) fgs_lds_tab[(k) * 4 + (j)]
#endif
#include "sincos_glibc.h"

__global__ __launch_bounds__(256) void k_latlon2xyz(FgLl2xSet gs, unsigned *err)
{
#if FG_LL2X_TAB_LDS
  for (int i = threadIdx.x; i < 112 * 4; i += 256) fgs_lds_tab[i] = FG_SINCOS_TAB[i >> 2][i & 3];
  __syncthreads();
#endif
  // the grid of this vertex: constant indices into the argument (scalar loads, selects), not an indexed copy of it
  long v = (long)blockIdx.x * 256 + threadIdx.x;
  FgLl2xGrid g = gs.g[0];
#pragma unroll
  for (int m = 1; m < FG_TILESET_MAX; m++)
    if (m < gs.n && v >= g.n) { v -= g.n; g = gs.g[m]; }
  if (v >= g.n) return;                      // past the last grid
  double x, y, z;
  if (!fgs_latlon2xyz_vertex(g.lon[v], g.lat[v], &x, &y, &z) && err) atomicOr(err, G_ERRBIT_LL2X);
  g.x[v] = x; g.y[v] = y; g.z[v] = z;
}

void fgd_latlon2xyz(const FgLl2xGrid *grids, int ngrids, unsigned *err, hipStream_t st)
{
  for (int m0 = 0; m0 < ngrids; m0 += FG_TILESET_MAX) {
    FgLl2xSet gs{};
    long total = 0;
    for (int m = m0; m < ngrids && m < m0 + FG_TILESET_MAX; m++)
      if (grids[m].n > 0) { gs.g[gs.n++] = grids[m]; total += grids[m].n; }
    if (total > 0) k_latlon2xyz<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(gs, err);
  }
}
