// coupler.h -- what coupler_kernels.hip (device) and coupler.hip (host orchestration) share of make_coupler_mosaic's exchange grids
// (tools/make_coupler_mosaic/make_coupler_mosaic.c:1198-2127, :2466-2811, :2976-3535, :3591-3661; design: DESIGN.md 3.13).
// min is the reference's macro (mosaic_util.h:35), operand order included.  Nothing here is contracted.
#pragma once
#include <hip/hip_runtime.h>

#define CP_MIN_AREA_FRAC 1.0e-4          /* make_coupler_mosaic.c:148 */
#define CP_TOLERANCE     1.0e-4          /* TOLORENCE, :149: |omask - ocn_frac| beyond it counts as bad */
#define CP_MIN(a, b) ((a) < (b) ? (a) : (b))

#define CP_ERR_MAXV   1u                 /* a remembered polygon has more than 8 vertices */
#define CP_ERR_NVERT  2u                 /* :1465: land on the atmosphere grid, but fix_lon left the two copies with different counts */

// one exchange-cell list in device memory: c1 / c2 = the cells of the two grids (atmosphere: over all tiles; land: in its tile);
// clon / clat the weighted centroid integrals; d = tile1 then tile2 distances (order 2)
struct CpList {
  long n = 0, cap = 0;
  int *c1 = nullptr, *c2 = nullptr;
  double *area = nullptr, *clon = nullptr, *clat = nullptr;
  double *d[4] = {nullptr, nullptr, nullptr, nullptr};
};
// per-cell sums of one grid (or one tile of it)
struct CpSums { double *area, *clon, *clat; };
// what k_a_sums walks for one atmosphere cell: the atmosphere cells of a list, sorted ascending
struct CpListRef { const int *c1; const double *area, *clon, *clat; long n; };
#define CP_MAX_LISTS 64                  /* land tiles of its own a handle takes */
struct CpListRefs { CpListRef l[CP_MAX_LISTS + 1]; int count; };

// exclusive scan of n ints (flags or counts): offs [n], *total (device)
void fgd_cp_scan(long n, const int *in, int *offs, int *bsum, int *total, hipStream_t st);
long fgd_cp_scan_blocks(long n);         /* ints of bsum scratch a scan of n needs */

// land on the atmosphere grid (:1463-1477): flags of the cells of one tile that enter the list, then the list itself
void fgd_cp_same_flag(int nx, int ny, const double *lon, const double *lat, const double *area, double thresh, int *flag, unsigned *err,
                      hipStream_t st);
void fgd_cp_same_emit(int nx, int ny, const double *lon, const double *lat, const double *area, const int *flag, const int *offs, int cell_off,
                      int *pa, int *pl, int *pn, double *plon, double *plat, double *lon_avg, double *area_ref, unsigned *err, hipStream_t st);
// land of its own (:1483-1548): flags of the plan's exchange cells that pass the coupler's own ratio test, then the list
void fgd_cp_cand_flag(long n, const int *x_src, const int *x_dst, const double *x_area, const double *area_atm, const double *area_lnd,
                      double thresh, int *flag, hipStream_t st);
void fgd_cp_cand_emit(long n, const int *x_src, const int *x_dst, const int *flag, const int *offs, const int *n_in, const double *lon_in,
                      const double *lat_in, const double *src_lon_avg, const double *area_atm, const double *area_lnd, int *pa, int *pl, int *pn,
                      double *plon, double *plat, double *lon_avg, double *area_ref, unsigned *err, hipStream_t st);
// great-circle handle (GREAT_CIRCLE_CLIP).  The cells of a tile as [cell][4][3] clockwise unit vectors and four [cell] = 4 (what
// fgd_gc_area_batch takes); land on the atmosphere grid: the :1507 test on those areas, flag and ref [cell] = min(area_lnd, area_atm)
// of a remembered cell, +inf of any other; land of its own: the survivors of the plan's list with x / y / z [n][8]
void fgd_cp_cells_xyz(int nx, int ny, const double *x, const double *y, const double *z, double *cells, int *four, hipStream_t st);
void fgd_cp_same_gc_flag(long n, const double *xarea, const double *area, double thresh, int *flag, double *ref, hipStream_t st);
void fgd_cp_cand_emit_gc(long n, const int *x_src, const int *x_dst, const int *flag, const int *offs, const int *n_in, const double *x_in,
                         const double *y_in, const double *z_in, const double *area_atm, const double *area_lnd, int *pa, int *pl, int *pn,
                         double *px, double *py, double *pz, double *area_ref, unsigned *err, hipStream_t st);
// :1604-1661 and :2660-2686 on a plan's list: weight by the ocean fraction, the two tests, the survivors in order
void fgd_cp_ocean_flag(long n, const int *x_src, const int *x_dst, const double *x_area, const double *omask, const double *area_ocn,
                       const double *area_src, double thresh, int *flag, hipStream_t st);
void fgd_cp_ocean_emit(long n, const int *x_src, const int *x_dst, const double *x_area, const double *x_c1, const double *x_c2,
                       const double *omask, const int *flag, const int *offs, CpList out, hipStream_t st);
// :1662-1719: per remembered polygon the ocean cells over land in order, the final area test (flag), the sums
void fgd_cp_poly_sums(int npoly, long nx, const int *x_src, const int *x_dst, const double *x_area, const double *x_c1, const double *x_c2,
                      const double *omask, const double *area_ref, double thresh, double *sum_area, double *sum_clon, double *sum_clat, int *flag,
                      hipStream_t st);
void fgd_cp_poly_emit(int npoly, const int *pa, const int *pl, const double *sum_area, const double *sum_clon, const double *sum_clat,
                      const int *flag, const int *offs, CpList out, hipStream_t st);
// :1881-1951 per atmosphere cell: the land lists, then the ocean list, each in list order; the centroid where the area is > 0
void fgd_cp_a_sums(int ncells, CpListRefs refs, int order, CpSums a, hipStream_t st);
// :1783, :1809, :1887-1889, :1932-1934, :2751-2757: the terms of a list added onto the cells of its second (which = 2) or first
// (which = 1) grid in list order; rows by counting, filling and sorting (no floating-point atomics)
void fgd_cp_row_count(long n, const int *key, int *cnt, hipStream_t st);
void fgd_cp_row_fill(long n, const int *key, const int *rowptr, int *fill, int *perm, hipStream_t st);
void fgd_cp_row_sums(int ncells, const int *rowptr, const int *cnt, int *perm, const double *area, const double *clon, const double *clat, int order,
                     CpSums s, hipStream_t st);
void fgd_cp_centroid(int ncells, CpSums s, hipStream_t st);
// :1955-2007, :2776-2800: clon / area - centroid of the cell, for the two grids of a list
void fgd_cp_distances(CpList l, CpSums s1, CpSums s2, hipStream_t st);
// :2035-2046 and :2087-2094: fraction = exchange area / model area; nbad counts the ocean cells from row j0 on whose omask differs
void fgd_cp_fraction(int ncells, const double *xarea, const double *area, const double *omask, int first_cell, double *frac, int *nbad,
                     hipStream_t st);
// first index of every tile's cells in a list sorted by c1: starts [ntiles + 1]
void fgd_cp_tile_starts(int ntiles, const int *cell_off, long n, const int *c1, int *starts, hipStream_t st);
// (i, j) of the cells [k0, k0 + n) of a list; off1 / nx1: cell offset and row length of the first grid's tile (off 0 for land and ocean)
void fgd_cp_indices(long n, const int *c1, const int *c2, int off1, int nx1, int nx2, int *i1, int *j1, int *i2, int *j2, hipStream_t st);
// wave x ocean (:3107-3117): the ocean corner rows [0, ny] that have a corner strictly inside (lo, hi): band [0] = the lowest, [1] = the
// highest such row (band preset to {ny, -1}); then the flags of a plan's pairs whose ocean row lies outside [js, je] are cleared
void fgd_cp_row_band(int nx, int ny, const double *lat, double lo, double hi, int *band, hipStream_t st);
void fgd_cp_band_mask(long n, const int *x_dst, int nx, int js, int je, int *flag, hipStream_t st);
// --check (:3612-3626): the largest |xarea - area| / area over the cells, the first cell among equals; best [0] = the ratio,
// cell [0] = the cell (-1: no cell had a ratio above -1).  scratch: fgd_cp_check_blocks(n) doubles and ints
long fgd_cp_check_blocks(long n);
void fgd_cp_check_ratio(long n, const double *xarea, const double *area, double *sc_ratio, int *sc_cell, double *best, int *cell, hipStream_t st);
