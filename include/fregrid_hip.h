/*
 * fregrid_hip.h -- C ABI of libfregrid_hip.so, the MI355X (gfx950) implementation of
 * FRE-NCtools' conservative-regrid hot path.  Plain C: pointers, ints and doubles only.
 *
 * Three groups of entry points:
 *
 *  (B1) drop-in replacements for libfrencutils symbols -- identical names, argument
 *       lists, ownership and fatal-error behaviour as the reference, host pointers in/out:
 *         get_maxxgrid               tools/libfrencutils/create_xgrid.c:45
 *         get_grid_area              tools/libfrencutils/create_xgrid.c:66    (create_xgrid.h:41)
 *         create_xgrid_2dx2d_order1  tools/libfrencutils/create_xgrid.c:621   (create_xgrid.h:65)
 *         create_xgrid_2dx2d_order2  tools/libfrencutils/create_xgrid.c:893   (create_xgrid.h:69)
 *         conserve_interp            tools/libfrencutils/interp.c:262         (interp.h)
 *         create_xgrid_great_circle  tools/libfrencutils/create_xgrid.c:1366  (create_xgrid.h:77)
 *         get_grid_great_circle_area create_xgrid.c:98, clip_2dx2d_great_circle :1479, great_circle_area mosaic_util.c:763,
 *         conserve_interp_great_circle interp.c:312
 *         create_xgrid_1dx2d_order1/2 create_xgrid.c:208/311, create_xgrid_2dx1d_order1/2 :414/509, clip :1159,
 *         box_ctrlat/box_ctrlon :2223/:2238, get_grid_area_no_adjust :166
 *         clip_2dx2d :1266, poly_area mosaic_util.c:474, poly_ctrlon/poly_ctrlat create_xgrid.c:2170/2096, fix_lon, pimod
 *         + trailing-underscore Fortran aliases (create_xgrid.c:60,91,196,301,396,491,608,881,1353)
 *
 *  (B2) device-resident "plan" API that replaces the pair
 *         setup_conserve_interp      tools/fregrid/conserve_interp.c:42   (compute branch :127-358)
 *         do_scalar_conserve_interp  tools/fregrid/conserve_interp.c:507
 *       so that exchange cells never leave HBM between the search and the sweep.
 *       INTEGRATION.md shows the conserve_interp_hip.c a maintainer links in place of
 *       conserve_interp.o (the same swap the reference's own fregrid_gpu makes,
 *       tools/fregrid_gpu/Makefile.am:28-41).
 *
 *  (F)  the callers either side of the path: fg_c2l_* (halo update + grad_c2l on the device,
 *       fregrid_util.c:2168-2216, gradient_c2l.c:58-118; fg_c2l_records + fg_plan_apply_records fuse them with the
 *       order-2 sweep), fg_remap_* (fregrid's remap file without libnetcdf, conserve_interp.c:368-445 / :62-126).
 *
 *  (G)  host grid generators used to synthesise inputs without make_hgrid files.
 *
 * Error handling: fg_* functions return 0 (or a count) on success and a negative
 * FG_ERR_* code on failure; fg_last_error() returns the message.  The B1 symbols
 * behave like the reference: fatal -> "FATAL Error: <msg>" on stderr and exit(1)
 * (tools/libfrencutils/mosaic_util.c:57-65).
 *
 * All longitudes/latitudes are FP64 radians, cell corners row-major [j*(nx+1)+i].
 */
#ifndef FREGRID_HIP_H_
#define FREGRID_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FG_ERR_ARG        (-1)   /* bad argument                                              */
#define FG_ERR_HIP        (-2)   /* HIP runtime failure (no device, out of memory, ...)        */
#define FG_ERR_MAXV       (-3)   /* a cell has more than MAX_V=8 vertices after fix_lon (create_xgrid.c:1007) */
#define FG_ERR_PARALLEL   (-4)   /* clip hit parallel edges, |determ| < 1e-30 (create_xgrid.c:1314) */
#define FG_ERR_CAPACITY   (-5)   /* caller's output arrays too small (reference: MAXXGRID fatal, :1087) */
#define FG_ERR_STATE      (-6)   /* call made in the wrong plan state                          */
/* FG_ERR_GEOM: the great-circle clip hit one of the reference's fatal geometry checks (create_xgrid.c:1575-1834: "grid box 1 / 2 is
 * not convex", the six fatals of the clip), or a pair the device clip cannot finish (its list capacity; a pair on which the
 * reference's insertIntersect does not end).  fg_last_error() holds the reference's text, or one that names the limit as the
 * device's.  Returned by every great-circle search: fg_plan_create_great_circle, _dev, _lonlat, _lonlat_dev,
 * fg_plan_create_polylist_gc, _dev, and fg_coupler_run of a handle made by fg_coupler_create_gc, which passes the search's code and
 * text through (and uses the code for its own two checks of the polygons).  DESIGN.md section 3.1b has the table. */
#define FG_ERR_GEOM       (-8)
#define FG_ERR_IO         (-9)   /* file I/O (fg_nc_*, fg_remap_*)                            */
#define FG_ERR_NOTFOUND   (-10)  /* attribute / variable not present                          */
#define FG_ERR_BILIN_NOTFOUND (-11) /* bilinear search: points without a lower-left corner after 10 sweeps (fg_bilin_create) */
#define FG_ERR_DATA       (-7)   /* the field data hit one of the reference's fatal checks (conserve_interp.c:584,:697,:709; interp.c:366-374) */

/* option bits, same values as tools/libfrencutils/globals.h:46-61 where they exist */
#define FG_CONSERVE_ORDER1 1
#define FG_CONSERVE_ORDER2 2

/* ---------------------------------------------------------------- (B1) ---- */
int  get_maxxgrid(void);
void get_grid_area(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area);
int  create_xgrid_2dx2d_order1(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out,
                               const double *lon_in, const double *lat_in, const double *lon_out, const double *lat_out,
                               const double *mask_in, int *i_in, int *j_in, int *i_out, int *j_out, double *xgrid_area);
int  create_xgrid_2dx2d_order2(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out,
                               const double *lon_in, const double *lat_in, const double *lon_out, const double *lat_out,
                               const double *mask_in, int *i_in, int *j_in, int *i_out, int *j_out,
                               double *xgrid_area, double *xgrid_clon, double *xgrid_clat);
void conserve_interp(int nx_src, int ny_src, int nx_dst, int ny_dst, const double *x_src,
                     const double *y_src, const double *x_dst, const double *y_dst,
                     const double *mask_src, const double *data_src, double *data_dst);
/* single-polygon primitives (create_xgrid.h:35-46, mosaic_util.h): same signatures as the reference;
 * each call is one tiny device launch -- use the *_batch forms below for volume */
int    clip_2dx2d(const double lon1_in[], const double lat1_in[], int n1_in, const double lon2_in[],
                  const double lat2_in[], int n2_in, double lon_out[], double lat_out[]);   /* create_xgrid.c:1266 */
double poly_area(const double lon[], const double lat[], int n);                             /* mosaic_util.c:474  */
double poly_ctrlon(const double lon[], const double lat[], int n, double clon);              /* create_xgrid.c:2170 */
double poly_ctrlat(const double lon[], const double lat[], int n);                           /* create_xgrid.c:2096 */
int    fix_lon(double lon[], double lat[], int n, double tlon);                              /* mosaic_util.c:667  */
void   pimod(double x[], int nn);                                                            /* create_xgrid.c:1343 */
/* Fortran aliases */
int  get_maxxgrid_(void);
void get_grid_area_(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area);
int  create_xgrid_2dx2d_order1_(const int *, const int *, const int *, const int *, const double *, const double *,
                                const double *, const double *, const double *, int *, int *, int *, int *, double *);
int  create_xgrid_2dx2d_order2_(const int *, const int *, const int *, const int *, const double *, const double *,
                                const double *, const double *, const double *, int *, int *, int *, int *,
                                double *, double *, double *);

/* ---------------------------------------------------------------- (B2) ---- */
typedef struct fg_plan fg_plan;

/* last error message of the calling thread ("" if none) */
const char *fg_last_error(void);

/* number of HIP devices visible; <0 on failure.  Does not create a context. */
int fg_device_count(void);

/*
 * Exchange-grid search between ntiles_in source tiles and ONE destination tile
 * (or the latitude band of it owned by this rank: pass the band's corner arrays,
 * exactly as the reference passes grid_out[n].lonc/latc of the compute domain,
 * conserve_interp.c:187-199).  Host corner arrays are copied to the device.
 *   order      FG_CONSERVE_ORDER1 | FG_CONSERVE_ORDER2
 *   mask_in    per-tile source masks (NULL or mask_in[m]==NULL => all ones, conserve_interp.c:160-161)
 *   device     HIP device ordinal
 * On success *plan_out owns the device-resident exchange cells in the reference's
 * canonical order (source tile, j_in, i_in, then destination cell index ascending
 * == create_xgrid_2dx2d_* with one thread, tiles concatenated as conserve_interp.c:234-316).
 * Returns nxgrid (>=0) or FG_ERR_*.
 */
long fg_plan_create(int order, int ntiles_in, const int *nx_in, const int *ny_in,
                    const double *const *lon_in, const double *const *lat_in,
                    const double *const *mask_in,
                    int nx_out, int ny_out, const double *lon_out, const double *lat_out,
                    int device, fg_plan **plan_out);
/*
 * Same search with every grid pointer already a DEVICE pointer (inputs resident in HBM; this
 * is what bench.py times).  mean_dlat/mean_dlon: typical destination cell extent in radians
 * used to size the search bins (<= 0: derived from a strided sample copied back to the host).
 * use_caller_stream != 0: all work is queued on `stream` (a hipStream_t, e.g. PyTorch's
 * current stream; NULL = the legacy default stream) instead of a private stream.
 * A plan's private stream is NON-BLOCKING: it does not wait for the legacy default stream.  Device buffers a caller hands to
 * a plan (fields, outputs it has just filled or zeroed on another stream) must be complete on that stream first -- or put the
 * plan on the caller's stream (this argument, fg_plan_set_stream).
 */
long fg_plan_create_dev(int order, int ntiles_in, const int *nx_in, const int *ny_in,
                        const double *const *d_lon_in, const double *const *d_lat_in,
                        const double *const *d_mask_in,
                        int nx_out, int ny_out, const double *d_lon_out, const double *d_lat_out,
                        double mean_dlat, double mean_dlon, int device, void *stream,
                        int use_caller_stream, fg_plan **plan_out);
/* A plan without a search; exchange cells are supplied by fg_plan_set_xgrid. */
int fg_plan_create_empty(int order, int ntiles_in, const int *nx_in, const int *ny_in,
                         int nx_out, int ny_out, int device, fg_plan **plan_out);
/* Does not synchronise the plan's stream (fg_set_search_async): work of the plan that is still queued -- an asynchronous apply
 * with the caller's buffers among it -- stays queued, on a plan-owned stream too, so a caller that frees or reuses those buffers
 * from the host calls fg_plan_sync first. */
void fg_plan_destroy(fg_plan *plan);
/* queue all further work of the plan on the caller's stream (hipStream_t) */
int fg_plan_set_stream(fg_plan *plan, void *stream);
/* return the cached device blocks of destroyed plans to the HIP runtime */
void fg_pool_release(void);
/* Device memory for plain-C callers (no HIP headers needed): blocks from the library's caching pool, synchronous copies.
 * fg_dev_alloc returns NULL on failure (fg_last_error has the reason). */
void *fg_dev_alloc(size_t bytes, int device);
void fg_dev_free(void *p);
int  fg_dev_upload(void *dst_dev, const void *src_host, size_t bytes);
int  fg_dev_download(void *dst_host, const void *src_dev, size_t bytes);
/* dst_dev[i] = src_dev[idx_dev[i]]  /  dst_dev[idx_dev[i]] = src_dev[i]  for i < n (all pointers device memory of the current device) */
int  fg_dev_gather_f64(double *dst_dev, const double *src_dev, const int *idx_dev, long n);
int  fg_dev_scatter_f64(double *dst_dev, const double *src_dev, const int *idx_dev, long n);

/* Give back the surplus of the capacity-sized exchange-cell arrays (8*max(nsrc, ndst) entries -> nxgrid entries; device-to-device
 * copies).  For callers that keep many plans resident.  Any state after the search. */
int  fg_plan_trim(fg_plan *plan);
long fg_plan_nxgrid(const fg_plan *plan);
long fg_plan_ncells_in(const fg_plan *plan);      /* sum over source tiles of nx*ny */
long fg_plan_ncells_out(const fg_plan *plan);     /* nx_out*ny_out */
int  fg_plan_order(const fg_plan *plan);
int  fg_plan_device(const fg_plan *plan);

/*
 * Order 2 only.  Device pointer to the per-source-cell partial sums
 * [3][ncells_in] = {sum xarea, sum clon, sum clat} over this plan's exchange cells
 * (conserve_interp.c:216-221).  With several destination tiles or several ranks the
 * caller adds these arrays up (one RCCL all-reduce over xGMI) and hands the total
 * to fg_plan_finalize.
 */
double *fg_plan_cell_sums_dev(fg_plan *plan);
/* copy those sums into a caller-owned DEVICE buffer of 3*ncells_in doubles (e.g. a torch tensor) */
int fg_plan_copy_cell_sums(fg_plan *plan, double *dst_dev);
/* total_dev[3][ncells_in] += this plan's exchange cells, added one by one in exchange-cell order onto the values already there
 * (conserve_interp.c:203-221 adds the exchange cells of all output tiles and all ranks in that order "for the purpose of
 * bitwise reproducing"): hand one running total from plan to plan, and from rank to rank for the source cells that have
 * exchange cells on more than one rank.  cells_dev (device, may be NULL = every source cell) restricts the update to a list
 * of source cells.  Order-2 plans, after the search and before fg_plan_finalize. */
int fg_plan_accumulate_cell_sums(fg_plan *plan, double *total_dev, const int *cells_dev, int ncells);
/* The same, queued on the plan's stream without waiting for it: for a caller whose other device work is ordered on that very
 * stream (fg_plan_set_stream, or the stream handed to fg_plan_create_dev).  total_dev / cells_dev must stay valid until the
 * stream has passed the kernel. */
int fg_plan_accumulate_cell_sums_async(fg_plan *plan, double *total_dev, const int *cells_dev, int ncells);

/*
 * Turn (clon, clat) into distances from the source-cell centroid
 * (conserve_interp.c:256-257,319-358) and build the destination-row (CSR) layout
 * used by the sweep.  total_cell_sums_dev: device pointer [3][ncells_in] with the
 * sums over ALL destination tiles/ranks, or NULL to use this plan's own sums.
 * Order 1 plans only build the CSR layout.
 */
int fg_plan_finalize(fg_plan *plan, const double *total_cell_sums_dev);

/*
 * Copy the exchange cells to host arrays of length fg_plan_nxgrid().  Any pointer
 * may be NULL.  Before fg_plan_finalize: c1/c2 receive the un-normalised xgrid_clon/
 * xgrid_clat of create_xgrid_2dx2d_order2; after it: di_in/dj_in of Interp_config
 * (globals.h:144-158).
 */
int fg_plan_get_xgrid(const fg_plan *plan, int *t_in, int *i_in, int *j_in, int *i_out, int *j_out,
                      double *area, double *c1, double *c2);

/* per-cell records (get_grid_cell_struct semantics, create_xgrid.c:991-1016) of the source
 * cells (which = 0, tiles concatenated) or destination cells (which = 1).  Host arrays, any
 * may be NULL; vlon/vlat are [ncells][8] (vertices after fix_lon, unused slots 0). */
int fg_plan_get_cell_struct(const fg_plan *plan, int which, double *lat_min, double *lat_max, double *lon_min,
                            double *lon_max, double *lon_avg, int *nvert, double *vlon, double *vlat);

/* The clipped polygon of every exchange cell of a searched plan, in canonical order: n_out[nxgrid] vertex counts and
 * [nxgrid][maxv] vertex arrays (host).  Legacy plans: v0 = longitudes, v1 = latitudes as clip_2dx2d returned them for the pair
 * inside create_xgrid (source cell after fix_lon(pi); destination cell after fix_lon(pi) and the +-2pi shift of
 * create_xgrid.c:1062-1079); v2 unused.  Great-circle plans: v0, v1, v2 = x, y, z as clip_2dx2d_great_circle returned them.
 * make_coupler_mosaic keeps these vertices of its atmosphere x land cells to clip them against the ocean grid
 * (make_coupler_mosaic.c:1560-1577, 1659-1692); see coupler.py. */
int fg_plan_get_polygons(const fg_plan *plan, int maxv, int *n_out, double *v0, double *v1, double *v2);
/* A legacy search whose SOURCE cells are a list of polygons of at most 8 vertices: n[npoly], lon / lat [npoly][8] (host) in the
 * longitude frame of each polygon's parent cell; lon_avg[npoly] = the parent's mean longitude (it decides the +-2pi shift of a
 * destination cell, create_xgrid.c:1062-1079, and is poly_ctrlon's reference); area_ref[npoly] = the area the 1e-6 ratio test
 * uses for the polygon.  Everything downstream is the ordinary plan (exchange cells with i_in = polygon index, j_in = t_in = 0,
 * fg_plan_get_xgrid / _polygons / accumulate / finalize / apply).  make_coupler_mosaic.c:1659-1692 clips its remembered
 * atmosphere x land polygons against the ocean grid this way; fre-nctools_amd/coupler.py is that loop over two plans and this. */
long fg_plan_create_polylist(int order, int npoly, const int *n, const double *lon, const double *lat, const double *lon_avg,
                             const double *area_ref, int nx_out, int ny_out, const double *lon_out, const double *lat_out,
                             int device, fg_plan **plan_out);
/* The great-circle twin: the SOURCE cells are convex polygons of 3..8 vertices given as unit vectors, clockwise as
 * clip_2dx2d_great_circle returns them -- n[npoly], x / y / z [npoly][8] (host); area_ref[npoly] = the area the 1e-6 ratio test
 * uses for the polygon (great_circle_area(clip) / min(area_ref, destination cell area) > 1e-6).  lon_out / lat_out: the
 * destination corners in radians; destination areas are get_grid_great_circle_area's.  Every (polygon, candidate cell) pair is
 * clipped by clip_2dx2d_great_circle (create_xgrid.c:1479-1908) with the polygon first; exchange cells come polygon by polygon,
 * destination cells ascending (i_in = polygon index, j_in = t_in = 0).  First order only.  A polygon with n < 3 takes no part;
 * n > 8 is FG_ERR_ARG; npoly = 0 gives a plan of one empty polygon and no exchange cell.  The plan is a great-circle plan:
 * fg_plan_get_xgrid / _polygons (x, y, z) / finalize / apply work on it.  make_coupler_mosaic.c:1662-1696 clips its remembered
 * atmosphere x land polygons against the ocean cells this way under GREAT_CIRCLE_CLIP. */
long fg_plan_create_polylist_gc(int npoly, const int *n, const double *x, const double *y, const double *z, const double *area_ref,
                                int nx_out, int ny_out, const double *lon_out, const double *lat_out, int device, fg_plan **plan_out);
/* cell areas computed during the search (get_grid_area semantics): source cells
 * concatenated over tiles / destination cells.  Host arrays, may be NULL. */
int fg_plan_get_cell_area(const fg_plan *plan, double *area_in, double *area_out);

/*
 * Replace the plan's exchange cells by caller-provided ones (the READ branch of
 * setup_conserve_interp, conserve_interp.c:62-126, after the remap file has been
 * parsed on the host; also used by tests to sweep with the oracle's weights).
 * di_in/dj_in are final distances (order 2) or NULL (order 1).  The plan is left
 * finalized.  Returns 0 or FG_ERR_*.
 */
int fg_plan_set_xgrid(fg_plan *plan, long nxgrid, const int *t_in, const int *i_in, const int *j_in,
                      const int *i_out, const int *j_out, const double *area,
                      const double *di_in, const double *dj_in);

/*
 * The sweep: do_scalar_conserve_interp for one destination tile, plain branch
 * (no weight field / cell_measures / cell_methods=sum / monotonic / target_grid),
 * conserve_interp.c:561-616 (order 1), :743-813 (order 2), :815-839.
 * All data pointers are DEVICE pointers:
 *   data     source field [nz][F]: one level holds the tiles back to back, each tile
 *            [ny][nx] (order 1) or [ny+2][nx+2] with a 1-cell halo (order 2, the layout
 *            fregrid_util.c:2137-2145 builds per tile); F = sum over tiles of that size
 *   grad_x, grad_y   [nz][ncells_in] (tiles back to back, no halo), order 2 only
 *   grad_mask        int [ncells_in], order 2 with has_missing only (else NULL)
 *   out      [nz][ny_out][nx_out]
 *   gsum_out host pointer or NULL: sum of out*area before normalisation (:815-819)
 * has_missing requires nz == 1 (:544).  Returns 0 or FG_ERR_*.
 */
int fg_plan_apply(fg_plan *plan, const double *data, const double *grad_x, const double *grad_y,
                  const int *grad_mask, int has_missing, double missing, int nz,
                  double *out, double *gsum_out);

/* The sweep on fields the caller keeps INTERLEAVED over nb in {2,4,8} levels/fields/time steps:
 * data_il [F][nb], grad_x_il/grad_y_il [ncells_in][nb], out_il [ndst][nb] (device pointers).  Every CSR entry
 * is read once for nb levels and each gather is nb*8 contiguous bytes; this is the layout the sweep
 * kernel works in -- fg_plan_apply transposes level-major input into it.  No missing values. */
int fg_plan_apply_interleaved(fg_plan *plan, int nb, const double *data_il, const double *grad_x_il,
                              const double *grad_y_il, double *out_il, double *gsum_out);

/* The order-2 sweep of 1 <= nz <= 8 levels on the records fg_c2l_gradient_records writes (rec[ncells_in][3][nb], device):
 * the layout fg_plan_apply builds internally, so out [nz][ndst] (level-major, device) equals fg_plan_apply's bit for bit
 * while the level-major gradient arrays and the transposition pass are skipped.  gsum_out as in fg_plan_apply. */
int fg_plan_apply_records(fg_plan *plan, int nz, const double *rec, double *out, double *gsum_out);

/* Levels that each carry missing values of their own, many per call: "the level loop".  The reference takes such a field one
 * level per call (fregrid.c:1045-1083: get_input_data, do_scalar_conserve_interp(..., 1), write_field_data per level;
 * conserve_interp.c:544 forbids has_missing with nz > 1), and so do fg_plan_apply / fg_plan_apply_ex, which keep that refusal.
 * fg_plan_apply_levels is that loop on the device: for k = 0 .. nlev-1, out level k holds the bits
 * do_scalar_conserve_interp(nz = 1, has_missing = 1) -- and fg_plan_apply(has_missing = 1, nz = 1) -- give on level k alone
 * (conserve_interp.c:562-591 order 1; :744-783 order 2; :815-839): per destination cell the exchange cells whose source value
 * differs from `missing` in level k are summed in CSR order; acc / asum where asum > 0, 0.0 where an exchange cell counted but
 * asum == 0, `missing` otherwise; an exchange cell whose source cell has grad_mask set in level k uses the flat value.  Eight
 * levels share one launch (every CSR record is read once for them); any nlev >= 1, the last chunk may be partial.
 *   data       [nlev][F], grad_x / grad_y [nlev][ncells_in] as fg_plan_apply takes them (device pointers)
 *   grad_mask  int [nlev][ncells_in] as fg_c2l_gradient writes it (fregrid_util.c:2203-2215).  grad_x, grad_y and grad_mask
 *              are NULL for order 1 and required for order 2
 *   out        [nlev][ndst] (device); gsum_out: host double[nlev] or NULL, the sum of :815-819 PER LEVEL (what
 *              fg_plan_apply_ex(has_missing, nz = 1) returns for that level, bit for bit)
 * Bad arguments -- nlev < 1, NULL buffers, an order-2 plan without gradients or mask, a plan that is not finalized -- return
 * FG_ERR_ARG, write nothing and leave the plan usable.
 * Weight field, cell_measures, cell_methods = sum and --target_grid on many levels: fg_plan_apply_levels_ex below.  The
 * monotone limiter on many levels: fg_plan_apply_levels_mono and fg_plan_mono_levels_* further below.  integration/ keeps the
 * reference's per-level loop. */
int fg_plan_apply_levels(fg_plan *plan, const double *data, const double *grad_x, const double *grad_y,
                         const int *grad_mask, double missing, int nlev, double *out, double *gsum_out);
/* The same sweep of 1 <= nz <= 8 levels on the records fg_c2l_records_levels writes: rec [ncells_in][3][8] (always eight
 * levels wide, zero padded) and maskbits, unsigned char [ncells_in]: bit k set = the cell's gradient is masked in level k (its
 * exchange cells use the flat value there).  Validity is read from the records themselves (field value == missing).  Order-2
 * plans only.  out [nz][ndst], gsum_out host double[nz] or NULL; bit-identical to fg_plan_apply_levels. */
int fg_plan_apply_records_levels(fg_plan *plan, int nz, const double *rec, const unsigned char *maskbits, double missing,
                                 double *out, double *gsum_out);
/* Exchange cells the eight-level masked sweep stages per chunk: a tile of destination rows with more of them (fine -> coarse
 * remaps) is walked in several chunks, the sums carried from chunk to chunk. */
int fg_plan_levels_capacity(void);

/* The sweep with every remaining option of do_scalar_conserve_interp (conserve_interp.c:507-910).  All pointers are
 * DEVICE pointers over the flattened source cells (tiles back to back, [ny][nx], no halo) or destination cells.
 *   weight          grid_in[].weight (weight_exist, --weight_file/--weight_field), or NULL
 *   cell_methods_sum  cell_methods == CELL_METHODS_SUM: area /= cell_area; un-normalised output (:821-830)
 *   field_area      field_in[].area of a cell_measures variable (area *= field_area/cell_area), or NULL;
 *                   with has_missing a field_area equal to area_missing under valid data is the reference's fatal
 *                   "data is not missing but area is missing" -> FG_ERR_DATA
 *   cell_area_in    grid_in[].cell_area; NULL = the plan's own get_grid_area values (search-built plans only)
 *   cell_area_out   grid_out.cell_area; non-NULL switches the --target_grid rescale on (:842-869; the caller
 *                   leaves it NULL for use_volume variables, :536)
 *   monotonic       --monotonic limiter, conserve_order2 only (:617-748): one level per call
 * nz > 1 is legal only without has_missing / field_area / cell_methods_sum (:544-546).  With every option off
 * the result equals fg_plan_apply's bit for bit.  Levels are swept one launch each (these are the rarely used
 * branches; the bandwidth path is fg_plan_apply / fg_plan_apply_interleaved). */
typedef struct fg_apply_opts {
  int has_missing;
  double missing;
  const double *weight;
  int cell_methods_sum;
  const double *field_area;
  double area_missing;
  const double *cell_area_in;
  const double *cell_area_out;
  int monotonic;
} fg_apply_opts;
int fg_plan_apply_ex(fg_plan *plan, const fg_apply_opts *opts, const double *data, const double *grad_x,
                     const double *grad_y, const int *grad_mask, int nz, double *out, double *gsum_out);
/* The level loop of a field that uses these options, many levels per call.  The reference refuses nz > 1 for has_missing,
 * cell_measures and cell_methods = sum (conserve_interp.c:544-546), so fregrid.c:1045-1083 calls it once per level -- ocean
 * diagnostics with cell_measures = "area: areacello" / "volume: volcello" or cell_methods = "area: sum" have 50-75 levels,
 * each with its own land mask.  fg_plan_apply_levels_ex is that loop on the device, eight levels per launch: for
 * k = 0 .. nlev-1, out level k and gsum_out[k] hold the bits of do_scalar_conserve_interp(nz = 1) -- and of
 * fg_plan_apply_ex(opts, nz = 1) -- on level k alone with the same options (:561-616 order 1, :743-813 order 2, :815-866).
 * Per (exchange cell, level), in the reference's order: area *= weight; the data == missing test (has_missing); area /=
 * cell_area for sum, else with cell_measures the field_area == area_missing check and area *= (field_area / cell_area); the
 * value times that area.  The --target_grid sum (:842-858) takes every exchange cell of the row, missing or not, with the term
 * area * field_area / cell_area (left to right), or the plain area without cell_measures; the rescale applies where the
 * result != missing.  With every option off the result equals fg_plan_apply_levels' bit for bit.
 *   data, grad_x, grad_y, grad_mask, out, gsum_out: as fg_plan_apply_levels takes them.  opts->has_missing may be 0 or 1; with
 *     0 grad_mask may be NULL (and is not read).
 *   field_area_ld: 0 = opts->field_area is [ncells_in], shared by all levels (an area variable without a z axis);
 *     ncells_in = it is [nlev][ncells_in] (area_has_zaxis, fregrid_util.c:2156-2162, e.g. volcello), and the --target_grid sum
 *     is per level.  weight, cell_area_in and cell_area_out are shared by the levels, as in the reference.
 * FG_ERR_ARG, nothing written, plan still usable: opts->monotonic != 0; field_area_ld neither 0 nor ncells_in, or != 0
 * without field_area; sum or field_area without a cell area on a plan that holds none; NULL buffers; nlev < 1; a plan that is
 * not finalized.  A valid (cell, level) whose field_area == area_missing: FG_ERR_DATA, "data is not missing but area is
 * missing", as in fg_plan_apply_ex.
 * The monotone limiter on many levels has entries of its own, three kernels and a multi-rank split: fg_plan_apply_levels_mono
 * and fg_plan_mono_levels_* below; this entry goes on refusing opts->monotonic.  integration/ keeps the reference's per-level
 * loop (fregrid.c drives it one level per call).  use_volume: the caller passes cell_area_out = NULL, as for fg_plan_apply_ex. */
int fg_plan_apply_levels_ex(fg_plan *plan, const fg_apply_opts *opts, const double *data, const double *grad_x,
                            const double *grad_y, const int *grad_mask, int nlev, long field_area_ld, double *out,
                            double *gsum_out);
/* The same on the records fg_c2l_records_levels writes (rec [ncells_in][3][8], maskbits [ncells_in]; maskbits may be NULL
 * without has_missing): order-2 plans, 1 <= nz <= 8, opts->field_area [nz][ncells_in] when field_area_ld = ncells_in.
 * Bit-identical to fg_plan_apply_levels_ex. */
int fg_plan_apply_records_levels_ex(fg_plan *plan, const fg_apply_opts *opts, int nz, const double *rec,
                                    const unsigned char *maskbits, long field_area_ld, double *out, double *gsum_out);
/* Exchange cells the sweep above stages per chunk, for an area shared by the levels (per_level_area = 0) and for an area per
 * level (!= 0), whose table of scaled areas and target terms per (exchange cell, level) leaves room for half as many. */
int fg_plan_levels_ex_capacity(int per_level_area);

/* The monotone sweep split at the reference's mpp_min_double/mpp_max_double (:672-677) so that ranks holding bands of
 * one destination grid can all-reduce the per-source-cell extremes (MIN over f_min, MAX over f_max, ncells_in doubles
 * each, device pointers) between the two calls.  fg_plan_apply_ex(monotonic=1) is begin + end. */
int fg_plan_mono_begin(fg_plan *plan, const fg_apply_opts *opts, const double *data, const double *grad_x,
                       const double *grad_y, const int *grad_mask);
int fg_plan_mono_minmax_dev(fg_plan *plan, double **f_min, double **f_max);
/* device-to-device copy of the extremes out of (to_plan = 0) or back into (to_plan = 1) the plan, for callers whose
 * collective library wants its own buffers (torch.distributed); synchronises the plan's stream */
int fg_plan_mono_copy_minmax(fg_plan *plan, int to_plan, double *f_min, double *f_max);
int fg_plan_mono_end(fg_plan *plan, const fg_apply_opts *opts, const double *data, double *out, double *gsum_out);

/* The level loop of the monotone sweep (conserve_order2_monotonic / --monotonic), eight levels per launch.  The reference
 * limits one level per call (conserve_interp.c:648-651 index level 0 only; fregrid.c:1045-1083 loops), and so does
 * fg_plan_apply_ex(monotonic = 1).  fg_plan_apply_levels_mono is that loop on the device: for k = 0 .. nlev-1, out level k and
 * gsum_out[k] hold the bits of do_scalar_conserve_interp(nz = 1) with MONOTONIC set (:617-742, :815-866) -- and of
 * fg_plan_apply_ex(opts->monotonic = 1, nz = 1) -- on level k alone.  Per chunk of eight levels three kernels run beside the
 * transposition of the inputs: the bounds of every source cell's 3 x 3 neighbourhood (:622-645), the extremes of its exchange
 * cells' second-order values (:647-669, atomic max / min, order independent), and the sweep, which recomputes those values,
 * limits them (:679-716) and sums them with the options below; no per-exchange-cell array is stored.
 *   data       [nlev][F] with the one-cell halo; grad_x / grad_y [nlev][ncells_in] (device pointers, as fg_plan_apply_levels)
 *   grad_mask  int [nlev][ncells_in], or NULL = no cell is masked (as fg_plan_mono_begin reads NULL); read whether or not the
 *              field has missing values (:656)
 *   out        [nlev][ndst] (device); gsum_out: host double[nlev] or NULL, the sum of :815-819 per level
 *   opts       weight, cell_methods_sum, field_area [ncells_in] shared by the levels, cell_area_in and cell_area_out as in
 *              fg_plan_mono_end (:731-737, :841-865); has_missing / missing as there, without has_missing the marker is -1e20
 *              (:541).  The branch never sets out_miss: a destination cell without area becomes `missing`, never 0.0; it has
 *              no area_missing check.  opts->monotonic is not read: these entries are the monotone ones.  A field_area with
 *              a level axis is not taken (there is no field_area_ld argument here).
 * FG_ERR_ARG, nothing written, plan still usable: a first-order plan; a plan that is not finalized; NULL opts, data, out or
 * gradients; nlev < 1 (nz outside 1 .. 8 for the split); sum or field_area without a cell area on a plan that holds none.
 * FG_ERR_DATA: the limiter's fatal checks (:697, :709) on any level, with the reference's message (" xdata is greater than
 * f_bar_max " / " xdata is less than f_bar_min "), as fg_plan_apply_ex reports them; out is unspecified then, the plan stays
 * usable.  The error word is read once, after the last chunk.  Device scratch is sized for one chunk whatever nlev is.
 *
 * The split at mpp_min_double / mpp_max_double (:672-677) for ranks that hold bands of one destination grid, 1 <= nz <= 8
 * levels per begin / end pair: fg_plan_mono_levels_begin queues the bounds and the extremes of the chunk;
 * fg_plan_mono_levels_copy_minmax moves the extremes of the open chunk out of (to_plan = 0) or back into (to_plan = 1) the
 * plan -- f_min and f_max are device buffers, level-major [nz][ncells_in] each, so a rank all-reduces (MIN, MAX) one buffer per
 * chunk instead of one per level -- and synchronises the plan's stream like fg_plan_mono_copy_minmax; fg_plan_mono_levels_end
 * takes the same field arguments again (the caller keeps them unchanged between the two calls), limits and sweeps.
 * fg_plan_apply_levels_mono is begin + end per chunk of eight.  copy_minmax or end without an open begin: FG_ERR_STATE.
 * The limiter on the gradient object's records and in the streamed sweep: fg_plan_apply_records_levels_mono,
 * fg_plan_mono_records_* and fg_sweep_run_levels_mono below.
 * Out of scope: the multi-rank exchange inside the streamed sweep (ranks use the records split, fg_plan_mono_records_*, on
 * resident chunks); a field_area with a level axis; integration/, which fregrid.c drives one level per call. */
int fg_plan_apply_levels_mono(fg_plan *plan, const fg_apply_opts *opts, const double *data, const double *grad_x,
                              const double *grad_y, const int *grad_mask, int nlev, double *out, double *gsum_out);
int fg_plan_mono_levels_begin(fg_plan *plan, const fg_apply_opts *opts, const double *data, const double *grad_x,
                              const double *grad_y, const int *grad_mask, int nz);
int fg_plan_mono_levels_copy_minmax(fg_plan *plan, int to_plan, double *f_min, double *f_max);
int fg_plan_mono_levels_end(fg_plan *plan, const fg_apply_opts *opts, const double *data, const double *grad_x,
                            const double *grad_y, const int *grad_mask, double *out, double *gsum_out);

/* The limited sweep of 1 <= nz <= 8 levels on what fg_c2l_records_levels_mono writes -- rec [ncells_in][3][8], maskbits
 * [ncells_in] (NULL = no cell is masked, as a NULL grad_mask above) and the bounds records b8 [ncells_in][4][8] = f_bar_max |
 * f_bar_min | f_max | f_min -- order-2 plans only.  Two kernels run, the extremes (:647-669) and the limited sweep (:679-866),
 * straight on the caller's buffers: no transposition of the inputs, no mask-bits pass, no bounds pass, no halo'd copy of the field.
 * b8 is read AND written: the extremes go into its rows 2 and 3, so the call consumes it.  out [nz][ndst] and gsum_out[k] (host
 * double[nz] or NULL) carry the bits of fg_plan_apply_levels_mono on the same levels, i.e. of fg_plan_apply_ex(monotonic = 1,
 * nz = 1) per level.  opts as fg_plan_apply_levels_mono reads them (weight, cell_methods_sum, a field_area shared by the levels,
 * cell_area_in, cell_area_out, has_missing / missing; the marker is -1e20 without has_missing).
 * FG_ERR_ARG, nothing written, plan still usable: a first-order plan; a plan that is not finalized; NULL opts, rec, b8 or out;
 * nz outside 1 .. 8; sum or field_area without a cell area on a plan that holds none.  FG_ERR_DATA: the limiter's fatal checks
 * with the reference's messages, as above; the plan stays usable.
 * Several plans over one source grid share the bounds but not the extremes: fg_plan_mono_records_reset puts rows 2 and 3 of b8
 * back to -1e20 / +1e20 (128 bytes per source cell, on the plan's stream), so the next plan takes the same b8 without a second
 * bounds pass.
 * The split for ranks on records, with the semantics and state rules of fg_plan_mono_levels_*: fg_plan_mono_records_begin queues
 * the extremes of the chunk into the caller's b8, which stays the open chunk's bounds buffer until the end (the caller keeps rec,
 * maskbits and b8 unchanged in between); fg_plan_mono_records_copy_minmax moves f_min / f_max, level-major [nz][ncells_in] device
 * buffers, out of (to_plan = 0) or back into (to_plan = 1) that b8 and synchronises the plan's stream; fg_plan_mono_records_end
 * limits and sweeps.  copy_minmax or end without an open begin: FG_ERR_STATE.  fg_plan_apply_records_levels_mono is begin + end
 * and closes an open chunk. */
int fg_plan_apply_records_levels_mono(fg_plan *plan, const fg_apply_opts *opts, int nz, const double *rec,
                                      const unsigned char *maskbits, double *b8, double *out, double *gsum_out);
int fg_plan_mono_records_reset(fg_plan *plan, double *b8);
int fg_plan_mono_records_begin(fg_plan *plan, const fg_apply_opts *opts, int nz, const double *rec,
                               const unsigned char *maskbits, double *b8);
int fg_plan_mono_records_copy_minmax(fg_plan *plan, int to_plan, double *f_min, double *f_max);
int fg_plan_mono_records_end(fg_plan *plan, const fg_apply_opts *opts, const double *rec, const unsigned char *maskbits,
                             double *out, double *gsum_out);

/* HIP stream the plan launches on (hipStream_t as void*), for event timing. */
void *fg_plan_stream(fg_plan *plan);
/* wait for everything queued on the plan's stream */
int fg_plan_sync(fg_plan *plan);

/* Optional HIP-event timing of the library's own launches (on the plan's stream).
 * fg_plan_phase_ms: [0] cell records [1] binning [2] candidates [3] clip quad kernel
 * [4] clip general kernel [5] compaction (incl. cell sums) [6] destination rows [7] whole search (device span, includes
 * the two host round trips) [8] finalize [9] last sweep.  Milliseconds; zeros when profiling is off.
 * Rectilinear target: [0] also holds the candidates (the record kernel makes them), [2] only those of the listed (heavy) cells. */
void fg_set_profiling(int on);
int  fg_plan_phase_ms(fg_plan *plan, float *ms, int n);   /* [9] = mean over the sweeps since the last call */

/* per-phase statistics of the last search (counts), for DESIGN.md/bench reporting:
 * stats[0]=candidate pairs after the bounding-box tests, [1]=pairs with a non-empty clip,
 * [2]=nxgrid, [3]=pairs whose area ratio is within 1e-9 (relative) of the 1e-6 threshold,
 * [4]=bins, [5]=bin entries.  n = capacity of stats. */
int fg_plan_stats(const fg_plan *plan, long *stats, int n);
/* The search switches (fg_set_search_*, fg_set_gc_split, and fg_set_profiling for the search phases) are process-wide, are read
 * once when a plan-creating call starts, and do not affect a search already running. */
/* Search mode.  0 (default): every buffer of the search is sized by capacity (bin records 3*ndst, candidate pairs and
 * exchange cells 8*max(nsrc, ndst)), counts stay on the device and the host synchronises once, at the end; a search that
 * outgrows a capacity is repeated transparently with the sizes its counters report.  1: size every buffer by counting
 * first (extra passes; smallest plans).  Also selectable with the environment variable FREGRID_HIP_EXACT_SEARCH=1. */
void fg_set_search_mode(int exact);
/* 1: source cells whose latitude range cannot meet the destination grid are skipped when the per-cell records are built (a
 * rank of a banded multi-GPU job meets a fraction of the source cells); fg_plan_get_cell_area / _cell_struct then return 0 /
 * unspecified values for those cells.  The exchange cells are unchanged.  Default 0. */
void fg_set_search_cull(int on);
/* 1: a search also queues its own fg_plan_finalize -- centroid pass from the plan's OWN per-source-cell sums, CSR records --
 * before its one synchronisation, for jobs with one destination tile on one rank (conserve_interp.c:203-358 with ntiles_out = 1,
 * npes = 1: the plan's sums are the totals).  The plan comes back finalized: fg_plan_finalize(plan, NULL) then returns 0 at once,
 * with totals it is an error.  Applies to legacy-clip searches that run in one chunk (others finalize in fg_plan_finalize as
 * before).  Results do not depend on it.  Default 0. */
void fg_set_search_finalize(int on);
/* Stream-ordered plans.  1 (default): no call drains the GPU between one plan and the next.  A search that queues its own finalize
 * (fg_set_search_finalize) returns as soon as its counters are back -- they are final when the compaction ends -- while its
 * centroid pass and CSR records are still queued on the plan's stream; fg_plan_finalize with a plan on a stream the caller
 * supplied returns without a host wait (total_cell_sums_dev is then ordered on that stream by the caller, like every buffer of
 * an asynchronous call); fg_plan_destroy returns the plan's device blocks to the pool tagged with its stream instead of
 * synchronising it, and the next plan on that stream reuses them in stream order, a plan on another stream behind an event.
 * Every entry that reads a plan's results on the host, or moves it to another stream, waits for what is outstanding first, so
 * callers see no difference but the time.  0: the search synchronises its stream at its end and fg_plan_destroy at its start.
 * Results do not depend on it (tests/test_gpu_stream_ordered_plans.py).  With fg_set_profiling(1) a search synchronises as under 0.  A stream given to a
 * plan lives as long as the plan, as before; after fg_plan_destroy the library does not touch it again. */
void fg_set_search_async(int on);
/* Rectilinear destination grids -- lon_out a function of the column and lat_out of the row, bit for bit: every target
 * get_output_grid_by_size makes (fregrid_util.c:588-654), whole or a rank's band.  1 (default): the legacy search finds the
 * candidates of a source cell by index arithmetic on the two axes and builds destination cells from per-column / per-row tables
 * (no bins, no per-cell records); the property is verified on the device inside the search, and a grid that fails it is searched
 * by the generic path in the same call.  0: always the generic path.  Results do not depend on it (tests/test_gpu_rect.py). */
void fg_set_search_rect(int on);
/* Rectilinear path, grid sources: source cells are kept as 64-byte quadrilateral records, and the few that fix_lon leaves with
 * more than four vertices (a lone pole vertex, a half-turn edge) in a side table of ncells / 16 + 64 slots; a search that meets
 * more of them is repeated on the generic path in the same call.  n >= 0 lowers the table's capacity to n slots (tests of that
 * route), n < 0 restores the default.  Results do not depend on it. */
void fg_set_search_wide_cap(int n);
/* Longitude frame of the destination cells of a legacy search: 0 (default) create_xgrid's -- fix_lon(cell, pi), then the +-2pi shift
 * towards the source cell per pair (create_xgrid.c:1004,1062-1079); 1 make_coupler_mosaic's -- the cell is moved once per pair,
 * fix_lon(cell, mean longitude of the other cell) (make_coupler_mosaic.c:1452,1598).  Same exchange cells; the vertices (and so
 * the last bits of the areas) differ only for grids whose raw longitudes lie outside [0, 2pi).  coupler.py uses 1. */
void fg_set_search_frame(int coupler);
/* Sweep tuning hook: 1 (default) = 8-level order-2 sweeps on merged records use the entry-parallel kernel when rows are short
 * (nxgrid <= 6 x destination cells), 0 = always the row-serial kernel.  Results do not depend on it. */
void fg_set_apply_ep(int on);
/* Sweep tuning hook: levels per lane (1, 2 or 4; 0 = automatic).  Results do not depend on it. */
void fg_set_apply_vec(int v);
/* Great-circle search: 1 (default) = the clip runs as three passes (screen / extended-precision solves / walk) with the
 * one-kernel clip for the unusual pairs; 0 = the one-kernel clip for every pair; 2 = three passes with a task buffer 64 times
 * too small (test hook for the overflow path).  Results do not depend on it. */
void fg_set_gc_split(int on);
/* Sweep tuning hook, the tile -> XCD mapping: 0 = blocks in row order; 1 = each XCD sweeps one contiguous band of
 * destination rows (measured slower); C >= 2 = chunks of C consecutive tiles per XCD, chunks dealt round-robin (default 64,
 * see csrc/apply_kernels.hip).  Results do not depend on it. */
void fg_set_apply_xcd(int on);

/* Batched polygon primitives on the device.  Polygons are rows of host arrays [npoly][24];
 * inputs have at most 12 vertices (8 for fix_lon).  fg_clip_2dx2d_batch: n_out[p] = vertex count,
 * 0 = empty, -1 = parallel edges (fatal in the reference), -2 = more than 24 vertices.
 * fg_poly_op_batch: op 0 poly_area, 1 poly_ctrlon (clon[p]), 2 poly_ctrlat -> result[p];
 * op 3 fix_lon with tlon = clon[p], in place (lon/lat/n updated);
 * op 4, 5, 6: area, ctrlon (clon[p]) and ctrlat again, from the fused routine the order-2 clip kernels integrate with (one pass
 * over the edges for all three) -- a probe for tests: they equal ops 0, 1, 2 bit for bit. */
int fg_clip_2dx2d_batch(int npoly, const double *lon1, const double *lat1, const int *n1,
                        const double *lon2, const double *lat2, const int *n2,
                        double *lon_out, double *lat_out, int *n_out);
int fg_poly_op_batch(int op, int npoly, double *lon, double *lat, int *n, const double *clon, double *result);

/* ------------------------------------------------- order-2 input preparation ---- */
/* What get_input_data does for conserve_order2 before the sweep (tools/fregrid/fregrid_util.c:2137-2216):
 * copy each level into a halo'd array, fill the halo from the neighbouring tiles (update_halo :2614), run
 * grad_c2l (tools/libfrencutils/gradient_c2l.c:58) and build the missing-value gradient mask.  On the device. */
typedef struct fg_c2l fg_c2l;

/* Host, once per mosaic.  lonc/latc: corners [(ny+1)][(nx+1)], lont/latt: T-cell centres [ny][nx] (radians, host).
 * Contacts in the convention read_mosaic_contact hands to fregrid (read_mosaic.c:655-777): tile numbers 1-based,
 * 0-based model indices, istart == iend for a west/east edge (0 / nx-1), jstart == jend for south/north.
 * Computes calc_c2l_grid_info (gradient_c2l.c:368) per tile on the host and keeps it in HBM.
 * Refused with FG_ERR_ARG (fg_halo_map): contact indices outside their tile, and contacts between tiles of different sizes
 * where setup_boundary (fregrid_util.c:2446-2560), which sizes the neighbour's strip with the receiving tile's nx / ny, would
 * read another column or leave the array -- the reference does not define those. */
int  fg_c2l_create(int ntiles, const int *nx, const int *ny, const double *const *lonc, const double *const *latc,
                   const double *const *lont, const double *const *latt,
                   int ncontacts, const int *tile1, const int *tile2,
                   const int *istart1, const int *iend1, const int *jstart1, const int *jend1,
                   const int *istart2, const int *iend2, const int *jstart2, const int *jend2,
                   int device, fg_c2l **out);
void fg_c2l_destroy(fg_c2l *h);
long fg_c2l_ncells(const fg_c2l *h);        /* sum of nx*ny                   */
long fg_c2l_halo_size(const fg_c2l *h);     /* F = sum of (nx+2)*(ny+2)       */
int  fg_c2l_set_stream(fg_c2l *h, void *stream);
int  fg_c2l_sync(fg_c2l *h);
int  fg_c2l_get_centres(const fg_c2l *h, double *lont_halo, double *latt_halo);   /* host copies [F] */
/* src [nz][ncells] (tiles back to back) -> halo_data [nz][F] with the halo filled (src == NULL: interiors are
 * already in halo_data).  Device pointers. */
int  fg_c2l_fill_halo(fg_c2l *h, const double *src, double *halo_data, int nz);
/* halo_data [nz][F] -> grad_x, grad_y [nz][ncells]; grad_mask int [nz][ncells] or NULL.  Device pointers. */
int  fg_c2l_gradient(fg_c2l *h, const double *halo_data, int nz, int has_missing, double missing,
                     double *grad_x, double *grad_y, int *grad_mask);
/* The same gradients for 1 <= nz <= 8 levels, written straight into the layout the order-2 sweep reads:
 * rec[ncells][3][nb] = {field, grad_x, grad_y} x levels, nb = 2, 4 or 8 (the least >= nz, zero padded).  Device pointers;
 * rec holds ncells * 3 * nb doubles.  Pair with fg_plan_apply_records: halo_data -> records -> remapped levels, with no
 * level-major gradient arrays in between (no missing values: nz > 1 forbids them, conserve_interp.c:541). */
int  fg_c2l_gradient_records(fg_c2l *h, const double *halo_data, int nz, double *rec);
/* The whole preparation in one pass: src [nz][ncells] (no halo, as fg_c2l_fill_halo takes it) -> the same records, reading the
 * neighbour tiles' cells through the halo map instead of materialising the halo'd copy.  Bit-identical to
 * fg_c2l_fill_halo + fg_c2l_gradient_records. */
int  fg_c2l_records(fg_c2l *h, const double *src, int nz, double *rec);
/* fg_c2l_records for 1 <= nz <= 8 levels with missing values of their own: rec [ncells][3][8] (eight levels wide whatever nz)
 * and maskbits, unsigned char [ncells], bit k = grad_mask of level k (fregrid_util.c:2203-2215): one of the cell's EIGHT
 * neighbours -- not the cell itself -- equals `missing`, neighbours in other tiles read through the halo map, so a missing
 * cell across a cube edge or corner masks its neighbour.  Same bits as fg_c2l_fill_halo + fg_c2l_gradient(has_missing).
 * Pair with fg_plan_apply_records_levels.  Device pointers. */
int  fg_c2l_records_levels(fg_c2l *h, const double *src, int nz, double missing, double *rec, unsigned char *maskbits);
/* fg_c2l_records_levels plus the monotone limiter's bounds in the same pass (conserve_interp.c:622-645): rec and maskbits as
 * above, the same bits, and b8 [ncells][4][8] = f_bar_max | f_bar_min | f_max | f_min per level.  Rows 0 and 1: the maximum and
 * minimum over the nine values of the cell's 3 x 3 stencil that differ from `missing`, the centre included, starting from -1e20
 * and +1e20; the values are the stencil's own, read through the halo map -- a neighbour in another tile across a cube edge or
 * corner counts, an element no contact fills is 0.0 and is compared like any value.  Rows 2 and 3: -1e20 and +1e20, the start
 * values of the extremes.  Levels >= nz hold the start values in all four rows.  Bit-identical to the bounds
 * fg_plan_mono_levels_begin takes from the copy fg_c2l_fill_halo writes; no halo'd copy is made here.  Pair with
 * fg_plan_apply_records_levels_mono.  Device pointers; b8 holds ncells * 32 doubles. */
int  fg_c2l_records_levels_mono(fg_c2l *h, const double *src, int nz, double missing, double *rec, unsigned char *maskbits,
                                double *b8);

/* Host helpers behind fg_c2l_create, exported for tests and for callers without a mosaic file. */
int fg_c2l_grid_info(int nx, int ny, const double *xt, const double *yt, const double *xc, const double *yc,
                     double *dx, double *dy, double *area, double *edge_w, double *edge_e, double *edge_s,
                     double *edge_n, double *en_n, double *en_e, double *vlon, double *vlat);
int fg_find_contacts(int ntiles, const int *nx, const int *ny, const double *const *lonc, const double *const *latc,
                     int max_contacts, int *tile1, int *tile2, int *istart1, int *iend1, int *jstart1, int *jend1,
                     int *istart2, int *iend2, int *jstart2, int *jend2);
int fg_halo_map(int ntiles, const int *nx, const int *ny, int ncontacts, const int *tile1, const int *tile2,
                const int *istart1, const int *iend1, const int *jstart1, const int *jend1,
                const int *istart2, const int *iend2, const int *jstart2, const int *jend2,
                long *map_off, int *map);

/* ------------------------------------------------- remap file without libnetcdf -- */
/* Classic-netCDF writer/reader for fregrid's --remap_file (written at tools/fregrid/conserve_interp.c:368-445, read
 * through tools/libfrencutils/read_mosaic.c:352-558).  Host functions; see csrc/remap_file.c for the layout. */
int  fg_remap_write(const char *path, int order, long ncells, const int *tile1, const int *tile1_cell,
                    const int *tile2_cell, const double *xgrid_area, const double *tile1_distance);  /* file variables as is (1-based) */
int  fg_remap_write_interp(const char *path, int order, long n, const int *t_in, const int *i_in, const int *j_in,
                           const int *i_out, const int *j_out, const double *area, const double *di_in,
                           const double *dj_in, int isc, int jsc);                                    /* from 0-based Interp_config arrays */
long fg_remap_read_size(const char *path);                                                            /* read_mosaic_xgrid_size */
int  fg_remap_read(const char *path, int order, long ncells, int *t_in, int *i_in, int *j_in, int *i_out, int *j_out,
                   double *area, double *di_in, double *dj_in);                                       /* 0-based, reference conversions applied */
const char *fg_remap_last_error(void);

/* ------------------------------------------------- field / grid files without libnetcdf -- */
/* The operations fregrid performs on its files through tools/libfrencutils/mpp_io.c (mpp_open, mpp_get_varid,
 * mpp_get_var_att, mpp_get_var_value_block :443, mpp_def_dim / mpp_def_var / mpp_def_*_att / mpp_end_def,
 * mpp_put_var_value_block :1349, mpp_close), directly on classic netCDF files (CDF-1, CDF-2, CDF-5; csrc/field_file.c).
 * Host functions.  Types follow netCDF's numbering. */
#define FG_NC_BYTE 1
#define FG_NC_CHAR 2
#define FG_NC_SHORT 3
#define FG_NC_INT 4
#define FG_NC_FLOAT 5
#define FG_NC_DOUBLE 6
typedef struct fg_ncfile fg_ncfile;
int  fg_nc_open(const char *path, fg_ncfile **out);                                  /* read only */
int  fg_nc_create(const char *path, int version /* 1, 2 or 5 */, fg_ncfile **out);   /* define mode */
int  fg_nc_def_dim(fg_ncfile *f, const char *name, long len /* 0: unlimited */);     /* returns the dimension id */
int  fg_nc_def_var(fg_ncfile *f, const char *name, int type, int ndims, const int *dimids);   /* returns the variable id */
int  fg_nc_put_att_text(fg_ncfile *f, int varid /* -1: global */, const char *name, const char *val);
int  fg_nc_put_att_double(fg_ncfile *f, int varid, const char *name, int type, int n, const double *vals);
int  fg_nc_enddef(fg_ncfile *f);
int  fg_nc_inq_ndims(const fg_ncfile *f);
int  fg_nc_inq_nvars(const fg_ncfile *f);
long fg_nc_inq_numrecs(const fg_ncfile *f);
int  fg_nc_inq_dimid(const fg_ncfile *f, const char *name);                          /* -1 if absent */
int  fg_nc_inq_dim(const fg_ncfile *f, int dimid, char *name, int cap, long *len);
int  fg_nc_inq_varid(const fg_ncfile *f, const char *name);                          /* -1 if absent */
int  fg_nc_inq_var(const fg_ncfile *f, int varid, char *name, int cap, int *type, int *ndims, int *dimids, long *shape);
int  fg_nc_get_att_double(const fg_ncfile *f, int varid, const char *name, double *val, int cap);   /* elements copied, or FG_ERR_NOTFOUND */
int  fg_nc_get_att_text(const fg_ncfile *f, int varid, const char *name, char *buf, int cap);       /* length, or FG_ERR_NOTFOUND */
int  fg_nc_get_vara(fg_ncfile *f, int varid, const long *start, const long *count, void *out);      /* the variable's own type */
int  fg_nc_get_vara_double(fg_ncfile *f, int varid, const long *start, const long *count, double *out);
int  fg_nc_put_vara(fg_ncfile *f, int varid, const long *start, const long *count, const void *data);
int  fg_nc_put_vara_double(fg_ncfile *f, int varid, const long *start, const long *count, const double *data);
int  fg_nc_close(fg_ncfile *f);
const char *fg_nc_last_error(void);

/* ------------------------------------------------- streamed sweep: fields from host memory through the plans ---- */
/* fregrid's per-field loop (fregrid.c:1001-1075): get_input_data (read a hyperslab, widen NC_FLOAT / NC_SHORT / NC_INT to
 * double, scale and offset, fregrid_util.c:2036-2165), [halo update + grad_c2l,] do_scalar_conserve_interp per output tile,
 * write_field_data (offset, scale, cast to the file type, :2339-2418).  fg_sweep keeps that loop's data path on the device
 * and the PCIe link busy: levels cross the link in their FILE type (a float level is half the bytes), in chunks of up to 8
 * levels, through pinned double buffers on a copy-in stream / compute stream / copy-out stream, so that the upload of
 * chunk k+1 and the download of chunk k-1 run beside the sweep of chunk k.  Widening, scaling and the inverse conversions
 * run on the device with the reference's operations (exact: float -> double is exact, (float)double is the C cast
 * nc_put_vara_double applies).
 *   plans[nplans]: finalized plans sharing the source grid, one per output tile.  c2l: gradient preparation for
 *   conserve_order2 plans (NULL for order 1).  in_type / out_type: FG_NC_SHORT, FG_NC_INT, FG_NC_FLOAT or FG_NC_DOUBLE.
 * fg_sweep_run: host_in [nlev][ncells_in] of in_type (tiles back to back, no halo), host_out[p] [nlev][ndst_p] of out_type.
 *   scale / offset: the variable's scale_factor / add_offset (0 = absent, as the reference treats them); applied to values
 *   != missing.  fg_sweep_run treats every value as data (conserve_interp.c:544 requires nz == 1 for a variable with missing
 *   values); such a variable goes through fg_sweep_run_levels.
 * fg_sweep_run_levels: the same arguments, buffers, slots, streams and events for a variable WITH missing values: every level
 *   is remapped as do_scalar_conserve_interp(nz = 1, has_missing = 1) would remap it alone (fg_plan_apply_levels; for order 2
 *   fg_c2l_records_levels + fg_plan_apply_records_levels per chunk), `missing` marking the cells to leave out; it comes back
 *   as `missing` cast to the output type (write_field_data leaves it alone).  A plan that is not finalized is refused with
 *   FG_ERR_ARG before anything is copied.
 * Buffers from fg_host_alloc are page-locked: copies go straight from / to them; other host memory is staged through the
 * object's own pinned buffers with one extra host copy.
 * Streams and lifetimes: the plans and the gradient object run on the sweep's compute stream only INSIDE fg_sweep_run (they get
 * their own streams back before it returns, on errors too), so several fg_sweep objects -- fregrid needs one per pair of
 * file types -- may share plans, and plans / sweeps may be destroyed in any order.  A plan serves one call at a time: do not
 * call fg_sweep_run on two host threads with a plan in common.  After an error return the object is clean and may be run again.
 * Out-of-range narrowing (NC_SHORT / NC_INT outputs beyond the type's range, e.g. a missing value of -1e20): the device cast
 * saturates, the reference's host cast (fregrid_util.c:2395-2406) is undefined behaviour that yields INT_MIN on x86 --
 * parity unpinned, no fixture in the reference covers it. */
/* The two conversions alone, on device buffers (synchronous): out[i] = (double)raw[i], `*= scale` / `+= offset` where != missing
 * (get_input_data, fregrid_util.c:2097-2123); and the inverse with the C cast to the file type (write_field_data, :2376-2406).
 * nc_type: FG_NC_SHORT / _INT / _FLOAT / _DOUBLE.  integration/field_io_hip.c builds fregrid's per-level loop from them. */
int fg_dev_widen(int nc_type, long n, const void *raw_dev, double scale, double offset, double missing, double *out_dev);
int fg_dev_narrow(int nc_type, long n, const double *in_dev, double scale, double offset, double missing, void *out_dev);
typedef struct fg_sweep fg_sweep;
int  fg_sweep_create(int nplans, fg_plan *const *plans, fg_c2l *c2l, int in_type, int out_type, fg_sweep **out);
int  fg_sweep_run(fg_sweep *sw, const void *host_in, long nlev, double scale, double offset, double missing,
                  void *const *host_out);
int  fg_sweep_run_levels(fg_sweep *sw, const void *host_in, long nlev, double scale, double offset, double missing,
                         void *const *host_out);
/* fg_sweep_run_levels with the options of fg_plan_apply_levels_ex (fg_apply_opts is declared with fg_plan_apply_ex).  The
 * option arrays are device-resident and shared by the levels (field_area_ld = 0) and by all plans of the sweep, so
 * opts->cell_area_out is legal only for a sweep of one plan (else FG_ERR_ARG).  The missing value is the options':
 * opts->missing with has_missing, else -1e20 (conserve_interp.c:541-542); it also steers the scale / offset conversion.
 * Out of scope: streaming a per-level area variable (volcello) beside the field -- such a field takes
 * fg_plan_apply_levels_ex on resident levels. */
int  fg_sweep_run_levels_ex(fg_sweep *sw, const fg_apply_opts *opts, const void *host_in, long nlev, double scale,
                            double offset, void *const *host_out);
/* fg_sweep_run_levels_ex for a --monotonic field (conserve_order2_monotonic): the same buffers, slots, three streams, events,
 * widening and narrowing; per chunk of eight levels the compute stream takes one fg_c2l_records_levels_mono and then, per plan,
 * the extremes reset (from the second plan on) and fg_plan_apply_records_levels_mono.  Scratch per slot: one chunk's b8.  Every
 * level of every output carries the bits of the per-level chain widen, fg_c2l_fill_halo, fg_c2l_gradient(has_missing),
 * fg_plan_apply_ex(monotonic = 1, nz = 1), narrow on that level alone.  Options and missing value as fg_sweep_run_levels_ex
 * (opts->monotonic is not read).  The plans' error word is cleared before the first chunk and read once after the last: a fatal
 * level gives FG_ERR_DATA with the reference's message; the object stays clean and may be run again.  FG_ERR_ARG before anything
 * is copied: a sweep created without a gradient object or with first-order plans; opts->cell_area_out with more than one plan; a
 * plan that is not finalized.  Out of scope: the multi-rank exchange of the extremes inside the streamed sweep. */
int  fg_sweep_run_levels_mono(fg_sweep *sw, const fg_apply_opts *opts, const void *host_in, long nlev, double scale,
                              double offset, void *const *host_out);
void fg_sweep_destroy(fg_sweep *sw);
void *fg_host_alloc(size_t bytes);      /* page-locked host memory (hipHostMalloc), NULL on failure */
void fg_host_free(void *p);

/* ---------------------------------------------------------------- (G) ----- */
/* Equal-distance gnomonic cubed sphere ("gnomonic_ed"), C<ni>: cell corners of the six
 * tiles, lonc/latc[6*(ni+1)*(ni+1)] radians.  shift_fac as make_hgrid (default 18).
 * via_degrees != 0 reproduces the radians->degrees->radians round trip of the grid file. */
int fg_gnomonic_ed_corners(int ni, double shift_fac, int via_degrees, double *lonc, double *latc);
/* same, plus the T-cell centres lont/latt[6*ni*ni] (cell_center, create_gnomonic_cubic_grid.c:2008) */
int fg_gnomonic_ed_grid(int ni, double shift_fac, int via_degrees, double *lonc, double *latc, double *lont, double *latt);
/* Regular lat-lon grid of get_output_grid_by_size (degrees in, radians out),
 * lonc/latc[(nlat+1)*(nlon+1)]. */
int fg_latlon_corners(int nlon, int nlat, double lonbegin, double lonend, double latbegin,
                      double latend, int center_y, double *lonc, double *latc);

/* ---------------------------------------------------------------------------------------------------------
 * Great-circle exchange grid: create_xgrid_great_circle (create_xgrid.c:1366-1466), used by fregrid for grids
 * flagged great_circle_algorithm (opcode GREAT_CIRCLE, conserve_interp.c:164-168; first order only, fregrid.c:763).
 * Cell edges are great-circle arcs; areas are spherical excesses.  The plan that results is an ordinary first-order
 * plan: fg_plan_finalize / fg_plan_get_xgrid / fg_plan_apply* work on it unchanged (xgrid_clon/clat are zero in the
 * reference, :1446-1447).  fg_plan_create_great_circle takes host corner arrays (radians); the unit vectors are
 * formed on the host with libm exactly like latlon2xyz (mosaic_util.c:212-222) -- see fg_latlon2xyz -- everything
 * else runs on the device.  fg_plan_create_great_circle_dev takes DEVICE arrays of unit vectors.
 * The source rows are not trimmed (conserve_interp.c:164 passes the whole tile).  Returns nxgrid or FG_ERR_*;
 * FG_ERR_GEOM carries the reference's fatal message ("grid box 1 is not convex", ...). */
long fg_plan_create_great_circle(int ntiles_in, const int *nx_in, const int *ny_in,
                                 const double *const *lon_in, const double *const *lat_in, const double *const *mask_in,
                                 int nx_out, int ny_out, const double *lon_out, const double *lat_out,
                                 int device, fg_plan **plan);
long fg_plan_create_great_circle_dev(int ntiles_in, const int *nx_in, const int *ny_in,
                                     const double *const *d_x_in, const double *const *d_y_in, const double *const *d_z_in,
                                     const double *const *d_mask_in, int nx_out, int ny_out,
                                     const double *d_x_out, const double *d_y_out, const double *d_z_out,
                                     double mean_dlat, double mean_dlon, int device, void *stream, int use_caller_stream,
                                     fg_plan **plan);
/* latlon2xyz (mosaic_util.c:212-222) with the host libm, threaded */
void fg_latlon2xyz(long size, const double *lon, const double *lat, double *x, double *y, double *z);
/* latlon2xyz on the device: d_lon, d_lat [n] in, d_x, d_y, d_z [n] out, all DEVICE pointers; queued on `stream` of `device`, no
 * synchronisation.  The results carry the bits of fg_latlon2xyz on an FMA-capable x86-64 host (glibc 2.35's sin() / cos(),
 * restated in csrc/sincos_glibc.h).  Domain: finite coordinates, |lat| < 2.4262 (libm's first three branches) and
 * |lon| <= 1024 rad; a point outside it becomes NaN in all three outputs.  Returns 0 or FG_ERR_*. */
int fg_dev_latlon2xyz(long n, const double *d_lon, const double *d_lat, double *d_x, double *d_y, double *d_z, int device, void *stream);
/* Great-circle plans from lon / lat corner arrays (radians) with the conversion above on the device -- no host trig.
 * fg_plan_create_great_circle_lonlat_dev: the argument list of fg_plan_create_great_circle_dev with DEVICE lon / lat arrays in
 * place of the unit vectors.  The plan takes the unit-vector buffers from its pool, queues the conversion of every grid (one
 * launch) ahead of the search on its stream and hands the buffers back when the search is done; the caller's arrays are not
 * read after the call returns.  mean_dlat / mean_dlon <= 0: derived from a sample of the converted destination corners.
 * fg_plan_create_great_circle_lonlat: the argument list of fg_plan_create_great_circle; uploads lon / lat (16 bytes per corner
 * instead of 24) and takes the same path.  A corner outside the conversion's domain gives FG_ERR_ARG (found at the search's
 * one read-back).  The unit vectors are the ones fg_plan_create_great_circle forms on the host, so the plans are identical. */
long fg_plan_create_great_circle_lonlat(int ntiles_in, const int *nx_in, const int *ny_in,
                                        const double *const *lon_in, const double *const *lat_in, const double *const *mask_in,
                                        int nx_out, int ny_out, const double *lon_out, const double *lat_out,
                                        int device, fg_plan **plan);
long fg_plan_create_great_circle_lonlat_dev(int ntiles_in, const int *nx_in, const int *ny_in,
                                            const double *const *d_lon_in, const double *const *d_lat_in,
                                            const double *const *d_mask_in, int nx_out, int ny_out,
                                            const double *d_lon_out, const double *d_lat_out,
                                            double mean_dlat, double mean_dlon, int device, void *stream, int use_caller_stream,
                                            fg_plan **plan);
/* B1 drop-ins (create_xgrid.h): same prototypes as the reference */
int create_xgrid_great_circle(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out,
                              const double *lon_in, const double *lat_in, const double *lon_out, const double *lat_out,
                              const double *mask_in, int *i_in, int *j_in, int *i_out, int *j_out,
                              double *xgrid_area, double *xgrid_clon, double *xgrid_clat);
int create_xgrid_great_circle_(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out,
                               const double *lon_in, const double *lat_in, const double *lon_out, const double *lat_out,
                               const double *mask_in, int *i_in, int *j_in, int *i_out, int *j_out,
                               double *xgrid_area, double *xgrid_clon, double *xgrid_clat);
void get_grid_great_circle_area(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area);
void get_grid_great_circle_area_(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area);
/* interp.c:312: first-order remap through the great-circle exchange grid (same contract as conserve_interp) */
void conserve_interp_great_circle(int nx_src, int ny_src, int nx_dst, int ny_dst, const double *x_src, const double *y_src,
                                  const double *x_dst, const double *y_dst, const double *mask_src, const double *data_src,
                                  double *data_dst);
int clip_2dx2d_great_circle(const double x1_in[], const double y1_in[], const double z1_in[], int n1_in,
                            const double x2_in[], const double y2_in[], const double z2_in[], int n2_in,
                            double x_out[], double y_out[], double z_out[]);
double great_circle_area(int n, const double *x, const double *y, const double *z);
/* npairs quadrilateral pairs at once: a, b [npairs][4][3] unit vectors (clockwise); out [npairs][16][3], n_out[npairs]
 * (negative = the reference would have aborted, code as in oracle/gc_oracle.c), area[npairs] of the clipped polygon.
 * Host pointers. */
int fg_gc_clip_batch(int npairs, const double *a, const double *b, double *out, int *n_out, double *area, int device);

/* ---------------------------------------------------------------------------------------------------------
 * The 1-D x 2-D exchange-grid variants and box primitives of libfrencutils (create_xgrid.h:37-64), same prototypes.
 * create_xgrid_1dx2d_*: the SOURCE grid is regular and given by its 1-D bounds lon_in[nlon_in+1], lat_in[nlat_in+1];
 * create_xgrid_2dx1d_*: the DESTINATION grid is (lon_out[nlon_out+1], lat_out[nlat_out+1]).  mask_in is on the source
 * cells in both.  Callers in the reference: make_coupler_mosaic, make_topog, river tools (not fregrid). */
int create_xgrid_1dx2d_order1(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out, const double *lon_in,
                              const double *lat_in, const double *lon_out, const double *lat_out, const double *mask_in,
                              int *i_in, int *j_in, int *i_out, int *j_out, double *xgrid_area);
int create_xgrid_1dx2d_order2(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out, const double *lon_in,
                              const double *lat_in, const double *lon_out, const double *lat_out, const double *mask_in,
                              int *i_in, int *j_in, int *i_out, int *j_out, double *xgrid_area, double *xgrid_clon, double *xgrid_clat);
int create_xgrid_2dx1d_order1(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out, const double *lon_in,
                              const double *lat_in, const double *lon_out, const double *lat_out, const double *mask_in,
                              int *i_in, int *j_in, int *i_out, int *j_out, double *xgrid_area);
int create_xgrid_2dx1d_order2(const int *nlon_in, const int *nlat_in, const int *nlon_out, const int *nlat_out, const double *lon_in,
                              const double *lat_in, const double *lon_out, const double *lat_out, const double *mask_in,
                              int *i_in, int *j_in, int *i_out, int *j_out, double *xgrid_area, double *xgrid_clon, double *xgrid_clat);
int create_xgrid_1dx2d_order1_(const int *, const int *, const int *, const int *, const double *, const double *, const double *,
                               const double *, const double *, int *, int *, int *, int *, double *);
int create_xgrid_1dx2d_order2_(const int *, const int *, const int *, const int *, const double *, const double *, const double *,
                               const double *, const double *, int *, int *, int *, int *, double *, double *, double *);
int create_xgrid_2dx1d_order1_(const int *, const int *, const int *, const int *, const double *, const double *, const double *,
                               const double *, const double *, int *, int *, int *, int *, double *);
int create_xgrid_2dx1d_order2_(const int *, const int *, const int *, const int *, const double *, const double *, const double *,
                               const double *, const double *, int *, int *, int *, int *, double *, double *, double *);
int clip(const double lon_in[], const double lat_in[], int n_in, double ll_lon, double ll_lat, double ur_lon, double ur_lat,
         double lon_out[], double lat_out[]);
double box_ctrlat(double ll_lon, double ll_lat, double ur_lon, double ur_lat);
double box_ctrlon(double ll_lon, double ll_lat, double ur_lon, double ur_lat, double clon);
void get_grid_area_no_adjust(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area);
void get_grid_area_no_adjust_(const int *nlon, const int *nlat, const double *lon, const double *lat, double *area);

/* sin and cos of n host values as the device kernels evaluate them for latitudes (|x| < 2.426): a parity probe --
 * the results must equal the host libm's bit for bit (tests/test_gpu_xgrid.py). */
int fg_sincos_batch(long n, const double *x, double *s, double *c, int device);

/* Tripolar ocean grid (make_hgrid --grid_type tripolar_grid, uniform bounds, Murray bipolar cap north of lat_join):
 * nlon x nlat model cells, bounds in degrees, lonc/latc[(nlat+1)*(nlon+1)] radians.  Input synthesis only (see grid_gen.c). */
int fg_tripolar_corners(int nlon, int nlat, double xbnd0, double xbnd1, double ybnd0, double ybnd1, double lat_join,
                        double *lonc, double *latc);

/* ---------------------------------------------------------------------------------------------------------
 * Bilinear cubed-sphere -> lat-lon regridding (fregrid --interp_method bilinear; tools/fregrid/bilinear_interp.c):
 * setup_bilinear_interp (:72-434) and do_scalar / do_vector_bilinear_interp (:436-560) on the device.
 * Source: the six N x N tiles of a cubed sphere as T-cell centres lont/latt [N][N] (radians, host) and the mosaic's 12 contacts
 * in fg_c2l_create's convention; the halo'd centres are built as get_input_grid does (fregrid_util.c:236-312: CENTER halo
 * update, halo corners left at init_halo's zero).  Target: the lat-lon grid of get_output_grid_by_size (degrees), refined
 * finer_step times; the search and the weights run on the fine grid, [nlat_fine][nlon_fine] with
 * nlon_fine = 2^finer_step * nlon and nlat_fine = 2^finer_step * (nlat - 1) + 1.
 * The libm functions of the search windows and of the weights (acos, sin, asin) are evaluated with the host libm between
 * two device passes, so the weights round as the reference's do.
 * index [npts][3] = (ic, jc, tile) of the lower-left source centre in halo'd coordinates (0..N), weight [npts][4] in the order
 * (ic, jc), (ic, jc+1), (ic+1, jc+1), (ic+1, jc) -- the reference's Interp_config arrays.
 * Refused with FG_ERR_ARG (the reference exits): ntiles != 6, ncontacts != 12, finer_step < 0, nlat < 2, tiles not N x N.
 * FG_ERR_BILIN_NOTFOUND: points still unfound after the 10 sweeps (the reference's "global sweep" fallback reads past its
 * arrays and is not reproduced); fg_last_error() gives the count. */
typedef struct fg_bilin fg_bilin;
int  fg_bilin_create(int ntiles, const int *nx, const int *ny, const double *const *lont, const double *const *latt,
                     int ncontacts, const int *tile1, const int *tile2, const int *istart1, const int *iend1,
                     const int *jstart1, const int *jend1, const int *istart2, const int *iend2, const int *jstart2,
                     const int *jend2, int nlon, int nlat, int finer_step, double lonbegin, double lonend,
                     double latbegin, double latend, int center_y, int device, fg_bilin **out);
/* the READ branch: index / weight (host, e.g. from fg_bilin_remap_read) instead of the search */
int  fg_bilin_create_from_weights(int ntiles, const int *nx, const int *ny, const double *const *lont, const double *const *latt,
                                  int ncontacts, const int *tile1, const int *tile2, const int *istart1, const int *iend1,
                                  const int *jstart1, const int *jend1, const int *istart2, const int *iend2, const int *jstart2,
                                  const int *jend2, int nlon, int nlat, int finer_step, double lonbegin, double lonend,
                                  double latbegin, double latend, int center_y, const int *index, const double *weight,
                                  int device, fg_bilin **out);
void fg_bilin_destroy(fg_bilin *h);
int  fg_bilin_get_index_weight(const fg_bilin *h, int *index, double *weight);   /* host [npts][3], [npts][4]; either may be NULL */
long fg_bilin_npoints_fine(const fg_bilin *h);
int  fg_bilin_nlon_fine(const fg_bilin *h);
int  fg_bilin_nlat_fine(const fg_bilin *h);
int  fg_bilin_nlon(const fg_bilin *h);
int  fg_bilin_nlat(const fg_bilin *h);
long fg_bilin_ncells(const fg_bilin *h);                                          /* 6 * N * N */
/* nearest-centre comparisons of the search between different distance cosines whose distances were equal or one ulp apart
 * once correctly rounded: the only
 * ones the host libm's acos, which is not correctly rounded, could order otherwise (0 for a computed plan that cannot differ
 * from the reference on that account; 0 for a plan read from weights) */
long fg_bilin_ambiguous_ties(const fg_bilin *h);
int  fg_bilin_set_stream(fg_bilin *h, void *stream);
int  fg_bilin_sync(fg_bilin *h);
/* src [nz][6*N*N] (tiles back to back, no halo; the halo is read through the contacts) -> out [nz][nlat][nlon], device pointers.
 * Every level equals a one-level call.  has_missing: a point with any of its four corners equal to missing (a halo corner
 * counts as 0) gets missing, or with fill_missing the corner of largest weight.  finer_step > 0 coarsens with redu2x, whose
 * missing-value branch divides the x-swept values by the missing value before the cos(lat) scaling (:1121), as the reference does. */
int  fg_bilin_apply_scalar(fg_bilin *h, const double *src, int nz, int has_missing, double missing, int fill_missing, double *out);
/* u, v [nz][6*N*N] eastward / northward components -> u_out, v_out [nz][nlat][nlon]: projected onto x, y, z, interpolated
 * (missing tested on the projected values) and rotated onto the lat-lon directions (:476-560) */
int  fg_bilin_apply_vector(fg_bilin *h, const double *u, const double *v, int nz, int has_missing, double missing, int fill_missing,
                           double *u_out, double *v_out);
/* Streamed bilinear fields: fregrid's field loop around the bilinear plan (fregrid.c:1013-1112: get_input_data, the halo
 * update, do_scalar / do_vector_bilinear_interp, write_field_data), built like fg_sweep above: levels cross the link in their
 * FILE type, in chunks of up to 8 levels, through three buffer slots on a copy-in, a compute and a copy-out stream, so that the
 * upload of chunk k+1 and the download of chunk k-1 run beside the remap of chunk k.  One kernel per chunk gathers the four
 * corners of every fine point in the file type, widens each as get_input_data does ((double)raw, `*= scale` / `+= offset` where
 * != missing; a halo corner stays init_halo's 0.0: the reference converts the unpadded block only, fregrid_util.c:2117-2124),
 * interpolates, and narrows as write_field_data does; no double copy of a level exists on the device.  finer_step > 0 gathers
 * into a double workspace, coarsens and narrows in the last coarsening step.
 *   in_type / out_type: FG_NC_SHORT, FG_NC_INT, FG_NC_FLOAT or FG_NC_DOUBLE.
 *   host_in (host_u, host_v) [nlev][6*N*N] of in_type, tiles back to back, no halo; outputs [nlev][nlat][nlon] of out_type.
 *   conv: the variable's scale_factor / add_offset (0 = absent) and missing_value, for its widening and its narrowing; u and v
 *   carry their own.  has_missing / fill_missing as fg_bilin_apply_*; the interpolation's and the coarsening's missing value is
 *   conv->missing, for vectors conv_u->missing (bilinear_interp.c:494-495).
 * Every level of every output carries the bits of the per-level chain fg_dev_widen, fg_bilin_apply_scalar / _vector(nz = 1),
 * fg_dev_narrow on that level alone.  FG_ERR_ARG before anything is copied: a type outside the four, a null pointer, nlev < 1.
 * Buffers from fg_host_alloc are used in place, other host memory is staged through the object's pinned buffers (allocated on
 * first need, like the second component's slots and the workspace).  The object launches on its own streams and only reads
 * the plan: the plan's stream is the same before and after a run, several sweeps -- one per pair of file types -- may share a
 * plan, plan and sweeps may be destroyed in any order, and after an error return the object is clean and may be run again.
 * A sweep serves one call at a time.  Out-of-range narrowing to NC_SHORT / NC_INT is parity-unpinned, as for fg_sweep.
 * Out of scope: more than one output tile, --extrapolate before the remap. */
typedef struct fg_bilin_sweep fg_bilin_sweep;
typedef struct { double scale, offset, missing; } fg_field_conv;   /* scale / offset 0 = absent */
int  fg_bilin_sweep_create(fg_bilin *h, int in_type, int out_type, fg_bilin_sweep **out);
int  fg_bilin_sweep_run_scalar(fg_bilin_sweep *sw, const void *host_in, long nlev, const fg_field_conv *conv,
                               int has_missing, int fill_missing, void *host_out);
int  fg_bilin_sweep_run_vector(fg_bilin_sweep *sw, const void *host_u, const void *host_v, long nlev,
                               const fg_field_conv *conv_u, const fg_field_conv *conv_v,
                               int has_missing, int fill_missing, void *host_u_out, void *host_v_out);
void fg_bilin_sweep_destroy(fg_bilin_sweep *sw);
/* fregrid's bilinear remap file (host): dimensions nlon, nlat, three, four; index NC_INT and weight NC_DOUBLE declared
 * (three|four, nlat, nlon) and holding the point-major arrays as they lie in memory, CDF-2 like fg_remap_write.
 * fg_bilin_remap_read refuses a file whose nlon / nlat differ from the fine grid's (FG_ERR_ARG). */
int  fg_bilin_remap_write(const char *path, int nlon_fine, int nlat_fine, const int *index, const double *weight);
int  fg_bilin_remap_read(const char *path, int nlon_fine, int nlat_fine, int *index, double *weight);
/* host helpers behind fg_bilin_create (exported for tests): unit_vect_latlon (mosaic_util.c:937) and the fine target grid */
void fg_unit_vect_latlon(long size, const double *lon, const double *lat, double *vlon, double *vlat);
void fg_bilin_fine_grid(int nlon, int nlat, int finer_step, double lonbegin, double lonend, double latbegin, double latend,
                        int center_y, double *lont, double *latt, double *latt1d);

/* ---------------------------------------------------------------------------------------------------------
 * fregrid --extrapolate and --dst_vgrid (the ocean initial-condition recipe: lat-lon climatology -> tripolar):
 * do_extrapolate (tools/fregrid/fregrid_util.c:2662-2812) fills the missing points (land) of a lat-lon source field before the
 * remap -- a relaxed Jacobi iteration of a spherical 5-point Laplacian, per level until the largest residual is <= stop_crit
 * or 4000 iterations have run; setup_vertical_interp / do_vertical_interp (:756-819, linear_vertical_interp interp.c:360-396)
 * put the remapped levels onto the --dst_vgrid levels.  Both on the device, bit for bit the reference's arithmetic.
 *
 * fg_extrap_create: the grid factors of one source grid (:2676-2720); lon[ni], lat[nj] the T-cell axes in radians (host),
 * grid_in[].lont1D / latt1D.  The cosines are evaluated with the operation sequence of the reference's build host's libm, on
 * the host, whatever libm this host has.  One handle serves every field and tile on that grid; it owns a non-blocking stream.
 * fg_extrap_run_dev: d_in, d_out [nk] levels of [nj][ni], level k at k * level_stride doubles (0 = ni*nj), device pointers; d_out may
 * equal d_in.  A point is missing where fabs(v - missing) <= 1e-10.  Missing points of level 0 start from 0, those of level k
 * from the solution of level k-1 (the reference's warm start: the levels are sequential).  iters_out[nk] (host, may be NULL)
 * receives the 0-based iteration the level stopped after -- the number the reference prints -- and resmax_out[nk] its largest
 * residual.  Iterations are queued in batches with no host synchronisation inside a batch (one per batch: ceil((iters+1)/batch)
 * per level); the call returns when d_out is complete.  fg_extrap_run: the same on host arrays [nk][nj][ni]. */
typedef struct fg_extrap fg_extrap;
int  fg_extrap_create(int ni, int nj, const double *lon, const double *lat, int is_cyclic, int device, fg_extrap **out);
void fg_extrap_destroy(fg_extrap *h);
int  fg_extrap_set_stream(fg_extrap *h, void *stream);      /* queue on the caller's hipStream_t instead */
void *fg_extrap_stream(fg_extrap *h);
int  fg_extrap_run_dev(fg_extrap *h, const double *d_in, double *d_out, int nk, long level_stride, double missing,
                       double stop_crit, int *iters_out, double *resmax_out);
int  fg_extrap_run(fg_extrap *h, const double *in, double *out, int nk, double missing, double stop_crit,
                   int *iters_out, double *resmax_out);
long fg_extrap_last_syncs(const fg_extrap *h);              /* host synchronisations of the last run's iteration loops */
/* fg_extrap_run_dev for nrec records of nk levels on the handle's grid, filled in the same launches: record r, level k at
 * r * rec_stride + k * level_stride doubles (a stride of 0: densely packed, level_stride = ni*nj, rec_stride = nk * level_stride);
 * d_out may equal d_in.  The records advance through the levels in lockstep -- level k of all records is prepared in one launch
 * and iterated with ONE launch per iteration for all records (the record is a grid dimension); the next level starts when every
 * record has stopped on this one -- but each record is its own problem: its own chain of 4000 maximum slots (a block of record r
 * in launch n first reads slot (r, n-1) and leaves when it is <= stop_crit, so every launch behind a record's stop is a no-op for
 * that record), its own iteration count and largest residual, its own ping-pong parity, its own mask-bit words.
 * CONTRACT: for every record d_out, iters_out [nrec*nk] and resmax_out [nrec*nk] (host, record-major, may be NULL) are bit for bit
 * what fg_extrap_run_dev gives for that record alone -- the reference's do_extrapolate -- whatever the other records are, in
 * whatever order, for every value of fg_set_extrap_batch and fg_set_extrap_coef.  Host synchronisations per level:
 * ceil((max_r iters[r][k] + 1) / batch); fg_extrap_last_syncs reports their sum.  The handle's state grows on demand to nrec
 * records.  FG_ERR_ARG (handle still usable): nrec < 1, nk < 1, a null array, a stride smaller than a level or a record. */
int  fg_extrap_run_batch_dev(fg_extrap *h, int nrec, const double *d_in, double *d_out, int nk, long level_stride, long rec_stride,
                             double missing, double stop_crit, int *iters_out, double *resmax_out);
/* the four coefficient arrays [nj*ni] (host) as the handle uses them / without a handle or a device (cfw, cfe, cfs, cfn of :2710-2718) */
int  fg_extrap_get_coef(fg_extrap *h, double *cfw, double *cfe, double *cfs, double *cfn);
int  fg_extrap_coef_host(int ni, int nj, const double *lon, const double *lat, double *cfw, double *cfe, double *cfs, double *cfn);
/* Test / tuning hooks; results never depend on them.  batch: iterations queued per host synchronisation (default 64, < 1 = default).
 * coef: 0 (default) the kernel forms the four coefficients of a cell from three row and two column factors on every use,
 * 1 it reads them from a stored [nj*ni][4] table. */
void fg_set_extrap_batch(int n);
void fg_set_extrap_coef(int stored);
/* setup_vertical_interp: kstart, kend, need_interp of (z1[nk1] source levels, z2[nk2] destination levels); host only. */
int  fg_setup_vertical_interp(int nk1, const double *z1, int nk2, const double *z2, int *kstart, int *kend, int *need_interp);
/* do_vertical_interp of a field with a z axis: d_in [nk1][nxy] -> d_out [nk2][nxy] (device, different arrays; z1, z2 host).
 * Levels above z1[0] take the shallowest source level, levels below z1[nk1-1] the deepest, the others
 * (1.-w)*upper + w*lower.  need_interp == 0: d_out = d_in.  The reference's fatal checks ("grid1 not monotonic",
 * "grid2 lies outside grid1", ...) return FG_ERR_DATA with its message.  Synchronous. */
int  fg_dev_vertical_interp(long nxy, int nk1, const double *z1, int nk2, const double *z2, const double *d_in, double *d_out);

/* The column loop: `fregrid --extrapolate --dst_vgrid` (fregrid.c:1026-1043) for nrec records of one lat-lon source tile, streamed.
 *   plans     finalized conserve_order1 plans, one per destination tile, whose source grid is the extrapolator's ni x nj (same
 *             device); anything else FG_ERR_ARG
 *   z1 [nk1]  source levels, z2 [nk2] the --dst_vgrid levels; z2 = NULL: no --dst_vgrid, the output has nk1 levels.
 *             linear_vertical_interp's fatal checks return FG_ERR_DATA with the reference's message from fg_column_create.
 *   host_in   [nrec][nk1][nj][ni] in in_type; host_out[tile] [nrec][nk2][ny][nx] in out_type (FG_NC_SHORT / _INT / _FLOAT /
 *             _DOUBLE, as fg_sweep); iters_out, resmax_out [nrec*nk1] (host, may be NULL) as fg_extrap_run_batch_dev fills them
 * Per chunk of records, on the copy-in, compute and copy-out streams with fg_sweep's slots and events: typed upload; widening with
 * get_input_data's rule (scale, then offset, each skipped when 0, only where data != missing); fg_extrap_run_batch_dev; the plain
 * sweep of all records x nk1 planes through each plan (the fill cleared has_missing: no missing test); one kernel that forms
 * (1.-w)*a + w*b per destination level and stores it in out_type; typed download.  Every value carries the bits of the chain
 * fg_dev_widen, fg_extrap_run_dev per record, fg_plan_apply, fg_dev_vertical_interp, fg_dev_narrow.  The fill's wait for its slots
 * is the only host synchronisation inside a chunk; the upload of the next chunk is queued before it and the download of the
 * previous one runs beside it.  Records per chunk: fg_set_column_records(n) (test / tuning hook, returns the value in force,
 * 0 = default); < 1 restores the default -- as many as fit with all buffers in a quarter of the free device memory, at most 8.
 * Results never depend on it.  Streams and lifetimes as fg_sweep_run: plans and extrapolator are borrowed inside a run only. */
typedef struct fg_column fg_column;
int  fg_column_create(fg_extrap *ex, int nplans, fg_plan *const *plans, int in_type, int out_type,
                      int nk1, const double *z1, int nk2, const double *z2, fg_column **out);
int  fg_column_run(fg_column *c, const void *host_in, long nrec, double scale, double offset, double missing,
                   double stop_crit, void *const *host_out, int *iters_out, double *resmax_out);
void fg_column_destroy(fg_column *c);
int  fg_set_column_records(int n);

/* ---- runoff_regrid on the device (tools/runoff_regrid/runoff_regrid.c: setup_remap :430, process_data :626-675, nearest :708) ----
 * All angles in radians, as setup_remap receives them.  The exchange list is create_xgrid_1dx2d_order1's; the nearest ocean
 * point (mask_out != 0) of every land point (mask_out == 0) is the reference's, bit for bit: the first point in row-major order
 * among those with the smallest rounded distance() r, r < distance(0, pi/2, 0, -pi/2) strictly; imap = jmap = -1 on ocean
 * points and where no ocean point qualifies.  A mask_out without an ocean point is FG_ERR_ARG (the reference indexes with -1). */
typedef struct fg_runoff fg_runoff;
int  fg_runoff_create(int nx_in, int ny_in, const double *lonb_in, const double *latb_in, const double *mask_in,
                      int nx_out, int ny_out, const double *xc, const double *yc, const double *xt, const double *yt,
                      const double *mask_out, const double *area_out, int device, fg_runoff **out);
/* the same with a given exchange list (the analogue of fg_plan_set_xgrid); mask_in, area_in [ny_in*nx_in] serve the input total */
int  fg_runoff_create_from_xgrid(int nx_in, int ny_in, const double *mask_in, const double *area_in, int nx_out, int ny_out,
                                 const double *xt, const double *yt, const double *mask_out, const double *area_out,
                                 long nxgrid, const int *i_in, const int *j_in, const int *i_out, const int *j_out,
                                 const double *xgrid_area, int device, fg_runoff **out);
void fg_runoff_destroy(fg_runoff *h);
long fg_runoff_nxgrid(const fg_runoff *h);
int  fg_runoff_get_xgrid(const fg_runoff *h, int *i_in, int *j_in, int *i_out, int *j_out, double *xgrid_area);   /* any may be NULL */
int  fg_runoff_get_maps(const fg_runoff *h, int *imap, int *jmap);          /* [ny_out*nx_out] */
int  fg_runoff_get_xyz(fg_runoff *h, double *x, double *y, double *z);      /* distance()'s point triples [ny_out*nx_out] (tests) */
/* queries, tiles, tiles visited over all queries, most tiles visited by one query -- of the handle's search */
int  fg_runoff_search_stats(const fg_runoff *h, long *stats4);
/* wall time of the handle's setup in ms (the first n of 5): exchange list with the input areas (fg_runoff_create only), point
 * conversion, nearest search (compaction, balls, kernel, read-back), its kernel alone (events), host sorts and uploads */
int  fg_runoff_phase_ms(const fg_runoff *h, float *ms, int n);
void *fg_runoff_stream(fg_runoff *h);
/* One time level: remap sum in list order, runoff move (ascending land index onto the target's own value; a value <= 0 stays),
 * division by area_out.  totals (may be NULL): sum of in*area_in over mask_in > 0, sum of out*area_out, each summed by 1024
 * strided partial sums and a binary tree over them.  _dev: device pointers (different arrays), on the handle's stream; it
 * synchronises only when totals is given. */
int  fg_runoff_apply(fg_runoff *h, const double *in, double *out, double *totals);
int  fg_runoff_apply_dev(fg_runoff *h, const double *d_in, double *d_out, double *totals);
/* nearest() alone for the grid points qindex[nq] (row-major indices): host pointers, device FREGRID_HIP_DEVICE or 0 */
int  fg_nearest_unmasked(int nlon, int nlat, const double *mask, const double *lon, const double *lat, int nq,
                         const int *qindex, int *iout, int *jout);
/* Test hook; results never depend on it.  1 (default): tiles are skipped by their bounding balls; 0: every tile is visited. */
void fg_set_runoff_prune(int on);
int  fg_runoff_tile(void);                                                  /* compacted ocean points per tile */

/* ---- remap_land's nearest-point search on the device (tools/remap_land/remap_land.c:2520-2607) ----
 * All angles in radians.  Masks are int, non-zero = present, as the tool's *_count_* arrays are.  The answer for a destination
 * point is the reference's, bit for bit: the first source point in scan order (flat index l = face * npts_src + i) among those
 * with the smallest great_circle_distance as gcc -O2 and the host libm evaluate it.  The device finds the source points whose
 * chord to the query is within 2^-40 of the smallest; the host decides among them with the reference's expression; queries
 * that argument does not cover (nearest point more than a quarter turn away, first point at the antipode, coordinates outside
 * |lon| <= 8, |lat| <= the double pi/2 = 1.5707963267948966, where cos(lat) is still >= 0) take the reference's loop on the host.
 * fg_rland_create converts and orders the nface_src * npts_src source points once (device FREGRID_HIP_DEVICE or 0).
 * lon_dst / lat_dst may be host or device memory; every other array is the host's. */
typedef struct fg_rland fg_rland;
int  fg_rland_create(int nface_src, int npts_src, const double *lon_src, const double *lat_src, fg_rland **out);
void fg_rland_destroy(fg_rland *h);
void *fg_rland_stream(fg_rland *h);
/* full_search_nearest (:2520).  face: -1 all faces, else that face's points only.  idx_map = face_map = -1 where mask_dst == 0.
 * No unmasked source point while a destination point is unmasked: FG_ERR_ARG, "... no nearest point is found". */
int  fg_rland_search(fg_rland *h, const int *mask_src, int face, int npts_dst, const void *lon_dst, const void *lat_dst,
                     const int *mask_dst, int *idx_map, int *face_map);
/* search_nearest_sface (:2569): idx_map_sf = idx_map where face_map == iface_dst, else the nearest unmasked point of face
 * iface_dst, searched for those points only (the error above applies only if there is such a point); -1 where mask_dst == 0. */
int  fg_rland_search_sface(fg_rland *h, const int *mask_src, int npts_dst, const void *lon_dst, const void *lat_dst,
                           const int *mask_dst, const int *idx_map, const int *face_map, int iface_dst, int *idx_map_sf);
/* of the last search call (the first n of 8), in this order: [0] queries, [1] tiles, [2] tiles visited in phase 1 (smallest
 * chord) and [3] in phase 2 (survivors) over all queries, [4] survivors in all, [5] queries decided on the host among several
 * survivors, [6] queries that took the reference's loop, [7] queries with more survivors than the 4 slots (second launch,
 * exact size).  There are two visited counts, so [4]..[7] sit one place later than in a list with a single one. */
int  fg_rland_stats(const fg_rland *h, long *stats, int n);
/* wall time in ms (the first n of 8): create's conversion and ordering; of the last search call: the destination points'
 * copy and conversion, compaction with balls, phase 1 and phase 2 (events), overflow pass, host finish.  The handle's device
 * buffers only grow, so a search allocates nothing once the handle has seen its sizes. */
int  fg_rland_phase_ms(const fg_rland *h, float *ms, int n);
/* Test hook; results never depend on it.  1 (default): tiles are skipped by their bounding balls; 0: every tile is visited. */
void fg_set_rland_prune(int on);
int  fg_rland_tile(void);                                                   /* compacted source points per tile */

/* ---- river_regrid on the device (tools/river_regrid/river_regrid.c: calc_max_subA :694, calc_tocell :880, calc_river_data
 * :991, sort_basin :1298, check_river_data :1180) ----
 * The arrays are those get_source_data and get_mosaic_grid leave in river_type; reading the files, the land fractions from
 * the exchange grids and write_river_data are the caller's.  Every output carries the reference's bits.
 * Source: xb_r [nx_in+1], yb_r [ny_in+1] (radians), subA_in [ny_in*nx_in]; missing6: the missing values of subA, tocell, travel,
 * basin, cellarea, celllength as the file gives them (doubles).  Limits: subA's must fit an int (init_river_data keeps it in
 * one); those of tocell, travel and basin must be negative integers (the reference's sweeps take any value >= 0 for data).
 * Mosaic: ntiles tiles of nx[n] x ny[n] cells, all equal; opcode = 1 (x cyclic) | 2 (y cyclic) | 4 (cubic grid, 6 tiles); per
 * tile xb, yb [(ny+1)*(nx+1)] (radians), xt, yt [(ny+2)*(nx+2)] (degrees: interior given, the halo is filled here by
 * update_halo_double's rule, what that rule never writes stays as given), area [ny*nx], landfrac [ny*nx] (thresholded, in [0, 1]).
 * Errors of the reference come back as FG_ERR_ARG with its message text, never as an abort. */
typedef struct fg_river fg_river;
int  fg_river_create(int nx_in, int ny_in, const double *xb_r, const double *yb_r, const double *subA_in, const double *missing6,
                     int ntiles, const int *nx, const int *ny, int opcode, const double *const *xb, const double *const *yb,
                     const double *const *xt, const double *const *yt, const double *const *area, const double *const *landfrac,
                     double suba_cutoff, int device, fg_river **out);
void fg_river_destroy(fg_river *h);
void *fg_river_stream(fg_river *h);
/* all five stages; the handle may be run again */
int  fg_river_run(fg_river *h);
/* the interior [ny*nx] of a tile, as write_river_data copies it; any pointer may be NULL */
int  fg_river_get(const fg_river *h, int tile, double *subA, int *tocell, int *travel, int *basin, double *cellarea, double *celllength);
/* calc_max_subA's result with its halo [(ny+2)*(nx+2)], as calc_tocell reads it (tests) */
int  fg_river_get_max_suba(const fg_river *h, int tile, double *out);
/* of the last run (the first n of 7): [0] maximum travel, [1] maximum basin, [2] coast points that are full land, [3] sink
 * points (check_river_data's counts), [4] full-land cells (those the search runs for), [5] source cells the search visited,
 * [6] kernel launches */
int  fg_river_stats(const fg_river *h, long *stats, int n);
/* wall time in ms (the first n of 5): create; of the last run: max subA; tocell, outlets, travel and basin; accumulated subA;
 * sort_basin and check_river_data on the host */
int  fg_river_phase_ms(const fg_river *h, float *ms, int n);
/* Test hook; results never depend on it.  1 (default): only the adjust_lon calls that change the longitudes are replayed and
 * only the source cells between them that can overlap are visited; 0: every land cell walks every source cell in the
 * reference's order.  A source grid whose bounds do not ascend always takes the second path. */
void fg_set_river_prune(int on);
/* qsort_index (:1538) on the host: sorts array [n] ascending in place and carries index [n] along, with the reference's order
 * among equal values (sort_basin's ids depend on it) */
int  fg_river_qsort_index(double *array, int n, int *index);

/* ---- make_topog --topog_type realistic on the device (tools/make_topog/topog.c: create_realistic_topog :355, process_topo :551,
 * filter_topo :687, remove_isolated_cells :830, restrict_partial_cells :878, show_deepest :945, enforce_min_depth :987) ----
 * The arrays are those the tool reads from the topography file, the vertical grid and the model grid; the tool's netCDF and
 * mosaic handling, its domain decomposition and the idealised topographies are the caller's.  The depth stays in device memory
 * from the remap to the last adjustment and carries the reference's bits; with use_great_circle_algorithm the
 * remap agrees to rounding, as the great-circle plans do.  Errors of the reference come back as FG_ERR_ARG with its message
 * text, never as an abort.  A source too large for one plan is the plan's error. */
typedef struct fg_topog fg_topog;
typedef struct fg_topog_opts {          /* every switch create_realistic_topog takes, in its order */
  double scale_factor;
  int tripolar_grid, cyclic_x, cyclic_y, fill_first_row, filter_topog, num_filter_pass, smooth_topo_allow_deepening;
  int round_shallow, fill_shallow, deepen_shallow, full_cell, flat_bottom, adjust_topo, fill_isolated_cells, dont_change_landmask;
  int kmt_min;
  double min_thickness;
  int open_very_this_cell;
  double fraction_full_cell;
  int use_great_circle_algorithm, on_grid;
} fg_topog_opts;
/* make_topog.c:297-323: scale_factor 1, num_filter_pass 1, adjust_topo 1, fill_isolated_cells 1, kmt_min 2, min_thickness 0.1,
 * open_very_this_cell 1, fraction_full_cell 0.2, everything else 0 */
void fg_topog_default_opts(fg_topog_opts *opts);
/* x_dst, y_dst [(ny_dst+1)*(nx_dst+1)]: the model grid's corners in DEGREES, as the tool holds them.  opts NULL: the defaults. */
int  fg_topog_create(int nx_dst, int ny_dst, const double *x_dst, const double *y_dst, const fg_topog_opts *opts, int device, fg_topog **out);
void fg_topog_destroy(fg_topog *h);
void *fg_topog_stream(fg_topog *h);
/* xt_src [nx_src], yt_src [ny_src]: the cell-centre axes of the file in degrees; data [ny_src*nx_src] in the file's type, dtype the
 * nc_type code 4 (NC_INT, int32), 5 (NC_FLOAT) or 6 (NC_DOUBLE); missing: the file's missing_value.  Forms the bounds (:416-427),
 * trims the rows to the model grid's latitudes (:437-449), uploads those rows in their narrow type, and on the device widens,
 * masks and scales them (:492-502; `missing` is tested before scaling, <= 0 after it is masked) and expands the two axes to the
 * corner arrays.  May be called again: the new source replaces the old one.  on_grid: the trimmed source must have nx_dst*ny_dst cells. */
int  fg_topog_set_source(fg_topog *h, int nx_src, int ny_src, const double *xt_src, const double *yt_src, const void *data, int dtype, double missing);
/* what set_source left on the device (tests): x_src, y_src [(ny_now+1)*(nx_src+1)] radians, depth_src, mask_src [ny_now*nx_src],
 * ny_now = jend - jstart + 1 (fg_topog_stats); any pointer may be NULL */
int  fg_topog_get_source(const fg_topog *h, double *x_src, double *y_src, double *depth_src, double *mask_src);
/* The stages, each leaving its result on the device.  remap: conserve_interp / conserve_interp_great_circle (interp.c:262-356), or
 * with on_grid the copy of :503-511 (only `missing` becomes 0, negative scaled values are kept).  filter: filter_topo, whatever
 * opts.filter_topog says.  process: process_topo with nk levels zw [nk].  run: :512-536, i.e. remap, filter if filter_topog, the
 * deepest depth, fill_first_row, process if nk > 0 (nk == 0: no vertical grid, no levels).  zw is checked where the stage begins
 * (the reference finds a non-monotone zw at the first ocean cell, and nk < kmt_min in enforce_min_depth). */
int  fg_topog_remap(fg_topog *h);
int  fg_topog_filter(fg_topog *h);
int  fg_topog_process(fg_topog *h, int nk, const double *zw);
int  fg_topog_run(fg_topog *h, int nk, const double *zw);
/* Test hook: overwrites the device depth [ny_dst*nx_dst], so that a stage can be fed the reference's intermediate. */
int  fg_topog_set_depth(fg_topog *h, const double *depth);
/* depth [ny_dst*nx_dst], num_levels [ny_dst*nx_dst] (after process; NULL to skip) */
int  fg_topog_get(const fg_topog *h, double *depth, int *num_levels);
/* the first n of 9: [0] jstart, [1] jend, [2] nxgrid of the last remap (0 for on_grid), [3] isolated cells filled, [4] partial
 * cells restricted, [5] shallow cells modified (the counts the reference prints under debug), [6] show_deepest's verdict: 0 the
 * topography is deeper than the grid by more than 1 m, 1 fewer levels would do, 2 the grid fits, -1 no vertical grid was given,
 * [7] launches of the isolated-cell sweep, [8] ny_now.  *deepest (may be NULL): the deepest non-zero depth after the filter stage. */
int  fg_topog_stats(const fg_topog *h, long *stats, double *deepest, int n);
/* wall time in ms (the first n of 5): create; set_source; remap; filter; process */
int  fg_topog_phase_ms(const fg_topog *h, float *ms, int n);
/* Test hook; results never depend on it (the sweep's result does not depend on its order, for depths without
 * NaN).  1 (default): remove_isolated_cells is evaluated for every cell at once on the arrays process_topo left, inside the last
 * kernel; 0: it runs as the reference's in-place sweep, one launch per anti-diagonal 2j + i. */
void fg_set_topog_sweep(int fused);
/* out_dev [ncells_out] = conserve_interp's area-fraction sweep (interp.c:283-294) of data_dev [ncells_in] over a finalized
 * first-order plan; device pointers, queued on the plan's stream and waited for */
int  fg_plan_apply_frac_dev(fg_plan *plan, const double *data_dev, double *out_dev);

/* ---- make_coupler_mosaic's exchange grids on the device (tools/make_coupler_mosaic/make_coupler_mosaic.c:1198-2127, :2466-2811;
 * DESIGN.md 3.13): atmosphere x land, atmosphere x ocean and land x ocean lists, the per-cell area and centroid sums, the centroid
 * distances of an order-2 exchange-grid file and the land and ocean masks.  Legacy clip, one process, one ocean tile, a nested
 * atmosphere tile (fg_coupler_set_nest), a wave grid (fg_coupler_add_wave), --check's sums (fg_coupler_check), any number of atmosphere tiles, land on the atmosphere grid (lnd_same_as_atm) or as tiles of its own.  The lists and
 * every clipped polygon stay in device memory between the searches; fg_coupler_run brings counts and error words to the host.
 *
 * fg_coupler_create: corner arrays in radians, [ny+1][nx+1] per tile (host).  ntile_lnd = 0: land is on the atmosphere grid and
 * the land arguments are ignored.  The ocean grid and omask [nyo][nxo] (ocean fraction in [0, 1]) are what the tool works on, i.e.
 * with the row down to -90 degrees already added (coupler.coupler_ocean_grid; :841-876); ocn_south_ext = the rows added (0 or 1):
 * they are left out of nbad.  area_ratio_thresh >= 1e-6 (the tool's default; the searches accept pairs at that ratio).
 * fg_coupler_run may be called again.  Errors: FG_ERR_ARG / FG_ERR_GEOM with the reference's message, never an abort. */
typedef struct fg_coupler fg_coupler;
int  fg_coupler_create(int interp_order, double area_ratio_thresh, int ntile_atm, const int *nx_atm, const int *ny_atm,
                       const double *const *lon_atm, const double *const *lat_atm, int ntile_lnd, const int *nx_lnd, const int *ny_lnd,
                       const double *const *lon_lnd, const double *const *lat_lnd, int nx_ocn, int ny_ocn, const double *lon_ocn,
                       const double *lat_ocn, const double *omask, int ocn_south_ext, int device, fg_coupler **out);
/* The tool's GREAT_CIRCLE_CLIP branch (:587-594, taken when the atmosphere grid carries great_circle_algorithm: a pole inside a
 * cell): the argument list of fg_coupler_create; interp_order must be 1 (:593), anything else is FG_ERR_ARG.  The corners go up as
 * lon / lat and become unit vectors on the device (fg_dev_latlon2xyz: the reference's latlon2xyz bits); cell areas are
 * get_grid_great_circle_area's; every clip is clip_2dx2d_great_circle, every area great_circle_area; the remembered atmosphere x
 * land polygons are searched against the ocean by fg_plan_create_polylist_gc's device twin.  The reference clips every pair of
 * cells in this branch; here the searches prune by bounding caps.  Every other fg_coupler_* entry works on such a
 * handle as on an order-1 legacy handle. */
int  fg_coupler_create_gc(int interp_order, double area_ratio_thresh, int ntile_atm, const int *nx_atm, const int *ny_atm,
                          const double *const *lon_atm, const double *const *lat_atm, int ntile_lnd, const int *nx_lnd, const int *ny_lnd,
                          const double *const *lon_lnd, const double *const *lat_lnd, int nx_ocn, int ny_ocn, const double *lon_ocn,
                          const double *lat_ocn, const double *omask, int ocn_south_ext, int device, fg_coupler **out);
void fg_coupler_destroy(fg_coupler *h);
void *fg_coupler_stream(fg_coupler *h);
/* A nested atmosphere tile (make_coupler_mosaic.c:1765, :1792, :1857, :1903), named before fg_coupler_run: an index into the
 * atmosphere tiles, -1 for none.  Its three lists and its own per-cell area sums are formed as any tile's; its terms
 * are left out of the land and ocean cells' sums, hence out of the land and ocean masks, nbad and every list's tile-2 distances.
 * At interp_order 2 the reference's guards also enclose its temporary a_area / a_clon / a_clat (:1882-1885, :1927-1930): the nest
 * lists' tile-1 distances are clon / area - 0, and fg_coupler_get_cells gives clon = clat = 0 on the nest tile; its xarea is the full
 * sum (atm_xarea of :2210 / :2333, which has no guard).
 * FG_ERR_ARG with land on the atmosphere grid (:742) and for an index out of range.  Legacy and great-circle handles. */
int  fg_coupler_set_nest(fg_coupler *h, int tile_nest);
/* The wave grid (:2976-3535), given before fg_coupler_run: corner arrays as fg_coupler_create's.  The wave x ocean list is the land x
 * ocean step with a wave tile for the land tile (ocn_frac > 1e-4, area x ocn_frac / min(area_ocn, area_wav) > thresh), inside the
 * tile's ocean row band of :3107-3117; list order: wave tile, wave cell, ocean cell.  wav_same_as_ocn changes nothing with one ocean
 * tile (:3119-3126) but fg_coupler_write_wave's file names.  interp_order 1: the reference's sum (:3262-3267) adds into w_area2,
 * which is never allocated; w_area is formed as the order-2 branch forms it and nothing else.  FG_ERR_ARG on a great-circle handle
 * (first order only: nothing of the wave sums could be pinned). */
int  fg_coupler_add_wave(fg_coupler *h, int ntile_wav, const int *nx, const int *ny, const double *const *lon, const double *const *lat,
                         int wav_same_as_ocn);
int  fg_coupler_run(fg_coupler *h);
/* which: 0 atmosphere x land (tile1 = atmosphere tile, tile2 = land tile), 1 atmosphere x ocean (tile1 = atmosphere tile, tile2 = 0),
 * 2 land x ocean (tile1 = land tile, tile2 = 0; land of its own only), 3 wave x ocean (tile1 = wave tile, tile2 = 0).  The list's
 * length, or FG_ERR_*. */
long fg_coupler_count(const fg_coupler *h, int which, int tile1, int tile2);
/* The list in the reference's order, host arrays of fg_coupler_count entries, any may be NULL: 0-based (i, j) of the two cells,
 * the exchange-cell area, the centroid integrals clon / clat and the distances tile1_distance (di1, dj1) and tile2_distance
 * (di2, dj2) of :1957-2006, :2778-2800 (interp_order 2 only). */
int  fg_coupler_get(const fg_coupler *h, int which, int tile1, int tile2, int *i1, int *j1, int *i2, int *j2, double *area,
                    double *clon, double *clat, double *di1, double *dj1, double *di2, double *dj2);
/* Per cell of one tile (grid: 0 atmosphere, 1 land, 2 ocean, 3 wave: w_area and the wave mask w_area / area_wav of :3397-3402), host arrays, any may be NULL: get_grid_area; the exchange area the
 * cell collected from the atmosphere's lists (a_area, l_area, o_area); their ratio (the land mask of :2089, the ocean fraction of
 * :2037, rows of the southern extension included); the cell's centroid (interp_order 2; the plain sums where the area is not > 0) */
int  fg_coupler_get_cells(const fg_coupler *h, int grid, int tile, double *model_area, double *xarea, double *frac, double *clon,
                          double *clat);
/* The ocean cells' wave-side sums (:3329-3332, :3366-3371; interp_order 2): exchange area and centroid per ocean cell from the wave x
 * ocean lists over all wave tiles.  They are never mixed into the atmosphere-side o_area of fg_coupler_get_cells. */
int  fg_coupler_get_wave_ocean(const fg_coupler *h, double *xarea, double *clon, double *clat);
/* --check (:2199-2219, :2326-2342, :3504, :3591-3661), the first n of 19 doubles: [0] the largest |atm_xarea - area_atm| / area_atm,
 * [1] its tile, [2] i, [3] j (0-based; the first cell with that ratio), [4] area_atm and [5] atm_xarea there, [6] atm_area_sum,
 * [7] axl_area_sum, [8] axo_area_sum, [9] the ocean and [10] the land percentage, [11] the tiling error in percent, [12 .. 17] the
 * same six of the nest tile (0 without one), [18] wxo_area_sum (0 without a wave grid).  The ratio and its cell are one device
 * reduction; the scalar sums are added on the host from the downloaded area columns in the reference's order (atmosphere tile, land
 * tile, list order; then per atmosphere tile the ocean list).  fg_coupler_run copies nothing more for it. */
int  fg_coupler_check(const fg_coupler *h, double *out, int n);
/* The tool's output files into `directory` (which exists), classic netCDF: one exchange-grid file per non-empty list
 * (<atm mosaic>_<tile>X<lnd mosaic>_<tile>.nc, ...X<ocn mosaic>_<tile>.nc, <lnd mosaic>_<tile>X<ocn mosaic>_<tile>.nc) with contact,
 * tile1_cell, tile2_cell (1-based; an ocean j carries 1 - ocn_south_ext), xgrid_area and for interp_order 2 tile1_distance and
 * tile2_distance, attributes as make_coupler_mosaic.c:2158-2182; ocean_mask.nc (mask, areaO, areaX, without the added southern
 * row) and land_mask.nc or land_mask_tile<k>.nc (mask, area_lnd, l_area, and area_atm when land is on the atmosphere grid).
 * names: NULL, or a table of [0] atmosphere, [1] land, [2] ocean mosaic name, then the atmosphere tiles' names, the land tiles'
 * names (one per land tile of the handle) and the ocean tile's name; NULL entries give "atmos_mosaic", "land_mosaic",
 * "ocean_mosaic", "tile<k>".  The coupler mosaic file that lists these files and the provenance attributes are not written. */
int  fg_coupler_write(const fg_coupler *h, const char *directory, const char *const *names);
/* The two kinds of file from host arrays, for lists a caller holds itself (fg_coupler_write goes through them).  An exchange-grid
 * file: n >= 1 cells, 0-based (i, j) of the two grids written as i + 1, j1 + 1, j2 + j2_shift; di1 .. dj2 all given (tile1_distance,
 * tile2_distance and the order-2 attributes) or all NULL.  A mask file [ny][nx]: ocean != 0: mask, areaO = a, areaX = b; else mask,
 * area_lnd = a, l_area = b and area_atm when given. */
int  fg_coupler_write_xgrid(const char *path, const char *contact, long n, const int *i1, const int *j1, const int *i2, const int *j2,
                            int j2_shift, const double *area, const double *di1, const double *dj1, const double *di2, const double *dj2);
int  fg_coupler_write_mask(const char *path, int ocean, int nx, int ny, const double *mask, const double *a, const double *b,
                           const double *area_atm);
/* The wave grid's files (:3397-3421, :3430-3535): per non-empty list <wave mosaic>_<tile>X<ocn mosaic>_<tile>.nc -- or, with
 * wav_same_as_ocn, wav_<wave mosaic>_<tile>Xocn_<ocn mosaic>_<tile>.nc (:3452-3455) -- with contact w:tile::o:tile and the variables of
 * the other exchange-grid files (tile2_cell's j = jo + 1 - ocn_south_ext), and wave_mask.nc or wave_mask_tile<k>.nc with the single
 * variable mask.  names: NULL, or [0] wave, [1] ocean mosaic name, the wave tiles' names, the ocean tile's name; NULL entries give
 * "wave_mosaic", "ocean_mosaic", "tile<k>".  fg_coupler_write's table is a different one.  _wave_xgrid / _wave_mask: from host arrays. */
int  fg_coupler_write_wave(const fg_coupler *h, const char *directory, const char *const *names);
int  fg_coupler_write_wave_xgrid(const char *path, const char *contact, long n, const int *iw, const int *jw, const int *io, const int *jo,
                                 int jo_shift, const double *area, const double *diw, const double *djw, const double *dio, const double *djo);
int  fg_coupler_write_wave_mask(const char *path, int nx, int ny, const double *mask);
/* the first n of 9: [0] bytes fg_coupler_run copied to the host, [1] nbad: ocean cells with |omask - ocn_frac| > 1e-4 (:2038),
 * [2] searches, [3] atmosphere x ocean cells, [4] atmosphere x land cells, [5] land x ocean cells, [6] remembered atmosphere x land
 * polygons, [7] ocn_south_ext, [8] wave x ocean cells */
int  fg_coupler_stats(const fg_coupler *h, long *stats, int n);
/* wall time in ms (the first n of 8): create; atmosphere x land candidates; atmosphere x ocean; polygons x ocean; land x ocean;
 * sums, distances and masks; the whole run; wave x ocean */
int  fg_coupler_phase_ms(const fg_coupler *h, float *ms, int n);

#ifdef __cplusplus
}
#endif
#endif /* FREGRID_HIP_H_ */
