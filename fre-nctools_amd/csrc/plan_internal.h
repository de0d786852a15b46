// plan_internal.h -- entries of plan.hip for the library's own pipelines (coupler.hip, topog.hip): not exported in fregrid_hip.h.  They let a
// pipeline keep the exchange cells, the clipped polygons and the grids of its searches in device memory from one search to the next.
#pragma once
#include "fregrid_hip.h"

// where a searched plan keeps its results (device pointers, the plan's for as long as it lives); c1 / c2 null for order 1 and
// still the un-normalised centroid integrals before fg_plan_finalize
struct FgPlanView {
  long nx;                         // exchange cells, in canonical order
  int nsrc, ndst;
  const int *x_src, *x_dst;        // flattened source cell (tiles back to back; a polygon list: the polygon) and destination cell
  const double *x_area, *x_c1, *x_c2;
  const double *src_area;          // [nsrc] get_grid_area of the source cells (a polygon list: the caller's area_ref)
  const double *src_lon_avg;       // [nsrc] mean longitude after fix_lon(pi) (a polygon list: the caller's lon_avg)
};
int fg_plan_view(const fg_plan *pl, FgPlanView *v);
// the clipped polygon of every exchange cell into device arrays n_out [nx], lon / lat [nx][8]; queued on the plan's stream
int fg_plan_polygons_dev(const fg_plan *pl, int *n_out, double *lon, double *lat);
// the same of a great-circle plan between grids: n_out [nx], x / y / z [nx][8]; queued on the plan's stream, which the call also
// synchronises (its scratch goes back to the pool).  A polygon of more than 8 vertices keeps its count
int fg_plan_polygons_gc_dev(const fg_plan *pl, int *n_out, double *x, double *y, double *z);
// A pipeline that made its own stream, ran plans on it and is about to destroy it calls this after synchronising the stream: the
// pool's blocks that are tagged with the stream become untagged and the events recorded on it leave the pool (dev_pool.h: retire).
void fg_pool_retire_stream(void *stream);
// ordering events the pool holds at the moment (C linkage: tests/test_gpu_coupler_stream_retire.py)
extern "C" long fg_pool_live_events(void);
// bytes the plan's search copied to the host (one block of counters per attempt)
long fg_plan_search_d2h(const fg_plan *pl);
// the plan's own block list: the pool's class size of every device block the plan holds into sizes [nmax] (may be null), their sum
// returned (C linkage: tests/test_gpu_stream_ordered_plans.py derives its footprint allowance from it)
extern "C" long fg_plan_device_bytes(const fg_plan *pl, long *sizes, int nmax);
// mean cell extents and the rectilinear hint of a destination grid from its host corner arrays, as fg_plan_create derives them
void fg_dst_extents(int nx, int ny, const double *lon, const double *lat, double *dlat, double *dlon, int *rect_hint);
// frame >= 0: the searches this thread starts use that longitude frame (fg_set_search_frame's values) whatever the process-wide
// switch says; -1: back to the switch.  Returns the previous override.
int fg_search_frame_override(int frame);
// fg_plan_create_dev on the caller's stream with the extents and hint of fg_dst_extents: no sample of the grid is read back
long fg_plan_create_dev_hint(int order, int ntiles_in, const int *nx_in, const int *ny_in, const double *const *d_lon_in,
                             const double *const *d_lat_in, int nx_out, int ny_out, const double *d_lon_out, const double *d_lat_out,
                             double mean_dlat, double mean_dlon, int rect_hint, int device, void *stream, fg_plan **plan_out);
// fg_plan_create_polylist with the list already on the device
long fg_plan_create_polylist_dev(int order, int npoly, const int *d_n, const double *d_lon, const double *d_lat, const double *d_lon_avg,
                                 const double *d_area_ref, int nx_out, int ny_out, const double *d_lon_out, const double *d_lat_out,
                                 double mean_dlat, double mean_dlon, int rect_hint, int device, void *stream, fg_plan **plan_out);
// fg_plan_create_polylist_gc with the list (n [npoly], x / y / z [npoly][8], area_ref [npoly]) and the destination's unit vectors
// already on the device (stream / use_caller_stream as fg_plan_create_great_circle_dev); extents <= 0: derived from a sample of the
// destination.  A polygon of more than 8 vertices is FG_ERR_MAXV (found by the record kernel)
extern "C" long fg_plan_create_polylist_gc_dev(int npoly, const int *d_n, const double *d_x, const double *d_y, const double *d_z,
                                               const double *d_area_ref, int nx_out, int ny_out, const double *d_x_out, const double *d_y_out,
                                               const double *d_z_out, double mean_dlat, double mean_dlon, int device, void *stream,
                                               int use_caller_stream, fg_plan **plan_out);
