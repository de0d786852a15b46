// plan_internal.h -- entries of plan.hip for the library's own pipelines (coupler.hip): not exported in fregrid_hip.h.  They let a
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
