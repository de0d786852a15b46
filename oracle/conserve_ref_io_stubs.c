/* oracle/conserve_ref_io_stubs.c -- TEST INFRASTRUCTURE ONLY, linked into oracle/_ref/libconserve_ref.so and
 * oracle/_ref/libbilinear_ref.so.
 *
 * The reference's conserve_interp.c calls twelve I/O routines (mpp_io.c, read_mosaic.c), and only from its READ and WRITE
 * remap-file branches; its bilinear_interp.c calls eight of them and mpp_get_dimlen, likewise only from READ and WRITE.  Those need libnetcdf, which this build does not have.  These definitions satisfy the linker; each
 * one stops the process through the reference's own mpp_error, so a caller that reaches a remap-file branch dies loudly
 * instead of reading garbage.  oracle/conserve_ref_adapter.c and oracle/bilinear_ref_adapter.c never set READ or WRITE in the opcode they pass on. */
#include <stddef.h>
#include "mpp.h"
#include "mpp_io.h"
#include "read_mosaic.h"

#define CREF_NO_IO(name) mpp_error("oracle build: " name " is not available")

int mpp_open(const char *file, int action) { (void)file; (void)action; CREF_NO_IO("mpp_open"); return -1; }
void mpp_close(int ncid) { (void)ncid; CREF_NO_IO("mpp_close"); }
int mpp_get_dimlen(int fid, const char *name) { (void)fid; (void)name; CREF_NO_IO("mpp_get_dimlen"); return -1; }
int mpp_get_varid(int fid, const char *varname) { (void)fid; (void)varname; CREF_NO_IO("mpp_get_varid"); return -1; }
void mpp_get_var_value(int fid, int vid, void *data) { (void)fid; (void)vid; (void)data; CREF_NO_IO("mpp_get_var_value"); }
int mpp_def_dim(int fid, const char *name, int size) { (void)fid; (void)name; (void)size; CREF_NO_IO("mpp_def_dim"); return -1; }
int mpp_def_var(int fid, const char *name, nc_type type, int ndim, const int *dims, int natts, ...)
{
  (void)fid; (void)name; (void)type; (void)ndim; (void)dims; (void)natts;
  CREF_NO_IO("mpp_def_var");
  return -1;
}
void mpp_end_def(int fid) { (void)fid; CREF_NO_IO("mpp_end_def"); }
void mpp_put_var_value(int fid, int vid, const void *data) { (void)fid; (void)vid; (void)data; CREF_NO_IO("mpp_put_var_value"); }
void mpp_put_var_value_block(int fid, int vid, const size_t *start, const size_t *nread, const void *data)
{
  (void)fid; (void)vid; (void)start; (void)nread; (void)data;
  CREF_NO_IO("mpp_put_var_value_block");
}
int read_mosaic_xgrid_size(const char *xgrid_file) { (void)xgrid_file; CREF_NO_IO("read_mosaic_xgrid_size"); return -1; }
void read_mosaic_xgrid_order1(const char *xgrid_file, int *i1, int *j1, int *i2, int *j2, double *area)
{
  (void)xgrid_file; (void)i1; (void)j1; (void)i2; (void)j2; (void)area;
  CREF_NO_IO("read_mosaic_xgrid_order1");
}
void read_mosaic_xgrid_order2(const char *xgrid_file, int *i1, int *j1, int *i2, int *j2, double *area, double *di, double *dj)
{
  (void)xgrid_file; (void)i1; (void)j1; (void)i2; (void)j2; (void)area; (void)di; (void)dj;
  CREF_NO_IO("read_mosaic_xgrid_order2");
}
