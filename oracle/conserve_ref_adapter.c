/* oracle/conserve_ref_adapter.c -- TEST INFRASTRUCTURE ONLY, linked into oracle/_ref/libconserve_ref.so.
 *
 * Flat-array entry points over the reference's own setup_conserve_interp and do_scalar_conserve_interp (its
 * tools/fregrid/conserve_interp.c, compiled in place by oracle/Makefile), so tests/orc.py can drive them through ctypes.
 * The adapter fills the reference's Grid_config / Interp_config / Field_config / Var_config (tools/libfrencutils/globals.h)
 * the way fregrid.c does for one process, calls the reference, copies the results out and frees what it allocated.
 *
 * Only the compute branches run: the opcode passed on never holds READ or WRITE (the remap-file I/O behind them is stubbed in
 * oracle/conserve_ref_io_stubs.c).  The reference's fatal checks call mpp_error, which exits the process: a caller that
 * may reach one runs the adapter in a child process. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "globals.h"
#include "create_xgrid.h"
#include "conserve_interp.h"
#include "mpp.h"
#include "mpp_domain.h"

static int cref_ready = 0;

void cref_init(void)
{
  if (cref_ready) return;
  mpp_init(NULL, NULL);
  mpp_domain_init();
  cref_ready = 1;
}

/* The reference prints its notes and the CHECK_CONSERVE sums with printf.  While a capture is open, file descriptor 1 points
 * at a temporary file; capture_end copies what was printed into msg (NUL-terminated, truncated to msglen - 1 bytes). */
typedef struct { int saved; FILE *tmp; } Capture;

static Capture capture_begin(void)
{
  Capture c = {-1, NULL};
  fflush(stdout);
  c.tmp = tmpfile();
  if (!c.tmp) return c;
  c.saved = dup(1);
  dup2(fileno(c.tmp), 1);
  return c;
}

static void capture_end(Capture c, char *msg, int msglen)
{
  if (!c.tmp) { if (msg && msglen > 0) msg[0] = 0; return; }
  fflush(stdout);
  dup2(c.saved, 1);
  close(c.saved);
  if (msg && msglen > 0) {
    rewind(c.tmp);
    size_t n = fread(msg, 1, (size_t)msglen - 1, c.tmp);
    msg[n] = 0;
  }
  fclose(c.tmp);
}

/* fregrid_util.c:get_input_output_cell_area for a grid without halo */
static void cell_area(unsigned int opcode, int nx, int ny, const double *lon, const double *lat, double *area)
{
  if (opcode & GREAT_CIRCLE) get_grid_great_circle_area(&nx, &ny, lon, lat, area);
  else get_grid_area(&nx, &ny, lon, lat, area);
}

/* setup_conserve_interp's compute branch.  opcode: CONSERVE_ORDER1 or CONSERVE_ORDER2, optionally | GREAT_CIRCLE (other bits
 * are dropped).  Corners lonc/latc [(ny+1)*(nx+1)] radians per tile.  Outputs: the exchange cells of every destination tile
 * back to back, xoff[n]..xoff[n+1] being tile n's (xoff has ntiles_out+1 entries); di/dj only for order 2 (may be NULL
 * otherwise); cell_area_in / cell_area_out per tile, as the reference's caller fills them.  Returns the total count, or -1
 * when it exceeds capacity (nothing is copied then).  The reference leaks its per-source-cell sums for first order
 * (conserve_interp.c frees them only in the second-order branch); that cannot be helped from here. */
long cref_setup(unsigned int opcode, int ntiles_in, const int *nx_in, const int *ny_in,
                const double *const *lonc_in, const double *const *latc_in,
                int ntiles_out, const int *nx_out, const int *ny_out,
                const double *const *lonc_out, const double *const *latc_out,
                long capacity, long *xoff, int *t_in, int *i_in, int *j_in, int *i_out, int *j_out,
                double *area, double *di, double *dj, double *const *cell_area_in, double *const *cell_area_out)
{
  cref_init();
  opcode &= (CONSERVE_ORDER1 | CONSERVE_ORDER2 | GREAT_CIRCLE);
  Grid_config *gin = (Grid_config *)calloc(ntiles_in, sizeof(Grid_config));
  Grid_config *gout = (Grid_config *)calloc(ntiles_out, sizeof(Grid_config));
  Interp_config *interp = (Interp_config *)calloc(ntiles_out, sizeof(Interp_config));
  for (int m = 0; m < ntiles_in; m++) {
    gin[m].nx = gin[m].nxc = nx_in[m];
    gin[m].ny = gin[m].nyc = ny_in[m];
    gin[m].lonc = (double *)lonc_in[m];
    gin[m].latc = (double *)latc_in[m];
    gin[m].cell_area = cell_area_in[m];
    cell_area(opcode, nx_in[m], ny_in[m], lonc_in[m], latc_in[m], cell_area_in[m]);
  }
  for (int n = 0; n < ntiles_out; n++) {
    gout[n].nx = gout[n].nxc = nx_out[n];
    gout[n].ny = gout[n].nyc = ny_out[n];
    gout[n].iec = nx_out[n] - 1;
    gout[n].jec = ny_out[n] - 1;
    gout[n].lonc = (double *)lonc_out[n];
    gout[n].latc = (double *)latc_out[n];
    gout[n].cell_area = cell_area_out[n];
    cell_area(opcode, nx_out[n], ny_out[n], lonc_out[n], latc_out[n], cell_area_out[n]);
  }

  Capture c = capture_begin();
  setup_conserve_interp(ntiles_in, gin, ntiles_out, gout, interp, opcode);
  capture_end(c, NULL, 0);

  long total = 0;
  for (int n = 0; n < ntiles_out; n++) total += (long)interp[n].nxgrid;
  if (total <= capacity) {
    long off = 0;
    for (int n = 0; n < ntiles_out; n++) {
      long k = (long)interp[n].nxgrid;
      xoff[n] = off;
      if (k > 0) {
        memcpy(t_in + off, interp[n].t_in, k * sizeof(int));
        memcpy(i_in + off, interp[n].i_in, k * sizeof(int));
        memcpy(j_in + off, interp[n].j_in, k * sizeof(int));
        memcpy(i_out + off, interp[n].i_out, k * sizeof(int));
        memcpy(j_out + off, interp[n].j_out, k * sizeof(int));
        memcpy(area + off, interp[n].area, k * sizeof(double));
        if ((opcode & CONSERVE_ORDER2) && di && dj) {
          memcpy(di + off, interp[n].di_in, k * sizeof(double));
          memcpy(dj + off, interp[n].dj_in, k * sizeof(double));
        }
      }
      off += k;
    }
    xoff[ntiles_out] = off;
  } else
    total = -1;

  for (int n = 0; n < ntiles_out; n++) {
    if (interp[n].nxgrid == 0) continue;          /* the reference allocates a tile's lists with its first cells */
    free(interp[n].t_in); free(interp[n].i_in); free(interp[n].j_in);
    free(interp[n].i_out); free(interp[n].j_out); free(interp[n].area);
    if (opcode & CONSERVE_ORDER2) { free(interp[n].di_in); free(interp[n].dj_in); }
  }
  free(interp); free(gout); free(gin);
  return total;
}

/* do_scalar_conserve_interp with every option, for one variable.  The exchange cells come back as cref_setup gave them
 * (concatenated, xoff).  Per source tile: data [nz][ny(+2)][nx(+2)] (halo 1 for order 2), grad_x / grad_y [nz][ny][nx] and
 * grad_mask [ny][nx] for order 2, weight [ny][nx] (NULL: no weight field), field_area [ny][nx] (read when cell_measures).
 * cell_area_in / cell_area_out as cref_setup returned them.  opcode: TARGET, MONOTONIC and CHECK_CONSERVE are passed on.
 * out[n]: [nz][ny_out][nx_out] per destination tile.  msg (may be NULL) receives what the reference printed.  Returns 0;
 * a fatal data check ends the process instead. */
int cref_apply(unsigned int opcode, int order, int nz,
               int ntiles_in, const int *nx_in, const int *ny_in, const double *const *cell_area_in,
               int ntiles_out, const int *nx_out, const int *ny_out, const double *const *cell_area_out,
               const long *xoff, const int *t_in, const int *i_in, const int *j_in, const int *i_out, const int *j_out,
               const double *area, const double *di, const double *dj,
               const double *const *data, const double *const *grad_x, const double *const *grad_y,
               const int *const *grad_mask, int has_missing, double missing, const double *const *weight,
               int cell_methods, int cell_measures, const double *const *field_area, double area_missing, int use_volume,
               double *const *out, char *msg, int msglen)
{
  cref_init();
  opcode &= (TARGET | MONOTONIC | CHECK_CONSERVE);
  opcode |= (order == 2) ? CONSERVE_ORDER2 : CONSERVE_ORDER1;
  Grid_config *gin = (Grid_config *)calloc(ntiles_in, sizeof(Grid_config));
  Grid_config *gout = (Grid_config *)calloc(ntiles_out, sizeof(Grid_config));
  Interp_config *interp = (Interp_config *)calloc(ntiles_out, sizeof(Interp_config));
  Field_config *fin = (Field_config *)calloc(ntiles_in, sizeof(Field_config));
  Field_config *fout = (Field_config *)calloc(ntiles_out, sizeof(Field_config));
  Var_config *var = (Var_config *)calloc(1, sizeof(Var_config));

  strcpy(var->name, "cref");
  var->interp_method = (order == 2) ? CONSERVE_ORDER2 : CONSERVE_ORDER1;
  var->has_missing = has_missing;
  var->missing = missing;
  var->cell_measures = cell_measures;
  var->cell_methods = cell_methods;
  var->area_missing = area_missing;
  var->use_volume = use_volume;
  for (int m = 0; m < ntiles_in; m++) {
    gin[m].nx = gin[m].nxc = nx_in[m];
    gin[m].ny = gin[m].nyc = ny_in[m];
    gin[m].cell_area = (double *)cell_area_in[m];
    gin[m].weight_exist = weight != NULL;
    gin[m].weight = weight ? (double *)weight[m] : NULL;
    fin[m].data = (double *)data[m];
    fin[m].grad_x = grad_x ? (double *)grad_x[m] : NULL;
    fin[m].grad_y = grad_y ? (double *)grad_y[m] : NULL;
    fin[m].grad_mask = grad_mask ? (int *)grad_mask[m] : NULL;
    fin[m].area = field_area ? (double *)field_area[m] : NULL;
    fin[m].var = var;
  }
  for (int n = 0; n < ntiles_out; n++) {
    gout[n].nx = gout[n].nxc = nx_out[n];
    gout[n].ny = gout[n].nyc = ny_out[n];
    gout[n].cell_area = (double *)cell_area_out[n];
    long o = xoff[n];
    interp[n].nxgrid = (size_t)(xoff[n + 1] - o);
    interp[n].t_in = (int *)t_in + o;
    interp[n].i_in = (int *)i_in + o;
    interp[n].j_in = (int *)j_in + o;
    interp[n].i_out = (int *)i_out + o;
    interp[n].j_out = (int *)j_out + o;
    interp[n].area = (double *)area + o;
    interp[n].di_in = di ? (double *)di + o : NULL;
    interp[n].dj_in = dj ? (double *)dj + o : NULL;
    fout[n].data = out[n];
    fout[n].var = var;
  }

  Capture c = {-1, NULL};
  if (msg) c = capture_begin();
  do_scalar_conserve_interp(interp, 0, ntiles_in, gin, ntiles_out, gout, fin, fout, opcode, nz);
  if (msg) capture_end(c, msg, msglen);
  else fflush(stdout);

  free(var); free(fout); free(fin); free(interp); free(gout); free(gin);
  return 0;
}
