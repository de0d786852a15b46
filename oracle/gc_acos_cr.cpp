/* TEST INFRASTRUCTURE ONLY -- the arc cosine of gc_oracle.c's second build (the orc_*_cr symbols): the host build of
 * csrc/fp80.h's fg_acosl, the correctly rounded replacement for acosl that the device's great-circle kernels call.
 * fp80.h is C++ on the host, hence this shim. */
#include "fp80.h"

extern "C" double orc_fg_acosl(double x) { return fg_acosl(x); }
