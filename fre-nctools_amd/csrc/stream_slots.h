// stream_slots.h -- what the streamed field loops share (sweep.hip: fg_sweep, bilinear.hip: fg_bilin_sweep, column.hip: fg_column): the shape of the
// pipeline -- NSLOT buffer slots of CHUNK levels on a copy-in, a compute and a copy-out stream -- and two host helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "fregrid_hip.h"

namespace fg_stream {
constexpr int NSLOT = 3;       // buffer slots in flight
constexpr int CHUNK = 8;       // levels per chunk: what fg_c2l_records / fg_plan_apply_records take per call

inline size_t type_size(int t) { return t == FG_NC_SHORT ? 2 : (t == FG_NC_INT || t == FG_NC_FLOAT) ? 4 : t == FG_NC_DOUBLE ? 8 : 0; }

inline bool is_pinned(const void *p)
{
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeHost;
}

// get_input_data's conversion (sweep.hip's k_widen) queued on `st`: out[i] = (double)raw[i], scaled / offset where != missing
void widen(int nc_type, long n, const void *raw, double scale, double offset, double missing, double *out, hipStream_t st);
}  // namespace fg_stream
