// fg_host.h -- what the host side of every .hip file shares: the error return over the library's last-error string, the HIP
// call check, the wall clock, the device choice, and device memory owned by a scope.  The C sources (remap_file.c, field_file.c)
// keep their own error buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <chrono>
#include <vector>
#include "fregrid_hip.h"

void fg_set_last_error(const char *msg);         // plan.hip owns the string behind fg_last_error()

// sets the calling thread's last error and returns `code`
static inline int fg_fail(int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  fg_set_last_error(buf);
  return code;
}
#define FGCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
  return fg_fail(FG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

static inline double fg_now_ms(void)
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the device of the entry points that take none: FREGRID_HIP_DEVICE, default 0
static inline int fg_env_device(void)
{
  const char *e = getenv("FREGRID_HIP_DEVICE");
  return e ? atoi(e) : 0;
}

// makes `device` the calling thread's current device; 0, or the error code with the message set
static inline int fg_use_device(const char *who, int device)
{
  int ndev = 0;
  FGCHK(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fg_fail(FG_ERR_HIP, "no HIP device visible: libfregrid_hip needs an MI355X-class GPU");
  if (device < 0 || device >= ndev) return fg_fail(FG_ERR_ARG, "%s: device %d out of range (0..%d)", who, device, ndev - 1);
  FGCHK(hipSetDevice(device));
  return 0;
}

// device memory that is released when the owner goes out of scope; get and put return null on failure
struct FgDev {
  std::vector<void *> ptrs;
  FgDev() = default;
  FgDev(const FgDev &) = delete;
  FgDev &operator=(const FgDev &) = delete;
  ~FgDev() { for (void *p : ptrs) (void)hipFree(p); }
  template <typename T> T *get(size_t n)
  {
    void *p = nullptr;
    if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return (T *)p;
  }
  template <typename T> T *put(const T *src, size_t n)
  {
    T *p = get<T>(n);
    if (p && n && hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
  }
  template <typename T> T *put(const std::vector<T> &v) { return put(v.data(), v.size()); }
};
