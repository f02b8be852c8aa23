// common.hpp — status/error plumbing shared by the host side of libvi_amd.so.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vi_amd.h"

namespace vi {

// Thread-local last-error message (vi_last_error()).
std::string &last_error_ref();

inline vi_status fail(vi_status st, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error_ref() = buf;
  return st;
}

#define VI_HIP(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return ::vi::fail(VI_ERR_DEVICE, "HIP error %s at %s:%d (%s)", hipGetErrorString(_e), \
                        __FILE__, __LINE__, #expr);                                         \
  } while (0)

#define VI_TRY(expr)                  \
  do {                                \
    vi_status _s = (expr);            \
    if (_s != VI_OK) return _s;       \
  } while (0)

// RAII device buffer (hipMalloc/hipFree).  288 GB of HBM per GPU: no pooling games needed,
// buffers are allocated once per index / grown-only per workspace.
template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  // grow-only
  vi_status reserve(size_t count) {
    if (count <= n && p) return VI_OK;
    release();
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return fail(VI_ERR_DEVICE, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    }
    n = count;
    return VI_OK;
  }
};

// The keys, the flag words and the uploaded host ids of an id set (id_table.hpp: id_set_build).  Here, not there: a
// FetchContext (device_index.hpp) keeps one, and every file that includes id_table.hpp compiles its kernel.
struct IdSetBuffers { DevBuf<unsigned long long> words; DevBuf<uint32_t> flags; DevBuf<uint64_t> upload; };

// the stream and the K events of a context (context_pool.hpp)
template <int K>
struct StreamEvents {
  hipStream_t stream = nullptr;
  hipEvent_t ev[K] = {};
  vi_status create() {
    if (hipStreamCreateWithFlags(&stream, hipStreamDefault) != hipSuccess)
      return fail(VI_ERR_DEVICE, "hipStreamCreate failed: %s", hipGetErrorString(hipGetLastError()));
    for (auto &e : ev)
      if (hipEventCreate(&e) != hipSuccess) return fail(VI_ERR_DEVICE, "hipEventCreate failed");
    return VI_OK;
  }
  ~StreamEvents() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// what a ContextPool makes its contexts with: null (and create's message) on failure
template <class Ctx>
std::unique_ptr<Ctx> make_context() {
  auto c = std::make_unique<Ctx>();
  if (c->create() != VI_OK) c.reset();
  return c;
}

inline float elapsed_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0.0f;
  (void)hipEventElapsedTime(&ms, a, b);
  return ms;
}

// the host clock of every ms_* figure that is no HIP-event time
inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// N spans of a stream, each between two HIP events of its own.  The events exist only once create(true) has made them:
// without them begin / end record nothing and ms is 0.  ms(i) is read once the stream has passed end(i).
template <int N>
struct EventSpans {
  hipEvent_t ev[2 * N] = {};
  ~EventSpans() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  vi_status create(bool timing) {
    if (timing)
      for (auto &e : ev) VI_HIP(hipEventCreate(&e));
    return VI_OK;
  }
  vi_status begin(int i, hipStream_t st) { return record(2 * i, st); }
  vi_status end(int i, hipStream_t st) { return record(2 * i + 1, st); }
  float ms(int i) const { return ev[2 * i + 1] ? elapsed_ms(ev[2 * i], ev[2 * i + 1]) : 0.0f; }

 private:
  vi_status record(int e, hipStream_t st) {
    if (ev[e]) VI_HIP(hipEventRecord(ev[e], st));
    return VI_OK;
  }
};

inline uint32_t ceil_div_u32(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace vi
