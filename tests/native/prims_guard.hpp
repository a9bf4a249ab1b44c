// prims_guard.hpp -- the guarded device buffer of the test-only wrappers in this
// directory (libsme_prims.so).  Every device buffer a kernel under test may write
// is followed by kGuard bytes (256 eight-byte elements) of 0xA5, and the whole
// buffer is filled with 0xA5 before the input is copied in, so a kernel writing
// past its output is a failed assertion rather than a fault.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sme_internal.hpp"

namespace smep {

constexpr size_t kGuard = 256 * 8;
constexpr int kFill = 0xA5;

struct GBuf {  // device buffer of `bytes` payload + guard, all 0xA5 at first
  uint8_t *p = nullptr;
  size_t bytes = 0;
  explicit GBuf(size_t b) : bytes(b) {
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), bytes + kGuard);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      throw sme::Error(e == hipErrorOutOfMemory ? SME_ENOMEM : SME_EHIP,
                       std::string("harness hipMalloc: ") + hipGetErrorString(e));
    }
    SME_HIP(hipMemset(p, kFill, bytes + kGuard));
  }
  GBuf(const GBuf &) = delete;
  GBuf &operator=(const GBuf &) = delete;
  ~GBuf() {
    if (p) (void)hipFree(p);
  }
  template <typename T>
  T *as() const {
    return reinterpret_cast<T *>(p);
  }
  void put(const void *h, size_t n) {
    if (h && n) SME_HIP(hipMemcpy(p, h, std::min(n, bytes), hipMemcpyHostToDevice));
  }
  void get(void *h, size_t n) const {
    if (h && n) SME_HIP(hipMemcpy(h, p, std::min(n, bytes), hipMemcpyDeviceToHost));
  }
  // bytes [from, bytes + kGuard) no longer the fill pattern?
  bool changed(size_t from) const {
    std::vector<uint8_t> g(bytes + kGuard - from);
    SME_HIP(hipMemcpy(g.data(), p + from, g.size(), hipMemcpyDeviceToHost));
    for (uint8_t x : g)
      if (x != (uint8_t)kFill) return true;
    return false;
  }
  bool guard_changed() const { return changed(bytes); }
};

}  // namespace smep
