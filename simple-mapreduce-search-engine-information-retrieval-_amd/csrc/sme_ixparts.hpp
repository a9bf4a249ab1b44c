// sme_ixparts.hpp -- small parts the index makers share (sme_load.hip, sme_merge.hip,
// sme_ixmerge.hip, sme_ixdelete.hip, sme_posfile.hip, sme_vunion.hip).  Internal:
// nothing of it enters include/sme.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sme_common.hpp"

namespace sme {

// ---- host ------------------------------------------------------------------------------
// workgroups for n items at `per` items each, at least 1 and at most cap
inline unsigned grid_n(int64_t n, int64_t per = 256, int64_t cap = 16384) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap));
}
// bits that hold v (at least 1)
inline int bits_of(uint64_t v) {
  int b = 1;
  while (b < 64 && (1ull << b) <= v) b++;
  return b;
}
// one device word, after everything queued on st
template <typename T>
T rd1(const T *d, hipStream_t st) {
  T h;
  SME_HIP(hipMemcpyAsync(&h, d, sizeof(T), hipMemcpyDeviceToHost, st));
  SME_HIP(hipStreamSynchronize(st));
  return h;
}

// ---- device ----------------------------------------------------------------------------
// last index r in [lo, hi) with tab[r] <= p (tab ascending, tab[lo] <= p); the
// interval halves every step
__device__ __forceinline__ int64_t last_le(const int64_t *tab, int64_t lo, int64_t hi, int64_t p) {
  for (int it = 0; it < 64 && hi - lo > 1; it++) {
    const int64_t m = lo + ((hi - lo) >> 1);
    if (tab[m] <= p)
      lo = m;
    else
      hi = m;
  }
  return lo;
}
// the input that flat item j belongs to (base: n + 1 ascending starts, base[0] = 0;
// inputs without items are skipped)
__device__ __forceinline__ int input_of(const int64_t *base, int n, int64_t j) {
  int a = 0;
  while (a + 1 < n && base[a + 1] <= j) a++;
  return a;
}

// The flat walk over CSR rows: f(p, row) for every element p of [0, M), row the last
// one with off[row] <= p (off: nrow + 1 ascending offsets from 0 to M).  A workgroup
// of NT threads takes kRowBlock elements at a time: two threads find the block's
// window of rows, every element then searches only that window, consecutive threads
// on consecutive elements.  Every thread of the workgroup must call it (barriers).
constexpr int kRowBlock = 1024;
template <int NT, class F>
__device__ __forceinline__ void for_row_elements(const int64_t *off, int64_t nrow, int64_t M, F f) {
  __shared__ int64_t s_r[2];
  const int64_t nblk = (M + kRowBlock - 1) / kRowBlock;
  for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    const int64_t p0 = b * kRowBlock, p1 = min(M, p0 + kRowBlock);
    if (threadIdx.x < 2) s_r[threadIdx.x] = last_le(off, 0, nrow + 1, threadIdx.x ? p1 - 1 : p0);
    __syncthreads();
    const int64_t w0 = s_r[0], w1 = s_r[1] + 1;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += NT) f(p, last_le(off, w0, w1, p));
    __syncthreads();  // s_r is rewritten
  }
}

}  // namespace sme
