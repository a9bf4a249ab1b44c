// prims_chunks.hip -- test-only C wrapper over the chunk kernel of
// csrc/sme_chunks.hpp, linked into libsme_prims.so beside prims_harness.hip
// (tests/test_gpu_chunks.py).  It launches k_chunks with a grid the caller gives,
// so one workgroup takes several chunks: the grid-stride loop and the restaging
// between chunks, which the features reach only past 2^20 chunks.
//
// The Op is the smallest one: the candidates are the integers 0, 1, 2 ... cut
// into R ranges (range r: rbeg[r] .. rbeg[r] + rcnt[r]); stage() copies the
// range's modulus into LDS and rejects the chunk if it is 0; a hit is
// value % modulus == 0; emit() writes the value.  A chunk counted or emitted with
// another range's staged modulus gives other numbers.
//
// The same discipline as prims_harness.hip: host pointers in, every device buffer
// guarded (prims_guard.hpp), the output sized to exactly the matches counted.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "prims_guard.hpp"
#include "sme_chunks.hpp"
#include "sme_internal.hpp"

namespace {
using smep::GBuf;
using namespace sme::chunks;

std::string g_err;

struct ModOp {
  const int64_t *rbeg;
  const int32_t *mod;
  struct Lds {
    int32_t mod;
  };
  struct Chunk {};
  struct Cand {
    int32_t v;
  };
  __device__ __forceinline__ bool stage(Lds &s, Chunk &, int64_t r, int64_t, int) const {
    if (threadIdx.x == 0) s.mod = mod[r];
    __syncthreads();
    return s.mod != 0;
  }
  __device__ __forceinline__ bool test(const Lds &s, const Chunk &, int64_t r, int64_t c, Cand &x) const {
    x.v = (int32_t)(rbeg[r] + c);
    return x.v % s.mod == 0;
  }
  __device__ __forceinline__ void emit(const Lds &, const Chunk &, int64_t, const Cand &x, int64_t at,
                                       int32_t *__restrict__ out) const {
    out[at] = x.v;
  }
};

}  // namespace

extern "C" {

#define SMEP_API __attribute__((visibility("default")))

SMEP_API const char *smep_chunks_last_error(void) { return g_err.c_str(); }

// R ranges of rcnt[r] >= 0 candidates and modulus mod[r] >= 0, cut into chunks of
// `chunk`, filtered by `grid` >= 1 workgroups.  -> moff[NC + 1], the scanned match
// counts of the NC = sum ceil(rcnt[r] / chunk) chunks, *total and the first
// min(*total, cap) emitted values.  guard bits: moff, values.
SMEP_API int smep_chunks_filter(const int32_t *rcnt, const int32_t *mod, int64_t R, int chunk, int64_t grid,
                                int64_t *moff, int32_t *vals, int64_t cap, int64_t *total, int *guard_bad) {
  g_err.clear();
  try {
    if (R < 0 || R >= INT32_MAX || chunk < 1 || grid < 1 || grid > kMaxGrid)
      throw sme::Error(SME_EINVAL, "smep_chunks_filter: sizes");
    std::vector<int64_t> h_rbeg((size_t)R + 1, 0), h_choff((size_t)R + 1, 0);
    for (int64_t r = 0; r < R; r++) {
      if (rcnt[r] < 0 || mod[r] < 0) throw sme::Error(SME_EINVAL, "smep_chunks_filter: negative count or modulus");
      h_rbeg[r + 1] = h_rbeg[r] + rcnt[r];
      h_choff[r + 1] = h_choff[r] + (rcnt[r] + chunk - 1) / chunk;
    }
    if (h_rbeg[R] > INT32_MAX) throw sme::Error(SME_EINVAL, "smep_chunks_filter: 2^31 or more candidates");
    const int64_t NC = h_choff[R];
    GBuf d_rcnt((size_t)R * 4), d_mod((size_t)R * 4), d_rbeg(((size_t)R + 1) * 8), d_choff(((size_t)R + 1) * 8);
    GBuf d_moff(((size_t)NC + 1) * 8);
    d_rcnt.put(rcnt, (size_t)R * 4);
    d_mod.put(mod, (size_t)R * 4);
    d_rbeg.put(h_rbeg.data(), ((size_t)R + 1) * 8);
    d_choff.put(h_choff.data(), ((size_t)R + 1) * 8);
    hipStream_t st = nullptr;
    SME_HIP(hipStreamCreate(&st));
    try {
      const ModOp op{d_rbeg.as<int64_t>(), d_mod.as<int32_t>()};
      int64_t *mo = d_moff.as<int64_t>();
      SME_HIP(hipMemsetAsync(mo + NC, 0, sizeof(int64_t), st));
      *total = 0;
      if (NC > 0) {
        sme::DevBuf scan;
        hipLaunchKernelGGL((k_chunks<ModOp, false>), dim3((unsigned)grid), dim3(kNT), 0, st, op, (int)R,
                           (const int64_t *)d_choff.as<int64_t>(), NC, (const int32_t *)d_rcnt.as<int32_t>(), chunk, mo,
                           (const int64_t *)nullptr);
        SME_CHECK_LAUNCH();
        sme::excl_scan<int64_t>(mo, mo, NC + 1, scan, st);
        SME_HIP(hipMemcpyAsync(total, mo + NC, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        SME_HIP(hipStreamSynchronize(st));
      }
      GBuf d_vals((size_t)*total * 4);
      if (*total > 0) {
        hipLaunchKernelGGL((k_chunks<ModOp, true, int32_t>), dim3((unsigned)grid), dim3(kNT), 0, st, op, (int)R,
                           (const int64_t *)d_choff.as<int64_t>(), NC, (const int32_t *)d_rcnt.as<int32_t>(), chunk,
                           (int64_t *)nullptr, (const int64_t *)mo, d_vals.as<int32_t>());
        SME_CHECK_LAUNCH();
      }
      SME_HIP(hipStreamSynchronize(st));
      d_moff.get(moff, ((size_t)NC + 1) * 8);
      d_vals.get(vals, (size_t)std::min(*total, cap) * 4);
      *guard_bad = (d_moff.guard_changed() ? 1 : 0) | (d_vals.guard_changed() ? 2 : 0);
    } catch (...) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
      throw;
    }
    (void)hipStreamDestroy(st);
    return SME_OK;
  } catch (const sme::Error &e) {
    g_err = e.what();
    return e.code;
  } catch (const std::exception &e) {
    g_err = e.what();
    return SME_EHIP;
  }
}

}  // extern "C"
