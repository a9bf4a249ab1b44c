// sme_chunks.hpp -- the chunked candidate filter shared by wildcard expansion
// (sme_wild.hip), spelling suggestions (sme_fuzzy.hip) and Boolean retrieval
// (sme_bool.hip).  Internal: nothing of it enters include/sme.h.
//
// A batch has R candidate ranges, range r holding rcnt[r] candidates and owning
// ceil(rcnt[r] / chunk) chunks; choff is the exclusive scan of those chunk counts
// (entry R = NC, all chunks).  k_chunks runs twice over the chunks, one workgroup
// per chunk and one candidate per thread: counting (mcnt[ch] = hits of the chunk)
// and, after a scan of the counts, emitting (hit x of chunk ch at moff[ch] + x, in
// candidate order).  What a candidate is, what a hit is and what is written for
// one is the feature's Op; DESIGN, "The chunked candidate filter", has the whole pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "sme_internal.hpp"

namespace sme {
namespace chunks {
constexpr int kNT = 256;  // threads of the chunk kernels
constexpr int64_t kMaxGrid = 1 << 20;

inline unsigned grid_for(int64_t n) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kNT - 1) / kNT, 65536));
}

// ---- device searches ----------------------------------------------------------
// first index of the ascending p[0 .. n) with p[i] >= v / with p[i] > v
// (the midpoint is taken unsigned: lo + hi may pass the index type's largest value)
template <typename T, typename I>
__device__ __forceinline__ I lower_bound(const T *__restrict__ p, I n, T v) {
  I lo = 0, hi = n;
  while (lo < hi) {
    const I m = (I)(((std::make_unsigned_t<I>)lo + (std::make_unsigned_t<I>)hi) >> 1);
    if (p[m] < v)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}
template <typename T, typename I>
__device__ __forceinline__ I upper_bound(const T *__restrict__ p, I n, T v) {
  I lo = 0, hi = n;
  while (lo < hi) {
    const I m = (I)(((std::make_unsigned_t<I>)lo + (std::make_unsigned_t<I>)hi) >> 1);
    if (p[m] <= v)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}

// The posting range of trigram key k in the table of sme_wild.hip: gterm[beg ..
// beg + cnt), cnt >= 1; a key no term holds gives the empty range (0, 0).
struct GramRange {
  int32_t beg, cnt;
};
__device__ __forceinline__ GramRange gram_postings(const uint64_t *__restrict__ keys,
                                                   const int32_t *__restrict__ goff, int64_t G, uint64_t k) {
  const int64_t g = lower_bound(keys, G, k);
  if (g == G || keys[g] != k) return GramRange{0, 0};
  return GramRange{goff[g], goff[g + 1] - goff[g]};
}

// The chunk's range: the last one whose first chunk is at or before `ch` (ranges
// without candidates own no chunk).  R < 2^31 (every caller refuses a larger
// batch), so the index is 32-bit: gfx950 has no scalar 64-bit ordered compare, and
// a 64-bit loop test goes through the vector unit once per step.
__device__ __forceinline__ int chunk_range(const int64_t *__restrict__ choff, int R, int64_t ch) {
  return upper_bound(choff, R, ch) - 1;
}

// ---- the chunk kernel ---------------------------------------------------------
// Op, a struct of pointers to what the feature reads, passed by value, is all that
// differs between the features:
//   Op::Lds    what stage() leaves in LDS for the chunk's threads
//   Op::Chunk  per thread, the uniform facts of the chunk that stage() worked out
//   Op::Cand   what a hit carries from test() to emit()
//   bool stage(Lds &, Chunk &, r, c0, len)  called by every thread for chunk
//       [c0, c0 + len) of range r; ends with a barrier after its last LDS write;
//       false (for all threads alike) rejects the whole chunk: no candidate hits
//   bool test(const Lds &, const Chunk &, r, c, Cand &)  is candidate c of range r
//       a hit?
//   void emit(const Lds &, const Chunk &, r, const Cand &, at, out...)  write hit
//       number `at` of the batch into the output arrays
// EMIT = false: mcnt[ch] = hits of the chunk.  EMIT = true: the hits are emitted at
// moff[ch] + rank, the rank from the waves' ballots, so they keep candidate order.
// The output arrays are kernel arguments of their own (`out`, only when emitting)
// and not members of Op: Op is the same for both passes, and as __restrict__
// arguments the outputs are known not to overlap what Op reads, so the compiler
// may keep a chunk's uniform loads scalar across the emit stores.
template <class Op, bool EMIT, class... Out>
__global__ __launch_bounds__(kNT) void k_chunks(Op op, int R, const int64_t *__restrict__ choff, int64_t NC,
                                                const int32_t *__restrict__ rcnt, int chunk,
                                                int64_t *__restrict__ mcnt, const int64_t *__restrict__ moff,
                                                Out *__restrict__... out) {
  __shared__ struct {  // one object: two would each be padded to their own alignment
    typename Op::Lds op;
    int wsum[kNT / 64];
  } s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int64_t ch = blockIdx.x; ch < NC; ch += gridDim.x) {
    const int r = chunk_range(choff, R, ch);
    const int64_t c0 = (ch - choff[r]) * chunk;
    const int len = (int)min((int64_t)chunk, (int64_t)rcnt[r] - c0);  // >= 1: only candidates make chunks
    typename Op::Chunk k;
    const bool live = op.stage(s.op, k, r, c0, len);
    int64_t run = EMIT ? moff[ch] : 0;  // matches of the rounds before
    for (int rd = 0; live && rd < len; rd += kNT) {
      const int c = rd + tid;
      typename Op::Cand cand{};
      const bool hit = c < len && op.test(s.op, k, r, c0 + c, cand);
      const unsigned long long m = __ballot(hit);
      if (lane == 0) s.wsum[wv] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kNT / 64; w++) {
        const int ws = s.wsum[w];
        before += w < wv ? ws : 0;
        total += ws;
      }
      if constexpr (EMIT) {
        if (hit) op.emit(s.op, k, r, cand, run + before + __popcll(m & ((1ull << lane) - 1)), out...);
      }
      run += total;
      __syncthreads();  // wsum is rewritten by the next round
    }
    if (!EMIT && tid == 0) mcnt[ch] = run;
    // Restaging (grid-stride: NC > gridDim.x): the next chunk's stage() rewrites the
    // LDS that this chunk's test() and emit() -- or, in a rejected chunk, stage()'s
    // own verdict -- may still be read from by a slower wave.  So one barrier ends
    // every chunk, whatever path it took.  After a chunk that ran its rounds the last
    // round's barrier would do as well; the rule is not made to depend on that.
    __syncthreads();
  }
}

// out[i] = matches before owner i's first chunk (i = n: all of them); first(i) is
// the owner's first range (first(n) = R), and an owner without chunks has the
// next one's offset
template <class First>
__global__ void k_owner_offs(First first, const int64_t *__restrict__ choff, const int64_t *__restrict__ moff,
                             int64_t n, int64_t *__restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = moff[choff[first(i)]];
}
// kept[i] = owner i's matches after the cut (m = 0: no cut); kept[n] = 0
// (static: every file that includes this header has its own)
static __global__ void k_cut(const int64_t *__restrict__ off, int64_t n, int64_t m, int64_t *__restrict__ kept) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i < n ? off[i + 1] - off[i] : 0;
    kept[i] = m > 0 && c > m ? m : c;
  }
}

// ---- host side ----------------------------------------------------------------
// The upload blob: aligned sections, one host-to-device copy for all of them.
struct Blob {
  std::vector<uint8_t> bytes;
  // appends `count` T from p, aligned; -> the section's byte offset
  template <typename T>
  size_t add(const T *p, size_t count) {
    const size_t a = (bytes.size() + alignof(T) - 1) / alignof(T) * alignof(T);
    bytes.resize(a + count * sizeof(T));
    if (count) memcpy(bytes.data() + a, p, count * sizeof(T));
    return a;
  }
};

// bits of a stable sort by owner id over n owners
inline int owner_bits(int64_t n) {
  int bits = 1;
  while (bits < 32 && (int64_t(1) << bits) < n) bits++;
  return bits;
}

struct Counted {  // what the counting pass leaves for the emitting one
  int R;
  const int64_t *choff;  // [R + 1] scanned
  const int32_t *rcnt;
  int chunk;
  int64_t NC, total;
  unsigned grid;
  const int64_t *moff;  // [NC + 1] matches before each chunk (entry NC = total)
};

// choff holds the ranges' chunk counts (entry R = 0).  Scans them in place, reads
// NC back (and with it, in the same synchronisation, the plan kernel's counter
// *d_extra if given), counts every chunk's matches into moff_buf and scans those;
// `limit` is the SME_ELIMIT message at 2^31 matches or more.  Two device
// synchronisations, one if there is no chunk.
template <class Op>
Counted count_chunks(const Op &op, int R, int64_t *choff, const int32_t *rcnt, int chunk, DevBuf &moff_buf,
                     DevBuf &scan_buf, const char *limit, hipStream_t st, const unsigned long long *d_extra = nullptr,
                     unsigned long long *extra = nullptr) {
  Counted c{R, choff, rcnt, chunk, 0, 0, 1, nullptr};
  excl_scan<int64_t>(choff, choff, (int64_t)R + 1, scan_buf, st);
  SME_HIP(hipMemcpyAsync(&c.NC, choff + R, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (d_extra) SME_HIP(hipMemcpyAsync(extra, d_extra, sizeof(*extra), hipMemcpyDeviceToHost, st));
  SME_HIP(hipStreamSynchronize(st));
  // matches per chunk, scanned in place (entry NC = all matches)
  int64_t *moff = moff_buf.as<int64_t>((size_t)c.NC + 1);
  c.moff = moff;
  c.grid = (unsigned)std::max<int64_t>(1, std::min(c.NC, kMaxGrid));
  SME_HIP(hipMemsetAsync(moff + c.NC, 0, sizeof(int64_t), st));
  if (c.NC > 0) {
    hipLaunchKernelGGL((k_chunks<Op, false>), dim3(c.grid), dim3(kNT), 0, st, op, R, c.choff, c.NC, rcnt, chunk, moff,
                       (const int64_t *)nullptr);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(moff, moff, c.NC + 1, scan_buf, st);
    SME_HIP(hipMemcpyAsync(&c.total, moff + c.NC, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
  }
  if (c.total >= (int64_t(1) << 31)) throw Error(SME_ELIMIT, limit);
  return c;
}

// the emitting pass into `out`, arrays the caller has sized for c.total matches
template <class Op, class... Out>
void emit_chunks(const Op &op, const Counted &c, hipStream_t st, Out *...out) {
  if (c.total == 0) return;
  hipLaunchKernelGGL((k_chunks<Op, true, Out...>), dim3(c.grid), dim3(kNT), 0, st, op, c.R, c.choff, c.NC, c.rcnt,
                     c.chunk, (int64_t *)nullptr, c.moff, out...);
  SME_CHECK_LAUNCH();
}
}  // namespace chunks
}  // namespace sme
