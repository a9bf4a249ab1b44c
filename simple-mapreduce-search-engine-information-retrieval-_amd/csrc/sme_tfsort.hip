// sme_tfsort.hip -- K8 of the index build: the reducer's output order.  Per term, a
// STABLE sort by tf descending of the docno-ascending postings (MyReducer.reduce's
// Collections.sort over PostingWritable.compareTo, TermKGramDocIndexer.java:211,
// PostingWritable.java:57-59).
//
// Segmented counting sort: the term CSR already delimits the segments and tf is a
// small integer, so one read + one write per posting replaces a full radix sort.
// Segments are handled by length class:
//   tiny   (<= 8)      one thread each, insertion sort in registers
//   small  (<= 64)     one wave each, rank by ballots over the distinct tfs
//   wave   (<= 512)    one wave each, the whole segment held in registers and
//                      sorted into LDS
//   medium (<= 8192)   one 4-wave workgroup each, two passes (the second from L2)
//   large              tiles of 4096 over the whole chip: count, one device-wide
//                      scan of the counters, place (a workgroup sorts its tile
//                      into LDS first)
// The kernels are bound by memory latency unless enough loads are in flight, so
// every pass issues kTfK 64-posting chunks per wave (or 16-byte loads where order
// does not matter) before it uses the first, and the per-segment kernels fetch
// the next segment's list entry and bounds while the current one runs.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>

#include "sme_internal.hpp"

namespace sme {
namespace {

constexpr int kTfTiny = 8;       // segments up to this: one thread each (insertion sort in registers)
constexpr int kTfSmall = 64;     // segments up to one wave chunk: rank by ballots
constexpr int kTfWave = 512;     // up to this: one wave, the segment in registers
constexpr int kTfMedium = 8192;  // up to this: 4-wave blocks; beyond: tiles
constexpr int kTfTile = 4096;    // postings per tile of a large segment
constexpr int kTfK = 8;          // 64-posting chunks (tf, docno) a wave has in flight
constexpr int kTfK4 = 4;         // 16-byte tf loads per lane the tile count has in flight
static_assert(kTfWave == kTfK * 64, "k_tfsort_wave holds a whole segment in kTfK chunks");

int grid_for(int64_t n, int nt = 256, int cap = 8192) {
  int64_t g = (n + nt - 1) / nt;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// segments of length <= kTfTiny (every docid term, most rare words): one thread
// each, a stable insertion sort by tf desc in registers
__global__ __launch_bounds__(256) void k_tfsort_tiny(const int64_t *__restrict__ off, int64_t V,
                                                     const int32_t *__restrict__ docno_d,
                                                     const int32_t *__restrict__ tf_d, int32_t *docno_o,
                                                     int32_t *tf_o) {
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < V; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = off[s];
    const int n = (int)(off[s + 1] - b);
    if (n > kTfTiny || n == 0) continue;
    int32_t t[kTfTiny], d[kTfTiny];
#pragma unroll
    for (int j = 0; j < kTfTiny; j++) {
      t[j] = j < n ? tf_d[b + j] : INT_MIN;  // INT_MIN: padding sinks to the end
      d[j] = j < n ? docno_d[b + j] : 0;
    }
#pragma unroll
    for (int j = 1; j < kTfTiny; j++) {  // stable: an item passes only strictly smaller tfs
#pragma unroll
      for (int k = j; k > 0; k--) {
        if (t[k - 1] < t[k]) {
          const int32_t x = t[k - 1], y = d[k - 1];
          t[k - 1] = t[k];
          d[k - 1] = d[k];
          t[k] = x;
          d[k] = y;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kTfTiny; j++)
      if (j < n) {
        docno_o[b + j] = d[j];
        tf_o[b + j] = t[j];
      }
  }
}

// The value of lane `l` (wave-uniform, as a ballot's first set bit is): a
// v_readlane, where __shfl would take a trip through the LDS crossbar.
__device__ __forceinline__ int32_t lane_value(int32_t v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int first_lane(uint64_t m) { return __ffsll((unsigned long long)m) - 1; }

// One 64-posting chunk into the counters cnt[(max_tf - tf) * NW + w]: one LDS add
// per distinct tf of the chunk (ballot groups), never one per lane -- most
// postings have tf 1, and per-lane atomics on that one counter serialise.  tf 1
// itself is counted in the scalar c1 and added once by the caller.  The adds
// return nothing, so a chunk does not wait for the previous one's.
template <int NW>
__device__ __forceinline__ void count_chunk(int32_t t, bool v, int32_t *cnt, int w, int max_tf, int lane, int &c1) {
  const uint64_t m1 = __ballot(v && t == 1);
  c1 += __popcll(m1);
  uint64_t pend = __ballot(v) & ~m1;
  while (pend) {
    const int32_t tv = lane_value(t, first_lane(pend));
    const uint64_t m = __ballot(t == tv) & pend;
    if (lane == 0) atomicAdd(&cnt[(max_tf - tv) * NW + w], __popcll(m));
    pend &= ~m;
  }
}

// One chunk placed from the scanned counters: a posting goes to its counter +
// its rank among the chunk's lanes of equal tf (ballot), which keeps docno
// order; chunks are placed in ascending order.  The tf 1 counter lives in the
// scalar base1, so the most common group takes no LDS round trip.  sb: the
// segment's first output position (0 where the outputs are an LDS staging area).
template <int NW>
__device__ __forceinline__ void place_chunk(int32_t t, int32_t d, bool v, int32_t *cnt, int w, int max_tf, int lane,
                                            uint64_t lt_mask, int &base1, int64_t sb, int32_t *docno_o,
                                            int32_t *tf_o) {
  const uint64_t m1 = __ballot(v && t == 1);
  if (m1) {  // wave-uniform
    if (m1 >> lane & 1) {
      const int64_t p = sb + base1 + __popcll(m1 & lt_mask);
      docno_o[p] = d;
      tf_o[p] = t;
    }
    base1 += __popcll(m1);
  }
  uint64_t pend = __ballot(v) & ~m1;
  while (pend) {
    const int32_t tv = lane_value(t, first_lane(pend));
    const uint64_t m = __ballot(t == tv) & pend;
    const int slot = (max_tf - tv) * NW + w;
    const int cb = cnt[slot];
    if (m >> lane & 1) {
      const int64_t p = sb + cb + __popcll(m & lt_mask);
      docno_o[p] = d;
      tf_o[p] = t;
    }
    if (lane == 0) cnt[slot] = cb + __popcll(m);
    pend &= ~m;
  }
}

// A class list walked with a stride, two entries ahead: while segment q runs, the
// bounds of q + stride and the list entry of q + 2 * stride are in flight
// (seg[q] -> off[s] -> postings would otherwise be three dependent loads per
// segment).  Every value is wave-uniform.
struct SegWalk {
  const int64_t *off;
  const int32_t *seg;
  int64_t ns, stride, q1, b, b1;  // q1: the segment after the current one
  int64_t n, n1;
  int32_t s2;
  __device__ __forceinline__ bool start(const int64_t *off_, const int32_t *seg_, int64_t ns_, int64_t q0,
                                        int64_t stride_) {
    off = off_, seg = seg_, ns = ns_, stride = stride_;
    if (q0 >= ns) return false;
    const int64_t s = seg[q0];
    b = off[s];
    n = off[s + 1] - b;
    q1 = q0 + stride;
    b1 = 0, n1 = 0;
    if (q1 < ns) {
      const int64_t s1 = seg[q1];
      b1 = off[s1];
      n1 = off[s1 + 1] - b1;
    }
    s2 = q1 + stride < ns ? seg[q1 + stride] : 0;
    return true;
  }
  // the loads of the segments after next; their results are first used by advance()
  int64_t b2, n2;
  int32_t s3;
  __device__ __forceinline__ void prefetch() {
    b2 = 0, n2 = 0;
    if (q1 + stride < ns) {
      b2 = off[s2];
      n2 = off[(int64_t)s2 + 1] - b2;
    }
    s3 = q1 + 2 * stride < ns ? seg[q1 + 2 * stride] : 0;
  }
  __device__ __forceinline__ bool advance() {
    if (q1 >= ns) return false;
    b = b1, n = n1;
    b1 = b2, n1 = n2;
    s2 = s3;
    q1 += stride;
    return true;
  }
};

// segments of length in (kTfTiny, kTfSmall] (from a class list): one wave each,
// one posting per lane; output rank of lane i = #{j : tf_j > tf_i} +
// #{j < i : tf_j == tf_i}, summed over the segment's distinct tfs (one ballot
// each).  The next segment's postings load while this one is ranked.
__global__ __launch_bounds__(256) void k_tfsort_small(const int64_t *__restrict__ off,
                                                      const int32_t *__restrict__ seg,
                                                      const unsigned long long *__restrict__ nseg,
                                                      const int32_t *__restrict__ docno_d,
                                                      const int32_t *__restrict__ tf_d, int32_t *docno_o,
                                                      int32_t *tf_o) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt_mask = (1ull << lane) - 1;
  SegWalk sw;
  if (!sw.start(off, seg, (int64_t)*nseg, (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6),
                (int64_t)gridDim.x * (blockDim.x >> 6)))
    return;
  int32_t t = lane < sw.n ? tf_d[sw.b + lane] : -1, d = lane < sw.n ? docno_d[sw.b + lane] : 0;
  for (;;) {
    const int32_t tn = lane < sw.n1 ? tf_d[sw.b1 + lane] : -1, dn = lane < sw.n1 ? docno_d[sw.b1 + lane] : 0;
    sw.prefetch();
    const bool v = lane < sw.n;
    const uint64_t vm = __ballot(v);
    int r = 0;
    uint64_t pend = vm;
    while (pend) {
      const int32_t tv = lane_value(t, first_lane(pend));
      const uint64_t m = __ballot(t == tv) & pend;
      r += t < tv ? __popcll(m) : t == tv ? __popcll(m & lt_mask) : 0;
      pend &= ~m;
    }
    if (v) {
      docno_o[sw.b + r] = d;
      tf_o[sw.b + r] = t;
    }
    if (!sw.advance()) break;
    t = tn, d = dn;
  }
}

// segments of length in (kTfSmall, kTfWave]: one wave each (four independent
// waves per workgroup, no workgroup barriers).  All of the segment's (tf, docno)
// load into registers with every load in flight; the wave counts from the
// registers, scans its LDS counters (tf desc), places from the registers into an
// LDS copy of the segment and writes that out in order: one read of the
// postings, and nothing waits on a chunk.
__global__ __launch_bounds__(256) void k_tfsort_wave(const int64_t *__restrict__ off,
                                                     const int32_t *__restrict__ seg,
                                                     const unsigned long long *__restrict__ nseg,
                                                     const int32_t *__restrict__ docno_d,
                                                     const int32_t *__restrict__ tf_d, int max_tf, int32_t *docno_o,
                                                     int32_t *tf_o) {
  extern __shared__ int32_t cnt[];  // 4 waves x (max_tf + 1), [max_tf - tf]; then 4 waves x 2 x kTfWave staging
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, F = max_tf + 1;
  int32_t *hw = cnt + w * F;
  int32_t *sd = cnt + 4 * F + w * 2 * kTfWave, *stf = sd + kTfWave;  // the sorted segment: docnos, tfs
  const uint64_t lt_mask = (1ull << lane) - 1;
  SegWalk sw;
  if (!sw.start(off, seg, (int64_t)*nseg, (int64_t)blockIdx.x * 4 + w, (int64_t)gridDim.x * 4)) return;
  do {
    const int64_t b = sw.b;
    const int n = (int)sw.n;
    int32_t t[kTfK], d[kTfK];
#pragma unroll
    for (int k = 0; k < kTfK; k++) t[k] = k * 64 + lane < n ? tf_d[b + k * 64 + lane] : -1;
#pragma unroll
    for (int k = 0; k < kTfK; k++) d[k] = k * 64 + lane < n ? docno_d[b + k * 64 + lane] : 0;
    sw.prefetch();
    for (int j = lane; j < F; j += 64) hw[j] = 0;
    __builtin_amdgcn_wave_barrier();
    int c1 = 0;
#pragma unroll
    for (int k = 0; k < kTfK; k++)
      if (k * 64 < n) count_chunk<1>(t[k], k * 64 + lane < n, hw, 0, max_tf, lane, c1);
    if (lane == 0) atomicAdd(&hw[max_tf - 1], c1);
    __builtin_amdgcn_wave_barrier();
    // exclusive scan of the counters, 64 at a time
    int carry = 0;
    for (int j0 = 0; j0 < F; j0 += 64) {
      const int j = j0 + lane;
      const int x = j < F ? hw[j] : 0;
      const int inc = wave_incl_sum(x);
      if (j < F) hw[j] = carry + inc - x;
      carry += lane_value(inc, 63);
    }
    __builtin_amdgcn_wave_barrier();
    int base1 = __builtin_amdgcn_readfirstlane(hw[max_tf - 1]);
#pragma unroll
    for (int k = 0; k < kTfK; k++)
      if (k * 64 < n)
        place_chunk<1>(t[k], d[k], k * 64 + lane < n, hw, 0, max_tf, lane, lt_mask, base1, 0, sd, stf);
    __builtin_amdgcn_wave_barrier();
    // the sorted segment leaves LDS in whole 256-byte rows (a tf group placed
    // straight to memory is one store instruction per group and chunk, most of
    // them a few lanes wide)
#pragma unroll
    for (int k = 0; k < kTfK; k++)
      if (k * 64 + lane < n) {
        docno_o[b + k * 64 + lane] = sd[k * 64 + lane];
        tf_o[b + k * 64 + lane] = stf[k * 64 + lane];
      }
    __builtin_amdgcn_wave_barrier();
  } while (sw.advance());
}

// exclusive scan of cnt[0..L) by a 256-thread workgroup (each thread a contiguous
// run, then across threads); barriers before and after are the caller's
__device__ __forceinline__ void block_scan_counters(int32_t *cnt, int L, int32_t *wsum) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int per = (L + 255) / 256, j0 = tid * per, j1 = j0 + per < L ? j0 + per : L;
  int run = 0;
  for (int j = j0; j < j1; j++) run += cnt[j];
  const int inc = wave_incl_sum(run);
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int base = inc - run;
  for (int k = 0; k < w; k++) base += wsum[k];
  for (int j = j0; j < j1; j++) {
    const int c = cnt[j];
    cnt[j] = base;
    base += c;
  }
}

// segments of length in (kTfWave, kTfMedium]: one 4-wave block per segment, wave
// w owns a contiguous run of 64-posting chunks.  Pass 1 counts tf per wave, a
// block scan orders the counters as (tf desc, wave asc), pass 2 places every
// posting (place_chunk).  Both passes have kTfK chunks per wave in flight; the
// second reads what the first just brought into L2.
__global__ __launch_bounds__(256) void k_tfsort_medium(const int64_t *__restrict__ off,
                                                       const int32_t *__restrict__ seg,
                                                       const unsigned long long *__restrict__ nseg,
                                                       const int32_t *__restrict__ docno_d,
                                                       const int32_t *__restrict__ tf_d, int max_tf,
                                                       int32_t *docno_o, int32_t *tf_o) {
  extern __shared__ int32_t cnt[];  // [(max_tf - tf) * NW + w]
  constexpr int NW = 4, NT = NW * 64;
  __shared__ int32_t wsum[NW];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int L = (max_tf + 1) * NW;
  const uint64_t lt_mask = (1ull << lane) - 1;
  SegWalk sw;
  if (!sw.start(off, seg, (int64_t)*nseg, blockIdx.x, gridDim.x)) return;  // block-uniform
  do {
    const int64_t b = sw.b;
    const int n = (int)sw.n;
    const int nch = (n + 63) >> 6, cpw = (nch + NW - 1) / NW;
    const int c0 = w * cpw, c1 = c0 + cpw < nch ? c0 + cpw : nch;
    int32_t t[kTfK], d[kTfK];
    // the first batch of pass 1 goes out before the counters are cleared
#pragma unroll
    for (int k = 0; k < kTfK; k++) {
      const int i = (c0 + k) * 64 + lane;
      t[k] = c0 + k < c1 && i < n ? tf_d[b + i] : -1;
    }
    sw.prefetch();
    for (int j = tid; j < L; j += NT) cnt[j] = 0;
    __syncthreads();
    int ones = 0;
    for (int cb = c0; cb < c1; cb += kTfK) {
      if (cb != c0) {
#pragma unroll
        for (int k = 0; k < kTfK; k++) {
          const int i = (cb + k) * 64 + lane;
          t[k] = cb + k < c1 && i < n ? tf_d[b + i] : -1;
        }
      }
#pragma unroll
      for (int k = 0; k < kTfK; k++)
        if (cb + k < c1) count_chunk<NW>(t[k], (cb + k) * 64 + lane < n, cnt, w, max_tf, lane, ones);
    }
    if (lane == 0) atomicAdd(&cnt[(max_tf - 1) * NW + w], ones);
    __syncthreads();
    block_scan_counters(cnt, L, wsum);
    __syncthreads();
    int base1 = __builtin_amdgcn_readfirstlane(cnt[(max_tf - 1) * NW + w]);
    for (int cb = c0; cb < c1; cb += kTfK) {
#pragma unroll
      for (int k = 0; k < kTfK; k++) {
        const int i = (cb + k) * 64 + lane;
        t[k] = cb + k < c1 && i < n ? tf_d[b + i] : -1;
      }
#pragma unroll
      for (int k = 0; k < kTfK; k++) {
        const int i = (cb + k) * 64 + lane;
        d[k] = cb + k < c1 && i < n ? docno_d[b + i] : 0;
      }
#pragma unroll
      for (int k = 0; k < kTfK; k++)
        if (cb + k < c1)
          place_chunk<NW>(t[k], d[k], (cb + k) * 64 + lane < n, cnt, w, max_tf, lane, lt_mask, base1, b, docno_o,
                          tf_o);
    }
    __syncthreads();
  } while (sw.advance());
}

// segment lists by class (medium: 4-wave blocks, large: tiles), appended with
// one global atomic per block and list; list order is free (segments are
// independent and their output ranges fixed)
__global__ __launch_bounds__(256) void k_tf_classify(const int64_t *__restrict__ off, int64_t V, int32_t *med,
                                                     int32_t *large, int32_t *small, int32_t *wave,
                                                     unsigned long long *ctr) {
  __shared__ unsigned int s_n[4];
  __shared__ unsigned long long s_b[4];
  for (int64_t s0 = (int64_t)blockIdx.x * 256; s0 < V; s0 += (int64_t)gridDim.x * 256) {  // block-uniform
    const int64_t s = s0 + threadIdx.x;
    const int64_t n = s < V ? off[s + 1] - off[s] : 0;
    const int cls = n > kTfMedium ? 1 : n > kTfWave ? 0 : n > kTfSmall ? 3 : n > kTfTiny ? 2 : -1;  // ctr index
    if (threadIdx.x < 4) s_n[threadIdx.x] = 0;
    __syncthreads();
    unsigned int pos = 0;
    if (cls >= 0) pos = atomicAdd(&s_n[cls], 1u);
    __syncthreads();
    if (threadIdx.x < 4)
      s_b[threadIdx.x] = s_n[threadIdx.x] ? atomicAdd(&ctr[threadIdx.x], (unsigned long long)s_n[threadIdx.x]) : 0ull;
    __syncthreads();
    if (cls == 0) med[s_b[0] + pos] = (int32_t)s;
    if (cls == 1) large[s_b[1] + pos] = (int32_t)s;
    if (cls == 2) small[s_b[2] + pos] = (int32_t)s;
    if (cls == 3) wave[s_b[3] + pos] = (int32_t)s;
    __syncthreads();
  }
}

// Segments longer than kTfMedium are cut into tiles of kTfTile postings so that a
// 1M-posting term spreads over many CUs: (1) per tile tf counts, (2) one
// exclusive scan of all the counters, laid out so that scan order is (segment,
// tf desc, tile asc), (3) per tile the ballot placement from the tile's scanned
// counters.  Segment q's T tiles start at tile toff[q]; the counter of its tile
// j and column f = max_tf - tf is tcnt[toff[q] * F + f * T + j], so the device
// scan of the flat array leaves every counter at the segment's first scanned
// value + the posting's start within the segment.

// tiles of large segment q (0 beyond the list: the scan covers nlmax + 1 entries)
__global__ void k_tf_ntiles(const int64_t *off, const int32_t *large, const unsigned long long *nlarge,
                            int64_t nlmax, int64_t *nt) {
  const int64_t nl = (int64_t)*nlarge;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q <= nlmax; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = q < nl ? off[large[q] + 1] - off[large[q]] : 0;
    nt[q] = (n + kTfTile - 1) / kTfTile;
  }
}

// segment of tile tau: the s with toff[s] <= tau < toff[s + 1]
__device__ __forceinline__ int64_t tile_segment(const int64_t *toff, int64_t V, int64_t tau) {
  int64_t lo = 0, hi = V;  // toff[lo] <= tau < toff[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (toff[mid] <= tau) lo = mid;
    else hi = mid;
  }
  return lo;
}

// four tfs at i (a multiple of 4; tf_d is 16-byte aligned) as one 16-byte load
// where all four lie in [b, e), else one by one with -1 outside
__device__ __forceinline__ int4 load_tf4(const int32_t *__restrict__ tf_d, int64_t i, int64_t b, int64_t e) {
  if (i >= b && i + 4 <= e) return *reinterpret_cast<const int4 *>(tf_d + i);
  int4 r;
  r.x = i >= b && i < e ? tf_d[i] : -1;
  r.y = i + 1 >= b && i + 1 < e ? tf_d[i + 1] : -1;
  r.z = i + 2 >= b && i + 2 < e ? tf_d[i + 2] : -1;
  r.w = i + 3 >= b && i + 3 < e ? tf_d[i + 3] : -1;
  return r;
}

// (1) one wave per tile: LDS counts.  The histogram does not depend on order, so
// the tile is read with 16-byte loads, kTfK4 per lane (4 KiB per wave) issued
// before the first is counted.
__global__ __launch_bounds__(256) void k_tf_tile_count(const int64_t *__restrict__ off,
                                                       const int32_t *__restrict__ large,
                                                       const unsigned long long *__restrict__ nlarge,
                                                       const int64_t *__restrict__ toff, int64_t ntiles,
                                                       const int32_t *__restrict__ tf_d, int max_tf,
                                                       uint32_t *tcnt, int32_t *tile_q) {
  extern __shared__ int32_t h[];  // 4 waves x (max_tf + 1)
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, F = max_tf + 1;
  int32_t *hw = h + w * F;
  const int64_t nwv = (int64_t)gridDim.x * 4;
  const int64_t nl = (int64_t)*nlarge;
  for (int64_t tau = (int64_t)blockIdx.x * 4 + w; tau < ntiles; tau += nwv) {  // wave-uniform
    const int64_t q = tile_segment(toff, nl, tau), s = large[q];
    const int64_t t0 = toff[q], T = toff[q + 1] - t0;
    const int64_t b = off[s] + (tau - t0) * kTfTile, e = min(off[s + 1], b + (int64_t)kTfTile);
    const int64_t a0 = b & ~(int64_t)3;
    const int ng = (int)((e - a0 + 3) >> 2);  // 16-byte groups covering [b, e)
    if (lane == 0) tile_q[tau] = (int32_t)q;  // the place pass skips the search
    for (int j = lane; j < F; j += 64) hw[j] = 0;
    __builtin_amdgcn_wave_barrier();
    int c1 = 0;
    for (int g0 = 0; g0 < ng; g0 += 64 * kTfK4) {
      int4 x[kTfK4];
#pragma unroll
      for (int k = 0; k < kTfK4; k++) {
        const int g = g0 + k * 64 + lane;
        x[k] = g < ng ? load_tf4(tf_d, a0 + 4 * (int64_t)g, b, e) : make_int4(-1, -1, -1, -1);
      }
#pragma unroll
      for (int k = 0; k < kTfK4; k++)
        if (g0 + k * 64 < ng) {  // (-1: outside the tile)
          count_chunk<1>(x[k].x, x[k].x >= 0, hw, 0, max_tf, lane, c1);
          count_chunk<1>(x[k].y, x[k].y >= 0, hw, 0, max_tf, lane, c1);
          count_chunk<1>(x[k].z, x[k].z >= 0, hw, 0, max_tf, lane, c1);
          count_chunk<1>(x[k].w, x[k].w >= 0, hw, 0, max_tf, lane, c1);
        }
    }
    if (lane == 0) atomicAdd(&hw[max_tf - 1], c1);
    __builtin_amdgcn_wave_barrier();
    uint32_t *col = tcnt + t0 * F + (tau - t0);
    for (int j = lane; j < F; j += 64) col[(int64_t)j * T] = (uint32_t)hw[j];
    __builtin_amdgcn_wave_barrier();
  }
}

// (3) one 4-wave workgroup per tile: stable placement from the tile's scanned
// counters.  Wave w holds the tile's w-th quarter in registers (16 chunks of
// (tf, docno), every load in flight).  The tile is first sorted into LDS -- the
// workgroup's own count, scan and placement, as k_tfsort_medium's -- and then
// leaves it in sorted order: position p of the sorted tile, of column f, goes to
// the tile's counter of f + p - the column's first position in the tile, so the
// stores of a wave are whole rows wherever a tf group is 64 long (a group placed
// straight to memory is one store instruction per group and chunk, most of them a
// few lanes wide).
constexpr int kTfQ = kTfTile / 4 / 64;  // chunks per wave
static_assert(kTfQ * 4 * 64 == kTfTile, "four waves hold a whole tile");
__global__ __launch_bounds__(256, 4) void k_tf_tile_place(const int64_t *__restrict__ off,
                                                       const int32_t *__restrict__ large,
                                                       const int32_t *__restrict__ tile_q,
                                                       const int64_t *__restrict__ toff, int64_t ntiles,
                                                       const int32_t *__restrict__ docno_d,
                                                       const int32_t *__restrict__ tf_d, int max_tf,
                                                       const uint32_t *__restrict__ tcnt, int32_t *docno_o,
                                                       int32_t *tf_o) {
  extern __shared__ int32_t h[];  // delta[F] | cnt[4 F] | sd[kTfTile] | stf[kTfTile]
  __shared__ int32_t wsum[4];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, F = max_tf + 1;
  int32_t *delta = h, *cnt = h + F, *sd = h + 5 * F, *stf = sd + kTfTile;
  const uint64_t lt_mask = (1ull << lane) - 1;
  for (int64_t tau = blockIdx.x; tau < ntiles; tau += gridDim.x) {  // block-uniform
    const int64_t q = tile_q[tau], s = large[q];
    const int64_t t0 = toff[q], T = toff[q + 1] - t0;
    const int64_t sb = off[s];
    const int64_t b = sb + (tau - t0) * kTfTile;
    const int n = (int)(min(off[s + 1], b + (int64_t)kTfTile) - b);
    const int i0 = w * (kTfQ * 64) + lane;  // this lane's first posting of the tile
    int32_t t[kTfQ], d[kTfQ];
#pragma unroll
    for (int k = 0; k < kTfQ; k++) t[k] = i0 + k * 64 < n ? tf_d[b + i0 + k * 64] : -1;
#pragma unroll
    for (int k = 0; k < kTfQ; k++) d[k] = i0 + k * 64 < n ? docno_d[b + i0 + k * 64] : 0;
    const uint32_t *col = tcnt + t0 * F + (tau - t0);
    const uint32_t seg0 = tcnt[t0 * F];  // the scan's value at the segment's first counter
    for (int j = tid; j < F; j += 256) delta[j] = (int32_t)(col[(int64_t)j * T] - seg0);
    for (int j = tid; j < 4 * F; j += 256) cnt[j] = 0;
    __syncthreads();
    int ones = 0;
#pragma unroll
    for (int k = 0; k < kTfQ; k++)
      if (w * (kTfQ * 64) + k * 64 < n) count_chunk<4>(t[k], i0 + k * 64 < n, cnt, w, max_tf, lane, ones);
    if (lane == 0) atomicAdd(&cnt[(max_tf - 1) * 4 + w], ones);
    __syncthreads();
    block_scan_counters(cnt, 4 * F, wsum);
    __syncthreads();
    for (int j = tid; j < F; j += 256) delta[j] -= cnt[j * 4];  // counter - the column's first position in the tile
    int base1 = __builtin_amdgcn_readfirstlane(cnt[(max_tf - 1) * 4 + w]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTfQ; k++)
      if (w * (kTfQ * 64) + k * 64 < n)
        place_chunk<4>(t[k], d[k], i0 + k * 64 < n, cnt, w, max_tf, lane, lt_mask, base1, 0, sd, stf);
    __syncthreads();
    for (int p = tid; p < n; p += 256) {
      const int32_t tv = stf[p];
      const int64_t g = sb + delta[max_tf - tv] + p;
      docno_o[g] = sd[p];
      tf_o[g] = tv;
    }
    __syncthreads();
  }
}

}  // namespace

void tf_sort_segments(const int64_t *off, int64_t V, int64_t P, const int32_t *docno_d, const int32_t *tf_d,
                      int max_tf, int32_t *docno_o, int32_t *tf_o, DevBuf &lists, DevBuf &tiles, DevBuf &tcnt_buf, DevBuf &scan,
                      unsigned long long *nseg, hipStream_t st, hipStream_t aux_stream, hipEvent_t ev_fork,
                      hipEvent_t ev_join) {
  if (max_tf < 1 || max_tf > kTfSortMaxTf || (reinterpret_cast<uintptr_t>(tf_d) & 15))
    throw Error(SME_EINVAL, "tf_sort_segments: max_tf outside 1.." + std::to_string(kTfSortMaxTf) +
                                " or tf_d not 16-byte aligned");
  if (V <= 0 || P <= 0) return;
  // the longer segments as lists by class (a grid-stride walk over all V terms costs
  // a dependent offset load per term and block)
  int64_t *ntl = lists.as<int64_t>(3 * (V + 1)), *toff = tiles.as<int64_t>(V + 1);
  int32_t *seg_med = reinterpret_cast<int32_t *>(ntl + V + 1), *seg_large = seg_med + V, *seg_small = seg_large + V,
          *seg_wave = seg_small + V;
  SME_HIP(hipMemsetAsync(nseg, 0, 4 * sizeof(unsigned long long), st));  // [0] medium, [1] large, [2] small, [3] wave
  hipLaunchKernelGGL(k_tf_classify, dim3(grid_for(V)), dim3(256), 0, st, off, V, seg_med, seg_large, seg_small,
                     seg_wave, nseg);
  // every class but the large one (disjoint terms, disjoint output ranges) runs on
  // the auxiliary stream beside the large tiles' count / scan / place chain, which
  // also waits on a host read of the tile count (on one stream the stage took
  // 3.1 ms where two took 2.8)
  SME_HIP(hipEventRecord(ev_fork, st));
  SME_HIP(hipStreamWaitEvent(aux_stream, ev_fork, 0));
  // every exit from here on -- a throw between the fork and the join included --
  // makes st wait for the auxiliary stream's kernels, so they never write
  // docno_o / tf_o after the caller's buffers are released or reused
  struct AuxJoin {
    hipStream_t st, s2;
    hipEvent_t ev;
    ~AuxJoin() {
      (void)hipEventRecord(ev, s2);
      (void)hipStreamWaitEvent(st, ev, 0);
    }
  } aux_join{st, aux_stream, ev_join};
  const int F = max_tf + 1;
  const size_t lds4 = (size_t)4 * F * sizeof(int32_t);
  hipLaunchKernelGGL(k_tfsort_small, dim3(grid_for(V * 64, 256, 8192)), dim3(256), 0, aux_stream, off, seg_small,
                     nseg + 2, docno_d, tf_d, docno_o, tf_o);
  hipLaunchKernelGGL(k_tfsort_medium, dim3((unsigned)std::min<int64_t>(V, 4096)), dim3(256), lds4, aux_stream, off,
                     seg_med, nseg, docno_d, tf_d, max_tf, docno_o, tf_o);
  hipLaunchKernelGGL(k_tfsort_wave, dim3(grid_for(V * 64, 256, 8192)), dim3(256),
                     lds4 + (size_t)4 * 2 * kTfWave * sizeof(int32_t), aux_stream, off, seg_wave, nseg + 3, docno_d, tf_d,
                     max_tf, docno_o, tf_o);
  hipLaunchKernelGGL(k_tfsort_tiny, dim3(grid_for(V)), dim3(256), 0, aux_stream, off, V, docno_d, tf_d, docno_o, tf_o);
  SME_CHECK_LAUNCH();
  // large segments: tiles spread over the whole chip.  A large segment has more
  // than kTfMedium postings, so at most nlmax of the V list entries are in use and
  // the tile offsets are scanned only that far.
  const int64_t nlmax = std::min<int64_t>(V, P / (kTfMedium + 1));
  hipLaunchKernelGGL(k_tf_ntiles, dim3(grid_for(nlmax + 1)), dim3(256), 0, st, off, seg_large, nseg + 1, nlmax, ntl);
  excl_scan(ntl, toff, nlmax + 1, scan, st);
  // (read back through a small pinned buffer of the calling thread: a pageable
  // destination takes the runtime's staged path, a longer stall)
  static thread_local int64_t *pin = nullptr;
  if (!pin) SME_HIP(hipHostMalloc(reinterpret_cast<void **>(&pin), 64, hipHostMallocDefault));
  SME_HIP(hipMemcpyAsync(pin, toff + nlmax, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  SME_HIP(hipStreamSynchronize(st));
  const int64_t ntiles = *pin;
  if (ntiles > 0) {
    uint32_t *tcnt = tcnt_buf.as<uint32_t>((size_t)ntiles * F + 2 + (size_t)ntiles);
    int32_t *tile_q = reinterpret_cast<int32_t *>(tcnt + (size_t)ntiles * F + 2);  // tile -> its entry of the large list
    const unsigned tg = (unsigned)std::min<int64_t>((ntiles + 3) / 4, 8192);
    hipLaunchKernelGGL(k_tf_tile_count, dim3(tg), dim3(256), lds4, st, off, seg_large, nseg + 1, toff, ntiles, tf_d,
                       max_tf, tcnt, tile_q);
    excl_scan(tcnt, tcnt, ntiles * F, scan, st);
    hipLaunchKernelGGL(k_tf_tile_place, dim3((unsigned)std::min<int64_t>(ntiles, 16384)), dim3(256),
                       (size_t)(5 * F + 2 * kTfTile) * sizeof(int32_t), st, off, seg_large, (const int32_t *)tile_q, toff,
                       ntiles, docno_d, tf_d, max_tf, tcnt, docno_o, tf_o);
  }
  SME_CHECK_LAUNCH();
}

}  // namespace sme
