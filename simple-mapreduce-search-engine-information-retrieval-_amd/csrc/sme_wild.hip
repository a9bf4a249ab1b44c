// sme_wild.hip -- wildcard term expansion: the character-trigram table of an
// index's vocabulary and the batched pattern -> term ids pass over it.
//
// Table (once per index; depends on the vocabulary only):
//   keys[G]      distinct trigram keys (sme_wild.hpp), ascending
//   goff[G + 1]  CSR offsets into gterm
//   gterm[NPu]   term ids holding each key, ascending inside a key
// built from (key, term id) pairs written in term order, a stable LSD sort by the
// key's 50 bits, and two neighbour compactions (repeated pairs, then key heads).
//
// Expansion: k_wild_plan picks per pattern the shortest posting list among its
// trigrams (or the whole vocabulary), the candidates are cut into chunks, and
// k_wild_chunks -- once counting, once emitting -- verifies every candidate with
// wild_match, one workgroup per chunk: the candidate source never changes the
// result.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sme_internal.hpp"
#include "sme_wild.hpp"

namespace sme {
namespace {
constexpr int kNT = 256;  // threads of the chunk kernels
constexpr int64_t kMaxGrid = 1 << 20;

unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kNT - 1) / kNT, 65536)); }

// ---- table build ------------------------------------------------------------
// A term of L units has L windows, so the windows' exclusive scan is the term
// offsets themselves: window w (0 <= w < NP) is the unit at toff[0] + w, and its
// term the last one starting at or before it (terms of 0 units own no window).
__global__ void k_wt_pairs(const int64_t *__restrict__ toff, const uint16_t *__restrict__ tch, int64_t V, int64_t NP,
                           uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const int64_t base = toff[0];
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < NP; w += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pos = base + w;
    int64_t lo = 0, hi = V;  // first term with toff > pos
    while (lo < hi) {
      const int64_t m = (lo + hi) >> 1;
      if (toff[m] <= pos)
        lo = m + 1;
      else
        hi = m;
    }
    const int64_t t = lo - 1, b = toff[t];
    keys[w] = wild::term_gram(tch + b, toff[t + 1] - b, pos - b);
    vals[w] = (uint32_t)t;
  }
}

// first of every run of equal (key, term) neighbours
__global__ void k_wt_pair_heads(const uint64_t *__restrict__ k, const uint32_t *__restrict__ v, int64_t n,
                                uint8_t *__restrict__ f) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    f[i] = (i == 0 || k[i] != k[i - 1] || v[i] != v[i - 1]) ? 1 : 0;
}
__global__ void k_wt_gather_pairs(const uint64_t *__restrict__ k, const uint32_t *__restrict__ v,
                                  const int32_t *__restrict__ idx, int64_t n, uint64_t *__restrict__ uk,
                                  int32_t *__restrict__ gterm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uk[i] = k[idx[i]];
    gterm[i] = (int32_t)v[idx[i]];
  }
}
__global__ void k_wt_key_heads(const uint64_t *__restrict__ k, int64_t n, uint8_t *__restrict__ f) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    f[i] = (i == 0 || k[i] != k[i - 1]) ? 1 : 0;
}
// goff[g] = head index of key g (already there), keys[g] = its key; goff[G] = NPu
__global__ void k_wt_keys(const uint64_t *__restrict__ uk, int32_t *__restrict__ goff, int64_t G, int64_t NPu,
                          uint64_t *__restrict__ keys) {
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g <= G; g += (int64_t)gridDim.x * blockDim.x) {
    if (g < G)
      keys[g] = uk[goff[g]];
    else
      goff[g] = (int32_t)NPu;
  }
}

// ---- expansion --------------------------------------------------------------
struct Batch {           // the uploaded batch (device pointers into one block)
  const uint64_t *gkey;  // gram keys of all patterns
  const int32_t *uoff;   // [n + 1] unit offsets
  const int32_t *goff;   // [n + 1] gram offsets
  const uint16_t *unit;
  const uint8_t *mask;
};

// One thread per pattern: cbeg < 0 = candidates are the term ids [0, ccnt), else
// gterm[cbeg .. cbeg + ccnt).
__global__ void k_wild_plan(Batch b, int n, const uint64_t *__restrict__ keys, const int32_t *__restrict__ goff,
                            int64_t G, int64_t V, int scan, int chunk, int32_t *__restrict__ cbeg,
                            int32_t *__restrict__ ccnt, int64_t *__restrict__ nchunk) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
    if (i == n) {
      nchunk[i] = 0;
      continue;
    }
    int32_t beg = -1, cnt = (int32_t)V;
    if (!scan) {
      for (int g = b.goff[i]; g < b.goff[i + 1]; g++) {
        const uint64_t k = b.gkey[g];
        int64_t lo = 0, hi = G;  // first key >= k
        while (lo < hi) {
          const int64_t m = (lo + hi) >> 1;
          if (keys[m] < k)
            lo = m + 1;
          else
            hi = m;
        }
        if (lo == G || keys[lo] != k) {  // a trigram no term holds: no match
          beg = 0;
          cnt = 0;
          break;
        }
        const int32_t c = goff[lo + 1] - goff[lo];
        if (beg < 0 || c < cnt) {
          beg = goff[lo];
          cnt = c;
        }
      }
    }
    cbeg[i] = beg;
    ccnt[i] = cnt;
    nchunk[i] = ((int64_t)cnt + chunk - 1) / chunk;
  }
}

// The chunk's pattern: the last one whose first chunk is at or before `ch`
// (patterns without candidates own no chunk).
__device__ __forceinline__ int chunk_pattern(const int64_t *__restrict__ choff, int n, int64_t ch) {
  int lo = 0, hi = n;  // first pattern with choff > ch
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (choff[m] <= ch)
      lo = m + 1;
    else
      hi = m;
  }
  return lo - 1;
}

// One workgroup per chunk (grid-stride over the chunks): the pattern is staged in
// LDS, the chunk's candidates are taken kNT at a time, one per thread.  EMIT = false:
// mcnt[ch] = matches of the chunk.  EMIT = true: the matches' term ids at
// moff[ch] + rank, the rank from the waves' ballots, so they come out ascending.
template <bool EMIT>
__global__ __launch_bounds__(kNT) void k_wild_chunks(Batch b, int n, const int64_t *__restrict__ choff, int64_t NC,
                                                     const int32_t *__restrict__ cbeg,
                                                     const int32_t *__restrict__ ccnt,
                                                     const int32_t *__restrict__ gterm,
                                                     const int64_t *__restrict__ toff,
                                                     const uint16_t *__restrict__ tch, int chunk,
                                                     int64_t *__restrict__ mcnt, const int64_t *__restrict__ moff,
                                                     int32_t *__restrict__ ids) {
  __shared__ uint16_t s_unit[256];
  __shared__ uint8_t s_mask[256];
  __shared__ int s_wsum[kNT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int64_t ch = blockIdx.x; ch < NC; ch += gridDim.x) {
    const int i = chunk_pattern(choff, n, ch);
    const int u0 = b.uoff[i], np = b.uoff[i + 1] - u0;
    if (tid < np) {
      s_unit[tid] = b.unit[u0 + tid];
      s_mask[tid] = b.mask[u0 + tid];
    }
    __syncthreads();
    const int32_t beg = cbeg[i];
    const int64_t c0 = (ch - choff[i]) * chunk;
    const int len = (int)min((int64_t)chunk, (int64_t)ccnt[i] - c0);
    int64_t run = EMIT ? moff[ch] : 0;  // matches of the rounds before
    for (int r = 0; r < len; r += kNT) {
      const int c = r + tid;
      bool hit = false;
      int32_t t = 0;
      if (c < len) {
        t = beg < 0 ? (int32_t)(c0 + c) : gterm[beg + c0 + c];
        const int64_t a = toff[t];
        hit = wild::wild_match(s_unit, s_mask, np, tch + a, (int)(toff[t + 1] - a));
      }
      const unsigned long long m = __ballot(hit);
      if (lane == 0) s_wsum[wv] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kNT / 64; w++) {
        const int s = s_wsum[w];
        before += w < wv ? s : 0;
        total += s;
      }
      if (EMIT && hit) ids[run + before + __popcll(m & ((1ull << lane) - 1))] = t;
      run += total;
      __syncthreads();  // s_wsum (and, after the last round, the staged pattern) is rewritten
    }
    if (!EMIT && tid == 0) mcnt[ch] = run;
  }
}

// match_off[i] = matches before pattern i's first chunk (i = n: all of them)
__global__ void k_wild_offs(const int64_t *__restrict__ choff, const int64_t *__restrict__ moff, int n,
                            int64_t *__restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) out[i] = moff[choff[i]];
}

// appends an aligned section of `count` T to the upload blob; *at = its byte offset
template <typename T>
void section(std::vector<uint8_t> &blob, size_t count, size_t *at) {
  const size_t a = (blob.size() + alignof(T) - 1) / alignof(T) * alignof(T);
  blob.resize(a + count * sizeof(T));
  *at = a;
}
}  // namespace

void prepare_wildcards(sme_index *ix, hipStream_t st) {
  if (ix->wild_ready) return;
  sme_ctx *cx = ix->ctx;
  const int64_t V = ix->V;
  const int64_t *toff = (const int64_t *)ix->d_term_off.p;
  const uint16_t *tch = (const uint16_t *)ix->d_term_chars.p;
  hipEvent_t e0, e1;
  SME_HIP(hipEventCreate(&e0));
  SME_HIP(hipEventCreate(&e1));
  struct Events {
    hipEvent_t a, b;
    ~Events() {
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
    }
  } events{e0, e1};
  SME_HIP(hipEventRecord(e0, st));
  int64_t NP = 0, NPu = 0, G = 0;
  if (V > 0) {
    int64_t ends[2];
    SME_HIP(hipMemcpyAsync(&ends[0], toff, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipMemcpyAsync(&ends[1], toff + V, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    NP = ends[1] - ends[0];
  }
  if (NP >= (int64_t(1) << 31)) throw Error(SME_ELIMIT, "wildcard table: 2^31 or more (trigram, term) pairs");
  if (NP > 0) {
    // temporaries of this build: pooled blocks, back in the pool on return
    DevBuf k0, k1, v0, v1, flag, idx, uk, cnt, s1, s2, radix;
    for (DevBuf *b : {&k0, &k1, &v0, &v1, &flag, &idx, &uk, &cnt, &s1, &s2, &radix}) b->pool = &cx->pool;
    try {
      uint64_t *ka = k0.as<uint64_t>(NP), *kb = k1.as<uint64_t>(NP);
      uint32_t *va = v0.as<uint32_t>(NP), *vb = v1.as<uint32_t>(NP);
      uint8_t *f = flag.as<uint8_t>(NP);
      int32_t *sel = idx.as<int32_t>(NP);
      int32_t *d_cnt = cnt.as<int32_t>(2);
      hipLaunchKernelGGL(k_wt_pairs, dim3(grid_for(NP)), dim3(kNT), 0, st, toff, tch, V, NP, ka, va);
      SME_CHECK_LAUNCH();
      sort_pairs<uint64_t>(ka, kb, va, vb, NP, wild::kKeyBits, radix, st);
      hipLaunchKernelGGL(k_wt_pair_heads, dim3(grid_for(NP)), dim3(kNT), 0, st, kb, vb, NP, f);
      select_flagged(f, NP, sel, d_cnt, s1, s2, st);
      int32_t h = 0;
      SME_HIP(hipMemcpyAsync(&h, d_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
      NPu = h;
      uint64_t *ukeys = uk.as<uint64_t>(NPu);
      int32_t *gterm = ix->d_wgterm.as<int32_t>(NPu);
      hipLaunchKernelGGL(k_wt_gather_pairs, dim3(grid_for(NPu)), dim3(kNT), 0, st, kb, vb, sel, NPu, ukeys, gterm);
      hipLaunchKernelGGL(k_wt_key_heads, dim3(grid_for(NPu)), dim3(kNT), 0, st, ukeys, NPu, f);
      select_flagged(f, NPu, sel, d_cnt + 1, s1, s2, st);
      SME_HIP(hipMemcpyAsync(&h, d_cnt + 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
      G = h;
      int32_t *goff = ix->d_wgoff.as<int32_t>(G + 1);
      uint64_t *keys = ix->d_wkeys.as<uint64_t>(G);
      SME_HIP(hipMemcpyAsync(goff, sel, (size_t)G * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(k_wt_keys, dim3(grid_for(G + 1)), dim3(kNT), 0, st, ukeys, goff, G, NPu, keys);
      SME_CHECK_LAUNCH();
      SME_HIP(hipEventRecord(e1, st));
      SME_HIP(hipStreamSynchronize(st));
    } catch (...) {
      (void)hipStreamSynchronize(st);  // kernels may still use the temporaries
      throw;
    }
  } else {
    SME_HIP(hipEventRecord(e1, st));
    SME_HIP(hipStreamSynchronize(st));
  }
  SME_HIP(hipEventElapsedTime(&ix->wild_ms, e0, e1));
  ix->wild_G = G;
  ix->wild_pairs = NPu;
  ix->wild_ready = true;
}

void expand_wildcards(sme_index *ix, const uint8_t *patterns, const int64_t *offs, int n, hipStream_t st) {
  sme_ctx *cx = ix->ctx;
  ix->wx_total = 0;
  // parse on the host: units, masks and gram keys of the batch as CSR
  std::vector<int32_t> uoff(n + 1, 0), goff(n + 1, 0);
  std::vector<uint16_t> units;
  std::vector<uint8_t> mask;
  std::vector<uint64_t> gkeys;
  {
    uint16_t u[wild::kMaxUnits];
    uint8_t m[wild::kMaxUnits];
    uint64_t k[wild::kMaxUnits];
    for (int i = 0; i < n; i++) {
      if (offs[i + 1] < offs[i]) throw Error(SME_EINVAL, "pattern offsets not ascending");
      int np = 0;
      const int rc = wild::parse_pattern(patterns + offs[i], offs[i + 1] - offs[i], u, m, &np);
      if (rc == wild::W_MALFORMED) throw Error(SME_EINVAL, "pattern " + std::to_string(i) + ": malformed UTF-8");
      if (rc == wild::W_TOO_LONG)
        throw Error(SME_ELIMIT, "pattern " + std::to_string(i) + ": more than 255 UTF-16 units");
      const int ng = wild::pattern_grams(u, m, np, k);
      if (units.size() + (size_t)np > (size_t)INT32_MAX)
        throw Error(SME_ELIMIT, "wildcard batch: 2^31 or more pattern units");
      units.insert(units.end(), u, u + np);
      mask.insert(mask.end(), m, m + np);
      gkeys.insert(gkeys.end(), k, k + ng);
      uoff[i + 1] = (int32_t)units.size();
      goff[i + 1] = (int32_t)gkeys.size();
    }
  }
  int64_t *d_moffs = ix->d_wx_off.as<int64_t>((size_t)n + 1);
  if (n == 0) {
    SME_HIP(hipMemsetAsync(d_moffs, 0, sizeof(int64_t), st));
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  if (!cx->opt_wild_scan) prepare_wildcards(ix, st);
  // one upload: gram keys | unit offsets | gram offsets | units | masks
  std::vector<uint8_t> blob;
  size_t a_key, a_uoff, a_goff, a_unit, a_mask;
  section<uint64_t>(blob, gkeys.size(), &a_key);
  section<int32_t>(blob, uoff.size(), &a_uoff);
  section<int32_t>(blob, goff.size(), &a_goff);
  section<uint16_t>(blob, units.size(), &a_unit);
  section<uint8_t>(blob, mask.size(), &a_mask);
  if (!gkeys.empty()) memcpy(blob.data() + a_key, gkeys.data(), gkeys.size() * sizeof(uint64_t));
  memcpy(blob.data() + a_uoff, uoff.data(), uoff.size() * sizeof(int32_t));
  memcpy(blob.data() + a_goff, goff.data(), goff.size() * sizeof(int32_t));
  if (!units.empty()) memcpy(blob.data() + a_unit, units.data(), units.size() * sizeof(uint16_t));
  if (!mask.empty()) memcpy(blob.data() + a_mask, mask.data(), mask.size());
  const uint8_t *d_in = ix->d_wx_in.as<uint8_t>(blob.size());
  const int chunk = (int)cx->opt_wild_chunk;
  const int64_t V = ix->V;
  try {
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    const Batch b{(const uint64_t *)(d_in + a_key), (const int32_t *)(d_in + a_uoff), (const int32_t *)(d_in + a_goff),
                  (const uint16_t *)(d_in + a_unit), d_in + a_mask};
    // per pattern: candidate range (2 x int32) and chunk offsets (int64)
    int32_t *cbeg = ix->d_wx_plan.as<int32_t>(2 * (size_t)n);
    int32_t *ccnt = cbeg + n;
    int64_t *choff = ix->d_wx_choff.as<int64_t>((size_t)n + 1);
    hipLaunchKernelGGL(k_wild_plan, dim3(grid_for(n + 1)), dim3(kNT), 0, st, b, n, (const uint64_t *)ix->d_wkeys.p,
                       (const int32_t *)ix->d_wgoff.p, cx->opt_wild_scan ? 0 : ix->wild_G, V, (int)cx->opt_wild_scan,
                       chunk, cbeg, ccnt, choff);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(choff, choff, (int64_t)n + 1, ix->d_wx_scan, st);
    int64_t NC = 0;
    SME_HIP(hipMemcpyAsync(&NC, choff + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    // matches per chunk, scanned in place (entry NC = all matches)
    int64_t *moff = ix->d_wx_moff.as<int64_t>((size_t)NC + 1);
    int64_t total = 0;
    const unsigned cgrid = (unsigned)std::max<int64_t>(1, std::min(NC, kMaxGrid));
    const int64_t *toff = (const int64_t *)ix->d_term_off.p;
    const uint16_t *tch = (const uint16_t *)ix->d_term_chars.p;
    const int32_t *gterm = (const int32_t *)ix->d_wgterm.p;
    SME_HIP(hipMemsetAsync(moff + NC, 0, sizeof(int64_t), st));
    if (NC > 0) {
      hipLaunchKernelGGL(k_wild_chunks<false>, dim3(cgrid), dim3(kNT), 0, st, b, n, (const int64_t *)choff, NC,
                         (const int32_t *)cbeg, (const int32_t *)ccnt, gterm, toff, tch, chunk, moff,
                         (const int64_t *)nullptr, (int32_t *)nullptr);
      SME_CHECK_LAUNCH();
      excl_scan<int64_t>(moff, moff, NC + 1, ix->d_wx_scan, st);
      SME_HIP(hipMemcpyAsync(&total, moff + NC, sizeof(int64_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
    }
    if (total >= (int64_t(1) << 31)) throw Error(SME_ELIMIT, "wildcard expansion: 2^31 or more matches in one batch");
    int32_t *ids = ix->d_wx_ids.as<int32_t>((size_t)total);
    if (total > 0) {
      hipLaunchKernelGGL(k_wild_chunks<true>, dim3(cgrid), dim3(kNT), 0, st, b, n, (const int64_t *)choff, NC,
                         (const int32_t *)cbeg, (const int32_t *)ccnt, gterm, toff, tch, chunk, (int64_t *)nullptr,
                         (const int64_t *)moff, ids);
      SME_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_wild_offs, dim3(grid_for(n + 1)), dim3(kNT), 0, st, (const int64_t *)choff,
                       (const int64_t *)moff, n, d_moffs);
    SME_CHECK_LAUNCH();
    SME_HIP(hipStreamSynchronize(st));
    ix->wx_total = total;
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the upload may still read `blob`
    throw;
  }
}

}  // namespace sme
