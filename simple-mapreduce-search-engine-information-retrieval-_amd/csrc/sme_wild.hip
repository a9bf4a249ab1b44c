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
// the chunk filter of sme_chunks.hpp -- once counting, once emitting -- verifies
// every candidate with wild_match (WildOp), one workgroup per chunk: the candidate
// source never changes the result.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sme_chunks.hpp"
#include "sme_internal.hpp"
#include "sme_wild.hpp"

namespace sme {
namespace {
using namespace chunks;

// ---- table build ------------------------------------------------------------
// A term of L units has L windows, so the windows' exclusive scan is the term
// offsets themselves: window w (0 <= w < NP) is the unit at toff[0] + w, and its
// term the last one starting at or before it (terms of 0 units own no window).
__global__ void k_wt_pairs(const int64_t *__restrict__ toff, const uint16_t *__restrict__ tch, int64_t V, int64_t NP,
                           uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const int64_t base = toff[0];
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < NP; w += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pos = base + w;
    const int64_t t = upper_bound(toff, V, pos) - 1, b = toff[t];
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
        const GramRange p = gram_postings(keys, goff, G, b.gkey[g]);
        if (p.cnt == 0) {  // a trigram no term holds: no match
          beg = 0;
          cnt = 0;
          break;
        }
        if (beg < 0 || p.cnt < cnt) {
          beg = p.beg;
          cnt = p.cnt;
        }
      }
    }
    cbeg[i] = beg;
    ccnt[i] = cnt;
    nchunk[i] = ((int64_t)cnt + chunk - 1) / chunk;
  }
}

// The chunk filter's Op (sme_chunks.hpp): range = pattern, candidate c of it the
// term id c (beg < 0) or gterm[beg + c].  The pattern is staged in LDS, a hit is a
// term wild_match accepts, and its term id is emitted: ids come out ascending.
struct WildOp {
  Batch b;
  const int32_t *cbeg;
  const int32_t *gterm;
  const int64_t *toff;
  const uint16_t *tch;
  struct Lds {
    uint16_t unit[256];
    uint8_t mask[256];
  };
  struct Chunk {
    int np;
    int32_t beg;
  };
  struct Cand {
    int32_t t;
  };
  __device__ __forceinline__ bool stage(Lds &s, Chunk &k, int64_t i, int64_t, int) const {
    const int tid = threadIdx.x;
    const int u0 = b.uoff[i];
    k.np = b.uoff[i + 1] - u0;
    k.beg = cbeg[i];
    if (tid < k.np) {
      s.unit[tid] = b.unit[u0 + tid];
      s.mask[tid] = b.mask[u0 + tid];
    }
    __syncthreads();
    return true;
  }
  __device__ __forceinline__ bool test(const Lds &s, const Chunk &k, int64_t, int64_t c, Cand &x) const {
    x.t = k.beg < 0 ? (int32_t)c : gterm[k.beg + c];
    const int64_t a = toff[x.t];
    return wild::wild_match(s.unit, s.mask, k.np, tch + a, (int)(toff[x.t + 1] - a));
  }
  __device__ __forceinline__ void emit(const Lds &, const Chunk &, int64_t, const Cand &x, int64_t at,
                                       int32_t *__restrict__ ids) const {
    ids[at] = x.t;
  }
};
struct FirstRange {  // pattern i's first (and only) range
  __device__ int64_t operator()(int64_t i) const { return i; }
};
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
  TermIds &out = ix->wx;
  out.reset();
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
  int64_t *d_moffs = out.offsets(n);
  if (n == 0) {
    SME_HIP(hipMemsetAsync(d_moffs, 0, sizeof(int64_t), st));
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  if (!cx->opt_wild_scan) prepare_wildcards(ix, st);
  // one upload: gram keys | unit offsets | gram offsets | units | masks
  Blob blob;
  const size_t a_key = blob.add(gkeys.data(), gkeys.size());
  const size_t a_uoff = blob.add(uoff.data(), uoff.size());
  const size_t a_goff = blob.add(goff.data(), goff.size());
  const size_t a_unit = blob.add(units.data(), units.size());
  const size_t a_mask = blob.add(mask.data(), mask.size());
  const uint8_t *d_in = ix->d_wx_in.as<uint8_t>(blob.bytes.size());
  const int chunk = (int)cx->opt_wild_chunk;
  const int64_t V = ix->V;
  try {
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st));
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
    const WildOp op{b, cbeg, (const int32_t *)ix->d_wgterm.p, (const int64_t *)ix->d_term_off.p,
                    (const uint16_t *)ix->d_term_chars.p};
    const Counted c = count_chunks(op, n, choff, ccnt, chunk, ix->d_wx_moff, ix->d_wx_scan,
                                   "wildcard expansion: 2^31 or more matches in one batch", st);
    emit_chunks(op, c, st, out.alloc<TermIds::ids>(c.total));
    hipLaunchKernelGGL(k_owner_offs<FirstRange>, dim3(grid_for(n + 1)), dim3(kNT), 0, st, FirstRange{}, c.choff,
                       c.moff, (int64_t)n, d_moffs);
    SME_CHECK_LAUNCH();
    SME_HIP(hipStreamSynchronize(st));
    out.total = c.total;
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the upload may still read `blob`
    throw;
  }
}

}  // namespace sme
