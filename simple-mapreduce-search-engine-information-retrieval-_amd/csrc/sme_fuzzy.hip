// sme_fuzzy.hip -- spelling suggestions: a batch of words -> per word the
// vocabulary terms within a small edit distance, ordered (distance asc, df desc,
// term id asc) and cut to the first m, over the character-trigram table of
// sme_wild.hip.
//
// k_fuzzy_plan picks per word the 3d + 1 distinct keys with the shortest posting
// lists (sme_fuzzy.hpp has the argument why their union holds every term within
// distance d), or the whole vocabulary for a word with fewer keys; the candidate
// ranges are cut into chunks, and the chunk filter of sme_chunks.hpp -- once
// counting, once emitting -- length-filters every candidate, verifies it with the
// bit-parallel distance and drops a match an earlier list of the word also holds
// (FuzzyOp), one workgroup per chunk, one candidate per thread.  Two stable sorts
// (by the in-word order key, then by word) and a gather order and cut the matches.
// Every candidate is verified: the candidate source never changes a result.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sme_chunks.hpp"
#include "sme_fuzzy.hpp"
#include "sme_internal.hpp"

namespace sme {
namespace {
using namespace chunks;

struct Batch {           // the uploaded batch (device pointers into one block)
  const uint64_t *wkey;  // distinct keys of all words
  const int32_t *uoff;   // [n + 1] unit offsets
  const int32_t *koff;   // [n + 1] key offsets
  const uint16_t *unit;
};

// One thread per word; NL = 3d + 1 candidate ranges per word.  Range (i, j):
// lbeg < 0 = the term ids [0, lcnt), else gterm[lbeg .. lbeg + lcnt).  A word with
// NL or more distinct keys gets the NL shortest posting lists, shortest first (an
// absent key is an empty list); any other word range 0 = the whole vocabulary.
// kbeg / kcnt: scratch, one entry per uploaded key.  *cands += the word's candidates.
__global__ void k_fuzzy_plan(Batch b, int n, int NL, const uint64_t *__restrict__ keys,
                             const int32_t *__restrict__ goff, int64_t G, int64_t V, int scan, int chunk,
                             int32_t *__restrict__ kbeg, int32_t *__restrict__ kcnt, int32_t *__restrict__ lbeg,
                             int32_t *__restrict__ lcnt, int64_t *__restrict__ nchunk,
                             unsigned long long *__restrict__ cands) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
    if (i == n) {
      nchunk[(int64_t)n * NL] = 0;
      continue;
    }
    const int k0 = b.koff[i], nk = b.koff[i + 1] - k0;
    const int64_t r0 = (int64_t)i * NL;
    if (scan || nk < NL) {
      for (int j = 0; j < NL; j++) {
        lbeg[r0 + j] = j == 0 ? -1 : 0;
        lcnt[r0 + j] = j == 0 ? (int32_t)V : 0;
        nchunk[r0 + j] = j == 0 ? (V + chunk - 1) / chunk : 0;
      }
      atomicAdd(cands, (unsigned long long)V);
      continue;
    }
    for (int g = 0; g < nk; g++) {
      const GramRange p = gram_postings(keys, goff, G, b.wkey[k0 + g]);
      kbeg[k0 + g] = p.beg;
      kcnt[k0 + g] = p.cnt;
    }
    // selection by (count, key index) ascending: each pass takes the smallest entry
    // past the last one taken
    int pc = -1, pg = -1;
    unsigned long long sum = 0;
    for (int j = 0; j < NL; j++) {
      int bc = 0, bg = -1;
      for (int g = 0; g < nk; g++) {
        const int c = kcnt[k0 + g];
        if (c < pc || (c == pc && g <= pg)) continue;
        if (bg < 0 || c < bc) {
          bc = c;
          bg = g;
        }
      }
      lbeg[r0 + j] = kbeg[k0 + bg];
      lcnt[r0 + j] = bc;
      nchunk[r0 + j] = ((int64_t)bc + chunk - 1) / chunk;
      sum += (unsigned long long)bc;
      pc = bc;
      pg = bg;
    }
    atomicAdd(cands, sum);
  }
}

// is t in the ascending ids g[0 .. n)?
__device__ __forceinline__ bool list_holds(const int32_t *__restrict__ g, int n, int32_t t) {
  const int at = lower_bound(g, n, t);
  return at < n && g[at] == t;
}

// The chunk filter's Op (sme_chunks.hpp): range r = list r % NL of word r / NL,
// candidate c of it the term id c (beg < 0) or gterm[beg + c].  The word and its
// Peq (distinct units ascending, one position mask each, a direct table for units
// below 128 beside them) are staged in LDS.  A candidate: length filter from
// term_off alone, then the bit-parallel distance, and a match of list j that also
// lies in one of the word's lists before j is dropped (a binary search each, the
// lists are sorted), so a term is emitted once per word.  Matches are rare, so
// searching the lists for the matches only beat searching them for every candidate
// before the distance (DESIGN 4e has the two times).  Emitted: the match's in-word
// order key dist << 62 | (0x7FFFFFFF - df) << 31 | term id, and its word.
struct FuzzyOp {
  Batch b;
  int NL, d;
  const int32_t *lbeg;
  const int32_t *lcnt;
  const int32_t *gterm;
  const int64_t *toff;
  const uint16_t *tch;
  const int64_t *doff;
  struct Lds {
    uint64_t pm[fuzzy::kMaxUnits];
    uint64_t direct[128];
    uint16_t unit[fuzzy::kMaxUnits];
    uint16_t su[fuzzy::kMaxUnits];
    int nd;
  };
  struct Chunk {
    int i, lj, Lw, nd;
    int32_t beg;
  };
  struct Cand {
    int32_t t;
    int dist;
  };
  __device__ __forceinline__ bool stage(Lds &s, Chunk &k, int64_t r, int64_t, int) const {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    k.i = (int)(r / NL);
    k.lj = (int)(r % NL);
    const int u0 = b.uoff[k.i], Lw = b.uoff[k.i + 1] - u0;  // Lw <= 64 (host parse)
    if (tid < Lw) s.unit[tid] = b.unit[u0 + tid];
    if (tid < 128) s.direct[tid] = 0;
    __syncthreads();
    if (wv == 0) {
      // Lw <= 64: wave 0's lane l is word position l.  Its unit's position mask;
      // the lane is the unit's first position if no lower bit is set; the unit's
      // rank is the count of first positions with a smaller unit.
      const bool on = lane < Lw;
      const uint16_t u = on ? s.unit[lane] : 0;
      uint64_t mask = 0;
      for (int j = 0; j < Lw; j++) mask |= (uint64_t)(s.unit[j] == u) << j;
      const bool first = on && (mask & ((1ull << lane) - 1)) == 0;
      const unsigned long long fm = __ballot(first);
      int rank = 0;
      for (int j = 0; j < Lw; j++) rank += ((fm >> j) & 1) && s.unit[j] < u ? 1 : 0;
      if (first) {
        s.su[rank] = u;
        s.pm[rank] = mask;
        if (u < 128) s.direct[u] = mask;
      }
      if (lane == 0) s.nd = __popcll(fm);
    }
    __syncthreads();
    k.Lw = Lw;
    k.nd = s.nd;
    k.beg = lbeg[r];
    return true;
  }
  __device__ __forceinline__ bool test(const Lds &s, const Chunk &k, int64_t r, int64_t c, Cand &x) const {
    x.t = k.beg < 0 ? (int32_t)c : gterm[k.beg + c];
    const int64_t a = toff[x.t];
    const int Lt = (int)min(toff[x.t + 1] - a, (int64_t)(2 * fuzzy::kMaxUnits));
    bool hit = false;
    if (Lt - k.Lw <= d && k.Lw - Lt <= d) {
      x.dist = k.Lw == 0 ? Lt : fuzzy::distance_peq(s.su, s.pm, k.nd, s.direct, k.Lw, tch + a, Lt, d);
      hit = x.dist <= d;
    }
    for (int jj = 0; hit && jj < k.lj; jj++) hit = !list_holds(gterm + lbeg[r - k.lj + jj], lcnt[r - k.lj + jj], x.t);
    return hit;
  }
  __device__ __forceinline__ void emit(const Lds &, const Chunk &k, int64_t, const Cand &x, int64_t at,
                                       uint64_t *__restrict__ mkey, uint32_t *__restrict__ mword) const {
    const uint64_t df = (uint64_t)(doff[x.t + 1] - doff[x.t]);
    mkey[at] = (uint64_t)x.dist << 62 | (uint64_t)(0x7FFFFFFFu - (uint32_t)df) << 31 | (uint64_t)(uint32_t)x.t;
    mword[at] = (uint32_t)k.i;
  }
};
struct FirstRange {  // word i's first range
  int NL;
  __device__ int64_t operator()(int64_t i) const { return i * NL; }
};

__global__ void k_fuzzy_iota(uint32_t *__restrict__ v, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    v[i] = (uint32_t)i;
}
// Sorted match x (word w[x], the perm[x]-th key of the key-sorted matches) is the
// (x - woff[w])-th of its word: kept if that is below the cut.
__global__ void k_fuzzy_gather(const uint32_t *__restrict__ w, const uint32_t *__restrict__ perm,
                               const uint64_t *__restrict__ key, int64_t total, const int64_t *__restrict__ woff,
                               const int64_t *__restrict__ soff, int64_t m, int32_t *__restrict__ ids,
                               uint8_t *__restrict__ dist) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t i = w[x];
    const int64_t rk = x - woff[i];
    if (m > 0 && rk >= m) continue;
    const uint64_t k = key[perm[x]];
    ids[soff[i] + rk] = (int32_t)(k & 0x7FFFFFFFu);
    dist[soff[i] + rk] = (uint8_t)(k >> 62);
  }
}
}  // namespace

void suggest_terms(sme_index *ix, const uint8_t *words, const int64_t *offs, int n, int max_dist, int m,
                   hipStream_t st) {
  sme_ctx *cx = ix->ctx;
  TermDists &out = ix->fz;
  out.reset();
  ix->fz_scanned = 0;
  const int NL = fuzzy::lists_for(max_dist);
  const bool scan = cx->opt_fuzzy_scan != 0;
  // parse on the host: units and distinct keys of the batch as CSR
  std::vector<int32_t> uoff(n + 1, 0), koff(n + 1, 0);
  std::vector<uint16_t> units;
  std::vector<uint64_t> wkeys;
  uint64_t scanned = 0;
  {
    uint16_t u[wild::kMaxUnits];
    uint8_t scratch[wild::kMaxUnits];
    uint64_t k[fuzzy::kMaxUnits];
    for (int i = 0; i < n; i++) {
      if (offs[i + 1] < offs[i]) throw Error(SME_EINVAL, "word offsets not ascending");
      int nu = 0;
      const int rc = fuzzy::parse_word(words + offs[i], offs[i + 1] - offs[i], u, scratch, &nu);
      if (rc == fuzzy::F_MALFORMED) throw Error(SME_EINVAL, "word " + std::to_string(i) + ": malformed UTF-8");
      if (rc == fuzzy::F_TOO_LONG)
        throw Error(SME_ELIMIT, "word " + std::to_string(i) + ": more than 64 UTF-16 units");
      const int nk = fuzzy::distinct_keys(u, nu, k);
      if (units.size() + (size_t)nu > (size_t)INT32_MAX)
        throw Error(SME_ELIMIT, "suggestion batch: 2^31 or more word units");
      units.insert(units.end(), u, u + nu);
      wkeys.insert(wkeys.end(), k, k + nk);
      uoff[i + 1] = (int32_t)units.size();
      koff[i + 1] = (int32_t)wkeys.size();
      scanned += (scan || nk < NL) ? 1 : 0;
    }
  }
  int64_t *d_soff = out.offsets(n);
  if (n == 0) {
    SME_HIP(hipMemsetAsync(d_soff, 0, sizeof(int64_t), st));
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  if ((int64_t)n * NL >= (int64_t(1) << 31)) throw Error(SME_ELIMIT, "suggestion batch: 2^31 or more candidate ranges");
  if (!scan) prepare_wildcards(ix, st);
  // one upload: word keys | unit offsets | key offsets | units
  Blob blob;
  const size_t a_key = blob.add(wkeys.data(), wkeys.size());
  const size_t a_uoff = blob.add(uoff.data(), uoff.size());
  const size_t a_koff = blob.add(koff.data(), koff.size());
  const size_t a_unit = blob.add(units.data(), units.size());
  const int chunk = (int)cx->opt_wild_chunk;
  const int64_t V = ix->V, R = (int64_t)n * NL;
  // temporaries of this call: pooled blocks, back in the pool on return
  DevBuf in, kscr, plan, chb, mob, cnd, wob, kpb, scn, ka, kb, wa, wb, pa, pb, wk, radix;
  for (DevBuf *b : {&in, &kscr, &plan, &chb, &mob, &cnd, &wob, &kpb, &scn, &ka, &kb, &wa, &wb, &pa, &pb, &wk, &radix})
    b->pool = &cx->pool;
  try {
    const uint8_t *d_in = in.as<uint8_t>(blob.bytes.size());
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st));
    const Batch b{(const uint64_t *)(d_in + a_key), (const int32_t *)(d_in + a_uoff), (const int32_t *)(d_in + a_koff),
                  (const uint16_t *)(d_in + a_unit)};
    int32_t *kbeg = kscr.as<int32_t>(2 * wkeys.size() + 2);
    int32_t *kcnt = kbeg + wkeys.size() + 1;
    int32_t *lbeg = plan.as<int32_t>(2 * (size_t)R);
    int32_t *lcnt = lbeg + R;
    int64_t *choff = chb.as<int64_t>((size_t)R + 1);
    unsigned long long *d_cands = cnd.as<unsigned long long>(1);
    SME_HIP(hipMemsetAsync(d_cands, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_fuzzy_plan, dim3(grid_for(n + 1)), dim3(kNT), 0, st, b, n, NL, (const uint64_t *)ix->d_wkeys.p,
                       (const int32_t *)ix->d_wgoff.p, scan ? 0 : ix->wild_G, V, (int)scan, chunk, kbeg, kcnt, lbeg,
                       lcnt, choff, d_cands);
    SME_CHECK_LAUNCH();
    unsigned long long cands = 0;
    const FuzzyOp op{b, NL, max_dist, lbeg, lcnt, (const int32_t *)ix->d_wgterm.p, (const int64_t *)ix->d_term_off.p,
                     (const uint16_t *)ix->d_term_chars.p, (const int64_t *)ix->d_off.p};
    const Counted c = count_chunks(op, (int)R, choff, lcnt, chunk, mob, scn,
                                   "suggestions: 2^31 or more matches in one batch", st, d_cands, &cands);
    const int64_t total = c.total;
    int64_t *woff = wob.as<int64_t>((size_t)n + 1);
    int64_t *kept = kpb.as<int64_t>((size_t)n + 1);
    hipLaunchKernelGGL(k_owner_offs<FirstRange>, dim3(grid_for(n + 1)), dim3(kNT), 0, st, FirstRange{NL}, c.choff,
                       c.moff, (int64_t)n, woff);
    hipLaunchKernelGGL(k_cut, dim3(grid_for(n + 1)), dim3(kNT), 0, st, (const int64_t *)woff, (int64_t)n, (int64_t)m,
                       kept);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(kept, d_soff, (int64_t)n + 1, scn, st);
    int64_t out_total = 0;
    SME_HIP(hipMemcpyAsync(&out_total, d_soff + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    int32_t *ids = out.alloc<TermDists::ids>(out_total);
    uint8_t *dist = out.alloc<TermDists::dist>(out_total);
    if (total > 0) {
      uint64_t *key0 = ka.as<uint64_t>((size_t)total), *key1 = kb.as<uint64_t>((size_t)total);
      uint32_t *w0 = wa.as<uint32_t>((size_t)total), *w1 = wb.as<uint32_t>((size_t)total);
      uint32_t *p0 = pa.as<uint32_t>((size_t)total), *p1 = pb.as<uint32_t>((size_t)total);
      uint32_t *w2 = wk.as<uint32_t>((size_t)total);
      emit_chunks(op, c, st, key0, w0);
      // the whole in-word order is one 64-bit key; then a stable sort by word
      sort_pairs<uint64_t>(key0, key1, w0, w1, total, 64, radix, st);
      hipLaunchKernelGGL(k_fuzzy_iota, dim3(grid_for(total)), dim3(kNT), 0, st, p0, total);
      sort_pairs<uint32_t>(w1, w2, p0, p1, total, owner_bits(n), radix, st);
      hipLaunchKernelGGL(k_fuzzy_gather, dim3(grid_for(total)), dim3(kNT), 0, st, (const uint32_t *)w2,
                         (const uint32_t *)p1, (const uint64_t *)key1, total, (const int64_t *)woff,
                         (const int64_t *)d_soff, (int64_t)m, ids, dist);
      SME_CHECK_LAUNCH();
    }
    SME_HIP(hipStreamSynchronize(st));
    out.total = out_total;
    out.cands = (uint64_t)cands;
    ix->fz_scanned = scanned;
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the upload may still read `blob`, kernels the temporaries
    throw;
  }
}

}  // namespace sme
