// sme_fuzzy.hip -- spelling suggestions: a batch of words -> per word the
// vocabulary terms within a small edit distance, ordered (distance asc, df desc,
// term id asc) and cut to the first m, over the character-trigram table of
// sme_wild.hip.
//
// k_fuzzy_plan picks per word the 3d + 1 distinct keys with the shortest posting
// lists (sme_fuzzy.hpp has the argument why their union holds every term within
// distance d), or the whole vocabulary for a word with fewer keys; the candidate
// ranges are cut into chunks, and k_fuzzy_chunks -- once counting, once emitting --
// length-filters every candidate, verifies it with the bit-parallel distance and
// drops a match an earlier list of the word also holds, one workgroup per chunk,
// one candidate per thread.  Two stable sorts
// (by the in-word order key, then by word) and a gather order and cut the matches.
// Every candidate is verified: the candidate source never changes a result.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sme_fuzzy.hpp"
#include "sme_internal.hpp"

namespace sme {
namespace {
constexpr int kNT = 256;  // threads of the chunk kernels
constexpr int64_t kMaxGrid = 1 << 20;

unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kNT - 1) / kNT, 65536)); }

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
      const uint64_t k = b.wkey[k0 + g];
      int64_t lo = 0, hi = G;  // first key >= k
      while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (keys[m] < k)
          lo = m + 1;
        else
          hi = m;
      }
      const bool have = lo < G && keys[lo] == k;
      kbeg[k0 + g] = have ? goff[lo] : 0;
      kcnt[k0 + g] = have ? goff[lo + 1] - goff[lo] : 0;
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

// The chunk's range: the last one whose first chunk is at or before `ch` (ranges
// without candidates own no chunk).
__device__ __forceinline__ int64_t chunk_range(const int64_t *__restrict__ choff, int64_t R, int64_t ch) {
  int64_t lo = 0, hi = R;  // first range with choff > ch
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (choff[m] <= ch)
      lo = m + 1;
    else
      hi = m;
  }
  return lo - 1;
}

// is t in the ascending ids g[0 .. n)?
__device__ __forceinline__ bool list_holds(const int32_t *__restrict__ g, int n, int32_t t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (g[m] < t)
      lo = m + 1;
    else
      hi = m;
  }
  return lo < n && g[lo] == t;
}

// One workgroup per chunk (grid-stride over the chunks).  The word and its Peq
// (distinct units ascending, one position mask each, a direct table for units
// below 128 beside them) are staged in LDS; the chunk's candidates are taken kNT
// at a time, one per thread: length filter from term_off alone, then the
// bit-parallel distance, and a match of list j that also lies in one of the
// word's lists before j is dropped (a binary search each, the lists are sorted),
// so a term is emitted once per word.  Matches are rare, so searching the lists
// for the matches only beat searching them for every candidate before the
// distance (DESIGN 4e has the two times).
// EMIT = false: mcnt[ch] = matches of the chunk.  EMIT = true: at moff[ch] + rank
// (rank from the waves' ballots) the match's in-word order key
// dist << 62 | (0x7FFFFFFF - df) << 31 | term id, and its word.
template <bool EMIT>
__global__ __launch_bounds__(kNT) void k_fuzzy_chunks(Batch b, int NL, int64_t R, const int64_t *__restrict__ choff,
                                                      int64_t NC, const int32_t *__restrict__ lbeg,
                                                      const int32_t *__restrict__ lcnt,
                                                      const int32_t *__restrict__ gterm,
                                                      const int64_t *__restrict__ toff,
                                                      const uint16_t *__restrict__ tch,
                                                      const int64_t *__restrict__ doff, int chunk, int d,
                                                      int64_t *__restrict__ mcnt, const int64_t *__restrict__ moff,
                                                      uint64_t *__restrict__ mkey, uint32_t *__restrict__ mword) {
  __shared__ uint16_t s_unit[fuzzy::kMaxUnits];
  __shared__ uint16_t s_su[fuzzy::kMaxUnits];
  __shared__ uint64_t s_pm[fuzzy::kMaxUnits];
  __shared__ uint64_t s_direct[128];
  __shared__ int s_nd;
  __shared__ int s_wsum[kNT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int64_t ch = blockIdx.x; ch < NC; ch += gridDim.x) {
    const int64_t r = chunk_range(choff, R, ch);
    const int i = (int)(r / NL), lj = (int)(r % NL);
    const int u0 = b.uoff[i], Lw = b.uoff[i + 1] - u0;  // Lw <= 64 (host parse)
    if (tid < Lw) s_unit[tid] = b.unit[u0 + tid];
    if (tid < 128) s_direct[tid] = 0;
    __syncthreads();
    if (wv == 0) {
      // Lw <= 64: wave 0's lane l is word position l.  Its unit's position mask;
      // the lane is the unit's first position if no lower bit is set; the unit's
      // rank is the count of first positions with a smaller unit.
      const bool on = lane < Lw;
      const uint16_t u = on ? s_unit[lane] : 0;
      uint64_t mask = 0;
      for (int j = 0; j < Lw; j++) mask |= (uint64_t)(s_unit[j] == u) << j;
      const bool first = on && (mask & ((1ull << lane) - 1)) == 0;
      const unsigned long long fm = __ballot(first);
      int rank = 0;
      for (int j = 0; j < Lw; j++) rank += ((fm >> j) & 1) && s_unit[j] < u ? 1 : 0;
      if (first) {
        s_su[rank] = u;
        s_pm[rank] = mask;
        if (u < 128) s_direct[u] = mask;
      }
      if (lane == 0) s_nd = __popcll(fm);
    }
    __syncthreads();
    const int nd = s_nd;
    const int32_t beg = lbeg[r];
    const int64_t c0 = (ch - choff[r]) * chunk;
    const int len = (int)min((int64_t)chunk, (int64_t)lcnt[r] - c0);
    int64_t run = EMIT ? moff[ch] : 0;  // matches of the rounds before
    for (int rd = 0; rd < len; rd += kNT) {
      const int c = rd + tid;
      bool hit = false;
      int32_t t = 0;
      int dist = 0;
      if (c < len) {
        t = beg < 0 ? (int32_t)(c0 + c) : gterm[beg + c0 + c];
        const int64_t a = toff[t];
        const int Lt = (int)min(toff[t + 1] - a, (int64_t)(2 * fuzzy::kMaxUnits));
        if (Lt - Lw <= d && Lw - Lt <= d) {
          dist = Lw == 0 ? Lt : fuzzy::distance_peq(s_su, s_pm, nd, s_direct, Lw, tch + a, Lt, d);
          hit = dist <= d;
        }
        for (int jj = 0; hit && jj < lj; jj++)
          hit = !list_holds(gterm + lbeg[r - lj + jj], lcnt[r - lj + jj], t);
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
      if (EMIT && hit) {
        const int64_t at = run + before + __popcll(m & ((1ull << lane) - 1));
        const uint64_t df = (uint64_t)(doff[t + 1] - doff[t]);
        mkey[at] = (uint64_t)dist << 62 | (uint64_t)(0x7FFFFFFFu - (uint32_t)df) << 31 | (uint64_t)(uint32_t)t;
        mword[at] = (uint32_t)i;
      }
      run += total;
      __syncthreads();  // s_wsum (and, after the last round, the staged word) is rewritten
    }
    if (!EMIT && tid == 0) mcnt[ch] = run;
  }
}

// woff[i] = matches before word i's first chunk (i = n: all of them)
__global__ void k_fuzzy_offs(const int64_t *__restrict__ choff, const int64_t *__restrict__ moff, int n, int NL,
                             int64_t *__restrict__ woff) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x)
    woff[i] = moff[choff[(int64_t)i * NL]];
}
// kept[i] = word i's matches after the cut (m = 0: no cut); kept[n] = 0
__global__ void k_fuzzy_cut(const int64_t *__restrict__ woff, int n, int64_t m, int64_t *__restrict__ kept) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
    const int64_t c = i < n ? woff[i + 1] - woff[i] : 0;
    kept[i] = m > 0 && c > m ? m : c;
  }
}
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

// appends an aligned section of `count` T to the upload blob; *at = its byte offset
template <typename T>
void section(std::vector<uint8_t> &blob, size_t count, size_t *at) {
  const size_t a = (blob.size() + alignof(T) - 1) / alignof(T) * alignof(T);
  blob.resize(a + count * sizeof(T));
  *at = a;
}
}  // namespace

void suggest_terms(sme_index *ix, const uint8_t *words, const int64_t *offs, int n, int max_dist, int m,
                   hipStream_t st) {
  sme_ctx *cx = ix->ctx;
  ix->fz_total = 0;
  ix->fz_scanned = 0;
  ix->fz_cands = 0;
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
  int64_t *d_soff = ix->d_fz_off.as<int64_t>((size_t)n + 1);
  if (n == 0) {
    SME_HIP(hipMemsetAsync(d_soff, 0, sizeof(int64_t), st));
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  if ((int64_t)n * NL >= (int64_t(1) << 31)) throw Error(SME_ELIMIT, "suggestion batch: 2^31 or more candidate ranges");
  if (!scan) prepare_wildcards(ix, st);
  // one upload: word keys | unit offsets | key offsets | units
  std::vector<uint8_t> blob;
  size_t a_key, a_uoff, a_koff, a_unit;
  section<uint64_t>(blob, wkeys.size(), &a_key);
  section<int32_t>(blob, uoff.size(), &a_uoff);
  section<int32_t>(blob, koff.size(), &a_koff);
  section<uint16_t>(blob, units.size(), &a_unit);
  if (!wkeys.empty()) memcpy(blob.data() + a_key, wkeys.data(), wkeys.size() * sizeof(uint64_t));
  memcpy(blob.data() + a_uoff, uoff.data(), uoff.size() * sizeof(int32_t));
  memcpy(blob.data() + a_koff, koff.data(), koff.size() * sizeof(int32_t));
  if (!units.empty()) memcpy(blob.data() + a_unit, units.data(), units.size() * sizeof(uint16_t));
  const int chunk = (int)cx->opt_wild_chunk;
  const int64_t V = ix->V, R = (int64_t)n * NL;
  // temporaries of this call: pooled blocks, back in the pool on return
  DevBuf in, kscr, plan, chb, mob, cnd, wob, kpb, scn, ka, kb, wa, wb, pa, pb, wk, radix;
  for (DevBuf *b : {&in, &kscr, &plan, &chb, &mob, &cnd, &wob, &kpb, &scn, &ka, &kb, &wa, &wb, &pa, &pb, &wk, &radix})
    b->pool = &cx->pool;
  try {
    const uint8_t *d_in = in.as<uint8_t>(blob.size());
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
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
    excl_scan<int64_t>(choff, choff, R + 1, scn, st);
    int64_t NC = 0;
    unsigned long long cands = 0;
    SME_HIP(hipMemcpyAsync(&NC, choff + R, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipMemcpyAsync(&cands, d_cands, sizeof(cands), hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    // matches per chunk, scanned in place (entry NC = all matches)
    int64_t *moff = mob.as<int64_t>((size_t)NC + 1);
    int64_t total = 0;
    const unsigned cgrid = (unsigned)std::max<int64_t>(1, std::min(NC, kMaxGrid));
    const int64_t *toff = (const int64_t *)ix->d_term_off.p;
    const uint16_t *tch = (const uint16_t *)ix->d_term_chars.p;
    const int32_t *gterm = (const int32_t *)ix->d_wgterm.p;
    const int64_t *doff = (const int64_t *)ix->d_off.p;
    SME_HIP(hipMemsetAsync(moff + NC, 0, sizeof(int64_t), st));
    if (NC > 0) {
      hipLaunchKernelGGL(k_fuzzy_chunks<false>, dim3(cgrid), dim3(kNT), 0, st, b, NL, R, (const int64_t *)choff, NC,
                         (const int32_t *)lbeg, (const int32_t *)lcnt, gterm, toff, tch, doff, chunk, max_dist, moff,
                         (const int64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
      SME_CHECK_LAUNCH();
      excl_scan<int64_t>(moff, moff, NC + 1, scn, st);
      SME_HIP(hipMemcpyAsync(&total, moff + NC, sizeof(int64_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
    }
    if (total >= (int64_t(1) << 31)) throw Error(SME_ELIMIT, "suggestions: 2^31 or more matches in one batch");
    int64_t *woff = wob.as<int64_t>((size_t)n + 1);
    int64_t *kept = kpb.as<int64_t>((size_t)n + 1);
    hipLaunchKernelGGL(k_fuzzy_offs, dim3(grid_for(n + 1)), dim3(kNT), 0, st, (const int64_t *)choff,
                       (const int64_t *)moff, n, NL, woff);
    hipLaunchKernelGGL(k_fuzzy_cut, dim3(grid_for(n + 1)), dim3(kNT), 0, st, (const int64_t *)woff, n, (int64_t)m,
                       kept);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(kept, d_soff, (int64_t)n + 1, scn, st);
    int64_t out_total = 0;
    SME_HIP(hipMemcpyAsync(&out_total, d_soff + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    int32_t *ids = ix->d_fz_ids.as<int32_t>((size_t)out_total);
    uint8_t *dist = ix->d_fz_dist.as<uint8_t>((size_t)out_total);
    if (total > 0) {
      uint64_t *key0 = ka.as<uint64_t>((size_t)total), *key1 = kb.as<uint64_t>((size_t)total);
      uint32_t *w0 = wa.as<uint32_t>((size_t)total), *w1 = wb.as<uint32_t>((size_t)total);
      uint32_t *p0 = pa.as<uint32_t>((size_t)total), *p1 = pb.as<uint32_t>((size_t)total);
      uint32_t *w2 = wk.as<uint32_t>((size_t)total);
      hipLaunchKernelGGL(k_fuzzy_chunks<true>, dim3(cgrid), dim3(kNT), 0, st, b, NL, R, (const int64_t *)choff, NC,
                         (const int32_t *)lbeg, (const int32_t *)lcnt, gterm, toff, tch, doff, chunk, max_dist,
                         (int64_t *)nullptr, (const int64_t *)moff, key0, w0);
      SME_CHECK_LAUNCH();
      // the whole in-word order is one 64-bit key; then a stable sort by word
      sort_pairs<uint64_t>(key0, key1, w0, w1, total, 64, radix, st);
      hipLaunchKernelGGL(k_fuzzy_iota, dim3(grid_for(total)), dim3(kNT), 0, st, p0, total);
      int wbits = 1;
      while (wbits < 32 && (int64_t(1) << wbits) < n) wbits++;
      sort_pairs<uint32_t>(w1, w2, p0, p1, total, wbits, radix, st);
      hipLaunchKernelGGL(k_fuzzy_gather, dim3(grid_for(total)), dim3(kNT), 0, st, (const uint32_t *)w2,
                         (const uint32_t *)p1, (const uint64_t *)key1, total, (const int64_t *)woff,
                         (const int64_t *)d_soff, (int64_t)m, ids, dist);
      SME_CHECK_LAUNCH();
    }
    SME_HIP(hipStreamSynchronize(st));
    ix->fz_total = out_total;
    ix->fz_scanned = scanned;
    ix->fz_cands = (uint64_t)cands;
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the upload may still read `blob`, kernels the temporaries
    throw;
  }
}

}  // namespace sme
