// sme_ixmerge.hip -- several indexes of one context into one full index
// (sme_index_merge; include/sme.h has the semantics, DESIGN.md 4k the pass).
//
//   terms      union_vocab (sme_vunion.hip, shared with sme_merge.hip): every input
//              term ranked among the other inputs' sorted term lists (String.compareTo);
//              equal strings are adjacent in rank order, sources in order.  A rank
//              position is a SEGMENT -- one input's posting list of one term -- and
//              the segments of a merged term are consecutive.  The per-input table
//              old id -> merged id falls out (the positions step rewrites with it).
//   postings   a true n-way merge of the segments' docno-ascending lists.  The
//              segments laid end to end are cut into tiles of "merge_tile"
//              postings; a tile boundary inside a term is found by the diagonal
//              search of sme_ixmerge.hpp and rounded down to a docno value, so the
//              equal docnos that become one posting never straddle tiles.  A tile is
//              one workgroup's: its pieces of every segment are staged in LDS, every
//              posting ranks itself among its term's other pieces there (searches
//              bounded by the tile), equal docnos are summed.  A count pass gives the
//              tiles' output sizes, one scan their places, an emit pass writes --
//              no temporary of the postings' size, and short terms share a tile.
//              Disjoint docno ranges: no merge, one flat copy (segments in range order).
//   tf order   tf_sort_segments, or sort_term_tf (a stable kv_sort) past kTfSortMaxTf
//   weights    reweight_index with N = sum N_i, one flat pass (term id per posting)
//   positions  the same tiled merge over the inputs' record docnos (exact cuts, no
//              summing), a scan of the record lengths, one flat gather of the streams
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>
#include <numeric>

#include "sme_internal.hpp"
#include "sme_ixmerge.hpp"
#include "sme_ixparts.hpp"

namespace sme {

namespace {

using namespace ixmerge;

constexpr int kNT = 256;

// the segments of a merge: ascending lists, grouped by merged term, the sources
// of a term in order
struct Segs {
  const int64_t *pstart;      // [nseg + 1] the lists laid end to end
  const int32_t *const *key;  // [nseg]
  const int32_t *const *val;  // [nseg], or null: the payload is the flat position pstart[r] + i
  const int32_t *gid;         // [nseg] merged term of a segment, or null: one term
  const int64_t *gstart;      // [G + 1] first segment of a merged term
  int64_t nseg, G, total;
};

// ---- tile boundaries ----------------------------------------------------------
// Boundary t lies at diagonal t * T of the segments laid end to end: inside merged
// term tg[t], before every element >= tv[t] but for the first ttake[t] elements
// equal to it (exact cuts; the postings merge cuts at the value: take 0).
// kNoValue: at the term's start.  Boundary ntiles is the end (term G).
struct ListOfTerm {
  const Segs &S;
  int64_t rs;
  __device__ void operator()(int s, const int32_t **p, int64_t *n) const {
    *p = S.key[rs + s];
    *n = S.pstart[rs + s + 1] - S.pstart[rs + s];
  }
};
__global__ void k_tile_bounds(Segs S, int T, int exact, int64_t ntiles, int32_t *tg, int64_t *tv, int64_t *ttake) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t <= ntiles; t += (int64_t)gridDim.x * blockDim.x) {
    if (t == ntiles) {
      tg[t] = (int32_t)S.G;
      tv[t] = kNoValue;
      ttake[t] = 0;
      continue;
    }
    const int64_t D = t * (int64_t)T;  // < S.total
    const int64_t r0 = last_le(S.pstart, 0, S.nseg + 1, D);
    const int64_t g = S.gid ? S.gid[r0] : 0, rs = S.gstart[g];
    const int k = (int)(S.gstart[g + 1] - rs);
    const int64_t d = D - S.pstart[rs];
    int64_t v = kNoValue, take = 0;
    if (d > 0) {
      int64_t before = 0;
      v = diagonal_value(ListOfTerm{S, rs}, k, d, &before);
      take = exact ? d - before : 0;
    }
    tg[t] = (int32_t)g;
    tv[t] = v;
    ttake[t] = take;
  }
}

// first index of the LDS run a[0, n) with a[i] >= v: bounded by the tile
__device__ __forceinline__ int lds_lower(const int32_t *a, int n, int64_t v) {
  int lo = 0, hi = n;
  for (int it = 0; it < 32 && lo < hi; it++) {
    const int m = (lo + hi) >> 1;
    if ((int64_t)a[m] < v)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}

// ---- the tile merge ----------------------------------------------------------------
// One workgroup per tile.  A tile holds the pieces of its first term (A: from the
// tile's boundary on), whole terms (M: a contiguous run of the segments laid end to
// end) and pieces of its last term (B: up to the next boundary); at most T + 63
// elements (cap = T + 64; a tile past it reports err[1] and writes nothing).
//   EMIT false  (dedup only) tile_cnt[t] = the tile's postings after equal docnos merge
//   EMIT true   writes them from tile_base[t] on (dedup: tf summed, the term id of
//               every posting, every term's offset, the largest tf; else: key and
//               payload of every element at t * T + rank)
template <bool EMIT>
__global__ __launch_bounds__(kNT) void k_tile_merge(Segs S, int T, int dedup, int64_t ntiles, const int32_t *tg,
                                                    const int64_t *tv, const int64_t *ttake, int64_t *tile_cnt,
                                                    const int64_t *tile_base, int32_t *okey, int32_t *oval,
                                                    uint32_t *oterm, int64_t *off, unsigned int *max_tf, int *err,
                                                    int64_t olimit) {
  extern __shared__ int32_t lds[];
  const int cap = T + 64;
  int32_t *in_key = lds, *in_val = lds + cap, *in_seg = lds + 2 * cap;
  int32_t *out_key = lds + 3 * cap, *out_val = lds + 4 * cap, *out_g = lds + 5 * cap;
  __shared__ int64_t sA_lo[64], sB_lo[64];
  __shared__ int32_t sA_n[64], sA_base[64], sB_n[64], sB_base[64];
  __shared__ int32_t s_nA, s_nB, s_afirst;
  __shared__ int s_scan[kNT / 64 + 1];
  const int tid = threadIdx.x;
  uint32_t mtf = 0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t g_a = tg[t], v_a = tv[t], take_a = ttake[t];
    const int64_t g_b = tg[t + 1], v_b = tv[t + 1], take_b = ttake[t + 1];
    const bool same = g_a == g_b;
    const int64_t rA = S.gstart[g_a];
    const int kA = (int)(S.gstart[g_a + 1] - rA);
    const int64_t rB = (!same && g_b < S.G) ? S.gstart[g_b] : 0;
    const int kB = (!same && g_b < S.G) ? (int)(S.gstart[g_b + 1] - rB) : 0;
    const int64_t rM0 = S.gstart[g_a + 1], rM1 = same ? rM0 : S.gstart[g_b];
    const int64_t pM0 = S.pstart[rM0];
    const int64_t nM64 = S.pstart[rM1] - pM0;
    if (tid < 64) {
      const int s = tid;
      const int32_t *p = nullptr;
      int64_t len = 0, eqa = 0, eqb = 0;
      if (s < kA) {
        p = S.key[rA + s];
        len = S.pstart[rA + s + 1] - S.pstart[rA + s];
        if (take_a > 0) eqa = lower_bound_i32(p, len, v_a + 1) - lower_bound_i32(p, len, v_a);
        if (same && take_b > 0) eqb = lower_bound_i32(p, len, v_b + 1) - lower_bound_i32(p, len, v_b);
      }
      const int64_t pa = wave_incl_sum(eqa) - eqa, pb = wave_incl_sum(eqb) - eqb;
      int64_t lo = 0, hi = 0;
      if (s < kA) {
        lo = cut_of(p, len, v_a, take_a, pa);
        hi = same ? cut_of(p, len, v_b, take_b, pb) : len;
      }
      int64_t n = hi > lo ? hi - lo : 0;
      if (n > cap + 1) n = cap + 1;  // (cannot be: the overflow test below then refuses the tile)
      const int64_t inc = wave_incl_sum(n), los = wave_incl_sum(lo);
      sA_lo[s] = lo;
      sA_n[s] = (int32_t)n;
      sA_base[s] = (int32_t)min(inc - n, (int64_t)cap + 1);
      if (s == 63) {
        s_nA = (int32_t)min(inc, (int64_t)cap + 1);
        s_afirst = los == 0;
      }
      // B: the last term's pieces up to the next boundary
      p = nullptr;
      len = 0;
      eqb = 0;
      if (s < kB) {
        p = S.key[rB + s];
        len = S.pstart[rB + s + 1] - S.pstart[rB + s];
        if (take_b > 0) eqb = lower_bound_i32(p, len, v_b + 1) - lower_bound_i32(p, len, v_b);
      }
      const int64_t qb = wave_incl_sum(eqb) - eqb;
      int64_t nb = s < kB ? cut_of(p, len, v_b, take_b, qb) : 0;
      if (nb > cap + 1) nb = cap + 1;
      const int64_t incb = wave_incl_sum(nb);
      sB_lo[s] = 0;
      sB_n[s] = (int32_t)nb;
      sB_base[s] = (int32_t)min(incb - nb, (int64_t)cap + 1);
      if (s == 63) s_nB = (int32_t)min(incb, (int64_t)cap + 1);
    }
    __syncthreads();
    const int nA = s_nA, nB = s_nB;
    const bool a_first = s_afirst != 0;
    const int64_t n64 = (int64_t)nA + nM64 + nB;
    if (n64 > cap || nM64 < 0) {  // uniform in the workgroup
      if (tid == 0) atomicExch(err + 1, 1);
      __syncthreads();
      continue;
    }
    const int nM = (int)nM64, nt = (int)n64;
    // ---- stage the tile's elements: consecutive threads, consecutive elements
    for (int q = tid; q < nt; q += kNT) {
      int64_t r, i;
      if (q < nA) {
        int s = 0;  // the last piece starting at or before q (kA <= 64)
        for (int x = 1; x < kA; x++)
          if (sA_base[x] <= q) s = x;
        r = rA + s;
        i = sA_lo[s] + (q - sA_base[s]);
      } else if (q < nA + nM) {
        const int64_t p = pM0 + (q - nA);
        r = last_le(S.pstart, rM0, rM1, p);
        i = p - S.pstart[r];
      } else {
        const int qq = q - nA - nM;
        int s = 0;
        for (int x = 1; x < kB; x++)
          if (sB_base[x] <= qq) s = x;
        r = rB + s;
        i = qq - sB_base[s];
      }
      in_key[q] = S.key[r][i];
      in_seg[q] = (int32_t)r;
      if (EMIT) in_val[q] = S.val ? S.val[r][i] : (int32_t)(S.pstart[r] + i);
    }
    __syncthreads();
    // ---- rank every element among its term's pieces in the tile
    for (int q = tid; q < nt; q += kNT) {
      const int64_t r = in_seg[q];
      const int64_t g = S.gid ? S.gid[r] : 0, rs = S.gstart[g], re = S.gstart[g + 1];
      const int64_t v = in_key[q];
      int rank = q;
      if (re - rs > 1) {
        rank = -1;
        for (int64_t x = rs; x < re; x++) {  // at most 64 sources
          int st, len;
          if (x >= rA && x < rA + kA) {
            st = sA_base[x - rA];
            len = sA_n[x - rA];
          } else if (kB && x >= rB && x < rB + kB) {
            st = nA + nM + sB_base[x - rB];
            len = sB_n[x - rB];
          } else {
            st = nA + (int)(S.pstart[x] - pM0);
            len = (int)(S.pstart[x + 1] - S.pstart[x]);
          }
          if (rank < 0) rank = st;  // the term's first piece starts its region
          if (x == r)
            rank += q - st;
          else
            rank += lds_lower(in_key + st, len, x < r ? v + 1 : v);
        }
      }
      if (rank < 0 || rank >= nt) {  // (cannot be: never a store outside the tile)
        atomicExch(err + 1, 1);
        continue;
      }
      out_key[rank] = (int32_t)v;
      out_g[rank] = (int32_t)g;
      if (EMIT) out_val[rank] = in_val[q];
    }
    __syncthreads();
    if (!dedup) {
      if (EMIT) {
        const int64_t o0 = tile_base[t];
        for (int x = tid; x < nt && o0 + x < olimit; x += kNT) {
          okey[o0 + x] = out_key[x];
          oval[o0 + x] = out_val[x];
        }
      }
      __syncthreads();
      continue;
    }
    // ---- equal (term, docno) runs become one posting
    int carry = 0;
    for (int c = 0; c < nt; c += kNT) {
      const int x = c + tid;
      int h = 0;
      if (x < nt) h = x == 0 || out_g[x - 1] != out_g[x] || out_key[x - 1] != out_key[x];
      int tot;
      const int ex = block_excl_sum<kNT, int>(h, s_scan, &tot) + carry;
      carry += tot;
      if (EMIT && h) {
        const int64_t o = tile_base[t] + ex;
        const int32_t g = out_g[x];
        int64_t sum = out_val[x];
        for (int y = x + 1; y < nt && y < x + kMaxInputs && out_g[y] == g && out_key[y] == out_key[x]; y++)
          sum += out_val[y];
        if (sum >= kTfLimit) {
          atomicExch(err, 1);
          sum = kTfLimit - 1;
        }
        if (o >= olimit) {  // (cannot be: the count pass saw the same tile)
          atomicExch(err + 1, 1);
          continue;
        }
        okey[o] = out_key[x];
        oval[o] = (int32_t)sum;
        oterm[o] = (uint32_t)g;
        mtf = max(mtf, (uint32_t)sum);
        if (x > 0 ? out_g[x - 1] != g : (g != g_a || a_first)) off[g] = o;
      }
    }
    if (!EMIT && tid == 0) tile_cnt[t] = carry;
    __syncthreads();
  }
  if (EMIT && dedup) {
    for (int o = 32; o > 0; o >>= 1) mtf = max(mtf, (uint32_t)__shfl_xor((int)mtf, o, 64));
    if ((tid & 63) == 0 && mtf) atomicMax(max_tf, mtf);
  }
}

// ---- the concatenation path: the segments laid end to end ARE the result ------
__global__ __launch_bounds__(kNT) void k_concat(Segs S, int32_t *docno_d, int32_t *tf_d, uint32_t *oterm,
                                                unsigned int *max_tf) {
  uint32_t mtf = 0;
  for_row_elements<kNT>(S.pstart, S.nseg, S.total, [&](int64_t p, int64_t r) {
    const int64_t i = p - S.pstart[r];
    const int32_t tf = S.val[r][i];
    docno_d[p] = S.key[r][i];
    tf_d[p] = tf;
    oterm[p] = (uint32_t)S.gid[r];
    mtf = max(mtf, (uint32_t)tf);
  });
  for (int o = 32; o > 0; o >>= 1) mtf = max(mtf, (uint32_t)__shfl_xor((int)mtf, o, 64));
  if ((threadIdx.x & 63) == 0 && mtf) atomicMax(max_tf, mtf);
}

// ---- positions ------------------------------------------------------------------------
struct PsDev {  // an input's kept streams
  const int64_t *off;
  const int32_t *terms;
};
// stream length of every merged record (src: its flat place in the inputs' record lists)
__global__ void k_ps_lens(const PsDev *ps, int n, const int64_t *rbase, const int32_t *src, int64_t nrec, int64_t *len) {
  for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o <= nrec; o += (int64_t)gridDim.x * blockDim.x) {
    if (o == nrec) {
      len[o] = 0;
      continue;
    }
    const int64_t f = src[o];
    const int a = input_of(rbase, n, f);
    const int64_t i = f - rbase[a];
    len[o] = ps[a].off[i + 1] - ps[a].off[i];
  }
}
// every record's stream into its place, ids rewritten: consecutive lanes,
// consecutive stream words
__global__ __launch_bounds__(kNT) void k_ps_gather(const PsDev *ps, int n, const int64_t *rbase, const int64_t *tbase,
                                                   const int32_t *tmap, const int32_t *src, int64_t nrec,
                                                   const int64_t *ooff, int64_t M, int32_t *out) {
  for_row_elements<kNT>(ooff, nrec, M, [&](int64_t p, int64_t o) {
    const int64_t f = src[o];
    const int a = input_of(rbase, n, f);
    const int64_t i = f - rbase[a];
    const int32_t id = ps[a].terms[ps[a].off[i] + (p - ooff[o])];
    out[p] = id >= 0 ? tmap[tbase[a] + id] : id;
  });
}

// the tiled merge of S: dedup (postings) -> count, scan, emit; else one emit pass.
// Returns the output length.
int64_t tiled_merge(sme_ctx *cx, const Segs &S, int T, bool dedup, int32_t *okey, int32_t *oval, uint32_t *oterm,
                    int64_t *off, unsigned int *d_max_tf, int *d_err, DevBuf &b_tg, DevBuf &b_tv, DevBuf &b_take,
                    DevBuf &b_cnt, DevBuf &b_base, DevBuf &scan, hipStream_t st) {
  const int64_t ntiles = (S.total + T - 1) / T;
  int32_t *tg = b_tg.as<int32_t>((size_t)ntiles + 1);
  int64_t *tv = b_tv.as<int64_t>((size_t)ntiles + 1), *take = b_take.as<int64_t>((size_t)ntiles + 1);
  int64_t *cnt = b_cnt.as<int64_t>((size_t)ntiles + 1), *base = b_base.as<int64_t>((size_t)ntiles + 1);
  hipLaunchKernelGGL(k_tile_bounds, dim3(grid_n(ntiles + 1)), dim3(kNT), 0, st, S, T, dedup ? 0 : 1, ntiles, tg, tv, take);
  SME_CHECK_LAUNCH();
  const size_t lds = (size_t)6 * (T + 64) * sizeof(int32_t);
  const unsigned grid = (unsigned)std::min<int64_t>(ntiles, 65536);
  int64_t total = S.total;
  if (dedup) {
    hipLaunchKernelGGL(k_tile_merge<false>, dim3(grid), dim3(kNT), lds, st, S, T, 1, ntiles, tg, tv, take, cnt,
                       (const int64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (uint32_t *)nullptr,
                       (int64_t *)nullptr, (unsigned int *)nullptr, d_err, (int64_t)0);
    SME_CHECK_LAUNCH();
    SME_HIP(hipMemsetAsync(cnt + ntiles, 0, sizeof(int64_t), st));
    excl_scan<int64_t>(cnt, base, ntiles + 1, scan, st);
    total = rd1(base + ntiles, st);
    if (rd1(d_err + 1, st)) throw Error(SME_EHIP, "index merge: a tile past its capacity (internal)");
  } else {
    std::vector<int64_t> hb((size_t)ntiles + 1);
    for (int64_t t = 0; t <= ntiles; t++) hb[(size_t)t] = std::min<int64_t>(t * (int64_t)T, S.total);
    SME_HIP(hipMemcpyAsync(base, hb.data(), hb.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    SME_HIP(hipStreamSynchronize(st));  // hb goes out of scope
  }
  hipLaunchKernelGGL(k_tile_merge<true>, dim3(grid), dim3(kNT), lds, st, S, T, dedup ? 1 : 0, ntiles, tg, tv, take,
                     (int64_t *)nullptr, (const int64_t *)base, okey, oval, oterm, off, d_max_tf, d_err, total);
  SME_CHECK_LAUNCH();
  return total;
}

}  // namespace

sme_index *merge_indexes(sme_ctx *cx, sme_index *const *ins, int n, hipStream_t st) {
  // ---- refusals, before any per-term work
  {
    std::vector<InputDesc> d((size_t)std::max(0, std::min(n, kMaxInputs)));
    for (size_t i = 0; i < d.size(); i++) {
      const sme_index *x = ins ? ins[i] : nullptr;
      d[i] = InputDesc{x != nullptr, x && x->ctx == cx, x && x->records_only, x ? x->job : 0, x ? x->K : 1};
    }
    int bad = -1;
    const int rc = validate(d.data(), ins ? n : 0, cx->cfg.k, &bad);
    if (rc != M_OK) {
      char msg[160];
      const bool notimpl = describe(rc, bad, msg, sizeof msg);
      throw Error(notimpl ? SME_ENOTIMPL : SME_EINVAL, msg);
    }
  }
  const int T = (int)cx->opt_merge_tile;
  Prof prof(st, &cx->prof_events);
  auto buf = [&](DevBuf &b) -> DevBuf & {
    b.pool = &cx->pool;
    return b;
  };
  DevBuf B[40];
  for (auto &b : B) buf(b);

  // ---- the inputs
  std::vector<TermSource> hin((size_t)n);
  std::vector<int64_t> tbase((size_t)n + 1, 0), rbase((size_t)n + 1, 0);
  int64_t Pt = 0, N = 0, ps_total = 0, dmin = 0, dmax = -1;
  bool keep_ps = true, any_rec = false, any_ps = false;
  for (int a = 0; a < n; a++) {
    const sme_index *x = ins[a];
    hin[(size_t)a] = TermSource{(const int64_t *)x->d_term_off.p, (const uint16_t *)x->d_term_chars.p, x->V,
                           (const int64_t *)x->d_off.p,      (const int32_t *)x->d_docno_d.p,     (const int32_t *)x->d_tf_d.p};
    tbase[(size_t)a + 1] = tbase[(size_t)a] + x->V;
    rbase[(size_t)a + 1] = rbase[(size_t)a] + x->N;
    Pt += x->P;
    N += x->N;
    any_ps |= x->has_positions;
    if (x->N > 0) {
      if (!x->has_positions || x->ps_records != x->N) keep_ps = false;
      ps_total += x->has_positions ? x->ps_terms : 0;
      dmin = any_rec ? std::min(dmin, x->dmin) : x->dmin;
      dmax = any_rec ? std::max(dmax, x->dmax) : x->dmax;
      any_rec = true;
    }
  }
  bool rec_complete = true;  // every input with records holds every record's real docno
  for (int a = 0; a < n; a++) rec_complete &= ins[a]->N == 0 || ins[a]->rec_complete;
  if (!any_ps) keep_ps = false;
  const int64_t Vt = tbase[(size_t)n];
  if (Pt > 0xFFFFFFFFll) throw Error(SME_ELIMIT, "index merge: more than 2^32 postings");
  if (Vt > 0x7FFFFFFFll || N > 0x7FFFFFFFll) throw Error(SME_ELIMIT, "index merge: 2^31 or more terms or records");
  if (keep_ps && ps_total > 0x7FFFFFFFll) throw Error(SME_ELIMIT, "index merge: more than 2^31 - 1 stream positions");
  // source order: by docno range when the ranges are pairwise disjoint (the
  // concatenation path), else the list's
  std::vector<int32_t> ord((size_t)n);
  std::iota(ord.begin(), ord.end(), 0);
  bool append = cx->opt_merge_append != 0;
  if (append) {
    std::vector<int> by((size_t)n);
    std::iota(by.begin(), by.end(), 0);
    std::stable_sort(by.begin(), by.end(), [&](int x, int y) {
      const bool ex = ins[x]->N == 0, ey = ins[y]->N == 0;
      if (ex != ey) return ey;  // inputs without records last
      return !ex && ins[x]->dmin < ins[y]->dmin;
    });
    for (int i = 0; i + 1 < n && append; i++)
      if (ins[by[(size_t)i + 1]]->N > 0 && ins[by[(size_t)i]]->dmax >= ins[by[(size_t)i + 1]]->dmin) append = false;
    if (append)
      for (int i = 0; i < n; i++) ord[(size_t)by[(size_t)i]] = i;
  }

  TermSource *d_in = B[0].as<TermSource>((size_t)n);
  int64_t *d_tbase = B[1].as<int64_t>((size_t)n + 1), *d_rbase = B[2].as<int64_t>((size_t)n + 1);
  int32_t *d_ord = B[3].as<int32_t>((size_t)n);
  SME_HIP(hipMemcpyAsync(d_in, hin.data(), (size_t)n * sizeof(TermSource), hipMemcpyHostToDevice, st));
  SME_HIP(hipMemcpyAsync(d_tbase, tbase.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  SME_HIP(hipMemcpyAsync(d_rbase, rbase.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  SME_HIP(hipMemcpyAsync(d_ord, ord.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  // [0] shared terms, [1] max_tf (u32), [2] the two error flags, [4..8) tf_sort_segments' counters
  unsigned long long *d_cnt = B[4].as<unsigned long long>(8);
  SME_HIP(hipMemsetAsync(d_cnt, 0, 8 * sizeof(unsigned long long), st));
  unsigned int *d_mtf = reinterpret_cast<unsigned int *>(d_cnt + 1);
  int *d_err = reinterpret_cast<int *>(d_cnt + 2);

  sme_index *ix = new sme_index(cx);
  std::unique_ptr<sme_index> guard(ix);
  ix->K = 1;
  ix->R = cx->cfg.num_partitions;
  ix->idf_mode = cx->cfg.idf_mode;
  ix->from_records = true;  // the doc counter is kept as its postings: no record docnos, no pieces
  ix->N = N;
  ix->rec_complete = rec_complete;
  if (any_rec) {
    ix->dmin = dmin;
    ix->dmax = dmax;
  }

  // ---------------- 1. terms ----------------
  const VocabUnion U = union_vocab(d_in, n, d_tbase, d_ord, Vt, ix, d_cnt,
                                   UnionScratch{B[5], B[6], B[7], B[8], B[9], B[10], B[11], B[12], B[13], B[14], B[15],
                                                B[16], B[17]},
                                   st);
  const int64_t V = U.V;
  prof.mark("terms");

  // ---------------- 2. docno-order postings ----------------
  int64_t P = 0;
  int64_t *off = ix->d_off.as<int64_t>((size_t)V + 1);
  SME_HIP(hipMemsetAsync(off, 0, ((size_t)V + 1) * sizeof(int64_t), st));
  uint32_t *term_of = B[18].as<uint32_t>((size_t)Pt + 1);
  // (tf_d: 16-byte aligned for tf_sort_segments -- hipMalloc'd blocks are)
  int32_t *docno_d = ix->d_docno_d.as<int32_t>((size_t)Pt + 1), *tf_d = ix->d_tf_d.as<int32_t>((size_t)Pt + 1);
  int mtf = 0;
  if (Pt > 0) {
    Segs S{U.pstart, U.seg_key, U.seg_val, U.gid, U.gstart, Vt, V, Pt};
    if (append) {
      hipLaunchKernelGGL(k_concat, dim3(grid_n(Pt, 1024, 65536)), dim3(kNT), 0, st, S, docno_d, tf_d, term_of, d_mtf);
      segment_term_offsets(U.pstart, U.gstart, V, off, st);
      P = Pt;
    } else {
      P = tiled_merge(cx, S, T, true, docno_d, tf_d, term_of, off, d_mtf, d_err, B[19], B[20], B[21], B[22], B[23], B[17],
                      st);
    }
    mtf = (int)rd1(d_mtf, st);
    if (rd1(d_err + 1, st)) throw Error(SME_EHIP, "index merge: a tile past its capacity (internal)");
    if (rd1(d_err, st)) throw Error(SME_ELIMIT, "index merge: a summed term frequency of 2^24 or more");
  }
  SME_HIP(hipMemcpyAsync(off + V, &P, sizeof(int64_t), hipMemcpyHostToDevice, st));
  SME_HIP(hipStreamSynchronize(st));
  ix->P = P;
  ix->max_tf = std::max(1, mtf);
  prof.mark("postings");

  // ---------------- 3. reduce order ----------------
  int32_t *docno_o = ix->d_docno_o.as<int32_t>((size_t)P + 1), *tf_o = ix->d_tf_o.as<int32_t>((size_t)P + 1);
  if (P > 0 && ix->max_tf <= kTfSortMaxTf) {
    tf_sort_segments(off, V, P, docno_d, tf_d, ix->max_tf, docno_o, tf_o, B[24], B[25], B[26], B[17], d_cnt + 4,
                     st, cx->aux_stream, cx->ev_fork, cx->ev_join);
  } else if (P > 0) {
    sort_term_tf(term_of, docno_d, tf_d, nullptr, P, V, ix->max_tf, docno_o, tf_o, B[24], B[25], B[26], B[27], B[28], st);
  }
  prof.mark("tf_order");

  // ---------------- 4. weights ----------------
  ix->d_idf.as<double>((size_t)V + 1);
  ix->d_w.as<double>((size_t)P + 1);
  reweight_index(ix, N, nullptr, st, P > 0 ? term_of : nullptr);
  prof.mark("weights");

  // ---------------- 5. doc counter and positions ----------------
  int32_t *rdn = ix->d_rec_docno.as<int32_t>((size_t)N + 1);
  uint8_t *fst = ix->d_rec_first.as<uint8_t>((size_t)N + 1);
  for (int a = 0; a < n; a++) {
    const sme_index *x = ins[a];
    if (x->N == 0) continue;
    SME_HIP(hipMemcpyAsync(rdn + rbase[(size_t)a], x->d_rec_docno.p, (size_t)x->N * sizeof(int32_t),
                           hipMemcpyDeviceToDevice, st));
    if (x->d_rec_first.p) {
      SME_HIP(hipMemcpyAsync(fst + rbase[(size_t)a], x->d_rec_first.p, (size_t)x->N, hipMemcpyDeviceToDevice, st));
    } else {  // a built index: one map task
      SME_HIP(hipMemsetAsync(fst + rbase[(size_t)a], 0, (size_t)x->N, st));
    }
    SME_HIP(hipMemsetAsync(fst + rbase[(size_t)a], 1, 1, st));
  }
  if (keep_ps) {
    std::vector<PsDev> hps((size_t)n);
    std::vector<const int32_t *> hkey((size_t)n);
    for (int a = 0; a < n; a++) {
      hps[(size_t)a] = PsDev{(const int64_t *)ins[a]->d_ps_off.p, (const int32_t *)ins[a]->d_ps_terms.p};
      hkey[(size_t)a] = ins[a]->N > 0 ? (const int32_t *)ins[a]->d_ps_docno.p : nullptr;
    }
    PsDev *d_ps = B[29].as<PsDev>((size_t)n);
    const int32_t **d_key = (const int32_t **)B[30].as<uint64_t>((size_t)n);
    int64_t *d_g01 = B[31].as<int64_t>(2);
    const int64_t g01[2] = {0, n};
    SME_HIP(hipMemcpyAsync(d_ps, hps.data(), (size_t)n * sizeof(PsDev), hipMemcpyHostToDevice, st));
    SME_HIP(hipMemcpyAsync(d_key, hkey.data(), (size_t)n * sizeof(void *), hipMemcpyHostToDevice, st));
    SME_HIP(hipMemcpyAsync(d_g01, g01, sizeof g01, hipMemcpyHostToDevice, st));
    int32_t *pdn = ix->d_ps_docno.as<int32_t>((size_t)N + 1);
    int32_t *src = B[32].as<int32_t>((size_t)N + 1);
    Segs S{d_rbase, d_key, nullptr, nullptr, d_g01, n, 1, N};
    if (N > 0)
      tiled_merge(cx, S, T, false, pdn, src, nullptr, nullptr, nullptr, d_err, B[19], B[20], B[21], B[22], B[23], B[17],
                  st);
    int64_t *len = B[33].as<int64_t>((size_t)N + 1), *ooff = ix->d_ps_off.as<int64_t>((size_t)N + 1);
    hipLaunchKernelGGL(k_ps_lens, dim3(grid_n(N + 1)), dim3(kNT), 0, st, d_ps, n, d_rbase, (const int32_t *)src, N, len);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(len, ooff, N + 1, B[17], st);
    const int64_t M = rd1(ooff + N, st);
    if (rd1(d_err + 1, st)) throw Error(SME_EHIP, "index merge: a tile past its capacity (internal)");
    if (M != ps_total) throw Error(SME_EHIP, "index merge: stream lengths do not add up (internal)");
    int32_t *out = ix->d_ps_terms.as<int32_t>((size_t)M + 1);
    if (M > 0)
      hipLaunchKernelGGL(k_ps_gather, dim3(grid_n(M, 1024, 65536)), dim3(kNT), 0, st, d_ps, n, d_rbase, d_tbase,
                         U.tmap, (const int32_t *)src, N, (const int64_t *)ooff, M, out);
    SME_CHECK_LAUNCH();
    ix->ps_records = N;
    ix->ps_terms = M;
    ix->has_positions = true;
  }
  prof.mark("positions");
  ix->profile = prof.finish();  // waits for the stream: the scratch goes back to the pool after it
  ix->mg_inputs = (uint64_t)n;
  ix->mg_shared = (uint64_t)rd1(d_cnt, st);
  ix->mg_merged = (uint64_t)(Pt - P);
  ix->mg_appended = append && Pt > 0 ? 1 : 0;
  guard.release();
  return ix;
}

}  // namespace sme
