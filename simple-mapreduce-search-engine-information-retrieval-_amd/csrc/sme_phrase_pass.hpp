// sme_phrase_pass.hpp -- the pass that phrase queries (sme_phrase.hip) and proximity
// queries (sme_near.hip) share: everything but the position predicate.  Internal:
// nothing of it enters include/sme.h.
//
// k_phrase_plan picks per query the driver, the term with the fewest postings,
// whose posting list holds the candidates; the chunk filter of sme_chunks.hpp --
// once counting, once emitting -- keeps the driver postings that every other
// distinct term of the query also holds, by binary searches bounded to the chunk's
// docno range (PhraseOp).  The feature's verify kernel then gives every surviving
// (query, docno) its freq and a flag; the flagged pairs are compacted, scored by
// the feature's score kernel and, for the score order, sorted by stable passes over
// an index permutation.  Candidates leave the filter by query and docno ascending,
// so the docno order needs no sort.  run_pass is that sequence on the host.  It
// takes the filter's Op as a parameter: PhraseOp for phrase and proximity calls,
// NarrowOp -- PhraseOp plus the group test of a structured query's term-only
// groups -- for the operator leaves of sme_structq.hip.
//
// The kernels stand in an unnamed namespace: each of the two files has its own.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sme_bool.hpp"
#include "sme_chunks.hpp"
#include "sme_internal.hpp"
#include "sme_phrase.hpp"

namespace sme {
namespace {
using namespace chunks;

struct Batch {           // the uploaded batch (device pointers into one block)
  const int64_t *poff;   // [np + 1] term offsets
  const int32_t *term;   // [nt] term ids (-1: unknown)
};

// One thread per phrase.  dpos[i] = the driver's place in phrase i (-1: the phrase
// matches nothing -- it is empty or holds an unknown term), dbeg / dcnt its posting
// list, nchunk[i] = the list's chunks (entry np = 0).  *cands += the driver's postings.
__global__ void k_phrase_plan(Batch b, int np, const int64_t *__restrict__ doff, int chunk,
                              int64_t *__restrict__ dbeg, int32_t *__restrict__ dcnt, int32_t *__restrict__ dpos,
                              int64_t *__restrict__ nchunk, unsigned long long *__restrict__ cands) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= np; i += (int64_t)gridDim.x * blockDim.x) {
    if (i == np) {
      nchunk[np] = 0;
      continue;
    }
    const int64_t t0 = b.poff[i];
    const int L = (int)(b.poff[i + 1] - t0);  // <= kMaxLen (validated on the host)
    int drv = -1;
    int64_t best = 0, beg = 0;
    bool dead = L == 0;
    for (int j = 0; j < L && !dead; j++) {
      const int32_t t = b.term[t0 + j];
      if (t < 0) {
        dead = true;
        break;
      }
      const int64_t cnt = doff[t + 1] - doff[t];
      if (drv < 0 || cnt < best) {
        drv = j;
        best = cnt;
        beg = doff[t];
      }
    }
    if (dead || best == 0) {
      drv = -1;
      best = 0;
      beg = 0;
    }
    dpos[i] = drv;
    dbeg[i] = beg;
    dcnt[i] = (int32_t)best;
    nchunk[i] = (best + chunk - 1) / chunk;
    if (best > 0) atomicAdd(cands, (unsigned long long)best);
  }
}

// the posting of document d in docno[start .. start + n), or -1
__device__ __forceinline__ int64_t find_doc(const int32_t *__restrict__ docno, int64_t start, int n, int32_t d) {
  const int at = lower_bound(docno + start, n, d);
  return at < n && docno[start + at] == d ? start + at : -1;
}

// The chunk filter's Op (sme_chunks.hpp): range = phrase, candidate c of it the
// driver posting dbeg[r] + c.  The chunk's docnos lie in [first, last]; per term of
// the phrase the sub-range of its posting list that can hold such a docno (two
// bounds) is staged in LDS -- length -1 for a term that needs no test: the driver
// itself, and one equal to the driver or to an earlier term of the phrase.  A term
// whose sub-range is empty rejects the whole chunk.  A candidate survives when
// every tested term holds its docno.  Emitted: the docno and the phrase.
struct PhraseOp {
  Batch b;
  const int64_t *dbeg;
  const int32_t *dpos;
  const int64_t *doff;
  const int32_t *docno;
  struct Lds {
    int64_t start[phrase::kMaxLen];
    int32_t len[phrase::kMaxLen];
    int reject;
  };
  struct Chunk {
    int L;
    int64_t base;  // the driver's first posting
  };
  struct Cand {
    int32_t d;
  };
  __device__ __forceinline__ bool stage(Lds &s, Chunk &k, int64_t r, int64_t c0, int len) const {
    const int tid = threadIdx.x;
    const int64_t t0 = b.poff[r];
    k.L = (int)(b.poff[r + 1] - t0);
    k.base = dbeg[r];
    const int dp = dpos[r];
    const int32_t first = docno[k.base + c0], last = docno[k.base + c0 + len - 1];
    if (tid == 0) s.reject = 0;
    if (tid < k.L) {
      const int32_t t = b.term[t0 + tid];
      bool skip = tid == dp || t == b.term[t0 + dp];
      for (int j = 0; !skip && j < tid; j++) skip = b.term[t0 + j] == t;
      if (skip) {
        s.start[tid] = 0;
        s.len[tid] = -1;
      } else {
        const int64_t beg = doff[t];
        const int n = (int)(doff[t + 1] - beg);  // a posting list holds fewer than 2^31 documents
        const int lo = lower_bound(docno + beg, n, first);
        const int hi = lo + upper_bound(docno + beg + lo, n - lo, last);
        s.start[tid] = beg + lo;
        s.len[tid] = hi - lo;
      }
    }
    __syncthreads();
    if (tid < k.L && s.len[tid] == 0) s.reject = 1;
    __syncthreads();
    return s.reject == 0;
  }
  __device__ __forceinline__ bool test(const Lds &s, const Chunk &k, int64_t, int64_t c, Cand &x) const {
    const int32_t d = x.d = docno[k.base + c];
    bool hit = true;
    for (int j = 0; hit && j < k.L; j++)
      if (s.len[j] >= 0) hit = find_doc(docno, s.start[j], s.len[j], d) >= 0;
    return hit;
  }
  __device__ __forceinline__ void emit(const Lds &, const Chunk &, int64_t r, const Cand &x, int64_t at,
                                       int32_t *__restrict__ cdoc, uint32_t *__restrict__ cph) const {
    cdoc[at] = x.d;
    cph[at] = (uint32_t)r;
  }
};
// PhraseOp narrowed (structured queries; NarrowSpec in sme_internal.hpp): phrase r
// belongs to owner[r], whose groups of term slots every result must lie in.  After
// PhraseOp's staging, per slot of the owner's groups the sub-range of its posting
// list inside the chunk's docno range is staged once; a group whose sub-ranges are
// all empty rejects the chunk.  A candidate survives PhraseOp's test and, per
// group, a search of at least one slot's sub-range (OR over the group's slots).
// A slot of term -1 and a group without slots hold nothing.
struct NarrowOp {
  PhraseOp p;
  const int32_t *owner;  // [np]
  const int64_t *qgoff;  // [owners + 1] group offsets
  const int64_t *goff;   // [groups + 1] slot offsets
  const int32_t *nterm;  // [slots]
  struct Lds {
    PhraseOp::Lds p;
    int64_t start[kNarrowSlots];
    int32_t len[kNarrowSlots];
    int32_t gbeg[kNarrowGroups + 1];
    int reject;
  };
  struct Chunk {
    PhraseOp::Chunk p;
    int ng;
  };
  using Cand = PhraseOp::Cand;
  __device__ __forceinline__ bool stage(Lds &s, Chunk &k, int64_t r, int64_t c0, int len) const {
    if (!p.stage(s.p, k.p, r, c0, len)) return false;  // (the same verdict in every thread)
    const int tid = threadIdx.x;
    const int o = owner[r];
    const int64_t g0 = qgoff[o];
    k.ng = (int)(qgoff[o + 1] - g0);  // <= kNarrowGroups (the host cuts the spec)
    if (k.ng == 0) return true;
    const int64_t s0 = goff[g0];
    const int S = (int)(goff[g0 + k.ng] - s0);  // <= kNarrowSlots
    const int32_t first = p.docno[k.p.base + c0], last = p.docno[k.p.base + c0 + len - 1];
    if (tid <= k.ng) s.gbeg[tid] = (int32_t)(goff[g0 + tid] - s0);
    if (tid == 0) s.reject = 0;
    for (int j = tid; j < S; j += kNT) {
      const int32_t t = nterm[s0 + j];
      const int64_t beg = t < 0 ? 0 : p.doff[t];
      const int n = t < 0 ? 0 : (int)(p.doff[t + 1] - beg);
      const int lo = lower_bound(p.docno + beg, n, first);
      const int hi = lo + upper_bound(p.docno + beg + lo, n - lo, last);
      s.start[j] = beg + lo;
      s.len[j] = hi - lo;
    }
    __syncthreads();
    if (tid < k.ng) {
      int any = 0;
      for (int j = s.gbeg[tid]; j < s.gbeg[tid + 1]; j++) any |= s.len[j];
      if (any == 0) s.reject = 1;
    }
    __syncthreads();
    return s.reject == 0;
  }
  __device__ __forceinline__ bool test(const Lds &s, const Chunk &k, int64_t r, int64_t c, Cand &x) const {
    bool hit = p.test(s.p, k.p, r, c, x);
    for (int g = 0; hit && g < k.ng; g++) {
      bool held = false;
      for (int j = s.gbeg[g]; !held && j < s.gbeg[g + 1]; j++)
        held = find_doc(p.docno, s.start[j], s.len[j], x.d) >= 0;
      hit = held;
    }
    return hit;
  }
  __device__ __forceinline__ void emit(const Lds &s, const Chunk &k, int64_t r, const Cand &x, int64_t at,
                                       int32_t *__restrict__ cdoc, uint32_t *__restrict__ cph) const {
    p.emit(s.p, k.p, r, x, at, cdoc, cph);
  }
};
struct SelfRange {  // phrase i owns range i
  __device__ int64_t operator()(int64_t i) const { return i; }
};

// The verify kernels' launch shape: one wave per candidate, grid-strided
constexpr int kVerifyNT = 256;
inline unsigned verify_grid(int64_t C) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((C + 3) / 4, 16384));
}

// woff[i] = matches before phrase i's first candidate: the compacted candidate
// indices idx[0 .. T) ascend, coff[i] = candidates before phrase i (entry np: all)
__global__ void k_phrase_offs(const int32_t *__restrict__ idx, const int32_t *__restrict__ d_T,
                              const int64_t *__restrict__ coff, int64_t np, int64_t *__restrict__ woff) {
  const int64_t T = *d_T;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= np; i += (int64_t)gridDim.x * blockDim.x)
    woff[i] = lower_bound(idx, T, (int32_t)coff[i]);  // (fewer than 2^31 candidates: count_chunks refuses more)
}

// match x (candidate idx[x]): its document, phrase, freq and score = lut[freq] *
// idf[phrase], the product k_weights forms for a posting
__global__ void k_phrase_score(const int32_t *__restrict__ idx, int64_t T, const int32_t *__restrict__ cdoc,
                               const uint32_t *__restrict__ cph, const int32_t *__restrict__ freq,
                               const double *__restrict__ lut, const double *__restrict__ idf,
                               int32_t *__restrict__ mdoc, uint32_t *__restrict__ mph, int32_t *__restrict__ mfreq,
                               double *__restrict__ mscore) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < T; x += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = idx[x];
    const uint32_t p = cph[c];
    const int32_t f = freq[c];
    mdoc[x] = cdoc[c];
    mph[x] = p;
    mfreq[x] = f;
    mscore[x] = __dmul_rn(lut[f], idf[p]);
  }
}
__global__ void k_phrase_key_score(const double *__restrict__ mscore, int64_t n, uint64_t *__restrict__ key,
                                   uint32_t *__restrict__ perm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    key[i] = boolq::score_key(mscore[i]);
    perm[i] = (uint32_t)i;
  }
}
__global__ void k_phrase_key_owner(const uint32_t *__restrict__ mph, const uint32_t *__restrict__ perm, int64_t n,
                                   uint32_t *__restrict__ key) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    key[i] = mph[perm[i]];
}
// Ordered match x (phrase qs[x], match perm[x]; both NULL: the matches as they are,
// docno order) is the (x - woff[q])-th of its phrase: kept if that is below the cut.
__global__ void k_phrase_gather(const uint32_t *__restrict__ qs, const uint32_t *__restrict__ perm,
                                const int32_t *__restrict__ mdoc, const uint32_t *__restrict__ mph,
                                const int32_t *__restrict__ mfreq, const double *__restrict__ mscore, int64_t total,
                                const int64_t *__restrict__ woff, const int64_t *__restrict__ roff, int64_t m,
                                int32_t *__restrict__ out_docno, int32_t *__restrict__ out_freq,
                                double *__restrict__ out_score) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = perm ? (int64_t)perm[x] : x;
    const uint32_t q = qs ? qs[x] : mph[i];
    const int64_t rk = x - woff[q];
    if (m > 0 && rk >= m) continue;
    out_docno[roff[q] + rk] = mdoc[i];
    out_freq[roff[q] + rk] = mfreq[i];
    out_score[roff[q] + rk] = mscore[i];
  }
}

struct PlainFilter {  // run_pass's make_op of a pass that filters by the phrase's own terms alone
  PhraseOp operator()(const uint8_t *, const PhraseOp &p) const { return p; }
};

// One pass over a validated batch of np queries into `out`, the feature's result
// on the index: `blob` is the upload, holding the term offsets at a_poff and
// the term ids at a_term beside whatever else the feature's kernels read.
//   make_op(d_in, phrase_op)  the chunk filter's Op: PhraseOp itself (PlainFilter),
//       or one that tests more on top of it (d_in: the uploaded blob)
//   verify(d_in, b, cdoc, cph, C, freq, flag)  launches the verify kernel over the
//       C candidates: freq[x] and flag[x] = freq[x] > 0 (d_in: the uploaded blob)
//   score(grid, idx, T, cdoc, cph, freq, d_idf, mdoc, mph, mfreq, mscore)  launches
//       the score kernel over the T matches
// `limit` is the SME_ELIMIT message at 2^31 candidates or more.
template <class MakeOp, class Verify, class Score>
void run_pass(sme_index *ix, DocFreqScores &out, const Blob &blob, size_t a_poff, size_t a_term, int np, int order,
              int m, const char *limit, hipStream_t st, MakeOp make_op, Verify verify, Score score) {
  sme_ctx *cx = ix->ctx;
  out.reset();
  int64_t *d_roff = out.offsets(np);
  SME_HIP(hipMemsetAsync(d_roff, 0, ((size_t)np + 1) * sizeof(int64_t), st));
  if (np == 0) {
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  const int chunk = (int)cx->opt_bool_chunk;
  // temporaries of this call: pooled blocks, back in the pool on return
  DevBuf in, dbb, dcb, dpb, chb, mob, cnd, scn, cdb, cpb, frb, flb, idb, s1b, s2b, cob, wob, tab, mdb, mpb, mfb, msb, ka,
      kb, pa, pb, sa, sb, radix;
  for (DevBuf *b : {&in, &dbb, &dcb, &dpb, &chb, &mob, &cnd, &scn, &cdb, &cpb, &frb, &flb, &idb, &s1b, &s2b, &cob, &wob,
                    &tab, &mdb, &mpb, &mfb, &msb, &ka, &kb, &pa, &pb, &sa, &sb, &radix})
    b->pool = &cx->pool;
  Blob tab_h;                   // second upload: result offsets | idf per phrase (outlives its async copy)
  std::vector<int64_t> h_woff;  // matches before each phrase (target of an async copy)
  try {
    const uint8_t *d_in = in.as<uint8_t>(blob.bytes.size());
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st));
    const Batch b{(const int64_t *)(d_in + a_poff), (const int32_t *)(d_in + a_term)};
    int64_t *dbeg = dbb.as<int64_t>((size_t)np);
    int32_t *dcnt = dcb.as<int32_t>((size_t)np);
    int32_t *dpos = dpb.as<int32_t>((size_t)np);
    int64_t *choff = chb.as<int64_t>((size_t)np + 1);
    unsigned long long *d_cands = cnd.as<unsigned long long>(1);
    const int64_t *doff = (const int64_t *)ix->d_off.p;
    const int32_t *docno = (const int32_t *)ix->d_docno_d.p;
    SME_HIP(hipMemsetAsync(d_cands, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_phrase_plan, dim3(grid_for((int64_t)np + 1)), dim3(kNT), 0, st, b, np, doff, chunk, dbeg, dcnt,
                       dpos, choff, d_cands);
    SME_CHECK_LAUNCH();
    unsigned long long cands = 0;
    const auto op = make_op(d_in, PhraseOp{b, dbeg, dpos, doff, docno});
    const Counted c = count_chunks(op, np, choff, dcnt, chunk, mob, scn, limit, st, d_cands, &cands);
    const int64_t C = c.total;  // (phrase, docno) pairs that hold all the phrase's terms
    int64_t T = 0, out_total = 0;
    if (C > 0) {
      int32_t *cdoc = cdb.as<int32_t>((size_t)C);
      uint32_t *cph = cpb.as<uint32_t>((size_t)C);
      int32_t *freq = frb.as<int32_t>((size_t)C);
      uint8_t *flag = flb.as<uint8_t>((size_t)C);
      int32_t *idx = idb.as<int32_t>((size_t)C + 1);
      int32_t *d_T = reinterpret_cast<int32_t *>(d_cands);  // (the candidate count has been read)
      int64_t *coff = cob.as<int64_t>((size_t)np + 1);
      int64_t *woff = wob.as<int64_t>((size_t)np + 1);
      emit_chunks(op, c, st, cdoc, cph);
      verify(d_in, b, (const int32_t *)cdoc, (const uint32_t *)cph, C, freq, flag);
      SME_CHECK_LAUNCH();
      SME_HIP(hipMemsetAsync(d_T, 0, sizeof(unsigned long long), st));
      select_flagged(flag, C, idx, d_T, s1b, s2b, st);
      hipLaunchKernelGGL(k_owner_offs<SelfRange>, dim3(grid_for((int64_t)np + 1)), dim3(kNT), 0, st, SelfRange{},
                         c.choff, c.moff, (int64_t)np, coff);
      hipLaunchKernelGGL(k_phrase_offs, dim3(grid_for((int64_t)np + 1)), dim3(kNT), 0, st, (const int32_t *)idx,
                         (const int32_t *)d_T, (const int64_t *)coff, (int64_t)np, woff);
      SME_CHECK_LAUNCH();
      h_woff.resize((size_t)np + 1);
      SME_HIP(hipMemcpyAsync(h_woff.data(), woff, ((size_t)np + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
      T = h_woff[(size_t)np];
      if (T > 0) {
        // per phrase: its results after the cut (scanned into offsets) and the idf of
        // its document frequency, the matches before the cut
        std::vector<int64_t> roff((size_t)np + 1, 0);
        std::vector<double> idf((size_t)np, 0.0);
        const bool ref = ix->idf_mode == SME_IDF_REFERENCE;
        for (int i = 0; i < np; i++) {
          const int64_t df = h_woff[(size_t)i + 1] - h_woff[(size_t)i];
          roff[(size_t)i + 1] = roff[(size_t)i] + (m > 0 && df > m ? (int64_t)m : df);
          if (df > 0) idf[(size_t)i] = idf_value(ix->idf_N, ref ? 1 : df);
        }
        out_total = roff[(size_t)np];
        const size_t a_roff = tab_h.add(roff.data(), roff.size());
        const size_t a_idf = tab_h.add(idf.data(), idf.size());
        const uint8_t *d_tab = tab.as<uint8_t>(tab_h.bytes.size());
        SME_HIP(hipMemcpyAsync((void *)d_tab, tab_h.bytes.data(), tab_h.bytes.size(), hipMemcpyHostToDevice, st));
        SME_HIP(hipMemcpyAsync(d_roff, d_tab + a_roff, ((size_t)np + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        const double *d_idf = (const double *)(d_tab + a_idf);
        int32_t *out_docno = out.alloc<DocFreqScores::docno>(out_total);
        int32_t *out_freq = out.alloc<DocFreqScores::freq>(out_total);
        double *out_score = out.alloc<DocFreqScores::score>(out_total);
        int32_t *mdoc = mdb.as<int32_t>((size_t)T);
        uint32_t *mph = mpb.as<uint32_t>((size_t)T);
        int32_t *mfreq = mfb.as<int32_t>((size_t)T);
        double *mscore = msb.as<double>((size_t)T);
        const unsigned g = grid_for(T);
        score(g, (const int32_t *)idx, T, (const int32_t *)cdoc, (const uint32_t *)cph, (const int32_t *)freq, d_idf,
              mdoc, mph, mfreq, mscore);
        const uint32_t *qs = nullptr, *perm = nullptr;
        if (order == 1) {
          // the matches stand by (phrase, docno): a stable sort by the score key, then
          // one by the phrase, leaves (phrase, score descending, docno ascending)
          uint64_t *s0 = sa.as<uint64_t>((size_t)T), *s1 = sb.as<uint64_t>((size_t)T);
          uint32_t *p0 = pa.as<uint32_t>((size_t)T), *p1 = pb.as<uint32_t>((size_t)T);
          uint32_t *k0 = ka.as<uint32_t>((size_t)T), *k1 = kb.as<uint32_t>((size_t)T);
          hipLaunchKernelGGL(k_phrase_key_score, dim3(g), dim3(kNT), 0, st, (const double *)mscore, T, s0, p0);
          sort_pairs<uint64_t>(s0, s1, p0, p1, T, 64, radix, st);
          hipLaunchKernelGGL(k_phrase_key_owner, dim3(g), dim3(kNT), 0, st, (const uint32_t *)mph,
                             (const uint32_t *)p1, T, k0);
          sort_pairs<uint32_t>(k0, k1, p1, p0, T, owner_bits(np), radix, st);
          qs = k1;
          perm = p0;
        }
        hipLaunchKernelGGL(k_phrase_gather, dim3(g), dim3(kNT), 0, st, qs, perm, (const int32_t *)mdoc,
                           (const uint32_t *)mph, (const int32_t *)mfreq, (const double *)mscore, T,
                           (const int64_t *)woff, (const int64_t *)d_roff, (int64_t)m, out_docno, out_freq, out_score);
        SME_CHECK_LAUNCH();
      }
    }
    SME_HIP(hipStreamSynchronize(st));
    out.total = out_total;
    out.cands = (uint64_t)cands;
    out.verified = (uint64_t)C;
    out.matches = (uint64_t)T;
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the uploads may still read the blobs, kernels the temporaries
    throw;
  }
}

}  // namespace
}  // namespace sme
