// sme_rescore.hip -- scoring given documents (include/sme.h, sme_query_rescore): per
// query a list of term slots and a strictly ascending list of candidate docnos ->
// every candidate's TF-IDF or BM25 score over the slots and the number of slots
// whose posting list holds it, the candidates with enough hits kept, ordered and cut.
// An intersection of a sorted candidate list with the terms' docno-ordered posting
// lists (d_off / d_docno_d / d_w / d_tf_d).
//
//   k_rs_check   (device candidates) a descending or equal pair inside a query ->
//                the first such query; k_rs_score does nothing once it is set
//   k_rs_score   one workgroup per (query, tile of kTile candidates); see the kernel
//   excl_scan    the tiles' kept counts -> the matches before every tile; k_rs_woff,
//                k_cut and a second scan -> the result offsets after the cut
//   k_rs_emit    order 0: the kept candidates straight into the result, in the given
//                order, below the cut -- no sort.  order 1: into the match arrays,
//                which lie in (query, docno) order; stable sorts of an index
//                permutation by the score key and by the query, and k_rs_gather
//
// The BM25 weight and norm are the functions of sme_bm25.hpp, the tables those of
// prepare_bm25; the call leaves d_bm_norm and the BM25 call's counts alone.
#include "sme_rescore.hpp"

#include <limits.h>

#include <algorithm>
#include <exception>
#include <string>

#include "sme_bm25.hpp"
#include "sme_bool.hpp"
#include "sme_chunks.hpp"
#include "sme_internal.hpp"

namespace sme {
namespace {
using namespace chunks;
using namespace rescore;

static_assert(kTile % kNT == 0, "a tile is a whole number of rounds");

struct ScoreArgs {
  const int64_t *off;  // [V + 1]
  const int32_t *dn;   // [P] docno-ascending per term
  const int32_t *tf;   // [P]
  const double *w;     // [P] TF-IDF weights
  const double *idf;   // [V] BM25 idf (model 1)
  const int32_t *dl;   // [span] document lengths (model 1)
  const int32_t *terms;
  const int64_t *qoff;  // [nq + 1] slots
  const int32_t *cand;
  const int64_t *doff;  // [nq + 1] candidates
  const int64_t *toff;  // [nq + 1] tiles
  int nq;
  int64_t ntiles, V, dmin, span;
  int model, path, min_hits;
  double k1, b, avgdl;
  const int *bad;  // the order check's verdict (INT_MAX: none)
  double *score;   // [candidates]
  int32_t *hits;   // [candidates]
  int64_t *tkept;  // [ntiles] candidates kept per tile
  unsigned long long *found;
};

// the query of tile `t`: the last one whose first tile is at or before it
__device__ __forceinline__ int tile_query(const int64_t *__restrict__ toff, int nq, int64_t t) {
  return upper_bound(toff, nq, t) - 1;
}

__global__ void k_rs_check(const int32_t *__restrict__ cand, const int64_t *__restrict__ doff, int nq, int64_t total,
                           int *__restrict__ bad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x + 1; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (cand[i - 1] < cand[i]) continue;
    const int q = upper_bound(doff, nq, i) - 1;  // the query holding candidate i
    if (doff[q] != i) atomicMin(bad, q);         // (its first candidate has no predecessor)
  }
}

// One workgroup per (query, tile): the tile's candidates, fp64 accumulators, hit
// counts and -- under BM25 -- norms (from dl directly) in LDS.  The slots go in
// batches of kNT: every thread narrows one slot's posting list to the postings
// whose docno lies in [the tile's first candidate, its last] by two binary
// searches; then the batch's slots in listed order, each in one of two forms:
//   scan    lanes walk the narrowed range, coalesced, and look each posting's docno
//           up in the LDS candidate array
//   search  lanes take candidates and binary-search the narrowed range in global
//           memory
// Docnos are distinct within a list and within a tile, so a slot writes no
// accumulator twice; the barrier that ends a slot fixes the summation order, the
// listed order, so both forms give the same bits.  A slot without a posting in the
// range costs nothing.
__global__ __launch_bounds__(kNT) void k_rs_score(const ScoreArgs A) {
  __shared__ double s_acc[kTile];
  __shared__ double s_norm[kTile];
  __shared__ int64_t s_lo[kNT];
  __shared__ int64_t s_n[kNT];
  __shared__ double s_idf[kNT];
  __shared__ int32_t s_doc[kTile];
  __shared__ int32_t s_hits[kTile];
  __shared__ unsigned long long s_found;
  const int tid = threadIdx.x;
  if (*A.bad != INT_MAX) return;  // (uniform: written before this launch)
  for (int64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    const int q = tile_query(A.toff, A.nq, tile);
    const int64_t c0 = A.doff[q] + (tile - A.toff[q]) * kTile;
    const int L = (int)min((int64_t)kTile, A.doff[q + 1] - c0);  // >= 1: only candidates make tiles
    if (tid == 0) s_found = 0;
    for (int j = tid; j < L; j += kNT) {
      const int32_t d = A.cand[c0 + j];
      s_doc[j] = d;
      s_acc[j] = 0.0;
      s_hits[j] = 0;
      if (A.model == MODEL_BM25) {
        // a candidate outside the index's docno range has no posting and no norm
        const int64_t i = (int64_t)d - A.dmin;
        s_norm[j] = i >= 0 && i < A.span ? bm25::doc_norm(A.k1, A.b, (double)A.dl[i], A.avgdl) : 0.0;
      }
    }
    __syncthreads();
    const int32_t first = s_doc[0], last = s_doc[L - 1];
    const int64_t q0 = A.qoff[q];
    const int ns = (int)min(A.qoff[q + 1] - q0, (int64_t)kMaxSlots);
    for (int sb = 0; sb < ns; sb += kNT) {
      if (sb + tid < ns) {
        const int32_t t = A.terms[q0 + sb + tid];
        int64_t lo = 0, n = 0;
        double idf = 0.0;
        if (t >= 0 && t < A.V) {
          const int64_t beg = A.off[t], cnt = A.off[t + 1] - beg;
          const int64_t a = lower_bound(A.dn + beg, cnt, first);
          n = upper_bound(A.dn + beg + a, cnt - a, last);
          lo = beg + a;
          if (A.model == MODEL_BM25) idf = A.idf[t];
        }
        s_lo[tid] = lo;
        s_n[tid] = n;
        s_idf[tid] = idf;
      }
      __syncthreads();
      const int nb = min(kNT, ns - sb);
      for (int x = 0; x < nb; x++) {
        const int64_t n = s_n[x];
        if (n == 0) continue;  // (uniform)
        const int64_t lo = s_lo[x];
        const double idf = s_idf[x];
        const bool scan = A.path == PATH_SCAN || (A.path == PATH_AUTO && scan_is_cheaper(n, L));
        if (scan) {
          for (int64_t i = tid; i < n; i += kNT) {
            const int32_t d = A.dn[lo + i];
            const int32_t tf = A.model == MODEL_BM25 ? A.tf[lo + i] : 0;  // (with the docno, not behind the lookup)
            const double w = A.model == MODEL_BM25 ? 0.0 : A.w[lo + i];
            const int j = lower_bound((const int32_t *)s_doc, L, d);
            if (j < L && s_doc[j] == d) {
              s_acc[j] += A.model == MODEL_BM25 ? bm25::weight(idf, (double)tf, A.k1, s_norm[j]) : w;
              s_hits[j]++;
            }
          }
        } else {
          for (int j = tid; j < L; j += kNT) {
            const int32_t d = s_doc[j];
            const int64_t p = lower_bound(A.dn + lo, n, d);
            if (p < n && A.dn[lo + p] == d) {
              s_acc[j] += A.model == MODEL_BM25 ? bm25::weight(idf, (double)A.tf[lo + p], A.k1, s_norm[j]) : A.w[lo + p];
              s_hits[j]++;
            }
          }
        }
        __syncthreads();
      }
      __syncthreads();  // (the next batch rewrites the slot tables)
    }
    unsigned long long fnd = 0;
    int64_t kept = 0;
    for (int r = 0; r < kTile; r += kNT) {
      if (r >= L) break;  // (uniform)
      const int j = r + tid;
      int h = -1;
      if (j < L) {
        h = s_hits[j];
        A.score[c0 + j] = s_acc[j];
        A.hits[c0 + j] = h;
        fnd += (unsigned long long)h;
      }
      kept += __syncthreads_count(h >= A.min_hits);
    }
    if (fnd) atomicAdd(&s_found, fnd);
    __syncthreads();
    if (tid == 0) {
      A.tkept[tile] = kept;
      if (s_found) atomicAdd(A.found, s_found);
    }
    __syncthreads();  // (the next tile rewrites everything)
  }
}

// woff[i] = matches before query i's first tile (i = nq: all of them)
__global__ void k_rs_woff(const int64_t *__restrict__ moff, const int64_t *__restrict__ toff, int64_t nq,
                          int64_t *__restrict__ woff) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nq; i += (int64_t)gridDim.x * blockDim.x)
    woff[i] = moff[toff[i]];
}

// The kept candidates of every tile, in the given order.  DIRECT (order 0): kept
// candidate number rk of its query goes to roff[q] + rk if that is below the cut.
// Else: match number moff[tile] + rank of the batch into the match arrays.
template <bool DIRECT>
__global__ __launch_bounds__(kNT) void k_rs_emit(const int32_t *__restrict__ cand, const int64_t *__restrict__ doff,
                                                 const int64_t *__restrict__ toff, int nq, int64_t ntiles,
                                                 const int32_t *__restrict__ hits, const double *__restrict__ score,
                                                 int min_hits, const int64_t *__restrict__ moff,
                                                 const int64_t *__restrict__ roff,
                                                 int32_t *__restrict__ odoc, int32_t *__restrict__ ohits,
                                                 double *__restrict__ oscore, uint32_t *__restrict__ oq) {
  __shared__ int s_w[kNT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int q = tile_query(toff, nq, tile);
    const int64_t c0 = doff[q] + (tile - toff[q]) * kTile;
    const int L = (int)min((int64_t)kTile, doff[q + 1] - c0);
    int64_t run = DIRECT ? roff[q] + (moff[tile] - moff[toff[q]]) : moff[tile];
    const int64_t end = DIRECT ? roff[q + 1] : moff[tile + 1];  // (the cut is in roff)
    for (int r = 0; r < L && run < end; r += kNT) {  // (uniform)
      const int j = r + tid;
      const int h = j < L ? hits[c0 + j] : -1;
      const bool keep = h >= min_hits;
      const unsigned long long mk = __ballot(keep);
      if (lane == 0) s_w[wv] = __popcll(mk);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kNT / 64; w++) {
        const int ws = s_w[w];
        before += w < wv ? ws : 0;
        total += ws;
      }
      const int64_t at = run + before + __popcll(mk & ((1ull << lane) - 1));
      if (keep && at < end) {
        odoc[at] = cand[c0 + j];
        ohits[at] = h;
        oscore[at] = score[c0 + j];
        if (!DIRECT) oq[at] = (uint32_t)q;
      }
      run += total;
      __syncthreads();  // (s_w is rewritten by the next round)
    }
  }
}

// the score key of every match and the identity permutation ...
__global__ void k_rs_key_score(const double *__restrict__ mscore, int64_t n, uint64_t *__restrict__ key,
                               uint32_t *__restrict__ perm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    key[i] = boolq::score_key(mscore[i]);
    perm[i] = (uint32_t)i;
  }
}
// ... and, through the permutation so far, the query
__global__ void k_rs_key_query(const uint32_t *__restrict__ mq, const uint32_t *__restrict__ perm, int64_t n,
                               uint32_t *__restrict__ key) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    key[i] = mq[perm[i]];
}
// Sorted match x (query qs[x], match perm[x]) is the (x - woff[q])-th of its query:
// kept if that is below the cut.
__global__ void k_rs_gather(const uint32_t *__restrict__ qs, const uint32_t *__restrict__ perm,
                            const int32_t *__restrict__ mdoc, const int32_t *__restrict__ mhits,
                            const double *__restrict__ mscore, int64_t total, const int64_t *__restrict__ woff,
                            const int64_t *__restrict__ roff, int64_t m, int32_t *__restrict__ odoc,
                            int32_t *__restrict__ ohits, double *__restrict__ oscore) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t q = qs[x];
    const int64_t rk = x - woff[q];
    if (m > 0 && rk >= m) continue;
    const uint32_t i = perm[x];
    odoc[roff[q] + rk] = mdoc[i];
    ohits[roff[q] + rk] = mhits[i];
    oscore[roff[q] + rk] = mscore[i];
  }
}

std::string at_query(int q) { return q >= 0 ? " (query " + std::to_string(q) + ")" : std::string(); }

}  // namespace

void rescore_docs(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *docnos,
                  bool on_device, const int64_t *d_offsets, const int64_t *d_offsets_dev, int nq, int model, double k1,
                  double b, int min_hits, int order, int m, hipStream_t st) {
  sme_ctx *cx = ix->ctx;
  DocFreqScores &out = ix->rs;
  out.reset();  // whatever ends the call from here on leaves an empty result behind
  int bad = -1;
  const int rc = validate(term_ids, -1, q_offsets, on_device ? nullptr : docnos, -1, d_offsets, nq, ix->V, &bad);
  switch (rc) {
    case R_OK:
      break;
    case R_QOFFSETS:
      throw Error(SME_EINVAL, "rescore: q_offsets do not ascend from 0" + at_query(bad));
    case R_DOFFSETS:
      throw Error(SME_EINVAL, "rescore: d_offsets do not ascend from 0" + at_query(bad));
    case R_SLOTS:
      throw Error(SME_ELIMIT, "rescore: more than " + std::to_string(kMaxSlots) + " term slots" + at_query(bad));
    case R_BATCH:
      throw Error(SME_ELIMIT, "rescore: 2^31 or more candidates or term slots in one batch");
    case R_TERM:
      throw Error(SME_EINVAL, "rescore: a term id outside [-1, V)" + at_query(bad));
    default:
      throw Error(SME_EINVAL, "rescore: candidates not strictly ascending" + at_query(bad));
  }
  int64_t *d_roff = out.offsets(nq);
  if (nq == 0) {
    SME_HIP(hipMemsetAsync(d_roff, 0, sizeof(int64_t), st));
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  if (model == MODEL_BM25) prepare_bm25(ix, st);
  const int64_t nt = q_offsets[nq], total = d_offsets[nq];
  std::vector<int64_t> toff((size_t)nq + 1, 0);
  for (int q = 0; q < nq; q++) toff[(size_t)q + 1] = toff[(size_t)q] + (d_offsets[q + 1] - d_offsets[q] + kTile - 1) / kTile;
  const int64_t ntiles = toff[(size_t)nq];
  // one upload: slot offsets | tile offsets | candidate offsets | term ids
  Blob blob;
  const size_t a_qoff = blob.add(q_offsets, (size_t)nq + 1);
  const size_t a_toff = blob.add(toff.data(), (size_t)nq + 1);
  const size_t a_doff = blob.add(d_offsets, (size_t)nq + 1);
  const size_t a_term = blob.add(term_ids, (size_t)nt);
  // temporaries of this call: pooled blocks, back in the pool on return
  DevBuf in, cnb, scb, htb, tkb, wob, kpb, scn, ctr, mdb, mhb, msb, mqb, sa, sb, pa, pb, ka, kb, radix;
  for (DevBuf *p : {&in, &cnb, &scb, &htb, &tkb, &wob, &kpb, &scn, &ctr, &mdb, &mhb, &msb, &mqb, &sa, &sb, &pa, &pb, &ka,
                    &kb, &radix})
    p->pool = &cx->pool;
  try {
    const uint8_t *d_in = in.as<uint8_t>(blob.bytes.size());
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st));
    const int64_t *d_toff = (const int64_t *)(d_in + a_toff);
    const int64_t *d_doff = on_device ? d_offsets_dev : (const int64_t *)(d_in + a_doff);
    const int32_t *d_cand = docnos;
    if (!on_device) {
      int32_t *c = cnb.as<int32_t>((size_t)total);
      if (total) SME_HIP(hipMemcpyAsync(c, docnos, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, st));
      d_cand = c;
    }
    struct Counters {
      unsigned long long found;
      int bad;
    } h{0, INT_MAX};
    Counters *d_ctr = ctr.as<Counters>(1);
    SME_HIP(hipMemcpyAsync(d_ctr, &h, sizeof h, hipMemcpyHostToDevice, st));
    double *score = scb.as<double>((size_t)total);
    int32_t *hits = htb.as<int32_t>((size_t)total);
    int64_t *moff = tkb.as<int64_t>((size_t)ntiles + 1);
    SME_HIP(hipMemsetAsync(moff + ntiles, 0, sizeof(int64_t), st));
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min(ntiles, kMaxGrid));
    if (ntiles > 0) {
      if (on_device) {
        hipLaunchKernelGGL(k_rs_check, dim3(grid_for(total)), dim3(kNT), 0, st, d_cand, d_doff, nq, total, &d_ctr->bad);
        SME_CHECK_LAUNCH();
      }
      ScoreArgs A;
      A.off = (const int64_t *)ix->d_off.p;
      A.dn = (const int32_t *)ix->d_docno_d.p;
      A.tf = (const int32_t *)ix->d_tf_d.p;
      A.w = (const double *)ix->d_w.p;
      A.idf = (const double *)ix->d_bm_idf.p;
      A.dl = (const int32_t *)ix->d_bm_dl.p;
      A.terms = (const int32_t *)(d_in + a_term);
      A.qoff = (const int64_t *)(d_in + a_qoff);
      A.cand = d_cand;
      A.doff = d_doff;
      A.toff = d_toff;
      A.nq = nq;
      A.ntiles = ntiles;
      A.V = ix->V;
      A.dmin = ix->dmin;
      A.span = model == MODEL_BM25 ? ix->bm_span : 0;
      A.model = model;
      A.path = (int)cx->opt_rescore_path;
      A.min_hits = min_hits;
      A.k1 = k1;
      A.b = b;
      A.avgdl = model == MODEL_BM25 && ix->bm_docs ? (double)ix->bm_total_len / (double)ix->bm_docs : 1.0;
      A.bad = &d_ctr->bad;
      A.score = score;
      A.hits = hits;
      A.tkept = moff;
      A.found = &d_ctr->found;
      hipLaunchKernelGGL(k_rs_score, dim3(grid), dim3(kNT), 0, st, A);
      SME_CHECK_LAUNCH();
    }
    // matches before every tile, before every query, and the result offsets after the cut
    excl_scan<int64_t>(moff, moff, ntiles + 1, scn, st);
    int64_t *woff = wob.as<int64_t>((size_t)nq + 1);
    int64_t *kept = kpb.as<int64_t>((size_t)nq + 1);
    hipLaunchKernelGGL(k_rs_woff, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, (const int64_t *)moff, d_toff,
                       (int64_t)nq, woff);
    hipLaunchKernelGGL(k_cut, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, (const int64_t *)woff, (int64_t)nq,
                       (int64_t)m, kept);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(kept, d_roff, (int64_t)nq + 1, scn, st);
    int64_t out_total = 0, matches = 0;
    SME_HIP(hipMemcpyAsync(&out_total, d_roff + nq, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipMemcpyAsync(&matches, moff + ntiles, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipMemcpyAsync(&h, d_ctr, sizeof h, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    if (h.bad != INT_MAX) {
      SME_HIP(hipMemsetAsync(d_roff, 0, ((size_t)nq + 1) * sizeof(int64_t), st));
      SME_HIP(hipStreamSynchronize(st));
      throw Error(SME_EINVAL, "rescore: candidates not strictly ascending" + at_query(h.bad));
    }
    int32_t *odoc = out.alloc<DocFreqScores::docno>(out_total);
    int32_t *ohits = out.alloc<DocFreqScores::freq>(out_total);
    double *oscore = out.alloc<DocFreqScores::score>(out_total);
    if (matches > 0 && order == 0) {
      hipLaunchKernelGGL(k_rs_emit<true>, dim3(grid), dim3(kNT), 0, st, d_cand, d_doff, d_toff, nq, ntiles,
                         (const int32_t *)hits, (const double *)score, min_hits, (const int64_t *)moff,
                         (const int64_t *)d_roff, odoc, ohits, oscore, (uint32_t *)nullptr);
      SME_CHECK_LAUNCH();
    } else if (matches > 0) {
      const size_t T = (size_t)matches;
      int32_t *mdoc = mdb.as<int32_t>(T), *mhits = mhb.as<int32_t>(T);
      double *mscore = msb.as<double>(T);
      uint32_t *mq = mqb.as<uint32_t>(T);
      hipLaunchKernelGGL(k_rs_emit<false>, dim3(grid), dim3(kNT), 0, st, d_cand, d_doff, d_toff, nq, ntiles,
                         (const int32_t *)hits, (const double *)score, min_hits, (const int64_t *)moff,
                         (const int64_t *)d_roff, mdoc, mhits, mscore, mq);
      SME_CHECK_LAUNCH();
      // the matches lie in (query, docno) order: a stable sort by the score key, one by
      // the query, and the order is (query, score descending, docno ascending)
      uint64_t *s0 = sa.as<uint64_t>(T), *s1 = sb.as<uint64_t>(T);
      uint32_t *p0 = pa.as<uint32_t>(T), *p1 = pb.as<uint32_t>(T);
      uint32_t *k0 = ka.as<uint32_t>(T), *k1q = kb.as<uint32_t>(T);
      const unsigned g = grid_for(matches);
      hipLaunchKernelGGL(k_rs_key_score, dim3(g), dim3(kNT), 0, st, (const double *)mscore, matches, s0, p0);
      sort_pairs<uint64_t>(s0, s1, p0, p1, matches, 64, radix, st);
      hipLaunchKernelGGL(k_rs_key_query, dim3(g), dim3(kNT), 0, st, (const uint32_t *)mq, (const uint32_t *)p1, matches,
                         k0);
      sort_pairs<uint32_t>(k0, k1q, p1, p0, matches, owner_bits(nq), radix, st);
      hipLaunchKernelGGL(k_rs_gather, dim3(g), dim3(kNT), 0, st, (const uint32_t *)k1q, (const uint32_t *)p0,
                         (const int32_t *)mdoc, (const int32_t *)mhits, (const double *)mscore, matches,
                         (const int64_t *)woff, (const int64_t *)d_roff, (int64_t)m, odoc, ohits, oscore);
      SME_CHECK_LAUNCH();
    }
    SME_HIP(hipStreamSynchronize(st));
    out.total = out_total;
    out.cands = (uint64_t)total;
    out.verified = h.found;
    out.matches = (uint64_t)matches;
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the upload may still read `blob`, kernels the temporaries
    throw;
  }
}

}  // namespace sme
