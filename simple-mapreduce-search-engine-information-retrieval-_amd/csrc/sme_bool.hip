// sme_bool.hip -- Boolean retrieval: a batch of queries, each a list of groups of
// term ids (a required group: the document lies in at least one of its posting
// lists; an excluded group: in none) -> per query the matching documents with
// their TF-IDF scores, ordered by docno or by score and cut to the first m, over
// the query-side CSR (d_off / d_docno_d / d_w).
//
// k_bool_plan picks per query the driver, the required group with the fewest
// postings (or the first one), whose slots' posting lists are the candidates; the
// candidate ranges are cut into chunks, and the chunk filter of sme_chunks.hpp --
// once counting, once emitting -- tests every candidate against the query's other
// lists by binary searches bounded to the chunk's docno range (BoolOp), one
// workgroup per chunk, one candidate per thread, and sums a survivor's weights in
// listed slot order.
// Stable sorts over an index permutation (docno, then the score key, then the
// query) and a gather order and cut the matches (sme_bool_tail.hpp, shared with
// structured queries).  Every candidate is tested against every group, so the
// driver never changes a result.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sme_bool.hpp"
#include "sme_bool_tail.hpp"
#include "sme_chunks.hpp"
#include "sme_internal.hpp"

namespace sme {
namespace {
using namespace chunks;

struct Batch {           // the uploaded batch (device pointers into one block)
  const int64_t *goff;   // [ngroups + 1] slot offsets
  const int64_t *qoff;   // [nq + 1] group offsets
  const int32_t *term;   // [nt] term id per slot (-1: no postings)
  const uint8_t *gflag;  // [ngroups] 0 required, 1 excluded
};

// One thread per query.  Per slot s: its posting list docno[sbeg .. sbeg + scnt)
// and its query sq; per query the driver group qdrv (-1: the query matches
// nothing -- no required group, or a required group without a posting); nchunk[s]
// = chunks of slot s as a candidate range (driver slots only; entry nt = 0).
// *cands += the driver's postings.
__global__ void k_bool_plan(Batch b, int nq, int64_t nt, const int64_t *__restrict__ doff, int chunk, int first_driver,
                            int64_t *__restrict__ sbeg, int32_t *__restrict__ scnt, int32_t *__restrict__ sq,
                            int32_t *__restrict__ qdrv, int64_t *__restrict__ nchunk,
                            unsigned long long *__restrict__ cands) {
  // (64-bit counters: nq + the grid's stride may pass INT_MAX)
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q <= nq; q += (int64_t)gridDim.x * blockDim.x) {
    if (q == nq) {
      nchunk[nt] = 0;
      continue;
    }
    const int64_t g0 = b.qoff[q], g1 = b.qoff[q + 1];
    int64_t drv = -1, best = 0;
    bool dead = false;
    for (int64_t g = g0; g < g1; g++) {
      int64_t sum = 0;
      for (int64_t s = b.goff[g]; s < b.goff[g + 1]; s++) {
        const int32_t t = b.term[s];
        const int64_t beg = t < 0 ? 0 : doff[t];
        const int64_t cnt = t < 0 ? 0 : doff[t + 1] - beg;
        sbeg[s] = beg;
        scnt[s] = (int32_t)cnt;
        sq[s] = (int32_t)q;
        sum += cnt;
      }
      if (b.gflag[g] != 0) continue;
      dead |= sum == 0;
      if (drv < 0 || (!first_driver && sum < best)) {
        drv = g;
        best = sum;
      }
    }
    if (dead) drv = -1;
    qdrv[q] = (int32_t)(drv < 0 ? -1 : drv - g0);
    const int64_t d0 = drv < 0 ? 0 : b.goff[drv], d1 = drv < 0 ? 0 : b.goff[drv + 1];
    for (int64_t s = b.goff[g0]; s < b.goff[g1]; s++)
      nchunk[s] = s >= d0 && s < d1 ? ((int64_t)scnt[s] + chunk - 1) / chunk : 0;
    if (drv >= 0) atomicAdd(cands, (unsigned long long)best);
  }
}

// the posting of document d in docno[start .. start + n), or -1
__device__ __forceinline__ int64_t find_doc(const int32_t *__restrict__ docno, int64_t start, int n, int32_t d) {
  const int at = lower_bound(docno + start, n, d);
  return at < n && docno[start + at] == d ? start + at : -1;
}

// The chunk filter's Op (sme_chunks.hpp): range = slot (driver slots own chunks),
// candidate c of it the posting sbeg[r] + c, so a chunk is at most `chunk`
// consecutive postings of one driver slot.  The chunk's docnos lie in [first,
// last]; per slot of the query the sub-range of its list that can hold such a
// docno (two bounds) is staged in LDS, with the groups' slot ranges and flags.
// A required group other than the driver whose sub-ranges are all empty rejects
// the whole chunk.  A candidate: every other required group must hold it (OR over
// the group's slots), no excluded slot may, and one an earlier slot of the driver
// group also holds is dropped, so a document is emitted once per query.  Emitted:
// the match's docno, query and score -- the sum from 0.0 of w at its posting over
// the required slots in listed order.
struct BoolOp {
  Batch b;
  const int64_t *sbeg;
  const int32_t *scnt;
  const int32_t *sq;
  const int32_t *qdrv;
  const int32_t *docno;
  const double *w;
  struct Lds {
    int64_t start[boolq::kMaxSlots];
    int32_t len[boolq::kMaxSlots];
    int32_t gbeg[boolq::kMaxGroups + 1];
    int reject;
    uint8_t gflag[boolq::kMaxGroups];
  };
  struct Chunk {
    int q, ng, dg, ds;
    int64_t base;  // the driver slot's first posting
  };
  struct Cand {
    int32_t d;
  };
  __device__ __forceinline__ bool stage(Lds &s, Chunk &k, int64_t r, int64_t c0, int len) const {
    const int tid = threadIdx.x;
    k.q = sq[r];
    const int64_t g0 = b.qoff[k.q];
    k.ng = (int)(b.qoff[k.q + 1] - g0);  // <= kMaxGroups (validated on the host)
    const int64_t s0 = b.goff[g0];
    const int S = (int)(b.goff[g0 + k.ng] - s0);  // <= kMaxSlots
    k.dg = qdrv[k.q];
    k.ds = (int)(r - s0);
    k.base = sbeg[r];
    const int32_t first = docno[k.base + c0], last = docno[k.base + c0 + len - 1];
    if (tid <= k.ng) s.gbeg[tid] = (int32_t)(b.goff[g0 + tid] - s0);
    if (tid < k.ng) s.gflag[tid] = b.gflag[g0 + tid];
    if (tid == 0) s.reject = 0;
    for (int j = tid; j < S; j += kNT) {
      const int64_t beg = sbeg[s0 + j];
      const int n = scnt[s0 + j];
      const int lo = lower_bound(docno + beg, n, first);
      const int hi = lo + upper_bound(docno + beg + lo, n - lo, last);
      s.start[j] = beg + lo;
      s.len[j] = hi - lo;
    }
    __syncthreads();
    if (tid < k.ng && tid != k.dg && s.gflag[tid] == 0) {
      int any = 0;
      for (int j = s.gbeg[tid]; j < s.gbeg[tid + 1]; j++) any |= s.len[j];
      if (any == 0) s.reject = 1;
    }
    __syncthreads();
    return s.reject == 0;
  }
  __device__ __forceinline__ bool test(const Lds &s, const Chunk &k, int64_t, int64_t c, Cand &x) const {
    const int32_t d = x.d = docno[k.base + c];
    bool hit = true;
    for (int g = 0; hit && g < k.ng; g++) {
      if (g == k.dg || s.gflag[g] != 0) continue;
      bool held = false;
      for (int j = s.gbeg[g]; !held && j < s.gbeg[g + 1]; j++) held = find_doc(docno, s.start[j], s.len[j], d) >= 0;
      hit = held;
    }
    for (int g = 0; hit && g < k.ng; g++) {
      if (s.gflag[g] == 0) continue;
      for (int j = s.gbeg[g]; hit && j < s.gbeg[g + 1]; j++) hit = find_doc(docno, s.start[j], s.len[j], d) < 0;
    }
    for (int j = s.gbeg[k.dg]; hit && j < k.ds; j++) hit = find_doc(docno, s.start[j], s.len[j], d) < 0;
    return hit;
  }
  __device__ __forceinline__ void emit(const Lds &s, const Chunk &k, int64_t, const Cand &x, int64_t at,
                                       int32_t *__restrict__ mdoc, double *__restrict__ mscore,
                                       uint32_t *__restrict__ mq) const {
    double sc = 0.0;
    for (int g = 0; g < k.ng; g++) {
      if (s.gflag[g] != 0) continue;
      for (int j = s.gbeg[g]; j < s.gbeg[g + 1]; j++) {
        const int64_t p = find_doc(docno, s.start[j], s.len[j], x.d);
        if (p >= 0) sc += w[p];
      }
    }
    mdoc[at] = x.d;
    mscore[at] = sc;
    mq[at] = (uint32_t)k.q;
  }
};
struct FirstRange {  // query i's first slot; a query without slots has the next one's
  const int64_t *goff, *qoff;
  __device__ int64_t operator()(int64_t i) const { return goff[qoff[i]]; }
};
}  // namespace

void query_boolean(sme_index *ix, const int32_t *term_ids, const int64_t *g_offsets, const uint8_t *g_flags,
                   const int64_t *q_offsets, int nq, int order, int m, hipStream_t st) {
  sme_ctx *cx = ix->ctx;
  int bad = -1;
  const int rc = boolq::validate(term_ids, -1, g_offsets, -1, g_flags, q_offsets, nq, ix->V, &bad);
  const std::string where = bad >= 0 ? "query " + std::to_string(bad) + ": " : std::string();
  switch (rc) {
    case boolq::B_OK:
      break;
    case boolq::B_OFFSETS:
      throw Error(SME_EINVAL, "boolean " + where + "offsets not ascending from 0 or inconsistent");
    case boolq::B_FLAG:
      throw Error(SME_EINVAL, "boolean " + where + "a group flag other than 0 (required) or 1 (excluded)");
    case boolq::B_GROUPS:
      throw Error(SME_ELIMIT, "boolean " + where + "more than 64 groups");
    case boolq::B_SLOTS:
      throw Error(SME_ELIMIT, "boolean " + where + "more than 1024 term slots");
    default:
      throw Error(SME_EINVAL, "boolean " + where + "a term id outside [-1, V)");
  }
  DocScores &out = ix->bq;
  out.reset();
  int64_t *d_roff = out.offsets(nq);
  if (nq == 0) {
    SME_HIP(hipMemsetAsync(d_roff, 0, sizeof(int64_t), st));
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  const int64_t ng = q_offsets[nq], nt = g_offsets[ng];
  if (nt >= (int64_t(1) << 31)) throw Error(SME_ELIMIT, "boolean batch: 2^31 or more term slots");
  // one upload: slot offsets | group offsets | term ids | flags
  Blob blob;
  const size_t a_goff = blob.add(g_offsets, (size_t)ng + 1);
  const size_t a_qoff = blob.add(q_offsets, (size_t)nq + 1);
  const size_t a_term = blob.add(term_ids, (size_t)nt);
  const size_t a_flag = blob.add(g_flags, (size_t)ng);
  const int chunk = (int)cx->opt_bool_chunk;
  const int64_t R = nt;  // one candidate range per slot (driver slots own chunks)
  // temporaries of this call: pooled blocks, back in the pool on return
  DevBuf in, sbb, scb, sqb, qdb, chb, mob, cnd, scn;
  for (DevBuf *b : {&in, &sbb, &scb, &sqb, &qdb, &chb, &mob, &cnd, &scn}) b->pool = &cx->pool;
  try {
    const uint8_t *d_in = in.as<uint8_t>(blob.bytes.size());
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st));
    const Batch b{(const int64_t *)(d_in + a_goff), (const int64_t *)(d_in + a_qoff), (const int32_t *)(d_in + a_term),
                  (const uint8_t *)(d_in + a_flag)};
    int64_t *sbeg = sbb.as<int64_t>((size_t)nt);
    int32_t *scnt = scb.as<int32_t>((size_t)nt);
    int32_t *sq = sqb.as<int32_t>((size_t)nt);
    int32_t *qdrv = qdb.as<int32_t>((size_t)nq);
    int64_t *choff = chb.as<int64_t>((size_t)R + 1);
    unsigned long long *d_cands = cnd.as<unsigned long long>(1);
    const int64_t *doff = (const int64_t *)ix->d_off.p;
    const int32_t *docno = (const int32_t *)ix->d_docno_d.p;
    const double *w = (const double *)ix->d_w.p;
    SME_HIP(hipMemsetAsync(d_cands, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_bool_plan, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, b, nq, nt, doff, chunk,
                       (int)cx->opt_bool_driver, sbeg, scnt, sq, qdrv, choff, d_cands);
    SME_CHECK_LAUNCH();
    unsigned long long cands = 0;
    const BoolOp op{b, sbeg, scnt, sq, qdrv, docno, w};
    const Counted c = count_chunks(op, (int)R, choff, scnt, chunk, mob, scn,
                                   "boolean: 2^31 or more matches in one batch", st, d_cands, &cands);
    bool_tail(cx, op, c, FirstRange{b.goff, b.qoff}, order, m, out, st);
    out.cands = (uint64_t)cands;
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the upload may still read `blob`, kernels the temporaries
    throw;
  }
}

}  // namespace sme
