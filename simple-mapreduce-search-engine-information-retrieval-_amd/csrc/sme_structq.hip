// sme_structq.hip -- structured queries: Boolean retrieval (sme_bool.hip) whose
// group members are leaves -- a term, or an ordered / unordered window over terms
// (sme_near.hip; a phrase is the ordered window of width 1) -- so that one call
// answers and scores `"new york" hotel* -"times square"`.  include/sme.h has the
// semantics in full.
//
// The batch's operator leaves go through the proximity pass (near_pass) once, in
// docno order and uncut, into buffers of their own on the index: per leaf a
// virtual posting list, docnos and values.  The Boolean stage is sme_bool.hip's
// with a list descriptor per slot -- where its documents and values stand, from
// where, how many -- in place of "the term's range in the CSR": k_structq_plan
// fills the descriptors from the uploaded leaf table, StructOp is BoolOp reading
// through them, and the tail (sme_bool_tail.hpp) is shared.
//
// Narrowing: a document outside any required group that holds term leaves only
// cannot be a result, so an operator leaf need not be verified there -- the pass's
// candidate filter also tests those groups (NarrowOp, sme_phrase_pass.hpp) and the
// position scan runs over what is left.  Only in SME_IDF_REFERENCE, where a leaf's
// value does not depend on its full document frequency.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sme_bool.hpp"
#include "sme_bool_tail.hpp"
#include "sme_chunks.hpp"
#include "sme_internal.hpp"
#include "sme_structq.hpp"

namespace sme {
namespace {
using namespace chunks;

struct Batch {           // the uploaded batch (device pointers into one block)
  const int64_t *goff;   // [ngroups + 1] leaf offsets
  const int64_t *qoff;   // [nq + 1] group offsets
  const int32_t *lref;   // [nl] per leaf: a term id (-1: no postings), or -2 - i for operator leaf i
  const uint8_t *gflag;  // [ngroups] 0 required, 1 excluded
};

// One thread per query: k_bool_plan over list descriptors.  Per slot s (a leaf):
// its list is entries [sbeg, sbeg + scnt) of the CSR's docno / weight arrays
// (svirt 0: a term leaf, the term's postings) or of the virtual lists' (svirt 1:
// operator leaf i, [voff[i], voff[i + 1])), and its query sq; per query the driver
// group qdrv (-1: the query matches nothing -- no required group, or a required
// group without an entry); nchunk[s] = chunks of slot s as a candidate range
// (driver slots only; entry nl = 0).  *cands += the driver's entries.
__global__ void k_structq_plan(Batch b, int nq, int64_t nl, const int64_t *__restrict__ doff,
                               const int64_t *__restrict__ voff, int chunk, int first_driver,
                               int64_t *__restrict__ sbeg, int32_t *__restrict__ scnt, uint8_t *__restrict__ svirt,
                               int32_t *__restrict__ sq, int32_t *__restrict__ qdrv, int64_t *__restrict__ nchunk,
                               unsigned long long *__restrict__ cands) {
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q <= nq; q += (int64_t)gridDim.x * blockDim.x) {
    if (q == nq) {
      nchunk[nl] = 0;
      continue;
    }
    const int64_t g0 = b.qoff[q], g1 = b.qoff[q + 1];
    int64_t drv = -1, best = 0;
    bool dead = false;
    for (int64_t g = g0; g < g1; g++) {
      int64_t sum = 0;
      for (int64_t s = b.goff[g]; s < b.goff[g + 1]; s++) {
        const int32_t t = b.lref[s];
        const bool virt = t < -1;
        const int64_t *off = virt ? voff + (-2 - (int64_t)t) : doff + (t < 0 ? 0 : t);  // (t == -1: not read)
        const int64_t beg = t == -1 ? 0 : off[0];
        const int64_t cnt = t == -1 ? 0 : off[1] - beg;  // a list holds fewer than 2^31 documents
        sbeg[s] = beg;
        scnt[s] = (int32_t)cnt;
        svirt[s] = virt;
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

// the entry of document d in docno[start .. start + n), or -1
__device__ __forceinline__ int64_t find_doc(const int32_t *__restrict__ docno, int64_t start, int n, int32_t d) {
  const int at = lower_bound(docno + start, n, d);
  return at < n && docno[start + at] == d ? start + at : -1;
}

// The chunk filter's Op (sme_chunks.hpp): BoolOp (sme_bool.hip) through the list
// descriptors.  range = slot (driver slots own chunks), candidate c of it the
// entry sbeg[r] + c of the slot's list.  Per slot of the query the sub-range of
// its list inside the chunk's docno range and which arrays it lies in are staged
// in LDS, with the groups' slot ranges and flags; the chunk rejection, the
// candidate test (every other required group holds it, no excluded slot does, no
// earlier slot of the driver group does) and the emitted match -- docno, query,
// the sum from 0.0 of the values over the required slots in listed order -- are
// BoolOp's.
struct StructOp {
  Batch b;
  const int64_t *sbeg;
  const int32_t *scnt;
  const uint8_t *svirt;
  const int32_t *sq;
  const int32_t *qdrv;
  const int32_t *docno;  // the CSR's documents and weights
  const double *w;
  const int32_t *vdoc;  // the virtual lists' documents and values
  const double *vval;
  struct Lds {
    int64_t start[structq::kMaxLeaves];
    int32_t len[structq::kMaxLeaves];
    int32_t gbeg[structq::kMaxGroups + 1];
    int reject;
    uint8_t gflag[structq::kMaxGroups];
    uint8_t virt[structq::kMaxLeaves];
  };
  struct Chunk {
    int q, ng, dg, ds;
    int64_t base;          // the driver slot's first entry
    const int32_t *ddoc;   // the array it lies in
  };
  struct Cand {
    int32_t d;
  };
  __device__ __forceinline__ const int32_t *docs(const Lds &s, int j) const { return s.virt[j] ? vdoc : docno; }
  __device__ __forceinline__ bool stage(Lds &s, Chunk &k, int64_t r, int64_t c0, int len) const {
    const int tid = threadIdx.x;
    k.q = sq[r];
    const int64_t g0 = b.qoff[k.q];
    k.ng = (int)(b.qoff[k.q + 1] - g0);  // <= kMaxGroups (validated on the host)
    const int64_t s0 = b.goff[g0];
    const int S = (int)(b.goff[g0 + k.ng] - s0);  // <= kMaxLeaves
    k.dg = qdrv[k.q];
    k.ds = (int)(r - s0);
    k.base = sbeg[r];
    k.ddoc = svirt[r] ? vdoc : docno;
    const int32_t first = k.ddoc[k.base + c0], last = k.ddoc[k.base + c0 + len - 1];
    if (tid <= k.ng) s.gbeg[tid] = (int32_t)(b.goff[g0 + tid] - s0);
    if (tid < k.ng) s.gflag[tid] = b.gflag[g0 + tid];
    if (tid == 0) s.reject = 0;
    for (int j = tid; j < S; j += kNT) {
      const int64_t beg = sbeg[s0 + j];
      const int n = scnt[s0 + j];
      const uint8_t v = svirt[s0 + j];
      const int32_t *dp = v ? vdoc : docno;
      const int lo = lower_bound(dp + beg, n, first);
      const int hi = lo + upper_bound(dp + beg + lo, n - lo, last);
      s.start[j] = beg + lo;
      s.len[j] = hi - lo;
      s.virt[j] = v;
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
    const int32_t d = x.d = k.ddoc[k.base + c];
    bool hit = true;
    for (int g = 0; hit && g < k.ng; g++) {
      if (g == k.dg || s.gflag[g] != 0) continue;
      bool held = false;
      for (int j = s.gbeg[g]; !held && j < s.gbeg[g + 1]; j++)
        held = find_doc(docs(s, j), s.start[j], s.len[j], d) >= 0;
      hit = held;
    }
    for (int g = 0; hit && g < k.ng; g++) {
      if (s.gflag[g] == 0) continue;
      for (int j = s.gbeg[g]; hit && j < s.gbeg[g + 1]; j++) hit = find_doc(docs(s, j), s.start[j], s.len[j], d) < 0;
    }
    for (int j = s.gbeg[k.dg]; hit && j < k.ds; j++) hit = find_doc(docs(s, j), s.start[j], s.len[j], d) < 0;
    return hit;
  }
  __device__ __forceinline__ void emit(const Lds &s, const Chunk &k, int64_t, const Cand &x, int64_t at,
                                       int32_t *__restrict__ mdoc, double *__restrict__ mscore,
                                       uint32_t *__restrict__ mq) const {
    double sc = 0.0;
    for (int g = 0; g < k.ng; g++) {
      if (s.gflag[g] != 0) continue;
      for (int j = s.gbeg[g]; j < s.gbeg[g + 1]; j++) {
        const int64_t p = find_doc(docs(s, j), s.start[j], s.len[j], x.d);
        if (p >= 0) sc += (s.virt[j] ? vval : w)[p];
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

void query_structured(sme_index *ix, const int32_t *term_ids, const int64_t *l_offsets, const uint8_t *l_kinds,
                      const int32_t *l_widths, const int64_t *g_offsets, const uint8_t *g_flags,
                      const int64_t *q_offsets, int nq, int order, int m, hipStream_t st) {
  sme_ctx *cx = ix->ctx;
  int bad = -1;
  int64_t ops = 0;
  const int rc = structq::validate(term_ids, -1, l_offsets, -1, l_kinds, l_widths, g_offsets, -1, g_flags, q_offsets,
                                   nq, ix->V, &bad, &ops);
  if (rc != structq::S_OK) {
    char msg[160];
    const bool limit = structq::describe(rc, bad, msg, sizeof msg);
    throw Error(limit ? SME_ELIMIT : SME_EINVAL, msg);
  }
  if (ops > 0) {  // what sme_query_near needs, in its words
    if (ix->K != 1) throw Error(SME_EINVAL, "proximity query: the index holds k-grams (K != 1), not terms");
    if (!ix->has_positions)
      throw Error(SME_EINVAL, "proximity query: the index keeps no positions (build it with option \"positions\" 1)");
  }
  DocScores &out = ix->sq;
  out.reset();
  ix->sq_leaves = 0;
  int64_t *d_roff = out.offsets(nq);
  if (nq == 0) {
    SME_HIP(hipMemsetAsync(d_roff, 0, sizeof(int64_t), st));
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  const int64_t ng = q_offsets[nq], nl = g_offsets[ng];
  // the leaf table, and the operator leaves as a proximity batch
  std::vector<int32_t> lref((size_t)nl);
  uint64_t verified = 0;
  if (ops == 0) {
    for (int64_t l = 0; l < nl; l++) lref[(size_t)l] = term_ids[l_offsets[l]];
  } else {
    const bool narrowing = cx->opt_struct_narrow != 0 && ix->idf_mode == SME_IDF_REFERENCE;
    std::vector<int64_t> n_off(1, 0);
    std::vector<int32_t> n_terms, n_widths;
    std::vector<uint8_t> n_kinds;
    NarrowSpec spec;
    spec.qgoff.push_back(0);
    spec.goff.push_back(0);
    for (int q = 0; q < nq; q++) {
      const int64_t l0 = g_offsets[q_offsets[q]], l1 = g_offsets[q_offsets[q + 1]];
      bool any = false;
      for (int64_t l = l0; l < l1; l++) {
        if (l_kinds[l] == structq::kTerm) {
          lref[(size_t)l] = term_ids[l_offsets[l]];
          continue;
        }
        lref[(size_t)l] = (int32_t)(-2 - (int64_t)n_widths.size());
        n_terms.insert(n_terms.end(), term_ids + l_offsets[l], term_ids + l_offsets[l + 1]);
        n_off.push_back((int64_t)n_terms.size());
        n_widths.push_back(l_widths[l]);
        n_kinds.push_back((uint8_t)(l_kinds[l] - 1));
        spec.owner.push_back((int32_t)spec.qgoff.size() - 1);
        any = true;
      }
      if (!any) continue;
      // the query's narrowing groups: required, term leaves only -- in listed order,
      // a group taken while kNarrowGroups groups and kNarrowSlots slots hold it
      int groups = 0;
      int64_t slots = 0;
      for (int64_t g = q_offsets[q]; narrowing && g < q_offsets[q + 1]; g++) {
        const int64_t a = g_offsets[g], e = g_offsets[g + 1];
        bool terms_only = g_flags[g] == 0;
        for (int64_t l = a; terms_only && l < e; l++) terms_only = l_kinds[l] == structq::kTerm;
        if (!terms_only || groups == kNarrowGroups || slots + (e - a) > kNarrowSlots) continue;
        for (int64_t l = a; l < e; l++) spec.terms.push_back(term_ids[l_offsets[l]]);
        spec.goff.push_back((int64_t)spec.terms.size());
        groups++;
        slots += e - a;
      }
      spec.qgoff.push_back((int64_t)spec.goff.size() - 1);
    }
    near_pass(ix, ix->sv, n_terms.data(), n_off.data(), n_widths.data(), n_kinds.data(), (int)ops, 0, 0,
              narrowing ? &spec : nullptr, st);
    verified = ix->sv.verified;
  }
  // one upload: leaf offsets | group offsets | leaf table | flags
  Blob blob;
  const size_t a_goff = blob.add(g_offsets, (size_t)ng + 1);
  const size_t a_qoff = blob.add(q_offsets, (size_t)nq + 1);
  const size_t a_lref = blob.add(lref.data(), (size_t)nl);
  const size_t a_flag = blob.add(g_flags, (size_t)ng);
  const int chunk = (int)cx->opt_bool_chunk;
  const int64_t R = nl;  // one candidate range per slot (driver slots own chunks)
  // temporaries of this call: pooled blocks, back in the pool on return
  DevBuf in, sbb, scb, svb, sqb, qdb, chb, mob, cnd, scn;
  for (DevBuf *b : {&in, &sbb, &scb, &svb, &sqb, &qdb, &chb, &mob, &cnd, &scn}) b->pool = &cx->pool;
  try {
    const uint8_t *d_in = in.as<uint8_t>(blob.bytes.size());
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st));
    const Batch b{(const int64_t *)(d_in + a_goff), (const int64_t *)(d_in + a_qoff), (const int32_t *)(d_in + a_lref),
                  (const uint8_t *)(d_in + a_flag)};
    int64_t *sbeg = sbb.as<int64_t>((size_t)nl);
    int32_t *scnt = scb.as<int32_t>((size_t)nl);
    uint8_t *svirt = svb.as<uint8_t>((size_t)nl);
    int32_t *sq = sqb.as<int32_t>((size_t)nl);
    int32_t *qdrv = qdb.as<int32_t>((size_t)nq);
    int64_t *choff = chb.as<int64_t>((size_t)R + 1);
    unsigned long long *d_cands = cnd.as<unsigned long long>(1);
    const int64_t *doff = (const int64_t *)ix->d_off.p;
    const int64_t *voff = ops > 0 ? ix->sv.dev_offsets() : nullptr;
    SME_HIP(hipMemsetAsync(d_cands, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_structq_plan, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, b, nq, nl, doff, voff, chunk,
                       (int)cx->opt_bool_driver, sbeg, scnt, svirt, sq, qdrv, choff, d_cands);
    SME_CHECK_LAUNCH();
    unsigned long long cands = 0;
    const StructOp op{b,
                      sbeg,
                      scnt,
                      svirt,
                      sq,
                      qdrv,
                      (const int32_t *)ix->d_docno_d.p,
                      (const double *)ix->d_w.p,
                      ops > 0 ? ix->sv.dev<DocFreqScores::docno>() : nullptr,
                      ops > 0 ? ix->sv.dev<DocFreqScores::score>() : nullptr};
    const Counted c = count_chunks(op, (int)R, choff, scnt, chunk, mob, scn,
                                   "structured query: 2^31 or more matches in one batch", st, d_cands, &cands);
    bool_tail(cx, op, c, FirstRange{b.goff, b.qoff}, order, m, out, st);
    ix->sq_leaves = (uint64_t)ops;
    out.verified = verified;
    out.cands = (uint64_t)cands;
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the upload may still read `blob`, kernels the temporaries
    throw;
  }
}

}  // namespace sme
