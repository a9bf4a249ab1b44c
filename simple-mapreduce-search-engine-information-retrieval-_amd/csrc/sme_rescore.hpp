// sme_rescore.hpp -- the host parts of scoring given documents (sme_rescore.hip,
// sme_query_rescore) that need no device: the limits, the values of its option and
// of its arguments, the rule that picks a slot's form, and the validator of a
// batch's two offset arrays, its term ids and its host candidate lists.  Plain C++,
// so tools/rescore_check.cc runs it under the host sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SME_RESCORE_HD __host__ __device__ __forceinline__
#else
#define SME_RESCORE_HD inline
#endif

namespace sme {
namespace rescore {

constexpr int kTile = 1024;      // candidates per workgroup
constexpr int kMaxSlots = 1024;  // term slots per query
constexpr int64_t kMaxBatch = (int64_t(1) << 31) - 1;  // candidates, and slots, of one batch

enum { MODEL_TFIDF = 0, MODEL_BM25 = 1 };
enum { PATH_AUTO = 0, PATH_SEARCH = 1, PATH_SCAN = 2 };  // option "rescore_path"
inline bool legal_path(int64_t v) { return v >= PATH_AUTO && v <= PATH_SCAN; }
inline bool legal_model(int v) { return v == MODEL_TFIDF || v == MODEL_BM25; }

// floor(log2(x)) + 1 for x >= 1: the steps of a binary search over x entries
SME_RESCORE_HD int search_steps(int64_t x) {
  int s = 0;
  while (x > 0) {
    s++;
    x >>= 1;
  }
  return s;
}
// The automatic rule, for one slot of one tile: `range` postings of the term lie in
// the tile's docno range, the tile holds `cands` candidates, and kLanes threads
// share the work in rounds.  A round of the scan costs one coalesced global load
// and search_steps(cands) LDS reads; a round of the search search_steps(range)
// dependent global loads.  A global load counts as kGlobalPerLds LDS reads: 8, the
// value of the first derivation (an L2 hit of some hundreds of cycles against an LDS
// read of some tens).  Measured at c2 (profiles/rescore_c2.json) the rule
// with 8 is within the run-to-run spread of the faster forced path on one batch and
// faster than both on the other; no other value was tried, so 8 is confirmed, not tuned.
constexpr int kLanes = 256;
constexpr int kGlobalPerLds = 8;
SME_RESCORE_HD bool scan_is_cheaper(int64_t range, int64_t cands) {
  const int64_t scan_rounds = (range + kLanes - 1) / kLanes, search_rounds = (cands + kLanes - 1) / kLanes;
  return scan_rounds * (kGlobalPerLds + search_steps(cands)) <= search_rounds * search_steps(range) * kGlobalPerLds;
}

enum {
  R_OK = 0,
  R_QOFFSETS = 1,  // q_offsets not ascending from 0, or not agreeing with the array size
  R_DOFFSETS = 2,  // d_offsets not ascending from 0, or not agreeing with the array size
  R_SLOTS = 3,     // more than kMaxSlots term slots in a query
  R_BATCH = 4,     // 2^31 or more candidates, or slots, in the batch
  R_TERM = 5,      // a term id outside [-1, V)
  R_ORDER = 6,     // a query's candidates not strictly ascending (signed int32)
};

// Validates nq queries: q_off[nq + 1] into term_ids[nterms], d_off[nq + 1] into
// docnos[ndocs].  nterms / ndocs are the sizes of the arrays the caller holds; -1 =
// implied by the offsets (q_off[nq], d_off[nq]), as a C-ABI caller passes them.
// docnos == nullptr: the candidates are not read (a device array: a kernel checks
// their order).  Nothing is trusted: an offset is compared with the array's size
// before anything is read through it, so a batch cut short anywhere is R_QOFFSETS /
// R_DOFFSETS and nothing past an array is read.
// *bad_query = the query of the first problem (-1: not inside a query).
inline int validate(const int32_t *term_ids, int64_t nterms, const int64_t *q_off, const int32_t *docnos,
                    int64_t ndocs, const int64_t *d_off, int nq, int64_t V, int *bad_query) {
  *bad_query = -1;
  if (nq < 0) return R_QOFFSETS;
  if (nq == 0) return R_OK;  // (no offset is read: both arrays may be absent)
  if (q_off[0] != 0) return R_QOFFSETS;
  for (int q = 0; q < nq; q++)
    if (q_off[q + 1] < q_off[q] || (nterms >= 0 && q_off[q + 1] > nterms)) {
      *bad_query = q;
      return R_QOFFSETS;
    }
  if (nterms < 0) nterms = q_off[nq];
  if (q_off[nq] != nterms) return R_QOFFSETS;
  if (d_off[0] != 0) return R_DOFFSETS;
  for (int q = 0; q < nq; q++)
    if (d_off[q + 1] < d_off[q] || (ndocs >= 0 && d_off[q + 1] > ndocs)) {
      *bad_query = q;
      return R_DOFFSETS;
    }
  if (ndocs < 0) ndocs = d_off[nq];
  if (d_off[nq] != ndocs) return R_DOFFSETS;
  if (nterms > kMaxBatch || ndocs > kMaxBatch) return R_BATCH;
  for (int q = 0; q < nq; q++) {
    *bad_query = q;
    if (q_off[q + 1] - q_off[q] > kMaxSlots) return R_SLOTS;
    for (int64_t s = q_off[q]; s < q_off[q + 1]; s++)
      if (term_ids[s] < -1 || term_ids[s] >= V) return R_TERM;
    if (docnos)
      for (int64_t i = d_off[q] + 1; i < d_off[q + 1]; i++)
        if (docnos[i - 1] >= docnos[i]) return R_ORDER;
  }
  *bad_query = -1;
  return R_OK;
}

}  // namespace rescore
}  // namespace sme
