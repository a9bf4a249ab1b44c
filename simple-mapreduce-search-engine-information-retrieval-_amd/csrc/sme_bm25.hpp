// sme_bm25.hpp -- the host/device parts of BM25 ranking (sme_bm25.hip) that need
// no device: the limits, the batch validator, and the weight, the norm and the
// window bound as the very functions the kernels call.  Plain C++, so
// tools/bm25_check.cc runs it under the host sanitizers and prints the functions'
// bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SME_BM25_HD __host__ __device__ __forceinline__
#else
#define SME_BM25_HD inline
#endif

namespace sme {
namespace bm25 {

constexpr int kMaxK = 1024;      // results per query
constexpr int kMaxSlots = 1024;  // term slots per query
constexpr int kWindow = 1024;    // documents per scorer window
constexpr int kMaxSplit = 4096;  // workgroups per query ("bm25_split" is capped at it and at the window count)

enum {
  M_OK = 0,
  M_OFFSETS = 1,  // offsets not ascending from 0, or not agreeing with the array size
  M_SLOTS = 2,    // more than kMaxSlots term slots in a query
  M_TERM = 3,     // a term id outside [-1, V)
};

// Validates nq queries: q_off[nq + 1] into term_ids[nterms].  nterms is the size of
// the array the caller holds; -1 = implied by the offsets (q_off[nq]), as a C-ABI
// caller passes it.  term_ids == nullptr: the ids are not read (a device array; the
// scorer skips an id outside [0, V) as it skips -1).  Nothing is trusted: an offset
// is compared with the array's size before anything is read through it, so a batch
// cut short anywhere is M_OFFSETS and nothing past an array is read.
// *bad_query = the query of the first problem (-1: not inside a query).
inline int validate(const int32_t *term_ids, int64_t nterms, const int64_t *q_off, int nq, int64_t V, int *bad_query) {
  *bad_query = -1;
  if (nq < 0) return M_OFFSETS;
  if (nq == 0) return M_OK;  // (no offset is read: q_off may be absent)
  if (q_off[0] != 0) return M_OFFSETS;
  for (int q = 0; q < nq; q++)
    if (q_off[q + 1] < q_off[q] || (nterms >= 0 && q_off[q + 1] > nterms)) {
      *bad_query = q;
      return M_OFFSETS;
    }
  if (nterms < 0) nterms = q_off[nq];
  if (q_off[nq] != nterms) return M_OFFSETS;
  for (int q = 0; q < nq; q++) {
    *bad_query = q;
    if (q_off[q + 1] - q_off[q] > kMaxSlots) return M_SLOTS;
    if (term_ids)
      for (int64_t s = q_off[q]; s < q_off[q + 1]; s++)
        if (term_ids[s] < -1 || term_ids[s] >= V) return M_TERM;
  }
  *bad_query = -1;
  return M_OK;
}

// k1 finite and >= 0, b in [0, 1]; NaN fails both
inline bool legal_params(double k1, double b) { return k1 >= 0.0 && k1 <= 1.79769313486231570815e308 && b >= 0.0 && b <= 1.0; }

// idf of a term in df of D documents.  Host only: the platform libm's log is the
// contract (a table by df, gathered on the device).
inline double idf_value(int64_t D, int64_t df) { return log(1.0 + ((double)(D - df) + 0.5) / ((double)df + 0.5)); }

// All of it fp64 in exactly this association (the build has -ffp-contract=off).
SME_BM25_HD double doc_norm(double k1, double b, double dl, double avgdl) { return k1 * ((1.0 - b) + b * (dl / avgdl)); }
SME_BM25_HD double weight(double idf, double tf, double k1, double norm) { return idf * ((tf * (k1 + 1.0)) / (tf + norm)); }
// What a posting of a term adds at most in a window: the weight of the term's
// largest tf in a document as short as the window's shortest.  weight() does not
// fall as tf grows nor rise as dl grows, for k1 >= 0 and b in [0, 1].
SME_BM25_HD double bound_term(double idf, double maxtf, double k1, double b, double mindl, double avgdl) {
  return weight(idf, maxtf, k1, doc_norm(k1, b, mindl, avgdl));
}

// A score as a 64-bit key that ascends with it (for an atomic max of the entry bar);
// 0 is below every score's key.
SME_BM25_HD uint64_t bar_key(double v) {
  union {
    double d;
    uint64_t u;
  } x;
  x.d = v;
  return (x.u >> 63) ? ~x.u : (x.u | 0x8000000000000000ull);
}
SME_BM25_HD double bar_value(uint64_t key) {
  union {
    double d;
    uint64_t u;
  } x;
  x.u = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
  return x.d;
}

}  // namespace bm25
}  // namespace sme
