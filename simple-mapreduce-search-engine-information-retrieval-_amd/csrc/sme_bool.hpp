// sme_bool.hpp -- the host/device parts of Boolean retrieval (sme_bool.hip) that
// need no device: the limits, the validator of the three-level query structure
// (queries -> groups -> term slots) and the sort key of a score.  Plain C++, so
// tools/bool_check.cc runs it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SME_BOOL_HD __host__ __device__ __forceinline__
#else
#define SME_BOOL_HD inline
#endif

namespace sme {
namespace boolq {

constexpr int kMaxGroups = 64;   // groups per query
constexpr int kMaxSlots = 1024;  // term slots per query (all its groups together)

enum {
  B_OK = 0,
  B_OFFSETS = 1,  // offsets not ascending from 0, or not agreeing with the array sizes
  B_FLAG = 2,     // a group flag other than 0 (required) / 1 (excluded)
  B_GROUPS = 3,   // more than kMaxGroups groups in a query
  B_SLOTS = 4,    // more than kMaxSlots term slots in a query
  B_TERM = 5,     // a term id outside [-1, V)
};

// Validates nq queries: q_off[nq + 1] into the groups, g_off[ngroups + 1] into
// term_ids[nterms], g_flags[ngroups].  ngroups / nterms are the sizes of the
// arrays the caller holds; -1 = implied by the offsets (q_off[nq], g_off[ngroups]),
// as a C-ABI caller passes them.  Nothing is trusted: an offset is compared with
// the size of the array it indexes before anything is read through it, so a
// structure cut short anywhere is B_OFFSETS and nothing past an array is read.
// *bad_query = the query of the first problem (-1: not inside a query).
inline int validate(const int32_t *term_ids, int64_t nterms, const int64_t *g_off, int64_t ngroups,
                    const uint8_t *g_flags, const int64_t *q_off, int nq, int64_t V, int *bad_query) {
  *bad_query = -1;
  if (nq < 0) return B_OFFSETS;
  if (nq == 0) return B_OK;  // (no offset is read: q_off may be absent)
  if (q_off[0] != 0) return B_OFFSETS;
  for (int q = 0; q < nq; q++) {
    if (q_off[q + 1] < q_off[q]) {
      *bad_query = q;
      return B_OFFSETS;
    }
    if (ngroups >= 0 && q_off[q + 1] > ngroups) {
      *bad_query = q;
      return B_OFFSETS;
    }
  }
  if (ngroups < 0) ngroups = q_off[nq];
  if (q_off[nq] != ngroups) return B_OFFSETS;
  // g_off has ngroups + 1 entries, all of them read from here on
  if (g_off[0] != 0) return B_OFFSETS;
  int q = 0;
  for (int64_t g = 0; g < ngroups; g++) {
    while (q_off[q + 1] <= g) q++;  // (q < nq: q_off[nq] = ngroups > g)
    if (g_off[g + 1] < g_off[g] || (nterms >= 0 && g_off[g + 1] > nterms)) {
      *bad_query = q;
      return B_OFFSETS;
    }
  }
  if (nterms < 0) nterms = g_off[ngroups];
  if (g_off[ngroups] != nterms) return B_OFFSETS;
  for (q = 0; q < nq; q++) {
    const int64_t g0 = q_off[q], g1 = q_off[q + 1];
    *bad_query = q;
    if (g1 - g0 > kMaxGroups) return B_GROUPS;
    if (g_off[g1] - g_off[g0] > kMaxSlots) return B_SLOTS;
    for (int64_t g = g0; g < g1; g++)
      if (g_flags[g] > 1) return B_FLAG;
    for (int64_t s = g_off[g0]; s < g_off[g1]; s++)
      if (term_ids[s] < -1 || term_ids[s] >= V) return B_TERM;
  }
  *bad_query = -1;
  return B_OK;
}

// The 64-bit sort key of a score for "score descending": for finite a, b
//   score_key(a) < score_key(b)  <=>  a > b,
// and +0.0 / -0.0, equal as doubles, get one key.  (The IEEE bit pattern orders
// like the value once negative numbers are complemented and the sign bit of the
// others is set; the final complement turns ascending into descending.)
SME_BOOL_HD uint64_t score_key(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  if (b == 0x8000000000000000ull) b = 0;  // -0.0 as +0.0
  const uint64_t asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  return ~asc;
}
// docno ascending in signed int32 order as an unsigned 32-bit key
SME_BOOL_HD uint32_t docno_key(int32_t d) { return (uint32_t)d ^ 0x80000000u; }

}  // namespace boolq
}  // namespace sme
