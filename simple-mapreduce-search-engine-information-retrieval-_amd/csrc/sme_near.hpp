// sme_near.hpp -- the host/device parts of proximity queries (sme_near.hip) that
// need no device: the validator of a batch and the plain restatements of one
// record's ordered-window and unordered-window counts (include/sme.h has the
// definitions in full).  Plain C++, so tools/near_check.cc runs it under the host
// sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "sme_phrase.hpp"

namespace sme {
namespace near {

constexpr int kMaxLen = phrase::kMaxLen;  // terms per query
constexpr int kOrdered = 0, kUnordered = 1;  // the kinds

enum {
  N_OK = 0,
  N_OFFSETS = 1,  // offsets not ascending from 0, or not agreeing with the array size
  N_LENGTH = 2,   // more than kMaxLen terms in a query
  N_TERM = 3,     // a term id outside [-1, V)
  N_SLOTS = 4,    // 2^31 or more term slots in the batch
  N_WIDTH = 5,    // a width below 1
  N_KIND = 6,     // a kind other than 0 / 1
};

// Validates nq queries: q_off[nq + 1] into term_ids[nterms], widths[nq], kinds[nq].
// nterms is the size of the array the caller holds; -1 = implied by the offsets.
// The offsets are checked first and as phrase::validate checks them: each is
// compared with the array's size before anything is read through it.  Per query
// then, in this order: its length, its term ids, its width, its kind.
// *bad_query = the query of the first problem (-1: not inside a query).
inline int validate(const int32_t *term_ids, int64_t nterms, const int64_t *q_off, const int32_t *widths,
                    const uint8_t *kinds, int nq, int64_t V, int *bad_query) {
  *bad_query = -1;
  if (nq < 0) return N_OFFSETS;
  if (nq == 0) return N_OK;  // (nothing is read: every array may be absent)
  if (q_off[0] != 0) return N_OFFSETS;
  for (int i = 0; i < nq; i++) {
    if (q_off[i + 1] < q_off[i] || (nterms >= 0 && q_off[i + 1] > nterms)) {
      *bad_query = i;
      return N_OFFSETS;
    }
  }
  if (nterms < 0) nterms = q_off[nq];
  if (q_off[nq] != nterms) return N_OFFSETS;
  if (nterms >= (int64_t(1) << 31)) return N_SLOTS;
  for (int i = 0; i < nq; i++) {
    *bad_query = i;
    if (q_off[i + 1] - q_off[i] > kMaxLen) return N_LENGTH;
    for (int64_t s = q_off[i]; s < q_off[i + 1]; s++)
      if (term_ids[s] < -1 || term_ids[s] >= V) return N_TERM;
    if (widths[i] < 1) return N_WIDTH;
    if (kinds[i] != kOrdered && kinds[i] != kUnordered) return N_KIND;
  }
  *bad_query = -1;
  return N_OK;
}

// The error message of a validate() result other than N_OK into buf, naming the
// query if the problem lies in one; true if the error is a limit (SME_ELIMIT),
// false if the batch is malformed (SME_EINVAL).
inline bool describe(int rc, int bad_query, char *buf, size_t n) {
  char where[32] = "";
  if (bad_query >= 0) snprintf(where, sizeof where, "query %d: ", bad_query);
  switch (rc) {
    case N_OFFSETS:
      snprintf(buf, n, "proximity query: %soffsets not ascending from 0", where);
      return false;
    case N_LENGTH:
      snprintf(buf, n, "proximity query: %smore than %d terms", where, kMaxLen);
      return true;
    case N_SLOTS:
      snprintf(buf, n, "proximity query: 2^31 or more term slots in the batch");
      return true;
    case N_WIDTH:
      snprintf(buf, n, "proximity query: %sa width below 1", where);
      return false;
    case N_KIND:
      snprintf(buf, n, "proximity query: %sa kind other than 0 (ordered) / 1 (unordered)", where);
      return false;
    default:
      snprintf(buf, n, "proximity query: %sa term id outside [-1, V)", where);
      return false;
  }
}

// Ordered window (#od:N) over one record's stream ts[0 .. len): with R_0[p] iff
// ts[p] == q[0], and R_j[p] iff ts[p] == q[j] and R_{j-1}[s] for some s in
// [p - N, p - 1], the number of p with R_{L-1}[p].  L <= 0 counts nothing.
// O(L len min(N, len)) time, 2 len bytes: a definition, not the device's tile scan.
inline int64_t count_ordered(const int32_t *ts, int64_t len, const int32_t *q, int L, int32_t N) {
  if (L <= 0 || len <= 0 || N < 1) return 0;
  bool *prev = new bool[len], *cur = new bool[len];
  for (int64_t p = 0; p < len; p++) prev[p] = ts[p] == q[0];
  for (int j = 1; j < L; j++) {
    for (int64_t p = 0; p < len; p++) {
      cur[p] = false;
      if (ts[p] != q[j]) continue;
      for (int64_t s = p - 1; s >= 0 && p - s <= N && !cur[p]; s--) cur[p] = prev[s];
    }
    bool *t = prev;
    prev = cur;
    cur = t;
  }
  int64_t c = 0;
  for (int64_t p = 0; p < len; p++) c += prev[p];
  delete[] prev;
  delete[] cur;
  return c;
}

// Unordered window (#uw:N): with T the set of q's distinct terms, the number of
// positions e with ts[e] in T and every term of T in ts[max(0, e - N + 1) .. e].
inline int64_t count_unordered(const int32_t *ts, int64_t len, const int32_t *q, int L, int32_t N) {
  if (L <= 0 || N < 1) return 0;
  int64_t c = 0;
  for (int64_t e = 0; e < len; e++) {
    bool in = false;
    for (int j = 0; j < L && !in; j++) in = ts[e] == q[j];
    if (!in) continue;
    const int64_t lo = e - N + 1 > 0 ? e - N + 1 : 0;
    bool all = true;
    for (int j = 0; j < L && all; j++) {
      bool seen = false;
      for (int64_t s = lo; s <= e && !seen; s++) seen = ts[s] == q[j];
      all = seen;
    }
    c += all;
  }
  return c;
}

}  // namespace near
}  // namespace sme
