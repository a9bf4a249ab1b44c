// sme_structq.hpp -- the host part of structured queries (sme_structq.hip) that
// needs no device: the limits, the validator of the four-level structure (queries
// -> groups -> leaves -> term ids) and its messages.  Plain C++, so
// tools/structq_check.cc runs it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "sme_bool.hpp"
#include "sme_phrase.hpp"

namespace sme {
namespace structq {

constexpr int kMaxGroups = boolq::kMaxGroups;  // groups per query
constexpr int kMaxLeaves = boolq::kMaxSlots;   // leaves per query (all its groups together)
constexpr int kMaxLen = phrase::kMaxLen;       // term ids per operator leaf
constexpr int kTerm = 0, kOrdered = 1, kUnordered = 2;  // the leaf kinds

enum {
  S_OK = 0,
  S_OFFSETS = 1,   // offsets not ascending from 0, or not agreeing with the level above / the array sizes
  S_FLAG = 2,      // a group flag other than 0 (required) / 1 (excluded)
  S_GROUPS = 3,    // more than kMaxGroups groups in a query
  S_LEAVES = 4,    // more than kMaxLeaves leaves in a query
  S_TERM = 5,      // a term id outside [-1, V)
  S_KIND = 6,      // a leaf kind outside 0 .. 2
  S_TERMLEAF = 7,  // a term leaf with other than one id
  S_LENGTH = 8,    // more than kMaxLen ids in an operator leaf
  S_WIDTH = 9,     // an operator width below 1
  S_SLOTS = 10,    // 2^31 or more ids or leaves in the batch
};

// Validates nq queries: q_off[nq + 1] into the groups, g_off[ngroups + 1] into the
// leaves, l_off[nleaves + 1] into term_ids[nterms]; g_flags[ngroups],
// l_kinds[nleaves], l_widths[nleaves].  ngroups / nleaves / nterms are the sizes of
// the arrays the caller holds; -1 = implied by the offsets, as a C-ABI caller
// passes them.  Nothing is trusted: every level's offsets are compared with the
// size of the array they index before anything is read through them, so a
// structure cut short anywhere is S_OFFSETS and nothing past an array is read.
// Per query then, in this order: its groups, its leaves, its flags; per leaf its
// kind, its length, its width (operators), its ids.
// *bad_query = the query of the first problem (-1: not inside a query);
// *operators = the operator leaves of a valid batch.
inline int validate(const int32_t *term_ids, int64_t nterms, const int64_t *l_off, int64_t nleaves,
                    const uint8_t *l_kinds, const int32_t *l_widths, const int64_t *g_off, int64_t ngroups,
                    const uint8_t *g_flags, const int64_t *q_off, int nq, int64_t V, int *bad_query,
                    int64_t *operators) {
  *bad_query = -1;
  *operators = 0;
  if (nq < 0) return S_OFFSETS;
  if (nq == 0) return S_OK;  // (no offset is read: every array may be absent)
  if (q_off[0] != 0) return S_OFFSETS;
  for (int q = 0; q < nq; q++) {
    if (q_off[q + 1] < q_off[q] || (ngroups >= 0 && q_off[q + 1] > ngroups)) {
      *bad_query = q;
      return S_OFFSETS;
    }
  }
  if (ngroups < 0) ngroups = q_off[nq];
  if (q_off[nq] != ngroups) return S_OFFSETS;
  // g_off has ngroups + 1 entries, all of them read from here on
  if (g_off[0] != 0) return S_OFFSETS;
  int q = 0;
  for (int64_t g = 0; g < ngroups; g++) {
    while (q_off[q + 1] <= g) q++;  // (q < nq: q_off[nq] = ngroups > g)
    if (g_off[g + 1] < g_off[g] || (nleaves >= 0 && g_off[g + 1] > nleaves)) {
      *bad_query = q;
      return S_OFFSETS;
    }
  }
  if (nleaves < 0) nleaves = g_off[ngroups];
  if (g_off[ngroups] != nleaves) return S_OFFSETS;
  // l_off has nleaves + 1 entries, all of them read from here on
  if (l_off[0] != 0) return S_OFFSETS;
  q = 0;
  for (int64_t l = 0; l < nleaves; l++) {
    while (g_off[q_off[q + 1]] <= l) q++;  // (q < nq: g_off[q_off[nq]] = nleaves > l)
    if (l_off[l + 1] < l_off[l] || (nterms >= 0 && l_off[l + 1] > nterms)) {
      *bad_query = q;
      return S_OFFSETS;
    }
  }
  if (nterms < 0) nterms = l_off[nleaves];
  if (l_off[nleaves] != nterms) return S_OFFSETS;
  if (nleaves >= (int64_t(1) << 31) || nterms >= (int64_t(1) << 31)) return S_SLOTS;
  int64_t ops = 0;
  for (q = 0; q < nq; q++) {
    const int64_t g0 = q_off[q], g1 = q_off[q + 1];
    *bad_query = q;
    if (g1 - g0 > kMaxGroups) return S_GROUPS;
    if (g_off[g1] - g_off[g0] > kMaxLeaves) return S_LEAVES;
    for (int64_t g = g0; g < g1; g++)
      if (g_flags[g] > 1) return S_FLAG;
    for (int64_t l = g_off[g0]; l < g_off[g1]; l++) {
      const int64_t n = l_off[l + 1] - l_off[l];
      if (l_kinds[l] > kUnordered) return S_KIND;
      if (l_kinds[l] == kTerm) {
        if (n != 1) return S_TERMLEAF;
      } else {
        if (n > kMaxLen) return S_LENGTH;
        if (l_widths[l] < 1) return S_WIDTH;
        ops++;
      }
      for (int64_t s = l_off[l]; s < l_off[l + 1]; s++)
        if (term_ids[s] < -1 || term_ids[s] >= V) return S_TERM;
    }
  }
  *bad_query = -1;
  *operators = ops;
  return S_OK;
}

// The error message of a validate() result other than S_OK into buf, naming the
// query if the problem lies in one; true if the error is a limit (SME_ELIMIT),
// false if the batch is malformed (SME_EINVAL).
inline bool describe(int rc, int bad_query, char *buf, size_t n) {
  char where[32] = "";
  if (bad_query >= 0) snprintf(where, sizeof where, "query %d: ", bad_query);
  switch (rc) {
    case S_OFFSETS:
      snprintf(buf, n, "structured query: %soffsets not ascending from 0 or inconsistent", where);
      return false;
    case S_FLAG:
      snprintf(buf, n, "structured query: %sa group flag other than 0 (required) or 1 (excluded)", where);
      return false;
    case S_GROUPS:
      snprintf(buf, n, "structured query: %smore than %d groups", where, kMaxGroups);
      return true;
    case S_LEAVES:
      snprintf(buf, n, "structured query: %smore than %d leaves", where, kMaxLeaves);
      return true;
    case S_KIND:
      snprintf(buf, n, "structured query: %sa leaf kind other than 0 (term), 1 (ordered) or 2 (unordered)", where);
      return false;
    case S_TERMLEAF:
      snprintf(buf, n, "structured query: %sa term leaf with other than one id", where);
      return false;
    case S_LENGTH:
      snprintf(buf, n, "structured query: %smore than %d ids in an operator leaf", where, kMaxLen);
      return true;
    case S_WIDTH:
      snprintf(buf, n, "structured query: %san operator width below 1", where);
      return false;
    case S_SLOTS:
      snprintf(buf, n, "structured query: 2^31 or more ids or leaves in the batch");
      return true;
    default:
      snprintf(buf, n, "structured query: %sa term id outside [-1, V)", where);
      return false;
  }
}

}  // namespace structq
}  // namespace sme
