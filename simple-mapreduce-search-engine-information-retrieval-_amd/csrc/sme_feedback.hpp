// sme_feedback.hpp -- the parts of relevance feedback (sme_feedback.hip) that need
// no device: the limits, the validator of a batch of document sets with its
// messages, and the plain restatement of one set's aggregation.  Plain C++, so
// tools/feedback_check.cc runs it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <set>
#include <vector>

namespace sme {
namespace feedback {

constexpr int kMaxEntries = 1024;              // docno entries per set
constexpr int kMinSlots = 16, kMaxSlots = 4096;  // "fb_slots": entries of the on-chip table, a power of two
constexpr int kSlotBytes = 12;                 // term | freq | document tag and count

// The on-chip table's load limit: a set with more distinct terms takes the large path.
constexpr int load_limit(int slots) { return slots - slots / 4; }
constexpr bool legal_slots(int64_t v) { return v >= kMinSlots && v <= kMaxSlots && (v & (v - 1)) == 0; }

enum {
  F_OK = 0,
  F_OFFSETS = 1,    // set offsets not ascending from 0, or not agreeing with the array size
  F_ENTRIES = 2,    // more than kMaxEntries entries in a set
  F_SLOTS = 3,      // 2^31 or more entries in the batch
  F_XOFFSETS = 4,   // exclusion offsets not ascending from 0, or not agreeing with the array size
  F_XTERM = 5,      // an exclusion id outside [-1, V)
  F_XPOINTERS = 6,  // one of x_ids / x_offsets without the other
};

// Validates n sets: f_off[n + 1] into a docno array of ndocnos entries, and the
// optional exclusion lists x_off[n + 1] into x_ids[nx] (both NULL: none).  ndocnos /
// nx are the sizes of the arrays the caller holds; -1 = implied by the offsets, as
// a C-ABI caller passes them.  The docnos themselves are not read (the device
// entry's are device memory, and every int32 is a docno some index may carry).  An
// offset is compared with the array's size before anything is read through it.
// *bad_set = the set of the first problem (-1: not inside a set).
inline int validate(const int64_t *f_off, int64_t ndocnos, int n, const int32_t *x_ids, int64_t nx,
                    const int64_t *x_off, int64_t V, int *bad_set) {
  *bad_set = -1;
  if (n < 0) return F_OFFSETS;
  if (n == 0) return F_OK;  // (no offset is read: the arrays may be absent)
  if (f_off[0] != 0) return F_OFFSETS;
  for (int i = 0; i < n; i++)
    if (f_off[i + 1] < f_off[i] || (ndocnos >= 0 && f_off[i + 1] > ndocnos)) {
      *bad_set = i;
      return F_OFFSETS;
    }
  if (ndocnos >= 0 && f_off[n] != ndocnos) return F_OFFSETS;
  for (int i = 0; i < n; i++)
    if (f_off[i + 1] - f_off[i] > kMaxEntries) {
      *bad_set = i;
      return F_ENTRIES;
    }
  if (f_off[n] >= (int64_t(1) << 31)) return F_SLOTS;
  if (!x_off && !x_ids) return F_OK;
  if (!x_off) return F_XPOINTERS;
  if (x_off[0] != 0) return F_XOFFSETS;
  for (int i = 0; i < n; i++)
    if (x_off[i + 1] < x_off[i] || (nx >= 0 && x_off[i + 1] > nx)) {
      *bad_set = i;
      return F_XOFFSETS;
    }
  if (nx >= 0 && x_off[n] != nx) return F_XOFFSETS;
  if (x_off[n] > 0 && !x_ids) return F_XPOINTERS;
  for (int i = 0; i < n; i++)
    for (int64_t s = x_off[i]; s < x_off[i + 1]; s++)
      if (x_ids[s] < -1 || x_ids[s] >= V) {
        *bad_set = i;
        return F_XTERM;
      }
  return F_OK;
}

// The error message of a validate() result other than F_OK into buf, naming the
// set if the problem lies in one; true if the error is a limit (SME_ELIMIT), false
// if the batch is malformed (SME_EINVAL).
inline bool describe(int rc, int bad_set, char *buf, size_t n) {
  char where[32] = "";
  if (bad_set >= 0) snprintf(where, sizeof where, "set %d: ", bad_set);
  switch (rc) {
    case F_OFFSETS:
      snprintf(buf, n, "feedback terms: %sset offsets not ascending from 0", where);
      return false;
    case F_ENTRIES:
      snprintf(buf, n, "feedback terms: %smore than %d entries", where, kMaxEntries);
      return true;
    case F_SLOTS:
      snprintf(buf, n, "feedback terms: 2^31 or more entries in the batch");
      return true;
    case F_XOFFSETS:
      snprintf(buf, n, "feedback terms: %sexclusion offsets not ascending from 0", where);
      return false;
    case F_XPOINTERS:
      snprintf(buf, n, "feedback terms: exclusion ids and exclusion offsets go together");
      return false;
    default:
      snprintf(buf, n, "feedback terms: %san exclusion id outside [-1, V)", where);
      return false;
  }
}

struct TermCount {
  int32_t term, freq, docs;
  bool operator==(const TermCount &o) const { return term == o.term && freq == o.freq && docs == o.docs; }
};

// One set's aggregation, plainly: docnos[0 .. n) over the stream records ps_off[nR
// + 1] / ps_terms / ps_docno[nR] (docno ascending).  -1 entries and later
// duplicates are dropped; every record of a remaining docno counts.  -> per term of
// those records, ascending, its occurrences (freq) and the distinct docnos holding
// it (docs).  *positions = stream positions read, *missing = remaining docnos that
// no record carries.
inline std::vector<TermCount> aggregate_set(const int32_t *docnos, int n, const int64_t *ps_off,
                                            const int32_t *ps_terms, const int32_t *ps_docno, int64_t nR,
                                            int64_t *positions, int64_t *missing) {
  std::map<int32_t, TermCount> acc;
  std::set<int32_t> seen;
  *positions = *missing = 0;
  for (int j = 0; j < n; j++) {
    const int32_t d = docnos[j];
    if (d == -1 || !seen.insert(d).second) continue;
    const int64_t r0 = std::lower_bound(ps_docno, ps_docno + nR, d) - ps_docno;
    const int64_t r1 = std::upper_bound(ps_docno + r0, ps_docno + nR, d) - ps_docno;
    if (r0 == r1) {
      ++*missing;
      continue;
    }
    std::set<int32_t> here;
    for (int64_t p = ps_off[r0]; p < ps_off[r1]; p++) {
      TermCount &c = acc.emplace(ps_terms[p], TermCount{ps_terms[p], 0, 0}).first->second;
      c.freq++;
      c.docs += here.insert(ps_terms[p]).second;
    }
    *positions += ps_off[r1] - ps_off[r0];
  }
  std::vector<TermCount> out;
  for (const auto &kv : acc) out.push_back(kv.second);
  return out;
}

}  // namespace feedback
}  // namespace sme
