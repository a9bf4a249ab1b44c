// sme_phrase.hpp -- the host/device parts of phrase queries (sme_phrase.hip) that
// need no device: the limit, the validator of a phrase batch and the plain
// restatement of one record's count.  Plain C++, so tools/phrase_check.cc runs it
// under the host sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define SME_PHRASE_HD __host__ __device__ __forceinline__
#else
#define SME_PHRASE_HD inline
#endif

namespace sme {
namespace phrase {

constexpr int kMaxLen = 32;  // terms per phrase

enum {
  P_OK = 0,
  P_OFFSETS = 1,  // offsets not ascending from 0, or not agreeing with the array size
  P_LENGTH = 2,   // more than kMaxLen terms in a phrase
  P_TERM = 3,     // a term id outside [-1, V)
  P_SLOTS = 4,    // 2^31 or more term slots in the batch
};

// Validates np phrases: p_off[np + 1] into term_ids[nterms].  nterms is the size
// of the array the caller holds; -1 = implied by the offsets (p_off[np]), as a
// C-ABI caller passes it.  An offset is compared with the array's size before
// anything is read through it, so a batch cut short anywhere is P_OFFSETS and
// nothing past an array is read.  *bad_phrase = the phrase of the first problem
// (-1: not inside a phrase).
inline int validate(const int32_t *term_ids, int64_t nterms, const int64_t *p_off, int np, int64_t V,
                    int *bad_phrase) {
  *bad_phrase = -1;
  if (np < 0) return P_OFFSETS;
  if (np == 0) return P_OK;  // (no offset is read: p_off may be absent)
  if (p_off[0] != 0) return P_OFFSETS;
  for (int i = 0; i < np; i++) {
    if (p_off[i + 1] < p_off[i] || (nterms >= 0 && p_off[i + 1] > nterms)) {
      *bad_phrase = i;
      return P_OFFSETS;
    }
  }
  if (nterms < 0) nterms = p_off[np];
  if (p_off[np] != nterms) return P_OFFSETS;
  if (nterms >= (int64_t(1) << 31)) return P_SLOTS;
  for (int i = 0; i < np; i++) {
    *bad_phrase = i;
    if (p_off[i + 1] - p_off[i] > kMaxLen) return P_LENGTH;
    for (int64_t s = p_off[i]; s < p_off[i + 1]; s++)
      if (term_ids[s] < -1 || term_ids[s] >= V) return P_TERM;
  }
  *bad_phrase = -1;
  return P_OK;
}

// The error message of a validate() result other than P_OK into buf, naming the
// phrase if the problem lies in one; true if the error is a limit (SME_ELIMIT),
// false if the batch is malformed (SME_EINVAL).
inline bool describe(int rc, int bad_phrase, char *buf, size_t n) {
  char where[32] = "";
  if (bad_phrase >= 0) snprintf(where, sizeof where, "phrase %d: ", bad_phrase);
  switch (rc) {
    case P_OFFSETS:
      snprintf(buf, n, "phrase query: %soffsets not ascending from 0", where);
      return false;
    case P_LENGTH:
      snprintf(buf, n, "phrase query: %smore than %d terms", where, kMaxLen);
      return true;
    case P_SLOTS:
      snprintf(buf, n, "phrase query: 2^31 or more term slots in the batch");
      return true;
    default:
      snprintf(buf, n, "phrase query: %sa term id outside [-1, V)", where);
      return false;
  }
}

// Occurrences of the phrase ph[0 .. L) in one record's term stream ts[0 .. len):
// the starts s with s + L <= len and ts[s + j] == ph[j] for every j.  Overlapping
// occurrences all count; nothing at or past ts[len] is read; L <= 0 counts nothing.
SME_PHRASE_HD int64_t phrase_count(const int32_t *ts, int64_t len, const int32_t *ph, int L) {
  if (L <= 0) return 0;
  int64_t c = 0;
  for (int64_t s = 0; s + L <= len; s++) {
    int j = 0;
    while (j < L && ts[s + j] == ph[j]) j++;
    c += j == L;
  }
  return c;
}

}  // namespace phrase
}  // namespace sme
