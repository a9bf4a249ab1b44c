// sme_fuzzy.hpp -- spelling suggestions over term strings: the word parser, the
// word's distinct trigram keys (the candidate filter over the wildcard table of
// sme_wild.hpp) and the bit-parallel edit-distance verifier, shared by the device
// code (sme_fuzzy.hip) and the stand-alone host check (tools/fuzzy_check.cc).
// No HIP header is needed: a host compiler sees plain inline functions.
//
//   word      UTF-8 on the way in, decoded by wild::parse_pattern (same refusals);
//             no unit is a metacharacter ('*' and '?' are ordinary units), no case
//             folding; at most kMaxUnits UTF-16 units.
//   distance  Levenshtein over UTF-16 units: insert, delete, substitute one unit at
//             cost 1 each, no transposition (a supplementary character is two units).
//   keys      the word's windows taken as a term's (wild::term_gram: Lw windows,
//             both boundaries), deduplicated: Dw distinct keys.
//
// Why the filter is sound.  Fix an optimal alignment of the word and a term with at
// most d edits.  A substitution or a deletion at a unit touches the at most 3
// windows of the word that hold that unit; an insertion between two neighbouring
// entries touches the at most 2 windows that hold both; START and END are never
// edited.  A window no edit touches has its three entries matched to three
// neighbouring entries of the term, so it appears verbatim, boundary flags
// included, among the term's windows.  Distinct keys sit at distinct window
// positions, so at most 3d DISTINCT keys of the word are absent from the term --
// also with the table's (key, term) pairs deduplicated ("aaaa", "ababab").  Hence
// a term within distance d holds at least one of ANY 3d + 1 distinct keys of the
// word: the candidates are the union of the posting lists of 3d + 1 distinct keys
// (the shortest ones; an absent key is an empty list), and a word with fewer than
// 3d + 1 distinct keys takes the whole vocabulary.  Every candidate is verified, so
// the candidate source never changes a result.
#pragma once
#include <stdint.h>

#include "sme_wild.hpp"

namespace sme {
namespace fuzzy {

enum {
  F_OK = 0,
  F_MALFORMED = 1,  // not UTF-8 (wild::parse_pattern)
  F_TOO_LONG = 2,   // more than kMaxUnits units
};

constexpr int kMaxUnits = 64;  // longest word: the pattern of one 64-bit word
constexpr int kMaxDist = 3;    // largest max_dist
constexpr int kMaxLists = 3 * kMaxDist + 1;

// posting lists a word needs at distance d
SME_WILD_HD int lists_for(int d) { return 3 * d + 1; }

// UTF-8 -> UTF-16 units.  units / scratch: wild::kMaxUnits entries each (the
// decoder's own limit; scratch takes its metacharacter mask, which is ignored).
SME_WILD_HD int parse_word(const uint8_t *p, int64_t n, uint16_t *units, uint8_t *scratch, int *nu) {
  int np = 0;
  const int rc = wild::parse_pattern(p, n, units, scratch, &np);
  if (rc == wild::W_MALFORMED) return F_MALFORMED;
  if (rc == wild::W_TOO_LONG || np > kMaxUnits) return F_TOO_LONG;
  *nu = np;
  return F_OK;
}

// The word's distinct window keys, ascending; keys: Lw entries.  Returns Dw.
SME_WILD_HD int distinct_keys(const uint16_t *w, int Lw, uint64_t *keys) {
  int n = 0;
  for (int i = 0; i < Lw; i++) {
    const uint64_t k = wild::term_gram(w, Lw, i);
    int at = n;  // insertion into the sorted prefix, repeats dropped
    while (at > 0 && keys[at - 1] > k) at--;
    if (at > 0 && keys[at - 1] == k) continue;
    for (int j = n; j > at; j--) keys[j] = keys[j - 1];
    keys[at] = k;
    n++;
  }
  return n;
}

// Peq of a word: its distinct units ascending in su[0 .. nd) and, beside each, the
// mask of the word positions holding it (bit i = w[i]).  su / pm: Lw entries.
SME_WILD_HD int peq_build(const uint16_t *w, int Lw, uint16_t *su, uint64_t *pm) {
  int nd = 0;
  for (int i = 0; i < Lw; i++) {
    const uint16_t u = w[i];
    int at = nd;
    while (at > 0 && su[at - 1] > u) at--;
    if (at > 0 && su[at - 1] == u) {
      pm[at - 1] |= uint64_t(1) << i;
      continue;
    }
    for (int j = nd; j > at; j--) {
      su[j] = su[j - 1];
      pm[j] = pm[j - 1];
    }
    su[at] = u;
    pm[at] = uint64_t(1) << i;
    nd++;
  }
  return nd;
}

SME_WILD_HD uint64_t peq_find(const uint16_t *su, const uint64_t *pm, int nd, uint16_t u) {
  int lo = 0, hi = nd;  // first unit >= u
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (su[m] < u)
      lo = m + 1;
    else
      hi = m;
  }
  return lo < nd && su[lo] == u ? pm[lo] : 0;
}

// One column of the global (Needleman-Wunsch) form of Myers' bit-vector algorithm
// as Hyyro states it: eq = Peq of the term's unit, (pv, mv) the vertical +1 / -1
// deltas of the column, score the cell of the word's last unit (bit `top`).  The
// horizontal delta entering row 0 is +1 per column (D[0][j] = j): that is the
// `| 1` below, and what tells this from the substring-search variant.
SME_WILD_HD void myers_step(uint64_t eq, uint64_t top, uint64_t &pv, uint64_t &mv, int &score) {
  const uint64_t xv = eq | mv;
  const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
  uint64_t ph = mv | ~(xh | pv);
  uint64_t mh = pv & xh;
  score += (ph & top) ? 1 : 0;
  score -= (mh & top) ? 1 : 0;
  ph = (ph << 1) | 1;
  mh <<= 1;
  pv = mh | ~(xv | ph);
  mv = ph & xv;
}

// Distance of the word behind (su, pm, nd, Lw), 1 <= Lw <= 64, to the term: one
// step per unit of the term, no array of its own.  `direct` (may be null): 128
// masks indexed by the unit, for units below 128.  The cell of the last row moves
// by at most 1 per column, so once score - (units left) passes `limit` the result
// cannot come back under it: the loop stops and the value returned is some
// number > limit (limit >= Lw + Lt: always the exact distance).
SME_WILD_HD int distance_peq(const uint16_t *su, const uint64_t *pm, int nd, const uint64_t *direct, int Lw,
                             const uint16_t *t, int Lt, int limit) {
  const uint64_t top = uint64_t(1) << (Lw - 1);
  uint64_t pv = ~uint64_t(0), mv = 0;
  int score = Lw;
  for (int j = 0; j < Lt; j++) {
    if (score - (Lt - j) > limit) return score - (Lt - j);
    const uint16_t c = t[j];
    const uint64_t eq = (direct && c < 128) ? direct[c] : peq_find(su, pm, nd, c);
    myers_step(eq, top, pv, mv, score);
  }
  return score;
}

// Host-side form (it keeps the word's Peq in local arrays, which device code must
// not: the kernels stage Peq in LDS and call distance_peq).
inline int edit_distance(const uint16_t *w, int Lw, const uint16_t *t, int Lt) {
  if (Lw == 0) return Lt;
  uint16_t su[kMaxUnits];
  uint64_t pm[kMaxUnits];
  const int nd = peq_build(w, Lw, su, pm);
  return distance_peq(su, pm, nd, nullptr, Lw, t, Lt, Lw + Lt);
}

}  // namespace fuzzy
}  // namespace sme
