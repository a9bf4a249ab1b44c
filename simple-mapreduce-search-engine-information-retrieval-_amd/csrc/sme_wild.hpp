// sme_wild.hpp -- wildcard patterns over term strings: the pattern parser, the
// character-trigram keys of terms and patterns, and the matcher, shared by the
// device code (sme_wild.hip) and the stand-alone host check (tools/wild_check.cc).
// No HIP header is needed: a host compiler sees plain inline functions.
//
//   term     L UTF-16 units (d_term_off / d_term_chars, String.compareTo order)
//   pattern  UTF-8 on the way in; '*' = any run of units (none included), '?' =
//            exactly one unit (a supplementary character needs "??"), every other
//            unit matches itself.  No escape syntax, no case folding.
//   trigram  three consecutive entries of  START t[0] .. t[L-1] END  (L windows; a
//            term of 0 units has none).  A pattern's windows lie inside one maximal
//            literal run each; START joins the first run when the pattern begins
//            with a literal, END the last run when it ends with one.
//   key      bits 32..47 first unit, 16..31 middle unit, 0..15 last unit, bit 48 =
//            the first entry is START, bit 49 = the last entry is END; a boundary's
//            unit field is 0.  The flags lie outside the 48 unit bits, so no term
//            content ('$', U+0000, U+FFFF ...) can alias a boundary.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SME_WILD_HD __host__ __device__ __forceinline__
#else
#define SME_WILD_HD inline
#endif

namespace sme {
namespace wild {

enum {
  W_OK = 0,
  W_MALFORMED = 1,  // not UTF-8 (see parse_pattern)
  W_TOO_LONG = 2,   // more than kMaxUnits units
};
enum : uint8_t { M_LIT = 0, M_STAR = 1, M_ONE = 2 };  // mask values

constexpr int kMaxUnits = 255;  // longest pattern, in UTF-16 units
constexpr int kKeyBits = 50;    // 48 unit bits + 2 boundary flags
constexpr uint64_t kStartFlag = uint64_t(1) << 48;
constexpr uint64_t kEndFlag = uint64_t(1) << 49;

// UTF-8 -> UTF-16 units + metacharacter mask.  The decoder maps as the one behind
// sme_lookup_terms does (1..4 byte forms; code points from U+10000 become a
// surrogate pair; a 3-byte form of a surrogate is taken as that unit, so a
// term holding an unpaired surrogate can be named), but refuses what that one
// lets through: a continuation byte where a sequence starts, a lead byte F8..FF,
// a missing or non-continuation trailing byte, an overlong form, a code point
// past U+10FFFF.  units / mask: kMaxUnits entries.
SME_WILD_HD int parse_pattern(const uint8_t *p, int64_t n, uint16_t *units, uint8_t *mask, int *np) {
  int64_t i = 0;
  int o = 0;
  while (i < n) {
    const unsigned c = p[i];
    unsigned cp, lo;
    int extra;
    if (c < 0x80) {
      cp = c, extra = 0, lo = 0;
    } else if (c < 0xC0) {
      return W_MALFORMED;
    } else if (c < 0xE0) {
      cp = c & 0x1F, extra = 1, lo = 0x80;
    } else if (c < 0xF0) {
      cp = c & 0x0F, extra = 2, lo = 0x800;
    } else if (c < 0xF8) {
      cp = c & 0x07, extra = 3, lo = 0x10000;
    } else {
      return W_MALFORMED;
    }
    if (i + 1 + extra > n) return W_MALFORMED;
    for (int k = 1; k <= extra; k++) {
      const unsigned d = p[i + k];
      if ((d & 0xC0) != 0x80) return W_MALFORMED;
      cp = (cp << 6) | (d & 0x3F);
    }
    i += 1 + extra;
    if (cp < lo || cp > 0x10FFFF) return W_MALFORMED;
    if (cp >= 0x10000) {
      if (o + 2 > kMaxUnits) return W_TOO_LONG;
      cp -= 0x10000;
      units[o] = (uint16_t)(0xD800 + (cp >> 10));
      mask[o++] = M_LIT;
      units[o] = (uint16_t)(0xDC00 + (cp & 0x3FF));
      mask[o++] = M_LIT;
    } else {
      if (o + 1 > kMaxUnits) return W_TOO_LONG;
      units[o] = (uint16_t)cp;
      mask[o++] = cp == '*' ? M_STAR : cp == '?' ? M_ONE : M_LIT;
    }
  }
  *np = o;
  return W_OK;
}

// Key of the window whose middle entry is u[i] (0 <= i < n), over
// START u[0] .. u[n-1] END.
SME_WILD_HD uint64_t window_key(const uint16_t *u, int64_t n, int64_t i) {
  uint64_t k = (uint64_t)u[i] << 16;
  k |= i == 0 ? kStartFlag : (uint64_t)u[i - 1] << 32;
  k |= i == n - 1 ? kEndFlag : (uint64_t)u[i + 1];
  return k;
}

// A term's windows: window i (0 <= i < L) has t[i] in the middle.
SME_WILD_HD uint64_t term_gram(const uint16_t *t, int64_t L, int64_t i) { return window_key(t, L, i); }

// A pattern's windows, in pattern order (repeats kept); keys: kMaxUnits entries
// (a run of len units with s + e boundaries has max(0, len + s + e - 2) windows,
// and only a pattern of one run has both, so the count is at most np).
SME_WILD_HD int pattern_grams(const uint16_t *u, const uint8_t *mask, int np, uint64_t *keys) {
  int g = 0;
  int a = 0;
  while (a < np) {
    if (mask[a] != M_LIT) {
      a++;
      continue;
    }
    int b = a;
    while (b < np && mask[b] == M_LIT) b++;
    // middles of the windows inside [a, b): the first needs a predecessor (START
    // when a == 0), the last a successor (END when b == np)
    const int first = a == 0 ? a : a + 1, last = b == np ? b - 1 : b - 2;
    for (int i = first; i <= last; i++) {
      uint64_t k = (uint64_t)u[i] << 16;
      k |= i == 0 ? kStartFlag : (uint64_t)u[i - 1] << 32;
      k |= i == np - 1 ? kEndFlag : (uint64_t)u[i + 1];
      keys[g++] = k;
    }
    a = b;
  }
  return g;
}

// Does the pattern match the whole term?  Greedy star with one saved backtrack
// point (the last '*' and the term position it was tried at): no recursion and
// no per-thread array; worst case O(np * nt).
SME_WILD_HD bool wild_match(const uint16_t *pu, const uint8_t *pm, int np, const uint16_t *t, int nt) {
  int p = 0, x = 0, star = -1, mark = 0;
  while (x < nt) {
    if (p < np && pm[p] == M_STAR) {
      star = p++;
      mark = x;
    } else if (p < np && (pm[p] == M_ONE || pu[p] == t[x])) {
      p++;
      x++;
    } else if (star >= 0) {
      p = star + 1;
      x = ++mark;
    } else {
      return false;
    }
  }
  while (p < np && pm[p] == M_STAR) p++;
  return p == np;
}

}  // namespace wild
}  // namespace sme
