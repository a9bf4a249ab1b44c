// wild_check -- host check of csrc/sme_wild.hpp, the wildcard parser, trigram keys
// and matcher the expansion kernels (csrc/sme_wild.hip) call.  Built with the
// address and undefined-behaviour sanitizers (make -C <package> wild-check): a read
// past a pattern or a term stops the program -- every buffer handed to the header
// is an exactly sized heap copy.
//
//   wild_check                               built-in cases; prints "all passed"
//   wild_check [--hex] --match PATTERN --terms FILE
//                                            indices of the matching lines of FILE, one
//                                            per line; a line of FILE is a term as hex
//                                            UTF-16 units, 4 digits each (empty = "")
//   wild_check [--hex] --grams PATTERN       the pattern's trigram keys, hex, one per line
//   wild_check [--hex] --term-grams TERM     the term's trigram keys
// PATTERN / TERM are UTF-8 arguments; with --hex PATTERN is the hex of its UTF-8
// bytes and TERM the hex of its UTF-16 units (so U+0000, unpaired surrogates and
// malformed UTF-8 can be sent).  Exit 3: malformed UTF-8, 4: more than 255 units.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "sme_wild.hpp"

using namespace sme::wild;
typedef std::vector<uint16_t> Units;

static int g_fail = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      g_fail++;                                               \
    }                                                         \
  } while (0)

struct Pattern {
  int rc = W_OK;
  Units units;
  std::vector<uint8_t> mask;
};

// parse through exactly sized heap buffers
static Pattern parse(const std::string &utf8) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[utf8.size()]);
  memcpy(in.get(), utf8.data(), utf8.size());
  std::unique_ptr<uint16_t[]> u(new uint16_t[kMaxUnits]);
  std::unique_ptr<uint8_t[]> m(new uint8_t[kMaxUnits]);
  Pattern p;
  int np = 0;
  p.rc = parse_pattern(in.get(), (int64_t)utf8.size(), u.get(), m.get(), &np);
  if (p.rc == W_OK) {
    p.units.assign(u.get(), u.get() + np);
    p.mask.assign(m.get(), m.get() + np);
  }
  return p;
}

static std::vector<uint64_t> grams_of(const Pattern &p) {
  const int np = (int)p.units.size();
  std::unique_ptr<uint16_t[]> u(new uint16_t[np]);
  std::unique_ptr<uint8_t[]> m(new uint8_t[np]);
  std::copy(p.units.begin(), p.units.end(), u.get());
  std::copy(p.mask.begin(), p.mask.end(), m.get());
  std::unique_ptr<uint64_t[]> k(new uint64_t[kMaxUnits]);
  const int g = pattern_grams(u.get(), m.get(), np, k.get());
  return std::vector<uint64_t>(k.get(), k.get() + g);
}

static std::vector<uint64_t> term_grams_of(const Units &t) {
  std::unique_ptr<uint16_t[]> u(new uint16_t[t.size()]);
  std::copy(t.begin(), t.end(), u.get());
  std::vector<uint64_t> out;
  for (size_t i = 0; i < t.size(); i++) out.push_back(term_gram(u.get(), (int64_t)t.size(), (int64_t)i));
  return out;
}

static bool match(const Pattern &p, const Units &t) {
  const int np = (int)p.units.size();
  std::unique_ptr<uint16_t[]> u(new uint16_t[np]), tt(new uint16_t[t.size()]);
  std::unique_ptr<uint8_t[]> m(new uint8_t[np]);
  std::copy(p.units.begin(), p.units.end(), u.get());
  std::copy(p.mask.begin(), p.mask.end(), m.get());
  std::copy(t.begin(), t.end(), tt.get());
  return wild_match(u.get(), m.get(), np, tt.get(), (int)t.size());
}

static Units ascii(const std::string &s) { return Units(s.begin(), s.end()); }
static bool m8(const std::string &pat, const std::string &term) {
  Pattern p = parse(pat), t = parse(term);  // the term through the decoder too (mask ignored)
  return p.rc == W_OK && t.rc == W_OK && match(p, t.units);
}
static uint64_t key(int a, int b, int c) {  // -1 = boundary
  uint64_t k = (uint64_t)(uint16_t)b << 16;
  k |= a < 0 ? kStartFlag : (uint64_t)a << 32;
  k |= c < 0 ? kEndFlag : (uint64_t)c;
  return k;
}

static void builtin() {
  // ---- parser
  Pattern p = parse("a*b?");
  CHECK(p.rc == W_OK && p.units == ascii("a*b?"));
  CHECK(p.mask == (std::vector<uint8_t>{M_LIT, M_STAR, M_LIT, M_ONE}));
  p = parse("");
  CHECK(p.rc == W_OK && p.units.empty());
  p = parse("caf\xC3\xA9");
  CHECK(p.rc == W_OK && p.units == (Units{'c', 'a', 'f', 0xE9}));
  p = parse("\xE2\x82\xAC");
  CHECK(p.rc == W_OK && p.units == (Units{0x20AC}));
  p = parse("\xF0\x9F\x98\x80");  // U+1F600 -> surrogate pair
  CHECK(p.rc == W_OK && p.units == (Units{0xD83D, 0xDE00}));
  p = parse("\xED\xA0\xBD");  // a 3-byte surrogate: taken as that unit
  CHECK(p.rc == W_OK && p.units == (Units{0xD83D}));
  p = parse(std::string("a\0b", 3));
  CHECK(p.rc == W_OK && p.units == (Units{'a', 0, 'b'}));
  for (const char *bad : {"\x80", "a\xBF", "\xC3", "\xC3\x28", "\xE2\x82", "\xE2\x28\xA1", "\xF0\x9F\x98", "\xF8\x88\x80\x80\x80",
                          "\xFF", "\xC0\x80", "\xC1\xBF", "\xE0\x80\x80", "\xF0\x80\x80\x80", "\xF4\x90\x80\x80"})
    CHECK(parse(bad).rc == W_MALFORMED);
  CHECK(parse(std::string(255, 'a')).rc == W_OK);
  CHECK(parse(std::string(256, 'a')).rc == W_TOO_LONG);
  CHECK(parse(std::string(255, '*')).units.size() == 255);
  {
    std::string s(254, 'a');  // 254 units + a surrogate pair = 256
    CHECK(parse(s + "\xF0\x9F\x98\x80").rc == W_TOO_LONG);
    s.pop_back();
    CHECK(parse(s + "\xF0\x9F\x98\x80").rc == W_OK);
  }
  // ---- term trigrams
  CHECK(term_grams_of(ascii("")).empty());
  CHECK(term_grams_of(ascii("a")) == (std::vector<uint64_t>{key(-1, 'a', -1)}));
  CHECK(term_grams_of(ascii("ab")) == (std::vector<uint64_t>{key(-1, 'a', 'b'), key('a', 'b', -1)}));
  CHECK(term_grams_of(ascii("abc")) ==
        (std::vector<uint64_t>{key(-1, 'a', 'b'), key('a', 'b', 'c'), key('b', 'c', -1)}));
  // no content aliases a boundary
  for (uint64_t k : term_grams_of(ascii("$ab$"))) CHECK(k != key(-1, 'a', 'b') && k != key('a', 'b', -1));
  CHECK(key('$', 'a', 'b') != key(-1, 'a', 'b') && key(0, 'a', 'b') != key(-1, 'a', 'b'));
  CHECK(key('a', 'b', 0) != key('a', 'b', -1) && key('a', 'b', 0xFFFF) != key('a', 'b', -1));
  CHECK(key(0xFFFF, 0xFFFF, 0xFFFF) < kStartFlag);
  CHECK((key(-1, 0xFFFF, -1) >> kKeyBits) == 0);
  // ---- pattern trigrams
  CHECK(grams_of(parse("abc")) == term_grams_of(ascii("abc")));
  CHECK(grams_of(parse("a")) == term_grams_of(ascii("a")));
  CHECK(grams_of(parse("")).empty());
  CHECK(grams_of(parse("abc*")) == (std::vector<uint64_t>{key(-1, 'a', 'b'), key('a', 'b', 'c')}));
  CHECK(grams_of(parse("*ing")) == (std::vector<uint64_t>{key('i', 'n', 'g'), key('n', 'g', -1)}));
  CHECK(grams_of(parse("*ab*")).empty());
  CHECK(grams_of(parse("*abc*")) == (std::vector<uint64_t>{key('a', 'b', 'c')}));
  CHECK(grams_of(parse("a*b*c")).empty());
  CHECK(grams_of(parse("ab*c*de")) == (std::vector<uint64_t>{key(-1, 'a', 'b'), key('d', 'e', -1)}));
  CHECK(grams_of(parse("a?c")).empty());
  CHECK(grams_of(parse("ab?cd")) == (std::vector<uint64_t>{key(-1, 'a', 'b'), key('c', 'd', -1)}));
  CHECK(grams_of(parse("*")).empty() && grams_of(parse("?")).empty() && grams_of(parse("?b")).empty());
  CHECK(grams_of(parse("?bc")) == (std::vector<uint64_t>{key('b', 'c', -1)}));
  CHECK(grams_of(parse(std::string(255, 'a'))).size() == 255);
  // every trigram of a pattern is one of every term it matches
  for (const char *pat : {"ab*", "*ab", "a*bcd*e", "??abc", "abc??", "aaaa", "*aaa*"})
    for (const char *term : {"ab", "abab", "abcde", "xbcde", "zzabc", "abczz", "aaaa", "aaaaa", "xaaay"}) {
      if (!m8(pat, term)) continue;
      const std::vector<uint64_t> tg = term_grams_of(ascii(term));
      for (uint64_t k : grams_of(parse(pat))) CHECK(std::find(tg.begin(), tg.end(), k) != tg.end());
    }
  // ---- matcher
  CHECK(m8("", "") && !m8("", "a") && m8("*", "") && m8("*", "abc") && m8("**", "") && m8("**", "x"));
  CHECK(!m8("?", "") && m8("?", "a") && !m8("?", "ab") && m8("??", "ab") && !m8("??", "a"));
  CHECK(m8("?*", "a") && !m8("?*", "") && m8("*?", "abc") && !m8("*?", ""));
  CHECK(m8("abc", "abc") && !m8("abc", "abcd") && !m8("abc", "ab") && !m8("abc", "xabc"));
  CHECK(m8("abc*", "abc") && m8("abc*", "abcdef") && !m8("abc*", "ab") && !m8("abc*", "xabc"));
  CHECK(m8("*ing", "ing") && m8("*ing", "running") && !m8("*ing", "ringo"));
  CHECK(m8("*ab*", "ab") && m8("*ab*", "cabd") && !m8("*ab*", "a") && !m8("*ab*", "ba"));
  CHECK(m8("a*b*c", "abc") && m8("a*b*c", "axxbyyc") && !m8("a*b*c", "acb") && m8("a*b*c", "abcbc"));
  CHECK(m8("a?c", "abc") && !m8("a?c", "ac") && !m8("a?c", "abbc"));
  CHECK(m8("???*???", "abcdef") && m8("???*???", "abcdefg") && !m8("???*???", "abcde"));
  CHECK(m8("*a", "aaa") && m8("a*a", "aa") && !m8("a*a", "a"));
  {
    const std::string as(60, 'a');
    CHECK(!m8("a*a*a*a*b", as) && m8("a*a*a*a*b", as + "b") && m8("a*a*a*a*a", as) && m8("*a*a*a*", as));
    CHECK(!m8(std::string(61, 'a'), as) && m8(std::string(60, '?'), as) && !m8(std::string(61, '?'), as));
  }
  // '?' is one UTF-16 unit: a supplementary character needs two
  CHECK(!m8("?", "\xF0\x9F\x98\x80") && m8("??", "\xF0\x9F\x98\x80") && m8("*", "\xF0\x9F\x98\x80"));
  CHECK(m8("caf?", "caf\xC3\xA9") && m8("stra?e", "stra\xC3\x9F" "e") && !m8("cafe", "caf\xC3\xA9"));
  // terms may hold the metacharacters (a loaded index): they are plain units there
  {
    Pattern q = parse("a*");
    CHECK(match(q, ascii("a*")) && match(q, ascii("a?b")));
    q = parse("a?");
    CHECK(match(q, ascii("a*")) && match(q, ascii("a?")) && !match(q, ascii("a")));
    q = parse("ab");
    CHECK(!match(q, ascii("ab$")) && !match(q, ascii("$ab")) && !match(q, Units{0, 'a', 'b'}) &&
          !match(q, Units{'a', 'b', 0xFFFF}) && match(q, ascii("ab")));
  }
}

static bool unhex(const std::string &h, std::string &out) {
  if (h.size() % 2) return false;
  out.clear();
  for (size_t i = 0; i < h.size(); i += 2) {
    char *end = nullptr;
    const std::string b = h.substr(i, 2);
    const long v = strtol(b.c_str(), &end, 16);
    if (*end) return false;
    out.push_back((char)v);
  }
  return true;
}
static bool unhex_units(const std::string &h, Units &out) {
  std::string bytes;
  if (!unhex(h, bytes) || bytes.size() % 2) return false;
  out.clear();
  for (size_t i = 0; i < bytes.size(); i += 2) out.push_back((uint16_t)(((uint8_t)bytes[i] << 8) | (uint8_t)bytes[i + 1]));
  return true;
}
static int parse_exit(int rc) {
  if (rc == W_MALFORMED) {
    printf("malformed UTF-8\n");
    return 3;
  }
  printf("more than %d units\n", kMaxUnits);
  return 4;
}

int main(int argc, char **argv) {
  bool hex = false;
  std::string mode, arg, terms;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--hex") {
      hex = true;
    } else if ((a == "--match" || a == "--grams" || a == "--term-grams") && i + 1 < argc) {
      mode = a;
      arg = argv[++i];
    } else if (a == "--terms" && i + 1 < argc) {
      terms = argv[++i];
    } else {
      fprintf(stderr, "usage: wild_check [--hex] [--match PATTERN --terms FILE | --grams PATTERN | --term-grams TERM]\n");
      return 2;
    }
  }
  if (mode.empty()) {
    builtin();
    if (g_fail) {
      printf("%d checks failed\n", g_fail);
      return 1;
    }
    printf("all passed\n");
    return 0;
  }
  if (mode == "--term-grams") {
    Units t;
    if (hex) {
      if (!unhex_units(arg, t)) return 2;
    } else {
      const Pattern p = parse(arg);
      if (p.rc != W_OK) return parse_exit(p.rc);
      t = p.units;
    }
    for (uint64_t k : term_grams_of(t)) printf("%llx\n", (unsigned long long)k);
    return 0;
  }
  std::string utf8 = arg;
  if (hex && !unhex(arg, utf8)) return 2;
  const Pattern p = parse(utf8);
  if (p.rc != W_OK) return parse_exit(p.rc);
  if (mode == "--grams") {
    for (uint64_t k : grams_of(p)) printf("%llx\n", (unsigned long long)k);
    return 0;
  }
  std::ifstream f(terms);
  if (!f) {
    fprintf(stderr, "cannot read %s\n", terms.c_str());
    return 2;
  }
  std::string line;
  for (long i = 0; std::getline(f, line); i++) {
    Units t;
    if (!unhex_units(line, t)) {
      fprintf(stderr, "line %ld is not hex UTF-16 units\n", i);
      return 2;
    }
    if (match(p, t)) printf("%ld\n", i);
  }
  return 0;
}
