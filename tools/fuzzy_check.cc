// fuzzy_check -- host check of csrc/sme_fuzzy.hpp, the word parser, distinct trigram
// keys and bit-parallel edit distance the suggestion kernels (csrc/sme_fuzzy.hip)
// call.  Built with the address and undefined-behaviour sanitizers (make -C
// <package> fuzzy-check): a read past a word or a term stops the program -- every
// buffer handed to the header is an exactly sized heap copy.
//
//   fuzzy_check                              built-in cases; prints "all passed"
//   fuzzy_check [--hex] --dist WORD --terms FILE
//                                            the word's distance to every line of FILE,
//                                            one per line; a line of FILE is a term as hex
//                                            UTF-16 units, 4 digits each (empty = "")
//   fuzzy_check [--hex] --keys WORD          the word's distinct keys, hex, ascending
// WORD is a UTF-8 argument; with --hex it is the hex of its UTF-8 bytes (so U+0000,
// unpaired surrogates and malformed UTF-8 can be sent).  Exit 3: malformed UTF-8,
// 4: more than 64 units.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "sme_fuzzy.hpp"

using namespace sme::fuzzy;
typedef std::vector<uint16_t> Units;

static int g_fail = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      g_fail++;                                               \
    }                                                         \
  } while (0)

struct Word {
  int rc = F_OK;
  Units units;
};

// parse through exactly sized heap buffers
static Word parse(const std::string &utf8) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[utf8.size()]);
  memcpy(in.get(), utf8.data(), utf8.size());
  std::unique_ptr<uint16_t[]> u(new uint16_t[sme::wild::kMaxUnits]);
  std::unique_ptr<uint8_t[]> m(new uint8_t[sme::wild::kMaxUnits]);
  Word w;
  int nu = 0;
  w.rc = parse_word(in.get(), (int64_t)utf8.size(), u.get(), m.get(), &nu);
  if (w.rc == F_OK) w.units.assign(u.get(), u.get() + nu);
  return w;
}

static std::vector<uint64_t> keys_of(const Units &w) {
  std::unique_ptr<uint16_t[]> u(new uint16_t[w.size()]);
  std::copy(w.begin(), w.end(), u.get());
  std::unique_ptr<uint64_t[]> k(new uint64_t[w.size()]);
  const int n = distinct_keys(u.get(), (int)w.size(), k.get());
  return std::vector<uint64_t>(k.get(), k.get() + n);
}

static int dist(const Units &w, const Units &t) {
  std::unique_ptr<uint16_t[]> a(new uint16_t[w.size()]), b(new uint16_t[t.size()]);
  std::copy(w.begin(), w.end(), a.get());
  std::copy(t.begin(), t.end(), b.get());
  return edit_distance(a.get(), (int)w.size(), b.get(), (int)t.size());
}

// the kernels' form: Peq in exactly sized arrays, the direct table beside it, a limit
static int dist_limit(const Units &w, const Units &t, int limit, bool direct) {
  const int Lw = (int)w.size();
  std::unique_ptr<uint16_t[]> a(new uint16_t[Lw]), b(new uint16_t[t.size()]), su(new uint16_t[Lw]);
  std::unique_ptr<uint64_t[]> pm(new uint64_t[Lw]), dt(new uint64_t[128]);
  std::copy(w.begin(), w.end(), a.get());
  std::copy(t.begin(), t.end(), b.get());
  const int nd = peq_build(a.get(), Lw, su.get(), pm.get());
  for (int i = 0; i < 128; i++) dt[i] = peq_find(su.get(), pm.get(), nd, (uint16_t)i);
  return distance_peq(su.get(), pm.get(), nd, direct ? dt.get() : nullptr, Lw, b.get(), (int)t.size(), limit);
}

// the plain dynamic program, two rows
static int dp(const Units &a, const Units &b) {
  std::vector<int> prev(b.size() + 1), cur(b.size() + 1);
  for (size_t j = 0; j <= b.size(); j++) prev[j] = (int)j;
  for (size_t i = 1; i <= a.size(); i++) {
    cur[0] = (int)i;
    for (size_t j = 1; j <= b.size(); j++)
      cur[j] = std::min(std::min(prev[j] + 1, cur[j - 1] + 1), prev[j - 1] + (a[i - 1] != b[j - 1]));
    prev.swap(cur);
  }
  return prev[b.size()];
}

static Units ascii(const std::string &s) { return Units(s.begin(), s.end()); }
static Units u8(const std::string &s) { return parse(s).units; }
static uint64_t key(int a, int b, int c) {  // -1 = boundary
  uint64_t k = (uint64_t)(uint16_t)b << 16;
  k |= a < 0 ? sme::wild::kStartFlag : (uint64_t)a << 32;
  k |= c < 0 ? sme::wild::kEndFlag : (uint64_t)c;
  return k;
}
// every form of the distance against the dynamic program
static void same(const Units &w, const Units &t) {
  const int want = dp(w, t);
  CHECK(dist(w, t) == want);
  if (w.empty()) return;
  for (bool direct : {false, true}) {
    CHECK(dist_limit(w, t, 1000, direct) == want);
    for (int limit = 0; limit <= 3; limit++) {
      const int got = dist_limit(w, t, limit, direct);
      CHECK(want <= limit ? got == want : got > limit);
    }
  }
}

static void builtin() {
  // ---- parser: the wildcard decoder, no metacharacters, 64 units
  Word w = parse("a*b?");
  CHECK(w.rc == F_OK && w.units == ascii("a*b?"));
  w = parse("");
  CHECK(w.rc == F_OK && w.units.empty());
  w = parse("caf\xC3\xA9");
  CHECK(w.rc == F_OK && w.units == (Units{'c', 'a', 'f', 0xE9}));
  w = parse("\xF0\x9F\x98\x80");  // U+1F600 -> surrogate pair
  CHECK(w.rc == F_OK && w.units == (Units{0xD83D, 0xDE00}));
  w = parse("\xED\xA0\xBD");  // a 3-byte surrogate: taken as that unit
  CHECK(w.rc == F_OK && w.units == (Units{0xD83D}));
  w = parse(std::string("a\0b", 3));
  CHECK(w.rc == F_OK && w.units == (Units{'a', 0, 'b'}));
  for (const char *bad : {"\x80", "a\xBF", "\xC3", "\xC3\x28", "\xE2\x82", "\xF0\x9F\x98", "\xF8\x88\x80\x80\x80", "\xFF",
                          "\xC0\x80", "\xE0\x80\x80", "\xF4\x90\x80\x80"})
    CHECK(parse(bad).rc == F_MALFORMED);
  CHECK(parse(std::string(64, 'a')).rc == F_OK && parse(std::string(64, 'a')).units.size() == 64);
  CHECK(parse(std::string(65, 'a')).rc == F_TOO_LONG);
  CHECK(parse(std::string(255, 'a')).rc == F_TOO_LONG && parse(std::string(256, 'a')).rc == F_TOO_LONG);
  CHECK(parse(std::string(5000, 'a')).rc == F_TOO_LONG);
  {
    std::string s(63, 'a');  // 63 units + a surrogate pair = 65
    CHECK(parse(s + "\xF0\x9F\x98\x80").rc == F_TOO_LONG);
    s.pop_back();
    CHECK(parse(s + "\xF0\x9F\x98\x80").rc == F_OK);
  }
  CHECK(parse(std::string(65, 'a') + "\xFF").rc == F_MALFORMED);  // malformed wins wherever it stands below 255 units
  // ---- distinct keys: a term's windows, each once, ascending
  CHECK(keys_of(ascii("")).empty());
  CHECK(keys_of(ascii("a")) == (std::vector<uint64_t>{key(-1, 'a', -1)}));
  {
    std::vector<uint64_t> want{key(-1, 'a', 'b'), key('a', 'b', 'c'), key('b', 'c', -1)};
    std::sort(want.begin(), want.end());
    CHECK(keys_of(ascii("abc")) == want);
  }
  CHECK(keys_of(ascii("aaaa")).size() == 3);      // START a a | a a a (twice) | a a END
  CHECK(keys_of(ascii("abababab")).size() == 4);  // START a b | b a b | a b a | a b END
  CHECK(keys_of(Units(64, 'a')).size() == 3);
  for (const char *s : {"apple", "running", "aaaa", "ababab", "$ab$", "a*c", "a?c"}) {
    const Units u = ascii(s);
    std::set<uint64_t> want;
    for (size_t i = 0; i < u.size(); i++) want.insert(sme::wild::term_gram(u.data(), (int64_t)u.size(), (int64_t)i));
    CHECK(keys_of(u) == std::vector<uint64_t>(want.begin(), want.end()));
  }
  for (uint64_t k : keys_of(ascii("$ab$"))) CHECK(k != key(-1, 'a', 'b') && k != key('a', 'b', -1));
  CHECK(lists_for(0) == 1 && lists_for(2) == 7 && lists_for(kMaxDist) == kMaxLists);
  // the filter's bound: a term within distance d misses at most 3d distinct keys of the word
  for (const char *a : {"apple", "running", "aaaa", "ababab", "abcdefgh", "a", "ab"})
    for (const char *b : {"apple", "aple", "appple", "applf", "bpple", "pple", "apples", "runing", "aaa", "aaaaa",
                          "abab", "abababab", "abcdxfgh", "xbcdefgy", "b", "", "ba"}) {
      const std::vector<uint64_t> ka = keys_of(ascii(a)), kb = keys_of(ascii(b));
      int missing = 0;
      for (uint64_t k : ka) missing += std::find(kb.begin(), kb.end(), k) == kb.end();
      CHECK(missing <= 3 * dp(ascii(a), ascii(b)));
    }
  // ---- Peq
  {
    const Units u = ascii("banana");
    std::unique_ptr<uint16_t[]> a(new uint16_t[6]), su(new uint16_t[6]);
    std::unique_ptr<uint64_t[]> pm(new uint64_t[6]);
    std::copy(u.begin(), u.end(), a.get());
    CHECK(peq_build(a.get(), 6, su.get(), pm.get()) == 3);
    CHECK(su[0] == 'a' && su[1] == 'b' && su[2] == 'n');
    CHECK(pm[0] == 0x2A && pm[1] == 0x01 && pm[2] == 0x14);
    CHECK(peq_find(su.get(), pm.get(), 3, 'n') == 0x14 && peq_find(su.get(), pm.get(), 3, 'c') == 0 &&
          peq_find(su.get(), pm.get(), 3, 0xFFFF) == 0 && peq_find(su.get(), pm.get(), 3, 0) == 0);
  }
  // ---- distance: every edit kind at the first, middle and last unit
  for (const char *s : {"apple", "running", "a", "ab", "abcdefghijklmnopqrstuvwxyz"}) {
    const Units t = ascii(s);
    const size_t n = t.size();
    same(t, t);
    for (size_t p : {size_t(0), n / 2, n - 1}) {
      Units sub = t, ins = t, del = t;
      sub[p] = 'Q';
      ins.insert(ins.begin() + (long)p, 'Q');
      del.erase(del.begin() + (long)p);
      CHECK(dist(sub, t) == 1 && dist(ins, t) == 1 && dist(del, t) == 1);
      CHECK(dist(t, sub) == 1 && dist(t, ins) == 1 && dist(t, del) == 1);
      for (const Units &x : {sub, ins, del}) {
        same(x, t);
        same(t, x);
      }
    }
    Units app = t;
    app.push_back('Q');
    CHECK(dist(app, t) == 1 && dist(t, app) == 1);
    same(app, t);
  }
  CHECK(dist(ascii("apply"), ascii("apple")) == 1 && dist(ascii("appel"), ascii("apple")) == 2);  // no transposition
  CHECK(dist(ascii("kitten"), ascii("sitting")) == 3 && dist(ascii("flaw"), ascii("lawn")) == 2);
  // the empty word and the empty term
  CHECK(dist(ascii(""), ascii("")) == 0 && dist(ascii(""), ascii("abc")) == 3 && dist(ascii("abc"), ascii("")) == 3);
  same(ascii(""), ascii("abc"));
  same(ascii("abc"), ascii(""));
  // 64-unit words: the top bit of the vectors
  {
    const Units a64(64, 'a'), a60(60, 'a'), a61(61, 'a'), a63(63, 'a');
    Units mix(64, 'a'), alt;
    mix[0] = 'b';
    mix[63] = 'c';
    mix[31] = 'd';
    for (int i = 0; i < 64; i++) alt.push_back(i % 2 ? 'a' : 'b');
    CHECK(dist(a64, a64) == 0 && dist(a64, a60) == 4 && dist(a61, a60) == 1 && dist(a64, a63) == 1);
    CHECK(dist(mix, a64) == 3 && dist(a64, mix) == 3 && dist(alt, a64) == 32);
    Units t65(65, 'a'), t70 = alt;
    t70.insert(t70.end(), 6, 'z');
    for (const Units &x : {a64, mix, alt})
      for (const Units &y : {a64, a60, a63, mix, alt, t65, t70, Units(), Units(120, 'a')}) same(x, y);
    Units distinct;  // 64 distinct units, some past the direct table
    for (int i = 0; i < 64; i++) distinct.push_back((uint16_t)(100 + 7 * i));
    Units rev(distinct.rbegin(), distinct.rend());
    same(distinct, distinct);
    same(distinct, rev);
    same(distinct, a60);
  }
  // supplementary pairs are two units
  {
    const Units smile = u8("\xF0\x9F\x98\x80"), grin = u8("\xF0\x9F\x98\x81"), word = u8("\xF0\x9F\x98\x80smile");
    CHECK(smile.size() == 2 && dist(smile, grin) == 1 && dist(smile, Units()) == 2 && dist(smile, word) == 5);
    CHECK(dist(Units{0xD83D}, smile) == 1 && dist(u8("x\xF0\x9F\x98\x80"), smile) == 1);
    same(word, smile);
    same(u8("\xF0\x9F\x98\x80smil"), word);
  }
  // repeated units
  for (const char *a : {"aaaa", "abababab", "aabbaabb", "banana", "mississippi"})
    for (const char *b : {"aaa", "aaaaa", "abab", "babababa", "aabbaab", "bananas", "ananas", "misisipi", ""}) {
      same(ascii(a), ascii(b));
      same(ascii(b), ascii(a));
    }
  // literal metacharacters and boundary look-alikes are plain units
  CHECK(dist(ascii("a*c"), ascii("abc")) == 1 && dist(ascii("a?c"), ascii("ac")) == 1 && dist(ascii("*"), ascii("abc")) == 3);
  CHECK(dist(ascii("ab"), ascii("$ab")) == 1 && dist(ascii("ab"), Units{0, 'a', 'b'}) == 1 &&
        dist(ascii("ab"), Units{'a', 'b', 0xFFFF}) == 1);
  // a seeded sweep over a small alphabet against the dynamic program
  {
    uint32_t s = 12345;
    auto rnd = [&](uint32_t n) {
      s = s * 1664525u + 1013904223u;
      return (s >> 8) % n;
    };
    for (int it = 0; it < 400; it++) {
      Units a(rnd(65)), b(rnd(70));
      const uint32_t alpha = 1 + rnd(4);
      for (auto &x : a) x = (uint16_t)('a' + rnd(alpha));
      for (auto &x : b) x = (uint16_t)('a' + rnd(alpha));
      same(a, b);
    }
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

int main(int argc, char **argv) {
  bool hex = false;
  std::string mode, arg, terms;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--hex") {
      hex = true;
    } else if ((a == "--dist" || a == "--keys") && i + 1 < argc) {
      mode = a;
      arg = argv[++i];
    } else if (a == "--terms" && i + 1 < argc) {
      terms = argv[++i];
    } else {
      fprintf(stderr, "usage: fuzzy_check [--hex] [--dist WORD --terms FILE | --keys WORD]\n");
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
  std::string utf8 = arg;
  if (hex && !unhex(arg, utf8)) return 2;
  const Word w = parse(utf8);
  if (w.rc == F_MALFORMED) {
    printf("malformed UTF-8\n");
    return 3;
  }
  if (w.rc == F_TOO_LONG) {
    printf("more than %d units\n", kMaxUnits);
    return 4;
  }
  if (mode == "--keys") {
    for (uint64_t k : keys_of(w.units)) printf("%llx\n", (unsigned long long)k);
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
    printf("%d\n", dist(w.units, t));
  }
  return 0;
}
