// phrase_check -- host check of csrc/sme_phrase.hpp, the validator of a phrase batch
// with its messages and the one-record phrase count that csrc/sme_phrase.hip
// restates on the device.  Built with the address and undefined-behaviour
// sanitizers (make -C <package> phrase-check): a read past an array stops the
// program -- every array handed to the header is an exactly sized heap copy.
//
//   phrase_check                          built-in cases; prints "all passed"
//   phrase_check --count PHRASE STREAM    the count of the phrase in the stream, each
//                                         a comma-separated list of ids ("" = empty)
//   phrase_check --validate V OFFS TERMS  "<rc> <limit 0/1> <phrase> <message>" for
//                                         the batch (comma-separated lists)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "sme_phrase.hpp"

using namespace sme::phrase;

static int g_fail = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                             \
    }                                                       \
  } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
  return p;
}

static int64_t count(const std::vector<int32_t> &ts, const std::vector<int32_t> &ph) {
  auto t = exact(ts), p = exact(ph);
  return phrase_count(t.get(), (int64_t)ts.size(), p.get(), (int)ph.size());
}

struct Res {
  int rc, phrase;
  bool limit;
  std::string msg;
};
// declared: the size of term_ids is given; otherwise left to the offsets
static Res run(const std::vector<int64_t> &off, const std::vector<int32_t> &term, int64_t V, bool declared) {
  auto o = exact(off);
  auto t = exact(term);
  Res r;
  r.rc = validate(t.get(), declared ? (int64_t)term.size() : -1, o.get(), (int)off.size() - 1, V, &r.phrase);
  r.limit = false;
  if (r.rc != P_OK) {
    char buf[128];
    r.limit = describe(r.rc, r.phrase, buf, sizeof buf);
    r.msg = buf;
  }
  return r;
}
static Res run(const std::vector<int64_t> &off, const std::vector<int32_t> &term, int64_t V) {
  const Res a = run(off, term, V, true), b = run(off, term, V, false);
  CHECK(a.rc == b.rc && a.phrase == b.phrase && a.msg == b.msg);
  return a;
}
static bool names(const Res &r, int phrase) {
  return r.msg.find("phrase " + std::to_string(phrase) + ":") != std::string::npos;
}

static void validator_cases() {
  Res r = run({0, 2, 2, 5}, {0, 1, 2, -1, 9}, 10);
  CHECK(r.rc == P_OK && r.phrase == -1);
  // no phrase: nothing is read
  int bad = 7;
  CHECK(validate(nullptr, -1, nullptr, 0, 10, &bad) == P_OK && bad == -1);
  CHECK(validate(nullptr, -1, nullptr, -1, 10, &bad) == P_OFFSETS);
  // only empty phrases, and an empty term array
  r = run({0, 0, 0}, {}, 10);
  CHECK(r.rc == P_OK);
  // a term id of V and one below -1: malformed, the phrase named
  r = run({0, 2, 3}, {0, 1, 10}, 10);
  CHECK(r.rc == P_TERM && r.phrase == 1 && !r.limit && names(r, 1));
  r = run({0, 2, 3}, {0, -2, 3}, 10);
  CHECK(r.rc == P_TERM && r.phrase == 0 && !r.limit && names(r, 0));
  r = run({0, 1}, {0}, 0);  // an index without terms knows none
  CHECK(r.rc == P_TERM && r.phrase == 0);
  r = run({0, 1}, {-1}, 0);
  CHECK(r.rc == P_OK);
  // the length limit: 32 passes, 33 is a limit, the phrase named
  std::vector<int32_t> t32(32, 3), t33(33, 3), t35(35, 3);
  r = run({0, 32}, t32, 10);
  CHECK(r.rc == P_OK);
  r = run({0, 33}, t33, 10);
  CHECK(r.rc == P_LENGTH && r.phrase == 0 && r.limit && names(r, 0));
  r = run({0, 1, 2, 35}, t35, 10);
  CHECK(r.rc == P_LENGTH && r.phrase == 2 && r.limit && names(r, 2));
  // the length is tested before the ids of that phrase
  t33[5] = 99;
  r = run({0, 33}, t33, 10);
  CHECK(r.rc == P_LENGTH);
  // offsets: not from 0, descending, past the declared array, short of it
  r = run({1, 2}, {0, 1}, 10);
  CHECK(r.rc == P_OFFSETS && !r.limit);
  r = run({0, 2, 1}, {0, 1}, 10, true);
  CHECK(r.rc == P_OFFSETS && r.phrase == 1 && names(r, 1));
  r = run({0, 2, 1}, {0, 1}, 10, false);
  CHECK(r.rc == P_OFFSETS && r.phrase == 1);
  r = run({0, 1, 4}, {0, 1}, 10, true);  // (declared only: implied sizes trust the last offset)
  CHECK(r.rc == P_OFFSETS && r.phrase == 1);
  r = run({0, 1}, {0, 1}, 10, true);
  CHECK(r.rc == P_OFFSETS && r.phrase == -1);
  r = run({0, -1}, {}, 10);
  CHECK(r.rc == P_OFFSETS && r.phrase == 0);
  // 2^31 term slots: refused from the offsets alone (no term is read)
  {
    const int64_t off[2] = {0, int64_t(1) << 31};
    CHECK(validate(nullptr, -1, off, 1, 10, &bad) == P_SLOTS);
    char buf[128];
    CHECK(describe(P_SLOTS, -1, buf, sizeof buf));
  }
}

static void count_cases() {
  for (int L : {1, 2, 5, 32}) {
    std::vector<int32_t> ph;
    for (int j = 0; j < L; j++) ph.push_back(100 + j);  // distinct terms: no overlaps
    // len = 0, L - 1, L, L + 1
    CHECK(count({}, ph) == 0);
    CHECK(count(std::vector<int32_t>(ph.begin(), ph.end() - 1), ph) == 0);
    CHECK(count(ph, ph) == 1);
    std::vector<int32_t> a = ph, b = ph;
    a.push_back(7);
    b.insert(b.begin(), 7);
    CHECK(count(a, ph) == 1);  // at the first start
    CHECK(count(b, ph) == 1);  // at the last start
    // first and last start of a longer stream, and a near miss in between
    std::vector<int32_t> s = ph;
    s.insert(s.end(), 40, 7);
    s.insert(s.end(), ph.begin(), ph.end() - 1);
    s.push_back(L == 1 ? 7 : 100 + L - 2);  // the last term wrong (L = 1: no phrase at all)
    s.insert(s.end(), ph.begin(), ph.end());
    CHECK(count(s, ph) == 2);
    // the phrase cut off by the end of the stream
    s.insert(s.end(), ph.begin(), ph.end() - 1);
    CHECK(count(s, ph) == 2);
  }
  // overlaps all count
  CHECK(count({5, 5, 5}, {5, 5}) == 2);
  CHECK(count({5, 5, 5, 5}, {5, 5, 5}) == 2);
  CHECK(count({1, 2, 1, 2, 1}, {1, 2, 1}) == 2);
  CHECK(count(std::vector<int32_t>(40, 9), std::vector<int32_t>(32, 9)) == 9);
  CHECK(count({5, 5, 5}, {5}) == 3);
  // L = 0 counts nothing
  CHECK(count({5, 5, 5}, {}) == 0);
  CHECK(count({}, {}) == 0);
}

template <typename T>
static std::vector<T> parse_list(const char *s) {
  std::vector<T> v;
  while (*s) {
    char *e;
    v.push_back((T)strtoll(s, &e, 10));
    s = *e == ',' ? e + 1 : e;
  }
  return v;
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "--count")) {
    printf("%lld\n", (long long)count(parse_list<int32_t>(argv[3]), parse_list<int32_t>(argv[2])));
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "--validate")) {
    const Res r = run(parse_list<int64_t>(argv[3]), parse_list<int32_t>(argv[4]), atoll(argv[2]), true);
    printf("%d %d %d %s\n", r.rc, (int)r.limit, r.phrase, r.msg.c_str());
    return 0;
  }
  validator_cases();
  count_cases();
  if (g_fail) {
    printf("%d check(s) FAILED\n", g_fail);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
