// bool_check -- host check of csrc/sme_bool.hpp, the validator of the Boolean query
// structure (queries -> groups -> term slots) and the score sort key that
// csrc/sme_bool.hip calls.  Built with the address and undefined-behaviour
// sanitizers (make -C <package> bool-check): a read past an array stops the
// program -- every array handed to the validator is an exactly sized heap copy.
//
//   bool_check                 built-in cases; prints "all passed"
//   bool_check --key HEX...    the score key (hex) of each double given as the hex
//                              of its IEEE bits, one per line
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <memory>
#include <vector>

#include "sme_bool.hpp"

using namespace sme::boolq;

static int g_fail = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                             \
    }                                                       \
  } while (0)

struct Q {
  std::vector<int32_t> term;
  std::vector<int64_t> goff{0}, qoff{0};
  std::vector<uint8_t> flag;
  void group(std::vector<int32_t> ids, int f) {
    term.insert(term.end(), ids.begin(), ids.end());
    goff.push_back((int64_t)term.size());
    flag.push_back((uint8_t)f);
  }
  void end_query() { qoff.push_back((int64_t)flag.size()); }
};

template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v, size_t n) {
  std::unique_ptr<T[]> p(new T[n]);
  for (size_t i = 0; i < n; i++) p[i] = v[i];
  return p;
}

struct Res {
  int rc, query;
};
// The arrays cut to nterms / ngroups entries (exactly sized heap copies) with
// those sizes declared, or (implied) the whole arrays with the sizes left to the
// offsets as a C-ABI caller passes them.
static Res run(const Q &s, int64_t V, int64_t nterms, int64_t ngroups, bool implied = false) {
  auto t = exact(s.term, (size_t)nterms);
  auto g = exact(s.goff, (size_t)ngroups + 1);
  auto f = exact(s.flag, (size_t)ngroups);
  auto q = exact(s.qoff, s.qoff.size());
  Res r;
  r.rc = validate(t.get(), implied ? -1 : nterms, g.get(), implied ? -1 : ngroups, f.get(), q.get(),
                  (int)s.qoff.size() - 1, V, &r.query);
  return r;
}
static Res run(const Q &s, int64_t V) {
  const Res a = run(s, V, (int64_t)s.term.size(), (int64_t)s.flag.size());
  const Res b = run(s, V, (int64_t)s.term.size(), (int64_t)s.flag.size(), true);
  CHECK(a.rc == b.rc && a.query == b.query);
  return a;
}

static Q small_valid() {
  Q s;
  s.group({0, 3}, 0);
  s.group({-1}, 1);
  s.group({}, 0);
  s.end_query();
  s.end_query();  // an empty query
  s.group({9, 9, 2}, 0);
  s.end_query();
  return s;
}

static void structure_cases() {
  const int64_t V = 10;
  Res r = run(small_valid(), V);
  CHECK(r.rc == B_OK && r.query == -1);
  {
    Q s;  // no query at all: no array is read
    int bad = 0;
    CHECK(validate(nullptr, -1, nullptr, -1, nullptr, nullptr, 0, V, &bad) == B_OK && bad == -1);
    CHECK(validate(nullptr, 0, nullptr, 0, nullptr, nullptr, -1, V, &bad) == B_OFFSETS);
    s.end_query();  // one query without groups
    r = run(s, V);
    CHECK(r.rc == B_OK);
  }
  {
    Q t;  // the limits themselves are accepted
    for (int g = 0; g < kMaxGroups; g++) t.group(std::vector<int32_t>(kMaxSlots / kMaxGroups, 1), g & 1);
    t.end_query();
    CHECK(run(t, V).rc == B_OK);
    t = Q();
    t.group(std::vector<int32_t>(kMaxSlots, (int32_t)V - 1), 0);
    t.end_query();
    CHECK(run(t, V).rc == B_OK);
  }
  // descending offsets
  {
    Q s = small_valid();
    s.qoff[2] = 2;  // query 1 ends before it begins
    r = run(s, V);
    CHECK(r.rc == B_OFFSETS && r.query == 1);
    s = small_valid();
    s.goff[2] = 1;  // group 1 ends before it begins
    r = run(s, V);
    CHECK(r.rc == B_OFFSETS && r.query == 0);
    s = small_valid();
    s.qoff[0] = 1;
    CHECK(run(s, V).rc == B_OFFSETS);
    s = small_valid();
    s.goff[0] = 1;
    CHECK(run(s, V).rc == B_OFFSETS);
    s = small_valid();
    s.qoff[0] = -1;
    CHECK(run(s, V).rc == B_OFFSETS);
  }
  // offsets past the arrays (declared sizes: the arrays end where they say)
  {
    Q s = small_valid();
    s.qoff[3] = 5;  // one group more than there are
    r = run(s, V, (int64_t)s.term.size(), (int64_t)s.flag.size());
    CHECK(r.rc == B_OFFSETS && r.query == 2);
    s = small_valid();
    s.goff[4] = 7;  // one slot more than there are
    r = run(s, V, (int64_t)s.term.size(), (int64_t)s.flag.size());
    CHECK(r.rc == B_OFFSETS && r.query == 2);
    s = small_valid();
    s.qoff[3] = 3;  // fewer groups than the arrays hold: inconsistent
    r = run(s, V, (int64_t)s.term.size(), (int64_t)s.flag.size());
    CHECK(r.rc == B_OFFSETS);
    s = small_valid();
    s.goff[4] = 5;  // fewer slots than the array holds
    r = run(s, V, (int64_t)s.term.size(), (int64_t)s.flag.size());
    CHECK(r.rc == B_OFFSETS);
  }
  // flags, limits, ids
  {
    Q s = small_valid();
    s.flag[3] = 2;
    r = run(s, V);
    CHECK(r.rc == B_FLAG && r.query == 2);
    s.flag[3] = 255;
    CHECK(run(s, V).rc == B_FLAG);
    Q t;
    t.group({1}, 0);
    t.end_query();
    for (int g = 0; g < kMaxGroups + 1; g++) t.group({}, 0);
    t.end_query();
    r = run(t, V);
    CHECK(r.rc == B_GROUPS && r.query == 1);
    t = Q();
    t.group(std::vector<int32_t>(kMaxSlots, 1), 0);
    t.group({1}, 1);
    t.end_query();
    r = run(t, V);
    CHECK(r.rc == B_SLOTS && r.query == 0);
    s = small_valid();
    s.term[4] = (int32_t)V;
    r = run(s, V);
    CHECK(r.rc == B_TERM && r.query == 2);
    s.term[4] = -2;
    CHECK(run(s, V).rc == B_TERM);
    s.term[4] = std::numeric_limits<int32_t>::min();
    CHECK(run(s, V).rc == B_TERM);
    s.term[4] = (int32_t)V - 1;
    CHECK(run(s, V).rc == B_OK);
    CHECK(run(s, 0).rc == B_TERM);  // no term at all: only -1 is an id
  }
  // every truncation of a small valid structure: the arrays cut short, the
  // offsets unchanged -- refused before anything past an array's end is read
  {
    const Q s = small_valid();
    const int64_t NT = (int64_t)s.term.size(), NG = (int64_t)s.flag.size();
    for (int64_t nt = 0; nt <= NT; nt++)
      for (int64_t ng = 0; ng <= NG; ng++) {
        r = run(s, V, nt, ng);
        CHECK((r.rc == B_OK) == (nt == NT && ng == NG));
        if (nt < NT || ng < NG) CHECK(r.rc == B_OFFSETS);
      }
    // and of the query list
    for (size_t nq = 0; nq + 1 < s.qoff.size(); nq++) {
      Q c = s;
      c.qoff.resize(nq + 1);
      r = run(c, V, NT, NG);
      CHECK(nq == 0 ? r.rc == B_OK : r.rc == B_OFFSETS);  // (no query: nothing is read)
    }
  }
}

static void key_cases() {
  const double inf = std::numeric_limits<double>::infinity();
  const double tab[] = {0.0,     -0.0,   1.0,     -1.0,   2.0,  0.5,   1e-300, -1e-300, 1e300, -1e300, 5e-324, -5e-324,
                        2.2250738585072014e-308, 1.0 + 2.220446049250313e-16, 1.0 - 1.1102230246251565e-16, 3.25, 3.25,
                        1.7976931348623157e308,  -1.7976931348623157e308,     inf, -inf, 0.30102999566398120, 12.5};
  const int n = (int)(sizeof(tab) / sizeof(tab[0]));
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      // descending: a greater score has the smaller key; equal doubles one key
      CHECK((score_key(tab[i]) < score_key(tab[j])) == (tab[i] > tab[j]));
      CHECK((score_key(tab[i]) == score_key(tab[j])) == (tab[i] == tab[j]));
    }
  CHECK(score_key(0.0) == score_key(-0.0));
  CHECK(docno_key(std::numeric_limits<int32_t>::min()) == 0u && docno_key(-1) == 0x7FFFFFFFu);
  CHECK(docno_key(0) == 0x80000000u && docno_key(std::numeric_limits<int32_t>::max()) == 0xFFFFFFFFu);
  const int32_t d[] = {std::numeric_limits<int32_t>::min(), -7, -1, 0, 1, 700, std::numeric_limits<int32_t>::max()};
  for (int i = 0; i + 1 < 7; i++) CHECK(docno_key(d[i]) < docno_key(d[i + 1]));
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "--key")) {
    for (int i = 2; i < argc; i++) {
      const uint64_t b = strtoull(argv[i], nullptr, 16);
      double v;
      memcpy(&v, &b, sizeof(v));
      printf("%016llx\n", (unsigned long long)score_key(v));
    }
    return 0;
  }
  structure_cases();
  key_cases();
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
