// bm25_check -- host check of csrc/sme_bm25.hpp, the batch validator, the parameter
// rule and the entry-bar key of BM25 ranking, and the weight / bound functions that
// csrc/sme_bm25.hip calls.  Built with the address and undefined-behaviour sanitizers
// (make -C <package> bm25-check): a read past an array stops the program -- every
// array handed to the validator is an exactly sized heap copy.
//
//   bm25_check                   built-in cases; prints "all passed"
//   bm25_check --weight T...     per tuple T = k1,b,tf,dl,avgdl,df,D (k1, b and avgdl as
//                                the hex of their IEEE bits, the rest decimal) one line:
//                                the hex bits of idf, norm, weight and of the bound term
//                                with tf as the term's largest tf and dl as the window's
//                                shortest document
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <memory>
#include <vector>

#include "sme_bm25.hpp"

using namespace sme::bm25;

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
  std::vector<int64_t> qoff{0};
  void query(std::vector<int32_t> ids) {
    term.insert(term.end(), ids.begin(), ids.end());
    qoff.push_back((int64_t)term.size());
  }
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
// The term array cut to nterms entries (an exactly sized heap copy) with that size
// declared, or (implied) whole with the size left to the offsets; ids == false: the
// ids are not handed over at all (the device entry's use).
static Res run(const Q &s, int64_t V, int64_t nterms, bool implied = false, bool ids = true) {
  auto t = exact(s.term, (size_t)nterms);
  auto q = exact(s.qoff, s.qoff.size());
  Res r;
  r.rc = validate(ids ? t.get() : nullptr, implied ? -1 : nterms, q.get(), (int)s.qoff.size() - 1, V, &r.query);
  return r;
}
static Res run(const Q &s, int64_t V) {
  const Res a = run(s, V, (int64_t)s.term.size());
  const Res b = run(s, V, (int64_t)s.term.size(), true);
  CHECK(a.rc == b.rc && a.query == b.query);
  return a;
}

static Q small_valid() {
  Q s;
  s.query({0, 3, -1});
  s.query({});
  s.query({9, 9, 2});
  s.query({-1});
  return s;
}

static void structure_cases() {
  const int64_t V = 10;
  Res r = run(small_valid(), V);
  CHECK(r.rc == M_OK && r.query == -1);
  {
    int bad = 0;  // no query at all: no array is read
    CHECK(validate(nullptr, -1, nullptr, 0, V, &bad) == M_OK && bad == -1);
    CHECK(validate(nullptr, 0, nullptr, -1, V, &bad) == M_OFFSETS);
    Q s;
    s.query({});
    CHECK(run(s, V).rc == M_OK);
  }
  {
    Q t;  // the limit itself is accepted, one more is not, and the query is named
    t.query({1});
    t.query(std::vector<int32_t>(kMaxSlots, (int32_t)V - 1));
    CHECK(run(t, V).rc == M_OK);
    t.query(std::vector<int32_t>(kMaxSlots + 1, -1));
    r = run(t, V);
    CHECK(r.rc == M_SLOTS && r.query == 2);
    r = run(t, V, (int64_t)t.term.size(), false, false);
    CHECK(r.rc == M_SLOTS && r.query == 2);
  }
  {
    Q s = small_valid();  // offsets that descend or do not start at 0
    s.qoff[2] = 2;
    r = run(s, V);
    CHECK(r.rc == M_OFFSETS && r.query == 1);
    s = small_valid();
    s.qoff[0] = 1;
    CHECK(run(s, V).rc == M_OFFSETS);
    s = small_valid();
    s.qoff[0] = -1;
    CHECK(run(s, V).rc == M_OFFSETS);
    s = small_valid();
    s.qoff[4] = std::numeric_limits<int64_t>::max();  // past the array
    r = run(s, V, (int64_t)s.term.size());
    CHECK(r.rc == M_OFFSETS && r.query == 3);
    s = small_valid();
    s.qoff[4] = 6;  // fewer slots than the array holds: inconsistent
    CHECK(run(s, V, (int64_t)s.term.size()).rc == M_OFFSETS);
  }
  {
    Q s = small_valid();  // ids
    s.term[4] = (int32_t)V;
    r = run(s, V);
    CHECK(r.rc == M_TERM && r.query == 2);
    CHECK(run(s, V, (int64_t)s.term.size(), false, false).rc == M_OK);  // (ids not handed over: not read)
    s.term[4] = -2;
    CHECK(run(s, V).rc == M_TERM);
    s.term[4] = std::numeric_limits<int32_t>::min();
    CHECK(run(s, V).rc == M_TERM);
    s.term[4] = (int32_t)V - 1;
    CHECK(run(s, V).rc == M_OK);
    CHECK(run(s, 0).rc == M_TERM);  // no term at all: only -1 is an id
  }
  {
    // every truncation of a small valid batch: the term array cut short, the offsets
    // unchanged -- refused before anything past the array's end is read
    const Q s = small_valid();
    const int64_t NT = (int64_t)s.term.size();
    for (int64_t nt = 0; nt <= NT; nt++) {
      r = run(s, V, nt);
      CHECK((r.rc == M_OK) == (nt == NT));
      if (nt < NT) CHECK(r.rc == M_OFFSETS);
    }
    for (size_t nq = 0; nq + 1 < s.qoff.size(); nq++) {  // and of the query list
      Q c = s;
      c.qoff.resize(nq + 1);
      r = run(c, V, NT);
      CHECK(nq == 0 ? r.rc == M_OK : r.rc == M_OFFSETS);  // (no query: nothing is read)
    }
  }
}

static void param_cases() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(legal_params(1.2, 0.75) && legal_params(0.0, 0.0) && legal_params(0.0, 1.0) && legal_params(1e300, 0.5));
  CHECK(legal_params(-0.0, -0.0));
  CHECK(!legal_params(-1e-9, 0.75) && !legal_params(inf, 0.75) && !legal_params(nan, 0.75));
  CHECK(!legal_params(1.2, -1e-9) && !legal_params(1.2, 1.5) && !legal_params(1.2, nan) && !legal_params(1.2, inf));
}

static void key_cases() {
  const double inf = std::numeric_limits<double>::infinity();
  const double tab[] = {0.0, 1.0, -1.0, 2.0, 0.5, 1e-300, -1e-300, 1e300, 5e-324, 11.7, 1.0 + 2.220446049250313e-16,
                        inf, -inf, 0.6931471805599453};
  const int n = (int)(sizeof(tab) / sizeof(tab[0]));
  for (int i = 0; i < n; i++) {
    CHECK(bar_key(tab[i]) != 0);  // 0 stays below every score: "no bar yet"
    CHECK(bar_value(bar_key(tab[i])) == tab[i]);
    for (int j = 0; j < n; j++) CHECK((bar_key(tab[i]) < bar_key(tab[j])) == (tab[i] < tab[j]));
  }
}

// the bound covers every weight of a smaller tf in a longer document
static void bound_cases() {
  const double k1s[] = {0.0, 0.9, 1.2, 2.0}, bs[] = {0.0, 0.75, 1.0};
  const double tfs[] = {1, 2, 3, 7, 1023, 16777216.0}, dls[] = {1, 5, 40, 100, 5000, 2147483647.0};
  const double avgdl = 100.0, idf = idf_value(1000, 10);
  for (double k1 : k1s)
    for (double b : bs)
      for (double maxtf : tfs)
        for (double mindl : dls) {
          const double bound = bound_term(idf, maxtf, k1, b, mindl, avgdl);
          for (double tf : tfs)
            for (double dl : dls)
              if (tf <= maxtf && dl >= mindl) CHECK(weight(idf, tf, k1, doc_norm(k1, b, dl, avgdl)) <= bound);
        }
  CHECK(idf_value(1, 1) > 0.0 && idf_value(1000, 1000) > 0.0 && idf_value(1000, 1) > idf_value(1000, 2));
}

static double from_hex(const char *s) {
  const uint64_t b = strtoull(s, nullptr, 16);
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}
static unsigned long long bits(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  return (unsigned long long)b;
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "--weight")) {
    for (int i = 2; i < argc; i++) {
      std::vector<char> buf(argv[i], argv[i] + strlen(argv[i]) + 1);
      std::vector<char *> f;
      for (char *p = strtok(buf.data(), ","); p; p = strtok(nullptr, ",")) f.push_back(p);
      if (f.size() != 7) {
        fprintf(stderr, "bad tuple %s\n", argv[i]);
        return 2;
      }
      const double k1 = from_hex(f[0]), b = from_hex(f[1]), avgdl = from_hex(f[4]);
      const long long tf = atoll(f[2]), dl = atoll(f[3]), df = atoll(f[5]), D = atoll(f[6]);
      const double idf = idf_value(D, df), norm = doc_norm(k1, b, (double)dl, avgdl);
      printf("%016llx %016llx %016llx %016llx\n", bits(idf), bits(norm), bits(weight(idf, (double)tf, k1, norm)),
             bits(bound_term(idf, (double)tf, k1, b, (double)dl, avgdl)));
    }
    return 0;
  }
  structure_cases();
  param_cases();
  key_cases();
  bound_cases();
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
