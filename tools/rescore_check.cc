// rescore_check -- host check of csrc/sme_rescore.hpp: the validator of a rescore
// batch (both offset arrays, the term ids, the host candidate lists and their
// order), its limits, the option's values and the rule that picks a slot's form.
// Built with the address and undefined-behaviour sanitizers (make -C <package>
// rescore-check): a read past an array stops the program -- every array handed to
// the validator is an exactly sized heap copy.
//
//   rescore_check     built-in cases; prints "all passed"
#include <stdio.h>

#include <limits>
#include <memory>
#include <vector>

#include "sme_rescore.hpp"

using namespace sme::rescore;

static int g_fail = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                             \
    }                                                       \
  } while (0)

struct Q {
  std::vector<int32_t> term, doc;
  std::vector<int64_t> qoff{0}, doff{0};
  void query(std::vector<int32_t> ids, std::vector<int32_t> docs) {
    term.insert(term.end(), ids.begin(), ids.end());
    qoff.push_back((int64_t)term.size());
    doc.insert(doc.end(), docs.begin(), docs.end());
    doff.push_back((int64_t)doc.size());
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
// The term array cut to nterms entries and the candidate array cut to ndocs (exactly
// sized heap copies) with those sizes declared, or (implied) whole with the sizes
// left to the offsets; docs == false: the candidates are not handed over at all (the
// device entry's use).
static Res run(const Q &s, int64_t V, int64_t nterms, int64_t ndocs, bool implied = false, bool docs = true) {
  auto t = exact(s.term, (size_t)nterms);
  auto d = exact(s.doc, (size_t)ndocs);
  auto q = exact(s.qoff, s.qoff.size());
  auto o = exact(s.doff, s.doff.size());
  Res r;
  r.rc = validate(t.get(), implied ? -1 : nterms, q.get(), docs ? d.get() : nullptr, implied ? -1 : ndocs, o.get(),
                  (int)s.qoff.size() - 1, V, &r.query);
  return r;
}
static Res run(const Q &s, int64_t V) {
  const Res a = run(s, V, (int64_t)s.term.size(), (int64_t)s.doc.size());
  const Res b = run(s, V, (int64_t)s.term.size(), (int64_t)s.doc.size(), true);
  CHECK(a.rc == b.rc && a.query == b.query);
  return a;
}
static Res run_device(const Q &s, int64_t V) {
  return run(s, V, (int64_t)s.term.size(), (int64_t)s.doc.size(), false, false);
}

static const int32_t kLo = std::numeric_limits<int32_t>::min(), kHi = std::numeric_limits<int32_t>::max();

static Q small_valid() {
  Q s;
  s.query({0, 3, -1}, {-5, 0, 7});
  s.query({}, {1, 2});
  s.query({9, 9, 2}, {});
  s.query({-1}, {kLo, -1, kHi});
  s.query({1}, {4});
  return s;
}

static void structure_cases() {
  const int64_t V = 10;
  Res r = run(small_valid(), V);
  CHECK(r.rc == R_OK && r.query == -1);
  CHECK(run_device(small_valid(), V).rc == R_OK);
  {
    int bad = 0;  // no query at all: no array is read
    CHECK(validate(nullptr, -1, nullptr, nullptr, -1, nullptr, 0, V, &bad) == R_OK && bad == -1);
    CHECK(validate(nullptr, 0, nullptr, nullptr, 0, nullptr, -1, V, &bad) == R_QOFFSETS);
  }
  {
    Q t;  // the slot limit itself is accepted, one more is not, and the query is named
    t.query({1}, {3});
    t.query(std::vector<int32_t>(kMaxSlots, (int32_t)V - 1), {4, 5});
    CHECK(run(t, V).rc == R_OK);
    t.query(std::vector<int32_t>(kMaxSlots + 1, -1), {});
    r = run(t, V);
    CHECK(r.rc == R_SLOTS && r.query == 2);
    r = run_device(t, V);
    CHECK(r.rc == R_SLOTS && r.query == 2);
  }
  {
    Q s = small_valid();  // slot offsets that descend or do not start at 0
    s.qoff[2] = 2;
    r = run(s, V);
    CHECK(r.rc == R_QOFFSETS && r.query == 1);
    s = small_valid();
    s.qoff[0] = 1;
    CHECK(run(s, V).rc == R_QOFFSETS);
    s = small_valid();
    s.qoff[0] = -1;
    CHECK(run(s, V).rc == R_QOFFSETS);
    s = small_valid();
    s.qoff[5] = std::numeric_limits<int64_t>::max();  // past the array
    r = run(s, V, (int64_t)s.term.size(), (int64_t)s.doc.size());
    CHECK(r.rc == R_QOFFSETS && r.query == 4);
    s = small_valid();
    s.qoff[5] = s.qoff[4] = 6;  // fewer slots than the array holds: inconsistent
    CHECK(run(s, V, (int64_t)s.term.size(), (int64_t)s.doc.size()).rc == R_QOFFSETS);
  }
  {
    Q s = small_valid();  // the same for the candidates' offsets
    s.doff[2] = 2;
    r = run(s, V);
    CHECK(r.rc == R_DOFFSETS && r.query == 1);
    CHECK(run_device(s, V).rc == R_DOFFSETS);
    s = small_valid();
    s.doff[0] = 1;
    CHECK(run(s, V).rc == R_DOFFSETS);
    s = small_valid();
    s.doff[0] = -1;
    CHECK(run(s, V).rc == R_DOFFSETS);
    s = small_valid();
    s.doff[5] = std::numeric_limits<int64_t>::max();
    r = run(s, V, (int64_t)s.term.size(), (int64_t)s.doc.size());
    CHECK(r.rc == R_DOFFSETS && r.query == 4);
    s = small_valid();
    s.doff[5] = s.doff[4] = 7;
    CHECK(run(s, V, (int64_t)s.term.size(), (int64_t)s.doc.size()).rc == R_DOFFSETS);
  }
  {
    // the batch limits, through offsets alone (implied sizes; no slot or candidate is
    // read: the limit is refused first)
    const int64_t q1[] = {0, kMaxBatch + 1}, d1[] = {0, 0};
    int bad = 0;
    CHECK(validate(nullptr, -1, q1, nullptr, -1, d1, 1, V, &bad) == R_BATCH && bad == -1);
    const int64_t q2[] = {0, 0}, d2[] = {0, kMaxBatch + 1};
    CHECK(validate(nullptr, -1, q2, nullptr, -1, d2, 1, V, &bad) == R_BATCH && bad == -1);
    const int64_t d3[] = {0, kMaxBatch};  // the limit itself, candidates not handed over
    CHECK(validate(nullptr, -1, q2, nullptr, -1, d3, 1, V, &bad) == R_OK);
  }
  {
    Q s = small_valid();  // ids
    s.term[4] = (int32_t)V;
    r = run(s, V);
    CHECK(r.rc == R_TERM && r.query == 2);
    CHECK(run_device(s, V).rc == R_TERM);
    s.term[4] = -2;
    CHECK(run(s, V).rc == R_TERM);
    s.term[4] = kLo;
    CHECK(run(s, V).rc == R_TERM);
    s.term[4] = (int32_t)V - 1;
    CHECK(run(s, V).rc == R_OK);
    CHECK(run(s, 0).rc == R_TERM);  // no term at all: only -1 is an id
  }
  {
    Q s = small_valid();  // candidates: an equal pair, a descending pair, the signed order
    s.doc[1] = s.doc[0];
    r = run(s, V);
    CHECK(r.rc == R_ORDER && r.query == 0);
    CHECK(run_device(s, V).rc == R_OK);  // (not handed over: a kernel's check)
    s = small_valid();
    s.doc[4] = 0;  // query 1: {1, 0}
    r = run(s, V);
    CHECK(r.rc == R_ORDER && r.query == 1);
    s = small_valid();
    s.doc[5] = 0;  // query 3: {0, -1, max}: an unsigned order would pass the first pair
    r = run(s, V);
    CHECK(r.rc == R_ORDER && r.query == 3);
    s = small_valid();
    s.doc[2] = 100;  // a query's last above the next one's first is no fault: {.., 100} {1, 2}
    CHECK(run(s, V).rc == R_OK);
    Q one;
    one.query({}, {5});
    CHECK(run(one, V).rc == R_OK);
  }
  {
    // every truncation of a small valid batch: an array cut short, the offsets
    // unchanged -- refused before anything past the array's end is read
    const Q s = small_valid();
    const int64_t NT = (int64_t)s.term.size(), ND = (int64_t)s.doc.size();
    for (int64_t nt = 0; nt <= NT; nt++) {
      r = run(s, V, nt, ND);
      CHECK((r.rc == R_OK) == (nt == NT));
      if (nt < NT) CHECK(r.rc == R_QOFFSETS);
    }
    for (int64_t nd = 0; nd <= ND; nd++) {
      r = run(s, V, NT, nd);
      CHECK((r.rc == R_OK) == (nd == ND));
      if (nd < ND) CHECK(r.rc == R_DOFFSETS);
    }
    for (size_t nq = 0; nq + 1 < s.qoff.size(); nq++) {  // and of the query list
      Q c = s;
      c.qoff.resize(nq + 1);
      c.doff.resize(nq + 1);
      r = run(c, V, NT, ND);
      CHECK(nq == 0 ? r.rc == R_OK : r.rc == R_QOFFSETS);  // (no query: nothing is read)
      c = s;
      c.qoff.resize(nq + 1);
      c.doff.resize(nq + 1);
      c.term.resize((size_t)c.qoff.back());  // the slots agree, the candidates do not
      r = run(c, V, (int64_t)c.term.size(), ND);
      CHECK(nq == 0 ? r.rc == R_OK : r.rc == R_DOFFSETS);
    }
  }
}

static void option_cases() {
  CHECK(legal_path(PATH_AUTO) && legal_path(PATH_SEARCH) && legal_path(PATH_SCAN));
  CHECK(!legal_path(-1) && !legal_path(3));
  CHECK(legal_model(MODEL_TFIDF) && legal_model(MODEL_BM25) && !legal_model(2) && !legal_model(-1));
  CHECK(search_steps(1) == 1 && search_steps(2) == 2 && search_steps(3) == 2 && search_steps(1024) == 11);
  CHECK(search_steps(std::numeric_limits<int64_t>::max()) == 63);
  // a range as long as a full tile is scanned, one far longer is searched, whatever
  // the tile holds; a handful of candidates search anything longer than a few rounds
  for (int64_t cands : {1, 2, 63, 64, 255, 256, 257, 1023, 1024}) {
    CHECK(!scan_is_cheaper(int64_t(1) << 31, cands));
    CHECK(!scan_is_cheaper(int64_t(1) << 20, cands));
  }
  for (int64_t cands : {1, 5, 64}) CHECK(!scan_is_cheaper(16 * kLanes, cands));
  for (int64_t cands : {769, 1023, 1024}) CHECK(scan_is_cheaper(cands, cands) && scan_is_cheaper(kLanes, cands));
  CHECK(scan_is_cheaper(kTile, kTile));
}

int main() {
  structure_cases();
  option_cases();
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
