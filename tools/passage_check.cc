// passage_check -- host check of csrc/sme_passage.hpp: the validator of a passages
// batch (both offset arrays, the term ids, the host candidate lists and their order),
// its limits, the normaliser that turns listed ids into slots, and the restatement of
// one record's best window, held here to windows worked out by hand and to a second,
// sliding, count over random records.  Built with the address and undefined-behaviour
// sanitizers (make -C <package> passage-check): a read past an array stops the
// program -- every array handed over is an exactly sized heap copy.
//
//   passage_check     built-in cases; prints "all passed"
#include <stdio.h>

#include <limits>
#include <memory>
#include <vector>

#include "sme_passage.hpp"

using namespace sme::passage;

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

static const int32_t kLo = std::numeric_limits<int32_t>::min(), kHi = std::numeric_limits<int32_t>::max();

static Q small_valid() {
  Q s;
  s.query({0, 3, -1}, {-5, 0, 7});
  s.query({}, {1, 2});
  s.query({9, 9, 2}, {});
  s.query({-1}, {kLo, -1, kHi});
  return s;
}

static void validator() {
  const Q ok = small_valid();
  Res r = run(ok, 10);
  CHECK(r.rc == P_OK && r.query == -1);
  r = run(ok, 10, (int64_t)ok.term.size(), (int64_t)ok.doc.size(), false, false);
  CHECK(r.rc == P_OK);
  int bad = 7;
  CHECK(validate(nullptr, -1, nullptr, nullptr, -1, nullptr, 0, 10, &bad) == P_OK && bad == -1);
  CHECK(validate(nullptr, -1, nullptr, nullptr, -1, nullptr, -1, 10, &bad) == P_QOFFSETS);
  // every truncation of either array, with its size declared
  for (size_t n = 0; n < ok.term.size(); n++) CHECK(run(ok, 10, (int64_t)n, (int64_t)ok.doc.size()).rc == P_QOFFSETS);
  for (size_t n = 0; n < ok.doc.size(); n++) CHECK(run(ok, 10, (int64_t)ok.term.size(), (int64_t)n).rc == P_DOFFSETS);
  {
    Q s = ok;
    s.qoff[0] = 1;
    CHECK(run(s, 10).rc == P_QOFFSETS);
    s = ok;
    s.qoff[2] = 1;  // descends
    r = run(s, 10, (int64_t)s.term.size(), (int64_t)s.doc.size());
    CHECK(r.rc == P_QOFFSETS && r.query == 1);
    s = ok;
    s.doff[0] = 2;
    CHECK(run(s, 10).rc == P_DOFFSETS);
    s = ok;
    s.doff[3] = 2;
    r = run(s, 10, (int64_t)s.term.size(), (int64_t)s.doc.size());
    CHECK(r.rc == P_DOFFSETS && r.query == 2);
  }
  {  // term ids
    Q s = ok;
    s.term[1] = 10;
    r = run(s, 10);
    CHECK(r.rc == P_TERM && r.query == 0);
    s.term[1] = 9;
    CHECK(run(s, 10).rc == P_OK);
    s.term[5] = -2;
    r = run(s, 10);
    CHECK(r.rc == P_TERM && r.query == 2);
  }
  {  // the candidates' order: signed, strict, per query
    Q s;
    s.query({1}, {3, 4});
    s.query({1}, {1, 2});  // below the query before: no fault
    CHECK(run(s, 5).rc == P_OK);
    s.query({1}, {5, 5});
    r = run(s, 5);
    CHECK(r.rc == P_ORDER && r.query == 2);
    CHECK(run(s, 5, (int64_t)s.term.size(), (int64_t)s.doc.size(), false, false).rc == P_OK);  // (not read)
    Q t;
    t.query({1}, {7, kLo});
    CHECK(run(t, 5).rc == P_ORDER);
    Q u;
    u.query({1}, {kLo, -1, 0, kHi});
    CHECK(run(u, 5).rc == P_OK);
  }
  {  // the limits: kMaxListed listed, kMaxSlots distinct
    Q s;
    std::vector<int32_t> ids;
    for (int i = 0; i < kMaxListed; i++) ids.push_back(i % kMaxSlots);
    s.query({0}, {1});
    s.query(ids, {1});
    CHECK(run(s, 100).rc == P_OK);
    ids.push_back(-1);
    Q t;
    t.query({0}, {1});
    t.query(ids, {1});
    r = run(t, 100);
    CHECK(r.rc == P_LISTED && r.query == 1);
    ids.assign(kMaxSlots, 0);
    for (int i = 0; i < kMaxSlots; i++) ids[(size_t)i] = 99 - i;
    ids.push_back(-1);
    ids.push_back(99);
    Q v;
    v.query(ids, {});
    CHECK(run(v, 100).rc == P_OK);
    ids.push_back(7);  // the 65th distinct id
    Q x;
    x.query({}, {});
    x.query({}, {});
    x.query(ids, {});
    r = run(x, 100);
    CHECK(r.rc == P_SLOTS && r.query == 2);
  }
  {  // the batch limits: refused before any id or docno is read (the arrays hold one entry)
    const std::vector<int32_t> one{0};
    const std::vector<int64_t> big{0, int64_t(1) << 31}, small{0, 1};
    auto t = exact(one, 1);
    auto d = exact(one, 1);
    auto b = exact(big, 2);
    auto s = exact(small, 2);
    int q = 0;
    CHECK(validate(t.get(), -1, b.get(), d.get(), -1, s.get(), 1, 5, &q) == P_BATCH);
    CHECK(validate(t.get(), -1, s.get(), d.get(), -1, b.get(), 1, 5, &q) == P_BATCH);
  }
  CHECK(check_width(0) == P_WIDTH_LOW && check_width(-3) == P_WIDTH_LOW && check_width(1) == P_OK);
  CHECK(check_width(kMaxWidth) == P_OK && check_width(kMaxWidth + 1) == P_WIDTH_HIGH);
}

static void normaliser() {
  std::vector<int32_t> out{42};  // (appends: what stands before stays)
  const std::vector<int32_t> listed{5, -1, 3, 5, 5, 9, 3, -1};
  auto p = exact(listed, listed.size());
  CHECK(normalise(p.get(), (int64_t)listed.size(), out) == 3);
  CHECK((out == std::vector<int32_t>{42, 5, 3, 9}));
  CHECK(normalise(p.get(), 0, out) == 0 && out.size() == 4);
  std::vector<int32_t> many;
  for (int i = 0; i < kMaxSlots + 1; i++) many.push_back(i);
  auto m = exact(many, many.size());
  CHECK(normalise(m.get(), kMaxSlots, out) == kMaxSlots && out.size() == 4 + (size_t)kMaxSlots);
  out.resize(4);
  CHECK(normalise(m.get(), kMaxSlots + 1, out) == -1 && out.size() == 4);
}

// a second count of one record: the windows' slot counts slid along the stream
static Window sliding(const std::vector<int32_t> &st, int32_t rec, const std::vector<int32_t> &ids,
                      const std::vector<double> &idf, int width) {
  const int64_t n = (int64_t)st.size();
  std::vector<int> slot((size_t)n, -1);
  for (int64_t p = 0; p < n; p++)
    for (size_t j = 0; j < ids.size(); j++)
      if (ids[j] == st[(size_t)p]) slot[(size_t)p] = (int)j;
  std::vector<int> cnt(ids.size(), 0);
  Window best;
  const int64_t last = n > width ? n - width : 0;
  for (int64_t p = 0; p < std::min<int64_t>(width, n); p++)
    if (slot[(size_t)p] >= 0) cnt[(size_t)slot[(size_t)p]]++;
  for (int64_t s = 0; s <= last; s++) {
    if (s > 0) {
      if (slot[(size_t)s - 1] >= 0) cnt[(size_t)slot[(size_t)s - 1]]--;
      if (slot[(size_t)(s + width - 1)] >= 0) cnt[(size_t)slot[(size_t)(s + width - 1)]]++;
    }
    Window w;
    w.rec = rec;
    w.start = (int32_t)s;
    w.len = (int32_t)(std::min<int64_t>(s + width, n) - s);
    for (size_t j = 0; j < ids.size(); j++)
      if (cnt[j]) {
        w.mask |= uint64_t(1) << j;
        w.hits += cnt[j];
      }
    w.score = score_of(w.mask, idf.data());
    if (s == 0 || before(w, best)) best = w;
  }
  return best;
}

static Window best(const std::vector<int32_t> &st, int32_t rec, const std::vector<int32_t> &ids,
                   const std::vector<double> &idf, int width) {
  auto s = exact(st, st.size());
  auto i = exact(ids, ids.size());
  auto f = exact(idf, idf.size());
  return best_of_record(s.get(), (int64_t)st.size(), rec, i.get(), (int)ids.size(), f.get(), width);
}
static bool same(const Window &a, const Window &b) {
  return a.rec == b.rec && a.start == b.start && a.len == b.len && a.hits == b.hits && a.mask == b.mask &&
         a.score == b.score;
}

static void windows() {
  const std::vector<int32_t> ids{7, 3, 9};  // slots 0, 1, 2
  const std::vector<double> idf{1.5, 0.25, 0.0};
  // positions:                   0  1  2  3  4  5  6  7  8
  const std::vector<int32_t> st{3, 1, 7, 1, 1, 3, 9, 7, 1};
  Window w = best(st, 4, ids, idf, 1);
  CHECK(w.rec == 4 && w.start == 2 && w.len == 1 && w.hits == 1 && w.mask == 1 && w.score == 1.5);
  w = best(st, 0, ids, idf, 3);  // [0,3) and [5,8) cover slots 0, 1; [5,8) also 2: cover decides (idf 0.0)
  CHECK(w.start == 5 && w.len == 3 && w.hits == 3 && w.mask == 7 && w.score == 0.0 + 1.5 + 0.25 + 0.0);
  w = best(st, 0, ids, idf, 2);  // [1,3) {7}, [2,4) {7}: equal, the earlier wins; [6,8) {9, 7} has more cover
  CHECK(w.start == 6 && w.mask == 5 && w.hits == 2 && w.score == 1.5);
  w = best(st, 0, ids, idf, 100);  // shorter than the width: the one window
  CHECK(w.start == 0 && w.len == 9 && w.hits == 5 && w.mask == 7);
  w = best({}, 2, ids, idf, 5);  // an empty record
  CHECK(w.rec == 2 && w.start == 0 && w.len == 0 && w.hits == 0 && w.mask == 0 && w.score == 0.0);
  w = best({1, 1, 1}, 0, ids, idf, 2);  // no hit at all: the first window
  CHECK(w.start == 0 && w.len == 2 && w.hits == 0 && w.mask == 0);
  w = best({3, 3, 1, 3}, 0, ids, idf, 2);  // equal score and cover: hits decide
  CHECK(w.start == 0 && w.hits == 2 && w.mask == 2);
  w = best({1, 7, 1, 7}, 0, ids, idf, 2);  // wholly equal windows: the first start
  CHECK(w.start == 0 && w.hits == 1);
  w = best({1, 1, 1, 7}, 0, ids, idf, 2);  // the last start of the record
  CHECK(w.start == 2 && w.len == 2 && w.hits == 1);
  w = best(st, 0, {}, {}, 4);  // a query without ids
  CHECK(w.start == 0 && w.len == 4 && w.mask == 0 && w.score == 0.0);
  // the order of two windows of different records
  Window a, b;
  a.rec = 1;
  b.rec = 0;
  CHECK(before(b, a) && !before(a, b));
  a.score = 0.5;
  CHECK(before(a, b));
  // the sum runs over the set bits in ascending slot order: (0.1 + 0.2) + 0.3, not 0.1 + (0.2 + 0.3)
  const std::vector<double> tenths{0.1, 0.2, 0.3};
  CHECK(score_of(7, tenths.data()) == (0.1 + 0.2) + 0.3 && score_of(7, tenths.data()) != 0.1 + (0.2 + 0.3));
  // random records against the sliding count
  uint64_t x = 88172645463325252ull;
  auto rnd = [&](int n) {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return (int)(x % (uint64_t)n);
  };
  for (int it = 0; it < 300; it++) {
    std::vector<int32_t> s((size_t)rnd(40));
    for (auto &t : s) t = rnd(8);
    std::vector<int32_t> q;
    std::vector<double> f;
    for (int t = 0; t < 8; t++)
      if (rnd(3) == 0) {
        q.push_back(t);
        f.push_back(rnd(3) * 0.125);
      }
    const int width = 1 + rnd(12);
    CHECK(same(best(s, it % 3, q, f, width), sliding(s, it % 3, q, f, width)));
  }
}

int main() {
  validator();
  normaliser();
  windows();
  if (g_fail) {
    printf("%d check(s) FAILED\n", g_fail);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
