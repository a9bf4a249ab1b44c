// ixmerge_check -- host check of csrc/sme_ixmerge.hpp: the validator of the index
// merger's input list with its messages, the diagonal search that cuts the n-way
// merge into tiles, and the plain n-way merge of one term that csrc/sme_ixmerge.hip
// restates on the device.  Built with the address and undefined-behaviour
// sanitizers (make -C <package> ixmerge-check): a read past an array stops the
// program -- every array handed to the header is an exactly sized heap copy.
//
//   ixmerge_check                      built-in cases; prints "all passed"
//   ixmerge_check --validate CTXK SPEC "<rc> <notimpl 0/1> <input> <message>" for the list
//                                      SPEC: one letter per input, comma-separated --
//                                      o ok, n null, c other context, r records-only,
//                                      g chargram output, k K = 2 ("" = no inputs)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "sme_ixmerge.hpp"

using namespace sme::ixmerge;

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

static InputDesc desc_of(char c) {
  InputDesc d{true, true, false, 0, 1};
  if (c == 'n') d.present = false;
  if (c == 'c') d.same_ctx = false;
  if (c == 'r') d.records_only = true;
  if (c == 'g') d.job = 1;
  if (c == 'k') d.K = 2;
  return d;
}
struct Res {
  int rc, bad;
  bool notimpl;
  std::string msg;
};
static Res run_validate(const std::string &spec, int ctx_k, int n_override = -1) {
  std::vector<InputDesc> v;
  for (char c : spec)
    if (c != ',') v.push_back(desc_of(c));
  auto p = exact(v);
  Res r;
  r.rc = validate(p.get(), n_override >= 0 ? n_override : (int)v.size(), ctx_k, &r.bad);
  r.notimpl = false;
  if (r.rc != M_OK) {
    char buf[160];
    r.notimpl = describe(r.rc, r.bad, buf, sizeof buf);
    r.msg = buf;
  }
  return r;
}

static uint64_t g_rng = 88172645463325252ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 11);
}

struct Lists {  // k ascending lists as exactly sized heap arrays
  std::vector<std::unique_ptr<int32_t[]>> dn, tf;
  std::vector<const int32_t *> pdn, ptf;
  std::vector<int64_t> len;
};
// strict: a docno at most once per list (posting lists); else duplicates inside a list too
static Lists make_lists(int k, int max_len, int span, bool strict, int32_t base) {
  Lists L;
  for (int s = 0; s < k; s++) {
    const int n = max_len ? (int)(rnd() % (uint32_t)(max_len + 1)) : 0;
    std::vector<int32_t> d, t;
    int32_t cur = base;
    for (int i = 0; i < n; i++) {
      cur += (int32_t)(rnd() % (uint32_t)span) + (strict ? 1 : 0);
      d.push_back(cur);
      t.push_back((int32_t)(rnd() % 9) + 1);
    }
    L.dn.push_back(exact(d));
    L.tf.push_back(exact(t));
    L.len.push_back(n);
  }
  for (int s = 0; s < k; s++) {
    L.pdn.push_back(L.dn[(size_t)s].get());
    L.ptf.push_back(L.tf[(size_t)s].get());
  }
  return L;
}

// the naive merge: every posting into a map by docno, tf summed
static std::vector<Posting> naive_merge(const Lists &L, int k) {
  std::map<int32_t, int64_t> m;
  for (int s = 0; s < k; s++)
    for (int64_t i = 0; i < L.len[(size_t)s]; i++) m[L.pdn[(size_t)s][i]] += L.ptf[(size_t)s][i];
  std::vector<Posting> o;
  for (auto &kv : m) o.push_back(Posting{kv.first, (int32_t)kv.second});
  return o;
}

struct ListFn {
  const Lists &L;
  void operator()(int s, const int32_t **p, int64_t *n) const {
    *p = L.pdn[(size_t)s];
    *n = L.len[(size_t)s];
  }
};

// every diagonal of the lists: the cuts hold exactly d elements (exact) or the
// elements below the diagonal's value (rounded), in (docno, list, place) order
static void check_diagonals(const Lists &L, int k) {
  struct E {
    int32_t dn;
    int s;
    int64_t i;
  };
  std::vector<E> all;
  for (int s = 0; s < k; s++)
    for (int64_t i = 0; i < L.len[(size_t)s]; i++) all.push_back(E{L.pdn[(size_t)s][i], s, i});
  std::stable_sort(all.begin(), all.end(), [](const E &a, const E &b) { return a.dn < b.dn; });
  for (int64_t d = 0; d < (int64_t)all.size(); d++) {
    int64_t before = -1;
    const int64_t v = diagonal_value(ListFn{L}, k, d, &before);
    CHECK(v == all[(size_t)d].dn);
    int64_t nb = 0;
    while (nb < (int64_t)all.size() && all[(size_t)nb].dn < v) nb++;
    CHECK(before == nb);
    // exact cuts: the first d elements of the stable order
    std::vector<int64_t> want((size_t)k, 0);
    for (int64_t x = 0; x < d; x++) want[(size_t)all[(size_t)x].s]++;
    int64_t eq_before = 0, total = 0, total_r = 0;
    for (int s = 0; s < k; s++) {
      const int32_t *p = L.pdn[(size_t)s];
      const int64_t n = L.len[(size_t)s];
      const int64_t c = cut_of(p, n, v, d - before, eq_before);
      CHECK(c == want[(size_t)s]);
      total += c;
      const int64_t cr = cut_of(p, n, v, 0, eq_before);
      CHECK(cr == lower_bound_i32(p, n, v));
      total_r += cr;
      eq_before += lower_bound_i32(p, n, v + 1) - lower_bound_i32(p, n, v);
    }
    CHECK(total == d);
    CHECK(total_r == before && before <= d && d - before < eq_before + 1);
  }
  for (int s = 0; s < k; s++) CHECK(cut_of(L.pdn[(size_t)s], L.len[(size_t)s], kNoValue, 0, 0) == 0);
}

static void builtin() {
  // ---- validator
  CHECK(run_validate("o", 1).rc == M_OK);
  CHECK(run_validate("o,o,o", 1).rc == M_OK);
  CHECK(run_validate("", 1).rc == M_COUNT);
  CHECK(run_validate(std::string(64, 'o'), 1).rc == M_OK);
  {
    Res r = run_validate(std::string(65, 'o'), 1);
    CHECK(r.rc == M_COUNT && r.bad == -1 && !r.notimpl && r.msg.find("64") != std::string::npos);
    r = run_validate("", 1, -3);  // n is checked before the (empty) array is read
    CHECK(r.rc == M_COUNT);
    r = run_validate("o,n,o", 1);
    CHECK(r.rc == M_NULL && r.bad == 1 && !r.notimpl && r.msg.find("input 1:") != std::string::npos);
    r = run_validate("o,o,c", 1);
    CHECK(r.rc == M_CONTEXT && r.bad == 2 && r.msg.find("input 2:") != std::string::npos);
    r = run_validate("r,o", 1);
    CHECK(r.rc == M_RECORDS && r.bad == 0 && r.msg.find("input 0:") != std::string::npos);
    r = run_validate("o,g", 1);
    CHECK(r.rc == M_CHARGRAM && r.bad == 1);
    r = run_validate("o,k,o", 1);
    CHECK(r.rc == M_KGRAM && r.bad == 1 && r.notimpl && r.msg.find("merging K >= 2 indexes") != std::string::npos);
    r = run_validate("o,o", 2);
    CHECK(r.rc == M_KGRAM && r.bad == -1 && r.notimpl);
    r = run_validate("k,n", 1);  // a malformed list is refused before K is looked at
    CHECK(r.rc == M_NULL && r.bad == 1);
  }
  CHECK(legal_tile(64) && legal_tile(1024) && legal_tile(2048) && !legal_tile(0) && !legal_tile(65) &&
        !legal_tile(2112) && !legal_tile(-64));

  // ---- lower_bound_i32 at the edges of an exactly sized array
  {
    auto a = exact(std::vector<int32_t>{INT32_MIN, -3, -3, 0, 7, INT32_MAX});
    CHECK(lower_bound_i32(a.get(), 6, (int64_t)INT32_MIN) == 0);
    CHECK(lower_bound_i32(a.get(), 6, -3) == 1 && lower_bound_i32(a.get(), 6, -2) == 3);
    CHECK(lower_bound_i32(a.get(), 6, (int64_t)INT32_MAX) == 5);
    CHECK(lower_bound_i32(a.get(), 6, (int64_t)INT32_MAX + 1) == 6);
    CHECK(lower_bound_i32(a.get(), 0, 5) == 0);
  }

  // ---- the merge of one term against the naive merge; every diagonal
  for (int round = 0; round < 300; round++) {
    const int k = 1 + (int)(rnd() % (round < 250 ? 5u : 64u));
    const int span = round % 3 == 0 ? 2 : 40;  // dense lists share many docnos
    const Lists L = make_lists(k, round % 7 == 0 ? 0 : 1 + (int)(rnd() % 90), span, true, round % 2 ? -50 : 0);
    std::vector<Posting> got;
    CHECK(merge_term(L.pdn.data(), L.ptf.data(), L.len.data(), k, &got));
    const std::vector<Posting> want = naive_merge(L, k);
    CHECK(got == want);
    // reduce order: stable by tf descending == sort by (tf desc, docno asc) of distinct docnos
    std::vector<Posting> ro = reduce_order(got), ws = want;
    std::sort(ws.begin(), ws.end(),
              [](const Posting &a, const Posting &b) { return a.tf != b.tf ? a.tf > b.tf : a.docno < b.docno; });
    CHECK(ro == ws);
    check_diagonals(L, k);
  }
  // record lists: equal docnos inside a list too (docno 0 of unmapped docids)
  for (int round = 0; round < 100; round++) {
    const int k = 1 + (int)(rnd() % 6);
    const Lists L = make_lists(k, 1 + (int)(rnd() % 70), 3, false, round % 2 ? -2 : 0);
    check_diagonals(L, k);
  }
  // a summed tf at the limit is refused, one below it is not
  {
    auto d0 = exact(std::vector<int32_t>{5}), d1 = exact(std::vector<int32_t>{5});
    auto t0 = exact(std::vector<int32_t>{(int32_t)(kTfLimit - 2)}), t1 = exact(std::vector<int32_t>{1});
    const int32_t *pd[2] = {d0.get(), d1.get()}, *pt[2] = {t0.get(), t1.get()};
    const int64_t len[2] = {1, 1};
    std::vector<Posting> got;
    CHECK(merge_term(pd, pt, len, 2, &got) && got.size() == 1 && got[0].tf == kTfLimit - 1);
    t1[0] = 2;
    CHECK(!merge_term(pd, pt, len, 2, &got));
  }
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "--validate")) {
    const Res r = run_validate(argv[3], atoi(argv[2]));
    printf("%d %d %d %s\n", r.rc, r.notimpl ? 1 : 0, r.bad, r.msg.c_str());
    return 0;
  }
  builtin();
  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
