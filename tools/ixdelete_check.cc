// ixdelete_check -- host check of csrc/sme_ixdelete.hpp: the validator of a deletion
// call with its messages, the index arithmetic of the docno bitmap at the int32
// extremes, the task-start rule of the doc counter and the plain compaction of one
// term that csrc/sme_ixdelete.hip restates on the device.  Built with the address
// and undefined-behaviour sanitizers (make -C <package> ixdelete-check): a read
// past an array stops the program -- every array handed to the header is an
// exactly sized heap copy.
//
//   ixdelete_check                 built-in cases; prints "all passed"
//   ixdelete_check --validate SPEC N   "<rc> <notimpl 0/1> <message>" for a call with
//                                  n = N and the letters of SPEC: i no index, o no
//                                  result pointer, l no list, g chargram output,
//                                  r records-only, k K = 2, p opened from part files
//                                  ("-" = a plain legal call)
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <set>
#include <string>
#include <vector>

#include "sme_ixdelete.hpp"

using namespace sme::ixdelete;

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

struct Res {
  int rc;
  bool notimpl;
  std::string msg;
};
static Res run_validate(const std::string &spec, int64_t n) {
  CallDesc c{true, true, true, n, false, 0, 1, true};
  for (char ch : spec) {
    if (ch == 'i') c.has_index = false;
    if (ch == 'o') c.has_out = false;
    if (ch == 'l') c.has_list = false;
    if (ch == 'g') c.job = 1;
    if (ch == 'r') c.records_only = true;
    if (ch == 'k') c.K = 2;
    if (ch == 'p') c.rec_complete = false;
  }
  Res r{validate(c), false, ""};
  if (r.rc != D_OK) {
    char buf[200];
    r.notimpl = describe(r.rc, buf, sizeof buf);
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

// the rule as the header of the C interface words it: a surviving record starts a
// map task iff no survivor lies between it and the nearest task start at or before it
static std::vector<uint8_t> naive_starts(const std::vector<uint8_t> &first, const std::vector<uint8_t> &keep) {
  std::vector<uint8_t> out;
  for (size_t i = 0; i < keep.size(); i++) {
    if (!keep[i]) continue;
    size_t s = i;
    while (s > 0 && !first[s]) s--;  // record 0 starts a task whatever its flag
    bool survivor_between = false;
    for (size_t x = s; x < i; x++) survivor_between |= keep[x] != 0;
    out.push_back(survivor_between ? 0 : 1);
  }
  return out;
}

static void check_bitmap() {
  // the whole int32 range: 2^32 bits, indices in 64 bits (no array of that size is touched)
  const int64_t dmin = INT32_MIN, dmax = INT32_MAX, span = span_of(dmin, dmax);
  CHECK(span == (int64_t(1) << 32) && bitmap_words(span) == (int64_t(1) << 27));
  CHECK(bit_of(INT32_MIN, dmin, span) == 0 && bit_of(INT32_MAX, dmin, span) == span - 1);
  CHECK(bit_of(0, dmin, span) == (int64_t(1) << 31));
  CHECK(span_of(0, -1) == 0 && bitmap_words(0) == 0 && span_of(5, 5) == 1 && bitmap_words(1) == 1);
  CHECK(bitmap_words(32) == 1 && bitmap_words(33) == 2);
  // a range at each extreme: everything outside is -1, and the difference does not wrap
  {
    const int64_t lo = (int64_t)INT32_MAX - 40, sp = span_of(lo, INT32_MAX);
    CHECK(sp == 41 && bit_of(INT32_MAX, lo, sp) == 40 && bit_of(INT32_MIN, lo, sp) == -1 && bit_of(0, lo, sp) == -1);
    auto bm = exact(std::vector<uint32_t>((size_t)bitmap_words(sp), 0u));
    bitmap_set(bm.get(), INT32_MAX, lo, sp);
    bitmap_set(bm.get(), INT32_MIN, lo, sp);  // ignored
    bitmap_set(bm.get(), (int32_t)lo, lo, sp);
    CHECK(bm[0] == 1u && bm[1] == (1u << 8));
    CHECK(bitmap_test(bm.get(), INT32_MAX, lo, sp) && !bitmap_test(bm.get(), INT32_MAX - 1, lo, sp));
    CHECK(!bitmap_test(bm.get(), INT32_MIN, lo, sp) && !bitmap_test(bm.get(), (int32_t)lo - 1, lo, sp));
  }
  {
    const int64_t sp = span_of(INT32_MIN, (int64_t)INT32_MIN + 63);
    CHECK(sp == 64 && bit_of(INT32_MAX, INT32_MIN, sp) == -1 && bit_of(INT32_MIN + 63, INT32_MIN, sp) == 63);
    CHECK(bit_of(INT32_MIN + 64, INT32_MIN, sp) == -1);
    auto bm = exact(std::vector<uint32_t>((size_t)bitmap_words(sp), 0u));
    bitmap_set(bm.get(), INT32_MIN + 63, INT32_MIN, sp);
    bitmap_set(bm.get(), INT32_MAX, INT32_MIN, sp);  // ignored
    CHECK(bm[0] == 0u && bm[1] == (1u << 31) && bitmap_test(bm.get(), INT32_MIN + 63, INT32_MIN, sp));
  }
  // negative docnos, docno 0 and positive ones in one range; an empty range holds nothing
  {
    const int64_t lo = -7, sp = span_of(lo, 30);
    auto bm = exact(std::vector<uint32_t>((size_t)bitmap_words(sp), 0u));
    for (int32_t d : {-7, 0, 24, 25, 30, 31, -8, INT32_MIN, INT32_MAX}) bitmap_set(bm.get(), d, lo, sp);
    for (int32_t d = -20; d < 50; d++)
      CHECK(bitmap_test(bm.get(), d, lo, sp) == (d == -7 || d == 0 || d == 24 || d == 25 || d == 30));
    CHECK(!bitmap_test(nullptr, 0, 0, 0) && bit_of(0, 0, 0) == -1);
  }
}

static void check_task_starts() {
  // a task that loses its first record starts at its next survivor; one that loses
  // every record disappears; the first record of all may go
  {
    const std::vector<int32_t> dn{1, 2, 3, 4, 5, 6, 7, 8, 9};
    const std::vector<uint8_t> first{1, 0, 0, 1, 0, 1, 0, 0, 1}, keep{0, 1, 1, 0, 0, 0, 1, 1, 1};
    auto pd = exact(dn);
    auto pf = exact(first), pk = exact(keep);
    std::vector<int32_t> od;
    std::vector<uint8_t> of;
    compact_records(pd.get(), pf.get(), pk.get(), 9, &od, &of);
    CHECK((od == std::vector<int32_t>{2, 3, 7, 8, 9}));
    CHECK((of == std::vector<uint8_t>{1, 0, 1, 0, 1}));
    compact_records(pd.get(), nullptr, pk.get(), 9, &od, &of);  // one task
    CHECK((of == std::vector<uint8_t>{1, 0, 0, 0, 0}));
    compact_records(pd.get(), pf.get(), pk.get(), 0, &od, &of);
    CHECK(od.empty() && of.empty());
  }
  for (int round = 0; round < 400; round++) {
    const size_t n = rnd() % 40;
    std::vector<int32_t> dn(n);
    std::vector<uint8_t> first(n), keep(n);
    for (size_t i = 0; i < n; i++) {
      dn[i] = (int32_t)(rnd() % 9) - 2;
      first[i] = rnd() % (round % 4 + 2) == 0;  // (first[0] may be 0: record 0 starts a task all the same)
      keep[i] = round % 5 == 0 ? rnd() % 8 == 0 : rnd() % 3 != 0;
    }
    auto pd = exact(dn);
    auto pf = exact(first), pk = exact(keep);
    std::vector<int32_t> od, wd;
    std::vector<uint8_t> of;
    compact_records(pd.get(), pf.get(), pk.get(), (int64_t)n, &od, &of);
    for (size_t i = 0; i < n; i++)
      if (keep[i]) wd.push_back(dn[i]);
    CHECK(od == wd);
    CHECK(of == naive_starts(first, keep));
  }
}

static void check_compact_term() {
  for (int round = 0; round < 300; round++) {
    const int64_t dmin = round % 3 == 0 ? -5 : (round % 3 == 1 ? (int64_t)INT32_MAX - 200 : 1);
    const int64_t sp = span_of(dmin, dmin + 199);
    const size_t n = rnd() % 120, nl = rnd() % 60;
    std::set<int32_t> gone;
    auto bm = exact(std::vector<uint32_t>((size_t)bitmap_words(sp), 0u));
    for (size_t i = 0; i < nl; i++) {
      // in range mostly; some far outside, on either side
      const int32_t d = rnd() % 6 == 0 ? (rnd() % 2 ? INT32_MIN + (int32_t)(rnd() % 3) : (int32_t)(dmin - 1 - rnd() % 3))
                                       : (int32_t)(dmin + rnd() % 200);
      bitmap_set(bm.get(), d, dmin, sp);
      gone.insert(d);
    }
    std::vector<int32_t> dn(n), tf(n);
    for (size_t i = 0; i < n; i++) {  // either order of a term's postings: the order is kept, whatever it is
      dn[i] = (int32_t)(dmin + rnd() % 200);
      tf[i] = (int32_t)(rnd() % 9) + 1;
    }
    auto pd = exact(dn), pt = exact(tf);
    std::vector<Posting> got, want;
    compact_term(pd.get(), pt.get(), (int64_t)n, bm.get(), dmin, sp, &got);
    for (size_t i = 0; i < n; i++)
      if (!gone.count(dn[i])) want.push_back(Posting{dn[i], tf[i]});
    CHECK(got == want);
  }
}

static void builtin() {
  // ---- validator: the order of the refusals, the code of each, a word of each message
  CHECK(run_validate("", 0).rc == D_OK && run_validate("", 5).rc == D_OK);
  CHECK(run_validate("l", 0).rc == D_OK);  // n = 0 needs no list
  {
    Res r = run_validate("i", 1);
    CHECK(r.rc == D_NULL && !r.notimpl && r.msg.find("null") != std::string::npos);
    r = run_validate("o", 1);
    CHECK(r.rc == D_NULL && !r.notimpl);
    r = run_validate("", -1);
    CHECK(r.rc == D_COUNT && !r.notimpl && r.msg.find("negative") != std::string::npos);
    r = run_validate("l", 3);
    CHECK(r.rc == D_LIST && !r.notimpl && r.msg.find("null docno list") != std::string::npos);
    r = run_validate("r", 1);
    CHECK(r.rc == D_RECORDS && !r.notimpl && r.msg.find("records-only") != std::string::npos);
    r = run_validate("g", 1);
    CHECK(r.rc == D_CHARGRAM && !r.notimpl && r.msg.find("TermKGramDocIndexer") != std::string::npos);
    r = run_validate("k", 1);
    CHECK(r.rc == D_KGRAM && r.notimpl && r.msg.find("deleting from K >= 2 indexes") != std::string::npos);
    r = run_validate("p", 1);
    CHECK(r.rc == D_PARTFILES && !r.notimpl && r.msg.find("part files") != std::string::npos);
    r = run_validate("kp", 1);  // K is looked at first
    CHECK(r.rc == D_KGRAM);
    r = run_validate("ik", -1);  // nothing of a missing index is read
    CHECK(r.rc == D_NULL);
  }
  CHECK(legal_tile(256) && legal_tile(4096) && legal_tile(65536) && legal_tile(kDefaultTile) && !legal_tile(0) &&
        !legal_tile(64) && !legal_tile(300) && !legal_tile(65792) && !legal_tile(-256));
  check_bitmap();
  check_task_starts();
  check_compact_term();
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "--validate")) {
    const Res r = run_validate(!strcmp(argv[2], "-") ? "" : argv[2], atoll(argv[3]));
    printf("%d %d %s\n", r.rc, r.notimpl ? 1 : 0, r.msg.c_str());
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
