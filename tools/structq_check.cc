// structq_check -- host check of csrc/sme_structq.hpp, the validator of a structured
// query batch (queries -> groups -> leaves -> term ids) with its messages.  Built
// with the address and undefined-behaviour sanitizers (make -C <package>
// structq-check): a read past an array stops the program -- every array handed to
// the header is an exactly sized heap copy.
//
//   structq_check                   built-in cases; prints "all passed"
//   structq_check --validate V QOFF GOFF FLAGS LOFF KINDS WIDTHS TERMS
//                                   "<rc> <limit 0/1> <query> <message>" for the
//                                   batch (comma-separated lists, "" = empty), the
//                                   array sizes declared
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "sme_structq.hpp"

using namespace sme::structq;

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

typedef std::vector<int64_t> Offs;
typedef std::vector<int32_t> Ids;
typedef std::vector<uint8_t> Bytes;

struct Batch {
  Offs qoff, goff;
  Bytes flags;
  Offs loff;
  Bytes kinds;
  Ids widths, terms;
};
struct Res {
  int rc, query;
  bool limit;
  int64_t ops;
  std::string msg;
};
// declared: the sizes of the arrays are given; otherwise left to the offsets
static Res run(const Batch &b, int64_t V, bool declared) {
  auto q = exact(b.qoff), g = exact(b.goff), l = exact(b.loff);
  auto f = exact(b.flags), k = exact(b.kinds);
  auto w = exact(b.widths), t = exact(b.terms);
  Res r;
  r.rc = validate(t.get(), declared ? (int64_t)b.terms.size() : -1, l.get(),
                  declared ? (int64_t)b.loff.size() - 1 : -1, k.get(), w.get(), g.get(),
                  declared ? (int64_t)b.goff.size() - 1 : -1, f.get(), q.get(), (int)b.qoff.size() - 1, V, &r.query,
                  &r.ops);
  r.limit = false;
  if (r.rc != S_OK) {
    char buf[160];
    r.limit = describe(r.rc, r.query, buf, sizeof buf);
    r.msg = buf;
  }
  return r;
}
static Res run(const Batch &b, int64_t V) {
  const Res a = run(b, V, true), c = run(b, V, false);
  CHECK(a.rc == c.rc && a.query == c.query && a.msg == c.msg);
  return a;
}
static bool names(const Res &r, int query) {
  return r.msg.find("query " + std::to_string(query) + ":") != std::string::npos;
}

// query 0: (t3 | "t1 t2") -t4 ; query 1: empty ; query 2: #uw:5(t0 t1 -1) | #od:2()
static Batch good() {
  return Batch{{0, 2, 2, 3}, {0, 2, 3, 5}, {0, 1, 0}, {0, 1, 3, 4, 7, 7}, {0, 1, 0, 2, 1}, {0, 1, 0, 5, 2},
               {3, 1, 2, 4, 0, 1, -1}};
}

static void cases() {
  Res r = run(good(), 10);
  CHECK(r.rc == S_OK && r.query == -1 && r.ops == 3);
  // no query: nothing is read
  int bad = 7;
  int64_t ops = 7;
  CHECK(validate(nullptr, -1, nullptr, -1, nullptr, nullptr, nullptr, -1, nullptr, nullptr, 0, 10, &bad, &ops) == S_OK &&
        bad == -1 && ops == 0);
  CHECK(validate(nullptr, -1, nullptr, -1, nullptr, nullptr, nullptr, -1, nullptr, nullptr, -1, 10, &bad, &ops) ==
        S_OFFSETS);
  // only empty queries; only empty groups
  r = run(Batch{{0, 0, 0}, {0}, {}, {0}, {}, {}, {}}, 10);
  CHECK(r.rc == S_OK && r.ops == 0);
  r = run(Batch{{0, 2}, {0, 0, 0}, {0, 1}, {0}, {}, {}, {}}, 10);
  CHECK(r.rc == S_OK);
  // term ids: V and below -1, in a term leaf and in an operator leaf
  Batch b = good();
  b.terms[0] = 10;
  r = run(b, 10);
  CHECK(r.rc == S_TERM && r.query == 0 && !r.limit && names(r, 0));
  b = good();
  b.terms[6] = -2;
  r = run(b, 10);
  CHECK(r.rc == S_TERM && r.query == 2 && names(r, 2));
  // a term leaf with two ids, with none
  r = run(Batch{{0, 1}, {0, 1}, {0}, {0, 2}, {0}, {0}, {1, 2}}, 10);
  CHECK(r.rc == S_TERMLEAF && r.query == 0 && !r.limit && names(r, 0));
  r = run(Batch{{0, 1, 2}, {0, 1, 2}, {0, 0}, {0, 1, 1}, {0, 0}, {0, 0}, {1}}, 10);
  CHECK(r.rc == S_TERMLEAF && r.query == 1 && names(r, 1));
  // kind 3; widths 0 and -1 (read for operators only)
  b = good();
  b.kinds[3] = 3;
  r = run(b, 10);
  CHECK(r.rc == S_KIND && r.query == 2 && !r.limit && names(r, 2));
  b = good();
  b.widths[1] = 0;
  r = run(b, 10);
  CHECK(r.rc == S_WIDTH && r.query == 0 && !r.limit && names(r, 0));
  b = good();
  b.widths[4] = -1;
  r = run(b, 10);
  CHECK(r.rc == S_WIDTH && r.query == 2);
  b = good();
  b.widths[0] = b.widths[2] = -5;  // term leaves: not read
  CHECK(run(b, 10).rc == S_OK);
  // flags
  b = good();
  b.flags[2] = 2;
  r = run(b, 10);
  CHECK(r.rc == S_FLAG && r.query == 2 && !r.limit && names(r, 2));
  // an operator leaf of 32 ids passes, 33 are a limit
  for (int n : {32, 33}) {
    Batch o{{0, 1, 2}, {0, 1, 2}, {0, 0}, {0, 1, 1 + n}, {0, 2}, {0, 3}, Ids(1 + n, 4)};
    r = run(o, 10);
    if (n == 32)
      CHECK(r.rc == S_OK && r.ops == 1);
    else
      CHECK(r.rc == S_LENGTH && r.query == 1 && r.limit && names(r, 1));
  }
  // 64 groups pass, 65 are a limit; 1024 leaves pass, 1025 are a limit
  for (int n : {64, 65}) {
    Batch o{{0, 0, n}, Offs(n + 1, 0), Bytes(n, 0), {0}, {}, {}, {}};
    r = run(o, 10);
    if (n == 64)
      CHECK(r.rc == S_OK);
    else
      CHECK(r.rc == S_GROUPS && r.query == 1 && r.limit && names(r, 1));
  }
  for (int n : {1024, 1025}) {
    Batch o{{0, 1}, {0, n}, {0}, Offs(n + 1), Bytes(n, 0), Ids(n, 0), Ids(n, 1)};
    for (int i = 0; i <= n; i++) o.loff[i] = i;
    r = run(o, 10);
    if (n == 1024)
      CHECK(r.rc == S_OK);
    else
      CHECK(r.rc == S_LEAVES && r.query == 0 && r.limit && names(r, 0));
  }
  // offsets: not from 0, descending, past the declared array, disagreeing between
  // levels -- each level, and before any flag, kind or id is looked at
  b = good();
  b.qoff[0] = 1;
  CHECK(run(b, 10).rc == S_OFFSETS);
  b = good();
  b.qoff = {0, 2, 1, 3};
  r = run(b, 10);
  CHECK(r.rc == S_OFFSETS && r.query == 1 && !r.limit && names(r, 1));
  b = good();
  b.qoff[3] = 4;  // one group more than g_offsets / g_flags hold
  r = run(b, 10, true);
  CHECK(r.rc == S_OFFSETS && r.query == 2);
  b = good();
  b.qoff[3] = 2;  // one group fewer than the arrays hold
  r = run(b, 10, true);
  CHECK(r.rc == S_OFFSETS && r.query == -1);
  b = good();
  b.goff[0] = 1;
  CHECK(run(b, 10).rc == S_OFFSETS);
  b = good();
  b.goff = {0, 3, 2, 5};
  b.kinds = {9, 9, 9, 9, 9};
  r = run(b, 10);
  CHECK(r.rc == S_OFFSETS && r.query == 0 && names(r, 0));
  b = good();
  b.goff[3] = 6;  // one leaf more than l_offsets holds
  r = run(b, 10, true);
  CHECK(r.rc == S_OFFSETS && r.query == 2);
  b = good();
  b.goff[3] = 4;
  r = run(b, 10, true);
  CHECK(r.rc == S_OFFSETS && r.query == -1);
  b = good();
  b.loff[0] = 1;
  CHECK(run(b, 10).rc == S_OFFSETS);
  b = good();
  b.loff = {0, 1, 3, 2, 7, 7};
  b.terms = {99, 99, 99, 99, 99, 99, 99};
  r = run(b, 10);
  CHECK(r.rc == S_OFFSETS && r.query == 0 && names(r, 0));
  b = good();
  b.loff[4] = b.loff[5] = 8;  // one id more than term_ids holds
  r = run(b, 10, true);
  CHECK(r.rc == S_OFFSETS && r.query == 2);
  b = good();
  b.terms.push_back(1);  // one id fewer than the array holds
  r = run(b, 10, true);
  CHECK(r.rc == S_OFFSETS && r.query == -1);
  // 2^31 ids: refused from the offsets alone (no id, kind or width is read)
  {
    const int64_t q[2] = {0, 1}, g[2] = {0, 1}, l[2] = {0, int64_t(1) << 31};
    const uint8_t f[1] = {0};
    CHECK(validate(nullptr, -1, l, -1, nullptr, nullptr, g, -1, f, q, 1, 10, &bad, &ops) == S_SLOTS);
    char buf[160];
    CHECK(describe(S_SLOTS, -1, buf, sizeof buf));
  }
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
  if (argc == 10 && !strcmp(argv[1], "--validate")) {
    const Batch b{parse_list<int64_t>(argv[3]), parse_list<int64_t>(argv[4]), parse_list<uint8_t>(argv[5]),
                  parse_list<int64_t>(argv[6]), parse_list<uint8_t>(argv[7]), parse_list<int32_t>(argv[8]),
                  parse_list<int32_t>(argv[9])};
    const Res r = run(b, atoll(argv[2]), true);
    printf("%d %d %d %s\n", r.rc, (int)r.limit, r.query, r.msg.c_str());
    return 0;
  }
  cases();
  if (g_fail) {
    printf("%d check(s) FAILED\n", g_fail);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
