// near_check -- host check of csrc/sme_near.hpp, the validator of a proximity batch
// with its messages and the one-record ordered-window and unordered-window counts
// that csrc/sme_near.hip evaluates on the device.  Built with the address and
// undefined-behaviour sanitizers (make -C <package> near-check): a read past an
// array stops the program -- every array handed to the header is an exactly sized
// heap copy.
//
//   near_check                                 built-in cases; prints "all passed"
//   near_check --count KIND N TERMS STREAM     the count of the query in the stream
//                                              (KIND 0 ordered, 1 unordered; comma-
//                                              separated lists of ids, "" = empty);
//                                              N may be a list: one count per width
//   near_check --validate V OFFS TERMS WIDTHS KINDS
//                                              "<rc> <limit 0/1> <query> <message>"
//                                              for the batch (comma-separated lists)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "sme_near.hpp"

using namespace sme::near;

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

typedef std::vector<int32_t> Ids;
constexpr int32_t kMaxN = 2147483647;

static int64_t od(const Ids &ts, const Ids &q, int32_t N) {
  auto t = exact(ts), p = exact(q);
  return count_ordered(t.get(), (int64_t)ts.size(), p.get(), (int)q.size(), N);
}
static int64_t uw(const Ids &ts, const Ids &q, int32_t N) {
  auto t = exact(ts), p = exact(q);
  return count_unordered(t.get(), (int64_t)ts.size(), p.get(), (int)q.size(), N);
}

struct Res {
  int rc, query;
  bool limit;
  std::string msg;
};
// declared: the size of term_ids is given; otherwise left to the offsets
static Res run(const std::vector<int64_t> &off, const Ids &term, const Ids &width, const std::vector<uint8_t> &kind,
               int64_t V, bool declared) {
  auto o = exact(off);
  auto t = exact(term);
  auto w = exact(width);
  auto k = exact(kind);
  Res r;
  r.rc = validate(t.get(), declared ? (int64_t)term.size() : -1, o.get(), w.get(), k.get(), (int)off.size() - 1, V,
                  &r.query);
  r.limit = false;
  if (r.rc != N_OK) {
    char buf[128];
    r.limit = describe(r.rc, r.query, buf, sizeof buf);
    r.msg = buf;
  }
  return r;
}
static Res run(const std::vector<int64_t> &off, const Ids &term, const Ids &width, const std::vector<uint8_t> &kind,
               int64_t V) {
  const Res a = run(off, term, width, kind, V, true), b = run(off, term, width, kind, V, false);
  CHECK(a.rc == b.rc && a.query == b.query && a.msg == b.msg);
  return a;
}
static bool names(const Res &r, int query) {
  return r.msg.find("query " + std::to_string(query) + ":") != std::string::npos;
}

static void validator_cases() {
  Res r = run({0, 2, 2, 5}, {0, 1, 2, -1, 9}, {1, 5, kMaxN}, {0, 1, 1}, 10);
  CHECK(r.rc == N_OK && r.query == -1);
  // no query: nothing is read
  int bad = 7;
  CHECK(validate(nullptr, -1, nullptr, nullptr, nullptr, 0, 10, &bad) == N_OK && bad == -1);
  CHECK(validate(nullptr, -1, nullptr, nullptr, nullptr, -1, 10, &bad) == N_OFFSETS);
  // only empty queries, and an empty term array
  r = run({0, 0, 0}, {}, {1, 1}, {0, 1}, 10);
  CHECK(r.rc == N_OK);
  // a term id of V and one below -1: malformed, the query named
  r = run({0, 2, 3}, {0, 1, 10}, {1, 1}, {0, 0}, 10);
  CHECK(r.rc == N_TERM && r.query == 1 && !r.limit && names(r, 1));
  r = run({0, 2, 3}, {0, -2, 3}, {1, 1}, {0, 0}, 10);
  CHECK(r.rc == N_TERM && r.query == 0 && !r.limit && names(r, 0));
  r = run({0, 1}, {-1}, {1}, {1}, 0);
  CHECK(r.rc == N_OK);
  // widths 0 and -1, kind 2: malformed, the query named
  r = run({0, 1, 2}, {0, 1}, {3, 0}, {0, 0}, 10);
  CHECK(r.rc == N_WIDTH && r.query == 1 && !r.limit && names(r, 1));
  r = run({0, 1, 2}, {0, 1}, {-1, 3}, {1, 1}, 10);
  CHECK(r.rc == N_WIDTH && r.query == 0 && !r.limit && names(r, 0));
  r = run({0, 1, 2, 2}, {0, 1}, {1, 1, 1}, {0, 1, 2}, 10);
  CHECK(r.rc == N_KIND && r.query == 2 && !r.limit && names(r, 2));
  // the length limit: 32 passes, 33 is a limit, the query named
  Ids t32(32, 3), t33(33, 3), t35(35, 3);
  r = run({0, 32}, t32, {1}, {0}, 10);
  CHECK(r.rc == N_OK);
  r = run({0, 33}, t33, {1}, {1}, 10);
  CHECK(r.rc == N_LENGTH && r.query == 0 && r.limit && names(r, 0));
  r = run({0, 1, 2, 35}, t35, {1, 1, 1}, {0, 0, 0}, 10);
  CHECK(r.rc == N_LENGTH && r.query == 2 && r.limit && names(r, 2));
  // the length is tested before the ids, the width and the kind of that query
  t33[5] = 99;
  r = run({0, 33}, t33, {0}, {2}, 10);
  CHECK(r.rc == N_LENGTH);
  // offsets: not from 0, descending, past the declared array, short of it -- and
  // tested before any width or kind
  r = run({1, 2}, {0, 1}, {1}, {0}, 10);
  CHECK(r.rc == N_OFFSETS && !r.limit);
  r = run({0, 2, 1}, {0, 1}, {0, 0}, {2, 2}, 10, true);
  CHECK(r.rc == N_OFFSETS && r.query == 1 && names(r, 1));
  r = run({0, 2, 1}, {0, 1}, {1, 1}, {0, 0}, 10, false);
  CHECK(r.rc == N_OFFSETS && r.query == 1);
  r = run({0, 1, 4}, {0, 1}, {1, 1}, {0, 0}, 10, true);  // (declared only: implied sizes trust the last offset)
  CHECK(r.rc == N_OFFSETS && r.query == 1);
  r = run({0, 1}, {0, 1}, {1}, {0}, 10, true);
  CHECK(r.rc == N_OFFSETS && r.query == -1);
  r = run({0, -1}, {}, {1}, {0}, 10);
  CHECK(r.rc == N_OFFSETS && r.query == 0);
  // 2^31 term slots: refused from the offsets alone (nothing else is read)
  {
    const int64_t off[2] = {0, int64_t(1) << 31};
    CHECK(validate(nullptr, -1, off, nullptr, nullptr, 1, 10, &bad) == N_SLOTS);
    char buf[128];
    CHECK(describe(N_SLOTS, -1, buf, sizeof buf));
  }
}

static void ordered_cases() {
  const int32_t a = 1, b = 2, c = 3, x = 9;
  // chain existence, not a greedy match
  CHECK(od({a, b, b, x, c}, {a, b, c}, 2) == 1);  // through the second b
  CHECK(od({a, b, c, b}, {a, b, c}, 3) == 1);     // through the first b
  CHECK(od({a, b, b, x, c}, {a, b, c}, 1) == 0);
  // a gap of exactly N and of N + 1
  CHECK(od({a, x, x, b}, {a, b}, 3) == 1 && od({a, x, x, b}, {a, b}, 2) == 0);
  // distinct END positions: two starts, one end; one start, two ends
  CHECK(od({a, a, b}, {a, b}, 2) == 1 && od({a, b, b}, {a, b}, 2) == 2 && od({a, b, b}, {a, b}, 1) == 1);
  // repeated terms
  CHECK(od({a, x, a, a}, {a, a}, 2) == 2 && od({a, x, a, a}, {a, a}, 1) == 1 && od({a}, {a, a}, 5) == 0);
  // order matters
  CHECK(od({b, a}, {a, b}, 5) == 0);
  // L = 1: the term's count; L = 0 and an empty stream: nothing
  CHECK(od({a, x, a}, {a}, 1) == 2 && od({a, x, a}, {a}, kMaxN) == 2 && od({a}, {}, 1) == 0 && od({}, {a}, 1) == 0);
  // the largest width does not wrap
  Ids far(131, x);
  far[1] = a;
  far[130] = b;
  CHECK(od(far, {a, b}, kMaxN) == 1 && od(far, {a, b}, 129) == 1 && od(far, {a, b}, 128) == 0);
  // N = 1 is the phrase count
  CHECK(od({5, 5, 5}, {5, 5}, 1) == sme::phrase::phrase_count(exact<int32_t>({5, 5, 5}).get(), 3,
                                                               exact<int32_t>({5, 5}).get(), 2));
  Ids ph, s;
  for (int j = 0; j < 32; j++) ph.push_back(100 + j);
  s = ph;
  s.insert(s.end(), ph.begin(), ph.end());
  CHECK(od(s, ph, 1) == 2 && od(Ids(s.begin() + 1, s.end()), ph, 1) == 1);
}

static void unordered_cases() {
  const int32_t a = 1, b = 2, c = 3, x = 9;
  CHECK(uw({a, x, b}, {a, b}, 3) == 1 && uw({a, x, b}, {b, a}, 3) == 1 && uw({a, x, b}, {a, b}, 2) == 0);
  // every end on a query term counts
  CHECK(uw({a, b, a}, {a, b}, 2) == 2 && uw({a, b, x, a}, {a, b}, 2) == 1 && uw({a, b, x, a}, {a, b}, 3) == 2);
  // a term listed twice is the set
  CHECK(uw({a, x, b}, {a, b, a}, 3) == 1 && uw({a, a}, {a, a}, 1) == 2);
  // N below |T| matches nothing; clipped at the stream's start
  CHECK(uw({a, b, c}, {a, b, c}, 2) == 0 && uw({a, b, c}, {a, b, c}, 3) == 1);
  CHECK(uw({a, b}, {a, b}, 100) == 1 && uw({a, b}, {a, b}, kMaxN) == 1);
  // L = 1: the term's count; nothing from nothing
  CHECK(uw({a, x, a}, {a}, 1) == 2 && uw({a}, {}, 1) == 0 && uw({}, {a}, 1) == 0);
  // 32 distinct terms in one window of 32
  Ids q, s;
  for (int j = 0; j < 32; j++) q.push_back(100 + j);
  s = q;
  s.push_back(100);
  CHECK(uw(s, q, 32) == 2 && uw(s, q, 31) == 0 && uw(Ids(s.begin(), s.end() - 2), q, 32) == 0);
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
  if (argc == 6 && !strcmp(argv[1], "--count")) {
    const Ids q = parse_list<int32_t>(argv[4]), ts = parse_list<int32_t>(argv[5]);
    for (int32_t N : parse_list<int32_t>(argv[3]))
      printf("%lld\n", (long long)(atoi(argv[2]) == kOrdered ? od(ts, q, N) : uw(ts, q, N)));
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "--validate")) {
    const Res r = run(parse_list<int64_t>(argv[3]), parse_list<int32_t>(argv[4]), parse_list<int32_t>(argv[5]),
                      parse_list<uint8_t>(argv[6]), atoll(argv[2]), true);
    printf("%d %d %d %s\n", r.rc, (int)r.limit, r.query, r.msg.c_str());
    return 0;
  }
  validator_cases();
  ordered_cases();
  unordered_cases();
  if (g_fail) {
    printf("%d check(s) FAILED\n", g_fail);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
