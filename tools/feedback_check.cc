// feedback_check -- host check of csrc/sme_feedback.hpp, the validator of a batch of
// document sets with its messages and the one-set aggregation that
// csrc/sme_feedback.hip restates on the device.  Built with the address and
// undefined-behaviour sanitizers (make -C <package> feedback-check): a read past an
// array stops the program -- every array handed to the header is an exactly sized
// heap copy.
//
//   feedback_check                         built-in cases; prints "all passed"
//   feedback_check --validate V FOFF XOFF XIDS
//                                          "<rc> <limit 0/1> <set> <message>" for the
//                                          batch (comma-separated lists; XOFF "-" =
//                                          no exclusion lists)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "sme_feedback.hpp"

using namespace sme::feedback;

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
  int rc, set;
  bool limit;
  std::string msg;
};
// ndocnos: the size of the docno array the offsets index.  with_x: exclusion lists
// given.  declared: the sizes of the arrays are given; otherwise left to the offsets
static Res run(const std::vector<int64_t> &foff, int64_t ndocnos, bool with_x, const std::vector<int64_t> &xoff,
               const std::vector<int32_t> &xids, int64_t V, bool declared) {
  auto f = exact(foff), xo = exact(xoff);
  auto xi = exact(xids);
  Res r;
  r.rc = validate(f.get(), declared ? ndocnos : -1, (int)foff.size() - 1, with_x ? xi.get() : nullptr,
                  declared ? (int64_t)xids.size() : -1, with_x ? xo.get() : nullptr, V, &r.set);
  r.limit = false;
  if (r.rc != F_OK) {
    char buf[128];
    r.limit = describe(r.rc, r.set, buf, sizeof buf);
    r.msg = buf;
  }
  return r;
}
static Res run(const std::vector<int64_t> &foff, bool with_x = false, const std::vector<int64_t> &xoff = {},
               const std::vector<int32_t> &xids = {}, int64_t V = 10) {
  const int64_t nd = foff.empty() ? 0 : foff.back();
  const Res a = run(foff, nd, with_x, xoff, xids, V, true), b = run(foff, nd, with_x, xoff, xids, V, false);
  CHECK(a.rc == b.rc && a.set == b.set && a.msg == b.msg);
  return a;
}
static bool names(const Res &r, int set) { return r.msg.find("set " + std::to_string(set) + ":") != std::string::npos; }

static void validator_cases() {
  Res r = run({0, 2, 2, 5});
  CHECK(r.rc == F_OK && r.set == -1);
  int bad = 7;
  CHECK(validate(nullptr, -1, 0, nullptr, -1, nullptr, 10, &bad) == F_OK && bad == -1);  // no set: nothing is read
  CHECK(validate(nullptr, -1, -1, nullptr, -1, nullptr, 10, &bad) == F_OFFSETS);
  r = run({0, 0, 0});
  CHECK(r.rc == F_OK);
  // set offsets: not from 0, descending, past / short of the declared array
  r = run({1, 2});
  CHECK(r.rc == F_OFFSETS && !r.limit);
  r = run({0, 2, 1}, 2, false, {}, {}, 10, true);
  CHECK(r.rc == F_OFFSETS && r.set == 1 && names(r, 1));
  r = run({0, 2, 1}, 2, false, {}, {}, 10, false);
  CHECK(r.rc == F_OFFSETS && r.set == 1);
  r = run({0, 1, 4}, 2, false, {}, {}, 10, true);
  CHECK(r.rc == F_OFFSETS && r.set == 1);
  r = run({0, 1}, 2, false, {}, {}, 10, true);
  CHECK(r.rc == F_OFFSETS && r.set == -1);
  r = run({0, -1});
  CHECK(r.rc == F_OFFSETS && r.set == 0);
  // the entry limit: 1024 passes, 1025 is a limit, the set named
  r = run({0, 3, 3 + kMaxEntries});
  CHECK(r.rc == F_OK);
  r = run({0, 3, 4 + kMaxEntries});
  CHECK(r.rc == F_ENTRIES && r.set == 1 && r.limit && names(r, 1));
  // exclusion lists: ids -1 .. V - 1 pass; V and -2 do not, the set named
  r = run({0, 1, 2}, true, {0, 2, 3}, {-1, 9, 0});
  CHECK(r.rc == F_OK);
  r = run({0, 1, 2}, true, {0, 2, 3}, {-1, 9, 10});
  CHECK(r.rc == F_XTERM && r.set == 1 && !r.limit && names(r, 1));
  r = run({0, 1, 2}, true, {0, 2, 3}, {-2, 9, 0});
  CHECK(r.rc == F_XTERM && r.set == 0 && names(r, 0));
  r = run({0, 1}, true, {0, 1}, {0}, 0);  // an index without terms knows none
  CHECK(r.rc == F_XTERM);
  r = run({0, 1, 2}, true, {0, 0, 0}, {});
  CHECK(r.rc == F_OK);
  // exclusion offsets: not from 0, descending, past / short of the declared array
  r = run({0, 1}, true, {1, 2}, {0, 0});
  CHECK(r.rc == F_XOFFSETS && !r.limit);
  r = run({0, 1, 2}, 2, true, {0, 2, 1}, {0, 0}, 10, true);
  CHECK(r.rc == F_XOFFSETS && r.set == 1 && names(r, 1));
  r = run({0, 1, 2}, 2, true, {0, 1, 4}, {0, 0}, 10, true);
  CHECK(r.rc == F_XOFFSETS && r.set == 1);
  r = run({0, 1}, 1, true, {0, 1}, {0, 0}, 10, true);
  CHECK(r.rc == F_XOFFSETS && r.set == -1);
  // one pointer without the other
  {
    const int64_t f[2] = {0, 1}, x[2] = {0, 1};
    const int32_t ids[1] = {0};
    CHECK(validate(f, -1, 1, ids, -1, nullptr, 10, &bad) == F_XPOINTERS);
    CHECK(validate(f, -1, 1, nullptr, -1, x, 10, &bad) == F_XPOINTERS);
    const int64_t x0[2] = {0, 0};
    CHECK(validate(f, -1, 1, nullptr, -1, x0, 10, &bad) == F_OK);  // (offsets without an id need no array)
    char buf[128];
    CHECK(!describe(F_XPOINTERS, -1, buf, sizeof buf));
    CHECK(describe(F_SLOTS, -1, buf, sizeof buf));
  }
  // the table option
  CHECK(legal_slots(16) && legal_slots(4096) && legal_slots(256));
  CHECK(!legal_slots(8) && !legal_slots(8192) && !legal_slots(48) && !legal_slots(0) && !legal_slots(-16));
  CHECK(load_limit(16) == 12 && load_limit(4096) == 3072);
  CHECK(kMaxSlots * kSlotBytes * 2 + 4096 <= 160 * 1024);  // two workgroups fit a CU's LDS
}

struct Agg {
  std::vector<TermCount> terms;
  int64_t positions, missing;
};
// records: (docno, stream) in docno-ascending order
static Agg agg(const std::vector<std::pair<int32_t, std::vector<int32_t>>> &records, const std::vector<int32_t> &set) {
  std::vector<int64_t> off{0};
  std::vector<int32_t> terms, docno;
  for (const auto &r : records) {
    docno.push_back(r.first);
    terms.insert(terms.end(), r.second.begin(), r.second.end());
    off.push_back((int64_t)terms.size());
  }
  auto o = exact(off);
  auto t = exact(terms), d = exact(docno), s = exact(set);
  Agg a;
  a.terms = aggregate_set(s.get(), (int)set.size(), o.get(), t.get(), d.get(), (int64_t)docno.size(), &a.positions,
                          &a.missing);
  return a;
}
static bool is(const Agg &a, std::vector<TermCount> want) { return a.terms == want; }

static void aggregate_cases() {
  // docno -3 and 0 in two records each, an empty record, docnos 2, 5, 9
  const std::vector<std::pair<int32_t, std::vector<int32_t>>> R = {
      {-3, {7, 7}}, {-3, {8}}, {0, {1, 2}}, {0, {2, 2, 3}}, {2, {}}, {5, {1, 1, 1, 4}}, {9, {4, 7}}};
  Agg a = agg(R, {5});
  CHECK(is(a, {{1, 3, 1}, {4, 1, 1}}) && a.positions == 4 && a.missing == 0);
  a = agg(R, {0});  // both records of docno 0: freq sums, docs stays 1
  CHECK(is(a, {{1, 1, 1}, {2, 3, 1}, {3, 1, 1}}) && a.positions == 5);
  a = agg(R, {-3, 9});
  CHECK(is(a, {{4, 1, 1}, {7, 3, 2}, {8, 1, 1}}) && a.positions == 5);
  a = agg(R, {5, -1, 5, 9, 5, -1});  // pads and repeats count nothing
  CHECK(is(a, {{1, 3, 1}, {4, 2, 2}, {7, 1, 1}}) && a.positions == 6 && a.missing == 0);
  a = agg(R, {4, 5, 100, 4, -2, 1});  // absent docnos, one listed twice
  CHECK(is(a, {{1, 3, 1}, {4, 1, 1}}) && a.missing == 4);
  a = agg(R, {2});  // a record without a term: present, nothing counted
  CHECK(a.terms.empty() && a.positions == 0 && a.missing == 0);
  a = agg(R, {});
  CHECK(a.terms.empty() && a.positions == 0 && a.missing == 0);
  a = agg(R, {-1, -1});
  CHECK(a.terms.empty() && a.missing == 0);
  a = agg({}, {1, 2});  // an index without records
  CHECK(a.terms.empty() && a.missing == 2);
  a = agg(R, {-3, 0, 2, 5, 9});
  CHECK(is(a, {{1, 4, 2}, {2, 3, 1}, {3, 1, 1}, {4, 2, 2}, {7, 3, 2}, {8, 1, 1}}) && a.positions == 14);
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
  if (argc == 6 && !strcmp(argv[1], "--validate")) {
    const bool with_x = strcmp(argv[4], "-") != 0;
    const std::vector<int64_t> foff = parse_list<int64_t>(argv[3]);
    const Res r = run(foff, foff.empty() ? 0 : foff.back(), with_x, with_x ? parse_list<int64_t>(argv[4]) : std::vector<int64_t>{},
                      parse_list<int32_t>(argv[5]), atoll(argv[2]), true);
    printf("%d %d %d %s\n", r.rc, (int)r.limit, r.set, r.msg.c_str());
    return 0;
  }
  validator_cases();
  aggregate_cases();
  if (g_fail) {
    printf("%d check(s) FAILED\n", g_fail);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
