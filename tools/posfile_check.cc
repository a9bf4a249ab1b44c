// posfile_check -- host check of csrc/sme_posfile.hpp: the positions file's header
// validator with its codes and messages, the size arithmetic at the 2^31 and 2^64
// edges, the packing and unpacking of one tile (what csrc/sme_posfile.hip's encode
// and decode kernels do over their LDS copies) against a naive bit loop for every
// width, the vocabulary digest against constants, and the validator of a call.
// Built with the address and undefined-behaviour sanitizers (make -C <package>
// posfile-check): a read past an array stops the program -- every array handed to
// the header is an exactly sized heap copy.
//
//   posfile_check                  built-in cases; prints "all passed"
//   posfile_check --validate SPEC  "<rc> <limit 0/1> <message>" for the header of a
//                                  valid file (3 records, 5 positions, V = 3, 2 bits,
//                                  104 bytes) changed by the letters of SPEC: h cut to
//                                  10 bytes, m magic, v version 2, z a reserved byte,
//                                  b bits 1, B bits 32, r records 4, R records and N
//                                  2^31, V V 4, t positions 2^31, T positions 40, s one
//                                  byte more, S one byte less ("-" = unchanged)
//   posfile_check --call SPEC      "<rc> <message>" for a call on a K = 1 index of V =
//                                  300: a attaching (else writing, of an index with
//                                  positions), n a null argument, g chargram output, r
//                                  records-only, k K = 2, p positions the other way
//                                  round, b bits 8, w bits 20, x bits 32, f flags 2, c
//                                  flags 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "sme_posfile.hpp"

using namespace sme::posfile;

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

static bool has(const std::string &s, const char *w) { return s.find(w) != std::string::npos; }

struct Res {
  int rc;
  bool limit;
  std::string msg;
};
// the digest of {"apple", "berry", "café€"}: tests/test_posfile_ref.py has the same constants
constexpr uint64_t kDigest3 = 0xa9603576f19cd8fdull;

static Res run_header(const std::string &spec) {
  uint64_t N = 3, V = 3, n = 104;
  Header h{kVersion, 2, 3, 5, 3, kDigest3};
  std::vector<uint8_t> buf(kHeaderBytes);
  bool cut = false;
  for (char ch : spec) {
    if (ch == 'v') h.version = 2;
    if (ch == 'b') h.bits = 1;
    if (ch == 'B') h.bits = 32;
    if (ch == 'r') h.records = 4;
    if (ch == 'R') h.records = N = uint64_t(1) << 31;
    if (ch == 'V') h.V = 4;
    if (ch == 't') h.positions = uint64_t(1) << 31;
    if (ch == 'T') h.positions = 40;
    if (ch == 's') n++;
    if (ch == 'S') n--;
    if (ch == 'h') cut = true;
  }
  write_header(buf.data(), h);
  for (char ch : spec) {
    if (ch == 'm') buf[6] = 1;
    if (ch == 'z') buf[63] = 1;
  }
  if (cut) {
    n = 10;
    buf.resize(10);
  }
  auto p = exact(buf);
  Header got{};
  Layout lay{};
  Res r{validate_header(p.get(), n, N, V, &got, &lay), false, ""};
  if (r.rc != H_OK) {
    char msg[200];
    r.limit = describe_header(r.rc, got, n, N, V, msg, sizeof msg);
    r.msg = msg;
  }
  return r;
}

static Res run_call(const std::string &spec) {
  CallDesc c{false, true, 0, 1, false, true, 300, 0, 0};
  for (char ch : spec)
    if (ch == 'a') c.attach = true, c.has_positions = false;
  for (char ch : spec) {
    if (ch == 'n') c.has_args = false;
    if (ch == 'g') c.job = 1;
    if (ch == 'r') c.records_only = true;
    if (ch == 'k') c.K = 2;
    if (ch == 'p') c.has_positions = !c.has_positions;
    if (ch == 'b') c.bits = 8;
    if (ch == 'w') c.bits = 20;
    if (ch == 'x') c.bits = 32;
    if (ch == 'f') c.flags = 2;
    if (ch == 'c') c.flags = 1;
  }
  Res r{validate_call(c), false, ""};
  if (r.rc != C_OK) {
    char msg[200];
    describe_call(r.rc, c, msg, sizeof msg);
    r.msg = msg;
  }
  return r;
}

static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

// the format, bit by bit: bit i of the string is bit i mod 32 of 32-bit word i / 32
static std::vector<uint32_t> naive_pack(const std::vector<int32_t> &ids, int b, size_t nwords32) {
  std::vector<uint32_t> w(nwords32, 0);
  for (size_t p = 0; p < ids.size(); p++)
    for (int k = 0; k < b; k++)
      if (((uint32_t)ids[p] >> k) & 1u) {
        const size_t bit = p * (size_t)b + (size_t)k;
        w[bit >> 5] |= 1u << (bit & 31);
      }
  return w;
}

static void check_tiles() {
  for (int b = 1; b <= kMaxBits; b++)
    for (int n : {1, 63, 64, 65, kTile - 1, kTile}) {
      std::vector<int32_t> ids((size_t)kTile, 0);  // zeros past the tile's last position, as the kernel's LDS copy
      for (int p = 0; p < n; p++) ids[(size_t)p] = (int32_t)(rnd() & ((uint64_t(1) << b) - 1));
      ids[0] = (int32_t)((uint64_t(1) << b) - 1);  // every bit of the width
      const size_t nw = 2 * (((size_t)n * (size_t)b + 63) / 64);
      CHECK(n != kTile || nw == (size_t)(kTile / 32 * b));
      const std::vector<uint32_t> want = naive_pack(std::vector<int32_t>(ids.begin(), ids.begin() + n), b, nw);
      auto pi = exact(ids);
      std::vector<uint32_t> got(nw + 1, 0);  // one word after the last: id_of reads it
      for (size_t w = 0; w < nw; w++) got[w] = word32_of(pi.get(), b, (int)w);
      CHECK(std::vector<uint32_t>(got.begin(), got.begin() + (long)nw) == want);
      auto pw = exact(got);
      bool same = true;
      for (int p = 0; p < n; p++) same &= id_of(pw.get(), b, p) == (uint32_t)ids[(size_t)p];
      CHECK(same);
    }
}

static void check_layout() {
  Layout l{};
  CHECK(layout(0, 0, 1, &l) && l.size == 64 && l.nwords == 0 && l.words_at == 64);
  CHECK(layout(3, 5, 2, &l) && l.docno_at == 64 && l.len_at == 80 && l.words_at == 96 && l.nwords == 1 && l.size == 104);
  CHECK(layout(2, 64, 31, &l) && l.len_at == 72 && l.words_at == 80 && l.nwords == 31 && l.size == 80 + 31 * 8);
  CHECK(layout(1, 65, 1, &l) && l.nwords == 2);
  // the largest legal counts
  const uint64_t top = (uint64_t(1) << 31) - 1;
  CHECK(layout(top, top, 31, &l) && l.len_at == 64 + (uint64_t(1) << 33) && l.nwords == (top * 31 + 63) / 64 &&
        l.size == 64 + (uint64_t(2) << 33) + 8 * l.nwords);
  CHECK(layout(uint64_t(1) << 31, uint64_t(1) << 31, 31, &l));  // past the limits, still inside 64 bits
  // 2^64: each step that leaves 64 bits is seen
  CHECK(!layout(uint64_t(1) << 62, 0, 1, &l));            // 4 records
  CHECK(!layout((uint64_t(1) << 62) - 1, 0, 1, &l));      // 4 records + 7
  CHECK(!layout(~uint64_t(0), 0, 1, &l));
  CHECK(!layout(0, ~uint64_t(0), 2, &l));                 // positions * bits
  CHECK(!layout(0, uint64_t(1) << 60, 31, &l));           // positions * bits
  CHECK(layout(0, uint64_t(1) << 59, 31, &l) && l.nwords == uint64_t(31) << 53);  // 31 * 2^59 bits still fit
  CHECK(layout(0, ~uint64_t(0), 1, &l) && l.nwords == uint64_t(1) << 58 && l.size == 64 + (uint64_t(1) << 61));
  CHECK(!layout((uint64_t(1) << 61) - 2, uint64_t(1) << 63, 1, &l));  // header + docno + len
  CHECK(!layout((uint64_t(1) << 61) - (uint64_t(1) << 58), ~uint64_t(0), 1, &l));  // ... + words
  CHECK(layout((uint64_t(1) << 61) - (uint64_t(1) << 58) - 16, ~uint64_t(0), 1, &l) && l.size == ~uint64_t(0) - 63);
  CHECK(need_bits(0) == 1 && need_bits(1) == 1 && need_bits(2) == 1 && need_bits(3) == 2 && need_bits(4) == 2 &&
        need_bits(5) == 3 && need_bits(256) == 8 && need_bits(257) == 9 && need_bits(300) == 9 &&
        need_bits(uint64_t(1) << 31) == 31 && need_bits((uint64_t(1) << 31) + 1) == 32);
}

static uint64_t digest_of(const std::vector<std::vector<uint16_t>> &terms) {
  uint64_t sum = 0;
  for (size_t t = 0; t < terms.size(); t++) {
    auto p = exact(terms[t]);
    sum += term_hash((uint64_t)t, p.get(), (int64_t)terms[t].size());
  }
  return sum;
}
static std::vector<uint16_t> u16(const char *ascii) {
  std::vector<uint16_t> v;
  for (; *ascii; ascii++) v.push_back((uint16_t)(unsigned char)*ascii);
  return v;
}

static void check_digest() {
  // FNV-1a-64 by the book: h = basis; per byte h = (h ^ byte) * prime
  {
    uint64_t h = 0xcbf29ce484222325ull;
    for (int i = 0; i < 8; i++) h = (h ^ 0) * 0x100000001b3ull;
    h = (h ^ 0x61) * 0x100000001b3ull;
    h = (h ^ 0x00) * 0x100000001b3ull;
    CHECK(h == 0x6962e1cc2097a744ull);
  }
  CHECK(digest_of({}) == 0);
  CHECK(digest_of({u16("a")}) == 0x6962e1cc2097a744ull);
  std::vector<uint16_t> cafe = u16("caf");
  cafe.push_back(0x00E9);
  cafe.push_back(0x20AC);
  const auto apple = u16("apple"), berry = u16("berry");
  {
    auto p = exact(apple);
    CHECK(term_hash(0, p.get(), 5) == 0x7e1fe7371f310b95ull);
    auto q = exact(cafe);
    CHECK(term_hash(2, q.get(), 5) == 0xfef24425352306e6ull);
  }
  CHECK(digest_of({apple, berry, cafe}) == kDigest3);
  CHECK(digest_of({berry, apple, cafe}) == 0xd3ea7f7a6af6f91dull);  // t is hashed in: the order counts
  CHECK(digest_of({{}, {0xD83D, 0xDE00}}) == 0xd926a30c124dd904ull);   // the empty term, a surrogate pair
}

static void builtin() {
  // ---- header validator: the order of the refusals, the code of each, the field in each message
  CHECK(run_header("").rc == H_OK);
  struct {
    const char *spec;
    int rc;
    bool limit;
    const char *word;
  } cases[] = {{"h", H_SHORT, false, "header"},      {"m", H_MAGIC, false, "magic"},     {"v", H_VERSION, false, "version"},
               {"z", H_RESERVED, false, "reserved"}, {"b", H_BITS, false, "bits 1"},     {"B", H_BITS, false, "bits 32"},
               {"r", H_RECORDS, false, "records 4"}, {"R", H_RECORDS, false, "records"}, {"V", H_V, false, "V 4"},
               {"t", H_POSITIONS, true, "positions"}, {"T", H_SIZE, false, "size"},      {"s", H_SIZE, false, "size 105"},
               {"S", H_SIZE, false, "size 103"}};
  for (const auto &c : cases) {
    const Res r = run_header(c.spec);
    CHECK(r.rc == c.rc && r.limit == c.limit && has(r.msg, c.word) && has(r.msg, "positions file:"));
  }
  // the documented order: magic, version, reserved, bits, records, V, limits, size
  CHECK(run_header("mvzbrVts").rc == H_MAGIC && run_header("vzbrVts").rc == H_VERSION &&
        run_header("zbrVts").rc == H_RESERVED && run_header("brVts").rc == H_BITS && run_header("rVts").rc == H_RECORDS &&
        run_header("Vts").rc == H_V && run_header("ts").rc == H_POSITIONS && run_header("hm").rc == H_SHORT);
  {
    Layout l{};
    Header h{};
    std::vector<uint8_t> buf(kHeaderBytes);
    write_header(buf.data(), Header{kVersion, 2, 3, 5, 3, kDigest3});
    auto p = exact(buf);
    CHECK(validate_header(p.get(), 104, 3, 3, &h, &l) == H_OK && l.size == 104 && h.digest == kDigest3 && h.bits == 2 &&
          h.records == 3 && h.positions == 5 && h.V == 3);
    static const uint8_t lit[24] = {0x53, 0x4D, 0x45, 0x50, 0x4F, 0x53, 0, 1, 1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0};
    CHECK(memcmp(p.get(), lit, 24) == 0 && p[40] == 0xfd && p[47] == 0xa9);  // little-endian
  }
  // ---- call validator
  CHECK(run_call("").rc == C_OK && run_call("a").rc == C_OK && run_call("ac").rc == C_OK && run_call("w").rc == C_OK);
  struct {
    const char *spec;
    int rc;
    const char *word;
  } calls[] = {{"n", C_NULL, "null"},           {"an", C_NULL, "null"},        {"g", C_CHARGRAM, "TermKGramDocIndexer"},
               {"ag", C_CHARGRAM, "TermKGram"}, {"r", C_RECORDS, "no query"},  {"ar", C_RECORDS, "no query side"},
               {"k", C_KGRAM, "K != 1"},        {"ak", C_KGRAM, "k-grams"},    {"p", C_NOPOS, "keeps no positions"},
               {"ap", C_HASPOS, "already"},     {"b", C_BITS, "bits 8"},       {"x", C_BITS, "bits 32"},
               {"af", C_FLAGS, "flag"}};
  for (const auto &c : calls) {
    const Res r = run_call(c.spec);
    CHECK(r.rc == c.rc && has(r.msg, c.word) && has(r.msg, (c.spec[0] == 'a' ? "positions attach:" : "positions file:")));
  }
  CHECK(run_call("ngrkp").rc == C_NULL && run_call("grk").rc == C_CHARGRAM && run_call("kpb").rc == C_KGRAM &&
        run_call("pb").rc == C_NOPOS && run_call("apf").rc == C_HASPOS);
  check_layout();
  check_tiles();
  check_digest();
}

int main(int argc, char **argv) {
  if (argc == 3 && (!strcmp(argv[1], "--validate") || !strcmp(argv[1], "--call"))) {
    const std::string spec = !strcmp(argv[2], "-") ? "" : argv[2];
    if (!strcmp(argv[1], "--validate")) {
      const Res r = run_header(spec);
      printf("%d %d %s\n", r.rc, r.limit ? 1 : 0, r.msg.c_str());
    } else {
      const Res r = run_call(spec);
      printf("%d %s\n", r.rc, r.msg.c_str());
    }
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
