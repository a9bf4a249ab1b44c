// recparse_check -- host check of csrc/sme_recparse.hpp, the record parser the
// loader kernels (csrc/sme_load.hip) call.  Built with the address and undefined-
// behaviour sanitizers (make -C <package> recparse-check): a read past a buffer
// or an overflow in the parser's bounds checks stops the program.
//
// check_stream() is the loader's validation restated sequentially over exactly
// sized heap copies of the partitions: the record chain (header), then class
// name, key bytes, stored df, key order, keys in two partitions, the " " record,
// postings.  It is run over
//   - valid streams (with sync escapes, n = 0 records, 3-byte and C0 80 units),
//   - every malformed case the loader refuses, each expecting its code,
//   - every truncation of a small valid stream (none may pass as a longer one),
//   - the unaligned big-endian read at all four alignments.
// With --file PATH --expect CODE it checks a stream written by the tests
// (u32 nparts, (nparts + 1) x u64 offsets, bytes; little-endian).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "sme_recparse.hpp"

using namespace sme::rp;
typedef std::vector<uint8_t> Bytes;
typedef std::vector<std::pair<int32_t, int32_t>> Posts;

static void put32(Bytes &b, uint32_t v) {
  for (int i = 3; i >= 0; i--) b.push_back((uint8_t)(v >> (8 * i)));
}
static void put16(Bytes &b, uint32_t v) {
  b.push_back((uint8_t)(v >> 8));
  b.push_back((uint8_t)v);
}
static void puts_(Bytes &b, const std::string &s) { b.insert(b.end(), s.begin(), s.end()); }

struct RecOpt {
  int32_t df = 1;
  int32_t rec_len_add = 0, key_len_add = 0;
  std::string cls = "sa.edu.kaust.io.PostingWritable";
  std::vector<std::string> more;  // further key components (K >= 2)
};
static Bytes record(const std::string &term, const Posts &posts, const RecOpt &o = RecOpt()) {
  Bytes key, val;
  put32(key, 1 + (uint32_t)o.more.size());
  put16(key, (uint32_t)term.size());
  puts_(key, term);
  for (const auto &m : o.more) {
    put16(key, (uint32_t)m.size());
    puts_(key, m);
  }
  put32(key, (uint32_t)o.df);
  put32(val, (uint32_t)posts.size());
  if (!posts.empty()) {
    put16(val, (uint32_t)o.cls.size());
    puts_(val, o.cls);
    for (const auto &p : posts) {
      put32(val, (uint32_t)p.first);
      put32(val, (uint32_t)p.second);
    }
  }
  Bytes r;
  put32(r, (uint32_t)(key.size() + val.size()) + (uint32_t)o.rec_len_add);
  put32(r, (uint32_t)key.size() + (uint32_t)o.key_len_add);
  r.insert(r.end(), key.begin(), key.end());
  r.insert(r.end(), val.begin(), val.end());
  return r;
}
static Bytes space(const Posts &posts, int32_t df = -1) {
  RecOpt o;
  o.df = df < 0 ? (int32_t)posts.size() : df;
  return record(" ", posts, o);
}
static Bytes sync_escape() {
  Bytes b;
  put32(b, 0xFFFFFFFFu);
  for (int i = 0; i < 16; i++) b.push_back((uint8_t)(0xA0 + i));
  return b;
}
static Bytes cat(std::initializer_list<Bytes> l) {
  Bytes o;
  for (const auto &b : l) o.insert(o.end(), b.begin(), b.end());
  return o;
}

// The loader's checks in sequence; every partition is copied to a heap block of
// exactly its size so the sanitizer sees any read past it.
static int check_stream(const std::vector<Bytes> &parts) {
  std::map<std::vector<uint16_t>, int> seen;  // key -> partition
  int spaces = 0;
  size_t nrec = 0;
  for (size_t p = 0; p < parts.size(); p++) {
    const size_t end = parts[p].size();
    std::unique_ptr<uint8_t[]> heap(new uint8_t[end ? end : 1]);
    if (end) memcpy(heap.get(), parts[p].data(), end);
    const uint8_t *s = heap.get();
    std::vector<uint16_t> prev;
    bool have_prev = false;
    uint64_t at = 0;
    while (at < end) {
      Hdr h;
      const int c = header(s, at, end, true, &h);
      if (c == RP_SYNC) {
        at += (uint64_t)h.len;
        continue;
      }
      if (c != RP_OK) return c;
      {  // the byte-parallel pass must agree
        Hdr h2;
        if (header(s, at, end, false, &h2) != RP_OK || h2.len != h.len) return -1;
      }
      const int32_t nu = mutf8_decode(s + key_str_at(at), h.utf_len, nullptr);
      if (nu < 0) return RP_MUTF8;
      std::vector<uint16_t> u((size_t)nu);
      mutf8_decode(s + key_str_at(at), h.utf_len, u.data());
      if (h.n > 0 && !class_ok(s, at, h)) return RP_CLASS;
      const bool sp = h.utf_len == 1 && s[key_str_at(at)] == ' ';
      if ((int32_t)be32(s + df_at(at, h)) != (sp ? h.n : 1)) return RP_DF;
      if (sp && ++spaces > 1) return RP_SPACE_MANY;
      if (have_prev && cmp_units(prev.data(), (int64_t)prev.size(), u.data(), (int64_t)u.size()) >= 0) return RP_KEY_ORDER;
      if (seen.count(u)) return RP_KEY_DUP;
      seen[u] = (int)p;
      prev = u;
      have_prev = true;
      nrec++;
      const uint8_t *post = s + posts_at(at, h);
      if (sp) {
        if (h.n == 0) return RP_COUNTER;
        for (int64_t i = 0; i < h.n; i++) {
          const int cc = counter_check(i, (int32_t)be32(post + 8 * i), (int32_t)be32(post + 8 * i + 4));
          if (cc != RP_OK) return cc;
        }
      } else {
        std::map<int32_t, int> docs;
        for (int64_t i = 0; i < h.n; i++) {
          const int32_t dn = (int32_t)be32(post + 8 * i), tf = (int32_t)be32(post + 8 * i + 4);
          int cc = post_check(dn, tf);
          if (cc == RP_OK && i > 0)
            cc = post_pair_check((int32_t)be32(post + 8 * i - 8), (int32_t)be32(post + 8 * i - 4), dn, tf);
          if (cc != RP_OK) return cc;
          if (docs.count(dn)) return RP_DOCNO_DUP;
          docs[dn] = 1;
        }
      }
      at += (uint64_t)h.len;
    }
  }
  if (nrec > 0 && spaces == 0) return RP_SPACE_NONE;
  return RP_OK;
}

static int failures = 0;
static void expect(const char *name, const std::vector<Bytes> &parts, int want) {
  const int got = check_stream(parts);
  if (got != want) {
    printf("FAIL %-28s got %d (%s), want %d (%s)\n", name, got, got >= 0 ? message(got) : "passes disagree", want,
           message(want));
    failures++;
  } else {
    printf("ok   %-28s %s\n", name, want == RP_OK ? "valid" : message(want));
  }
}

static int run_file(const char *path, int want) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    perror(path);
    return 2;
  }
  Bytes all;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) all.insert(all.end(), buf, buf + n);
  fclose(f);
  if (all.size() < 4) return 2;
  uint32_t np;
  memcpy(&np, all.data(), 4);
  if (all.size() < 4 + 8 * ((size_t)np + 1)) return 2;
  std::vector<uint64_t> po((size_t)np + 1);
  memcpy(po.data(), all.data() + 4, 8 * ((size_t)np + 1));
  const uint8_t *body = all.data() + 4 + 8 * ((size_t)np + 1);
  const size_t nbody = all.size() - (4 + 8 * ((size_t)np + 1));
  std::vector<Bytes> parts;
  for (uint32_t p = 0; p < np; p++) {
    if (po[p + 1] < po[p] || po[p + 1] > nbody) return 2;
    parts.emplace_back(body + po[p], body + po[p + 1]);
  }
  expect(path, parts, want);
  return failures ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "--file") && !strcmp(argv[3], "--expect")) return run_file(argv[2], atoi(argv[4]));

  const Posts cnt = {{0, 0}, {7, 1}, {9, 1}};
  const Bytes sp = space(cnt);
  const Bytes a = record("apple", {{9, 3}, {7, 1}, {12, 1}});
  const Bytes b = record("berry", {});
  const Bytes c3 = record("caf\xC3\xA9\xE2\x82\xAC", {{7, 2}});  // 2- and 3-byte units
  const Bytes z0 = record("nul\xC0\x80z", {{12, 1}});            // C0 80 = U+0000
  const Bytes empty;

  // ---- valid streams
  expect("empty input", {}, RP_OK);
  expect("empty partitions", {empty, empty}, RP_OK);
  expect("one partition", {cat({sp, a, b, c3, z0})}, RP_OK);
  expect("sync escapes", {cat({sync_escape(), sp, sync_escape(), a, b, sync_escape()}), cat({c3, z0})}, RP_OK);
  expect("counter alone", {sp}, RP_OK);
  expect("three map tasks", {cat({space({{0, 0}, {5, 1}, {0, 0}, {0, 0}, {-3, 1}}), a})}, RP_OK);

  // ---- refused streams
  {
    Bytes t = cat({sp, a});
    t.resize(t.size() - 5);
    expect("truncated tail", {t}, RP_PAST_END);
    Bytes t2 = cat({sp, a});
    t2.push_back(0);
    t2.push_back(0);
    expect("stray tail bytes", {t2}, RP_TRUNC);
    Bytes t3 = cat({sp, sync_escape()});
    t3.resize(t3.size() - 1);
    expect("truncated sync escape", {t3}, RP_PAST_END);
  }
  {
    RecOpt o;
    o.rec_len_add = 4096;
    expect("recLen past the end", {cat({sp, record("apple", {{9, 3}}, o)})}, RP_PAST_END);
    Bytes neg = cat({sp, a});
    neg[sp.size()] = 0xFF;  // recLen = 0xFF.. < -1
    neg[sp.size() + 3] = 0xFE;
    expect("recLen < -1", {neg}, RP_RECLEN_NEG);
    RecOpt k;
    k.key_len_add = 1;
    expect("bad keyLen", {cat({sp, record("apple", {{9, 3}}, k)})}, RP_KEYLEN);
    RecOpt r;
    r.rec_len_add = 8;  // still inside the partition: b follows
    expect("recLen formula", {cat({sp, record("apple", {{9, 3}}, r), b})}, RP_RECLEN);
    Bytes nn = cat({sp, b});
    nn[nn.size() - 4] = 0x80;  // n < 0
    expect("n < 0", {nn}, RP_N_NEG);
  }
  {
    RecOpt o;
    o.cls = "sa.edu.kaust.io.PostingWritablf";
    expect("wrong class name", {cat({sp, record("apple", {{9, 3}}, o)})}, RP_CLASS);
    expect("bad UTF-8: lone continuation", {cat({sp, record("a\x80z", {{9, 1}})})}, RP_MUTF8);
    expect("bad UTF-8: cut 3-byte unit", {cat({sp, record("a\xE2\x82", {{9, 1}})})}, RP_MUTF8);
    expect("bad UTF-8: 4-byte lead", {cat({sp, record("a\xF0\x9F\x98\x80", {{9, 1}})})}, RP_MUTF8);
    expect("bad UTF-8: overlong", {cat({sp, record("a\xC1\x81", {{9, 1}})})}, RP_MUTF8);
    std::string z("a");
    z.push_back('\0');
    expect("bad UTF-8: raw NUL", {cat({sp, record(z, {{9, 1}})})}, RP_MUTF8);
  }
  expect("unsorted keys", {cat({sp, b, a})}, RP_KEY_ORDER);
  expect("equal neighbours", {cat({sp, a, a})}, RP_KEY_ORDER);
  expect("key in two partitions", {cat({sp, a}), cat({a, b})}, RP_KEY_DUP);
  {
    RecOpt o;
    o.df = 3;
    expect("df of a real term", {cat({sp, record("apple", {{9, 3}}, o)})}, RP_DF);
    expect("df of the counter", {space(cnt, 2)}, RP_DF);
  }
  expect("two counters", {cat({sp, a}), cat({sp, b})}, RP_SPACE_MANY);
  expect("no counter", {cat({a, b})}, RP_SPACE_NONE);
  expect("tf <= 0", {cat({sp, record("apple", {{9, 3}, {7, 0}})})}, RP_TF);
  expect("tf limit", {cat({sp, record("apple", {{9, 1 << 24}})})}, RP_TF_LIMIT);
  expect("tf order", {cat({sp, record("apple", {{9, 1}, {7, 3}})})}, RP_POST_ORDER);
  expect("docno order", {cat({sp, record("apple", {{9, 2}, {7, 2}})})}, RP_POST_ORDER);
  expect("duplicate docno", {cat({sp, record("apple", {{9, 2}, {9, 2}})})}, RP_DOCNO_DUP);
  expect("duplicate docno, other tf", {cat({sp, record("apple", {{9, 3}, {7, 1}, {9, 1}})})}, RP_DOCNO_DUP);
  expect("counter form", {space({{0, 0}, {7, 2}})}, RP_COUNTER);
  expect("counter start", {space({{7, 1}, {9, 1}})}, RP_COUNTER);
  {
    RecOpt o;
    o.more = {"pie"};
    expect("K = 2 key", {cat({sp, record("apple", {{9, 1}}, o)})}, RP_KGRAM);
  }

  // ---- every truncation of a small valid stream: no cut may read past the copy,
  // and only cuts on a record boundary may pass
  {
    const std::vector<Bytes> recs = {sp, sync_escape(), a, b, c3, z0};
    Bytes whole;
    std::vector<size_t> bounds = {0};
    for (const auto &r : recs) {
      whole.insert(whole.end(), r.begin(), r.end());
      bounds.push_back(whole.size());
    }
    int bad = 0;
    for (size_t cut = 0; cut <= whole.size(); cut++) {
      const Bytes t(whole.begin(), whole.begin() + cut);
      const int got = check_stream({t});
      bool boundary = false;
      for (size_t x : bounds) boundary |= x == cut;
      if ((got == RP_OK) != boundary) bad++;
      // the candidate pass over every byte of the cut stream
      std::unique_ptr<uint8_t[]> heap(new uint8_t[cut ? cut : 1]);
      if (cut) memcpy(heap.get(), t.data(), cut);
      for (size_t at = 0; at < cut; at++) {
        Hdr h;
        const int c = header(heap.get(), at, cut, false, &h);
        if ((c == RP_OK || c == RP_SYNC) && at + (uint64_t)h.len > cut) bad++;
      }
    }
    printf("%s every truncation (%zu cuts)\n", bad ? "FAIL" : "ok  ", whole.size() + 1);
    failures += bad;
  }

  // ---- unaligned big-endian words from aligned dwords
  {
    int bad = 0;
    alignas(4) uint8_t m[16];
    for (int i = 0; i < 16; i++) m[i] = (uint8_t)(0x11 * (i + 1) + 3);
    for (int a = 0; a < 4; a++) {
      uint32_t lo, hi;
      memcpy(&lo, m + 4, 4);
      memcpy(&hi, m + 8, 4);
      if (be32_unaligned(lo, hi, a) != be32(m + 4 + a)) bad++;
    }
    printf("%s unaligned big-endian reads\n", bad ? "FAIL" : "ok  ");
    failures += bad;
  }
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
