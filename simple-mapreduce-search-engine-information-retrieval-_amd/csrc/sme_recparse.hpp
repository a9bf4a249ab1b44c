// sme_recparse.hpp -- field decoding of the reduce output's record stream, with
// its bounds checks, shared by the loader kernels (sme_load.hip) and the
// stand-alone host check (tools/recparse_check.cc).  No HIP header is needed: a
// host compiler sees plain inline functions.
//
//   record   int32 recLen, int32 keyLen, TermDF bytes, ArrayListWritable bytes (big-endian)
//   key      int32 k, k x writeUTF, int32 df                       TermDF.java:50-56
//   value    int32 n, [writeUTF(class name), n x (int32 docno, int32 tf)]
//            ArrayListWritable.java:90-105, PostingWritable.java:46-49
//   escape   where a record would start: int32 -1, 16 sync bytes   SequenceFile.Writer.checkAndWriteSync
//
// Every function reads only bytes it has first shown to lie inside [0, end).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SME_RP_HD __host__ __device__ __forceinline__
#else
#define SME_RP_HD inline
#endif

namespace sme {
namespace rp {

enum {
  RP_OK = 0,
  RP_SYNC = 1,         // a sync escape (20 bytes)
  RP_TRUNC = 2,        // fewer than 8 header bytes left in the partition
  RP_RECLEN_NEG = 3,   // recLen < -1
  RP_PAST_END = 4,     // the record or escape runs past its partition's end
  RP_KEYLEN = 5,       // keyLen inconsistent with the key's own fields
  RP_KGRAM = 6,        // a well-formed key of k != 1 components (K >= 2 streams: not loaded)
  RP_N_NEG = 7,        // posting count < 0
  RP_RECLEN = 8,       // recLen != keyLen + 4 + (n > 0 ? 2 + 31 + 8 n : 0)
  RP_CLASS = 9,        // value class name is not PostingWritable's
  RP_MUTF8 = 10,       // key string is not modified UTF-8 as writeUTF writes it
  RP_KEY_ORDER = 11,   // keys of a partition not strictly ascending (TermDF.compareTo)
  RP_KEY_DUP = 12,     // the same key in two partitions
  RP_DF = 13,          // stored df: 1 for a real term, the posting count for " "
  RP_SPACE_MANY = 14,  // more than one " " record
  RP_SPACE_NONE = 15,  // real terms but no " " record
  RP_TF = 16,          // a real term's posting with tf <= 0
  RP_TF_LIMIT = 17,    // tf >= 2^24
  RP_POST_ORDER = 18,  // postings not in (tf desc, docno asc) order
  RP_DOCNO_DUP = 19,   // a docno repeated within a term
  RP_COUNTER = 20,     // " " postings not the mapper's (0,0) / (docno,1) lists
};

constexpr int kClassLen = 31;
constexpr int kSyncLen = 20;            // int32 -1 + 16 sync bytes
constexpr int32_t kMaxTf = (1 << 24) - 1;  // as the reference tie word holds (sme_query.hip)

SME_RP_HD const char *class_name() { return "sa.edu.kaust.io.PostingWritable"; }

SME_RP_HD uint32_t be32(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
SME_RP_HD uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | (uint32_t)p[1]; }

// The big-endian int32 whose first byte is byte `a` (0..3) of the aligned
// little-endian dword lo; hi is the next aligned dword (unused when a == 0).
SME_RP_HD uint32_t be32_unaligned(uint32_t lo, uint32_t hi, int a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bswap32(a == 0 ? lo : __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)a));
#else
  const uint32_t v = a == 0 ? lo : (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * a));
  return ((v & 0xFFu) << 24) | ((v & 0xFF00u) << 8) | ((v >> 8) & 0xFF00u) | (v >> 24);
#endif
}

struct Hdr {
  int64_t len;     // framed bytes: 8 + recLen, or 20 for an escape
  int32_t key_len;  // TermDF bytes
  int32_t utf_len;  // writeUTF body bytes of the one component
  int32_t n;       // postings
};

// Key fields of a key of k components against key_len: 4 + sum(2 + len) + 4
// (k <= 255: the walk is one thread's, and no k-gram index is that wide).
SME_RP_HD bool key_fields_ok(const uint8_t *s, uint64_t at, int32_t key_len, int32_t k) {
  if (k < 0 || k > 255 || (int64_t)k * 2 + 8 > (int64_t)key_len) return false;
  int64_t q = 4;
  for (int32_t j = 0; j < k; j++) {
    if (q + 2 > (int64_t)key_len - 4) return false;
    q += 2 + (int64_t)be16(s + at + 8 + q);
  }
  return q + 4 == (int64_t)key_len;
}

// What starts at byte `at` of a partition ending at `end` (at <= end; at == end
// is the caller's "no more records").  RP_OK fills every field of *h, RP_SYNC
// h->len.  diagnose: a key of k != 1 components is walked to tell RP_KGRAM from
// RP_KEYLEN; the byte-parallel candidate pass only needs "not a K = 1 record".
SME_RP_HD int header(const uint8_t *s, uint64_t at, uint64_t end, bool diagnose, Hdr *h) {
  const uint64_t left = end - at;
  if (left < 4) return RP_TRUNC;
  const int32_t rec_len = (int32_t)be32(s + at);
  if (rec_len == -1) {
    if (left < (uint64_t)kSyncLen) return RP_PAST_END;
    h->len = kSyncLen;
    return RP_SYNC;
  }
  if (rec_len < -1) return RP_RECLEN_NEG;
  if (left < 8) return RP_TRUNC;
  if ((uint64_t)rec_len + 8 > left) return RP_PAST_END;
  const int32_t key_len = (int32_t)be32(s + at + 4);
  // the key and the value's count field lie inside the record
  if (key_len < 8 || (int64_t)key_len + 4 > (int64_t)rec_len) return RP_KEYLEN;
  const int32_t k = (int32_t)be32(s + at + 8);
  if (k != 1) return diagnose && key_fields_ok(s, at, key_len, k) ? RP_KGRAM : RP_KEYLEN;
  if (key_len < 10) return RP_KEYLEN;
  const int32_t utf_len = (int32_t)be16(s + at + 12);
  if (key_len != 10 + utf_len) return RP_KEYLEN;
  const int32_t n = (int32_t)be32(s + at + 8 + (uint64_t)key_len);
  if (n < 0) return RP_N_NEG;
  if ((int64_t)rec_len != (int64_t)key_len + 4 + (n > 0 ? 2 + kClassLen + 8 * (int64_t)n : 0)) return RP_RECLEN;
  h->len = 8 + (int64_t)rec_len;
  h->key_len = key_len;
  h->utf_len = utf_len;
  h->n = n;
  return RP_OK;
}

// byte offsets inside a K = 1 record (h from header())
SME_RP_HD uint64_t key_str_at(uint64_t at) { return at + 14; }
SME_RP_HD uint64_t df_at(uint64_t at, const Hdr &h) { return at + 8 + (uint64_t)h.key_len - 4; }
SME_RP_HD uint64_t class_at(uint64_t at, const Hdr &h) { return at + 8 + (uint64_t)h.key_len + 4; }
SME_RP_HD uint64_t posts_at(uint64_t at, const Hdr &h) { return class_at(at, h) + 2 + kClassLen; }

// writeUTF(class name) of a record with n > 0
SME_RP_HD bool class_ok(const uint8_t *s, uint64_t at, const Hdr &h) {
  const uint8_t *c = s + class_at(at, h);
  if (c[0] != 0 || c[1] != (uint8_t)kClassLen) return false;
  const char *nm = class_name();
  for (int i = 0; i < kClassLen; i++)
    if (c[2 + i] != (uint8_t)nm[i]) return false;
  return true;
}

// One UTF-16 unit of a writeUTF body b[0, len) at *i (advanced).  Only the
// forms DataOutputStream.writeUTF writes are taken: 1..0x7F one byte, 0 and
// 0x80..0x7FF two, 0x800.. three; anything else cannot be written back as it was.
SME_RP_HD bool mutf8_unit(const uint8_t *b, int32_t len, int32_t *i, uint16_t *u) {
  const uint32_t c = b[*i];
  if (c >= 1 && c < 0x80) {
    *u = (uint16_t)c;
    *i += 1;
    return true;
  }
  if ((c & 0xE0) == 0xC0) {
    if (*i + 1 >= len || (b[*i + 1] & 0xC0) != 0x80) return false;
    const uint32_t v = ((c & 0x1F) << 6) | (b[*i + 1] & 0x3Fu);
    if (v >= 1 && v < 0x80) return false;
    *u = (uint16_t)v;
    *i += 2;
    return true;
  }
  if ((c & 0xF0) == 0xE0) {
    if (*i + 2 >= len || (b[*i + 1] & 0xC0) != 0x80 || (b[*i + 2] & 0xC0) != 0x80) return false;
    const uint32_t v = ((c & 0x0F) << 12) | ((b[*i + 1] & 0x3Fu) << 6) | (b[*i + 2] & 0x3Fu);
    if (v < 0x800) return false;
    *u = (uint16_t)v;
    *i += 3;
    return true;
  }
  return false;
}
// units of a writeUTF body, or -1 if malformed; out (may be null) gets them
SME_RP_HD int32_t mutf8_decode(const uint8_t *b, int32_t len, uint16_t *out) {
  int32_t i = 0, nu = 0;
  while (i < len) {
    uint16_t u;
    if (!mutf8_unit(b, len, &i, &u)) return -1;
    if (out) out[nu] = u;
    nu++;
  }
  return nu;
}

// String.compareTo over UTF-16 units (TermDF.compareTo of one-component keys)
SME_RP_HD int cmp_units(const uint16_t *a, int64_t la, const uint16_t *b, int64_t lb) {
  const int64_t m = la < lb ? la : lb;
  for (int64_t i = 0; i < m; i++)
    if (a[i] != b[i]) return (int)a[i] - (int)b[i];
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

// a real term's posting, and its place after the previous one (tf desc, docno asc)
SME_RP_HD int post_check(int32_t docno, int32_t tf) { return tf <= 0 ? RP_TF : (tf > kMaxTf ? RP_TF_LIMIT : RP_OK); }
SME_RP_HD int post_pair_check(int32_t pd, int32_t pt, int32_t d, int32_t t) {
  if (pt == t && pd == d) return RP_DOCNO_DUP;
  return (pt > t || (pt == t && pd < d)) ? RP_OK : RP_POST_ORDER;
}
// a " " posting: (0,0) opens a map task's list, (docno,1) is the record before
SME_RP_HD int counter_check(int64_t i, int32_t docno, int32_t tf) {
  if (tf == 0) return docno == 0 ? RP_OK : RP_COUNTER;
  return tf == 1 && i > 0 ? RP_OK : RP_COUNTER;
}

SME_RP_HD const char *message(int code) {
  switch (code) {
    case RP_TRUNC: return "truncated record header";
    case RP_RECLEN_NEG: return "recLen < -1";
    case RP_PAST_END: return "record or sync escape runs past its partition's end";
    case RP_KEYLEN: return "keyLen inconsistent with the key's fields";
    case RP_KGRAM: return "loading K >= 2 record streams";
    case RP_N_NEG: return "posting count < 0";
    case RP_RECLEN: return "recLen does not match keyLen and the posting count";
    case RP_CLASS: return "value class is not sa.edu.kaust.io.PostingWritable";
    case RP_MUTF8: return "key is not modified UTF-8 as writeUTF writes it";
    case RP_KEY_ORDER: return "keys of a partition not strictly ascending";
    case RP_KEY_DUP: return "the same key in two partitions";
    case RP_DF: return "stored df is not 1 (real term) or the posting count (\" \")";
    case RP_SPACE_MANY: return "more than one \" \" doc-counter record";
    case RP_SPACE_NONE: return "terms but no \" \" doc-counter record";
    case RP_TF: return "a posting with tf <= 0";
    case RP_TF_LIMIT: return "a term frequency >= 2^24";
    case RP_POST_ORDER: return "postings not in (tf desc, docno asc) order";
    case RP_DOCNO_DUP: return "a docno repeated within a term";
    case RP_COUNTER: return "\" \" postings are not (0,0) / (docno,1) lists";
  }
  return "ok";
}

}  // namespace rp
}  // namespace sme
