// sme_posfile.hpp -- the parts of the positions file (sme_posfile.hip; include/sme.h
// has the format, DESIGN.md 4m the passes) shared by device and host: the header's
// fields, its validator with the messages, the overflow-safe size arithmetic, the
// bit packing of one tile and the vocabulary digest's term hash.  All of it is
// plain C++, so tools/posfile_check.cc runs it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if defined(__HIPCC__)
#define SME_PF_HD __host__ __device__
#else
#define SME_PF_HD
#endif

namespace sme {
namespace posfile {

constexpr uint8_t kMagic[8] = {0x53, 0x4D, 0x45, 0x50, 0x4F, 0x53, 0x00, 0x01};  // "SMEPOS", 0, 1
constexpr uint32_t kVersion = 1;
constexpr uint64_t kHeaderBytes = 64;
constexpr int kMaxBits = 31;
constexpr uint64_t kLimit = uint64_t(1) << 31;  // records and positions stay below it
// Positions per tile of the encode and decode kernels: a multiple of 64, so a
// tile is b * kTile / 64 whole 64-bit words and two tiles never share a word.
constexpr int kTile = 1024;
constexpr int kTileWords32 = kTile / 32 * kMaxBits;  // the 32-bit words of the widest tile

// need = max(1, bit length of (V - 1)): the narrowest width that holds every id < V
SME_PF_HD inline int need_bits(uint64_t V) {
  int b = 1;
  while (b < 64 && V > (uint64_t(1) << b)) b++;
  return b;
}

// ---- the header -----------------------------------------------------------------
struct Header {
  uint32_t version, bits;
  uint64_t records, positions, V, digest;
};

inline uint64_t rd_le(const uint8_t *p, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}
inline void wr_le(uint8_t *p, int n, uint64_t v) {
  for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}
inline void write_header(uint8_t *p, const Header &h) {
  memset(p, 0, kHeaderBytes);
  memcpy(p, kMagic, 8);
  wr_le(p + 8, 4, h.version);
  wr_le(p + 12, 4, h.bits);
  wr_le(p + 16, 8, h.records);
  wr_le(p + 24, 8, h.positions);
  wr_le(p + 32, 8, h.V);
  wr_le(p + 40, 8, h.digest);
}
// (the magic and the reserved bytes are the validator's to look at)
inline Header read_header(const uint8_t *p) {
  Header h;
  h.version = (uint32_t)rd_le(p + 8, 4);
  h.bits = (uint32_t)rd_le(p + 12, 4);
  h.records = rd_le(p + 16, 8);
  h.positions = rd_le(p + 24, 8);
  h.V = rd_le(p + 32, 8);
  h.digest = rd_le(p + 40, 8);
  return h;
}

// ---- the sections' places -----------------------------------------------------------
// 64 header bytes, int32 docno[records] and u32 len[records], each zero-padded to a
// multiple of 8 bytes, then ceil(positions * bits / 64) words of 8 bytes.  Every
// step is checked: false if a product or a sum leaves 64 bits, whatever the counts.
struct Layout {
  uint64_t docno_at, len_at, words_at, nwords, size;
};
inline bool layout(uint64_t records, uint64_t positions, uint32_t bits, Layout *out) {
  uint64_t sec, nbits, wbytes, at;
  if (__builtin_mul_overflow(records, (uint64_t)4, &sec)) return false;
  if (__builtin_add_overflow(sec, (uint64_t)7, &sec)) return false;
  sec &= ~uint64_t(7);
  if (__builtin_mul_overflow(positions, (uint64_t)bits, &nbits)) return false;
  const uint64_t nwords = nbits / 64 + (nbits % 64 ? 1 : 0);
  if (__builtin_mul_overflow(nwords, (uint64_t)8, &wbytes)) return false;
  out->docno_at = kHeaderBytes;
  if (__builtin_add_overflow(kHeaderBytes, sec, &at)) return false;
  out->len_at = at;
  if (__builtin_add_overflow(at, sec, &at)) return false;
  out->words_at = at;
  out->nwords = nwords;
  if (__builtin_add_overflow(at, wbytes, &at)) return false;
  out->size = at;
  return true;
}

// ---- the validator -------------------------------------------------------------------
enum {
  H_OK = 0,
  H_SHORT = 1,      // fewer bytes than a header
  H_MAGIC = 2,
  H_VERSION = 3,
  H_RESERVED = 4,
  H_BITS = 5,       // bits outside [need, 31]
  H_RECORDS = 6,    // records != the index's N, or 2^31 or more
  H_V = 7,          // V != the index's V
  H_POSITIONS = 8,  // 2^31 positions or more: the build's own limit (SME_ELIMIT)
  H_SIZE = 9,       // the file is not exactly as long as its header says
};

// The header of an n-byte file meant for an index of N records and V terms, in the
// order the fields are documented; p has min(n, 64) readable bytes.  *lay is filled
// when the result is H_OK, before any section offset is used.
inline int validate_header(const uint8_t *p, uint64_t n, uint64_t N, uint64_t V, Header *hdr, Layout *lay) {
  if (n < kHeaderBytes) return H_SHORT;
  if (memcmp(p, kMagic, 8) != 0) return H_MAGIC;
  const Header h = read_header(p);
  *hdr = h;
  if (h.version != kVersion) return H_VERSION;
  for (int i = 48; i < 64; i++)
    if (p[i] != 0) return H_RESERVED;
  if (h.bits < (uint32_t)need_bits(V) || h.bits > (uint32_t)kMaxBits) return H_BITS;
  if (h.records != N || h.records >= kLimit) return H_RECORDS;
  if (h.V != V) return H_V;
  if (h.positions >= kLimit) return H_POSITIONS;
  if (!layout(h.records, h.positions, h.bits, lay) || lay->size != n) return H_SIZE;
  return H_OK;
}

// The message of a validate_header() result other than H_OK; true if the refusal
// is SME_ELIMIT (the positions limit), false if SME_EPARSE.
inline bool describe_header(int rc, const Header &h, uint64_t n, uint64_t N, uint64_t V, char *buf, size_t cap) {
  Layout lay;
  switch (rc) {
    case H_SHORT:
      snprintf(buf, cap, "positions file: size %llu is shorter than the 64-byte header", (unsigned long long)n);
      return false;
    case H_MAGIC:
      snprintf(buf, cap, "positions file: magic is not \"SMEPOS\" 0 1");
      return false;
    case H_VERSION:
      snprintf(buf, cap, "positions file: version %u (this library reads version %u)", h.version, kVersion);
      return false;
    case H_RESERVED:
      snprintf(buf, cap, "positions file: reserved bytes are not zero");
      return false;
    case H_BITS:
      snprintf(buf, cap, "positions file: bits %u outside [%d, %d] for V = %llu", h.bits, need_bits(V), kMaxBits,
               (unsigned long long)V);
      return false;
    case H_RECORDS:
      snprintf(buf, cap, "positions file: records %llu, the index has N = %llu (fewer than 2^31)",
               (unsigned long long)h.records, (unsigned long long)N);
      return false;
    case H_V:
      snprintf(buf, cap, "positions file: V %llu, the index has V = %llu", (unsigned long long)h.V,
               (unsigned long long)V);
      return false;
    case H_POSITIONS:
      snprintf(buf, cap, "positions file: positions %llu: 2^31 or more term positions", (unsigned long long)h.positions);
      return true;
    default:
      if (layout(h.records, h.positions, h.bits, &lay))
        snprintf(buf, cap, "positions file: size %llu, its header gives %llu bytes", (unsigned long long)n,
                 (unsigned long long)lay.size);
      else
        snprintf(buf, cap, "positions file: size %llu, its header's counts leave 64 bits", (unsigned long long)n);
      return false;
  }
}

// ---- the bit string of one tile ------------------------------------------------------
// Position p's id occupies bits [p b, (p + 1) b) of the words seen as one
// little-endian bit string, so 32-bit word w of a tile holds the ids of positions
// floor(32 w / b) .. floor((32 w + 31) / b).  ids: the tile's kTile ids, zeros past
// its last position.  This is the encode kernel's inner step over its LDS copy.
SME_PF_HD inline uint32_t word32_of(const int32_t *ids, int b, int w) {
  const int bit = 32 * w;
  int p = bit / b;
  const int sh = bit - p * b;  // bits of id p that the words before took
  uint64_t acc = (uint64_t)(uint32_t)ids[p] >> sh;
  for (int filled = b - sh; filled < 32; filled += b) acc |= (uint64_t)(uint32_t)ids[++p] << filled;
  return (uint32_t)acc;
}
// The id of the tile's position p out of its 32-bit words; w[(p b >> 5) + 1] is read
// too (the caller keeps one word after the tile's last).  The decode kernel's step.
SME_PF_HD inline uint32_t id_of(const uint32_t *w, int b, int p) {
  const int bit = p * b, i = bit >> 5, sh = bit & 31;
  const uint64_t two = (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32);
  return (uint32_t)(two >> sh) & ((uint32_t(1) << b) - 1u);
}

// ---- the vocabulary digest -----------------------------------------------------------
// h_t = FNV-1a-64 over the 8 bytes of t, little-endian, then term t's UTF-16 code
// units, each low byte first; the digest is the sum of h_t over t < V mod 2^64.
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;
SME_PF_HD inline uint64_t term_hash(uint64_t t, const uint16_t *units, int64_t n) {
  uint64_t h = kFnvBasis;
  for (int i = 0; i < 8; i++) h = (h ^ ((t >> (8 * i)) & 0xFF)) * kFnvPrime;
  for (int64_t i = 0; i < n; i++) {
    h = (h ^ (uint64_t)(units[i] & 0xFF)) * kFnvPrime;
    h = (h ^ (uint64_t)(units[i] >> 8)) * kFnvPrime;
  }
  return h;
}

// ---- the calls -------------------------------------------------------------------------
enum {
  C_OK = 0,
  C_NULL = 1,       // a null index, buffer or result pointer
  C_CHARGRAM = 2,   // a CharKGramTermIndexer output
  C_RECORDS = 3,    // a records-only index (sme_merge_pieces output)
  C_KGRAM = 4,      // K != 1
  C_NOPOS = 5,      // writing: the index keeps no positions
  C_HASPOS = 6,     // attaching: the index already keeps positions
  C_BITS = 7,       // writing: bits outside {0} and [need, 31]
  C_FLAGS = 8,      // attaching: unknown flag bits
};
constexpr int kAttachNoCrosscheck = 1;  // SME_ATTACH_NO_CROSSCHECK

struct CallDesc {  // what the validator reads of one call
  bool attach;     // attaching (else writing)
  bool has_args;   // no null pointer among the arguments
  int job, K;
  bool records_only, has_positions;
  uint64_t V;
  int bits, flags;
};

inline int validate_call(const CallDesc &c) {
  if (!c.has_args) return C_NULL;
  if (c.job != 0) return C_CHARGRAM;
  if (c.records_only) return C_RECORDS;
  if (c.K != 1) return C_KGRAM;
  if (c.attach) {
    if (c.has_positions) return C_HASPOS;
    if (c.flags & ~kAttachNoCrosscheck) return C_FLAGS;
  } else {
    if (!c.has_positions) return C_NOPOS;
    if (c.bits != 0 && (c.bits < need_bits(c.V) || c.bits > kMaxBits)) return C_BITS;
  }
  return C_OK;
}

// the SME_EINVAL message of a validate_call() result other than C_OK
inline void describe_call(int rc, const CallDesc &c, char *buf, size_t cap) {
  const char *what = c.attach ? "positions attach" : "positions file";
  switch (rc) {
    case C_NULL:
      snprintf(buf, cap, "%s: null argument", what);
      break;
    case C_CHARGRAM:
      snprintf(buf, cap, "%s: not a TermKGramDocIndexer index", what);
      break;
    case C_RECORDS:
      snprintf(buf, cap, "%s: the index has no query side (merged shard pieces)", what);
      break;
    case C_KGRAM:
      snprintf(buf, cap, "%s: the index holds k-grams (K != 1), not terms", what);
      break;
    case C_NOPOS:
      snprintf(buf, cap, "%s: the index keeps no positions (build it with option \"positions\" 1)", what);
      break;
    case C_HASPOS:
      snprintf(buf, cap, "%s: the index already keeps positions", what);
      break;
    case C_BITS:
      snprintf(buf, cap, "%s: bits %d is neither 0 nor in [%d, %d]", what, c.bits, need_bits(c.V), kMaxBits);
      break;
    default:
      snprintf(buf, cap, "%s: unknown flag bits 0x%x", what, (unsigned)(c.flags & ~kAttachNoCrosscheck));
      break;
  }
}

}  // namespace posfile
}  // namespace sme
