// sme_ixdelete.hpp -- the parts of the index deletion pass (sme_ixdelete.hip) shared
// by device and host: the limits, the validator of a call with its messages, the
// index arithmetic of the docno bitmap, the task-start rule of the doc counter and
// the plain restatement of the compaction of one term.  All of it is plain C++, so
// tools/ixdelete_check.cc runs it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#if defined(__HIPCC__)
#define SME_IXD_HD __host__ __device__
#else
#define SME_IXD_HD
#endif

namespace sme {
namespace ixdelete {

// "delete_tile": postings per tile of the compaction, a multiple of 256.  A workgroup
// walks its tile in steps of 1024 postings (256 lanes x 16 bytes), so the LDS it
// takes (12 KiB) does not depend on the tile; the tile sets the grain of the count
// table and how often a workgroup searches d_off for its window of terms.  The
// default is the best of 1024 .. 65536 measured on c2.
constexpr int kMinTile = 256, kMaxTile = 65536;
constexpr int kDefaultTile = 16384;
constexpr bool legal_tile(int64_t v) { return v >= kMinTile && v <= kMaxTile && v % 256 == 0; }

// ---- the validator ----------------------------------------------------------
enum {
  D_OK = 0,
  D_NULL = 1,       // a null index or a null result pointer
  D_COUNT = 2,      // n < 0
  D_LIST = 3,       // n > 0 with a null list
  D_CHARGRAM = 4,   // a CharKGramTermIndexer output
  D_RECORDS = 5,    // a records-only index (sme_merge_pieces output)
  D_KGRAM = 6,      // K != 1
  D_PARTFILES = 7,  // the record docnos are not all known (opened from part files)
};

struct CallDesc {  // what the validator reads of one call
  bool has_index, has_out, has_list;
  int64_t n;
  bool records_only;
  int job, K;
  bool rec_complete;
};

// Decided before any per-posting work; the index's fields are read only when
// there is an index.
inline int validate(const CallDesc &c) {
  if (!c.has_index || !c.has_out) return D_NULL;
  if (c.n < 0) return D_COUNT;
  if (c.n > 0 && !c.has_list) return D_LIST;
  if (c.job != 0) return D_CHARGRAM;
  if (c.records_only) return D_RECORDS;
  if (c.K != 1) return D_KGRAM;
  if (!c.rec_complete) return D_PARTFILES;
  return D_OK;
}

// The message of a validate() result other than D_OK; true if the refusal is
// SME_ENOTIMPL (K >= 2), false if SME_EINVAL.
inline bool describe(int rc, char *buf, size_t n) {
  switch (rc) {
    case D_NULL:
      snprintf(buf, n, "index delete: a null index or result pointer");
      return false;
    case D_COUNT:
      snprintf(buf, n, "index delete: a negative docno count");
      return false;
    case D_LIST:
      snprintf(buf, n, "index delete: a null docno list");
      return false;
    case D_CHARGRAM:
      snprintf(buf, n, "index delete: not a TermKGramDocIndexer index");
      return false;
    case D_RECORDS:
      snprintf(buf, n, "index delete: a records-only index (merged shard pieces) has no docno order");
      return false;
    case D_PARTFILES:
      snprintf(buf, n,
               "index delete: an index opened from part files (or merged from one) does not hold every "
               "record's docno: a map task's last docno is never stored");
      return false;
    default:
      snprintf(buf, n, "index delete: deleting from K >= 2 indexes");
      return true;
  }
}

// ---- the docno bitmap ---------------------------------------------------------
// One bit per docno of [dmin, dmax], 32 to a word.  The differences are taken in
// 64 bits: dmax - dmin + 1 reaches 2^32, and a listed docno may be any int32.
SME_IXD_HD inline int64_t span_of(int64_t dmin, int64_t dmax) { return dmax >= dmin ? dmax - dmin + 1 : 0; }
SME_IXD_HD inline int64_t bitmap_words(int64_t span) { return (span + 31) >> 5; }
// the bit of docno d, or -1 if d is outside the range
SME_IXD_HD inline int64_t bit_of(int32_t d, int64_t dmin, int64_t span) {
  const int64_t b = (int64_t)d - dmin;
  return b >= 0 && b < span ? b : -1;
}
SME_IXD_HD inline bool bitmap_test(const uint32_t *bm, int32_t d, int64_t dmin, int64_t span) {
  const int64_t b = bit_of(d, dmin, span);
  return b >= 0 && ((bm[b >> 5] >> (b & 31)) & 1u);
}
// host fill (the device fills with atomicOr)
inline void bitmap_set(uint32_t *bm, int32_t d, int64_t dmin, int64_t span) {
  const int64_t b = bit_of(d, dmin, span);
  if (b >= 0) bm[b >> 5] |= 1u << (b & 31);
}

// ---- the doc counter's task starts ---------------------------------------------
// first[i] != 0: record i starts a map task (record 0 always does; first may be
// null: one task).  keep[i] != 0: record i survives.  A surviving record starts a
// task of the result if and only if an input task start lies after the survivor
// before it and at or before itself.  As the device computes it: starts_upto[i] =
// the task starts among records 0 .. i, carried along with every survivor; two
// neighbouring survivors with different counts have a start between them.
inline void compact_records(const int32_t *docno, const uint8_t *first, const uint8_t *keep, int64_t n,
                            std::vector<int32_t> *out_docno, std::vector<uint8_t> *out_first) {
  out_docno->clear();
  out_first->clear();
  int64_t starts = 0, last = -1;
  for (int64_t i = 0; i < n; i++) {
    if (i == 0 || (first && first[i])) starts++;
    if (!keep[i]) continue;
    out_docno->push_back(docno[i]);
    out_first->push_back(out_first->empty() || starts != last ? 1 : 0);
    last = starts;
  }
}

// ---- the compaction of one term, plainly ---------------------------------------
struct Posting {
  int32_t docno, tf;
  bool operator==(const Posting &o) const { return docno == o.docno && tf == o.tf; }
};
// the postings of (docno[0 .. n), tf beside) whose docno is not in the bitmap, in
// the list's order -- either order of a term's postings
inline void compact_term(const int32_t *docno, const int32_t *tf, int64_t n, const uint32_t *bm, int64_t dmin,
                         int64_t span, std::vector<Posting> *out) {
  out->clear();
  for (int64_t i = 0; i < n; i++)
    if (!bitmap_test(bm, docno[i], dmin, span)) out->push_back(Posting{docno[i], tf[i]});
}

}  // namespace ixdelete
}  // namespace sme
