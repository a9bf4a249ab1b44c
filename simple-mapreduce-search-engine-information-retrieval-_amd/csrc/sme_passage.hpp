// sme_passage.hpp -- the host parts of the best-passage scan (sme_passage.hip,
// sme_query_passages) that need no device: the limits, the validator of a batch's two
// offset arrays, its term ids and its host candidate lists, the normaliser that turns
// a query's listed term ids into slots, and the plain restatement of one record's
// best window, which the kernel is held to.  Plain C++, so tools/passage_check.cc runs
// it under the host sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sme {
namespace passage {

constexpr int kMaxWidth = 256;   // positions of a window
constexpr int kMaxSlots = 64;    // distinct term ids of a query: the bits of a row's mask
constexpr int kMaxListed = 1024; // term ids listed by a query, -1 and repeats included
constexpr int kChunk = 256;      // window starts a wave takes at a time (sme_query_passages_stats)
constexpr int kTile = 256;       // candidates per workgroup
constexpr int64_t kMaxBatch = (int64_t(1) << 31) - 1;  // candidates, and listed ids, of one batch

enum {
  P_OK = 0,
  P_QOFFSETS = 1,  // q_offsets not ascending from 0, or not agreeing with the array size
  P_DOFFSETS = 2,  // d_offsets not ascending from 0, or not agreeing with the array size
  P_LISTED = 3,    // more than kMaxListed term ids listed by a query
  P_BATCH = 4,     // 2^31 or more candidates, or listed ids, in the batch
  P_TERM = 5,      // a term id outside [-1, V)
  P_ORDER = 6,     // a query's candidates not strictly ascending (signed int32)
  P_SLOTS = 7,     // more than kMaxSlots distinct term ids in a query
  P_WIDTH_LOW = 8, // width < 1
  P_WIDTH_HIGH = 9 // width > kMaxWidth
};

inline int check_width(int width) { return width < 1 ? P_WIDTH_LOW : width > kMaxWidth ? P_WIDTH_HIGH : P_OK; }

// A query's slots: of the listed ids, -1 dropped and a repeated id kept at its first
// place; the j-th id left is slot j.  Appends them to `ids` (listed order) and
// returns their number, or -1 past kMaxSlots (nothing is appended then).
inline int normalise(const int32_t *listed, int64_t n, std::vector<int32_t> &ids) {
  const size_t base = ids.size();
  for (int64_t i = 0; i < n; i++) {
    const int32_t t = listed[i];
    if (t == -1) continue;
    if (std::find(ids.begin() + (ptrdiff_t)base, ids.end(), t) != ids.end()) continue;
    if (ids.size() - base == (size_t)kMaxSlots) {
      ids.resize(base);
      return -1;
    }
    ids.push_back(t);
  }
  return (int)(ids.size() - base);
}

// Validates nq queries: q_off[nq + 1] into term_ids[nterms], d_off[nq + 1] into
// docnos[ndocs].  nterms / ndocs are the sizes of the arrays the caller holds; -1 =
// implied by the offsets (q_off[nq], d_off[nq]), as a C-ABI caller passes them.
// docnos == nullptr: the candidates are not read (a device array: a kernel checks
// their order).  An offset is compared with the array's size before anything is read
// through it, so a batch cut short anywhere is P_QOFFSETS / P_DOFFSETS and nothing
// past an array is read.  *bad_query = the query of the first problem (-1: not
// inside a query).
inline int validate(const int32_t *term_ids, int64_t nterms, const int64_t *q_off, const int32_t *docnos,
                    int64_t ndocs, const int64_t *d_off, int nq, int64_t V, int *bad_query) {
  *bad_query = -1;
  if (nq < 0) return P_QOFFSETS;
  if (nq == 0) return P_OK;  // (no offset is read: both arrays may be absent)
  if (q_off[0] != 0) return P_QOFFSETS;
  for (int q = 0; q < nq; q++)
    if (q_off[q + 1] < q_off[q] || (nterms >= 0 && q_off[q + 1] > nterms)) {
      *bad_query = q;
      return P_QOFFSETS;
    }
  if (nterms < 0) nterms = q_off[nq];
  if (q_off[nq] != nterms) return P_QOFFSETS;
  if (d_off[0] != 0) return P_DOFFSETS;
  for (int q = 0; q < nq; q++)
    if (d_off[q + 1] < d_off[q] || (ndocs >= 0 && d_off[q + 1] > ndocs)) {
      *bad_query = q;
      return P_DOFFSETS;
    }
  if (ndocs < 0) ndocs = d_off[nq];
  if (d_off[nq] != ndocs) return P_DOFFSETS;
  if (nterms > kMaxBatch || ndocs > kMaxBatch) return P_BATCH;
  std::vector<int32_t> ids;
  for (int q = 0; q < nq; q++) {
    *bad_query = q;
    if (q_off[q + 1] - q_off[q] > kMaxListed) return P_LISTED;
    for (int64_t s = q_off[q]; s < q_off[q + 1]; s++)
      if (term_ids[s] < -1 || term_ids[s] >= V) return P_TERM;
    ids.clear();
    if (normalise(term_ids + q_off[q], q_off[q + 1] - q_off[q], ids) < 0) return P_SLOTS;
    if (docnos)
      for (int64_t i = d_off[q] + 1; i < d_off[q + 1]; i++)
        if (docnos[i - 1] >= docnos[i]) return P_ORDER;
  }
  *bad_query = -1;
  return P_OK;
}

// A window and its place in the order that picks the best one.
struct Window {
  int32_t rec = -1, start = 0, len = 0, hits = 0;
  uint64_t mask = 0;
  double score = 0.0;
};
inline int cover_of(uint64_t mask) {
  int c = 0;
  for (; mask; mask &= mask - 1) c++;
  return c;
}
// a stands before b: score descending, cover descending, hits descending, rec
// ascending, start ascending
inline bool before(const Window &a, const Window &b) {
  if (a.score != b.score) return a.score > b.score;
  const int ca = cover_of(a.mask), cb = cover_of(b.mask);
  if (ca != cb) return ca > cb;
  if (a.hits != b.hits) return a.hits > b.hits;
  if (a.rec != b.rec) return a.rec < b.rec;
  return a.start < b.start;
}
// the score of a mask: the fp64 sum from 0.0 over its set bits, ascending, of the
// slots' idfs (the callers are built without contraction; there is no product anyway)
inline double score_of(uint64_t mask, const double *slot_idf) {
  double s = 0.0;
  for (int j = 0; j < kMaxSlots; j++)
    if (mask >> j & 1) s = s + slot_idf[j];
  return s;
}

// The best window of one record, ordinal `rec` of its docno: stream[0 .. n), the
// query's nslots distinct ids (slot j = ids[j]) and their idfs.  Every start 0 ..
// max(0, n - width) is looked at on its own, nothing carried from one to the next.
inline Window best_of_record(const int32_t *stream, int64_t n, int32_t rec, const int32_t *ids, int nslots,
                             const double *slot_idf, int width) {
  Window best;
  const int64_t last = n > width ? n - width : 0;
  for (int64_t s = 0; s <= last; s++) {
    Window w;
    w.rec = rec;
    w.start = (int32_t)s;
    const int64_t e = std::min<int64_t>(s + width, n);
    w.len = (int32_t)(e - s);
    for (int64_t p = s; p < e; p++)
      for (int j = 0; j < nslots; j++)
        if (ids[j] == stream[p]) {
          w.mask |= uint64_t(1) << j;
          w.hits++;
        }
    w.score = score_of(w.mask, slot_idf);
    if (s == 0 || before(w, best)) best = w;
  }
  return best;
}

}  // namespace passage
}  // namespace sme
