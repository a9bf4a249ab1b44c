// sme_ixmerge.hpp -- the parts of the index merger (sme_ixmerge.hip) shared by
// device and host: the limits, the validator of the input list with its messages,
// the diagonal search that cuts an n-way merge into tiles, and the plain
// restatement of the n-way merge of one term.  The validator and the restatement
// are plain C++, so tools/ixmerge_check.cc runs them under the host sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define SME_IXM_HD __host__ __device__
#else
#define SME_IXM_HD
#endif

namespace sme {
namespace ixmerge {

constexpr int kMaxInputs = 64;                      // one wave lane per input of a term
constexpr int kMinTile = 64, kMaxTile = 2048;       // "merge_tile": output postings per tile, a multiple of 64
constexpr int kDefaultTile = 1024;                  // 6 LDS words per posting: 26 KiB, two workgroups and more per CU
constexpr int64_t kTfLimit = int64_t(1) << 24;      // a summed tf at or past it is SME_ELIMIT, as in the loader
constexpr int64_t kNoValue = INT64_MIN;             // a tile boundary at a term's start: every docno is after it
constexpr bool legal_tile(int64_t v) { return v >= kMinTile && v <= kMaxTile && v % 64 == 0; }

// ---- the validator ----------------------------------------------------------
enum {
  M_OK = 0,
  M_COUNT = 1,     // n outside 1..kMaxInputs
  M_NULL = 2,      // a null input
  M_CONTEXT = 3,   // an input of another context
  M_RECORDS = 4,   // a records-only input (sme_merge_pieces output)
  M_CHARGRAM = 5,  // a CharKGramTermIndexer output
  M_KGRAM = 6,     // the context or an input has K != 1
};

struct InputDesc {  // what the validator reads of one input
  bool present, same_ctx, records_only;
  int job, K;
};

// Validates the list; *bad = the place of the first refused input (-1: not an
// input's fault).  Decided before any per-term work.  n is checked before the
// array is read, and in[i] is read only for i < n.
inline int validate(const InputDesc *in, int n, int ctx_K, int *bad) {
  *bad = -1;
  if (n < 1 || n > kMaxInputs) return M_COUNT;
  for (int i = 0; i < n; i++) {
    int rc = M_OK;
    if (!in[i].present)
      rc = M_NULL;
    else if (!in[i].same_ctx)
      rc = M_CONTEXT;
    else if (in[i].job != 0)
      rc = M_CHARGRAM;
    else if (in[i].records_only)
      rc = M_RECORDS;
    if (rc != M_OK) {
      *bad = i;
      return rc;
    }
  }
  if (ctx_K != 1) return M_KGRAM;
  for (int i = 0; i < n; i++)
    if (in[i].K != 1) {
      *bad = i;
      return M_KGRAM;
    }
  return M_OK;
}

// The message of a validate() result other than M_OK; true if the refusal is
// SME_ENOTIMPL (K >= 2), false if SME_EINVAL.
inline bool describe(int rc, int bad, char *buf, size_t n) {
  char where[32] = "";
  if (bad >= 0) snprintf(where, sizeof where, "input %d: ", bad);
  switch (rc) {
    case M_COUNT:
      snprintf(buf, n, "index merge: between 1 and %d inputs", kMaxInputs);
      return false;
    case M_NULL:
      snprintf(buf, n, "index merge: %sa null index", where);
      return false;
    case M_CONTEXT:
      snprintf(buf, n, "index merge: %san index of another context", where);
      return false;
    case M_RECORDS:
      snprintf(buf, n, "index merge: %sa records-only index (merged shard pieces) has no docno order", where);
      return false;
    case M_CHARGRAM:
      snprintf(buf, n, "index merge: %snot a TermKGramDocIndexer index", where);
      return false;
    default:
      snprintf(buf, n, "index merge: %smerging K >= 2 indexes", where);
      return true;
  }
}

// ---- the diagonal search ------------------------------------------------------
// first i in [0, n) with a[i] >= v (n if none).  The interval halves every step:
// it ends by its bound, 64 steps at the most, whatever the data.
SME_IXM_HD inline int64_t lower_bound_i32(const int32_t *a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  for (int it = 0; it < 64 && lo < hi; it++) {
    const int64_t m = lo + ((hi - lo) >> 1);
    if ((int64_t)a[m] < v)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}

// Where diagonal d of the merge of k ascending lists lies: the value v of element
// d (0 <= d < total length) of the merged sequence -- the least v with more than d
// elements <= v -- and *before = the elements below v.  Elements equal to v that
// the diagonal takes: d - *before, in list order.  `list(s, &ptr, &len)` names list
// s.  The value interval [INT32_MIN, INT32_MAX] halves every step (33 at the most).
template <typename F>
SME_IXM_HD inline int64_t diagonal_value(F list, int k, int64_t d, int64_t *before) {
  int64_t lo = INT32_MIN, hi = INT32_MAX;
  for (int it = 0; it < 33 && lo < hi; it++) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    int64_t c = 0;  // elements <= mid
    for (int s = 0; s < k; s++) {
      const int32_t *p;
      int64_t n;
      list(s, &p, &n);
      c += lower_bound_i32(p, n, mid + 1);
    }
    if (c > d)
      hi = mid;
    else
      lo = mid + 1;
  }
  int64_t b = 0;
  for (int s = 0; s < k; s++) {
    const int32_t *p;
    int64_t n;
    list(s, &p, &n);
    b += lower_bound_i32(p, n, lo);
  }
  *before = b;
  return lo;
}

// The cut of list s at a boundary (v, take): every element below v, and of the
// elements equal to v as many as `take` leaves after the `eq_before` equal
// elements of the lists before s.  take = 0 cuts at the value: equal docnos stay
// together on the far side (the postings merge, where they become one posting).
SME_IXM_HD inline int64_t cut_of(const int32_t *p, int64_t n, int64_t v, int64_t take, int64_t eq_before) {
  if (v == kNoValue) return 0;
  const int64_t lb = lower_bound_i32(p, n, v);
  if (take <= eq_before) return lb;
  const int64_t eq = lower_bound_i32(p, n, v + 1) - lb;
  const int64_t left = take - eq_before;
  return lb + (eq < left ? eq : left);
}

// ---- the merge of one term, plainly --------------------------------------------
struct Posting {
  int32_t docno, tf;
  bool operator==(const Posting &o) const { return docno == o.docno && tf == o.tf; }
};

// k docno-ascending lists (docno[s][0 .. len[s]), tf beside) -> the docno-order
// list: merged by docno, ties in list order, equal docnos one posting with the tfs
// summed (MyReducer.reduce).  false if a summed tf reaches kTfLimit.
inline bool merge_term(const int32_t *const *docno, const int32_t *const *tf, const int64_t *len, int k,
                       std::vector<Posting> *out) {
  out->clear();
  std::vector<int64_t> at((size_t)k, 0);
  for (;;) {
    int best = -1;
    for (int s = 0; s < k; s++)
      if (at[(size_t)s] < len[s] && (best < 0 || docno[s][at[(size_t)s]] < docno[best][at[(size_t)best]])) best = s;
    if (best < 0) break;
    const int32_t d = docno[best][at[(size_t)best]];
    int64_t sum = 0;
    for (int s = best; s < k; s++)
      while (at[(size_t)s] < len[s] && docno[s][at[(size_t)s]] == d) sum += tf[s][at[(size_t)s]++];
    if (sum >= kTfLimit) return false;
    out->push_back(Posting{d, (int32_t)sum});
  }
  return true;
}

// the reduce order of a docno-order list: stable by tf descending
inline std::vector<Posting> reduce_order(const std::vector<Posting> &dl) {
  std::vector<Posting> o = dl;
  std::stable_sort(o.begin(), o.end(), [](const Posting &a, const Posting &b) { return a.tf > b.tf; });
  return o;
}

}  // namespace ixmerge
}  // namespace sme
