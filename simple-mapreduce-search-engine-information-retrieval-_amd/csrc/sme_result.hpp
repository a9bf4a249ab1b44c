// sme_result.hpp -- what a batched query call leaves on the index: n + 1 offsets
// and up to seven value columns of `total` entries, query i's values at
// [off[i], off[i + 1]), beside the call's counts.
//
// Ownership: the device arrays and the host mirrors belong to the index until the
// same feature's next call -- that is what include/sme.h promises a host.  Every
// feature therefore has a ResultSet of its own on the index (sme_internal.hpp);
// two features never share one, however alike their columns.  The buffers are
// pooled blocks of the context; a feature's temporaries are pooled blocks of the
// call and never live here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <tuple>
#include <vector>

#include "sme_common.hpp"

namespace sme {

struct ResultSet {
  static constexpr int kMaxCols = 7;
  struct Column {
    DevBuf d;                // [total] elements of esize bytes
    size_t esize = 0;        // 0: no such column
    std::vector<uint8_t> h;  // host mirror, filled by fetch
  };
  DevBuf off;  // int64 [n + 1]
  Column col[kMaxCols];
  std::vector<int64_t> h_off;
  int n = 0;          // queries of the last call (offsets)
  int64_t total = 0;  // entries of every column
  // the call's counts, where the feature has them: candidates examined; candidates
  // that passed the filter; matches before the cut
  uint64_t cands = 0, verified = 0, matches = 0;

  explicit ResultSet(std::initializer_list<size_t> esizes) {
    int c = 0;
    for (size_t e : esizes) col[c++].esize = e;
  }
  void bind(BufPool *pool) {
    off.pool = pool;
    for (Column &c : col) c.d.pool = pool;
  }
  // A call resets its result before it launches anything: whatever ends it after
  // that leaves an empty result and zero counts behind, not the previous call's.
  void reset() {
    total = 0;
    cands = verified = matches = 0;
  }
  int64_t *offsets(int queries) {
    n = queries;
    return off.as<int64_t>((size_t)n + 1);
  }
  const int64_t *dev_offsets() const { return (const int64_t *)off.p; }
  // Offsets and columns of the last call into the host mirrors, through `st`, which
  // is synchronised.  A mirror is never an empty vector, so data() stays a valid
  // pointer when total == 0; the columns are then not copied (their device buffers
  // may never have been allocated).  Defined in sme_api.hip, its only user.
  void fetch(hipStream_t st);
};

// A ResultSet whose column c holds elements of the c-th type: the one place a
// feature's column types are written (the layouts below); every access is by index.
template <typename... Ts>
struct ResultOf : ResultSet {
  static_assert(sizeof...(Ts) <= kMaxCols, "more columns than a ResultSet holds");
  template <int C>
  using elem = std::tuple_element_t<C, std::tuple<Ts...>>;
  ResultOf() : ResultSet({sizeof(Ts)...}) {}
  template <int C>
  elem<C> *alloc(int64_t count) {  // column C sized for `count` entries (DevBuf::as)
    return col[C].d.template as<elem<C>>((size_t)count);
  }
  template <int C>
  const elem<C> *dev() const {
    return (const elem<C> *)col[C].d.p;
  }
  template <int C>
  const elem<C> *host() const {
    return (const elem<C> *)col[C].h.data();
  }
};

// the features' layouts: column names and element types
struct TermIds : ResultOf<int32_t> {  // wildcard expansion
  enum { ids };  // matching term ids
};
struct TermDists : ResultOf<int32_t, uint8_t> {  // spelling suggestions
  enum { ids, dist };  // term ids; their distances
};
struct DocScores : ResultOf<int32_t, double> {  // Boolean retrieval, structured queries
  enum { docno, score };  // matching documents; their scores
};
struct DocFreqScores : ResultOf<int32_t, int32_t, double> {  // phrase / proximity pass (sme_phrase_pass.hpp)
  enum { docno, freq, score };  // matching documents; the query's count in each; their scores
};
struct TermFreqDocsScores : ResultOf<int32_t, int32_t, int32_t, double> {  // relevance feedback (sme_feedback.hip)
  enum { term, freq, docs, score };  // a set's terms; their occurrences; the set's documents holding them; their scores
};
struct PassageRows : ResultOf<int32_t, int32_t, int32_t, int32_t, int32_t, uint64_t, double> {  // best passages (sme_passage.hip)
  // a kept candidate; its best window's record ordinal, first position and length; the
  // window's hits; the slots it covers; the sum of their idfs
  enum { docno, rec, start, len, hits, mask, score };
};
struct WindowTerms : ResultOf<int32_t, int8_t> {  // best passages: the rows' windows, row i's at offsets i, i + 1
  enum { term, slot };  // the stream's term ids; each one's slot in its row's query, or -1
};

}  // namespace sme
