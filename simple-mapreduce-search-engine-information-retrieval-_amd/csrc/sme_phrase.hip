// sme_phrase.hip -- phrase queries: a batch of phrases, each a list of term ids ->
// per phrase the documents that hold its terms at consecutive positions of one
// record, with the number of such places (freq) and the TF-IDF score a K = L index
// gives that gram, ordered by docno or by score and cut to the first m.  Runs over
// the query-side CSR (d_off / d_docno_d) and the positions a K = 1 build kept
// (d_ps_off / d_ps_terms / d_ps_docno: the records' term streams, a forward index).
//
// The pass -- plan, chunk filter, compaction, scoring, ordering and the cut -- is
// sme_phrase_pass.hpp's, shared with proximity queries (sme_near.hip); this file
// holds the phrase predicate: k_phrase_verify counts, one wave per surviving
// (phrase, docno), the phrase's occurrences in the streams of the docno's records.
#include "sme_phrase_pass.hpp"

namespace sme {
namespace {
// One wave per candidate (phrase p, docno d), grid-strided: freq[x] = the phrase's
// occurrences summed over the records of docno d -- ps_docno[r0 .. r1), found by two
// bounds -- and flag[x] = freq > 0.  Lane j < L keeps phrase term j in a register;
// the lanes stride a record's start positions (consecutive lanes, consecutive
// stream words), compare the first term, and the wave goes on to term j only while
// a lane still matches, every lane reading term j from lane j.  A start s is tried
// only if s + L <= the record's length, so nothing at or past ps_off[r + 1] is
// read and no window crosses into the next record.  Positions within a record are
// 32-bit (a build refuses 2^31 stream positions), stream offsets 64-bit.
__global__ __launch_bounds__(kVerifyNT) void k_phrase_verify(Batch b, const int32_t *__restrict__ cdoc,
                                                            const uint32_t *__restrict__ cph, int64_t C,
                                                            const int64_t *__restrict__ ps_off,
                                                            const int32_t *__restrict__ ps_terms,
                                                            const int32_t *__restrict__ ps_docno, int64_t nR,
                                                            int32_t *__restrict__ freq, uint8_t *__restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = blockIdx.x * (int64_t)(kVerifyNT / 64) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (kVerifyNT / 64);
  for (int64_t x = wave; x < C; x += nwaves) {
    const uint32_t p = cph[x];
    const int32_t d = cdoc[x];
    const int64_t t0 = b.poff[p];
    const int L = (int)(b.poff[p + 1] - t0);  // 1 .. kMaxLen
    const int32_t mine = lane < L ? b.term[t0 + lane] : -1;
    const int32_t ph0 = __builtin_amdgcn_readfirstlane(mine);
    const int64_t r0 = lower_bound(ps_docno, nR, d);
    const int64_t r1 = r0 + upper_bound(ps_docno + r0, nR - r0, d);
    int32_t f = 0;
    for (int64_t r = r0; r < r1; r++) {
      const int64_t o0 = ps_off[r];
      const int32_t nst = (int32_t)(ps_off[r + 1] - o0) - L + 1;  // start positions of this record
      const int32_t *__restrict__ ts = ps_terms + o0;
      // (unsigned rounds: nst may be near 2^31, and s0 + 64 must not wrap)
      for (uint32_t s0 = 0; nst > 0 && s0 < (uint32_t)nst; s0 += 64) {
        const uint32_t s = s0 + (uint32_t)lane;
        bool m = s < (uint32_t)nst && ts[s] == ph0;
        for (int j = 1; j < L && __ballot(m) != 0; j++) {
          const int32_t pj = __shfl(mine, j, 64);
          if (m) m = ts[s + j] == pj;
        }
        f += __popcll(__ballot(m));
      }
    }
    if (lane == 0) {
      freq[x] = f;
      flag[x] = f > 0;
    }
  }
}
}  // namespace

void query_phrase(sme_index *ix, const int32_t *term_ids, const int64_t *p_offsets, int np, int order, int m,
                  hipStream_t st) {
  int bad = -1;
  const int rc = phrase::validate(term_ids, -1, p_offsets, np, ix->V, &bad);
  if (rc != phrase::P_OK) {
    char msg[128];
    const bool limit = phrase::describe(rc, bad, msg, sizeof msg);
    throw Error(limit ? SME_ELIMIT : SME_EINVAL, msg);
  }
  Blob blob;  // one upload: term offsets | term ids
  size_t a_poff = 0, a_term = 0;
  if (np > 0) {
    a_poff = blob.add(p_offsets, (size_t)np + 1);
    a_term = blob.add(term_ids, (size_t)p_offsets[np]);
  }
  run_pass(
      ix, ix->pq, blob, a_poff, a_term, np, order, m, "phrase query: 2^31 or more candidate documents in one batch",
      st, PlainFilter{},
      [&](const uint8_t *, Batch b, const int32_t *cdoc, const uint32_t *cph, int64_t C, int32_t *freq, uint8_t *flag) {
        hipLaunchKernelGGL(k_phrase_verify, dim3(verify_grid(C)), dim3(kVerifyNT), 0, st, b, cdoc, cph, C,
                           (const int64_t *)ix->d_ps_off.p, (const int32_t *)ix->d_ps_terms.p,
                           (const int32_t *)ix->d_ps_docno.p, ix->ps_records, freq, flag);
      },
      [&](unsigned g, const int32_t *idx, int64_t T, const int32_t *cdoc, const uint32_t *cph, const int32_t *freq,
          const double *d_idf, int32_t *mdoc, uint32_t *mph, int32_t *mfreq, double *mscore) {
        hipLaunchKernelGGL(k_phrase_score, dim3(g), dim3(kNT), 0, st, idx, T, cdoc, cph, freq,
                           (const double *)ix->d_lut.p, d_idf, mdoc, mph, mfreq, mscore);
      });
}

}  // namespace sme
