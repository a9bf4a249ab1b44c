// sme_near.hip -- proximity queries: a batch of queries, each a list of term ids, a
// width N and a kind -> per query the documents that hold its terms near each other
// in one record, with the number of such places (freq) and the score (1 + ln freq)
// * idf(df), ordered by docno or by score and cut to the first m.  Kind 0 is the
// ordered window (#od:N: every next term at most N positions after the previous
// one), kind 1 the unordered window (#uw:N: all distinct terms within N positions);
// include/sme.h has both definitions in full.  Runs over the query-side CSR and the
// positions a K = 1 build kept, as phrase queries do.
//
// The pass -- plan, chunk filter, compaction, scoring, ordering and the cut -- is
// sme_phrase_pass.hpp's, shared with phrase queries (sme_phrase.hip); this file
// holds the position predicate, k_near_verify, and the scorer over a table that
// reaches past max_tf (an unordered freq can).
#include <hip/hip_runtime.h>
#include <math.h>

#include "sme_near.hpp"
#include "sme_phrase_pass.hpp"

namespace sme {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // "no position": above every position of a record (< 2^31)

// the highest set bit of m (m != 0)
__device__ __forceinline__ uint32_t top_bit(unsigned long long m) { return 63u - (uint32_t)__clzll((long long)m); }

// One wave per candidate (query q, docno d), grid-strided: freq[x] = the query's
// count summed over the records of docno d -- ps_docno[r0 .. r1), found by two
// bounds -- and flag[x] = freq > 0.  A record's stream is walked in tiles of 64
// positions; lane l loads ts[base + l] once, and a lane past the record's end
// holds -2, which no term has.  Lane j < L keeps query term j in a register, read
// by the others through readlane, and carry_j: the last position before this tile
// at which level j was reachable (ordered) or term j stood (unordered), kNone at
// every record start -- so nothing crosses a record's end.
//
// Ordered, level j >= 1: B = the ballot of level j - 1 in this tile; lane l's last
// reachable position before its own is B's highest bit below l, else carry_{j-1}
// as it stood before the tile; reach_j = ts == term_j and that position lies
// within N.  Only then does carry_{j-1} take B's highest bit.  freq += the last
// level's ballot.  Unordered, per distinct term j (dmask: the lanes whose term no
// earlier lane holds): one ballot of ts == term_j, lane l's last occurrence at or
// before l, else carry_j; the minimum over the terms is the window's far end, and
// a lane on a query term whose window reaches it within N counts.
//
// Positions within a record are below 2^31 (a build refuses more) and every
// "last" lies before (ordered) or at or before (unordered) the lane's own, so the
// unsigned difference pos - last is exact and compares with N <= 2^31 - 1 without
// wrapping; base + 64 stays below 2^32.  No LDS.
__global__ __launch_bounds__(kVerifyNT) void k_near_verify(Batch b, const int32_t *__restrict__ width,
                                                          const uint8_t *__restrict__ kind,
                                                          const int32_t *__restrict__ cdoc,
                                                          const uint32_t *__restrict__ cph, int64_t C,
                                                          const int64_t *__restrict__ ps_off,
                                                          const int32_t *__restrict__ ps_terms,
                                                          const int32_t *__restrict__ ps_docno, int64_t nR,
                                                          int32_t *__restrict__ freq, uint8_t *__restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = blockIdx.x * (int64_t)(kVerifyNT / 64) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (kVerifyNT / 64);
  const unsigned long long below = (1ull << lane) - 1;  // the lanes before this one
  const unsigned long long upto = below | (1ull << lane);
  for (int64_t x = wave; x < C; x += nwaves) {
    const uint32_t q = cph[x];
    const int32_t d = cdoc[x];
    const int64_t t0 = b.poff[q];
    const int L = __builtin_amdgcn_readfirstlane((int)(b.poff[q + 1] - t0));  // 1 .. kMaxLen
    const uint32_t N = (uint32_t)__builtin_amdgcn_readfirstlane(width[q]);    // 1 .. 2^31 - 1
    const bool unordered = __builtin_amdgcn_readfirstlane((int)kind[q]) == near::kUnordered;
    const int32_t mine = lane < L ? b.term[t0 + lane] : -1;
    // unordered: the lanes holding a term's first mention
    bool dup = false;
    for (int j = 0; unordered && j < L; j++) dup |= lane > j && mine == __builtin_amdgcn_readlane(mine, j);
    const unsigned long long dmask = __ballot(lane < L && !dup);
    const int64_t r0 = lower_bound(ps_docno, nR, d);
    const int64_t r1 = r0 + upper_bound(ps_docno + r0, nR - r0, d);
    int32_t f = 0;
    for (int64_t r = r0; r < r1; r++) {
      const int64_t o0 = ps_off[r];
      const uint32_t len = (uint32_t)(ps_off[r + 1] - o0);  // < 2^31
      const int32_t *__restrict__ ts = ps_terms + o0;
      uint32_t carry = kNone;
      for (uint32_t base = 0; base < len; base += 64) {
        const uint32_t pos = base + (uint32_t)lane;
        const int32_t w = pos < len ? ts[pos] : -2;
        unsigned long long hits;
        if (!unordered) {
          unsigned long long B = __ballot(w == __builtin_amdgcn_readlane(mine, 0));
          for (int j = 1; j < L; j++) {
            const int32_t tj = __builtin_amdgcn_readlane(mine, j);
            const uint32_t cprev = (uint32_t)__builtin_amdgcn_readlane((int)carry, j - 1);
            const unsigned long long lower = B & below;
            const uint32_t last = lower ? base + top_bit(lower) : cprev;
            const bool reach = w == tj && last != kNone && pos - last <= N;
            if (B && lane == j - 1) carry = base + top_bit(B);
            B = __ballot(reach);
          }
          hits = B;
        } else {
          bool in = false, all = true;
          uint32_t far = kNone;  // the earliest of the terms' last occurrences
          for (unsigned long long todo = dmask; todo; todo &= todo - 1) {
            const int j = __builtin_ctzll(todo);
            const bool eq = w == __builtin_amdgcn_readlane(mine, j);
            const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)carry, j);
            const unsigned long long B = __ballot(eq);
            const unsigned long long lower = B & upto;
            const uint32_t last = lower ? base + top_bit(lower) : cj;
            in |= eq;
            all &= last != kNone;
            far = last < far ? last : far;
            if (B && lane == j) carry = base + top_bit(B);
          }
          hits = __ballot(in && all && pos - far <= N - 1);
        }
        f += __popcll(hits);
      }
    }
    if (lane == 0) {
      freq[x] = f;
      flag[x] = f > 0;
    }
  }
}

// k_phrase_score over a table of lut_n entries: a freq at or past it is counted in
// *over and scored 0 -- never read past the table.
__global__ void k_near_score(const int32_t *__restrict__ idx, int64_t T, const int32_t *__restrict__ cdoc,
                             const uint32_t *__restrict__ cph, const int32_t *__restrict__ freq,
                             const double *__restrict__ lut, int64_t lut_n, const double *__restrict__ idf,
                             int32_t *__restrict__ mdoc, uint32_t *__restrict__ mph, int32_t *__restrict__ mfreq,
                             double *__restrict__ mscore, unsigned int *__restrict__ over) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < T; x += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = idx[x];
    const uint32_t p = cph[c];
    const int32_t f = freq[c];
    mdoc[x] = cdoc[c];
    mph[x] = p;
    mfreq[x] = f;
    const bool ok = f >= 0 && f < lut_n;
    if (!ok) atomicAdd(over, 1u);
    mscore[x] = ok ? __dmul_rn(lut[f], idf[p]) : 0.0;
  }
}

// *out = the most stream positions any docno has over all its records (the runs of
// equal ps_docno; a run's first record finds its end by one bound): no count of
// positions within a docno passes it
__global__ void k_near_doc_span(const int64_t *__restrict__ ps_off, const int32_t *__restrict__ ps_docno, int64_t nR,
                                unsigned long long *__restrict__ out) {
  unsigned long long best = 0;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nR; r += (int64_t)gridDim.x * blockDim.x) {
    const int32_t d = ps_docno[r];
    if (r > 0 && ps_docno[r - 1] == d) continue;
    const int64_t e = r + upper_bound(ps_docno + r, nR - r, d);
    best = max(best, (unsigned long long)(ps_off[e] - ps_off[r]));
  }
  for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor((long long)best, o, 64));
  if ((threadIdx.x & 63) == 0 && best) atomicMax(out, best);
}
}  // namespace

void grow_score_lut(sme_index *ix, int64_t n, hipStream_t st) {
  if (n <= ix->nq_lut_n) return;
  std::vector<double> lut((size_t)n, 0.0);
  for (int64_t i = 1; i < n; i++) lut[(size_t)i] = 1.0 + log((double)i);
  double *d = ix->d_nq_lut.as<double>((size_t)n);
  ix->nq_lut_n = 0;
  SME_HIP(hipMemcpyAsync(d, lut.data(), lut.size() * sizeof(double), hipMemcpyHostToDevice, st));
  SME_HIP(hipStreamSynchronize(st));  // (lut leaves scope)
  ix->nq_lut_n = n;
}

void query_near(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *widths,
                const uint8_t *kinds, int nq, int order, int m, hipStream_t st) {
  int bad = -1;
  const int rc = near::validate(term_ids, -1, q_offsets, widths, kinds, nq, ix->V, &bad);
  if (rc != near::N_OK) {
    char msg[128];
    const bool limit = near::describe(rc, bad, msg, sizeof msg);
    throw Error(limit ? SME_ELIMIT : SME_EINVAL, msg);
  }
  near_pass(ix, ix->nq, term_ids, q_offsets, widths, kinds, nq, order, m, nullptr, st);
}

void near_pass(sme_index *ix, DocFreqScores &out, const int32_t *term_ids, const int64_t *q_offsets,
               const int32_t *widths, const uint8_t *kinds, int nq, int order, int m, const NarrowSpec *narrow,
               hipStream_t st) {
  Blob blob;  // one upload: term offsets | term ids | widths | kinds (| the narrowing tables)
  size_t a_poff = 0, a_term = 0, a_width = 0, a_kind = 0;
  // The scorer table: an ordered freq is at most the last term's tf (<= max_tf), an
  // unordered one at most the sum of its distinct terms' tfs, |T| * max_tf -- the
  // index's tf of a docno being the sum of its records' stream counts -- and never
  // more than the docno's stream positions (nq_max_span, found once per index).
  // Sized for the batch's largest bound, filled by the build's own expression (so
  // its first max_tf + 1 entries are d_lut's bits), and kept: it only grows.
  int64_t lut_n = (int64_t)ix->max_tf + 1;
  if (nq > 0 && ix->nq_max_span < 0) {
    DevBuf spb;
    spb.pool = &ix->ctx->pool;
    unsigned long long *d_span = spb.as<unsigned long long>(1), span = 0;
    SME_HIP(hipMemsetAsync(d_span, 0, sizeof span, st));
    if (ix->ps_records > 0) {
      hipLaunchKernelGGL(k_near_doc_span, dim3(grid_for(ix->ps_records)), dim3(kNT), 0, st,
                         (const int64_t *)ix->d_ps_off.p, (const int32_t *)ix->d_ps_docno.p, ix->ps_records, d_span);
      SME_CHECK_LAUNCH();
    }
    SME_HIP(hipMemcpyAsync(&span, d_span, sizeof span, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    ix->nq_max_span = (int64_t)span;
  }
  if (nq > 0) {
    a_poff = blob.add(q_offsets, (size_t)nq + 1);
    a_term = blob.add(term_ids, (size_t)q_offsets[nq]);
    a_width = blob.add(widths, (size_t)nq);
    a_kind = blob.add(kinds, (size_t)nq);
    for (int i = 0; i < nq; i++) {
      if (kinds[i] != near::kUnordered) continue;
      int distinct = 0;
      for (int64_t s = q_offsets[i]; s < q_offsets[i + 1]; s++)
        distinct += std::find(term_ids + q_offsets[i], term_ids + s, term_ids[s]) == term_ids + s;
      lut_n = std::max(lut_n, std::min((int64_t)distinct * ix->max_tf, ix->nq_max_span) + 1);
    }
    grow_score_lut(ix, lut_n, st);
    lut_n = ix->nq_lut_n;
  }
  DevBuf ovb;
  ovb.pool = &ix->ctx->pool;
  unsigned int *d_over = nullptr;
  const char *limit = "proximity query: 2^31 or more candidate documents in one batch";
  const auto verify = [&](const uint8_t *d_in, Batch b, const int32_t *cdoc, const uint32_t *cph, int64_t C, int32_t *freq,
          uint8_t *flag) {
        hipLaunchKernelGGL(k_near_verify, dim3(verify_grid(C)), dim3(kVerifyNT), 0, st, b,
                           (const int32_t *)(d_in + a_width), d_in + a_kind, cdoc, cph, C,
                           (const int64_t *)ix->d_ps_off.p, (const int32_t *)ix->d_ps_terms.p,
                           (const int32_t *)ix->d_ps_docno.p, ix->ps_records, freq, flag);
      };
  const auto score = [&](unsigned g, const int32_t *idx, int64_t T, const int32_t *cdoc, const uint32_t *cph, const int32_t *freq,
          const double *d_idf, int32_t *mdoc, uint32_t *mph, int32_t *mfreq, double *mscore) {
        d_over = ovb.as<unsigned int>(1);
        SME_HIP(hipMemsetAsync(d_over, 0, sizeof(unsigned int), st));
        hipLaunchKernelGGL(k_near_score, dim3(g), dim3(kNT), 0, st, idx, T, cdoc, cph, freq,
                           (const double *)ix->d_nq_lut.p, lut_n, d_idf, mdoc, mph, mfreq, mscore, d_over);
      };
  if (narrow && nq > 0) {
    // the filter of structured queries: every candidate must also lie in the owner's groups
    const size_t owners = narrow->qgoff.size() - 1;
    for (size_t o = 0; o < owners; o++)
      if (narrow->qgoff[o + 1] - narrow->qgoff[o] > kNarrowGroups ||
          narrow->goff[(size_t)narrow->qgoff[o + 1]] - narrow->goff[(size_t)narrow->qgoff[o]] > kNarrowSlots)
        throw Error(SME_EINVAL, "proximity pass: a narrowing spec past what the filter stages");
    const size_t a_own = blob.add(narrow->owner.data(), narrow->owner.size());
    const size_t a_qg = blob.add(narrow->qgoff.data(), narrow->qgoff.size());
    const size_t a_g = blob.add(narrow->goff.data(), narrow->goff.size());
    const size_t a_nt = blob.add(narrow->terms.data(), narrow->terms.size());
    run_pass(
        ix, out, blob, a_poff, a_term, nq, order, m, limit, st,
        [&](const uint8_t *d_in, const PhraseOp &p) {
          return NarrowOp{p, (const int32_t *)(d_in + a_own), (const int64_t *)(d_in + a_qg),
                          (const int64_t *)(d_in + a_g), (const int32_t *)(d_in + a_nt)};
        },
        verify, score);
  } else {
    run_pass(ix, out, blob, a_poff, a_term, nq, order, m, limit, st, PlainFilter{}, verify, score);
  }
  if (d_over) {
    unsigned int over = 0;
    SME_HIP(hipMemcpyAsync(&over, d_over, sizeof over, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    if (over) {
      out.reset();  // the call returns nothing, and its stats say so
      SME_HIP(hipMemsetAsync(out.off.p, 0, ((size_t)nq + 1) * sizeof(int64_t), st));
      SME_HIP(hipStreamSynchronize(st));
      throw Error(SME_ELIMIT, "proximity query: " + std::to_string(over) +
                                  " match(es) with a freq past the scorer table (the index's tfs and its streams disagree)");
    }
  }
}

}  // namespace sme
