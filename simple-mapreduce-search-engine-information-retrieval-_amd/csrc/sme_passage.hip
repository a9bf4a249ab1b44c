// sme_passage.hip -- best passages (include/sme.h, sme_query_passages): per query a
// list of term ids and a strictly ascending list of candidate docnos -> for every
// candidate the best window of at most `width` consecutive positions of one of its
// records' term streams (d_ps_off / d_ps_terms / d_ps_docno): where it lies, which
// query terms it covers, how many hits it holds and the sum of the covered terms'
// idfs; the candidates covering enough terms kept, ordered and cut; and, if asked
// for, the kept windows' term ids with the hits marked.
//
//   k_pw_check   (device candidates) a descending or equal pair inside a query ->
//                the first such query; k_pw_best does nothing once it is set
//   k_pw_best    one workgroup per (query, tile of kTile candidates), one wave per
//                candidate; see the kernel
//   excl_scan    the tiles' kept counts -> the rows before every tile; k_pw_woff,
//                k_cut and a second scan -> the result offsets after the cut
//   k_pw_emit    order 0: the kept candidates' rows straight into the result, in the
//                given order, below the cut -- no sort.  order 1: their candidate
//                numbers, score keys and queries, which lie in (query, docno) order;
//                stable sorts by the score key and by the query, and k_pw_gather
//   k_pw_terms   (with_terms) one wave per row: the window's stream words and slots
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>
#include <exception>
#include <string>

#include "sme_bool.hpp"
#include "sme_chunks.hpp"
#include "sme_internal.hpp"
#include "sme_passage.hpp"

namespace sme {
namespace {
using namespace chunks;
using namespace passage;

constexpr int kWaves = kNT / 64;
constexpr int kStrip = kChunk + kMaxWidth;  // a chunk's starts and the width - 1 positions behind them
static_assert(kTile == 64 * kWaves, "a tile gives every lane of the workgroup one candidate to look up");
static_assert(kChunk % 64 == 0 && kStrip < 65536, "whole rounds; match counts fit 16 bits");

enum { C_WITH_RECORD, C_POSITIONS, C_COUNT };  // the call's device counters

struct BestArgs {
  const int64_t *ps_off;
  const int32_t *ps_terms, *ps_docno;
  int64_t nR;
  const double *idf;     // [V]
  const int32_t *sid;    // every query's distinct ids, ascending within the query
  const uint8_t *sslot;  // their slots
  const int64_t *uoff;   // [nq + 1] into sid / sslot
  const int32_t *cand;
  const int64_t *doff;  // [nq + 1] candidates
  const int64_t *toff;  // [nq + 1] tiles
  int nq;
  int64_t ntiles;
  int width, min_cover;
  const int *bad;  // the order check's verdict (INT_MAX: none)
  int32_t *rec, *start, *len, *hits;  // [candidates]
  uint64_t *mask;
  double *score;
  int64_t *tkept;  // [ntiles] candidates kept per tile
  unsigned long long *counters;
};

__device__ __forceinline__ int tile_query(const int64_t *__restrict__ toff, int nq, int64_t t) {
  return upper_bound(toff, nq, t) - 1;
}
// lane l's value in every lane (l the same in all of them)
__device__ __forceinline__ int64_t lane_value64(int64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
// The lanes of a wave exchange values through its own LDS strip: the wave's DS
// operations execute in program order, so all that is needed is that the compiler
// keeps them in that order.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ void k_pw_check(const int32_t *__restrict__ cand, const int64_t *__restrict__ doff, int nq, int64_t total,
                           int *__restrict__ bad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x + 1; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (cand[i - 1] < cand[i]) continue;
    const int q = upper_bound(doff, nq, i) - 1;  // the query holding candidate i
    if (doff[q] != i) atomicMin(bad, q);         // (its first candidate has no predecessor)
  }
}

// a lane's best window so far; `any`: it has one
struct Best {
  double score;
  uint64_t mask;
  int32_t hits, rec, start, len;
  bool any;
};
// (score, cover, hits) of a window against the best: strictly better
__device__ __forceinline__ bool better(double sc, uint64_t mk, int h, const Best &b) {
  if (sc != b.score) return sc > b.score;
  const int c = __popcll(mk), bc = __popcll(b.mask);
  if (c != bc) return c > bc;
  return h > b.hits;
}

// One workgroup per (query, tile).  The query's distinct ids (sorted, with their
// slots) and the slots' idfs go to LDS once.  Candidate j of the tile belongs to wave
// j % kWaves, and lane j / kWaves of that wave finds its records -- the two bounds on
// d_ps_docno, the first record's stream bounds and the docno's whole span -- so a
// wave's 64 dependent searches run side by side and none of them stands between two
// scans.  The wave then takes its candidates one after another.  A record is worked
// through in chunks of kChunk window starts: the chunk's positions and the width - 1
// behind them are loaded, consecutive lanes consecutive words, each looked up in the
// LDS id list and written as a one-hot mask into the wave's strip, with the matches
// before each position (ballots) beside it.  A chunk without a match is settled by
// its first window.  Otherwise log2(width) in-place rounds leave M[i] = OR of the P
// masks from i on, P the largest power of two <= width, and the window at s is
// M[s] | M[s + width - P]; its hits the difference of two match counts.  A lane
// meets its starts in ascending order, so it keeps a window only if it is strictly
// better in (score, cover, hits), and adds idfs only when the mask differs from its
// last one; one butterfly picks the candidate's best window with (rec, start) as the
// last keys.
__global__ __launch_bounds__(kNT) void k_pw_best(const BestArgs A) {
  __shared__ uint64_t s_mask[kWaves][kStrip];
  __shared__ double s_idf[kMaxSlots];
  __shared__ int32_t s_id[kMaxSlots];
  __shared__ uint16_t s_pre[kWaves][kStrip + 2];
  __shared__ uint8_t s_slot[kMaxSlots];
  __shared__ unsigned long long s_cnt[C_COUNT];
  __shared__ int s_kept;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (*A.bad != INT_MAX) return;  // (uniform: written before this launch)
  const int w = A.width;
  const int P = 1 << (31 - __clz(w));
  uint64_t *__restrict__ M = s_mask[wv];
  uint16_t *__restrict__ pre = s_pre[wv];
  for (int64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    const int q = tile_query(A.toff, A.nq, tile);
    const int64_t c0 = A.doff[q] + (tile - A.toff[q]) * kTile;
    const int L = (int)min((int64_t)kTile, A.doff[q + 1] - c0);  // >= 1: only candidates make tiles
    const int64_t u0 = A.uoff[q];
    const int nd = (int)(A.uoff[q + 1] - u0);  // <= kMaxSlots
    if (tid < nd) {
      const int32_t t = A.sid[u0 + tid];
      const int sl = A.sslot[u0 + tid];
      s_id[tid] = t;
      s_slot[tid] = (uint8_t)sl;
      s_idf[sl] = A.idf[t];
    }
    if (tid < C_COUNT) s_cnt[tid] = 0;
    if (tid == 0) s_kept = 0;
    __syncthreads();
    // this lane's candidate: its records [r0, r0 + nrec), the first one's stream [p0, p1)
    int64_t r0 = 0, p0 = 0, p1 = 0;
    int nrec = 0;
    {
      const int j = lane * kWaves + wv;
      int64_t span = 0;
      if (j < L) {
        const int32_t d = A.cand[c0 + j];
        r0 = lower_bound(A.ps_docno, A.nR, d);
        nrec = (int)upper_bound(A.ps_docno + r0, A.nR - r0, d);
        if (nrec > 0) {
          p0 = A.ps_off[r0];
          p1 = A.ps_off[r0 + 1];
          span = A.ps_off[r0 + nrec] - p0;
        }
      }
      const unsigned long long with = __ballot(nrec > 0);
      for (int o = 32; o > 0; o >>= 1) span += __shfl_xor(span, o, 64);
      if (lane == 0 && with) {
        atomicAdd(&s_cnt[C_WITH_RECORD], (unsigned long long)__popcll(with));
        atomicAdd(&s_cnt[C_POSITIONS], (unsigned long long)span);
      }
    }
    const int mine = (L - wv + kWaves - 1) / kWaves;  // candidates of this wave
    int kept = 0;
    for (int l = 0; l < mine; l++) {
      const int nr = __builtin_amdgcn_readlane(nrec, l);
      const int64_t cr0 = lane_value64(r0, l);
      int64_t b = lane_value64(p0, l), e = lane_value64(p1, l);
      Best best{0.0, 0, 0, -1, 0, 0, false};
      uint64_t last_mask = 0;
      double last_score = 0.0;
      for (int rec = 0; rec < nr; rec++) {
        if (rec > 0) {  // (the streams of a docno's records are adjacent)
          b = e;
          e = A.ps_off[cr0 + rec + 1];
        }
        const int32_t *__restrict__ ts = A.ps_terms + b;
        const int64_t n = e - b;
        const int64_t ns = n > w ? n - w + 1 : 1;  // window starts of the record
        for (int64_t cb = 0; cb < ns; cb += kChunk) {
          const int nsc = (int)min((int64_t)kChunk, ns - cb);  // starts of the chunk
          const int Lz = nsc + w - 1;                          // strip entries its windows read
          const int Lp = (int)min((int64_t)Lz, n - cb);        // those inside the record
          int run = 0;
          for (int i0 = 0; i0 < Lz; i0 += 64) {
            const int i = i0 + lane;
            uint64_t mk = 0;
            if (i < Lp) {
              const int32_t t = ts[cb + i];
              const int x = lower_bound((const int32_t *)s_id, nd, t);
              if (x < nd && s_id[x] == t) mk = 1ull << s_slot[x];
            }
            const unsigned long long bal = __ballot(mk != 0);
            if (i < Lz) {
              M[i] = mk;
              pre[i] = (uint16_t)(run + __popcll(bal & ((1ull << lane) - 1)));
            }
            run += __popcll(bal);
          }
          if (run == 0) {  // no match in the chunk: its windows are alike and the first stands for them
            if (lane == 0 && (!best.any || better(0.0, 0, 0, best)))
              best = Best{0.0, 0, 0, rec, (int32_t)cb, (int32_t)min((int64_t)w, n - cb), true};
            continue;
          }
          if (lane == 0) pre[Lz] = (uint16_t)run;
          wave_lds_order();
          for (int k = 1; 2 * k <= w; k <<= 1) {
            // ascending and in place: entry i reads i and i + k, both still of this round
            for (int i0 = 0; i0 < Lz; i0 += 64) {
              const int i = i0 + lane;
              uint64_t a = 0;
              if (i < Lz) {
                a = M[i];
                if (i + k < Lz) a |= M[i + k];
              }
              wave_lds_order();
              if (i < Lz) M[i] = a;
              wave_lds_order();
            }
          }
          for (int i0 = 0; i0 < nsc; i0 += 64) {
            const int s = i0 + lane;
            if (s < nsc) {
              const uint64_t mk = M[s] | M[s + w - P];
              const int h = (int)pre[s + w] - (int)pre[s];
              if (mk != last_mask) {
                double sc = 0.0;
                for (uint64_t mm = mk; mm; mm &= mm - 1) sc = __dadd_rn(sc, s_idf[__ffsll((unsigned long long)mm) - 1]);
                last_mask = mk;
                last_score = sc;
              }
              if (!best.any || better(last_score, mk, h, best))
                best = Best{last_score, mk, h, rec, (int32_t)(cb + s), (int32_t)min((int64_t)w, n - cb - s), true};
            }
          }
          wave_lds_order();  // (the next chunk rewrites the strip)
        }
      }
      // the wave's best: (score, cover, hits) descending, then (rec, start) ascending
      for (int o = 32; o > 0; o >>= 1) {
        Best x;
        x.score = __shfl_xor(best.score, o, 64);
        x.mask = (uint64_t)__shfl_xor((long long)best.mask, o, 64);
        x.hits = __shfl_xor(best.hits, o, 64);
        x.rec = __shfl_xor(best.rec, o, 64);
        x.start = __shfl_xor(best.start, o, 64);
        x.len = __shfl_xor(best.len, o, 64);
        x.any = __shfl_xor((int)best.any, o, 64) != 0;
        bool take = false;
        if (x.any) {
          if (!best.any)
            take = true;
          else if (better(x.score, x.mask, x.hits, best))
            take = true;
          else if (!better(best.score, best.mask, best.hits, x))
            take = x.rec != best.rec ? x.rec < best.rec : x.start < best.start;
        }
        if (take) best = x;
      }
      if (lane == 0) {
        const int64_t c = c0 + l * kWaves + wv;
        A.rec[c] = best.rec;  // (no record: -1, and zeros)
        A.start[c] = best.start;
        A.len[c] = best.len;
        A.hits[c] = best.hits;
        A.mask[c] = best.mask;
        A.score[c] = best.score;
        kept += __popcll(best.mask) >= A.min_cover;
      }
    }
    if (lane == 0 && kept) atomicAdd(&s_kept, kept);
    __syncthreads();
    if (tid == 0) {
      A.tkept[tile] = s_kept;
      if (s_cnt[C_WITH_RECORD]) {
        atomicAdd(&A.counters[C_WITH_RECORD], s_cnt[C_WITH_RECORD]);
        atomicAdd(&A.counters[C_POSITIONS], s_cnt[C_POSITIONS]);
      }
    }
    __syncthreads();  // (the next tile rewrites everything)
  }
}

// woff[i] = rows before query i's first tile (i = nq: all of them)
__global__ void k_pw_woff(const int64_t *__restrict__ moff, const int64_t *__restrict__ toff, int64_t nq,
                          int64_t *__restrict__ woff) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nq; i += (int64_t)gridDim.x * blockDim.x)
    woff[i] = moff[toff[i]];
}

// the candidates' windows (k_pw_best's output) and the result's columns
struct Rows {
  int32_t *docno, *rec, *start, *len, *hits;
  uint64_t *mask;
  double *score;
};
__device__ __forceinline__ void copy_row(const Rows &to, int64_t at, int32_t docno, const Rows &from, int64_t c) {
  to.docno[at] = docno;
  to.rec[at] = from.rec[c];
  to.start[at] = from.start[c];
  to.len[at] = from.len[c];
  to.hits[at] = from.hits[c];
  to.mask[at] = from.mask[c];
  to.score[at] = from.score[c];
}

// The kept candidates of every tile, in the given order.  DIRECT (order 0): kept
// candidate number rk of its query goes to row roff[q] + rk if that is below the cut.
// Else: kept candidate number moff[tile] + rank of the batch leaves its candidate
// number, its score key and its query.
template <bool DIRECT>
__global__ __launch_bounds__(kNT) void k_pw_emit(const int32_t *__restrict__ cand, const int64_t *__restrict__ doff,
                                                 const int64_t *__restrict__ toff, int nq, int64_t ntiles, Rows win,
                                                 int min_cover, const int64_t *__restrict__ moff,
                                                 const int64_t *__restrict__ roff, Rows out,
                                                 uint32_t *__restrict__ ocand, uint64_t *__restrict__ okey,
                                                 uint32_t *__restrict__ operm, uint32_t *__restrict__ oq) {
  __shared__ int s_w[kNT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int q = tile_query(toff, nq, tile);
    const int64_t c0 = doff[q] + (tile - toff[q]) * kTile;
    const int L = (int)min((int64_t)kTile, doff[q + 1] - c0);
    int64_t run = DIRECT ? roff[q] + (moff[tile] - moff[toff[q]]) : moff[tile];
    const int64_t end = DIRECT ? roff[q + 1] : moff[tile + 1];  // (the cut is in roff)
    for (int r = 0; r < L && run < end; r += kNT) {  // (uniform)
      const int j = r + tid;
      const bool keep = j < L && __popcll(win.mask[c0 + j]) >= min_cover;
      const unsigned long long mk = __ballot(keep);
      if (lane == 0) s_w[wv] = __popcll(mk);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int x = 0; x < kNT / 64; x++) {
        const int ws = s_w[x];
        before += x < wv ? ws : 0;
        total += ws;
      }
      const int64_t at = run + before + __popcll(mk & ((1ull << lane) - 1));
      if (keep && at < end) {
        if (DIRECT) {
          copy_row(out, at, cand[c0 + j], win, c0 + j);
        } else {
          ocand[at] = (uint32_t)(c0 + j);
          okey[at] = boolq::score_key(win.score[c0 + j]);
          operm[at] = (uint32_t)at;
          oq[at] = (uint32_t)q;
        }
      }
      run += total;
      __syncthreads();  // (s_w is rewritten by the next round)
    }
  }
}

// the query of every kept candidate, through the permutation so far
__global__ void k_pw_key_query(const uint32_t *__restrict__ mq, const uint32_t *__restrict__ perm, int64_t n,
                               uint32_t *__restrict__ key) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    key[i] = mq[perm[i]];
}
// Sorted kept candidate x (query qs[x], kept candidate perm[x]) is the (x - woff[q])-th
// of its query: a row if that is below the cut.
__global__ void k_pw_gather(const uint32_t *__restrict__ qs, const uint32_t *__restrict__ perm,
                            const uint32_t *__restrict__ mcand, const int32_t *__restrict__ cand, Rows win,
                            int64_t total, const int64_t *__restrict__ woff, const int64_t *__restrict__ roff, int64_t m,
                            Rows out) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t q = qs[x];
    const int64_t rk = x - woff[q];
    if (m > 0 && rk >= m) continue;
    const int64_t c = mcand[perm[x]];
    copy_row(out, roff[q] + rk, cand[c], win, c);
  }
}

// len64[i] = row i's len (entry `total`: 0): the window terms' offsets before their scan
__global__ void k_pw_len64(const int32_t *__restrict__ len, int64_t total, int64_t *__restrict__ len64) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= total; i += (int64_t)gridDim.x * blockDim.x)
    len64[i] = i < total ? len[i] : 0;
}

// One wave per row: the window's stream words, and for each its slot in the row's
// query or -1.  The row's record is found as k_pw_best found it.
__global__ __launch_bounds__(kNT) void k_pw_terms(Rows row, int64_t total, const int64_t *__restrict__ roff, int nq,
                                                  const int64_t *__restrict__ woff, const int64_t *__restrict__ ps_off,
                                                  const int32_t *__restrict__ ps_terms,
                                                  const int32_t *__restrict__ ps_docno, int64_t nR,
                                                  const int32_t *__restrict__ sid, const uint8_t *__restrict__ sslot,
                                                  const int64_t *__restrict__ uoff, int32_t *__restrict__ wterm,
                                                  int8_t *__restrict__ wslot) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t r = blockIdx.x * (int64_t)kWaves + wv; r < total; r += (int64_t)gridDim.x * kWaves) {
    const int len = row.len[r];
    if (len == 0) continue;  // (no record, or an empty one)
    const int q = upper_bound(roff, nq, r) - 1;
    const int64_t u0 = uoff[q];
    const int nd = (int)(uoff[q + 1] - u0);
    const int64_t rc = lower_bound(ps_docno, nR, row.docno[r]) + row.rec[r];
    const int32_t *__restrict__ ts = ps_terms + ps_off[rc] + row.start[r];
    const int64_t at = woff[r];
    for (int i = lane; i < len; i += 64) {
      const int32_t t = ts[i];
      const int x = lower_bound(sid + u0, nd, t);
      wterm[at + i] = t;
      wslot[at + i] = x < nd && sid[u0 + x] == t ? (int8_t)sslot[u0 + x] : (int8_t)-1;
    }
  }
}

std::string at_query(int q) { return q >= 0 ? " (query " + std::to_string(q) + ")" : std::string(); }

}  // namespace

void query_passages(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *docnos,
                    bool on_device, const int64_t *d_offsets, const int64_t *d_offsets_dev, int nq, int width,
                    int min_cover, int order, int m, int with_terms, hipStream_t st) {
  sme_ctx *cx = ix->ctx;
  PassageRows &out = ix->pw;
  WindowTerms &wout = ix->pwt;
  // whatever ends the call from here on leaves two empty results behind
  out.reset();
  wout.reset();
  ix->pw_with_record = ix->pw_positions = 0;
  switch (check_width(width)) {
    case P_OK:
      break;
    case P_WIDTH_LOW:
      throw Error(SME_EINVAL, "passages: width must be >= 1");
    default:
      throw Error(SME_ELIMIT, "passages: width above " + std::to_string(kMaxWidth));
  }
  int bad = -1;
  const int rc = validate(term_ids, -1, q_offsets, on_device ? nullptr : docnos, -1, d_offsets, nq, ix->V, &bad);
  switch (rc) {
    case P_OK:
      break;
    case P_QOFFSETS:
      throw Error(SME_EINVAL, "passages: q_offsets do not ascend from 0" + at_query(bad));
    case P_DOFFSETS:
      throw Error(SME_EINVAL, "passages: d_offsets do not ascend from 0" + at_query(bad));
    case P_LISTED:
      throw Error(SME_ELIMIT, "passages: more than " + std::to_string(kMaxListed) + " term ids listed" + at_query(bad));
    case P_SLOTS:
      throw Error(SME_ELIMIT,
                  "passages: more than " + std::to_string(kMaxSlots) + " distinct term ids" + at_query(bad));
    case P_BATCH:
      throw Error(SME_ELIMIT, "passages: 2^31 or more candidates or term ids in one batch");
    case P_TERM:
      throw Error(SME_EINVAL, "passages: a term id outside [-1, V)" + at_query(bad));
    default:
      throw Error(SME_EINVAL, "passages: candidates not strictly ascending" + at_query(bad));
  }
  int64_t *d_roff = out.offsets(nq);
  int64_t *d_woff0 = wout.offsets(0);
  SME_HIP(hipMemsetAsync(d_woff0, 0, sizeof(int64_t), st));
  if (nq == 0) {
    SME_HIP(hipMemsetAsync(d_roff, 0, sizeof(int64_t), st));
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  const int64_t total = d_offsets[nq];
  // every query's slots: its distinct ids sorted for the kernels' searches, each with its slot
  std::vector<int32_t> ids, sid;
  std::vector<uint8_t> sslot;
  std::vector<int64_t> uoff((size_t)nq + 1, 0), toff((size_t)nq + 1, 0);
  std::vector<std::pair<int32_t, uint8_t>> pairs;
  for (int q = 0; q < nq; q++) {
    ids.clear();
    const int nd = normalise(term_ids + q_offsets[q], q_offsets[q + 1] - q_offsets[q], ids);  // >= 0: validated
    pairs.clear();
    for (int j = 0; j < nd; j++) pairs.emplace_back(ids[(size_t)j], (uint8_t)j);
    std::sort(pairs.begin(), pairs.end());
    for (const auto &p : pairs) {
      sid.push_back(p.first);
      sslot.push_back(p.second);
    }
    uoff[(size_t)q + 1] = (int64_t)sid.size();
    toff[(size_t)q + 1] = toff[(size_t)q] + (d_offsets[q + 1] - d_offsets[q] + kTile - 1) / kTile;
  }
  const int64_t ntiles = toff[(size_t)nq];
  // one upload: slot offsets | tile offsets | candidate offsets | sorted ids | their slots
  Blob blob;
  const size_t a_uoff = blob.add(uoff.data(), (size_t)nq + 1);
  const size_t a_toff = blob.add(toff.data(), (size_t)nq + 1);
  const size_t a_doff = blob.add(d_offsets, (size_t)nq + 1);
  const size_t a_sid = blob.add(sid.data(), sid.size());
  const size_t a_slot = blob.add(sslot.data(), sslot.size());
  // temporaries of this call: pooled blocks, back in the pool on return
  DevBuf in, cnb, rcb, stb, lnb, htb, mkb, scb, tkb, wob, kpb, scn, ctr, mcb, mqb, sa, sb, pa, pb, ka, kb, radix, l64;
  for (DevBuf *p : {&in, &cnb, &rcb, &stb, &lnb, &htb, &mkb, &scb, &tkb, &wob, &kpb, &scn, &ctr, &mcb, &mqb, &sa, &sb, &pa,
                    &pb, &ka, &kb, &radix, &l64})
    p->pool = &cx->pool;
  try {
    const uint8_t *d_in = in.as<uint8_t>(blob.bytes.size());
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st));
    const int64_t *d_toff = (const int64_t *)(d_in + a_toff);
    const int64_t *d_uoff = (const int64_t *)(d_in + a_uoff);
    const int64_t *d_doff = on_device ? d_offsets_dev : (const int64_t *)(d_in + a_doff);
    const int32_t *d_sid = (const int32_t *)(d_in + a_sid);
    const uint8_t *d_slot = d_in + a_slot;
    const int32_t *d_cand = docnos;
    if (!on_device) {
      int32_t *c = cnb.as<int32_t>((size_t)total);
      if (total) SME_HIP(hipMemcpyAsync(c, docnos, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, st));
      d_cand = c;
    }
    struct Counters {
      unsigned long long n[C_COUNT];
      int bad;
    } h{{0, 0}, INT_MAX};
    Counters *d_ctr = ctr.as<Counters>(1);
    SME_HIP(hipMemcpyAsync(d_ctr, &h, sizeof h, hipMemcpyHostToDevice, st));
    const Rows win{nullptr,
                   rcb.as<int32_t>((size_t)total),
                   stb.as<int32_t>((size_t)total),
                   lnb.as<int32_t>((size_t)total),
                   htb.as<int32_t>((size_t)total),
                   mkb.as<uint64_t>((size_t)total),
                   scb.as<double>((size_t)total)};
    int64_t *moff = tkb.as<int64_t>((size_t)ntiles + 1);
    SME_HIP(hipMemsetAsync(moff + ntiles, 0, sizeof(int64_t), st));
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min(ntiles, kMaxGrid));
    const int64_t *ps_off = (const int64_t *)ix->d_ps_off.p;
    const int32_t *ps_terms = (const int32_t *)ix->d_ps_terms.p;
    const int32_t *ps_docno = (const int32_t *)ix->d_ps_docno.p;
    if (ntiles > 0) {
      if (on_device) {
        hipLaunchKernelGGL(k_pw_check, dim3(grid_for(total)), dim3(kNT), 0, st, d_cand, d_doff, nq, total, &d_ctr->bad);
        SME_CHECK_LAUNCH();
      }
      BestArgs A;
      A.ps_off = ps_off;
      A.ps_terms = ps_terms;
      A.ps_docno = ps_docno;
      A.nR = ix->ps_records;
      A.idf = (const double *)ix->d_idf.p;
      A.sid = d_sid;
      A.sslot = d_slot;
      A.uoff = d_uoff;
      A.cand = d_cand;
      A.doff = d_doff;
      A.toff = d_toff;
      A.nq = nq;
      A.ntiles = ntiles;
      A.width = width;
      A.min_cover = min_cover;
      A.bad = &d_ctr->bad;
      A.rec = win.rec;
      A.start = win.start;
      A.len = win.len;
      A.hits = win.hits;
      A.mask = win.mask;
      A.score = win.score;
      A.tkept = moff;
      A.counters = d_ctr->n;
      hipLaunchKernelGGL(k_pw_best, dim3(grid), dim3(kNT), 0, st, A);
      SME_CHECK_LAUNCH();
    }
    // kept candidates before every tile, before every query, and the result offsets after the cut
    excl_scan<int64_t>(moff, moff, ntiles + 1, scn, st);
    int64_t *woff = wob.as<int64_t>((size_t)nq + 1);
    int64_t *kept = kpb.as<int64_t>((size_t)nq + 1);
    hipLaunchKernelGGL(k_pw_woff, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, (const int64_t *)moff, d_toff,
                       (int64_t)nq, woff);
    hipLaunchKernelGGL(k_cut, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, (const int64_t *)woff, (int64_t)nq,
                       (int64_t)m, kept);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(kept, d_roff, (int64_t)nq + 1, scn, st);
    int64_t out_total = 0, matches = 0;
    SME_HIP(hipMemcpyAsync(&out_total, d_roff + nq, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipMemcpyAsync(&matches, moff + ntiles, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipMemcpyAsync(&h, d_ctr, sizeof h, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    if (h.bad != INT_MAX) {
      SME_HIP(hipMemsetAsync(d_roff, 0, ((size_t)nq + 1) * sizeof(int64_t), st));
      SME_HIP(hipStreamSynchronize(st));
      throw Error(SME_EINVAL, "passages: candidates not strictly ascending" + at_query(h.bad));
    }
    const Rows rows{out.alloc<PassageRows::docno>(out_total), out.alloc<PassageRows::rec>(out_total),
                    out.alloc<PassageRows::start>(out_total), out.alloc<PassageRows::len>(out_total),
                    out.alloc<PassageRows::hits>(out_total),  out.alloc<PassageRows::mask>(out_total),
                    out.alloc<PassageRows::score>(out_total)};
    if (matches > 0 && order == 0) {
      hipLaunchKernelGGL(k_pw_emit<true>, dim3(grid), dim3(kNT), 0, st, d_cand, d_doff, d_toff, nq, ntiles, win,
                         min_cover, (const int64_t *)moff, (const int64_t *)d_roff, rows, (uint32_t *)nullptr,
                         (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr);
      SME_CHECK_LAUNCH();
    } else if (matches > 0) {
      const size_t T = (size_t)matches;
      uint32_t *mcand = mcb.as<uint32_t>(T), *mq = mqb.as<uint32_t>(T);
      uint64_t *s0 = sa.as<uint64_t>(T), *s1 = sb.as<uint64_t>(T);
      uint32_t *p0 = pa.as<uint32_t>(T), *p1 = pb.as<uint32_t>(T);
      uint32_t *k0 = ka.as<uint32_t>(T), *k1q = kb.as<uint32_t>(T);
      hipLaunchKernelGGL(k_pw_emit<false>, dim3(grid), dim3(kNT), 0, st, d_cand, d_doff, d_toff, nq, ntiles, win,
                         min_cover, (const int64_t *)moff, (const int64_t *)d_roff, rows, mcand, s0, p0, mq);
      SME_CHECK_LAUNCH();
      // the kept candidates lie in (query, docno) order: a stable sort by the score key,
      // one by the query, and the order is (query, score descending, docno ascending)
      const unsigned g = grid_for(matches);
      sort_pairs<uint64_t>(s0, s1, p0, p1, matches, 64, radix, st);
      hipLaunchKernelGGL(k_pw_key_query, dim3(g), dim3(kNT), 0, st, (const uint32_t *)mq, (const uint32_t *)p1, matches,
                         k0);
      sort_pairs<uint32_t>(k0, k1q, p1, p0, matches, owner_bits(nq), radix, st);
      hipLaunchKernelGGL(k_pw_gather, dim3(g), dim3(kNT), 0, st, (const uint32_t *)k1q, (const uint32_t *)p0,
                         (const uint32_t *)mcand, d_cand, win, matches, (const int64_t *)woff, (const int64_t *)d_roff,
                         (int64_t)m, rows);
      SME_CHECK_LAUNCH();
    }
    int64_t win_total = 0;
    if (with_terms) {
      // (rows < 2^31: no more than the candidates)
      int64_t *d_woff = wout.offsets((int)out_total);
      int64_t *len64 = l64.as<int64_t>((size_t)out_total + 1);
      hipLaunchKernelGGL(k_pw_len64, dim3(grid_for(out_total + 1)), dim3(kNT), 0, st, (const int32_t *)rows.len,
                         out_total, len64);
      SME_CHECK_LAUNCH();
      excl_scan<int64_t>(len64, d_woff, out_total + 1, scn, st);
      SME_HIP(hipMemcpyAsync(&win_total, d_woff + out_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
      if (win_total > kMaxBatch) {
        wout.offsets(0);
        SME_HIP(hipMemsetAsync(wout.off.p, 0, sizeof(int64_t), st));
        SME_HIP(hipMemsetAsync(d_roff, 0, ((size_t)nq + 1) * sizeof(int64_t), st));
        SME_HIP(hipStreamSynchronize(st));
        throw Error(SME_ELIMIT, "passages: 2^31 or more window term entries");
      }
      int32_t *wterm = wout.alloc<WindowTerms::term>(win_total);
      int8_t *wslot = wout.alloc<WindowTerms::slot>(win_total);
      if (win_total > 0) {
        const unsigned gt = (unsigned)std::max<int64_t>(1, std::min<int64_t>((out_total + kWaves - 1) / kWaves, 65536));
        hipLaunchKernelGGL(k_pw_terms, dim3(gt), dim3(kNT), 0, st, rows, out_total, (const int64_t *)d_roff, nq,
                           (const int64_t *)d_woff, ps_off, ps_terms, ps_docno, ix->ps_records, d_sid, d_slot, d_uoff,
                           wterm, wslot);
        SME_CHECK_LAUNCH();
      }
    }
    SME_HIP(hipStreamSynchronize(st));
    out.total = out_total;
    out.cands = (uint64_t)total;
    out.matches = (uint64_t)matches;
    wout.total = win_total;
    ix->pw_with_record = h.n[C_WITH_RECORD];
    ix->pw_positions = h.n[C_POSITIONS];
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the upload may still read `blob`, kernels the temporaries
    throw;
  }
}

}  // namespace sme
