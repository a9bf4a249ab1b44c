// sme_feedback.hip -- relevance feedback: a batch of document sets, each a list of
// docnos -> per set the terms of those documents' kept streams with their
// occurrences (freq), the set's documents holding them (docs) and the score
// (1 + ln freq) * idf, filtered, ordered by score and cut to the first m.  The
// one pass that goes from documents to terms: it reads the forward index a K = 1
// build kept (d_ps_off / d_ps_terms / d_ps_docno); include/sme.h has the semantics.
//
// The records of a docno are adjacent (d_ps_docno ascends) and so are their streams,
// so a document is ONE run of d_ps_terms.  k_fb_plan finds every set's runs;
// k_fb_agg counts a set's terms in an LDS hash table, one workgroup per set; a set
// with more distinct terms than the table's load limit is redone by the large path
// -- a key per position, one stable sort, a segmented reduce -- which has no size
// cliff.  Both leave (set, term, freq, docs) pairs; the filter, the score, three
// stable sorts (term, score, set) and the cut follow.
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sme_bool.hpp"
#include "sme_chunks.hpp"
#include "sme_feedback.hpp"
#include "sme_internal.hpp"

namespace sme {
namespace {
using namespace chunks;

constexpr int kEmpty = -1;  // an unused table slot, an unused pair slot: no stream holds a negative term id
constexpr int64_t kSetGrid = 1 << 20;

inline unsigned set_grid(int n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(n, kSetGrid)); }

enum { C_POSITIONS, C_MISSING, C_SPILLED, C_PAIRS, C_COUNT };  // the call's device counters

// One workgroup per set, grid-strided.  Entry j of the set survives if it is not -1
// and no earlier entry holds the same docno; a survivor's records are ps_docno[r0 ..
// r1) (two bounds), its stream the run [ps_off[r0], ps_off[r1]).  The survivors
// with a record, in entry order, are the set's documents: document k's run start,
// length and positions before it in the set go to dp0 / dlen / dstart[f0 + k].
// Per set: ndoc, spos = its positions, bound = the pair slots the on-chip path may
// fill, min(spos, limit).  A set of 2^31 positions or more lowers *badset to itself.
__global__ __launch_bounds__(kNT) void k_fb_plan(const int32_t *__restrict__ docnos, const int64_t *__restrict__ foff,
                                                 int nq, const int64_t *__restrict__ ps_off,
                                                 const int32_t *__restrict__ ps_docno, int64_t nR, int limit,
                                                 int64_t *__restrict__ dp0, int64_t *__restrict__ dlen,
                                                 int64_t *__restrict__ dstart, int32_t *__restrict__ ndoc,
                                                 int64_t *__restrict__ spos, int64_t *__restrict__ bound,
                                                 unsigned long long *__restrict__ counters, int *__restrict__ badset) {
  __shared__ int32_t s_doc[feedback::kMaxEntries];
  __shared__ int64_t s_p0[feedback::kMaxEntries], s_len[feedback::kMaxEntries];
  __shared__ int s_scr[kNT / 64 + 1];
  __shared__ int s_missing;
  const int tid = threadIdx.x;
  for (int i = blockIdx.x; i < nq; i += gridDim.x) {
    const int64_t f0 = foff[i];
    const int n = (int)(foff[i + 1] - f0);  // <= kMaxEntries (validated on the host)
    for (int j = tid; j < n; j += kNT) s_doc[j] = docnos[f0 + j];
    if (tid == 0) s_missing = 0;
    __syncthreads();
    int run = 0;  // documents of the rounds before
    for (int rd = 0; rd < n; rd += kNT) {
      const int j = rd + tid;
      bool has = false;
      int64_t p0 = 0, len = 0;
      if (j < n) {
        const int32_t d = s_doc[j];
        bool keep = d != -1;
        for (int e = 0; keep && e < j; e++) keep = s_doc[e] != d;
        if (keep) {
          const int64_t r0 = lower_bound(ps_docno, nR, d);
          const int64_t r1 = r0 + upper_bound(ps_docno + r0, nR - r0, d);
          if (r1 > r0) {
            has = true;
            p0 = ps_off[r0];
            len = ps_off[r1] - p0;
          } else {
            atomicAdd(&s_missing, 1);
          }
        }
      }
      int tot = 0;
      const int at = block_excl_sum<kNT, int>(has ? 1 : 0, s_scr, &tot);
      if (has) {
        s_p0[run + at] = p0;
        s_len[run + at] = len;
      }
      run += tot;
    }
    __syncthreads();
    for (int k = tid; k < run; k += kNT) {
      dp0[f0 + k] = s_p0[k];
      dlen[f0 + k] = s_len[k];
    }
    if (tid == 0) {
      int64_t acc = 0;
      for (int k = 0; k < run; k++) {
        dstart[f0 + k] = acc;
        acc += s_len[k];
      }
      ndoc[i] = run;
      spos[i] = acc;
      bound[i] = acc < limit ? acc : limit;
      if (acc) atomicAdd(&counters[C_POSITIONS], (unsigned long long)acc);
      if (s_missing) atomicAdd(&counters[C_MISSING], (unsigned long long)s_missing);
      if (acc >= (int64_t(1) << 31)) atomicMin(badset, i);
    }
    __syncthreads();  // the next set rewrites the LDS
  }
}

// Term t of document tag (= ordinal + 1, ascending from one document to the next,
// a barrier in between) into the table: linear probing from a multiplicative hash;
// the slot's term is claimed by a compare-and-swap, its freq counted by an atomic
// add, and its third word holds tag << 16 | docs -- the first lane of a document to
// reach the slot moves the tag and adds one to docs, the others find the tag in
// place.  True if the table is past its load limit or full: the set spills.
__device__ __forceinline__ bool fb_insert(int32_t *tterm, uint32_t *tfreq, uint32_t *ttag, int slots, int shift,
                                          int32_t t, uint32_t tag, int limit, int *count) {
  bool over = false;
  uint32_t s = ((uint32_t)t * 2654435761u) >> shift;
  for (int probe = 0; probe < slots; probe++, s = (s + 1) & (uint32_t)(slots - 1)) {
    int32_t cur = __hip_atomic_load(&tterm[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == kEmpty) {
      cur = atomicCAS(&tterm[s], kEmpty, t);
      if (cur == kEmpty) {
        over = atomicAdd(count, 1) >= limit;
        cur = t;
      }
    }
    if (cur != t) continue;
    atomicAdd(&tfreq[s], 1u);
    uint32_t v = __hip_atomic_load(&ttag[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while ((v >> 16) != tag) {
      const uint32_t old = atomicCAS(&ttag[s], v, (tag << 16) | ((v & 0xFFFFu) + 1));
      if (old == v) break;
      v = old;
    }
    return over;
  }
  return true;  // no slot left
}

// The on-chip path: one workgroup per set, grid-strided, over a table of `slots`
// entries in dynamic LDS (term | freq | tag and docs: 12 bytes a slot).  The set's
// documents are taken one after another; consecutive lanes read consecutive stream
// words, four loads in flight per lane.  A set that stays within the load limit
// writes its table's entries to the pair slots base[i] + 0 .. count - 1 (count <=
// bound[i]); one that passes it writes nothing and is marked in spill[i].
__global__ __launch_bounds__(kNT) void k_fb_agg(const int64_t *__restrict__ foff, int nq,
                                                const int64_t *__restrict__ dp0, const int64_t *__restrict__ dlen,
                                                const int32_t *__restrict__ ndoc, const int64_t *__restrict__ spos,
                                                const int32_t *__restrict__ ps_terms, int slots, int shift, int limit,
                                                const int64_t *__restrict__ base, uint32_t *__restrict__ pset,
                                                int32_t *__restrict__ pterm, int32_t *__restrict__ pfreq,
                                                int32_t *__restrict__ pdocs, uint8_t *__restrict__ spill) {
  extern __shared__ uint32_t fb_table[];
  int32_t *tterm = (int32_t *)fb_table;
  uint32_t *tfreq = fb_table + slots, *ttag = fb_table + 2 * slots;
  __shared__ int s_count, s_emit, s_over;
  const int tid = threadIdx.x;
  for (int i = blockIdx.x; i < nq; i += gridDim.x) {
    if (spos[i] == 0) {  // (the same in every thread)
      if (tid == 0) spill[i] = 0;
      continue;
    }
    for (int s = tid; s < slots; s += kNT) {
      tterm[s] = kEmpty;
      tfreq[s] = 0;
      ttag[s] = 0;
    }
    if (tid == 0) s_count = s_emit = s_over = 0;
    __syncthreads();
    const int64_t f0 = foff[i];
    const int nd = ndoc[i];
    int over = 0;
    for (int k = 0; k < nd && !over; k++) {
      const int32_t *__restrict__ ts = ps_terms + dp0[f0 + k];
      const int64_t len = dlen[f0 + k];  // < 2^31: the host refuses a larger set before this launch
      bool mine = false;
      for (int64_t p = tid; p < len; p += 4 * kNT) {
        int32_t t[4];
#pragma unroll
        for (int u = 0; u < 4; u++) t[u] = p + u * kNT < len ? ts[p + u * kNT] : kEmpty;
#pragma unroll
        for (int u = 0; u < 4; u++)
          if (t[u] >= 0) mine |= fb_insert(tterm, tfreq, ttag, slots, shift, t[u], (uint32_t)k + 1, limit, &s_count);
      }
      if (mine) s_over = 1;
      __syncthreads();  // the document is counted: the next one's tag may move
      over = s_over;
      __syncthreads();  // (read by all before the next document may set it)
    }
    if (!over) {
      const int64_t b = base[i];
      for (int s = tid; s < slots; s += kNT) {
        const int32_t t = tterm[s];
        if (t == kEmpty) continue;
        const int64_t x = b + atomicAdd(&s_emit, 1);
        pset[x] = (uint32_t)i;
        pterm[x] = t;
        pfreq[x] = (int32_t)tfreq[s];
        pdocs[x] = (int32_t)(ttag[s] & 0xFFFFu);
      }
    }
    if (tid == 0) spill[i] = over ? 1 : 0;
    __syncthreads();  // the next set clears the table
  }
}

// lpos[i] = the positions set i sends through the large path (entry nq = 0)
__global__ void k_fb_lplan(const uint8_t *__restrict__ spill, const int64_t *__restrict__ spos, int nq,
                           int64_t *__restrict__ lpos, unsigned long long *__restrict__ counters) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nq; i += (int64_t)gridDim.x * blockDim.x) {
    const bool sp = i < nq && spill[i];
    lpos[i] = sp ? spos[i] : 0;
    if (sp) atomicAdd(&counters[C_SPILLED], 1ull);
  }
}

// The large path's emit, one workgroup per spilled set: position p of document k is
// entry lbase[i] + dstart[f0 + k] + p -- document order -- with the key set << 32 |
// term and the value k.
__global__ __launch_bounds__(kNT) void k_fb_lemit(const int64_t *__restrict__ foff, int nq,
                                                  const int64_t *__restrict__ dp0, const int64_t *__restrict__ dlen,
                                                  const int64_t *__restrict__ dstart, const int32_t *__restrict__ ndoc,
                                                  const uint8_t *__restrict__ spill, const int64_t *__restrict__ lbase,
                                                  const int32_t *__restrict__ ps_terms, uint64_t *__restrict__ key,
                                                  uint32_t *__restrict__ val) {
  for (int i = blockIdx.x; i < nq; i += gridDim.x) {
    if (!spill[i]) continue;
    const int64_t f0 = foff[i];
    const int nd = ndoc[i];
    for (int k = 0; k < nd; k++) {
      const int32_t *__restrict__ ts = ps_terms + dp0[f0 + k];
      const int64_t len = dlen[f0 + k], at = lbase[i] + dstart[f0 + k];
      for (int64_t p = threadIdx.x; p < len; p += kNT) {
        key[at + p] = ((uint64_t)(uint32_t)i << 32) | (uint32_t)ts[p];
        val[at + p] = (uint32_t)k;
      }
    }
  }
}
// over the sorted keys: head[x] = entry x starts a run of equal keys, chg[x] = it
// starts a run or its document differs from the entry before (values ascend within
// a run: the sort is stable); entry E of both = 0
__global__ void k_fb_lflags(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, int64_t E,
                            uint8_t *__restrict__ head, int32_t *__restrict__ chg) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x <= E; x += (int64_t)gridDim.x * blockDim.x) {
    const bool h = x < E && (x == 0 || key[x] != key[x - 1]);
    head[x] = h;
    chg[x] = x < E && (h || val[x] != val[x - 1]);
  }
}
// run r of the sorted keys, [hidx[r], hidx[r + 1]) (the last one ends at E): its
// length is freq, the document changes inside it (pc: chg scanned) are docs
__global__ void k_fb_lpairs(const uint64_t *__restrict__ key, const int32_t *__restrict__ hidx, int64_t H, int64_t E,
                            const int32_t *__restrict__ pc, uint32_t *__restrict__ pset, int32_t *__restrict__ pterm,
                            int32_t *__restrict__ pfreq, int32_t *__restrict__ pdocs) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < H; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = hidx[r], b = r + 1 < H ? (int64_t)hidx[r + 1] : E;
    const uint64_t k = key[a];
    pset[r] = (uint32_t)(k >> 32);
    pterm[r] = (int32_t)(uint32_t)k;
    pfreq[r] = (int32_t)(b - a);
    pdocs[r] = pc[b] - pc[a];
  }
}

// The pair slots of both paths as one array of B + H: the on-chip path's first
// (unused slots hold term kEmpty and freq 0), the large path's after them.
struct Pairs {
  const uint32_t *set[2];
  const int32_t *term[2], *freq[2], *docs[2];
  int64_t B;
  __device__ __forceinline__ int side(int64_t &x) const {
    if (x < B) return 0;
    x -= B;
    return 1;
  }
};

struct Filter {
  int32_t min_docs, min_df, max_df;
  const int64_t *doff;   // the index's posting offsets: df(t) = doff[t + 1] - doff[t]
  const int64_t *xoff;   // [nq + 1] exclusion offsets, or NULL
  const int32_t *xterm;  // every set's exclusion ids, ascending within the set
};
// flag[x] = pair slot x holds a pair that passes the filters; C_PAIRS += the slots
// holding one, summed per workgroup first: one atomic per wave and round on the one
// counter took 57.7 of a 147 ms call over 307 M slots
__global__ __launch_bounds__(kNT) void k_fb_filter(Pairs p, int64_t S, Filter f, uint8_t *__restrict__ flag,
                                                   unsigned long long *__restrict__ counters) {
  __shared__ unsigned int s_valid;
  if (threadIdx.x == 0) s_valid = 0;
  __syncthreads();
  unsigned int mine = 0;  // (per wave: the same in all its lanes)
  for (int64_t x0 = blockIdx.x * (int64_t)blockDim.x; x0 < S; x0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t x = x0 + threadIdx.x;
    bool valid = false, keep = false;
    if (x < S) {
      int64_t y = x;
      const int a = p.side(y);
      const int32_t t = p.term[a][y];
      valid = t != kEmpty;
      if (valid) {
        const int64_t df = f.doff[t + 1] - f.doff[t];
        keep = p.docs[a][y] >= f.min_docs && df >= f.min_df && (f.max_df == 0 || df <= f.max_df);
        if (keep && f.xoff) {
          const uint32_t s = p.set[a][y];
          const int64_t b = f.xoff[s];
          const int n = (int)(f.xoff[s + 1] - b);
          const int at = lower_bound(f.xterm + b, n, t);
          keep = !(at < n && f.xterm[b + at] == t);
        }
      }
      flag[x] = keep;
    }
    mine += (unsigned int)__popcll(__ballot(valid));
  }
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_valid, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_valid) atomicAdd(&counters[C_PAIRS], (unsigned long long)s_valid);
}

// kept pair x (pair slot idx[x]): its set, term, counts and score = lut[freq] *
// idf[term], the product k_weights forms for a posting.  freq < lut_n: the table
// was sized from the largest freq of the pair slots.
__global__ void k_fb_score(const int32_t *__restrict__ idx, int64_t T, Pairs p, const double *__restrict__ lut,
                           const double *__restrict__ idf, uint32_t *__restrict__ mset, int32_t *__restrict__ mterm,
                           int32_t *__restrict__ mfreq, int32_t *__restrict__ mdocs, double *__restrict__ mscore) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < T; x += (int64_t)gridDim.x * blockDim.x) {
    int64_t y = idx[x];
    const int a = p.side(y);
    const int32_t t = p.term[a][y], fq = p.freq[a][y];
    mset[x] = p.set[a][y];
    mterm[x] = t;
    mfreq[x] = fq;
    mdocs[x] = p.docs[a][y];
    mscore[x] = __dmul_rn(lut[fq], idf[t]);
  }
}
__global__ void k_fb_key_term(const int32_t *__restrict__ mterm, int64_t n, uint32_t *__restrict__ key,
                              uint32_t *__restrict__ perm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    key[i] = (uint32_t)mterm[i];
    perm[i] = (uint32_t)i;
  }
}
__global__ void k_fb_key_score(const double *__restrict__ mscore, const uint32_t *__restrict__ perm, int64_t n,
                               uint64_t *__restrict__ key) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    key[i] = boolq::score_key(mscore[perm[i]]);
}
__global__ void k_fb_key_set(const uint32_t *__restrict__ mset, const uint32_t *__restrict__ perm, int64_t n,
                             uint32_t *__restrict__ key) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    key[i] = mset[perm[i]];
}
// woff[i] = kept pairs of the sets before i in the sorted set keys (entry nq: all)
__global__ void k_fb_offs(const uint32_t *__restrict__ qs, int64_t T, int nq, int64_t *__restrict__ woff) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nq; i += (int64_t)gridDim.x * blockDim.x)
    woff[i] = i < nq ? lower_bound(qs, T, (uint32_t)i) : T;
}
// ordered pair x (set qs[x], kept pair perm[x]) is the (x - woff[set])-th of its
// set: written if that is below the cut
__global__ void k_fb_gather(const uint32_t *__restrict__ qs, const uint32_t *__restrict__ perm,
                            const int32_t *__restrict__ mterm, const int32_t *__restrict__ mfreq,
                            const int32_t *__restrict__ mdocs, const double *__restrict__ mscore, int64_t T,
                            const int64_t *__restrict__ woff, const int64_t *__restrict__ roff, int64_t m,
                            int32_t *__restrict__ out_term, int32_t *__restrict__ out_freq,
                            int32_t *__restrict__ out_docs, double *__restrict__ out_score) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < T; x += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t q = qs[x];
    const int64_t rk = x - woff[q];
    if (m > 0 && rk >= m) continue;
    const uint32_t i = perm[x];
    const int64_t at = roff[q] + rk;
    out_term[at] = mterm[i];
    out_freq[at] = mfreq[i];
    out_docs[at] = mdocs[i];
    out_score[at] = mscore[i];
  }
}

int log2_of(int64_t pow2) {
  int b = 0;
  while ((int64_t(1) << b) < pow2) b++;
  return b;
}
}  // namespace

void feedback_terms(sme_index *ix, const int32_t *docnos, bool on_device, const int64_t *f_offsets, int nq,
                    const int32_t *x_ids, const int64_t *x_offsets, int m, int min_docs, int min_df, int max_df,
                    hipStream_t st) {
  int bad = -1;
  const int rc = feedback::validate(f_offsets, -1, nq, x_ids, -1, x_offsets, ix->V, &bad);
  if (rc != feedback::F_OK) {
    char msg[128];
    const bool limit = feedback::describe(rc, bad, msg, sizeof msg);
    throw Error(limit ? SME_ELIMIT : SME_EINVAL, msg);
  }
  sme_ctx *cx = ix->ctx;
  TermFreqDocsScores &out = ix->fb;
  out.reset();
  ix->fb_positions = ix->fb_pairs = ix->fb_kept = ix->fb_missing = ix->fb_spilled = 0;
  int64_t *d_roff = out.offsets(nq);
  SME_HIP(hipMemsetAsync(d_roff, 0, ((size_t)nq + 1) * sizeof(int64_t), st));
  if (nq == 0) {
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  const int slots = (int)cx->opt_fb_slots, limit = feedback::load_limit(slots), shift = 32 - log2_of(slots);
  const int64_t nE = f_offsets[nq];  // entries of the batch, < 2^31
  // one upload: set offsets | exclusion offsets | exclusion ids, each set's ascending
  Blob blob;
  const size_t a_foff = blob.add(f_offsets, (size_t)nq + 1);
  size_t a_xoff = 0, a_xterm = 0;
  const bool excl = x_offsets && x_offsets[nq] > 0;
  if (excl) {
    std::vector<int32_t> xs(x_ids, x_ids + x_offsets[nq]);
    for (int i = 0; i < nq; i++) std::sort(xs.begin() + x_offsets[i], xs.begin() + x_offsets[i + 1]);
    a_xoff = blob.add(x_offsets, (size_t)nq + 1);
    a_xterm = blob.add(xs.data(), xs.size());
  }
  // temporaries of this call: pooled blocks, back in the pool on return
  DevBuf dnb, in, p0b, lnb, dsb, ndb, spb, bnb, cnb, scn, spl, sa, ta, fa, da, lpb, kb0, kb1, vb0, vb1, hdb, chb, pcb, hib, s1b,
      s2b, sb, tb, fb, db, flb, idb, mxb, msb, mtb, mfb, mdb, mcb, ka, kb, pa, pb, ska, skb, wob, keb, radix;
  for (DevBuf *b : {&dnb, &in,  &p0b, &lnb, &dsb, &ndb, &spb, &bnb, &cnb, &scn, &spl, &sa,  &ta,  &fa,  &da,  &lpb, &kb0,
                    &kb1, &vb0, &vb1, &hdb, &chb, &pcb, &hib, &s1b, &s2b, &sb,  &tb,  &fb,  &db,  &flb, &idb, &mxb,
                    &msb, &mtb, &mfb, &mdb, &mcb, &ka,  &kb,  &pa,  &pb,  &ska, &skb, &wob, &keb, &radix})
    b->pool = &cx->pool;
  try {
    const uint8_t *d_in = in.as<uint8_t>(blob.bytes.size());
    SME_HIP(hipMemcpyAsync((void *)d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st));
    const int64_t *foff = (const int64_t *)(d_in + a_foff);
    const int32_t *d_docnos = docnos;
    if (!on_device) {  // the host entry's docnos: uploaded; the caller's array lives through the call
      int32_t *d = dnb.as<int32_t>((size_t)nE);
      if (nE) SME_HIP(hipMemcpyAsync(d, docnos, (size_t)nE * sizeof(int32_t), hipMemcpyHostToDevice, st));
      d_docnos = d;
    }
    const int64_t *ps_off = (const int64_t *)ix->d_ps_off.p;
    const int32_t *ps_terms = (const int32_t *)ix->d_ps_terms.p;
    const int32_t *ps_docno = (const int32_t *)ix->d_ps_docno.p;
    // ---- plan
    int64_t *dp0 = p0b.as<int64_t>((size_t)nE), *dlen = lnb.as<int64_t>((size_t)nE), *dstart = dsb.as<int64_t>((size_t)nE);
    int32_t *ndoc = ndb.as<int32_t>((size_t)nq);
    int64_t *spos = spb.as<int64_t>((size_t)nq), *base = bnb.as<int64_t>((size_t)nq + 1);
    // the counters, then the first set past the position limit
    unsigned long long *d_cnt = cnb.as<unsigned long long>(C_COUNT + 1), h_cnt[C_COUNT + 1];
    int *d_bad = reinterpret_cast<int *>(d_cnt + C_COUNT);
    int h_bad = INT_MAX;
    SME_HIP(hipMemsetAsync(d_cnt, 0, C_COUNT * sizeof(unsigned long long), st));
    SME_HIP(hipMemcpyAsync(d_bad, &h_bad, sizeof h_bad, hipMemcpyHostToDevice, st));
    SME_HIP(hipMemsetAsync(base + nq, 0, sizeof(int64_t), st));
    const unsigned gs = set_grid(nq);
    hipLaunchKernelGGL(k_fb_plan, dim3(gs), dim3(kNT), 0, st, d_docnos, foff, nq, ps_off, ps_docno, ix->ps_records, limit,
                       dp0, dlen, dstart, ndoc, spos, base, d_cnt, d_bad);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(base, base, (int64_t)nq + 1, scn, st);
    int64_t B = 0;  // pair slots of the on-chip path
    SME_HIP(hipMemcpyAsync(&B, base + nq, sizeof B, hipMemcpyDeviceToHost, st));
    SME_HIP(hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    if (h_bad != INT_MAX)
      throw Error(SME_ELIMIT, "feedback terms: set " + std::to_string(h_bad) + ": 2^31 or more stream positions");
    const char *many = "feedback terms: 2^31 or more (set, term) pairs in one batch";
    if (B >= (int64_t(1) << 31)) throw Error(SME_ELIMIT, many);
    // ---- the on-chip path
    uint8_t *spill = spl.as<uint8_t>((size_t)nq);
    uint32_t *aset = sa.as<uint32_t>((size_t)B);
    int32_t *aterm = ta.as<int32_t>((size_t)B), *afreq = fa.as<int32_t>((size_t)B), *adocs = da.as<int32_t>((size_t)B);
    if (B > 0) {
      SME_HIP(hipMemsetAsync(aterm, 0xFF, (size_t)B * sizeof(int32_t), st));  // kEmpty
      SME_HIP(hipMemsetAsync(afreq, 0, (size_t)B * sizeof(int32_t), st));
    }
    hipLaunchKernelGGL(k_fb_agg, dim3(gs), dim3(kNT), (size_t)slots * feedback::kSlotBytes, st, foff, nq,
                       (const int64_t *)dp0, (const int64_t *)dlen, (const int32_t *)ndoc, (const int64_t *)spos,
                       ps_terms, slots, shift, limit, (const int64_t *)base, aset, aterm, afreq, adocs, spill);
    SME_CHECK_LAUNCH();
    int64_t *lbase = lpb.as<int64_t>((size_t)nq + 1);
    hipLaunchKernelGGL(k_fb_lplan, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, (const uint8_t *)spill,
                       (const int64_t *)spos, nq, lbase, d_cnt);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(lbase, lbase, (int64_t)nq + 1, scn, st);
    int64_t E = 0, H = 0;  // positions of the spilled sets; their (set, term) pairs
    SME_HIP(hipMemcpyAsync(&E, lbase + nq, sizeof E, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    // ---- the large path
    uint32_t *bset = nullptr;
    int32_t *bterm = nullptr, *bfreq = nullptr, *bdocs = nullptr;
    if (E >= (int64_t(1) << 31))
      throw Error(SME_ELIMIT, "feedback terms: 2^31 or more stream positions in the sets past the on-chip table");
    if (E > 0) {
      uint64_t *k0 = kb0.as<uint64_t>((size_t)E), *k1 = kb1.as<uint64_t>((size_t)E);
      uint32_t *v0 = vb0.as<uint32_t>((size_t)E), *v1 = vb1.as<uint32_t>((size_t)E);
      hipLaunchKernelGGL(k_fb_lemit, dim3(gs), dim3(kNT), 0, st, foff, nq, (const int64_t *)dp0, (const int64_t *)dlen,
                         (const int64_t *)dstart, (const int32_t *)ndoc, (const uint8_t *)spill, (const int64_t *)lbase,
                         ps_terms, k0, v0);
      SME_CHECK_LAUNCH();
      sort_pairs<uint64_t>(k0, k1, v0, v1, E, 32 + owner_bits(nq), radix, st);
      uint8_t *head = hdb.as<uint8_t>((size_t)E + 1);
      int32_t *chg = chb.as<int32_t>((size_t)E + 1), *pc = pcb.as<int32_t>((size_t)E + 1);
      int32_t *hidx = hib.as<int32_t>((size_t)E + 1);
      int32_t *d_H = reinterpret_cast<int32_t *>(d_bad);  // (the limit flag has been read)
      hipLaunchKernelGGL(k_fb_lflags, dim3(grid_for(E + 1)), dim3(kNT), 0, st, (const uint64_t *)k1,
                         (const uint32_t *)v1, E, head, chg);
      SME_CHECK_LAUNCH();
      SME_HIP(hipMemsetAsync(d_H, 0, sizeof(int32_t), st));
      select_flagged(head, E, hidx, d_H, s1b, s2b, st);
      excl_scan<int32_t>(chg, pc, E + 1, scn, st);
      int32_t h32 = 0;
      SME_HIP(hipMemcpyAsync(&h32, d_H, sizeof h32, hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
      H = h32;
      bset = sb.as<uint32_t>((size_t)H);
      bterm = tb.as<int32_t>((size_t)H), bfreq = fb.as<int32_t>((size_t)H), bdocs = db.as<int32_t>((size_t)H);
      hipLaunchKernelGGL(k_fb_lpairs, dim3(grid_for(H)), dim3(kNT), 0, st, (const uint64_t *)k1, (const int32_t *)hidx,
                         H, E, (const int32_t *)pc, bset, bterm, bfreq, bdocs);
      SME_CHECK_LAUNCH();
    }
    const int64_t S = B + H;
    if (S >= (int64_t(1) << 31)) throw Error(SME_ELIMIT, many);
    const Pairs pairs{{aset, bset}, {aterm, bterm}, {afreq, bfreq}, {adocs, bdocs}, B};
    // ---- filter; the largest freq sizes the scorer table
    int64_t T = 0, out_total = 0;
    if (S > 0) {
      uint8_t *flag = flb.as<uint8_t>((size_t)S);
      int32_t *idx = idb.as<int32_t>((size_t)S + 1);
      int32_t *d_max = mxb.as<int32_t>(3), h_max[3] = {0, 0, 0};  // largest freq of either side; kept pairs
      const Filter f{min_docs, min_df, max_df, (const int64_t *)ix->d_off.p,
                     excl ? (const int64_t *)(d_in + a_xoff) : nullptr,
                     excl ? (const int32_t *)(d_in + a_xterm) : nullptr};
      hipLaunchKernelGGL(k_fb_filter, dim3(grid_for(S)), dim3(kNT), 0, st, pairs, S, f, flag, d_cnt);
      SME_CHECK_LAUNCH();
      SME_HIP(hipMemsetAsync(d_max, 0, 3 * sizeof(int32_t), st));
      select_flagged(flag, S, idx, d_max + 2, s1b, s2b, st);
      if (B > 0) reduce_max<int32_t>(afreq, B, d_max, st);
      if (H > 0) reduce_max<int32_t>(bfreq, H, d_max + 1, st);
      SME_HIP(hipMemcpyAsync(h_max, d_max, sizeof h_max, hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
      T = h_max[2];
      if (T > 0) {
        grow_score_lut(ix, std::max<int64_t>((int64_t)std::max(h_max[0], h_max[1]), ix->max_tf) + 1, st);
        // ---- score, order, cut
        uint32_t *mset = msb.as<uint32_t>((size_t)T);
        int32_t *mterm = mtb.as<int32_t>((size_t)T), *mfreq = mfb.as<int32_t>((size_t)T);
        int32_t *mdocs = mdb.as<int32_t>((size_t)T);
        double *mscore = mcb.as<double>((size_t)T);
        const unsigned g = grid_for(T);
        hipLaunchKernelGGL(k_fb_score, dim3(g), dim3(kNT), 0, st, (const int32_t *)idx, T, pairs,
                           (const double *)ix->d_nq_lut.p, (const double *)ix->d_idf.p, mset, mterm, mfreq, mdocs,
                           mscore);
        // a stable sort by term, by the score key, then by set leaves (set, score
        // descending, term ascending) whichever order the pairs stood in
        uint32_t *k0 = ka.as<uint32_t>((size_t)T), *k1 = kb.as<uint32_t>((size_t)T);
        uint32_t *p0 = pa.as<uint32_t>((size_t)T), *p1 = pb.as<uint32_t>((size_t)T);
        uint64_t *s0 = ska.as<uint64_t>((size_t)T), *s1 = skb.as<uint64_t>((size_t)T);
        hipLaunchKernelGGL(k_fb_key_term, dim3(g), dim3(kNT), 0, st, (const int32_t *)mterm, T, k0, p0);
        sort_pairs<uint32_t>(k0, k1, p0, p1, T, owner_bits(ix->V), radix, st);
        hipLaunchKernelGGL(k_fb_key_score, dim3(g), dim3(kNT), 0, st, (const double *)mscore, (const uint32_t *)p1, T,
                           s0);
        sort_pairs<uint64_t>(s0, s1, p1, p0, T, 64, radix, st);
        hipLaunchKernelGGL(k_fb_key_set, dim3(g), dim3(kNT), 0, st, (const uint32_t *)mset, (const uint32_t *)p0, T, k0);
        sort_pairs<uint32_t>(k0, k1, p0, p1, T, owner_bits(nq), radix, st);
        int64_t *woff = wob.as<int64_t>((size_t)nq + 1), *kept = keb.as<int64_t>((size_t)nq + 1);
        hipLaunchKernelGGL(k_fb_offs, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, (const uint32_t *)k1, T, nq,
                           woff);
        hipLaunchKernelGGL(k_cut, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, (const int64_t *)woff, (int64_t)nq,
                           (int64_t)m, kept);
        SME_CHECK_LAUNCH();
        excl_scan<int64_t>(kept, d_roff, (int64_t)nq + 1, scn, st);
        SME_HIP(hipMemcpyAsync(&out_total, d_roff + nq, sizeof out_total, hipMemcpyDeviceToHost, st));
        SME_HIP(hipStreamSynchronize(st));
        int32_t *out_term = out.alloc<TermFreqDocsScores::term>(out_total);
        int32_t *out_freq = out.alloc<TermFreqDocsScores::freq>(out_total);
        int32_t *out_docs = out.alloc<TermFreqDocsScores::docs>(out_total);
        double *out_score = out.alloc<TermFreqDocsScores::score>(out_total);
        hipLaunchKernelGGL(k_fb_gather, dim3(g), dim3(kNT), 0, st, (const uint32_t *)k1, (const uint32_t *)p1,
                           (const int32_t *)mterm, (const int32_t *)mfreq, (const int32_t *)mdocs,
                           (const double *)mscore, T, (const int64_t *)woff, (const int64_t *)d_roff, (int64_t)m,
                           out_term, out_freq, out_docs, out_score);
        SME_CHECK_LAUNCH();
      }
    }
    SME_HIP(hipMemcpyAsync(h_cnt, d_cnt, C_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    out.total = out_total;
    ix->fb_positions = h_cnt[C_POSITIONS];
    ix->fb_missing = h_cnt[C_MISSING];
    ix->fb_spilled = h_cnt[C_SPILLED];
    ix->fb_pairs = h_cnt[C_PAIRS];
    ix->fb_kept = (uint64_t)T;
  } catch (...) {
    (void)hipStreamSynchronize(st);  // the upload may still read the blob, kernels the temporaries
    throw;
  }
}

}  // namespace sme
