// sme_load.hip -- an index from its reduce-output record streams (the bytes of
// part-NNNNN files after their SequenceFile header), the step the reference
// takes between its two programs: TermKGramDocIndexer writes the part files,
// IntDocVectorsForwardIndex opens them (C/sa/edu/kaust/fwindex/
// BuildIntDocVectorsForwardIndex.java:84-158, IntDocVectorsForwardIndex.java:93-184).
//
//   records   Record starts are a chain (each start follows from the record
//             before).  A byte-parallel pass marks every offset where a well-formed
//             K = 1 record header or a sync escape could start (rp::header, all
//             reads bounds-checked against the partition's end) and compacts them;
//             every candidate's successor is found by binary search among the
//             candidates.  The chain from each partition's first byte is then
//             resolved by blocks of B ~ sqrt(M) candidates: per block, every
//             candidate's first successor outside the block (one thread per block,
//             B steps); one thread per partition hops from block to block (M / B
//             steps); per block, the chain inside it is marked from its entry.
//             Candidates off the chain -- header-shaped bytes inside a posting
//             list -- are never reached; a chain that ends anywhere but at its
//             partition's end names the malformed record.
//   keys      modified UTF-8 -> UTF-16, strict TermDF.compareTo order inside each
//             partition, global rank = own index + lower bounds in the other
//             partitions' sorted keys (as sme_vunion.hip ranks sources); a key
//             found in another partition is refused.
//   postings  one wave per term (tiles of 8192 postings for longer lists): big-
//             endian (docno, tf) pairs at any byte alignment from aligned dword
//             loads + v_alignbyte (rp::be32_unaligned), the mirror of ser_posts;
//             order, tf and the docno range are checked in the same pass.
//   docno     the docno-ascending order: a list of one tf run has it already; the
//             others by radix sort (kv_sort) -- tf << dbits | docno - dmin words by
//             their docno bits, then by term id, or one sort of 64-bit (term, docno)
//             keys when tf and the docno span do not share 32 bits; equal
//             neighbours are a docno repeated within a term.
//   weights   reweight_index (the build's LUT and idf tables).
//   " "       the doc-counter record's (0,0) / (docno,1) lists give d_rec_first and
//             d_rec_docno back, so k_ser_space rewrites the record byte for byte.
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>
#include <memory>
#include <string>

#include "sme_internal.hpp"
#include "sme_ixparts.hpp"
#include "sme_recparse.hpp"

namespace sme {

namespace {

constexpr int kCandPer = 16;                 // stream bytes per thread of the candidate pass
constexpr int kCandTile = 256 * kCandPer;    // per workgroup
constexpr int64_t kBigDf = 8192;             // longer posting lists are decoded in tiles of this many
constexpr int64_t kNxtEnd = -1, kNxtBad = -2;
constexpr uint64_t kNoErr = ~0ull;

// partition p with po[p] <= x < po[p + 1] (x < po[np]; empty partitions skipped)
__device__ __forceinline__ int part_of(const uint64_t *po, int np, uint64_t x) {
  int lo = 0, hi = np;
  while (hi - lo > 1) {
    const int m = (lo + hi) >> 1;
    if (po[m] <= x)
      lo = m;
    else
      hi = m;
  }
  return lo;
}
__device__ __forceinline__ int64_t lower_bound_u64(const uint64_t *a, int64_t n, uint64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (a[m] < x)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}
// the first problem wins: smallest (position, code)
__device__ __forceinline__ void report(unsigned long long *err, uint64_t pos, int code) {
  atomicMin(err, (unsigned long long)((pos << 8) | (uint64_t)code));
}

// ---- a. record starts ------------------------------------------------------
// Candidate mask of the kCandPer bytes from b0.  The thread's bytes and the 16
// after them come in as two aligned 16-byte loads; recLen, keyLen and k of
// every offset are cut from those registers, and only offsets whose three words
// could open a K = 1 record (or an escape) go through rp::header with its
// bounds checks.  The filter drops nothing header() would take: RP_OK implies
// k == 1, keyLen >= 10 and keyLen + 4 <= recLen, all inside the partition.
__device__ __forceinline__ uint32_t cand_mask(const uint8_t *__restrict__ s, uint64_t T, const uint64_t *__restrict__ po,
                                              int np, uint64_t b0) {
  uint32_t mask = 0;
  if (b0 >= T) return 0;
  int p = -1;
  auto full = [&](int e) {  // the bounds-checked header of offset b0 + e
    const uint64_t at = b0 + e;
    if (p < 0) p = part_of(po, np, at);
    while (at >= po[p + 1]) p++;
    rp::Hdr h;
    const int c = rp::header(s, at, po[p + 1], false, &h);
    if (c == rp::RP_OK || c == rp::RP_SYNC) mask |= 1u << e;
  };
  if ((((uintptr_t)(s + b0)) & 15) == 0 && b0 + 32 <= T) {
    const uint4 x = *reinterpret_cast<const uint4 *>(s + b0), y = *reinterpret_cast<const uint4 *>(s + b0 + 16);
    const uint32_t d[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
    for (int e = 0; e < kCandPer; e++) {
      const int a = e & 3, i = e >> 2;
      const int32_t rec_len = (int32_t)rp::be32_unaligned(d[i], d[i + 1], a);
      const int32_t key_len = (int32_t)rp::be32_unaligned(d[i + 1], d[i + 2], a);
      const int32_t k = (int32_t)rp::be32_unaligned(d[i + 2], d[i + 3], a);
      if (rec_len == -1 || (rec_len >= 0 && k == 1 && key_len >= 10 && (int64_t)key_len + 4 <= (int64_t)rec_len)) full(e);
    }
  } else {
    for (int e = 0; e < kCandPer && b0 + e < T; e++) full(e);
  }
  return mask;
}
// every thread's candidate mask, and the tile's count
__global__ __launch_bounds__(256) void k_cand_scan(const uint8_t *__restrict__ s, uint64_t T,
                                                   const uint64_t *__restrict__ po, int np, int64_t nblk,
                                                   uint16_t *masks, int64_t *cnt) {
  __shared__ int scr[256 / 64 + 1];
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint32_t mask = cand_mask(s, T, po, np, (uint64_t)blk * kCandTile + (uint64_t)threadIdx.x * kCandPer);
    masks[blk * 256 + threadIdx.x] = (uint16_t)mask;
    int total;
    block_excl_sum<256, int>(__popc(mask), scr, &total);
    if (threadIdx.x == 0) cnt[blk] = total;
  }
}
// the candidates in offset order from base[blk]: their offsets and the offsets they end at
__global__ __launch_bounds__(256) void k_cand_write(const uint8_t *__restrict__ s, const uint64_t *__restrict__ po,
                                                    int np, int64_t nblk, const uint16_t *masks, const int64_t *base,
                                                    uint64_t *coff, uint64_t *cend) {
  __shared__ int scr[256 / 64 + 1];
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t b0 = (uint64_t)blk * kCandTile + (uint64_t)threadIdx.x * kCandPer;
    const uint32_t mask = masks[blk * 256 + threadIdx.x];
    int total;
    const int ex = block_excl_sum<256, int>(__popc(mask), scr, &total);
    if (!mask) continue;
    int64_t o = base[blk] + ex;
    int p = part_of(po, np, b0);
    for (int e = 0; e < kCandPer; e++) {
      if (!((mask >> e) & 1u)) continue;
      const uint64_t at = b0 + e;
      while (at >= po[p + 1]) p++;
      rp::Hdr h;
      rp::header(s, at, po[p + 1], false, &h);
      coff[o] = at;
      cend[o] = at + (uint64_t)h.len;
      o++;
    }
  }
}
// successor of every candidate: the candidate starting where it ends, kNxtEnd at
// its partition's end, kNxtBad where nothing well-formed starts
__global__ void k_cand_next(const uint64_t *coff, const uint64_t *cend, int64_t M, const uint64_t *po, int np,
                            int64_t *nxt) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < M; j += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t e = cend[j];
    const int p = part_of(po, np, coff[j]);
    int64_t x = kNxtEnd;
    if (e != po[p + 1]) {
      x = lower_bound_u64(coff, M, e);
      if (x >= M || coff[x] != e) x = kNxtBad;
    }
    nxt[j] = x;
  }
}
// per block of B candidates: every candidate's first successor outside the block
// (successors lie behind their candidate, so one descending sweep resolves them)
__global__ void k_cand_exit(const int64_t *nxt, int64_t M, int64_t B, int64_t *ex) {
  const int64_t nb = (M + B - 1) / B;
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < nb; b += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j0 = b * B, j1 = min(M, j0 + B);
    for (int64_t j = j1 - 1; j >= j0; j--) {
      const int64_t x = nxt[j];
      ex[j] = (x < 0 || x >= j1) ? x : ex[x];
    }
  }
}
// one thread per partition: the chain from the partition's first byte, hopping
// from block to block; every landing candidate is flagged as its block's entry
__global__ void k_cand_walk(const uint64_t *coff, int64_t M, const int64_t *ex, const uint64_t *po, int np,
                            uint8_t *onchain, unsigned long long *err) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < np; p += gridDim.x * blockDim.x) {
    if (po[p] == po[p + 1]) continue;
    int64_t j = lower_bound_u64(coff, M, po[p]);
    if (j >= M || coff[j] != po[p]) {
      report(err, po[p], 0);
      continue;
    }
    while (j >= 0) {
      onchain[j] = 1;
      j = ex[j];
    }
  }
}
// per block: the chain inside it, forward from the flagged entries; a successor
// that is no candidate ends the chain at a malformed record
__global__ void k_cand_mark(const int64_t *nxt, const uint64_t *cend, int64_t M, int64_t B, uint8_t *onchain,
                            unsigned long long *err) {
  const int64_t nb = (M + B - 1) / B;
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < nb; b += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j0 = b * B, j1 = min(M, j0 + B);
    for (int64_t j = j0; j < j1; j++) {
      if (!onchain[j]) continue;
      const int64_t x = nxt[j];
      if (x == kNxtBad)
        report(err, cend[j], 0);
      else if (x >= 0 && x < j1)
        onchain[x] = 1;
    }
  }
}
// records = chain candidates that are no sync escape (no record has 20 bytes)
__global__ void k_cand_records(const uint64_t *coff, const uint64_t *cend, int64_t M, uint8_t *onchain) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < M; j += (int64_t)gridDim.x * blockDim.x)
    if (onchain[j] && cend[j] - coff[j] == (uint64_t)rp::kSyncLen) onchain[j] = 0;
}
__global__ void k_diagnose(const uint8_t *s, uint64_t at, uint64_t end, int *code) {
  rp::Hdr h;
  *code = rp::header(s, at, end, true, &h);
}

// ---- b. keys ---------------------------------------------------------------
struct RecInfo {
  uint64_t *at;      // record offset
  int32_t *n;        // postings
  int32_t *key_len;  // TermDF bytes
  int32_t *part;     // input partition
  int64_t *ulen;     // UTF-16 units of the key
};
__global__ void k_rec_info(const uint8_t *s, const uint64_t *coff, const int32_t *ridx, int64_t nR, const uint64_t *po,
                           int np, RecInfo ri, unsigned long long *space, unsigned long long *err) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nR; r += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t at = coff[ridx[r]];
    const int p = part_of(po, np, at);
    rp::Hdr h;
    rp::header(s, at, po[p + 1], false, &h);  // RP_OK: it was a candidate
    ri.at[r] = at;
    ri.n[r] = h.n;
    ri.key_len[r] = h.key_len;
    ri.part[r] = p;
    const int32_t nu = rp::mutf8_decode(s + rp::key_str_at(at), h.utf_len, nullptr);
    ri.ulen[r] = nu < 0 ? 0 : nu;
    if (nu < 0) {
      report(err, (uint64_t)r, rp::RP_MUTF8);
      continue;
    }
    if (h.n > 0 && !rp::class_ok(s, at, h)) report(err, (uint64_t)r, rp::RP_CLASS);
    const bool sp = h.utf_len == 1 && s[rp::key_str_at(at)] == (uint8_t)' ';
    const int32_t df = (int32_t)rp::be32(s + rp::df_at(at, h));
    if (df != (sp ? h.n : 1)) report(err, (uint64_t)r, rp::RP_DF);
    if (sp) {
      atomicAdd(&space[0], 1ull);
      atomicMin(&space[1], (unsigned long long)r);
    }
  }
}
__global__ void k_rec_chars(const uint8_t *s, const uint64_t *at, int64_t nR, const int64_t *uoff, uint16_t *tch) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nR; r += (int64_t)gridDim.x * blockDim.x)
    if (uoff[r + 1] > uoff[r]) rp::mutf8_decode(s + rp::key_str_at(at[r]), (int32_t)rp::be16(s + at[r] + 12), tch + uoff[r]);
}
// first record of every partition (pbase[np] = nR)
__global__ void k_part_base(const uint64_t *at, int64_t nR, const uint64_t *po, int np, int64_t *pbase) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p <= np; p += gridDim.x * blockDim.x)
    pbase[p] = p == np ? nR : lower_bound_u64(at, nR, po[p]);
}
// first key of records [r0, r1) that is >= s
__device__ int64_t key_bound(const int64_t *uoff, const uint16_t *tch, int64_t r0, int64_t r1, const uint16_t *s,
                             int64_t ls) {
  int64_t lo = r0, hi = r1;
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (rp::cmp_units(tch + uoff[m], uoff[m + 1] - uoff[m], s, ls) < 0)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}
// order inside the partition, and the rank over all partitions (sme_vunion.hip's k_rank
// scheme; here a key may be held by one partition only).  One thread per key: a
// thread per (key, partition) with the counts summed by atomics was slower
// (c2: 3.9 ms against 2.3).
__global__ void k_key_rank(const int64_t *uoff, const uint16_t *tch, const int32_t *part, const int64_t *pbase, int np,
                           int64_t nR, int64_t *rank, unsigned long long *err) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nR; r += (int64_t)gridDim.x * blockDim.x) {
    const int a = part[r];
    const uint16_t *s = tch + uoff[r];
    const int64_t ls = uoff[r + 1] - uoff[r];
    if (r > pbase[a] && rp::cmp_units(tch + uoff[r - 1], uoff[r] - uoff[r - 1], s, ls) >= 0)
      report(err, (uint64_t)r, rp::RP_KEY_ORDER);
    int64_t k = r - pbase[a];
    for (int b = 0; b < np; b++) {
      if (b == a || pbase[b + 1] == pbase[b]) continue;
      const int64_t lb = key_bound(uoff, tch, pbase[b], pbase[b + 1], s, ls);
      if (lb < pbase[b + 1] && rp::cmp_units(tch + uoff[lb], uoff[lb + 1] - uoff[lb], s, ls) == 0)
        report(err, (uint64_t)r, rp::RP_KEY_DUP);
      k += lb - pbase[b];
    }
    rank[r] = k;
  }
}
// terms in rank order (the " " record, rank sp_rank, taken out)
// (slen: the postings the docno sort has to take -- none for a list of one tf
// run, first tf == last tf, which is docno-ascending as it stands)
__global__ void k_term_slots(const uint8_t *s, const uint64_t *at, const int32_t *key_len, const int64_t *rank,
                             const int64_t *ulen, const int32_t *n, int64_t nR, int64_t sp_r, int64_t sp_rank,
                             int64_t *src, int64_t *tlen, int64_t *plen, int64_t *slen) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nR; r += (int64_t)gridDim.x * blockDim.x) {
    if (r == sp_r) continue;
    const int64_t t = rank[r] - (sp_r >= 0 && rank[r] > sp_rank ? 1 : 0);
    src[t] = r;
    tlen[t] = ulen[r];
    plen[t] = n[r];
    const uint64_t pat = at[r] + 8 + (uint64_t)key_len[r] + 4 + 2 + rp::kClassLen;
    slen[t] = n[r] > 1 && rp::be32(s + pat + 4) != rp::be32(s + pat + 8 * (uint64_t)(n[r] - 1) + 4) ? n[r] : 0;
  }
}

// ---- c. postings -----------------------------------------------------------
struct PostOut {
  int32_t *docno, *tf;   // reduce-order CSR
  int32_t *docno_d, *tf_d;  // docno-order CSR: written here for the lists that need no sort
  const int64_t *soff;   // offsets of the lists that do, among themselves
  uint32_t *term;        // term id of every posting (the docno sort carries it)
  unsigned int *max_tf;
  int *dmin, *dmax;
  unsigned long long *err;
};
struct PostAcc {
  uint32_t mtf = 0;
  int dmn = INT_MAX, dmx = INT_MIN;
};
// Postings [k0, k1) of term t, whose stream starts at s + pat and whose CSR slots
// start at p0.  The stream's big-endian words are read as aligned dwords (the
// dword holding a stream byte never leaves that byte's page) and realigned.
__device__ __forceinline__ void load_posts(const uint8_t *s, uint64_t pat, int64_t t, int64_t p0, int64_t k0, int64_t k1,
                                           int lane, const PostOut &o, PostAcc &acc) {
  const bool direct = o.soff[t + 1] == o.soff[t];
  const uintptr_t addr = (uintptr_t)(s + pat);
  const int a = (int)(addr & 3);
  const uint32_t *A = reinterpret_cast<const uint32_t *>(addr - a);
  for (int64_t k = k0 + lane; k < k1; k += 64) {
    const uint32_t d0 = A[2 * k], d1 = A[2 * k + 1], d2 = a ? A[2 * k + 2] : 0u;
    const int32_t dn = (int32_t)rp::be32_unaligned(d0, d1, a), tf = (int32_t)rp::be32_unaligned(d1, d2, a);
    int c = rp::post_check(dn, tf);
    if (c == rp::RP_OK && k > 0) {
      const uint32_t q0 = A[2 * k - 2], q1 = A[2 * k - 1];
      c = rp::post_pair_check((int32_t)rp::be32_unaligned(q0, q1, a), (int32_t)rp::be32_unaligned(q1, d0, a), dn, tf);
    }
    if (c != rp::RP_OK) report(o.err, (uint64_t)t, c);
    o.docno[p0 + k] = dn;
    o.tf[p0 + k] = tf;
    o.term[p0 + k] = (uint32_t)t;
    if (direct) {
      o.docno_d[p0 + k] = dn;
      o.tf_d[p0 + k] = tf;
    }
    acc.mtf = max(acc.mtf, (uint32_t)max(tf, 0));
    acc.dmn = min(acc.dmn, dn);
    acc.dmx = max(acc.dmx, dn);
  }
}
__device__ __forceinline__ void flush_acc(const PostOut &o, PostAcc &acc, int lane) {
  for (int w = 32; w > 0; w >>= 1) {
    acc.mtf = max(acc.mtf, (uint32_t)__shfl_xor((int)acc.mtf, w, 64));
    acc.dmn = min(acc.dmn, __shfl_xor(acc.dmn, w, 64));
    acc.dmx = max(acc.dmx, __shfl_xor(acc.dmx, w, 64));
  }
  // (single-address atomics serialise: only a wave that still improves a value issues one)
  if (lane == 0 && acc.dmn <= acc.dmx) {
    if (acc.mtf > *(volatile unsigned int *)o.max_tf) atomicMax(o.max_tf, acc.mtf);
    if (acc.dmn < *(volatile int *)o.dmin) atomicMin(o.dmin, acc.dmn);
    if (acc.dmx > *(volatile int *)o.dmax) atomicMax(o.dmax, acc.dmx);
  }
}
// one wave per term: its UTF-16 units, and the postings of lists up to kBigDf
__global__ __launch_bounds__(256) void k_load_terms(const uint8_t *__restrict__ s, const int64_t *src, const uint64_t *at,
                                                    const int32_t *key_len, const int64_t *uoff, const uint16_t *tch,
                                                    int64_t V, const int64_t *term_off, uint16_t *term_chars,
                                                    const int64_t *off, PostOut o) {
  const int lane = threadIdx.x & 63;
  const int64_t wpb = blockDim.x / 64;
  PostAcc acc;
  for (int64_t t = blockIdx.x * wpb + (threadIdx.x >> 6); t < V; t += (int64_t)gridDim.x * wpb) {
    const int64_t r = src[t], ul = term_off[t + 1] - term_off[t], df = off[t + 1] - off[t];
    for (int64_t i = lane; i < ul; i += 64) term_chars[term_off[t] + i] = tch[uoff[r] + i];
    if (df > 0 && df <= kBigDf)
      load_posts(s, at[r] + 8 + (uint64_t)key_len[r] + 4 + 2 + rp::kClassLen, t, off[t], 0, df, lane, o, acc);
  }
  flush_acc(o, acc, lane);
}
__global__ void k_big_flags(const int64_t *off, int64_t V, uint8_t *f) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < V; t += (int64_t)gridDim.x * blockDim.x)
    f[t] = off[t + 1] - off[t] > kBigDf;
}
__global__ void k_big_ntiles(const int32_t *big, int64_t nbig, const int64_t *off, int64_t *ntile) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j <= nbig; j += (int64_t)gridDim.x * blockDim.x)
    ntile[j] = j == nbig ? 0 : (off[big[j] + 1] - off[big[j]] + kBigDf - 1) / kBigDf;
}
// tiles of the long lists, one wave per tile (tile_off = exclusive scan of the tile counts)
__global__ __launch_bounds__(256) void k_load_big(const uint8_t *__restrict__ s, const int32_t *big, int64_t nbig,
                                                  const int64_t *tile_off, const int64_t *src, const uint64_t *at,
                                                  const int32_t *key_len, const int64_t *off, PostOut o) {
  const int lane = threadIdx.x & 63;
  const int64_t wpb = blockDim.x / 64, ntiles = tile_off[nbig];
  PostAcc acc;
  for (int64_t x = blockIdx.x * wpb + (threadIdx.x >> 6); x < ntiles; x += (int64_t)gridDim.x * wpb) {
    int64_t lo = 0, hi = nbig;  // last j with tile_off[j] <= x
    while (hi - lo > 1) {
      const int64_t m = (lo + hi) >> 1;
      if (tile_off[m] <= x)
        lo = m;
      else
        hi = m;
    }
    const int64_t t = big[lo], r = src[t], df = off[t + 1] - off[t];
    const int64_t k0 = (x - tile_off[lo]) * kBigDf, k1 = min(df, k0 + kBigDf);
    load_posts(s, at[r] + 8 + (uint64_t)key_len[r] + 4 + 2 + rp::kClassLen, t, off[t], k0, k1, lane, o, acc);
  }
  flush_acc(o, acc, lane);
}
// the " " record: map-task starts, and every record's docno from the posting
// after its own (0 where none follows: the last record of a task is never written)
__global__ __launch_bounds__(256) void k_load_counter(const uint8_t *s, uint64_t pat, int64_t N, int32_t *rec_docno,
                                                      uint8_t *first, int *dmin, int *dmax, unsigned long long *err) {
  int dmn = INT_MAX, dmx = INT_MIN;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t dn = (int32_t)rp::be32(s + pat + 8 * i), tf = (int32_t)rp::be32(s + pat + 8 * i + 4);
    const int c = rp::counter_check(i, dn, tf);
    if (c != rp::RP_OK) report(err, (uint64_t)i, c);
    first[i] = tf == 0;
    if (tf == 1) {
      dmn = min(dmn, dn);
      dmx = max(dmx, dn);
    }
    int32_t mine = 0;
    if (i + 1 < N && rp::be32(s + pat + 8 * (i + 1) + 4) == 1u) mine = (int32_t)rp::be32(s + pat + 8 * (i + 1));
    rec_docno[i] = mine;
  }
  // one atomic pair per wave (single-address atomics serialise)
  for (int w = 32; w > 0; w >>= 1) {
    dmn = min(dmn, __shfl_xor(dmn, w, 64));
    dmx = max(dmx, __shfl_xor(dmx, w, 64));
  }
  if ((threadIdx.x & 63) == 0 && dmn <= dmx) {
    atomicMin(dmin, dmn);
    atomicMax(dmax, dmx);
  }
}

// ---- d. docno order --------------------------------------------------------
// Narrow path (docno span and tf fit 32 bits together): tf << dbits | docno - dmin
// is sorted by its docno bits with the term id as value, then the pairs by term
// id (both stable): two sorts of 8-byte pairs.
__global__ void k_pack32(const int32_t *docno, const int32_t *tf, const uint32_t *term, const int64_t *off,
                         const int64_t *soff, int64_t P, int dbits, int64_t dmin, uint32_t *key, uint32_t *val) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t t = term[i];
    const int64_t s0 = soff[t];
    if (soff[t + 1] == s0) continue;
    const int64_t j = s0 + (i - off[t]);
    key[j] = ((uint32_t)tf[i] << dbits) | (uint32_t)((int64_t)docno[i] - dmin);
    val[j] = t;
  }
}
__global__ void k_docno_order32(const uint32_t *term, const uint32_t *packed, int64_t Ps, const int64_t *off,
                                const int64_t *soff, int dbits, int64_t dmin, int32_t *docno_d, int32_t *tf_d,
                                unsigned long long *err) {
  const uint32_t dmask = (uint32_t)((1ull << dbits) - 1);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < Ps; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t v = packed[i], t = term[i];
    if (i > 0 && term[i - 1] == t && (packed[i - 1] & dmask) == (v & dmask)) report(err, (uint64_t)t, rp::RP_DOCNO_DUP);
    const int64_t g = off[t] + (i - soff[t]);
    docno_d[g] = (int32_t)((int64_t)(v & dmask) + dmin);
    tf_d[g] = (int32_t)(v >> dbits);
  }
}
// Wide path: (term << dbits | docno - dmin) 64-bit keys, the posting index as value.
__global__ void k_pack64(const int32_t *docno, const uint32_t *term, const int64_t *off, const int64_t *soff, int64_t P,
                         int dbits, int64_t dmin, uint64_t *key, uint32_t *val) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t t = term[i];
    const int64_t s0 = soff[t];
    if (soff[t + 1] == s0) continue;
    const int64_t j = s0 + (i - off[t]);
    key[j] = ((uint64_t)t << dbits) | (uint64_t)((int64_t)docno[i] - dmin);
    val[j] = (uint32_t)i;
  }
}
__global__ void k_docno_order64(const uint64_t *key, const uint32_t *val, int64_t Ps, const int64_t *off,
                                const int64_t *soff, int dbits, int64_t dmin, const int32_t *tf_o, int32_t *docno_d,
                                int32_t *tf_d, unsigned long long *err) {
  const uint64_t dmask = (1ull << dbits) - 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < Ps; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = key[i], t = k >> dbits;
    if (i > 0 && key[i - 1] == k) report(err, t, rp::RP_DOCNO_DUP);
    const int64_t g = off[t] + (i - soff[t]);
    docno_d[g] = (int32_t)((int64_t)(k & dmask) + dmin);
    tf_d[g] = tf_o[val[i]];
  }
}

[[noreturn]] void refuse(int code, const std::string &where) {
  const int sc = code == rp::RP_KGRAM ? SME_ENOTIMPL : (code == rp::RP_TF_LIMIT ? SME_ELIMIT : SME_EPARSE);
  throw Error(sc, std::string(rp::message(code)) + " (" + where + ")");
}

}  // namespace

sme_index *load_records(sme_ctx *cx, const uint8_t *s, const uint64_t *part_offsets, int np, hipStream_t st) {
  if (np < 0 || (np > 0 && !part_offsets)) throw Error(SME_EINVAL, "bad partition table");
  if (cx->cfg.k != 1) throw Error(SME_ENOTIMPL, "loading K >= 2 record streams");
  std::vector<uint64_t> hpo((size_t)np + 1, 0);
  for (int p = 0; p <= np && np > 0; p++) {
    hpo[p] = part_offsets[p];
    if (p > 0 && hpo[p] < hpo[p - 1]) throw Error(SME_EINVAL, "partition offsets decrease");
  }
  if (np > 0 && hpo[0] != 0) throw Error(SME_EINVAL, "partition offsets must start at 0");
  const uint64_t T = hpo[np];
  if (T > 0 && !s) throw Error(SME_EINVAL, "null record stream");
  auto &W = cx->ws;
  Prof prof(st, &cx->prof_events);

  sme_index *ix = new sme_index(cx);
  std::unique_ptr<sme_index> guard(ix);
  ix->K = 1;
  ix->R = cx->cfg.num_partitions;
  ix->idf_mode = cx->cfg.idf_mode;
  ix->from_records = true;
  ix->rec_complete = false;  // k_load_counter stores 0 for every map task's last docno

  uint64_t *po = W[0].as<uint64_t>((size_t)np + 2);
  SME_HIP(hipMemcpyAsync(po, hpo.data(), ((size_t)np + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  // [0] first problem, [1] " " records, [2] the first of them
  unsigned long long *err = W[1].as<unsigned long long>(4);
  const unsigned long long h_init[3] = {kNoErr, 0ull, kNoErr};
  SME_HIP(hipMemcpyAsync(err, h_init, sizeof h_init, hipMemcpyHostToDevice, st));
  auto where_of = [&](uint64_t at) {
    int p = 0;
    while (p + 1 < np && hpo[p + 1] <= at) p++;
    return "partition " + std::to_string(p) + ", byte " + std::to_string(at - hpo[p]);
  };

  // ---------------- a. record starts ----------------
  int64_t nR = 0;
  const uint64_t *coff = nullptr;
  const int32_t *ridx = nullptr;
  if (T > 0) {
    const int64_t nblk = (int64_t)((T + kCandTile - 1) / kCandTile);
    int64_t *cnt = W[2].as<int64_t>((size_t)nblk + 1), *base = W[3].as<int64_t>((size_t)nblk + 1);
    const unsigned cg = (unsigned)std::min<int64_t>(nblk, 65536);
    uint16_t *masks = W[36].as<uint16_t>((size_t)nblk * 256);
    hipLaunchKernelGGL(k_cand_scan, dim3(cg), dim3(256), 0, st, s, T, po, np, nblk, masks, cnt);
    SME_CHECK_LAUNCH();
    SME_HIP(hipMemsetAsync(cnt + nblk, 0, sizeof(int64_t), st));
    excl_scan<int64_t>(cnt, base, nblk + 1, W[4], st);
    const int64_t M = rd1(base + nblk, st);
    if (M > 0x7FFFFFFFll) throw Error(SME_ELIMIT, "more than 2^31 record candidates");
    uint64_t *co = W[5].as<uint64_t>((size_t)M + 1), *ce = W[6].as<uint64_t>((size_t)M + 1);
    if (M > 0)
      hipLaunchKernelGGL(k_cand_write, dim3(cg), dim3(256), 0, st, s, po, np, nblk, masks, base, co, ce);
    prof.mark("scan_candidates");
    int64_t *nxt = W[7].as<int64_t>((size_t)M + 1), *ex = W[8].as<int64_t>((size_t)M + 1);
    uint8_t *onchain = W[9].as<uint8_t>((size_t)M + 1);
    SME_HIP(hipMemsetAsync(onchain, 0, (size_t)M, st));
    if (M > 0) hipLaunchKernelGGL(k_cand_next, dim3(grid_n(M)), dim3(256), 0, st, co, ce, M, po, np, nxt);
    int64_t B = 64;
    while (B < 4096 && B * B < M) B <<= 1;
    const int64_t nb = (M + B - 1) / B;
    if (M > 0) hipLaunchKernelGGL(k_cand_exit, dim3(grid_n(nb, 64)), dim3(64), 0, st, nxt, M, B, ex);
    if (M > 0) hipLaunchKernelGGL(k_cand_walk, dim3(grid_n(np, 64)), dim3(64), 0, st, co, M, ex, po, np, onchain, err);
    if (M > 0) hipLaunchKernelGGL(k_cand_mark, dim3(grid_n(nb, 64)), dim3(64), 0, st, nxt, ce, M, B, onchain, err);
    SME_CHECK_LAUNCH();
    unsigned long long e = rd1(err, st);
    if (M == 0)  // nothing record-shaped anywhere: the first partition with bytes starts malformed
      for (int p = np - 1; p >= 0; p--)
        if (hpo[p + 1] > hpo[p]) e = hpo[p] << 8;
    if (e != kNoErr) {  // the chain stops short of its partition's end: name what is there
      const uint64_t at = e >> 8;
      int p = 0;
      while (p + 1 < np && hpo[p + 1] <= at) p++;
      int *d_code = reinterpret_cast<int *>(err + 3);
      hipLaunchKernelGGL(k_diagnose, dim3(1), dim3(1), 0, st, s, at, hpo[p + 1], d_code);
      SME_CHECK_LAUNCH();
      int code = rd1(d_code, st);
      if (code == rp::RP_OK || code == rp::RP_SYNC) code = rp::RP_KEYLEN;  // (cannot be: it would be a candidate)
      refuse(code, where_of(at));
    }
    hipLaunchKernelGGL(k_cand_records, dim3(grid_n(M)), dim3(256), 0, st, co, ce, M, onchain);
    int32_t *ri = W[10].as<int32_t>((size_t)M + 1), *d_n = W[11].as<int32_t>(4);
    select_flagged(onchain, M, ri, d_n, W[12], W[4], st);
    nR = rd1(d_n, st);
    coff = co;
    ridx = ri;
  }
  prof.mark("scan_records");

  // ---------------- b. keys ----------------
  RecInfo ri;
  ri.at = W[13].as<uint64_t>((size_t)nR + 1);
  ri.n = W[14].as<int32_t>((size_t)nR + 1);
  ri.key_len = W[15].as<int32_t>((size_t)nR + 1);
  ri.part = W[16].as<int32_t>((size_t)nR + 1);
  ri.ulen = W[17].as<int64_t>((size_t)nR + 2);
  int64_t *uoff = W[18].as<int64_t>((size_t)nR + 2);
  int64_t sp_r = -1, sp_rank = -1, V = 0;
  int64_t *rank = W[20].as<int64_t>((size_t)nR + 1), *pbase = W[21].as<int64_t>((size_t)np + 2);
  uint16_t *tch = nullptr;
  auto check_err = [&](const char *unit) {
    const unsigned long long e = rd1(err, st);
    if (e != kNoErr) refuse((int)(e & 0xFF), std::string(unit) + " " + std::to_string(e >> 8));
  };
  if (nR > 0) {
    hipLaunchKernelGGL(k_rec_info, dim3(grid_n(nR)), dim3(256), 0, st, s, coff, ridx, nR, po, np, ri, err + 1, err);
    SME_CHECK_LAUNCH();
    SME_HIP(hipMemsetAsync(ri.ulen + nR, 0, sizeof(int64_t), st));
    excl_scan<int64_t>(ri.ulen, uoff, nR + 1, W[4], st);
    check_err("record");
    unsigned long long h_sp[2];
    SME_HIP(hipMemcpyAsync(h_sp, err + 1, sizeof h_sp, hipMemcpyDeviceToHost, st));
    const int64_t nunits = rd1(uoff + nR, st);
    if (h_sp[0] > 1) refuse(rp::RP_SPACE_MANY, std::to_string(h_sp[0]) + " records");
    if (h_sp[0] == 0) refuse(rp::RP_SPACE_NONE, std::to_string(nR) + " records");
    sp_r = (int64_t)h_sp[1];
    tch = W[19].as<uint16_t>((size_t)nunits + 1);
    hipLaunchKernelGGL(k_rec_chars, dim3(grid_n(nR)), dim3(256), 0, st, s, ri.at, nR, uoff, tch);
    hipLaunchKernelGGL(k_part_base, dim3(grid_n(np + 1, 64)), dim3(64), 0, st, ri.at, nR, po, np, pbase);
    SME_CHECK_LAUNCH();
    prof.mark("keys");
    hipLaunchKernelGGL(k_key_rank, dim3(grid_n(nR)), dim3(256), 0, st, uoff, tch, ri.part, pbase, np, nR, rank, err);
    SME_CHECK_LAUNCH();
    check_err("record");
    sp_rank = rd1(rank + sp_r, st);
    V = nR - 1;
  } else {
    prof.mark("keys");
  }
  ix->V = ix->Vt = V;
  int64_t *term_off = ix->d_term_off.as<int64_t>((size_t)V + 1), *off = ix->d_off.as<int64_t>((size_t)V + 1);
  int64_t *src = W[22].as<int64_t>((size_t)V + 1);
  int64_t *soff = W[40].as<int64_t>((size_t)V + 1);
  int64_t P = 0, tchars = 0, Ps = 0;  // Ps: postings of the lists the docno sort takes
  if (V > 0) {
    int64_t *tlen = W[23].as<int64_t>((size_t)V + 1), *plen = W[24].as<int64_t>((size_t)V + 1);
    int64_t *slen = W[39].as<int64_t>((size_t)V + 1);
    hipLaunchKernelGGL(k_term_slots, dim3(grid_n(nR)), dim3(256), 0, st, s, ri.at, ri.key_len, rank, ri.ulen, ri.n, nR,
                       sp_r, sp_rank, src, tlen, plen, slen);
    SME_CHECK_LAUNCH();
    SME_HIP(hipMemsetAsync(tlen + V, 0, sizeof(int64_t), st));
    SME_HIP(hipMemsetAsync(plen + V, 0, sizeof(int64_t), st));
    excl_scan<int64_t>(tlen, term_off, V + 1, W[4], st);
    SME_HIP(hipMemsetAsync(slen + V, 0, sizeof(int64_t), st));
    excl_scan<int64_t>(plen, off, V + 1, W[4], st);
    excl_scan<int64_t>(slen, soff, V + 1, W[4], st);
    tchars = rd1(term_off + V, st);
    P = rd1(off + V, st);
    Ps = rd1(soff + V, st);
  } else {
    SME_HIP(hipMemsetAsync(term_off, 0, sizeof(int64_t), st));
    SME_HIP(hipMemsetAsync(off, 0, sizeof(int64_t), st));
    SME_HIP(hipMemsetAsync(soff, 0, sizeof(int64_t), st));
  }
  if (P > 0xFFFFFFFFll) throw Error(SME_ELIMIT, "term sort of more than 2^32 pairs");
  ix->P = P;
  prof.mark("merge_terms");

  // ---------------- c. postings ----------------
  uint16_t *term_chars = ix->d_term_chars.as<uint16_t>((size_t)tchars + 1);
  PostOut o;
  o.docno = ix->d_docno_o.as<int32_t>((size_t)P + 1);
  o.tf = ix->d_tf_o.as<int32_t>((size_t)P + 1);
  o.term = W[26].as<uint32_t>((size_t)P + 1);
  o.docno_d = ix->d_docno_d.as<int32_t>((size_t)P + 1);
  o.tf_d = ix->d_tf_d.as<int32_t>((size_t)P + 1);
  o.soff = soff;
  int *stats = W[27].as<int>(4);  // max_tf, dmin, dmax
  const int h_stats[3] = {0, INT_MAX, INT_MIN};
  SME_HIP(hipMemcpyAsync(stats, h_stats, sizeof h_stats, hipMemcpyHostToDevice, st));
  o.max_tf = reinterpret_cast<unsigned int *>(stats);
  o.dmin = stats + 1;
  o.dmax = stats + 2;
  o.err = err;
  if (V > 0) {
    hipLaunchKernelGGL(k_load_terms, dim3((unsigned)std::min<int64_t>((V + 3) / 4, 65536)), dim3(256), 0, st, s, src,
                       ri.at, ri.key_len, uoff, tch, V, term_off, term_chars, off, o);
    SME_CHECK_LAUNCH();
    uint8_t *bflag = W[28].as<uint8_t>((size_t)V + 1);
    int32_t *big = W[29].as<int32_t>((size_t)V + 1), *d_nbig = W[11].as<int32_t>(4);
    hipLaunchKernelGGL(k_big_flags, dim3(grid_n(V)), dim3(256), 0, st, off, V, bflag);
    select_flagged(bflag, V, big, d_nbig, W[12], W[4], st);
    const int32_t nbig = rd1(d_nbig, st);
    if (nbig > 0) {
      int64_t *ntile = W[30].as<int64_t>((size_t)nbig + 1), *tile_off = W[31].as<int64_t>((size_t)nbig + 1);
      hipLaunchKernelGGL(k_big_ntiles, dim3(grid_n(nbig + 1)), dim3(256), 0, st, big, (int64_t)nbig, off, ntile);
      excl_scan<int64_t>(ntile, tile_off, nbig + 1, W[4], st);
      hipLaunchKernelGGL(k_load_big, dim3(8192), dim3(256), 0, st, s, big, (int64_t)nbig, tile_off, src, ri.at,
                         ri.key_len, off, o);
      SME_CHECK_LAUNCH();
    }
  }
  // the doc counter
  int64_t N = 0;
  if (sp_r >= 0) {
    N = rd1(ri.n + sp_r, st);
    if (N == 0) refuse(rp::RP_COUNTER, "an empty list");
    const uint64_t sp_at = rd1(ri.at + sp_r, st);
    int32_t *rdn = ix->d_rec_docno.as<int32_t>((size_t)N + 1);
    uint8_t *fst = ix->d_rec_first.as<uint8_t>((size_t)N + 1);
    if (N > 0)
      hipLaunchKernelGGL(k_load_counter, dim3(grid_n(N)), dim3(256), 0, st, s, sp_at + 8 + 11 + 4 + 2 + rp::kClassLen, N,
                         rdn, fst, o.dmin, o.dmax, err);
    SME_CHECK_LAUNCH();
  } else {
    ix->d_rec_docno.get(16);
  }
  ix->N = N;
  {
    const unsigned long long e = rd1(err, st);
    if (e != kNoErr) {
      const int code = (int)(e & 0xFF);
      refuse(code, std::string(code == rp::RP_COUNTER ? "\" \" posting " : "term ") + std::to_string(e >> 8));
    }
  }
  int h_st[3];
  SME_HIP(hipMemcpyAsync(h_st, stats, sizeof h_st, hipMemcpyDeviceToHost, st));
  SME_HIP(hipStreamSynchronize(st));
  ix->max_tf = std::max(1, h_st[0]);
  if (h_st[1] <= h_st[2]) {
    ix->dmin = h_st[1];
    ix->dmax = h_st[2];
  }
  prof.mark("postings");

  // ---------------- d. docno order ----------------
  int32_t *docno_d = o.docno_d, *tf_d = o.tf_d;
  if (Ps > 0) {
    const int dbits = bits_of((uint64_t)(ix->dmax - ix->dmin));
    const int tbits = bits_of((uint64_t)std::max<int64_t>(V - 1, 1));
    uint32_t *rscr = W[34].as<uint32_t>(kv_sort_scratch(Ps) / sizeof(uint32_t) + 1);
    if (dbits + bits_of((uint64_t)ix->max_tf) <= 32) {
      uint32_t *ka = W[25].as<uint32_t>((size_t)Ps + 1), *kb = W[32].as<uint32_t>((size_t)Ps + 1);
      uint32_t *va = W[35].as<uint32_t>((size_t)Ps + 1), *vb = W[33].as<uint32_t>((size_t)Ps + 1);
      hipLaunchKernelGGL(k_pack32, dim3(grid_n(P)), dim3(256), 0, st, o.docno, o.tf, o.term, off, soff, P, dbits,
                         ix->dmin, ka, va);
      // by docno (the packed word's low bits), the term ids riding along ...
      uint32_t *t1 = kv_sort<uint32_t>(ka, va, kb, vb, Ps, dbits, rscr, st, true);
      uint32_t *p1 = t1 == va ? ka : kb;
      // ... then by term id, the packed words riding along
      uint32_t *t_free = t1 == va ? vb : va, *p_free = t1 == va ? kb : ka;
      const uint32_t *p2 = kv_sort<uint32_t>(t1, p1, t_free, p_free, Ps, tbits, rscr, st, true);
      const uint32_t *t2 = p2 == p1 ? t1 : t_free;
      hipLaunchKernelGGL(k_docno_order32, dim3(grid_n(Ps)), dim3(256), 0, st, t2, p2, Ps, off, soff, dbits, ix->dmin,
                         docno_d, tf_d, err);
    } else {
      uint64_t *k0 = W[37].as<uint64_t>((size_t)Ps + 1), *k1 = W[38].as<uint64_t>((size_t)Ps + 1);
      uint32_t *v0 = W[25].as<uint32_t>((size_t)Ps + 1), *v1 = W[33].as<uint32_t>((size_t)Ps + 1);
      hipLaunchKernelGGL(k_pack64, dim3(grid_n(P)), dim3(256), 0, st, o.docno, o.term, off, soff, P, dbits, ix->dmin, k0,
                         v0);
      const uint32_t *vs = kv_sort<uint64_t>(k0, v0, k1, v1, Ps, tbits + dbits, rscr, st, true);
      const uint64_t *ks = vs == v0 ? k0 : k1;
      hipLaunchKernelGGL(k_docno_order64, dim3(grid_n(Ps)), dim3(256), 0, st, ks, vs, Ps, off, soff, dbits, ix->dmin,
                         o.tf, docno_d, tf_d, err);
    }
    SME_CHECK_LAUNCH();
    check_err("term");
  }
  const uint32_t *term_of = P > 0 ? o.term : nullptr;  // both CSR orders share the term offsets
  prof.mark("docno_order");

  // ---------------- weights ----------------
  ix->d_idf.as<double>((size_t)V + 1);
  ix->d_w.as<double>((size_t)P + 1);
  reweight_index(ix, N, nullptr, st, term_of);
  prof.mark("weights");
  ix->profile = prof.finish();
  guard.release();
  return ix;
}

}  // namespace sme
