// sme_posfile.hip -- the term streams of an index as a file, and back
// (sme_index_positions_file*, sme_index_attach_positions*; include/sme.h has the
// format and the semantics, DESIGN.md 4m the passes and their measurements).
//
//   digest      one thread per term hashes (t, its UTF-16 units) with FNV-1a-64; the
//               sums meet by wave shuffles and LDS, one 64-bit add per workgroup
//   encode      one workgroup per tile of kTile positions: the ids loaded 16 bytes a
//               lane into LDS, then every 32-bit word of the tile's bit string put
//               together from the one to 33 ids it covers and stored, consecutive
//               lanes on consecutive words.  A tile is whole 64-bit words, so no two
//               workgroups share one: no atomics, no per-position global store
//   records     docno[] and len[] of the file checked (ascending docnos, zero padding)
//               and copied; excl_scan of the lengths gives d_ps_off, its last entry
//               must be the header's position count
//   decode      the mirror of encode: the tile's words into LDS, every lane takes its
//               four ids out of the one or two words each straddles, tests them
//               against V, stores 16 bytes; the smallest offending position goes to
//               one word by atomicMin, once per wave that saw one
//   crosscheck  a zeroed int32 counter per posting; every position finds its posting
//               (id, docno of its record) by a lower bound in the term's docno-order
//               list and adds one; a second pass compares the counters with d_tf_d.
//               The first (term, docno) without a posting or with another count goes
//               to one word by atomicMin
//
// An attach decodes into buffers of its own and hands them to the index only when
// every check has passed: a refused file leaves the index as it was.  The file is
// not trusted: nothing is read through a count before the header's size
// arithmetic has held it to the byte count, and the cross-check, the only pass that
// indexes by a stream id, runs after the decode has seen every id below V.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sme_chunks.hpp"
#include "sme_internal.hpp"
#include "sme_ixparts.hpp"
#include "sme_posfile.hpp"

namespace sme {

namespace {

using namespace posfile;

constexpr int kNT = 256;
constexpr int kPer = kTile / kNT;  // ids per lane: one 16-byte access
static_assert(kPer == 4 && kTile % 64 == 0, "a lane moves one int4; a tile is whole words");
constexpr int64_t kGridCap = 65536;  // workgroups of a launch, at most
constexpr unsigned long long kNone = ~0ull;
// the error words of an attach
enum { E_DOCNO = 0, E_ID = 1, E_PAD = 2, E_CROSS = 3, E_INTERNAL = 4, E_WORDS = 8 };

void swap_buf(DevBuf &a, DevBuf &b) {  // both of one pool
  std::swap(a.p, b.p);
  std::swap(a.cap, b.cap);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
// the cross-check's order of (term, docno): term ascending, then signed docno ascending
__device__ __forceinline__ unsigned long long cross_key(int64_t t, int32_t d) {
  return ((unsigned long long)t << 32) | ((uint32_t)d ^ 0x80000000u);
}

// ---- digest -------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void k_pf_digest(const int64_t *__restrict__ toff, const uint16_t *__restrict__ chars,
                                                   int64_t V, unsigned long long *__restrict__ out) {
  __shared__ unsigned long long s_sum[kNT / 64];
  unsigned long long acc = 0;
  for (int64_t t = blockIdx.x * (int64_t)kNT + threadIdx.x; t < V; t += (int64_t)gridDim.x * kNT) {
    const int64_t a = toff[t];
    acc += term_hash((uint64_t)t, chars + a, toff[t + 1] - a);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0;
    for (int w = 0; w < kNT / 64; w++) sum += s_sum[w];
    atomicAdd(out, sum);  // an integer sum: the same bits whatever the grid
  }
}

// ---- writing ------------------------------------------------------------------------
// docno[] and len[] of the file with their zero padding (n odd: one more entry each)
__global__ void k_pf_sections(const int32_t *__restrict__ ps_docno, const int64_t *__restrict__ ps_off, int64_t n,
                              int32_t *__restrict__ fdocno, uint32_t *__restrict__ flen) {
  const int64_t padded = (n + 1) & ~int64_t(1);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < padded; i += (int64_t)gridDim.x * blockDim.x) {
    fdocno[i] = i < n ? ps_docno[i] : 0;
    flen[i] = i < n ? (uint32_t)(ps_off[i + 1] - ps_off[i]) : 0u;
  }
}

// ids: T stream ids, 16-byte aligned; w32: the file's words as 2 ceil(T b / 64) 32-bit halves
__global__ __launch_bounds__(kNT) void k_pf_encode(const int32_t *__restrict__ ids, int64_t T, int b, uint32_t V,
                                                   int64_t ntiles, uint32_t *__restrict__ w32,
                                                   unsigned long long *__restrict__ err) {
  __shared__ __attribute__((aligned(16))) int32_t s_id[kTile];
  const int tid = threadIdx.x, q = tid * kPer;
  bool bad = false;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t p0 = t * (int64_t)kTile;
    const int n = (int)min((int64_t)kTile, T - p0);
    int4 v = make_int4(0, 0, 0, 0);
    if (q + kPer <= n) {
      v = *reinterpret_cast<const int4 *>(ids + p0 + q);
    } else if (q < n) {
      v.x = ids[p0 + q];
      if (q + 1 < n) v.y = ids[p0 + q + 1];
      if (q + 2 < n) v.z = ids[p0 + q + 2];
    }
    // (an id outside [0, V) would spill into its neighbour's bits: the streams never hold one)
    bad |= (uint32_t)v.x >= V || (uint32_t)v.y >= V || (uint32_t)v.z >= V || (uint32_t)v.w >= V;
    *reinterpret_cast<int4 *>(s_id + q) = v;
    __syncthreads();
    const int nw = n == kTile ? kTile / 32 * b : 2 * (int)(((int64_t)n * b + 63) >> 6);
    const int64_t base = (p0 >> 5) * b;
    for (int w = tid; w < nw; w += kNT) w32[base + w] = word32_of(s_id, b, w);
    __syncthreads();  // the next tile's ids overwrite s_id
  }
  if (__ballot(bad) && (tid & 63) == 0) atomicMin(err + E_INTERNAL, 1ull);
}

// ---- attaching ----------------------------------------------------------------------
// The file's docno[] and len[] checked and copied: docno ascending (the first record
// below its predecessor to err[E_DOCNO]), zero padding; len[] widened for the scan
// (n + 1 entries, the last 0).
__global__ void k_pf_records(const int32_t *__restrict__ fdocno, const uint32_t *__restrict__ flen, int64_t n,
                             int32_t *__restrict__ docno, int64_t *__restrict__ len,
                             unsigned long long *__restrict__ err) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n) {
      const int32_t d = fdocno[i];
      docno[i] = d;
      len[i] = (int64_t)flen[i];
      if (i > 0 && fdocno[i - 1] > d) atomicMin(err + E_DOCNO, (unsigned long long)i);
    } else {
      len[n] = 0;
      if ((n & 1) && (fdocno[n] != 0 || flen[n] != 0u)) atomicMin(err + E_PAD, 0ull);  // the sections' padding
    }
  }
}

// w32: the file's words as 32-bit halves; ids: T decoded ids, 16-byte aligned.  The
// smallest position whose id is not below V goes to err[E_ID]; a set bit past the
// last position's to err[E_PAD].
__global__ __launch_bounds__(kNT) void k_pf_decode(const uint32_t *__restrict__ w32, int64_t T, int b, uint32_t V,
                                                   int64_t ntiles, int32_t *__restrict__ ids,
                                                   unsigned long long *__restrict__ err) {
  __shared__ uint32_t s_w[kTileWords32 + 1];  // id_of reads one word past an id's first
  const int tid = threadIdx.x, q = tid * kPer;
  unsigned long long first = kNone;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t p0 = t * (int64_t)kTile;
    const int n = (int)min((int64_t)kTile, T - p0);
    const int nw = n == kTile ? kTile / 32 * b : 2 * (int)(((int64_t)n * b + 63) >> 6);
    const int64_t base = (p0 >> 5) * b;
    for (int w = tid; w <= kTile / 32 * b; w += kNT) s_w[w] = w < nw ? w32[base + w] : 0u;
    __syncthreads();
    uint32_t id[kPer];
#pragma unroll
    for (int j = 0; j < kPer; j++) {
      id[j] = q + j < n ? id_of(s_w, b, q + j) : 0u;
      if (q + j < n && id[j] >= V && first == kNone) first = (unsigned long long)(p0 + q + j);
    }
    if (q + kPer <= n) {
      *reinterpret_cast<int4 *>(ids + p0 + q) = make_int4((int)id[0], (int)id[1], (int)id[2], (int)id[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kPer; j++)
        if (q + j < n) ids[p0 + q + j] = (int32_t)id[j];
    }
    if (tid == 0 && n < kTile) {  // the last tile: the bits past position n - 1, to the end of its last word
      const int bit = n * b;
      for (int w = bit >> 5; w < nw; w++) {
        const uint32_t x = w == (bit >> 5) ? s_w[w] >> (bit & 31) : s_w[w];
        if (x) atomicMin(err + E_PAD, 1ull);
      }
    }
    __syncthreads();  // the next tile's words overwrite s_w
  }
  first = wave_min(first);
  if ((tid & 63) == 0 && first != kNone) atomicMin(err + E_ID, first);
}

// Every position adds one to the counter of its posting (its id, the docno of its
// record); one without a posting reports (id, docno).  Needs every id below V and
// ps_off ascending from 0 to T: the decode and the scan have checked both.
// (The flat row walk of sme_ixparts.hpp's for_row_elements, kept as its own text:
// through the template the cross-check measured 1 % slower, 64.3 ms against 63.7.)
__global__ __launch_bounds__(kNT) void k_pf_count(const int32_t *__restrict__ ids, int64_t T,
                                                  const int64_t *__restrict__ ps_off,
                                                  const int32_t *__restrict__ ps_docno, int64_t nrec,
                                                  const int64_t *__restrict__ off, const int32_t *__restrict__ docno_d,
                                                  int64_t ntiles, int32_t *__restrict__ cnt,
                                                  unsigned long long *__restrict__ err) {
  __shared__ int64_t s_r[2];
  unsigned long long first = kNone;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t p0 = t * (int64_t)kTile, p1 = min(T, p0 + kTile);
    // the tile's window of records: the last record starting at or before a position holds it
    if (threadIdx.x < 2) s_r[threadIdx.x] = chunks::upper_bound(ps_off, nrec + 1, threadIdx.x ? p1 - 1 : p0) - 1;
    __syncthreads();
    const int64_t r0 = s_r[0], r1 = s_r[1];
    for (int64_t p = p0 + threadIdx.x; p < p1; p += kNT) {
      const int64_t r = r0 + chunks::upper_bound(ps_off + r0, r1 - r0 + 1, p) - 1;
      const int32_t d = ps_docno[r];
      const int64_t term = ids[p], lo = off[term], hi = off[term + 1];
      const int64_t i = lo + chunks::lower_bound(docno_d + lo, hi - lo, d);
      if (i < hi && docno_d[i] == d)
        atomicAdd(cnt + i, 1);
      else
        first = min(first, cross_key(term, d));
    }
    __syncthreads();  // s_r is rewritten
  }
  first = wave_min(first);
  if ((threadIdx.x & 63) == 0 && first != kNone) atomicMin(err + E_CROSS, first);
}

// every posting's counter against its tf; the term of a posting that disagrees is
// searched for only then
__global__ void k_pf_compare(const int32_t *__restrict__ cnt, const int32_t *__restrict__ tf_d,
                             const int32_t *__restrict__ docno_d, int64_t P, const int64_t *__restrict__ off, int64_t V,
                             unsigned long long *__restrict__ err) {
  unsigned long long first = kNone;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x)
    if (cnt[i] != tf_d[i]) first = min(first, cross_key(chunks::upper_bound(off, V + 1, i) - 1, docno_d[i]));
  first = wave_min(first);
  if ((threadIdx.x & 63) == 0 && first != kNone) atomicMin(err + E_CROSS, first);
}

float stage_ms(const std::vector<std::pair<std::string, float>> &prof, const char *name) {
  for (const auto &p : prof)
    if (p.first == name) return p.second;
  return 0.0f;
}

// *d_word = the digest of the index's vocabulary (read it after a synchronisation)
void vocabulary_digest(sme_index *ix, unsigned long long *d_word, hipStream_t st) {
  SME_HIP(hipMemsetAsync(d_word, 0, sizeof(unsigned long long), st));
  if (ix->V > 0) {
    hipLaunchKernelGGL(k_pf_digest, dim3(grid_n(ix->V, kNT, 4096)), dim3(kNT), 0, st, (const int64_t *)ix->d_term_off.p,
                       (const uint16_t *)ix->d_term_chars.p, ix->V, d_word);
    SME_CHECK_LAUNCH();
  }
}

void refuse_call(const CallDesc &c) {
  const int rc = validate_call(c);
  if (rc == C_OK) return;
  char msg[200];
  describe_call(rc, c, msg, sizeof msg);
  throw Error(SME_EINVAL, msg);
}

}  // namespace

void positions_file(sme_index *ix, int bits, hipStream_t st) {
  sme_ctx *cx = ix->ctx;
  ix->pf_bytes = ix->pf_bits = ix->pf_checked = 0;
  ix->pf_encode_ms = ix->pf_decode_ms = ix->pf_crosscheck_ms = 0.0f;
  const int64_t Rn = ix->ps_records, T = ix->ps_terms, V = ix->V;
  const int b = bits ? bits : need_bits((uint64_t)V);
  Layout lay;
  if (Rn >= (int64_t)kLimit || T >= (int64_t)kLimit || !layout((uint64_t)Rn, (uint64_t)T, (uint32_t)b, &lay))
    throw Error(SME_ELIMIT, "positions file: 2^31 or more records or term positions");
  Prof prof(st, &cx->prof_events);
  DevBuf werr;
  werr.pool = &cx->pool;
  unsigned long long *d_err = werr.as<unsigned long long>(E_WORDS);  // [0] the digest, [E_INTERNAL] the flag
  SME_HIP(hipMemsetAsync(d_err, 0xFF, E_WORDS * sizeof(unsigned long long), st));
  uint8_t *file = ix->d_pf_file.as<uint8_t>((size_t)lay.size);

  vocabulary_digest(ix, d_err, st);
  const uint64_t digest = rd1(d_err, st);
  prof.mark("digest");

  uint8_t hdr[kHeaderBytes];
  write_header(hdr, Header{kVersion, (uint32_t)b, (uint64_t)Rn, (uint64_t)T, (uint64_t)V, digest});
  SME_HIP(hipMemcpyAsync(file, hdr, kHeaderBytes, hipMemcpyHostToDevice, st));
  if (Rn > 0) {
    hipLaunchKernelGGL(k_pf_sections, dim3(grid_n(Rn + 1, kNT, kGridCap)), dim3(kNT), 0, st, (const int32_t *)ix->d_ps_docno.p,
                       (const int64_t *)ix->d_ps_off.p, Rn, reinterpret_cast<int32_t *>(file + lay.docno_at),
                       reinterpret_cast<uint32_t *>(file + lay.len_at));
    SME_CHECK_LAUNCH();
  }
  SME_HIP(hipStreamSynchronize(st));  // hdr is the host's again
  prof.mark("sections");

  const int64_t ntiles = (T + kTile - 1) / kTile;
  if (T > 0) {
    hipLaunchKernelGGL(k_pf_encode, dim3(grid_n(ntiles, 1, kGridCap)), dim3(kNT), 0, st, (const int32_t *)ix->d_ps_terms.p, T, b,
                       (uint32_t)V, ntiles, reinterpret_cast<uint32_t *>(file + lay.words_at), d_err);
    SME_CHECK_LAUNCH();
  }
  prof.mark("encode");
  const auto profile = prof.finish();  // waits for the stream
  if (rd1(d_err + E_INTERNAL, st) != kNone)
    throw Error(SME_EHIP, "positions file: a stream id outside the vocabulary (internal)");
  cx->last_profile = profile;
  ix->pf_bytes = lay.size;
  ix->pf_bits = (uint64_t)b;
  ix->pf_encode_ms = stage_ms(profile, "encode");
}

void check_positions_file_call(const sme_index *ix, bool has_args, int bits) {
  refuse_call(CallDesc{false, has_args && ix != nullptr, ix ? ix->job : 0, ix ? ix->K : 1, ix && ix->records_only,
                       ix && ix->has_positions, ix ? (uint64_t)ix->V : 0, bits, 0});
}

void attach_positions(sme_index *ix, const uint8_t *h_file, const void *d_file, size_t n, int flags, bool has_args,
                      hipStream_t st) {
  refuse_call(CallDesc{true, has_args && ix != nullptr && (h_file != nullptr || d_file != nullptr), ix ? ix->job : 0,
                       ix ? ix->K : 1, ix && ix->records_only, ix && ix->has_positions, ix ? (uint64_t)ix->V : 0, 0,
                       flags});
  if (!h_file && ((uintptr_t)d_file & 7)) throw Error(SME_EINVAL, "positions attach: the device file is not 8-byte aligned");
  sme_ctx *cx = ix->ctx;
  ix->pf_bytes = ix->pf_bits = ix->pf_checked = 0;
  ix->pf_encode_ms = ix->pf_decode_ms = ix->pf_crosscheck_ms = 0.0f;
  const int64_t N = ix->N, V = ix->V, P = ix->P;

  // ---------------- header, on the host ----------------
  uint8_t hdr[kHeaderBytes] = {0};
  const size_t hn = std::min<size_t>(n, kHeaderBytes);
  if (h_file) {
    memcpy(hdr, h_file, hn);
  } else if (hn) {
    SME_HIP(hipMemcpyAsync(hdr, d_file, hn, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
  }
  Header h{};
  Layout lay{};
  const int rc = validate_header(hdr, (uint64_t)n, (uint64_t)N, (uint64_t)V, &h, &lay);
  if (rc != H_OK) {
    char msg[200];
    const bool limit = describe_header(rc, h, (uint64_t)n, (uint64_t)N, (uint64_t)V, msg, sizeof msg);
    throw Error(limit ? SME_ELIMIT : SME_EPARSE, msg);
  }
  const int64_t Rn = (int64_t)h.records, T = (int64_t)h.positions;
  const int b = (int)h.bits;

  Prof prof(st, &cx->prof_events);
  DevBuf W[8];
  for (auto &w : W) w.pool = &cx->pool;
  const uint8_t *file = reinterpret_cast<const uint8_t *>(d_file);
  if (h_file) {
    uint8_t *up = W[0].as<uint8_t>(n);
    SME_HIP(hipMemcpyAsync(up, h_file, n, hipMemcpyHostToDevice, st));
    SME_HIP(hipStreamSynchronize(st));  // the caller's file is free again
    file = up;
  }
  // [0 .. E_WORDS) the first offences, all ones = none; [E_WORDS] the digest
  unsigned long long *d_err = W[1].as<unsigned long long>(E_WORDS + 1);
  SME_HIP(hipMemsetAsync(d_err, 0xFF, E_WORDS * sizeof(unsigned long long), st));
  prof.mark("header");

  // ---------------- digest, structure and decode: one synchronisation ----------------
  vocabulary_digest(ix, d_err + E_WORDS, st);
  prof.mark("digest");
  DevBuf t_off, t_ids, t_docno;  // handed to the index when every check has passed
  for (DevBuf *x : {&t_off, &t_ids, &t_docno}) x->pool = &cx->pool;
  int64_t *ps_off = t_off.as<int64_t>((size_t)Rn + 1), *len = W[2].as<int64_t>((size_t)Rn + 1);
  int32_t *ps_docno = t_docno.as<int32_t>((size_t)Rn + 1), *ids = t_ids.as<int32_t>((size_t)T + 1);
  hipLaunchKernelGGL(k_pf_records, dim3(grid_n(Rn + 1, kNT, kGridCap)), dim3(kNT), 0, st,
                     reinterpret_cast<const int32_t *>(file + lay.docno_at),
                     reinterpret_cast<const uint32_t *>(file + lay.len_at), Rn, ps_docno, len, d_err);
  SME_CHECK_LAUNCH();
  excl_scan<int64_t>(len, ps_off, Rn + 1, W[3], st);
  prof.mark("records");
  const int64_t ntiles = (T + kTile - 1) / kTile;
  if (T > 0) {
    hipLaunchKernelGGL(k_pf_decode, dim3(grid_n(ntiles, 1, kGridCap)), dim3(kNT), 0, st,
                       reinterpret_cast<const uint32_t *>(file + lay.words_at), T, b, (uint32_t)V, ntiles, ids, d_err);
    SME_CHECK_LAUNCH();
  }
  prof.mark("decode");
  unsigned long long e[E_WORDS + 1];
  int64_t sum = 0;
  SME_HIP(hipMemcpyAsync(e, d_err, sizeof e, hipMemcpyDeviceToHost, st));
  SME_HIP(hipMemcpyAsync(&sum, ps_off + Rn, sizeof sum, hipMemcpyDeviceToHost, st));
  SME_HIP(hipStreamSynchronize(st));
  if (e[E_WORDS] != h.digest) throw Error(SME_EPARSE, "positions file: digest: the file was written for another vocabulary");
  if (e[E_DOCNO] != kNone)
    throw Error(SME_EPARSE, "positions file: docno of record " + std::to_string(e[E_DOCNO]) + " is below the record's before it");
  if (sum != T)
    throw Error(SME_EPARSE, "positions file: len: the records' lengths add up to " + std::to_string(sum) +
                                ", the header's positions are " + std::to_string(T));
  if (e[E_ID] != kNone)
    throw Error(SME_EPARSE, "positions file: the id at position " + std::to_string(e[E_ID]) + " is not below V = " +
                                std::to_string(V));
  if (e[E_PAD] != kNone)
    throw Error(SME_EPARSE, e[E_PAD] == 0 ? "positions file: nonzero padding after the docno or len section"
                                          : "positions file: nonzero padding bits after the last position");

  // ---------------- cross-check with the postings ----------------
  uint64_t checked = 0;
  if (!(flags & kAttachNoCrosscheck)) {
    int32_t *cnt = W[4].as<int32_t>((size_t)P + 1);
    SME_HIP(hipMemsetAsync(cnt, 0, ((size_t)P + 1) * sizeof(int32_t), st));
    if (T > 0)
      hipLaunchKernelGGL(k_pf_count, dim3(grid_n(ntiles, 1, kGridCap)), dim3(kNT), 0, st, (const int32_t *)ids, T,
                         (const int64_t *)ps_off, (const int32_t *)ps_docno, Rn, (const int64_t *)ix->d_off.p,
                         (const int32_t *)ix->d_docno_d.p, ntiles, cnt, d_err);
    if (P > 0)
      hipLaunchKernelGGL(k_pf_compare, dim3(grid_n(P, kNT, kGridCap)), dim3(kNT), 0, st, (const int32_t *)cnt,
                         (const int32_t *)ix->d_tf_d.p, (const int32_t *)ix->d_docno_d.p, P, (const int64_t *)ix->d_off.p,
                         V, d_err);
    SME_CHECK_LAUNCH();
    const unsigned long long k = rd1(d_err + E_CROSS, st);
    if (k != kNone) {
      const int64_t term = (int64_t)(k >> 32);
      const int32_t d = (int32_t)((uint32_t)k ^ 0x80000000u);
      throw Error(SME_EPARSE, "positions file: cross-check: term " + std::to_string(term) + " in docno " +
                                  std::to_string(d) + ": the positions and the posting's tf disagree");
    }
    checked = (uint64_t)P;
  }
  prof.mark("crosscheck");
  const auto profile = prof.finish();  // waits for the stream: the scratch goes back to the pool after it

  swap_buf(ix->d_ps_off, t_off);
  swap_buf(ix->d_ps_terms, t_ids);
  swap_buf(ix->d_ps_docno, t_docno);
  ix->ps_records = Rn;
  ix->ps_terms = T;
  ix->has_positions = true;
  ix->nq_max_span = -1;
  cx->last_profile = profile;
  ix->pf_bytes = (uint64_t)n;
  ix->pf_bits = (uint64_t)b;
  ix->pf_checked = checked;
  ix->pf_decode_ms = stage_ms(profile, "decode");
  ix->pf_crosscheck_ms = (flags & kAttachNoCrosscheck) ? 0.0f : stage_ms(profile, "crosscheck");
}

}  // namespace sme
