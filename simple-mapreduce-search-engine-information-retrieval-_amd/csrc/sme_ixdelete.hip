// sme_ixdelete.hip -- documents out of a full index, into a new full index
// (sme_index_delete_docnos; include/sme.h has the semantics, DESIGN.md 4l the pass).
// Removing postings keeps both posting orders, so nothing is sorted:
//
//   set        one bit per docno of the input's [dmin, dmax], filled from the list
//              with atomicOr; listed docnos outside the range are skipped
//   records    survivors of d_rec_docno flagged against the bitmap, one scan, the
//              docnos compacted; every survivor carries the count of task starts up
//              to itself, and two neighbours with different counts have a task start
//              between them (sme_ixdelete.hpp's rule)
//   postings   the docno-order postings laid flat and cut into tiles of "delete_tile";
//              a count pass gives the tiles' survivors, one scan their places, the
//              emit pass ranks the survivors by ballots in the wave and through LDS
//              across waves, stages them in LDS and writes whole rows.  The thread on
//              an old term's first posting writes the survivors before it: the term's
//              new start.  The emit writes OLD term ids ...
//   terms      ... the terms with a non-empty new range are kept, one scan is the
//              old id -> new id table, d_off and the term strings are compacted and a
//              flat pass rewrites the term id of every posting
//   tf order   the same compaction over d_docno_o / d_tf_o, without the term part
//   weights    reweight_index with the new N, one flat pass (term id per posting)
//   positions  the records of d_ps_docno flagged, a scan of the kept lengths, one flat
//              gather of the streams with ids through the table
//
// No temporary of the postings' size but d_term_of.  Every search ends by a step
// bound; an output slot past the counted total or a vanished term id in a surviving
// stream sets a flag and stores nothing (SME_EHIP "(internal)").
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>

#include "sme_internal.hpp"
#include "sme_ixdelete.hpp"
#include "sme_ixparts.hpp"

namespace sme {

namespace {

using namespace ixdelete;

constexpr int kNT = 256;
constexpr int kPer = 4;              // postings per lane and step: one 16-byte load
constexpr int kStep = kNT * kPer;    // postings per workgroup step, and the LDS staging rows
constexpr int kWaves = kNT / 64;

struct Bits {  // the docno bitmap
  uint32_t *bm;
  int64_t dmin, span;
  __device__ __forceinline__ bool has(int32_t d) const { return bitmap_test(bm, d, dmin, span); }
};

// ---- set ---------------------------------------------------------------------------
__global__ void k_set(const int32_t *list, int64_t n, Bits B) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = bit_of(list[i], B.dmin, B.span);
    if (b >= 0) atomicOr(B.bm + (b >> 5), 1u << (b & 31));
  }
}

// ---- records -------------------------------------------------------------------------
// keep[i] = record i survives, start[i] = it starts a map task (n + 1 entries, the last 0)
__global__ void k_rec_flags(const int32_t *docno, const uint8_t *first, int64_t n, Bits B, int64_t *keep,
                            int64_t *start) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
    keep[i] = i < n && !B.has(docno[i]) ? 1 : 0;
    if (start) start[i] = i < n && (i == 0 || (first && first[i])) ? 1 : 0;
  }
}
// the survivors into their places (kex, sex: the exclusive scans of the flags):
// docno, the task starts up to the record, and the docno range
__global__ void k_rec_compact(const int32_t *docno, const int64_t *kex, const int64_t *sex, int64_t n, int64_t limit,
                              int32_t *odocno, int32_t *ostarts, int *range, int *err) {
  int mn = INT_MAX, mx = INT_MIN;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = kex[i];
    if (kex[i + 1] == j) continue;
    if (j >= limit) {  // (cannot be: the scan counted the same flags)
      atomicExch(err, 1);
      continue;
    }
    const int32_t d = docno[i];
    odocno[j] = d;
    ostarts[j] = (int32_t)sex[i + 1];
    mn = min(mn, d);
    mx = max(mx, d);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o, 64));
    mx = max(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0 && mn <= mx) {
    atomicMin(range, mn);
    atomicMax(range + 1, mx);
  }
}
__global__ void k_rec_first(const int32_t *starts, int64_t n, uint8_t *first) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x)
    first[j] = j == 0 || starts[j] != starts[j - 1] ? 1 : 0;
}
// the distinct docnos removed: every removed record clears its docno's bit, and the
// one that finds it set counts.  Runs last: nothing reads the bitmap after it.
__global__ void k_distinct(const int32_t *docno, const int64_t *kex, int64_t n, Bits B, unsigned long long *count) {
  const int64_t span = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x; i0 < n; i0 += span) {
    const int64_t i = i0 + threadIdx.x;
    bool hit = false;
    if (i < n && kex[i + 1] == kex[i]) {
      const int64_t b = bit_of(docno[i], B.dmin, B.span);
      if (b >= 0) hit = (atomicAnd(B.bm + (b >> 5), ~(1u << (b & 31))) >> (b & 31)) & 1u;
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (unsigned long long)__popcll(m));
  }
}

// ---- the compaction of a posting order ------------------------------------------------
// One workgroup per tile of T postings, in steps of kStep: lane l of the step holds
// postings 4 l .. 4 l + 3 (one 16-byte load per array), so the survivors' order is
// lane-major.  Ballot j holds the lanes whose posting j survives; a posting's rank in
// the wave is the survivors of the lanes below (four masked popcounts) plus those
// before it in its own lane, and the waves' totals meet in LDS.
//   EMIT false  tile_cnt[t] = the tile's survivors
//   EMIT true   writes them from tile_base[t] on, staged in LDS and stored as whole
//               rows; TERMS: also the OLD term id of every survivor, every old term's
//               new start (the survivors before its first posting) and the largest tf
template <bool EMIT, bool TERMS>
__global__ __launch_bounds__(kNT) void k_compact(const int32_t *dn, const int32_t *tf, int64_t P, int T, int64_t ntiles,
                                                 Bits B, const int64_t *off, int64_t V, int64_t *tile_cnt,
                                                 const int64_t *tile_base, int32_t *odn, int32_t *otf, uint32_t *oterm,
                                                 int64_t *nstart, unsigned int *max_tf, int *err, int64_t olimit) {
  __shared__ int32_t s_dn[EMIT ? kStep : 1], s_tf[EMIT ? kStep : 1];
  __shared__ uint32_t s_tm[EMIT && TERMS ? kStep : 1];
  __shared__ int s_wtot[kWaves];
  __shared__ int64_t s_win[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const bool vec = (((uintptr_t)dn | (uintptr_t)tf) & 15) == 0;  // 16-byte loads need the alignment (uniform)
  uint32_t mtf = 0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t p0 = t * (int64_t)T, p1 = min(P, p0 + T);
    int64_t w0 = 0, w1 = 0;
    if (EMIT && TERMS) {
      // the tile's window of terms: two searches of d_off, bounded by their step count
      if (tid < 2) s_win[tid] = last_le(off, 0, V + 1, tid ? p1 - 1 : p0);
      __syncthreads();
      w0 = s_win[0];
      w1 = s_win[1] + 1;
    }
    const int64_t base = EMIT ? tile_base[t] : 0;
    int64_t carry = 0;  // the tile's survivors before this step
    for (int64_t c = p0; c < p1; c += kStep) {
      const int64_t q = c + (int64_t)tid * kPer;
      int32_t d[kPer] = {0, 0, 0, 0}, f[kPer] = {0, 0, 0, 0};
      if (vec && q + kPer <= p1) {
        const int4 v = *reinterpret_cast<const int4 *>(dn + q);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        if (EMIT) {
          const int4 w = *reinterpret_cast<const int4 *>(tf + q);
          f[0] = w.x, f[1] = w.y, f[2] = w.z, f[3] = w.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < kPer; j++)
          if (q + j < p1) {
            d[j] = dn[q + j];
            if (EMIT) f[j] = tf[q + j];
          }
      }
      bool keep[kPer];
      int r = 0, wtot = 0;  // survivors of the lanes below; of the wave
#pragma unroll
      for (int j = 0; j < kPer; j++) {
        keep[j] = q + j < p1 && !B.has(d[j]);
        const unsigned long long m = __ballot(keep[j]);
        r += __popcll(m & below);
        wtot += __popcll(m);
      }
      if (lane == 0) s_wtot[wave] = wtot;
      __syncthreads();
      int tot = 0;
#pragma unroll
      for (int x = 0; x < kWaves; x++) {
        if (x < wave) r += s_wtot[x];
        tot += s_wtot[x];
      }
      if (EMIT) {
        int64_t term = 0;
        if (TERMS && q < p1) term = last_le(off, w0, w1, q);
#pragma unroll
        for (int j = 0; j < kPer; j++) {
          if (q + j >= p1) break;
          if (TERMS) {
            // every term has a posting, so the term of the next posting is this one or the next
            if (j > 0 && off[term + 1] <= q + j) term++;
            if (off[term] == q + j) nstart[term] = base + carry + r;
          }
          if (keep[j]) {
            s_dn[r] = d[j];
            s_tf[r] = f[j];
            if (TERMS) {
              s_tm[r] = (uint32_t)term;
              mtf = max(mtf, (uint32_t)f[j]);
            }
            r++;
          }
        }
        __syncthreads();
        // whole rows: consecutive lanes, consecutive output slots
        for (int x = tid; x < tot; x += kNT) {
          const int64_t o = base + carry + x;
          if (o >= olimit) {  // (cannot be: the count pass saw the same tile)
            atomicExch(err, 1);
            continue;
          }
          odn[o] = s_dn[x];
          otf[o] = s_tf[x];
          if (TERMS) oterm[o] = s_tm[x];
        }
      }
      carry += tot;
      __syncthreads();  // s_wtot and the staging rows are free again
    }
    if (!EMIT && tid == 0) tile_cnt[t] = carry;
  }
  if (EMIT && TERMS) {
    for (int o = 32; o > 0; o >>= 1) mtf = max(mtf, (uint32_t)__shfl_xor((int)mtf, o, 64));
    if (lane == 0 && mtf) atomicMax(max_tf, mtf);
  }
}

// ---- terms -----------------------------------------------------------------------------
// nstart: V + 1 new starts of the old terms (nstart[V] = the surviving postings)
__global__ void k_term_flags(const int64_t *nstart, int64_t V, int64_t *keep) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t <= V; t += (int64_t)gridDim.x * blockDim.x)
    keep[t] = t < V && nstart[t + 1] > nstart[t] ? 1 : 0;
}
// tex: the exclusive scan of the flags = the old id -> new id table of the kept terms
__global__ void k_term_compact(const int64_t *nstart, const int64_t *tex, const int64_t *toff, int64_t V, int64_t limit,
                               int32_t *tmap, int64_t *noff, int64_t *nlen, int32_t *src, int *err) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < V; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = tex[t];
    if (tex[t + 1] == g) {
      tmap[t] = -1;
      continue;
    }
    if (g >= limit) {  // (cannot be)
      atomicExch(err, 1);
      tmap[t] = -1;
      continue;
    }
    tmap[t] = (int32_t)g;
    noff[g] = nstart[t];
    nlen[g] = toff[t + 1] - toff[t];
    src[g] = (int32_t)t;
  }
}
__global__ void k_term_remap(uint32_t *term_of, int64_t P, const int32_t *tmap, int64_t V, int *err) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t t = term_of[p];
    const int32_t g = t < (uint64_t)V ? tmap[t] : -1;
    if (g < 0) {  // (cannot be: a term with a surviving posting is kept)
      atomicExch(err, 1);
      continue;
    }
    term_of[p] = (uint32_t)g;
  }
}

// ---- the flat gather of kept rows (term strings, term streams) ---------------------------
// Output row o = input row src[o], ooff the output rows' offsets (nrow + 1, M =
// ooff[nrow]): consecutive lanes on consecutive output elements.  REMAP: an element
// >= 0 is an old term id and goes through tmap; a vanished id sets the flag and is
// not stored.
template <typename E, bool REMAP>
__global__ __launch_bounds__(kNT) void k_gather(const int64_t *ooff, int64_t nrow, const int32_t *src,
                                                const int64_t *ioff, const E *in, int64_t M, const int32_t *tmap,
                                                int64_t V, E *out, int *err) {
  for_row_elements<kNT>(ooff, nrow, M, [&](int64_t p, int64_t o) {
    E v = in[ioff[src[o]] + (p - ooff[o])];
    if (REMAP && (int64_t)v >= 0) {
      const int32_t g = (int64_t)v < V ? tmap[(int64_t)v] : -1;
      if (g < 0) {
        atomicExch(err, 1);
        return;
      }
      v = (E)g;
    }
    out[p] = v;
  });
}

// ---- positions ------------------------------------------------------------------------------
__global__ void k_ps_compact(const int32_t *docno, const int64_t *kex, const int64_t *ioff, int64_t n, int64_t limit,
                             int32_t *odocno, int32_t *src, int64_t *len, int *err) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = kex[i];
    if (kex[i + 1] == j) continue;
    if (j >= limit) {  // (cannot be)
      atomicExch(err, 1);
      continue;
    }
    odocno[j] = docno[i];
    src[j] = (int32_t)i;
    len[j] = ioff[i + 1] - ioff[i];
  }
}

// one posting order compacted: count, scan, emit.  Returns the survivors.
template <bool TERMS>
int64_t compact_order(const int32_t *dn, const int32_t *tf, int64_t P, int T, Bits B, const int64_t *off, int64_t V,
                      int32_t *odn, int32_t *otf, uint32_t *oterm, int64_t *nstart, unsigned int *d_mtf, int *d_err,
                      int64_t expect, DevBuf &b_cnt, DevBuf &b_base, DevBuf &scan, hipStream_t st) {
  const int64_t ntiles = (P + T - 1) / T;
  int64_t *cnt = b_cnt.as<int64_t>((size_t)ntiles + 1), *base = b_base.as<int64_t>((size_t)ntiles + 1);
  const unsigned grid = (unsigned)std::min<int64_t>(ntiles, 65536);
  hipLaunchKernelGGL((k_compact<false, TERMS>), dim3(grid), dim3(kNT), 0, st, dn, tf, P, T, ntiles, B, off, V, cnt,
                     (const int64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (uint32_t *)nullptr,
                     (int64_t *)nullptr, (unsigned int *)nullptr, d_err, (int64_t)0);
  SME_CHECK_LAUNCH();
  SME_HIP(hipMemsetAsync(cnt + ntiles, 0, sizeof(int64_t), st));
  excl_scan<int64_t>(cnt, base, ntiles + 1, scan, st);
  const int64_t total = rd1(base + ntiles, st);
  if (total < 0 || total > P || (expect >= 0 && total != expect))
    throw Error(SME_EHIP, "index delete: the two posting orders do not agree (internal)");
  hipLaunchKernelGGL((k_compact<true, TERMS>), dim3(grid), dim3(kNT), 0, st, dn, tf, P, T, ntiles, B, off, V,
                     (int64_t *)nullptr, (const int64_t *)base, odn, otf, oterm, nstart, d_mtf, d_err, total);
  SME_CHECK_LAUNCH();
  return total;
}

}  // namespace

sme_index *delete_docnos(sme_index *in, const int32_t *list, int64_t n, bool list_on_device, bool has_out,
                         hipStream_t st) {
  // ---- refusals, before any per-posting work
  {
    const CallDesc c{in != nullptr,    has_out,        list != nullptr, n, in && in->records_only,
                     in ? in->job : 0, in ? in->K : 1, in ? in->rec_complete : true};
    const int rc = validate(c);
    if (rc != D_OK) {
      char msg[200];
      const bool notimpl = describe(rc, msg, sizeof msg);
      throw Error(notimpl ? SME_ENOTIMPL : SME_EINVAL, msg);
    }
  }
  sme_ctx *cx = in->ctx;
  const int T = (int)cx->opt_delete_tile;
  Prof prof(st, &cx->prof_events);
  DevBuf W[32];
  for (auto &b : W) b.pool = &cx->pool;

  const int64_t N = in->N, V = in->V, P = in->P;
  // [0] distinct docnos removed, [1] max_tf (u32), [2] the error flag, [3] the docno range (2 int)
  unsigned long long *d_cnt = W[0].as<unsigned long long>(4);
  SME_HIP(hipMemsetAsync(d_cnt, 0, 4 * sizeof(unsigned long long), st));
  unsigned int *d_mtf = reinterpret_cast<unsigned int *>(d_cnt + 1);
  int *d_err = reinterpret_cast<int *>(d_cnt + 2), *d_range = reinterpret_cast<int *>(d_cnt + 3);
  const int h_range[2] = {INT_MAX, INT_MIN};
  SME_HIP(hipMemcpyAsync(d_range, h_range, sizeof h_range, hipMemcpyHostToDevice, st));
  auto internal = [&](const char *what) {
    if (rd1(d_err, st)) throw Error(SME_EHIP, std::string("index delete: ") + what + " (internal)");
  };

  sme_index *ix = new sme_index(cx);
  std::unique_ptr<sme_index> guard(ix);
  ix->K = 1;
  ix->R = cx->cfg.num_partitions;
  ix->idf_mode = cx->cfg.idf_mode;
  ix->from_records = true;  // like a merged index: no record docnos handed out, no pieces
  ix->rec_complete = true;

  // ---------------- 1. set ----------------
  Bits B;
  B.dmin = in->dmin;
  B.span = N > 0 ? span_of(in->dmin, in->dmax) : 0;
  const int64_t words = bitmap_words(B.span);
  B.bm = W[1].as<uint32_t>((size_t)words + 1);
  SME_HIP(hipMemsetAsync(B.bm, 0, ((size_t)words + 1) * sizeof(uint32_t), st));
  if (n > 0 && B.span > 0) {
    const int32_t *d_list = list;
    if (!list_on_device) {
      int32_t *up = W[2].as<int32_t>((size_t)n);
      SME_HIP(hipMemcpyAsync(up, list, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
      SME_HIP(hipStreamSynchronize(st));  // the caller's list is free again
      d_list = up;
    }
    hipLaunchKernelGGL(k_set, dim3(grid_n(n)), dim3(kNT), 0, st, d_list, n, B);
    SME_CHECK_LAUNCH();
  }
  prof.mark("set");

  // ---------------- 2. records ----------------
  int64_t *kex = W[3].as<int64_t>((size_t)N + 1), *sex = W[4].as<int64_t>((size_t)N + 1);
  hipLaunchKernelGGL(k_rec_flags, dim3(grid_n(N + 1)), dim3(kNT), 0, st, (const int32_t *)in->d_rec_docno.p,
                     (const uint8_t *)in->d_rec_first.p, N, B, kex, sex);
  SME_CHECK_LAUNCH();
  excl_scan<int64_t>(kex, kex, N + 1, W[5], st);
  excl_scan<int64_t>(sex, sex, N + 1, W[5], st);
  const int64_t Nn = rd1(kex + N, st);
  if (Nn < 0 || Nn > N) throw Error(SME_EHIP, "index delete: the record count (internal)");
  int32_t *rdn = ix->d_rec_docno.as<int32_t>((size_t)Nn + 1);
  uint8_t *fst = ix->d_rec_first.as<uint8_t>((size_t)Nn + 1);
  if (N > 0) {
    int32_t *starts = W[6].as<int32_t>((size_t)Nn + 1);
    hipLaunchKernelGGL(k_rec_compact, dim3(grid_n(N)), dim3(kNT), 0, st, (const int32_t *)in->d_rec_docno.p,
                       (const int64_t *)kex, (const int64_t *)sex, N, Nn, rdn, starts, d_range, d_err);
    if (Nn > 0) hipLaunchKernelGGL(k_rec_first, dim3(grid_n(Nn)), dim3(kNT), 0, st, (const int32_t *)starts, Nn, fst);
    SME_CHECK_LAUNCH();
  }
  ix->N = Nn;
  if (Nn > 0) {
    int h_r[2];
    SME_HIP(hipMemcpyAsync(h_r, d_range, sizeof h_r, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    ix->dmin = h_r[0];
    ix->dmax = h_r[1];
  }
  prof.mark("records");

  // ---------------- 3. docno-order postings ----------------
  int64_t Pn = 0;
  uint32_t *term_of = W[7].as<uint32_t>((size_t)P + 1);
  int64_t *nstart = W[8].as<int64_t>((size_t)V + 1);
  // (16-byte aligned for the vector loads of a later pass -- hipMalloc'd blocks are)
  int32_t *docno_d = ix->d_docno_d.as<int32_t>((size_t)P + 1), *tf_d = ix->d_tf_d.as<int32_t>((size_t)P + 1);
  if (P > 0) {
    Pn = compact_order<true>((const int32_t *)in->d_docno_d.p, (const int32_t *)in->d_tf_d.p, P, T, B,
                             (const int64_t *)in->d_off.p, V, docno_d, tf_d, term_of, nstart, d_mtf, d_err, -1, W[9],
                             W[10], W[5], st);
    internal("an output slot past the counted postings");
  }
  SME_HIP(hipMemcpyAsync(nstart + V, &Pn, sizeof(int64_t), hipMemcpyHostToDevice, st));
  SME_HIP(hipStreamSynchronize(st));
  ix->P = Pn;
  ix->max_tf = std::max(1, P > 0 ? (int)rd1(d_mtf, st) : 0);
  prof.mark("postings");

  // ---------------- 4. terms ----------------
  int64_t Vn = 0;
  int64_t *tex = W[11].as<int64_t>((size_t)V + 1);
  int32_t *tmap = W[12].as<int32_t>((size_t)V + 1);
  if (V > 0) {
    hipLaunchKernelGGL(k_term_flags, dim3(grid_n(V + 1)), dim3(kNT), 0, st, (const int64_t *)nstart, V, tex);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(tex, tex, V + 1, W[5], st);
    Vn = rd1(tex + V, st);
    if (Vn < 0 || Vn > V) throw Error(SME_EHIP, "index delete: the term count (internal)");
  }
  int64_t *off = ix->d_off.as<int64_t>((size_t)Vn + 1);
  int64_t *term_off = ix->d_term_off.as<int64_t>((size_t)Vn + 1);
  int64_t *nlen = W[13].as<int64_t>((size_t)Vn + 1);
  int32_t *tsrc = W[14].as<int32_t>((size_t)Vn + 1);
  if (V > 0) {
    hipLaunchKernelGGL(k_term_compact, dim3(grid_n(V)), dim3(kNT), 0, st, (const int64_t *)nstart, (const int64_t *)tex,
                       (const int64_t *)in->d_term_off.p, V, Vn, tmap, off, nlen, tsrc, d_err);
    SME_CHECK_LAUNCH();
  }
  SME_HIP(hipMemcpyAsync(off + Vn, &Pn, sizeof(int64_t), hipMemcpyHostToDevice, st));
  SME_HIP(hipMemsetAsync(nlen + Vn, 0, sizeof(int64_t), st));
  excl_scan<int64_t>(nlen, term_off, Vn + 1, W[5], st);
  const int64_t tchars = rd1(term_off + Vn, st);
  uint16_t *tch = ix->d_term_chars.as<uint16_t>((size_t)tchars + 8);
  if (tchars > 0)
    hipLaunchKernelGGL((k_gather<uint16_t, false>), dim3(grid_n(tchars, 1024, 65536)), dim3(kNT), 0, st,
                       (const int64_t *)term_off, Vn, (const int32_t *)tsrc, (const int64_t *)in->d_term_off.p,
                       (const uint16_t *)in->d_term_chars.p, tchars, (const int32_t *)nullptr, (int64_t)0, tch, d_err);
  if (Pn > 0)
    hipLaunchKernelGGL(k_term_remap, dim3(grid_n(Pn, kNT, 65536)), dim3(kNT), 0, st, term_of, Pn, (const int32_t *)tmap,
                       V, d_err);
  SME_CHECK_LAUNCH();
  internal("a surviving posting of a vanished term");
  ix->V = ix->Vt = Vn;
  prof.mark("terms");

  // ---------------- 5. reduce order ----------------
  // (tf_sort_segments over the compacted docno order would give the same lists; not built, not measured)
  int32_t *docno_o = ix->d_docno_o.as<int32_t>((size_t)P + 1), *tf_o = ix->d_tf_o.as<int32_t>((size_t)P + 1);
  if (P > 0) {
    compact_order<false>((const int32_t *)in->d_docno_o.p, (const int32_t *)in->d_tf_o.p, P, T, B,
                         (const int64_t *)nullptr, 0, docno_o, tf_o, (uint32_t *)nullptr, (int64_t *)nullptr,
                         (unsigned int *)nullptr, d_err, Pn, W[9], W[10], W[5], st);
    internal("an output slot past the counted postings");
  }
  prof.mark("tf_order");

  // ---------------- 6. weights ----------------
  ix->d_idf.as<double>((size_t)Vn + 1);
  ix->d_w.as<double>((size_t)Pn + 1);
  reweight_index(ix, Nn, nullptr, st, Pn > 0 ? term_of : nullptr);
  prof.mark("weights");

  // ---------------- 7. positions ----------------
  if (in->has_positions) {
    const int64_t R = in->ps_records;
    int64_t *pex = W[15].as<int64_t>((size_t)R + 1);
    hipLaunchKernelGGL(k_rec_flags, dim3(grid_n(R + 1)), dim3(kNT), 0, st, (const int32_t *)in->d_ps_docno.p,
                       (const uint8_t *)nullptr, R, B, pex, (int64_t *)nullptr);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(pex, pex, R + 1, W[5], st);
    const int64_t Rn = rd1(pex + R, st);
    if (Rn < 0 || Rn > R) throw Error(SME_EHIP, "index delete: the stream record count (internal)");
    int32_t *pdn = ix->d_ps_docno.as<int32_t>((size_t)Rn + 1);
    int32_t *psrc = W[16].as<int32_t>((size_t)Rn + 1);
    int64_t *plen = W[17].as<int64_t>((size_t)Rn + 1), *ooff = ix->d_ps_off.as<int64_t>((size_t)Rn + 1);
    if (R > 0)
      hipLaunchKernelGGL(k_ps_compact, dim3(grid_n(R)), dim3(kNT), 0, st, (const int32_t *)in->d_ps_docno.p,
                         (const int64_t *)pex, (const int64_t *)in->d_ps_off.p, R, Rn, pdn, psrc, plen, d_err);
    SME_CHECK_LAUNCH();
    SME_HIP(hipMemsetAsync(plen + Rn, 0, sizeof(int64_t), st));
    excl_scan<int64_t>(plen, ooff, Rn + 1, W[5], st);
    const int64_t M = rd1(ooff + Rn, st);
    if (M < 0 || M > in->ps_terms) throw Error(SME_EHIP, "index delete: stream lengths do not add up (internal)");
    int32_t *ps = ix->d_ps_terms.as<int32_t>((size_t)M + 1);
    if (M > 0)
      hipLaunchKernelGGL((k_gather<int32_t, true>), dim3(grid_n(M, 1024, 65536)), dim3(kNT), 0, st,
                         (const int64_t *)ooff, Rn, (const int32_t *)psrc, (const int64_t *)in->d_ps_off.p,
                         (const int32_t *)in->d_ps_terms.p, M, (const int32_t *)tmap, V, ps, d_err);
    SME_CHECK_LAUNCH();
    internal("a vanished term in a surviving record's stream");
    ix->ps_records = Rn;
    ix->ps_terms = M;
    ix->has_positions = true;
  }
  // the distinct docnos removed (clears the bitmap: nothing reads it afterwards)
  if (N > Nn)
    hipLaunchKernelGGL(k_distinct, dim3(grid_n(N)), dim3(kNT), 0, st, (const int32_t *)in->d_rec_docno.p,
                       (const int64_t *)kex, N, B, d_cnt);
  SME_CHECK_LAUNCH();
  prof.mark("positions");
  ix->profile = prof.finish();  // waits for the stream: the scratch goes back to the pool after it
  ix->dl_made = 1;
  ix->dl_docnos = (uint64_t)rd1(d_cnt, st);
  ix->dl_records = (uint64_t)(N - Nn);
  ix->dl_postings = (uint64_t)(P - Pn);
  ix->dl_terms = (uint64_t)(V - Vn);
  guard.release();
  return ix;
}

}  // namespace sme
