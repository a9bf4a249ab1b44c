// sme_bm25.hip -- BM25 ranking on the device (include/sme.h, sme_query_topk_bm25).
//
//   prepare   once per index, from the docno-order postings alone:
//             k_bm_len     dl[d] += tf, one 64-bit integer atomic per posting
//             k_bm_windows per window of kWindow documents: dl as int32, the smallest
//                          non-zero dl, and D, L, the longest document
//             k_bm_terms   per term (one wave each): the largest tf, and the largest df
//             k_bm_idf     idf[t] = table[df_t], the table from the host's libm
//   per call  k_bm_norm    norm[d] = k1 ((1 - b) + b dl[d] / avgdl)
//             k_bm_score   one workgroup per (query, range of windows): window-major
//                          and exhaustive inside a window; see the kernel
//             k_merge_rows the split's S rows per query into one (sme_owner.hip)
//
// The weight, the norm and the window bound are the functions of sme_bm25.hpp.
#include "sme_bm25.hpp"

#include <algorithm>
#include <cmath>

#include "sme_common.hpp"
#include "sme_internal.hpp"

namespace sme {
namespace {

using namespace bm25;

constexpr int kNT = 256;        // threads of k_bm_score
constexpr int kCand = 2048;     // candidate list: the best kMaxK so far + one window's documents
static_assert(kCand >= kMaxK + kWindow && (kCand & (kCand - 1)) == 0, "candidate list");
static_assert(kWindow % kNT == 0 && kWindow % 64 == 0, "window sweep");

// prepare's counters
enum { C_DOCS = 0, C_LEN, C_MAXLEN, C_MAXDF, C_RANGE, C_WIDE, C_N };

__global__ void k_bm_len(const int32_t *dn, const int32_t *tf, int64_t P, int64_t dmin, int64_t span,
                         unsigned long long *len, unsigned long long *cnt) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t d = (int64_t)dn[i] - dmin;
    if (d < 0 || d >= span) {
      atomicAdd(cnt + C_RANGE, 1ull);
      continue;
    }
    atomicAdd(len + d, (unsigned long long)(int64_t)tf[i]);
  }
}

// one workgroup per window
__global__ __launch_bounds__(256) void k_bm_windows(const unsigned long long *len, int64_t span, int32_t *dl,
                                                     int32_t *mindl, unsigned long long *cnt) {
  __shared__ unsigned long long s_len, s_max;
  __shared__ unsigned s_docs, s_min, s_wide;
  if (threadIdx.x == 0) {
    s_len = 0;
    s_max = 0;
    s_docs = 0;
    s_min = 0xFFFFFFFFu;
    s_wide = 0;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kWindow;
  unsigned long long sum = 0, mx = 0;
  unsigned docs = 0, mn = 0xFFFFFFFFu, wide = 0;
  for (int j = threadIdx.x; j < kWindow; j += 256) {
    const int64_t i = base + j;
    if (i >= span) break;
    const unsigned long long v = len[i];
    if (v > 0x7FFFFFFFull) wide = 1;
    dl[i] = (int32_t)(v > 0x7FFFFFFFull ? 0x7FFFFFFFull : v);
    if (v) {
      docs++;
      sum += v;
      mx = max(mx, v);
      mn = min(mn, (unsigned)min(v, 0x7FFFFFFFull));
    }
  }
  if (docs) {
    atomicAdd(&s_len, sum);
    atomicMax(&s_max, mx);
    atomicAdd(&s_docs, docs);
    atomicMin(&s_min, mn);
    if (wide) atomicOr(&s_wide, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mindl[blockIdx.x] = s_docs ? (int32_t)s_min : 0;
    if (s_docs) {
      atomicAdd(cnt + C_DOCS, (unsigned long long)s_docs);
      atomicAdd(cnt + C_LEN, s_len);
      atomicMax(cnt + C_MAXLEN, s_max);
      if (s_wide) atomicAdd(cnt + C_WIDE, 1ull);
    }
  }
}

// one wave per term
__global__ __launch_bounds__(256) void k_bm_terms(const int64_t *off, const int32_t *tf, int64_t V, int32_t *maxtf,
                                                   unsigned long long *cnt) {
  const int64_t w0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int l = lane_id();
  long long dfmax = 0;
  for (int64_t t = w0; t < V; t += nw) {
    const int64_t a = off[t], e = off[t + 1];
    int m = 0;
    for (int64_t i = a + l; i < e; i += 64) m = max(m, tf[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if (l == 0) maxtf[t] = m;
    dfmax = max(dfmax, (long long)(e - a));
  }
  if (l == 0 && dfmax > 0) atomicMax(cnt + C_MAXDF, (unsigned long long)dfmax);
}

__global__ void k_bm_idf(const int64_t *off, int64_t V, const double *by_df, double *idf) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < V; t += (int64_t)gridDim.x * blockDim.x)
    idf[t] = by_df[off[t + 1] - off[t]];
}

__global__ void k_bm_norm(const int32_t *dl, int64_t span, double k1, double b, double avgdl, double *norm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x)
    norm[i] = doc_norm(k1, b, (double)dl[i], avgdl);
}

struct ScoreArgs {
  const int64_t *off;    // [V + 1]
  const int32_t *dn;     // [P] docno-ascending per term
  const int32_t *tf;     // [P]
  const double *idf;     // [V]
  const int32_t *maxtf;  // [V]
  const int32_t *mindl;  // [nwin]
  const double *norm;    // [span]
  const int32_t *terms;
  const int64_t *qoff;
  int64_t V, dmin, span;
  int nwin, S, k;
  double k1, b, avgdl;
  int32_t *od;  // [nq * S, k]
  double *os;
  unsigned long long *bar;   // [nq] the queries' shared entry bars as bar_key (S > 1)
  unsigned long long *stat;  // windows, skipped, postings
};

__device__ __forceinline__ bool bm_better(double as, int32_t ad, double bs, int32_t bd) {
  return as > bs || (as == bs && ad < bd);
}

// The candidate list [0, n) sorted best first (score descending, docno ascending) and
// cut to its best k; returns the entries kept.  Every thread of the workgroup calls it.
__device__ int bm_sort_cut(double *ls, int32_t *ld, int n, int k) {
  int n2 = 2;
  while (n2 < n) n2 <<= 1;
  for (int i = n + threadIdx.x; i < n2; i += kNT) {
    ls[i] = -INFINITY;
    ld[i] = 0x7FFFFFFF;
  }
  __syncthreads();
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < (n2 >> 1); i += kNT) {
        const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo + stride;
        const double a = ls[lo], b = ls[hi];
        const int32_t da = ld[lo], db = ld[hi];
        const bool sw = (lo & size) == 0 ? bm_better(b, db, a, da) : bm_better(a, da, b, db);
        if (sw) {
          ls[lo] = b;
          ls[hi] = a;
          ld[lo] = db;
          ld[hi] = da;
        }
      }
      __syncthreads();
    }
  return min(n, k);
}

constexpr int kNoWindow = 0x7FFFFFFF;  // the head window of a slot without a posting left

// One workgroup per (query, part): the query's term slots over the windows
// [part nwin / S, (part + 1) nwin / S).  Every slot keeps a cursor that only moves
// forward (the lists ascend) and the window of the posting under it, its head; the
// workgroup goes from one window that holds a posting to the next one that does --
// the smallest head -- and the slots whose head it is are the window's slots:
//   skip     once k candidates stand, the window's bound against the entry bar; the
//            slots of a skipped window search their lists for the window's end
//   score    the window's norm slice into LDS, fp64 accumulators and a touched map
//            cleared; the slots in listed order, lanes over a slot's postings from its
//            cursor while they lie in the window (docnos are distinct within a list, so
//            no accumulator is written twice; the lane behind the last one holds the
//            slot's next head).  The barrier that counts a chunk's postings is the
//            barrier between slots: the summation order is the listed order
//   sweep    touched documents not below the bar join the candidate list, which is
//            sorted and cut to its best k before a window could overflow it; the k-th
//            becomes the bar (and, under a split, is offered to the query's shared bar)
// The list holds the best k of the documents seen plus whatever is not below a bar
// that is never above the final k-th score, so the best k at the end are exact.
__global__ __launch_bounds__(kNT) void k_bm_score(const ScoreArgs A) {
  __shared__ double s_norm[kWindow];
  __shared__ double s_acc[kWindow];  // (the slots' bound terms before a window is scored)
  __shared__ double s_ls[kCand];
  __shared__ int64_t s_cur[kMaxSlots];
  __shared__ int32_t s_ld[kCand];
  __shared__ int32_t s_term[kMaxSlots];
  __shared__ int32_t s_head[kMaxSlots];
  __shared__ int64_t s_end[kMaxSlots];  // the slots' list ends and idf: no global read stands before a slot's postings
  __shared__ double s_idf[kMaxSlots];
  __shared__ uint8_t s_touched[kWindow];
  __shared__ unsigned long long s_bar;
  // the smallest head, for the windows it, it + 1 and it + 2 in turn: read for the
  // window at hand, gathered for the next, reset for the one after
  __shared__ int s_wmin[3];
  __shared__ int s_ncand, s_skip;

  const int q = blockIdx.x / A.S, part = blockIdx.x % A.S;
  const int tid = threadIdx.x;
  const int64_t q0 = A.qoff[q];
  const int ns = (int)min<int64_t>(max<int64_t>(A.qoff[q + 1] - q0, 0), kMaxSlots);
  const int w_first = (int)((int64_t)part * A.nwin / A.S), w_last = (int)((int64_t)(part + 1) * A.nwin / A.S);
  const int k = A.k;

  if (tid == 0) {
    s_ncand = 0;
    s_wmin[0] = s_wmin[1] = s_wmin[2] = kNoWindow;
  }
  __syncthreads();
  // the slots' cursors at the range's first docno
  const int64_t first_doc = A.dmin + (int64_t)w_first * kWindow;
  for (int s = tid; s < ns; s += kNT) {
    int32_t t = A.terms[q0 + s];
    if (t < 0 || t >= A.V) t = -1;
    int64_t lo = 0, end = 0;
    int head = kNoWindow;
    if (t >= 0) {
      lo = A.off[t];
      end = A.off[t + 1];
      int64_t hi = end;
      if (w_first > 0)
        while (lo < hi) {
          const int64_t m = (lo + hi) >> 1;
          if ((int64_t)A.dn[m] < first_doc)
            lo = m + 1;
          else
            hi = m;
        }
      if (lo < end) head = (int)(((int64_t)A.dn[lo] - A.dmin) / kWindow);
    }
    s_term[s] = t;
    s_cur[s] = lo;
    s_head[s] = head;
    s_end[s] = end;
    s_idf[s] = t >= 0 ? A.idf[t] : 0.0;
    if (head != kNoWindow) atomicMin(&s_wmin[0], head);
  }
  __syncthreads();

  double theta = -INFINITY;  // the entry bar: the k-th best score of some subset of the documents, or none
  unsigned long long n_windows = 0, n_skipped = 0, n_postings = 0;  // (thread 0's)
  int ncand = 0;

  for (int it = 0;; it = it == 2 ? 0 : it + 1) {
    const int nx = it == 2 ? 0 : it + 1;  // where the next window's smallest head is gathered
    const int w = s_wmin[it];
    if (w >= w_last) break;  // (uniform; kNoWindow: every list is at its end)
    const int64_t wbase = A.dmin + (int64_t)w * kWindow, wend = wbase + kWindow;
    if (tid == 0) {
      s_wmin[nx == 2 ? 0 : nx + 1] = kNoWindow;
      s_skip = 0;
      n_windows++;
    }
    if (A.S > 1) {
      if (tid == 0) s_bar = __hip_atomic_load(A.bar + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      if (s_bar) theta = fmax(theta, bar_value(s_bar));  // (one read for the workgroup: theta stays uniform)
    }
    const bool barred = theta > -INFINITY;
    // the slots that rest: their heads stand for the next window
    for (int s = tid; s < ns; s += kNT) {
      const int h = s_head[s];
      if (h != w && h != kNoWindow) atomicMin(&s_wmin[nx], h);
    }
    if (barred) {
      // skip: the bound summed in listed order, as a score is; a slot without a posting
      // here adds +0.0.  Strictly below the bar only: an equal score may win its tie.
      const double mindl = (double)A.mindl[w];
      for (int s = tid; s < ns; s += kNT) {
        const int32_t t = s_term[s];
        s_acc[s] = s_head[s] == w ? bound_term(s_idf[s], (double)A.maxtf[t], A.k1, A.b, mindl, A.avgdl) : 0.0;
      }
      __syncthreads();
      if (tid == 0) {
        double bound = 0.0;
        for (int s = 0; s < ns; s++) bound += s_acc[s];
        if (bound < theta) {
          s_skip = 1;
          n_skipped++;
        }
      }
      __syncthreads();
      if (s_skip) {  // (uniform) the window's slots move to the first posting at or past its end
        for (int s = tid; s < ns; s += kNT) {
          if (s_head[s] != w) continue;
          const int64_t end = s_end[s];
          int64_t l = s_cur[s], r, step = 1;
          for (;;) {  // gallop: entries before l lie below wend
            r = l + step;
            if (r >= end) {
              r = end;
              break;
            }
            if ((int64_t)A.dn[r - 1] >= wend) break;
            l = r;
            step <<= 1;
          }
          while (l < r) {
            const int64_t m = (l + r) >> 1;
            if ((int64_t)A.dn[m] < wend)
              l = m + 1;
            else
              r = m;
          }
          const int h = l < end ? (int)(((int64_t)A.dn[l] - A.dmin) / kWindow) : kNoWindow;
          s_cur[s] = l;
          s_head[s] = h;
          if (h != kNoWindow) atomicMin(&s_wmin[nx], h);
        }
        __syncthreads();
        continue;
      }
    }
    // score
    for (int j = tid; j < kWindow; j += kNT) {
      const int64_t i = (int64_t)w * kWindow + j;
      s_norm[j] = i < A.span ? A.norm[i] : 0.0;
      s_acc[j] = 0.0;
      s_touched[j] = 0;
    }
    __syncthreads();
    for (int s = 0; s < ns; s++) {
      if (s_head[s] != w) continue;  // (uniform)
      const int64_t lo = s_cur[s], end = s_end[s];
      const double idf = s_idf[s];
      int64_t done = 0;
      for (;;) {
        const int64_t i = lo + done + tid;
        const int64_t d = i < end ? (int64_t)A.dn[i] : (int64_t)1 << 40;
        const int32_t tf = i < end ? A.tf[i] : 0;  // (with the docno, not behind it: one memory round trip a chunk)
        const int64_t j = d - wbase;
        const bool in = j < kWindow;
        if (in && j >= 0) {
          s_acc[j] += weight(idf, (double)tf, A.k1, s_norm[j]);
          s_touched[j] = 1;
        }
        const int c = __syncthreads_count(in);
        if (tid == c) {  // (c < kNT) the first posting past the window, or the list's end
          const int h = i < end ? (int)((d - A.dmin) / kWindow) : kNoWindow;
          s_cur[s] = i;
          s_head[s] = h;
          if (h != kNoWindow) atomicMin(&s_wmin[nx], h);
        }
        done += c;
        if (c < kNT) break;
      }
      if (tid == 0) n_postings += (unsigned long long)done;
    }
    // sweep (the list has room for a whole window: ncand <= kCand - kWindow here)
#pragma unroll 1
    for (int j = tid; j < kWindow; j += kNT) {
      const double sc = s_acc[j];
      const bool in = s_touched[j] && !(sc < theta);
      const unsigned long long m = __ballot(in);
      if (m) {
        const int l = lane_id();
        int at = 0;
        if (l == (int)__builtin_ctzll(m)) at = atomicAdd(&s_ncand, (int)__builtin_popcountll(m));
        at = __shfl(at, (int)__builtin_ctzll(m), 64);
        if (in) {
          const int p = at + (int)__builtin_popcountll(m & ((1ull << l) - 1ull));
          if (p < kCand) {
            s_ls[p] = sc;
            s_ld[p] = (int32_t)(wbase + j);
          }
        }
      }
    }
    __syncthreads();
    ncand = min(s_ncand, kCand);
    const bool first_bar = ncand >= k && !barred;  // the first k candidates already make a bar: windows can be skipped
    if (ncand > kCand - kWindow || first_bar) {
      const bool full = ncand >= k;
      ncand = bm_sort_cut(s_ls, s_ld, ncand, k);
      if (full) {
        theta = fmax(theta, s_ls[k - 1]);
        if (A.S > 1 && tid == 0) atomicMax(A.bar + q, (unsigned long long)bar_key(theta));
      }
      __syncthreads();
      if (tid == 0) s_ncand = ncand;
    }
  }

  __syncthreads();
  ncand = min(s_ncand, kCand);
  ncand = bm_sort_cut(s_ls, s_ld, ncand, k);
  const int64_t row = (int64_t)blockIdx.x * k;
  for (int i = tid; i < k; i += kNT) {
    A.od[row + i] = i < ncand ? s_ld[i] : -1;
    A.os[row + i] = i < ncand ? s_ls[i] : 0.0;
  }
  if (tid == 0 && n_windows) {
    atomicAdd(A.stat + 0, n_windows);
    if (n_skipped) atomicAdd(A.stat + 1, n_skipped);
    if (n_postings) atomicAdd(A.stat + 2, n_postings);
  }
}

__global__ void k_bm_pads(int32_t *od, double *os, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    od[i] = -1;
    os[i] = 0.0;
  }
}

unsigned grid_for(int64_t n, int64_t per, int64_t cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap));
}

}  // namespace

void prepare_bm25(sme_index *ix, hipStream_t st) {
  if (ix->bm_ready) return;
  sme_ctx *cx = ix->ctx;
  hipEvent_t e0, e1;
  SME_HIP(hipEventCreate(&e0));
  SME_HIP(hipEventCreate(&e1));
  struct Events {
    hipEvent_t a, b;
    ~Events() {
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
    }
  } events{e0, e1};
  SME_HIP(hipEventRecord(e0, st));
  const int64_t V = ix->V, P = ix->P;
  const int64_t span = (V > 0 && P > 0 && ix->dmax >= ix->dmin) ? ix->dmax - ix->dmin + 1 : 0;
  const int64_t nwin = (span + kWindow - 1) / kWindow;
  if (nwin > 0x7FFFFFF0) throw Error(SME_ELIMIT, "bm25: the docno span needs 2^31 windows or more");
  DevBuf len64, cnt, tab;
  len64.pool = cnt.pool = tab.pool = &cx->pool;
  unsigned long long *d_cnt = cnt.as<unsigned long long>(C_N);
  SME_HIP(hipMemsetAsync(d_cnt, 0, C_N * sizeof(unsigned long long), st));
  int32_t *dl = ix->d_bm_dl.as<int32_t>((size_t)span);
  int32_t *mindl = ix->d_bm_mindl.as<int32_t>((size_t)nwin);
  int32_t *maxtf = ix->d_bm_maxtf.as<int32_t>((size_t)V);
  double *idf = ix->d_bm_idf.as<double>((size_t)V);
  const int64_t *off = (const int64_t *)ix->d_off.p;
  const int32_t *dn = (const int32_t *)ix->d_docno_d.p, *tf = (const int32_t *)ix->d_tf_d.p;
  if (span > 0) {
    unsigned long long *len = len64.as<unsigned long long>((size_t)span);
    SME_HIP(hipMemsetAsync(len, 0, (size_t)span * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_bm_len, dim3(grid_for(P, 1024, 16384)), dim3(256), 0, st, dn, tf, P, ix->dmin, span, len, d_cnt);
    SME_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bm_windows, dim3((unsigned)nwin), dim3(256), 0, st, len, span, dl, mindl, d_cnt);
    SME_CHECK_LAUNCH();
  }
  if (V > 0) {
    hipLaunchKernelGGL(k_bm_terms, dim3(grid_for(V, 4, 16384)), dim3(256), 0, st, off, tf, V, maxtf, d_cnt);
    SME_CHECK_LAUNCH();
  }
  unsigned long long h[C_N];
  SME_HIP(hipMemcpyAsync(h, d_cnt, sizeof h, hipMemcpyDeviceToHost, st));
  SME_HIP(hipStreamSynchronize(st));
  if (h[C_RANGE]) throw Error(SME_EINVAL, "bm25: a posting's docno lies outside the index's docno range");
  if (h[C_WIDE]) throw Error(SME_ELIMIT, "bm25: a document's length does not fit 32 bits");
  if (V > 0) {
    // idf by df from the host's libm, as the build's idf tables are (k_term_idf)
    const int64_t D = (int64_t)h[C_DOCS], maxdf = (int64_t)h[C_MAXDF];
    std::vector<double> by_df((size_t)maxdf + 1);
    for (int64_t df = 0; df <= maxdf; df++) by_df[(size_t)df] = bm25::idf_value(D, df);
    double *d_tab = tab.as<double>(by_df.size());
    SME_HIP(hipMemcpyAsync(d_tab, by_df.data(), by_df.size() * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bm_idf, dim3(grid_for(V, 256, 16384)), dim3(256), 0, st, off, V, d_tab, idf);
    SME_CHECK_LAUNCH();
    SME_HIP(hipStreamSynchronize(st));  // (by_df and tab leave scope)
  }
  SME_HIP(hipEventRecord(e1, st));
  SME_HIP(hipEventSynchronize(e1));
  SME_HIP(hipEventElapsedTime(&ix->bm_ms, e0, e1));
  ix->bm_span = span;
  ix->bm_nwin = nwin;
  ix->bm_docs = h[C_DOCS];
  ix->bm_total_len = h[C_LEN];
  ix->bm_max_len = h[C_MAXLEN];
  ix->bm_ready = true;
}

void query_topk_bm25(sme_index *ix, const int32_t *d_terms, const int64_t *d_qoff, const int64_t *h_qoff, int nq, int k,
                     double k1, double b, int32_t *d_out_docno, double *d_out_score, hipStream_t st) {
  sme_ctx *cx = ix->ctx;
  prepare_bm25(ix, st);
  unsigned long long *stat = ix->d_bm_stat.as<unsigned long long>(3);
  SME_HIP(hipMemsetAsync(stat, 0, 3 * sizeof(unsigned long long), st));
  ix->bm_called = true;
  ix->bm_stream = st;
  if (nq <= 0) return;
  const int64_t rows = (int64_t)nq * k;
  if (ix->bm_docs == 0 || h_qoff[nq] == 0) {
    hipLaunchKernelGGL(k_bm_pads, dim3(grid_for(rows, 256, 16384)), dim3(256), 0, st, d_out_docno, d_out_score, rows);
    SME_CHECK_LAUNCH();
    return;
  }
  const int64_t span = ix->bm_span, nwin = ix->bm_nwin;
  const double avgdl = (double)ix->bm_total_len / (double)ix->bm_docs;
  double *norm = ix->d_bm_norm.as<double>((size_t)span);
  hipLaunchKernelGGL(k_bm_norm, dim3(grid_for(span, 256, 16384)), dim3(256), 0, st, (const int32_t *)ix->d_bm_dl.p,
                     span, k1, b, avgdl, norm);
  SME_CHECK_LAUNCH();
  // the split: a few workgroups per CU for small batches, one per query once nq alone gives them
  int64_t S = cx->opt_bm25_split;
  if (S <= 0) {
    int cus = 0;
    SME_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cx->device));
    S = (4 * (int64_t)std::max(cus, 1) + nq - 1) / nq;
  }
  S = std::max<int64_t>(1, std::min<int64_t>({S, nwin, (int64_t)kMaxSplit}));
  if ((int64_t)nq * S > 0x7FFFFFFF) throw Error(SME_ELIMIT, "bm25: 2^31 or more workgroups (queries x bm25_split)");
  ScoreArgs A;
  A.off = (const int64_t *)ix->d_off.p;
  A.dn = (const int32_t *)ix->d_docno_d.p;
  A.tf = (const int32_t *)ix->d_tf_d.p;
  A.idf = (const double *)ix->d_bm_idf.p;
  A.maxtf = (const int32_t *)ix->d_bm_maxtf.p;
  A.mindl = (const int32_t *)ix->d_bm_mindl.p;
  A.norm = norm;
  A.terms = d_terms;
  A.qoff = d_qoff;
  A.V = ix->V;
  A.dmin = ix->dmin;
  A.span = span;
  A.nwin = (int)nwin;
  A.S = (int)S;
  A.k = k;
  A.k1 = k1;
  A.b = b;
  A.avgdl = avgdl;
  A.stat = stat;
  A.bar = nullptr;
  A.od = d_out_docno;
  A.os = d_out_score;
  DevBuf td, ts, bar;
  td.pool = ts.pool = bar.pool = &cx->pool;
  if (S > 1) {
    A.od = td.as<int32_t>((size_t)(rows * S));
    A.os = ts.as<double>((size_t)(rows * S));
    A.bar = bar.as<unsigned long long>((size_t)nq);
    SME_HIP(hipMemsetAsync(A.bar, 0, (size_t)nq * sizeof(unsigned long long), st));
  }
  hipLaunchKernelGGL(k_bm_score, dim3((unsigned)((int64_t)nq * S)), dim3(kNT), 0, st, A);
  SME_CHECK_LAUNCH();
  if (S > 1) {
    merge_rows(A.os, A.od, nullptr, nq, (int)(S * k), k, d_out_docno, d_out_score, nullptr, st);
    SME_HIP(hipStreamSynchronize(st));  // (the rows' buffers go back to the pool)
  }
}

}  // namespace sme
