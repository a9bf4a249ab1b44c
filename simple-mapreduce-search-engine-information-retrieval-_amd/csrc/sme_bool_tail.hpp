// sme_bool_tail.hpp -- the tail that Boolean retrieval (sme_bool.hip) and
// structured queries (sme_structq.hip) share: from the chunk filter's counted
// matches to the ordered and cut result arrays.  The matches are emitted (docno,
// score, query), ordered by stable sorts over an index permutation -- docno, then
// for the score order the score key, then the query -- and gathered below the cut.
// Internal: nothing of it enters include/sme.h.
//
// The kernels stand in an unnamed namespace: each of the two files has its own.
#pragma once
#include <hip/hip_runtime.h>

#include <exception>

#include "sme_bool.hpp"
#include "sme_chunks.hpp"
#include "sme_internal.hpp"

namespace sme {
namespace {
using namespace chunks;

// sort keys of the matches: the docno key and the identity permutation ...
__global__ void k_bool_key_docno(const int32_t *__restrict__ mdoc, int64_t n, uint32_t *__restrict__ key,
                                 uint32_t *__restrict__ perm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    key[i] = boolq::docno_key(mdoc[i]);
    perm[i] = (uint32_t)i;
  }
}
// ... and, through the permutation so far, the score key and the query
__global__ void k_bool_key_score(const double *__restrict__ mscore, const uint32_t *__restrict__ perm, int64_t n,
                                 uint64_t *__restrict__ key) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    key[i] = boolq::score_key(mscore[perm[i]]);
}
__global__ void k_bool_key_query(const uint32_t *__restrict__ mq, const uint32_t *__restrict__ perm, int64_t n,
                                 uint32_t *__restrict__ key) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    key[i] = mq[perm[i]];
}
// Sorted match x (query qs[x], match perm[x]) is the (x - woff[q])-th of its
// query: kept if that is below the cut.
__global__ void k_bool_gather(const uint32_t *__restrict__ qs, const uint32_t *__restrict__ perm,
                              const int32_t *__restrict__ mdoc, const double *__restrict__ mscore, int64_t total,
                              const int64_t *__restrict__ woff, const int64_t *__restrict__ roff, int64_t m,
                              int32_t *__restrict__ out_docno, double *__restrict__ out_score) {
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t q = qs[x];
    const int64_t rk = x - woff[q];
    if (m > 0 && rk >= m) continue;
    const uint32_t i = perm[x];
    out_docno[roff[q] + rk] = mdoc[i];
    out_score[roff[q] + rk] = mscore[i];
  }
}

// The counted matches `c` of filter `op` -> `out`, whose offsets the caller has
// sized for its out.n queries: the result offsets after the cut, docno and score
// sized for them, total and matches (those before the cut); first(i) = query i's
// first range (k_owner_offs).  Synchronises the stream.  The temporaries are
// pooled blocks of the call.
template <class Op, class First>
void bool_tail(sme_ctx *cx, const Op &op, const Counted &c, First first, int order, int m, DocScores &out,
               hipStream_t st) {
  const int nq = out.n;
  int64_t *d_roff = (int64_t *)out.off.p;
  DevBuf wob, kpb, scn, mdb, msb, mqb, ka, kb, pa, pb, pc, sa, sb, radix;
  for (DevBuf *b : {&wob, &kpb, &scn, &mdb, &msb, &mqb, &ka, &kb, &pa, &pb, &pc, &sa, &sb, &radix}) b->pool = &cx->pool;
  // (declared after the temporaries, so it runs before they go back to the pool:
  // on an exception kernels may still read them)
  struct SyncOnUnwind {
    hipStream_t st;
    int live = std::uncaught_exceptions();
    ~SyncOnUnwind() {
      if (std::uncaught_exceptions() > live) (void)hipStreamSynchronize(st);
    }
  } sync_on_unwind{st};
  const int64_t total = c.total;
  int64_t *woff = wob.as<int64_t>((size_t)nq + 1);
  int64_t *kept = kpb.as<int64_t>((size_t)nq + 1);
  hipLaunchKernelGGL(k_owner_offs<First>, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, first, c.choff, c.moff,
                     (int64_t)nq, woff);
  hipLaunchKernelGGL(k_cut, dim3(grid_for((int64_t)nq + 1)), dim3(kNT), 0, st, (const int64_t *)woff, (int64_t)nq,
                     (int64_t)m, kept);
  SME_CHECK_LAUNCH();
  excl_scan<int64_t>(kept, d_roff, (int64_t)nq + 1, scn, st);
  int64_t out_total = 0;
  SME_HIP(hipMemcpyAsync(&out_total, d_roff + nq, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  SME_HIP(hipStreamSynchronize(st));
  int32_t *out_docno = out.alloc<DocScores::docno>(out_total);
  double *out_score = out.alloc<DocScores::score>(out_total);
  if (total > 0) {
    const size_t T = (size_t)total;
    int32_t *mdoc = mdb.as<int32_t>(T);
    double *mscore = msb.as<double>(T);
    uint32_t *mq = mqb.as<uint32_t>(T);
    uint32_t *k0 = ka.as<uint32_t>(T), *k1 = kb.as<uint32_t>(T);
    uint32_t *p0 = pa.as<uint32_t>(T), *p1 = pb.as<uint32_t>(T);
    emit_chunks(op, c, st, mdoc, mscore, mq);
    // least significant key first, every pass stable: docno, (score,) query
    const unsigned g = grid_for(total);
    hipLaunchKernelGGL(k_bool_key_docno, dim3(g), dim3(kNT), 0, st, (const int32_t *)mdoc, total, k0, p0);
    sort_pairs<uint32_t>(k0, k1, p0, p1, total, 32, radix, st);
    uint32_t *perm = p1, *spare = p0;
    if (order == 1) {
      uint64_t *s0 = sa.as<uint64_t>(T), *s1 = sb.as<uint64_t>(T);
      hipLaunchKernelGGL(k_bool_key_score, dim3(g), dim3(kNT), 0, st, (const double *)mscore, (const uint32_t *)perm,
                         total, s0);
      uint32_t *p2 = pc.as<uint32_t>(T);
      sort_pairs<uint64_t>(s0, s1, perm, p2, total, 64, radix, st);
      perm = p2;
    }
    hipLaunchKernelGGL(k_bool_key_query, dim3(g), dim3(kNT), 0, st, (const uint32_t *)mq, (const uint32_t *)perm,
                       total, k0);
    sort_pairs<uint32_t>(k0, k1, perm, spare, total, owner_bits(nq), radix, st);
    hipLaunchKernelGGL(k_bool_gather, dim3(g), dim3(kNT), 0, st, (const uint32_t *)k1, (const uint32_t *)spare,
                       (const int32_t *)mdoc, (const double *)mscore, total, (const int64_t *)woff,
                       (const int64_t *)d_roff, (int64_t)m, out_docno, out_score);
    SME_CHECK_LAUNCH();
  }
  SME_HIP(hipStreamSynchronize(st));
  out.total = out_total;
  out.matches = (uint64_t)total;
}

}  // namespace
}  // namespace sme
