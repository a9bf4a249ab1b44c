// sme_vunion.hip -- what the shard-piece merge (sme_merge.hip) and the index merge
// (sme_ixmerge.hip) share: the vocabulary union of their sources and the reducer's
// final (term, tf desc) order.  sme_internal.hpp has the contracts.
//
//   union   k_rank        every source term's rank among the other sources' terms
//           k_segments    the segment at every rank position: its source term, its
//                         posting list, the first-occurrence flag as a scan input
//           (scan)        flags -> merged ids
//           k_merged_ids  merged id of every segment and source term, every merged
//                         term's first segment and string length, the shared terms
//           (scans)       list lengths -> pstart, string lengths -> d_term_off
//           k_term_chars  the strings, one wave per merged term
//   order   k_keys_term_tf, kv_sort<uint64_t>, k_gather_posts
// Every search ends by a step bound.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sme_internal.hpp"
#include "sme_ixparts.hpp"
#include "sme_recparse.hpp"

namespace sme {

namespace {

constexpr int kNT = 256;

// first term of source p that is >= s (upper: > s); the interval halves every step
__device__ int64_t term_bound(const TermSource &p, const uint16_t *s, int64_t ls, bool upper) {
  int64_t lo = 0, hi = p.n;
  for (int it = 0; it < 64 && lo < hi; it++) {
    const int64_t m = lo + ((hi - lo) >> 1);
    const int c = rp::cmp_units(p.tch + p.toff[m], p.toff[m + 1] - p.toff[m], s, ls);
    if (c < 0 || (upper && c == 0))
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}

// rank of every source term in the merged sequence: equal strings adjacent, in
// source order (ord[a]: source a's place in it); first: no earlier source holds it
__global__ void k_rank(const TermSource *in, int n, const int64_t *base, const int32_t *ord, int64_t Vt, int64_t *pos,
                       uint8_t *first_at) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < Vt; j += (int64_t)gridDim.x * blockDim.x) {
    const int a = input_of(base, n, j);
    const int64_t i = j - base[a];
    const uint16_t *s = in[a].tch + in[a].toff[i];
    const int64_t ls = in[a].toff[i + 1] - in[a].toff[i];
    int64_t r = i;
    bool first = true;
    for (int b = 0; b < n; b++) {
      if (b == a || in[b].n == 0) continue;
      const int64_t lb = term_bound(in[b], s, ls, false);
      if (ord[b] < ord[a]) {
        const int64_t ub = term_bound(in[b], s, ls, true);
        r += ub;
        if (ub > lb) first = false;
      } else {
        r += lb;
      }
    }
    pos[j] = r;
    first_at[r] = first ? 1 : 0;
  }
}
// the segment at every rank position
__global__ void k_segments(const TermSource *in, int n, const int64_t *base, int64_t Vt, const int64_t *pos,
                           int64_t *at_pos, int64_t *cnt_at, const int32_t **key, const int32_t **val,
                           const uint8_t *first_at, int64_t *flag64) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < Vt; j += (int64_t)gridDim.x * blockDim.x) {
    const int a = input_of(base, n, j);
    const int64_t i = j - base[a], r = pos[j], p0 = in[a].off[i];
    at_pos[r] = j;
    cnt_at[r] = in[a].off[i + 1] - p0;
    key[r] = in[a].dn + p0;
    val[r] = in[a].tf + p0;
    flag64[j] = first_at[j];
  }
}
// merged id of every segment, first segment of every merged term, old id -> merged
// id of every source term, the length of every merged term's string, and (shared
// given) the count of merged terms that two or more sources hold
__global__ void k_merged_ids(const TermSource *in, int n, const int64_t *base, const uint8_t *first_at,
                             const int64_t *excl, const int64_t *at_pos, int64_t Vt, int32_t *gid, int64_t *gstart,
                             int32_t *tmap, int64_t *glen, unsigned long long *shared) {
  const int64_t span = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r0 = blockIdx.x * (int64_t)blockDim.x; r0 < Vt; r0 += span) {
    const int64_t r = r0 + threadIdx.x;
    bool hit = false;
    if (r < Vt) {
      const int64_t g = excl[r] + first_at[r] - 1, j = at_pos[r];
      gid[r] = (int32_t)g;
      tmap[j] = (int32_t)g;
      if (first_at[r]) {
        const int a = input_of(base, n, j);
        const int64_t i = j - base[a];
        gstart[g] = r;
        glen[g] = in[a].toff[i + 1] - in[a].toff[i];
      } else {
        hit = first_at[r - 1] != 0;  // the second source of its term
      }
    }
    const unsigned long long m = __ballot(hit);
    if (shared && (threadIdx.x & 63) == 0 && m) atomicAdd(shared, (unsigned long long)__popcll(m));
  }
}
// merged term strings from every term's first source: one wave per term
__global__ void k_term_chars(const TermSource *in, int n, const int64_t *base, const int64_t *gstart,
                             const int64_t *at_pos, int64_t V, const int64_t *goff, uint16_t *gch) {
  const int lane = threadIdx.x & 63;
  const int64_t wpb = blockDim.x / 64;
  for (int64_t g = blockIdx.x * wpb + (threadIdx.x >> 6); g < V; g += (int64_t)gridDim.x * wpb) {
    const int64_t j = at_pos[gstart[g]];
    const int a = input_of(base, n, j);
    const int64_t i = j - base[a];
    const uint16_t *s = in[a].tch + in[a].toff[i];
    const int64_t l = goff[g + 1] - goff[g];
    for (int64_t k = lane; k < l; k += 64) gch[goff[g] + k] = s[k];
  }
}
__global__ void k_concat_off(const int64_t *pstart, const int64_t *gstart, int64_t V, int64_t *off) {
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < V; g += (int64_t)gridDim.x * blockDim.x)
    off[g] = pstart[gstart[g]];
}

// (term, tf desc) keys of the items in `perm` order (perm: nullptr = identity)
__global__ void k_keys_term_tf(const uint32_t *term, const int32_t *tf, const uint32_t *perm, int64_t n, int tfb,
                               uint32_t mtf, uint64_t *k, uint32_t *v) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t x = perm ? perm[i] : (uint32_t)i;
    k[i] = ((uint64_t)term[x] << tfb) | (uint64_t)(mtf - (uint32_t)tf[x]);
    v[i] = x;
  }
}
__global__ void k_gather_posts(const uint32_t *perm, const int32_t *dn, const int32_t *tf, int64_t n, int32_t *odn,
                               int32_t *otf) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t x = perm[i];
    odn[i] = dn[x];
    otf[i] = tf[x];
  }
}

}  // namespace

VocabUnion union_vocab(const TermSource *d_src, int n, const int64_t *d_tbase, const int32_t *d_ord, int64_t Vt,
                       sme_index *ix, unsigned long long *d_shared, UnionScratch s, hipStream_t st) {
  int64_t V = 0;
  int64_t *pos = s.pos.as<int64_t>((size_t)Vt + 1), *at_pos = s.at_pos.as<int64_t>((size_t)Vt + 1);
  uint8_t *first_at = s.first_at.as<uint8_t>((size_t)Vt + 1);
  int64_t *cnt_at = s.cnt_at.as<int64_t>((size_t)Vt + 1), *pstart = s.pstart.as<int64_t>((size_t)Vt + 1);
  int64_t *excl = s.excl.as<int64_t>((size_t)Vt + 1);
  const int32_t **seg_key = (const int32_t **)s.seg_key.as<uint64_t>((size_t)Vt + 1);
  const int32_t **seg_val = (const int32_t **)s.seg_val.as<uint64_t>((size_t)Vt + 1);
  int32_t *gid = s.gid.as<int32_t>((size_t)Vt + 1), *tmap = s.tmap.as<int32_t>((size_t)Vt + 1);
  int64_t *gstart = s.gstart.as<int64_t>((size_t)Vt + 2), *glen = s.glen.as<int64_t>((size_t)Vt + 2);
  if (Vt > 0) {
    hipLaunchKernelGGL(k_rank, dim3(grid_n(Vt)), dim3(kNT), 0, st, d_src, n, d_tbase, d_ord, Vt, pos, first_at);
    hipLaunchKernelGGL(k_segments, dim3(grid_n(Vt)), dim3(kNT), 0, st, d_src, n, d_tbase, Vt, (const int64_t *)pos,
                       at_pos, cnt_at, seg_key, seg_val, (const uint8_t *)first_at, excl);
    SME_CHECK_LAUNCH();
    excl_scan<int64_t>(excl, excl, Vt, s.scan, st);
    hipLaunchKernelGGL(k_merged_ids, dim3(grid_n(Vt)), dim3(kNT), 0, st, d_src, n, d_tbase, (const uint8_t *)first_at,
                       (const int64_t *)excl, (const int64_t *)at_pos, Vt, gid, gstart, tmap, glen, d_shared);
    SME_CHECK_LAUNCH();
    V = (int64_t)rd1(gid + Vt - 1, st) + 1;
  }
  SME_HIP(hipMemsetAsync(cnt_at + Vt, 0, sizeof(int64_t), st));
  excl_scan<int64_t>(cnt_at, pstart, Vt + 1, s.scan, st);
  SME_HIP(hipMemcpyAsync(gstart + V, &Vt, sizeof(int64_t), hipMemcpyHostToDevice, st));
  ix->V = ix->Vt = V;
  int64_t *term_off = ix->d_term_off.as<int64_t>((size_t)V + 1);
  if (V > 0) {
    SME_HIP(hipMemsetAsync(glen + V, 0, sizeof(int64_t), st));
    excl_scan<int64_t>(glen, term_off, V + 1, s.scan, st);
    const int64_t tchars = rd1(term_off + V, st);
    uint16_t *gch = ix->d_term_chars.as<uint16_t>((size_t)tchars + 1);
    hipLaunchKernelGGL(k_term_chars, dim3(grid_n(V * 64)), dim3(kNT), 0, st, d_src, n, d_tbase, (const int64_t *)gstart,
                       (const int64_t *)at_pos, V, (const int64_t *)term_off, gch);
    SME_CHECK_LAUNCH();
  } else {
    SME_HIP(hipMemsetAsync(term_off, 0, sizeof(int64_t), st));
    ix->d_term_chars.get(16);
  }
  SME_HIP(hipStreamSynchronize(st));  // (the host word gstart[V] was copied from)
  return VocabUnion{V, pos, at_pos, first_at, gid, gstart, tmap, pstart, seg_key, seg_val};
}

void segment_term_offsets(const int64_t *pstart, const int64_t *gstart, int64_t V, int64_t *off, hipStream_t st) {
  hipLaunchKernelGGL(k_concat_off, dim3(grid_n(V)), dim3(kNT), 0, st, pstart, gstart, V, off);
  SME_CHECK_LAUNCH();
}

void sort_term_tf(const uint32_t *term, const int32_t *dn, const int32_t *tf, const uint32_t *perm, int64_t P,
                  int64_t V, int max_tf, int32_t *odn, int32_t *otf, DevBuf &q0, DevBuf &q1, DevBuf &v0, DevBuf &v1,
                  DevBuf &radix, hipStream_t st) {
  const int tfb = bits_of((uint64_t)std::max(max_tf, 1));
  uint64_t *k0 = q0.as<uint64_t>((size_t)P), *k1 = q1.as<uint64_t>((size_t)P);
  uint32_t *p0 = v0.as<uint32_t>((size_t)P), *p1 = v1.as<uint32_t>((size_t)P);
  uint32_t *rscr = radix.as<uint32_t>(kv_sort_scratch(P) / sizeof(uint32_t) + 1);
  hipLaunchKernelGGL(k_keys_term_tf, dim3(grid_n(P)), dim3(kNT), 0, st, term, tf, perm, P, tfb, (uint32_t)max_tf, k0, p0);
  const uint32_t *fin = kv_sort<uint64_t>(k0, p0, k1, p1, P, bits_of((uint64_t)std::max<int64_t>(V, 1)) + tfb, rscr, st);
  hipLaunchKernelGGL(k_gather_posts, dim3(grid_n(P)), dim3(kNT), 0, st, fin, dn, tf, P, odn, otf);
  SME_CHECK_LAUNCH();
}

}  // namespace sme
