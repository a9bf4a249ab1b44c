// prims_tfsort.hip -- test-only C wrapper over the tf-desc segment sort
// (csrc/sme_tfsort.hip: tf_sort_segments), linked into libsme_prims.so with the
// product's own build/sme_tfsort.o and build/sme_sort.o
// (tests/test_gpu_tfsort.py).
//
// The same discipline as prims_harness.hip: host pointers in, every device buffer
// filled with 0xA5 and followed by kGuard bytes of 0xA5.  The scratch buffers are
// handed over at exactly the sizes sme_internal.hpp documents; the sort runs on
// two streams of its own.  The inputs are read back and must be unchanged.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "prims_guard.hpp"
#include "sme_internal.hpp"

namespace {
using smep::GBuf;

std::string g_err;

// a DevBuf over a guarded buffer's payload: it must not grow, and never frees
struct Lent {
  sme::DevBuf d;
  GBuf &g;
  explicit Lent(GBuf &gb) : g(gb) {
    d.p = gb.p;
    d.cap = gb.bytes;
  }
  bool outgrown() const { return d.p != g.p; }
  ~Lent() {
    if (outgrown()) g.p = nullptr;  // the DevBuf freed the guarded block and owns another
    else d.p = nullptr, d.cap = 0;
  }
};

struct Streams {
  hipStream_t st = nullptr, aux = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  ~Streams() {
    if (fork) (void)hipEventDestroy(fork);
    if (join) (void)hipEventDestroy(join);
    if (aux) (void)hipStreamDestroy(aux);
    if (st) (void)hipStreamDestroy(st);
  }
};

bool same(const GBuf &g, const void *h, size_t n) {
  std::vector<uint8_t> back(n);
  g.get(back.data(), n);
  return n == 0 || memcmp(back.data(), h, n) == 0;
}

}  // namespace

extern "C" {

#define SMEP_API __attribute__((visibility("default")))

SMEP_API const char *smep_tfsort_last_error(void) { return g_err.c_str(); }
SMEP_API int smep_tfsort_max_tf(void) { return sme::kTfSortMaxTf; }

// tf_sort_segments over the CSR off[0..V] (host, ascending, off[0] == 0) of
// P = off[V] postings.  Guard bits: off, docno_d, tf_d, docno_o, tf_o, lists,
// tiles, tcnt, scan, nseg; bit 10: an input buffer's contents changed; bit 11: a
// scratch buffer was asked for more than its documented size.
SMEP_API int smep_tf_sort_segments(const int64_t *off, int64_t V, const int32_t *docno_d, const int32_t *tf_d,
                                   int max_tf, int32_t *docno_o, int32_t *tf_o, int *guard_bad) {
  g_err.clear();
  try {
    if (V < 0 || !off || off[0] != 0) throw sme::Error(SME_EINVAL, "smep_tf_sort_segments: inconsistent sizes");
    const size_t P = (size_t)off[V];
    int64_t ntiles = 0;
    for (int64_t s = 0; s < V; s++) {
      const int64_t n = off[s + 1] - off[s];
      if (n < 0) throw sme::Error(SME_EINVAL, "smep_tf_sort_segments: offsets not ascending");
      if (n > 8192) ntiles += (n + 4095) / 4096;
    }
    const size_t F = (size_t)max_tf + 1, Vs = (size_t)V;
    GBuf doff((Vs + 1) * 8), din(P * 4), tin(P * 4), dout(P * 4), tout(P * 4);
    GBuf lists(3 * (Vs + 1) * 8), tiles((Vs + 1) * 8), tcnt(((size_t)ntiles * F + 2 + (size_t)ntiles) * 4);
    GBuf scan(std::max(((Vs + 1 + 4095) / 4096 + 1) * 8, (((size_t)ntiles * F + 4095) / 4096 + 1) * 4));
    GBuf nseg(4 * 8);
    doff.put(off, (Vs + 1) * 8);
    din.put(docno_d, P * 4);
    tin.put(tf_d, P * 4);
    Streams s;
    SME_HIP(hipStreamCreate(&s.st));
    SME_HIP(hipStreamCreate(&s.aux));
    SME_HIP(hipEventCreateWithFlags(&s.fork, hipEventDisableTiming));
    SME_HIP(hipEventCreateWithFlags(&s.join, hipEventDisableTiming));
    int bad = 0;
    {
      Lent l_lists(lists), l_tiles(tiles), l_tcnt(tcnt), l_scan(scan);
      sme::tf_sort_segments(doff.as<int64_t>(), V, (int64_t)P, din.as<int32_t>(), tin.as<int32_t>(), max_tf,
                            dout.as<int32_t>(), tout.as<int32_t>(), l_lists.d, l_tiles.d, l_tcnt.d, l_scan.d,
                            nseg.as<unsigned long long>(), s.st, s.aux, s.fork, s.join);
      SME_HIP(hipStreamSynchronize(s.st));  // st waited for the auxiliary stream
      SME_CHECK_LAUNCH();
      if (l_lists.outgrown() || l_tiles.outgrown() || l_tcnt.outgrown() || l_scan.outgrown()) bad |= 1 << 11;
    }
    dout.get(docno_o, P * 4);
    tout.get(tf_o, P * 4);
    int bit = 0;
    for (const GBuf *g : {&doff, &din, &tin, &dout, &tout, &lists, &tiles, &tcnt, &scan, &nseg}) {
      if (g->p && g->guard_changed()) bad |= 1 << bit;
      bit++;
    }
    if (!same(doff, off, (Vs + 1) * 8) || !same(din, docno_d, P * 4) || !same(tin, tf_d, P * 4)) bad |= 1 << 10;
    *guard_bad = bad;
    return SME_OK;
  } catch (const sme::Error &e) {
    g_err = e.what();
    return e.code;
  } catch (const std::exception &e) {
    g_err = e.what();
    return SME_EHIP;
  }
}

}  // extern "C"
