// prims_packed.hip -- test-only C wrapper over term_sort's packed gather mode
// (csrc/sme_sort.hip: rec_val / tf_shift), linked into libsme_prims.so beside
// prims_harness.hip with the product's own build/sme_sort.o
// (tests/test_gpu_term_sort_packed.py).
//
// The same discipline as prims_harness.hip: host pointers in, device buffers
// filled with 0xA5 and followed by kGuard bytes of 0xA5, scratch of exactly
// term_sort_scratch(P) bytes, the sort on a stream of its own.  The first pass
// of this mode must read no value buffer and fewer than three passes must write
// none into v0: v0 is a fill-pattern buffer here and is compared whole.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "prims_guard.hpp"
#include "sme_internal.hpp"

namespace {
using smep::GBuf;

std::string g_err;

}  // namespace

extern "C" {

#define SMEP_API __attribute__((visibility("default")))

SMEP_API const char *smep_packed_last_error(void) { return g_err.c_str(); }

// term_sort in packed gather mode.  words: nslots source words (pair x of record
// i at reg[i] + x - xoff[i] < nslots, term | tf << tf_shift); rec_val: nrec base
// values.  lut: nlut doubles or NULL; xw: W (x, y) u32 pairs or NULL (with Pout).
// The outputs hold nout >= max(P, Pout) elements, as smep_term_sort's.  guard
// bits: k0, k1, v0, v1, docno, tf, w, scratch; bit 8: v0 was written although the
// sort has fewer than three passes.
SMEP_API int smep_term_sort_packed(const uint32_t *words, int64_t nslots, int64_t nrec, const int64_t *reg,
                                   const int64_t *xoff, const uint32_t *rec_val, int tf_shift, int64_t P, int bits,
                                   int64_t dmin, uint32_t F, const double *lut, int64_t nlut, double idf, int maxbits,
                                   const uint32_t *xw, int64_t W, int64_t Pout, int64_t nout, uint32_t *out_keys,
                                   int32_t *out_docno, int32_t *out_tf, double *out_w, int *which, int *guard_bad) {
  g_err.clear();
  try {
    if (P < 0 || nslots < 0 || nrec < 0 || nout < std::max(P, Pout) || !reg || !xoff || !rec_val)
      throw sme::Error(SME_EINVAL, "smep_term_sort_packed: inconsistent sizes");
    const size_t a = (size_t)std::max(nslots, nout), b = (size_t)nout;
    GBuf k0(a * 4), k1(b * 4), v0(b * 4), v1(b * 4), dn(b * 4), tf(b * 4), w(lut ? b * 8 : 0);
    GBuf scr(sme::term_sort_scratch(P));
    GBuf dreg((size_t)nrec * 8), dxoff((size_t)(nrec + 1) * 8), drv((size_t)nrec * 4);
    GBuf dlut(lut ? (size_t)nlut * 8 : 0), dxw(xw ? (size_t)W * 8 : 0);
    k0.put(words, (size_t)nslots * 4);
    dreg.put(reg, (size_t)nrec * 8);
    dxoff.put(xoff, (size_t)(nrec + 1) * 8);
    drv.put(rec_val, (size_t)nrec * 4);
    dlut.put(lut, (size_t)nlut * 8);
    dxw.put(xw, (size_t)W * 8);
    hipStream_t st = nullptr;
    SME_HIP(hipStreamCreate(&st));
    uint32_t *r = nullptr;
    try {
      r = sme::term_sort(k0.as<uint32_t>(), v0.as<uint32_t>(), k1.as<uint32_t>(), v1.as<uint32_t>(), nrec,
                         dreg.as<int64_t>(), dxoff.as<int64_t>(), P, bits, dmin, F, dn.as<int32_t>(), tf.as<int32_t>(),
                         scr.as<uint32_t>(), st, lut ? dlut.as<double>() : nullptr, idf,
                         lut ? w.as<double>() : nullptr, maxbits, xw ? dxw.as<uint2>() : nullptr, Pout,
                         drv.as<uint32_t>(), tf_shift);
      SME_HIP(hipStreamSynchronize(st));
      SME_CHECK_LAUNCH();
    } catch (...) {
      (void)hipStreamDestroy(st);
      throw;
    }
    (void)hipStreamDestroy(st);
    *which = r == k0.as<uint32_t>() ? 0 : r == k1.as<uint32_t>() ? 1 : -1;
    (*which == 1 ? k1 : k0).get(out_keys, b * 4);
    dn.get(out_docno, b * 4);
    tf.get(out_tf, b * 4);
    if (lut) w.get(out_w, b * 8);
    int bad = 0, bit = 0;
    for (const GBuf *g : {&k0, &k1, &v0, &v1, &dn, &tf, &w, &scr}) bad |= (g->guard_changed() ? 1 : 0) << bit++;
    if (sme::term_sort_passes(bits, maxbits) < 3 && v0.changed(0)) bad |= 1 << 8;
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
