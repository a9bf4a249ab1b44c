// prims_termoff.hip -- test-only C wrapper over term_sort's offset output
// (csrc/sme_sort.hip: off_out / V / vend / write_keys, k_rs_term_off), linked
// into libsme_prims.so beside prims_harness.hip with the product's own
// build/sme_sort.o (tests/test_gpu_term_offsets.py).
//
// The same discipline as prims_harness.hip: host pointers in, device buffers
// filled with 0xA5 and followed by kGuard bytes of 0xA5, scratch of exactly
// term_sort_scratch(P) bytes, the sort on a stream of its own.  The offsets
// array has vend + 1 elements and is 0xA5 before the call, so an entry the sort
// does not write reads back as the fill pattern.
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

SMEP_API const char *smep_termoff_last_error(void) { return g_err.c_str(); }

// term_sort with off_out.  keys / vals: nslots source elements (vals NULL in the
// packed gather mode, where rec_val holds nrec base values and keys the packed
// words); reg / xoff: gather mode, or NULL.  lut: nlut doubles or NULL; xw: W
// (x, y) u32 pairs or NULL (with Pout).  V term ids, the pair count at
// out_off[vend]; out_off holds vend + 1 elements, the other outputs nout >=
// max(P, Pout).  out_keys: the whole returned key buffer, whether or not the last
// pass wrote it (write_keys).  guard bits: k0, k1, v0, v1, docno, tf, w, scratch,
// off.
SMEP_API int smep_term_sort_off(const uint32_t *keys, const uint32_t *vals, int64_t nslots, int64_t nrec,
                                const int64_t *reg, const int64_t *xoff, const uint32_t *rec_val, int tf_shift,
                                int64_t P, int bits, int64_t dmin, uint32_t F, const double *lut, int64_t nlut,
                                double idf, int maxbits, const uint32_t *xw, int64_t W, int64_t Pout, int64_t nout,
                                int64_t V, int64_t vend, int write_keys, uint32_t *out_keys, int32_t *out_docno,
                                int32_t *out_tf, double *out_w, int64_t *out_off, int *which, int *guard_bad) {
  g_err.clear();
  try {
    if (P < 0 || nslots < 0 || nrec < 0 || nout < std::max(P, Pout) || (reg == nullptr) != (xoff == nullptr) ||
        (reg == nullptr && nslots < P) || (rec_val != nullptr && reg == nullptr) || V < 0 || vend < V ||
        (xw != nullptr && W < V))
      throw sme::Error(SME_EINVAL, "smep_term_sort_off: inconsistent sizes");
    const size_t a = (size_t)std::max(nslots, nout), b = (size_t)nout;
    GBuf k0(a * 4), k1(b * 4), v0(a * 4), v1(b * 4), dn(b * 4), tf(b * 4), w(lut ? b * 8 : 0);
    GBuf scr(sme::term_sort_scratch(P));
    GBuf dreg(reg ? (size_t)nrec * 8 : 0), dxoff(reg ? (size_t)(nrec + 1) * 8 : 0), drv(rec_val ? (size_t)nrec * 4 : 0);
    GBuf dlut(lut ? (size_t)nlut * 8 : 0), dxw(xw ? (size_t)W * 8 : 0), doff((size_t)(vend + 1) * 8);
    k0.put(keys, (size_t)nslots * 4);
    v0.put(vals, (size_t)nslots * 4);
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
                         reg ? dreg.as<int64_t>() : nullptr, reg ? dxoff.as<int64_t>() : nullptr, P, bits, dmin, F,
                         dn.as<int32_t>(), tf.as<int32_t>(), scr.as<uint32_t>(), st, lut ? dlut.as<double>() : nullptr,
                         idf, lut ? w.as<double>() : nullptr, maxbits, xw ? dxw.as<uint2>() : nullptr, Pout,
                         rec_val ? drv.as<uint32_t>() : nullptr, tf_shift, doff.as<int64_t>(), V, vend,
                         write_keys != 0);
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
    doff.get(out_off, (size_t)(vend + 1) * 8);
    int bad = 0, bit = 0;
    for (const GBuf *g : {&k0, &k1, &v0, &v1, &dn, &tf, &w, &scr, &doff}) bad |= (g->guard_changed() ? 1 : 0) << bit++;
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
