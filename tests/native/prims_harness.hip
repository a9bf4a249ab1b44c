// prims_harness.hip -- test-only C wrappers over the sort / scan / compaction
// primitives of csrc/sme_sort.hip.  Linked with the product's own build/sme_sort.o
// into libsme_prims.so (never into libsme.so: no test hook enters the product
// ABI), so tests/test_gpu_prims.py runs the product's compiled kernels.
//
// Every wrapper takes host pointers, allocates device buffers, runs the
// primitive on a stream of its own, synchronises and copies the results out.
// Two rules keep a wrong kernel a failed assertion rather than a fault:
//   * every device buffer a primitive may write is followed by kGuard bytes
//     (256 eight-byte elements) of 0xA5, and the whole buffer is filled with
//     0xA5 before the input is copied in; *guard_bad gets one bit per buffer
//     whose guard changed (bit order: see each wrapper);
//   * sort scratch is exactly term_sort_scratch(P) / kv_sort_scratch(n) bytes,
//     so a kernel needing more than the documented scratch trips its guard.
// Return value: an SME_* status; smep_last_error() has the message.
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
using smep::kFill;
using smep::kGuard;

std::string g_err;

struct Stream {
  hipStream_t s = nullptr;
  Stream() { SME_HIP(hipStreamCreate(&s)); }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  void sync() { SME_HIP(hipStreamSynchronize(s)); }
};

int guard_bits(std::initializer_list<const GBuf *> bufs) {
  int bad = 0, bit = 0;
  for (const GBuf *b : bufs) {
    if (b && b->guard_changed()) bad |= 1 << bit;
    bit++;
  }
  return bad;
}

template <typename F>
int guarded(F &&f) {
  g_err.clear();
  try {
    f();
    return SME_OK;
  } catch (const sme::Error &e) {
    g_err = e.what();
    return e.code;
  } catch (const std::exception &e) {
    g_err = e.what();
    return SME_EHIP;
  }
}

template <typename K>
void run_kv_sort(const K *keys, const uint32_t *vals, int64_t n, int bits, bool keys_out, K *out_keys,
                 uint32_t *out_vals, int *which, int *guard_bad) {
  const size_t m = (size_t)std::max<int64_t>(n, 0);
  GBuf k0(m * sizeof(K)), k1(m * sizeof(K)), v0(m * 4), v1(m * 4), scr(sme::kv_sort_scratch(n));
  k0.put(keys, m * sizeof(K));
  v0.put(vals, m * 4);
  Stream st;
  uint32_t *r = sme::kv_sort<K>(k0.as<K>(), v0.as<uint32_t>(), k1.as<K>(), v1.as<uint32_t>(), n, bits,
                                scr.as<uint32_t>(), st.s, keys_out);
  st.sync();
  SME_CHECK_LAUNCH();
  *which = r == v0.as<uint32_t>() ? 0 : r == v1.as<uint32_t>() ? 1 : -1;
  (*which == 1 ? k1 : k0).get(out_keys, m * sizeof(K));
  (*which == 1 ? v1 : v0).get(out_vals, m * 4);
  *guard_bad = guard_bits({&k0, &k1, &v0, &v1, &scr});
}

template <typename K>
void run_sort_pairs(const K *keys, const uint32_t *vals, int64_t n, int bits, K *out_keys, uint32_t *out_vals,
                    int *guard_bad) {
  const size_t m = (size_t)std::max<int64_t>(n, 0);
  GBuf ki(m * sizeof(K)), ko(m * sizeof(K)), vi(m * 4), vo(m * 4);
  ki.put(keys, m * sizeof(K));
  vi.put(vals, m * 4);
  Stream st;
  {
    sme::DevBuf radix;
    sme::sort_pairs<K>(ki.as<K>(), ko.as<K>(), vi.as<uint32_t>(), vo.as<uint32_t>(), n, bits, radix, st.s);
    st.sync();
    SME_CHECK_LAUNCH();
  }
  ko.get(out_keys, m * sizeof(K));
  vo.get(out_vals, m * 4);
  *guard_bad = guard_bits({&ki, &ko, &vi, &vo});
}

template <typename K>
void run_sort_pairs_v64(const K *keys, const uint64_t *vals, int64_t n, int bits, K *out_keys, uint64_t *out_vals,
                        int *guard_bad) {
  const size_t m = (size_t)std::max<int64_t>(n, 0);
  GBuf ki(m * sizeof(K)), ko(m * sizeof(K)), vi(m * 8), vo(m * 8);
  ki.put(keys, m * sizeof(K));
  vi.put(vals, m * 8);
  Stream st;
  {
    sme::DevBuf ia, ib, radix;
    sme::sort_pairs_v64<K>(ki.as<K>(), ko.as<K>(), vals ? vi.as<uint64_t>() : nullptr, vo.as<uint64_t>(), n, bits,
                           ia, ib, radix, st.s);
    st.sync();
    SME_CHECK_LAUNCH();
  }
  ko.get(out_keys, m * sizeof(K));
  vo.get(out_vals, m * 8);  // still the fill pattern when vals == nullptr
  *guard_bad = guard_bits({&ki, &ko, &vi, &vo});
}

template <typename T>
void run_excl_scan(const T *in, T *out, int64_t n, bool inplace, int *guard_bad) {
  const size_t m = (size_t)std::max<int64_t>(n, 0);
  GBuf a(m * sizeof(T)), b(inplace ? 0 : m * sizeof(T));
  a.put(in, m * sizeof(T));
  Stream st;
  {
    sme::DevBuf scratch;
    sme::excl_scan<T>(a.as<T>(), inplace ? a.as<T>() : b.as<T>(), n, scratch, st.s);
    st.sync();
    SME_CHECK_LAUNCH();
  }
  (inplace ? a : b).get(out, m * sizeof(T));
  *guard_bad = guard_bits({&a, &b});
}

template <typename T>
void run_reduce_max(const T *in, int64_t n, T *out, int *guard_bad) {
  const size_t m = (size_t)std::max<int64_t>(n, 0);
  GBuf a(m * sizeof(T)), r(sizeof(T));  // *d_max starts as the fill pattern, not 0
  a.put(in, m * sizeof(T));
  Stream st;
  sme::reduce_max<T>(a.as<T>(), n, r.as<T>(), st.s);
  st.sync();
  SME_CHECK_LAUNCH();
  r.get(out, sizeof(T));
  *guard_bad = guard_bits({&a, &r});
}

}  // namespace

extern "C" {

#define SMEP_API __attribute__((visibility("default")))

SMEP_API const char *smep_last_error(void) { return g_err.c_str(); }
SMEP_API int64_t smep_guard_elems(void) { return (int64_t)(kGuard / 8); }
SMEP_API int smep_fill_byte(void) { return kFill; }
SMEP_API uint64_t smep_term_sort_scratch(int64_t P) { return (uint64_t)sme::term_sort_scratch(P); }
SMEP_API uint64_t smep_kv_sort_scratch(int64_t n) { return (uint64_t)sme::kv_sort_scratch(n); }

// kv_sort<uint32_t | uint64_t> (key_bytes 4 | 8).  *which: 0 = the sort returned
// v0 (the input buffers), 1 = v1; out_keys / out_vals are read from that pair.
// guard bits: k0, k1, v0, v1, scratch.
SMEP_API int smep_kv_sort(int key_bytes, const void *keys, const uint32_t *vals, int64_t n, int bits, int keys_out,
                          void *out_keys, uint32_t *out_vals, int *which, int *guard_bad) {
  return guarded([&] {
    if (key_bytes == 4)
      run_kv_sort<uint32_t>((const uint32_t *)keys, vals, n, bits, keys_out != 0, (uint32_t *)out_keys, out_vals,
                            which, guard_bad);
    else if (key_bytes == 8)
      run_kv_sort<uint64_t>((const uint64_t *)keys, vals, n, bits, keys_out != 0, (uint64_t *)out_keys, out_vals,
                            which, guard_bad);
    else
      throw sme::Error(SME_EINVAL, "key_bytes must be 4 or 8");
  });
}

// sort_pairs<K>: results read from keys_out / vals_out.  guard bits: keys_in,
// keys_out, vals_in, vals_out.
SMEP_API int smep_sort_pairs(int key_bytes, const void *keys, const uint32_t *vals, int64_t n, int bits,
                             void *out_keys, uint32_t *out_vals, int *guard_bad) {
  return guarded([&] {
    if (key_bytes == 4)
      run_sort_pairs<uint32_t>((const uint32_t *)keys, vals, n, bits, (uint32_t *)out_keys, out_vals, guard_bad);
    else if (key_bytes == 8)
      run_sort_pairs<uint64_t>((const uint64_t *)keys, vals, n, bits, (uint64_t *)out_keys, out_vals, guard_bad);
    else
      throw sme::Error(SME_EINVAL, "key_bytes must be 4 or 8");
  });
}

// sort_pairs_v64<K>: vals may be NULL (vals_in == nullptr; out_vals then comes
// back as the untouched fill pattern).  guard bits as smep_sort_pairs.
SMEP_API int smep_sort_pairs_v64(int key_bytes, const void *keys, const uint64_t *vals, int64_t n, int bits,
                                 void *out_keys, uint64_t *out_vals, int *guard_bad) {
  return guarded([&] {
    if (key_bytes == 4)
      run_sort_pairs_v64<uint32_t>((const uint32_t *)keys, vals, n, bits, (uint32_t *)out_keys, out_vals, guard_bad);
    else if (key_bytes == 8)
      run_sort_pairs_v64<uint64_t>((const uint64_t *)keys, vals, n, bits, (uint64_t *)out_keys, out_vals, guard_bad);
    else
      throw sme::Error(SME_EINVAL, "key_bytes must be 4 or 8");
  });
}

// term_sort.  keys / vals: nslots source elements (direct mode: nslots >= P, pair
// x at x; gather mode: reg / xoff non-NULL, nrec records, pair x of record i at
// reg[i] + x - xoff[i] < nslots).  lut: nlut doubles or NULL (then no weights).
// xw: W (x, y) u32 pairs or NULL (K6b, with Pout).  The outputs hold nout >=
// max(P, Pout) elements: out_keys from the returned key buffer (*which: 0 = k0,
// 1 = k1), out_docno / out_tf / out_w from buffers that start as the fill
// pattern.  guard bits: k0, k1, v0, v1, docno, tf, w, scratch.
SMEP_API int smep_term_sort(const uint32_t *keys, const uint32_t *vals, int64_t nslots, int64_t nrec,
                            const int64_t *reg, const int64_t *xoff, int64_t P, int bits, int64_t dmin, uint32_t F,
                            const double *lut, int64_t nlut, double idf, int maxbits, const uint32_t *xw, int64_t W,
                            int64_t Pout, int64_t nout, uint32_t *out_keys, int32_t *out_docno, int32_t *out_tf,
                            double *out_w, int *which, int *guard_bad) {
  return guarded([&] {
    if (P < 0 || nslots < 0 || nout < std::max(P, Pout) || (reg == nullptr) != (xoff == nullptr) ||
        (reg == nullptr && nslots < P))
      throw sme::Error(SME_EINVAL, "smep_term_sort: inconsistent sizes");
    const size_t a = (size_t)std::max(nslots, nout), b = (size_t)nout;
    GBuf k0(a * 4), k1(b * 4), v0(a * 4), v1(b * 4), dn(b * 4), tf(b * 4), w(lut ? b * 8 : 0);
    GBuf scr(sme::term_sort_scratch(P));
    GBuf dreg(reg ? (size_t)nrec * 8 : 0), dxoff(reg ? (size_t)(nrec + 1) * 8 : 0);
    GBuf dlut(lut ? (size_t)nlut * 8 : 0), dxw(xw ? (size_t)W * 8 : 0);
    k0.put(keys, (size_t)nslots * 4);
    v0.put(vals, (size_t)nslots * 4);
    dreg.put(reg, (size_t)nrec * 8);
    dxoff.put(xoff, (size_t)(nrec + 1) * 8);
    dlut.put(lut, (size_t)nlut * 8);
    dxw.put(xw, (size_t)W * 8);
    Stream st;
    uint32_t *r = sme::term_sort(k0.as<uint32_t>(), v0.as<uint32_t>(), k1.as<uint32_t>(), v1.as<uint32_t>(), nrec,
                                 reg ? dreg.as<int64_t>() : nullptr, reg ? dxoff.as<int64_t>() : nullptr, P, bits,
                                 dmin, F, dn.as<int32_t>(), tf.as<int32_t>(), scr.as<uint32_t>(), st.s,
                                 lut ? dlut.as<double>() : nullptr, idf, lut ? w.as<double>() : nullptr, maxbits,
                                 xw ? dxw.as<uint2>() : nullptr, Pout);
    st.sync();
    SME_CHECK_LAUNCH();
    *which = r == k0.as<uint32_t>() ? 0 : r == k1.as<uint32_t>() ? 1 : -1;
    (*which == 1 ? k1 : k0).get(out_keys, b * 4);
    dn.get(out_docno, b * 4);
    tf.get(out_tf, b * 4);
    if (lut) w.get(out_w, b * 8);
    *guard_bad = guard_bits({&k0, &k1, &v0, &v1, &dn, &tf, &w, &scr});
  });
}

// excl_scan<T>: type 0 = int32, 1 = uint32, 2 = int64.  guard bits: in (the
// output too when inplace), out.
SMEP_API int smep_excl_scan(int type, const void *in, void *out, int64_t n, int inplace, int *guard_bad) {
  return guarded([&] {
    if (type == 0)
      run_excl_scan<int32_t>((const int32_t *)in, (int32_t *)out, n, inplace != 0, guard_bad);
    else if (type == 1)
      run_excl_scan<uint32_t>((const uint32_t *)in, (uint32_t *)out, n, inplace != 0, guard_bad);
    else if (type == 2)
      run_excl_scan<int64_t>((const int64_t *)in, (int64_t *)out, n, inplace != 0, guard_bad);
    else
      throw sme::Error(SME_EINVAL, "excl_scan type must be 0, 1 or 2");
  });
}

// select_flagged: out holds n elements (the fill pattern past *count).  guard
// bits: flag, out, count.
SMEP_API int smep_select_flagged(const uint8_t *flag, int64_t n, int32_t *out, int32_t *count, int *guard_bad) {
  return guarded([&] {
    const size_t m = (size_t)std::max<int64_t>(n, 0);
    GBuf f(m), o(m * 4), c(4);
    f.put(flag, m);
    Stream st;
    {
      sme::DevBuf s1, s2;
      sme::select_flagged(f.as<uint8_t>(), n, o.as<int32_t>(), c.as<int32_t>(), s1, s2, st.s);
      st.sync();
      SME_CHECK_LAUNCH();
    }
    o.get(out, m * 4);
    c.get(count, 4);
    *guard_bad = guard_bits({&f, &o, &c});
  });
}

// reduce_max<T>: type 0 = int32, 2 = int64.  guard bits: in, max.
SMEP_API int smep_reduce_max(int type, const void *in, int64_t n, void *out_max, int *guard_bad) {
  return guarded([&] {
    if (type == 0)
      run_reduce_max<int32_t>((const int32_t *)in, n, (int32_t *)out_max, guard_bad);
    else if (type == 2)
      run_reduce_max<int64_t>((const int64_t *)in, n, (int64_t *)out_max, guard_bad);
    else
      throw sme::Error(SME_EINVAL, "reduce_max type must be 0 or 2");
  });
}

// reduce_by_key_sum: ukeys / sums hold n elements.  guard bits: keys, vals,
// ukeys, sums, runs.
SMEP_API int smep_reduce_by_key_sum(const uint64_t *keys, const int32_t *vals, int64_t n, uint64_t *ukeys,
                                    int32_t *sums, int64_t *runs, int *guard_bad) {
  return guarded([&] {
    const size_t m = (size_t)std::max<int64_t>(n, 0);
    GBuf k(m * 8), v(m * 4), uk(m * 8), s(m * 4), r(8);
    k.put(keys, m * 8);
    v.put(vals, m * 4);
    Stream st;
    {
      sme::DevBuf flags, pos, scan;
      sme::reduce_by_key_sum(k.as<uint64_t>(), v.as<int32_t>(), n, uk.as<uint64_t>(), s.as<int32_t>(),
                             r.as<int64_t>(), flags, pos, scan, st.s);
      st.sync();
      SME_CHECK_LAUNCH();
    }
    uk.get(ukeys, m * 8);
    s.get(sums, m * 4);
    r.get(runs, 8);
    *guard_bad = guard_bits({&k, &v, &uk, &s, &r});
  });
}

}  // extern "C"
