// sme_api.hip -- the C-ABI (include/sme.h).  Every entry point converts
// sme::Error / std::exception into a negative status and a thread-local message.
#include <hip/hip_runtime.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include <algorithm>
#include <system_error>
#include <thread>

#include "sme_bm25.hpp"
#include "sme_passage.hpp"
#include "sme_rescore.hpp"
#include "sme_feedback.hpp"
#include "sme_internal.hpp"
#include "sme_ixmerge.hpp"
#include "sme_ixdelete.hpp"

namespace {
thread_local std::string g_err;

int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

template <typename F>
int guard(F &&f) {
  try {
    f();
    g_err.clear();
    return SME_OK;
  } catch (const sme::Error &e) {
    return fail(e.code, e.what());
  } catch (const std::bad_alloc &) {
    return fail(SME_ENOMEM, "host allocation failed");
  } catch (const std::exception &e) {
    return fail(SME_EINVAL, e.what());
  }
}

hipStream_t stream_of(sme_ctx *cx, void *s) { return s ? (hipStream_t)s : cx->own_stream; }

// merged shard pieces (sme_merge_pieces) hold the reduce output only
void need_query_side(const sme_index *ix) {
  if (ix->records_only)
    throw sme::Error(SME_EINVAL, "records-only index (merged shard pieces): query the shard indexes");
}

// an index loaded from record streams holds the doc counter's bytes, not every record's docno
void need_record_docnos(const sme_index *ix) {
  if (ix->from_records)
    throw sme::Error(SME_EINVAL, "index loaded from records: the doc counter never holds a map task's last docno");
}

void set_device(sme_ctx *cx) { SME_HIP(hipSetDevice(cx->device)); }

// DataInput.readUTF body -> UTF-16
bool read_mutf8(const uint8_t *p, size_t len, std::vector<uint16_t> &out) {
  size_t i = 0;
  while (i < len) {
    unsigned c = p[i];
    if (c < 0x80) {
      out.push_back((uint16_t)c);
      i++;
    } else if ((c & 0xE0) == 0xC0) {
      if (i + 1 >= len) return false;
      out.push_back((uint16_t)(((c & 0x1F) << 6) | (p[i + 1] & 0x3F)));
      i += 2;
    } else if ((c & 0xF0) == 0xE0) {
      if (i + 2 >= len) return false;
      out.push_back((uint16_t)(((c & 0x0F) << 12) | ((p[i + 1] & 0x3F) << 6) | (p[i + 2] & 0x3F)));
      i += 3;
    } else {
      return false;
    }
  }
  return true;
}

// standard UTF-8 -> UTF-16 (API inputs of already-processed terms)
std::vector<uint16_t> utf8_to_u16(const uint8_t *p, size_t n) {
  std::vector<uint16_t> o;
  size_t i = 0;
  while (i < n) {
    unsigned c = p[i];
    unsigned cp;
    int extra;
    if (c < 0x80) {
      cp = c;
      extra = 0;
    } else if ((c & 0xE0) == 0xC0) {
      cp = c & 0x1F;
      extra = 1;
    } else if ((c & 0xF0) == 0xE0) {
      cp = c & 0x0F;
      extra = 2;
    } else {
      cp = c & 0x07;
      extra = 3;
    }
    i++;
    for (int k = 0; k < extra && i < n; k++, i++) cp = (cp << 6) | (p[i] & 0x3F);
    if (cp >= 0x10000) {
      cp -= 0x10000;
      o.push_back((uint16_t)(0xD800 + (cp >> 10)));
      o.push_back((uint16_t)(0xDC00 + (cp & 0x3FF)));
    } else {
      o.push_back((uint16_t)cp);
    }
  }
  return o;
}

// DataOutput.writeUTF body of UTF-16 units
void u16_to_mutf8(const uint16_t *u, size_t n, std::vector<uint8_t> &o) {
  for (size_t i = 0; i < n; i++) {
    uint16_t c = u[i];
    if (c >= 1 && c <= 0x7F) {
      o.push_back((uint8_t)c);
    } else if (c > 0x7FF) {
      o.push_back((uint8_t)(0xE0 | ((c >> 12) & 0x0F)));
      o.push_back((uint8_t)(0x80 | ((c >> 6) & 0x3F)));
      o.push_back((uint8_t)(0x80 | (c & 0x3F)));
    } else {
      o.push_back((uint8_t)(0xC0 | ((c >> 6) & 0x1F)));
      o.push_back((uint8_t)(0x80 | (c & 0x3F)));
    }
  }
}

void ensure_host_terms(sme_index *ix) {
  if (ix->h_terms_ready) return;
  const int64_t Vt = ix->Vt;
  ix->h_term_off.resize(Vt + 1);
  SME_HIP(hipMemcpy(ix->h_term_off.data(), ix->d_term_off.p, (Vt + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  ix->h_term_chars.resize(ix->h_term_off[Vt] + 1);
  if (ix->h_term_off[Vt] > 0)
    SME_HIP(hipMemcpy(ix->h_term_chars.data(), ix->d_term_chars.p, ix->h_term_off[Vt] * sizeof(uint16_t),
                      hipMemcpyDeviceToHost));
  if (ix->K > 1 && ix->V > 0 && ix->d_gram.p) {  // (a merged K >= 2 index holds joined gram strings instead)
    ix->h_gram.resize((size_t)(ix->V * ix->K));
    SME_HIP(hipMemcpy(ix->h_gram.data(), ix->d_gram.p, ix->h_gram.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  ix->h_terms_ready = true;
}

// Device -> host copy of n bytes at d into dst.  Pinned dst (hipHostMalloc /
// hipHostRegister memory): one DMA.  Pageable dst: 64 MiB chunks DMA'd into
// the context's two pinned staging buffers while the host copies the previous
// chunk out of the other buffer, spread over up to 8 threads (one host thread
// moves ~10 GB/s; PCIe Gen5 x16 ~50 GB/s).  A plain pageable hipMemcpy of the
// c2 record stream ran at ~2 GB/s.
void copy_d2h(sme_ctx *cx, void *dst, const void *d, size_t n, hipStream_t st) {
  if (!n) return;
  hipPointerAttribute_t at{};
  bool pinned = false;
  if (hipPointerGetAttributes(&at, dst) == hipSuccess)
    pinned = at.type == hipMemoryTypeHost;
  else
    (void)hipGetLastError();  // pageable memory: not an error for the caller
  if (pinned) {
    SME_HIP(hipMemcpyAsync(dst, d, n, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    return;
  }
  constexpr size_t kStage = size_t(64) << 20;
  if (!cx->h_stage[0]) {
    for (auto &b : cx->h_stage) SME_HIP(hipHostMalloc(&b, kStage, hipHostMallocDefault));
    cx->h_stage_cap = kStage;
  }
  hipEvent_t ev[2];
  for (auto &e : ev) SME_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const size_t nch = (n + kStage - 1) / kStage;
  auto issue = [&](size_t c) {
    const size_t o = c * kStage, len = std::min(kStage, n - o);
    SME_HIP(hipMemcpyAsync(cx->h_stage[c & 1], (const uint8_t *)d + o, len, hipMemcpyDeviceToHost, st));
    SME_HIP(hipEventRecord(ev[c & 1], st));
  };
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const unsigned nth = std::min(8u, hw);
  try {
    issue(0);
    for (size_t c = 0; c < nch; c++) {
      SME_HIP(hipEventSynchronize(ev[c & 1]));
      if (c + 1 < nch) issue(c + 1);  // the other buffer's chunk was copied out last iteration
      const size_t o = c * kStage, len = std::min(kStage, n - o);
      const uint8_t *src = (const uint8_t *)cx->h_stage[c & 1];
      uint8_t *out = (uint8_t *)dst + o;
      const unsigned t = len >= (size_t(8) << 20) ? nth : 1u;
      const size_t per = (len + t - 1) / t;
      std::vector<std::thread> th;
      struct Joiner {  // joins every started thread on any exit (a joinable std::thread's destructor aborts)
        std::vector<std::thread> &v;
        ~Joiner() {
          for (auto &x : v)
            if (x.joinable()) x.join();
        }
      } joiner{th};
      for (unsigned i = 1; i < t; i++) {
        const size_t lo = std::min(len, i * per), hi = std::min(len, lo + per);
        if (hi <= lo) continue;
        try {
          th.emplace_back([=] { memcpy(out + lo, src + lo, hi - lo); });
        } catch (const std::system_error &) {  // no thread (EAGAIN): copy this slice here
          memcpy(out + lo, src + lo, hi - lo);
        }
      }
      memcpy(out, src, std::min(len, per));
    }
  } catch (...) {
    (void)hipStreamSynchronize(st);
    for (auto &e : ev) (void)hipEventDestroy(e);
    throw;
  }
  for (auto &e : ev) (void)hipEventDestroy(e);
}
}  // namespace

extern "C" {

const char *sme_last_error(void) { return g_err.c_str(); }

int sme_device_alloc(int device, size_t n, void **d) {
  return guard([&] {
    if (!d) throw sme::Error(SME_EINVAL, "null argument");
    SME_HIP(hipSetDevice(device));
    *d = nullptr;
    SME_HIP(hipMalloc(d, n ? n : 16));
  });
}

void sme_device_free(void *d) {
  if (d) (void)hipFree(d);
}

int sme_memcpy(void *dst, const void *src, size_t n, void *stream) {
  return guard([&] {
    if (n == 0) return;
    if (!dst || !src) throw sme::Error(SME_EINVAL, "null argument");
    if (stream)
      SME_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, (hipStream_t)stream));
    else
      SME_HIP(hipMemcpy(dst, src, n, hipMemcpyDefault));
  });
}
const char *sme_version(void) { return "sme 0.1 (gfx950)"; }

int sme_create(const sme_config *cfg, sme_ctx **out) {
  return guard([&] {
    if (!cfg || !out) throw sme::Error(SME_EINVAL, "null argument");
    if (cfg->k < 1) throw sme::Error(SME_EINVAL, "k must be >= 1");
    if (cfg->num_partitions < 1) throw sme::Error(SME_EINVAL, "num_partitions must be >= 1");
    if (cfg->idf_mode != SME_IDF_REFERENCE && cfg->idf_mode != SME_IDF_TRUE_DF)
      throw sme::Error(SME_EINVAL, "bad idf_mode");
    if (cfg->tiebreak != SME_TIE_DOCNO && cfg->tiebreak != SME_TIE_REFERENCE && cfg->tiebreak != SME_TIE_JAVA7)
      throw sme::Error(SME_EINVAL, "bad tiebreak");
    int ndev = 0;
    SME_HIP(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) throw sme::Error(SME_EINVAL, "bad device ordinal");
    sme_ctx *cx = new sme_ctx();
    cx->cfg = *cfg;
    cx->device = cfg->device;
    try {
      set_device(cx);
      SME_HIP(hipStreamCreateWithFlags(&cx->own_stream, hipStreamNonBlocking));
      SME_HIP(hipStreamCreateWithFlags(&cx->aux_stream, hipStreamNonBlocking));
      SME_HIP(hipEventCreateWithFlags(&cx->ev_fork, hipEventDisableTiming));
      SME_HIP(hipEventCreateWithFlags(&cx->ev_join, hipEventDisableTiming));
    } catch (...) {
      delete cx;
      throw;
    }
    *out = cx;
  });
}

int sme_set_option(sme_ctx *cx, const char *name, int64_t v) {
  return guard([&] {
    if (!cx || !name) throw sme::Error(SME_EINVAL, "null argument");
    const std::string n(name);
    auto range = [&](int64_t lo, int64_t hi) {
      if (v < lo || v > hi) throw sme::Error(SME_EINVAL, "option " + n + " out of range");
    };
    if (n == "query_kernel") {
      range(0, 2);
      cx->opt_query_kernel = v;
    } else if (n == "heavy_div") {
      range(0, int64_t(1) << 40);
      cx->opt_heavy_div = v;
    } else if (n == "seed_tiles") {
      range(0, 8);
      cx->opt_seed_tiles = v;
    } else if (n == "query_order") {
      range(0, 1);
      cx->opt_query_order = v;
    } else if (n == "agg_two_pass") {
      range(0, 1);
      cx->opt_agg_two_pass = v;
    } else if (n == "agg_grid") {
      range(0, int64_t(1) << 30);
      cx->opt_agg_grid = v;
    } else if (n == "tok_grid") {
      range(1, int64_t(1) << 30);
      cx->opt_tok_grid = v;
    } else if (n == "cand_cap") {
      range(1, 2048);
      cx->opt_cand_cap = v;
    } else if (n == "win_sample") {
      range(0, 1);
      cx->opt_win_sample = v;
    } else if (n == "win_stage_min") {
      range(0, int64_t(1) << 20);
      cx->opt_win_stage_min = v;
    } else if (n == "kgram_rank") {
      range(0, 1);
      cx->opt_kgram_rank = v;
    } else if (n == "win_slice") {
      range(0, int64_t(1) << 30);
      cx->opt_win_slice = v;
    } else if (n == "seed_m") {
      range(0, 4096);
      cx->opt_seed_m = v;
    } else if (n == "query_table_budget") {
      range(0, int64_t(1) << 50);
      cx->opt_query_budget = v;
    } else if (n == "corpus_keep_bytes") {
      range(0, int64_t(1) << 50);
      cx->opt_corpus_keep = v;
    } else if (n == "raw_load_pct") {
      range(10, 90);
      cx->opt_raw_load_pct = v;
    } else if (n == "docid_terms") {
      range(0, 1);
      cx->opt_docid_terms = v;
    } else if (n == "sort_digit_bits") {
      if (v != 0) range(6, 11);
      cx->opt_sort_bits = v;
    } else if (n == "term_off_tables") {
      range(0, 1);
      cx->opt_term_off_tables = v;
    } else if (n == "docid_split") {
      range(0, 2);
      cx->opt_docid_split = v;
    } else if (n == "wild_scan") {
      range(0, 1);
      cx->opt_wild_scan = v;
    } else if (n == "wild_chunk") {
      range(64, 4096);
      if (v % 64) throw sme::Error(SME_EINVAL, "option " + n + " must be a multiple of 64");
      cx->opt_wild_chunk = v;
    } else if (n == "fuzzy_scan") {
      range(0, 1);
      cx->opt_fuzzy_scan = v;
    } else if (n == "bool_chunk") {
      range(64, 4096);
      if (v % 64) throw sme::Error(SME_EINVAL, "option " + n + " must be a multiple of 64");
      cx->opt_bool_chunk = v;
    } else if (n == "bool_driver") {
      range(0, 1);
      cx->opt_bool_driver = v;
    } else if (n == "positions") {
      range(0, 1);
      cx->opt_positions = v;
    } else if (n == "struct_narrow") {
      range(0, 1);
      cx->opt_struct_narrow = v;
    } else if (n == "fb_slots") {
      if (!sme::feedback::legal_slots(v))
        throw sme::Error(SME_EINVAL, "option " + n + " must be a power of two in [" +
                                         std::to_string(sme::feedback::kMinSlots) + ", " +
                                         std::to_string(sme::feedback::kMaxSlots) + "]");
      cx->opt_fb_slots = v;
    } else if (n == "merge_tile") {
      if (!sme::ixmerge::legal_tile(v))
        throw sme::Error(SME_EINVAL, "option " + n + " must be a multiple of 64 in [" +
                                         std::to_string(sme::ixmerge::kMinTile) + ", " +
                                         std::to_string(sme::ixmerge::kMaxTile) + "]");
      cx->opt_merge_tile = v;
    } else if (n == "delete_tile") {
      if (!sme::ixdelete::legal_tile(v))
        throw sme::Error(SME_EINVAL, "option " + n + " must be a multiple of 256 in [" +
                                         std::to_string(sme::ixdelete::kMinTile) + ", " +
                                         std::to_string(sme::ixdelete::kMaxTile) + "]");
      cx->opt_delete_tile = v;
    } else if (n == "merge_append") {
      range(0, 1);
      cx->opt_merge_append = v;
    } else if (n == "bm25_split") {
      range(0, int64_t(1) << 30);
      cx->opt_bm25_split = v;
    } else if (n == "rescore_path") {
      range(sme::rescore::PATH_AUTO, sme::rescore::PATH_SCAN);
      cx->opt_rescore_path = v;
    } else {
      throw sme::Error(SME_EINVAL, "unknown option " + n);
    }
  });
}

static void ctx_release(sme_ctx *cx) {
  (void)hipSetDevice(cx->device);
  (void)hipDeviceSynchronize();
  if (cx->own_stream) (void)hipStreamDestroy(cx->own_stream);
  if (cx->aux_stream) (void)hipStreamDestroy(cx->aux_stream);
  if (cx->ev_fork) (void)hipEventDestroy(cx->ev_fork);
  if (cx->ev_join) (void)hipEventDestroy(cx->ev_join);
  for (hipEvent_t e : cx->prof_events) (void)hipEventDestroy(e);
  for (auto &b : cx->h_stage)
    if (b) (void)hipHostFree(b);
  delete cx;
}

void sme_destroy(sme_ctx *cx) {
  if (!cx) return;
  cx->destroyed = true;
  if (cx->live_indexes == 0) ctx_release(cx);
}

int sme_load_docno_mapping(sme_ctx *cx, const uint8_t *m, size_t n) {
  return guard([&] {
    if (!cx || (!m && n)) throw sme::Error(SME_EINVAL, "null argument");
    set_device(cx);
    if (n < 4) throw sme::Error(SME_EINVAL, "mapping file shorter than its int32 count");
    int32_t cnt = (int32_t)(((uint32_t)m[0] << 24) | ((uint32_t)m[1] << 16) | ((uint32_t)m[2] << 8) | m[3]);
    if (cnt < 0) throw sme::Error(SME_EINVAL, "negative mapping count");
    std::vector<uint16_t> chars;
    std::vector<int64_t> off;
    off.push_back(0);
    off.push_back(0);  // "" sentinel at index 0 (readDocnoData)
    size_t p = 4;
    for (int32_t i = 0; i < cnt; i++) {
      if (p + 2 > n) throw sme::Error(SME_EINVAL, "truncated mapping file");
      size_t l = ((size_t)m[p] << 8) | m[p + 1];
      p += 2;
      if (p + l > n) throw sme::Error(SME_EINVAL, "truncated mapping file");
      if (!read_mutf8(m + p, l, chars)) throw sme::Error(SME_EINVAL, "bad modified UTF-8 in mapping file");
      p += l;
      off.push_back((int64_t)chars.size());
    }
    chars.push_back(0);
    hipStream_t st = cx->own_stream;
    uint16_t *dc = cx->map_chars.as<uint16_t>(chars.size());
    int64_t *doff = cx->map_off.as<int64_t>(off.size());
    SME_HIP(hipMemcpyAsync(dc, chars.data(), chars.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    SME_HIP(hipMemcpyAsync(doff, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    SME_HIP(hipStreamSynchronize(st));
    cx->map_n = (int64_t)off.size() - 1;
    cx->has_map = true;
    // The docid hash equals Arrays.binarySearch only when the entries {"", docids...}
    // are strictly ascending in String.compareTo (UTF-16 unit) order -- a sorted
    // file of distinct docids, as writeDocnoData produces.  Any other file (unsorted,
    // or with duplicates) keeps the device binary search, which then reproduces
    // binarySearch's result on that array exactly.
    bool distinct = true;
    for (size_t i = 1; i + 1 < off.size() && distinct; i++)
      distinct = std::lexicographical_compare(chars.begin() + off[i - 1], chars.begin() + off[i],
                                              chars.begin() + off[i], chars.begin() + off[i + 1]);
    sme::build_docid_hash(cx, distinct, st);
  });
}

int sme_number_documents(sme_ctx *cx, const uint8_t *corpus, size_t nbytes, const uint8_t **mapping, size_t *n) {
  return guard([&] {
    if (!cx || !mapping || !n || (!corpus && nbytes)) throw sme::Error(SME_EINVAL, "null argument");
    set_device(cx);
    hipStream_t st = cx->own_stream;
    sme::DevBuf buf;
    uint8_t *d = buf.as<uint8_t>(nbytes + 16);
    if (nbytes) SME_HIP(hipMemcpyAsync(d, corpus, nbytes, hipMemcpyHostToDevice, st));
    sme::number_documents(cx, d, nbytes, st, cx->mapping_out);
    *mapping = cx->mapping_out.data();
    *n = cx->mapping_out.size();
  });
}

int sme_split_points(sme_ctx *cx, const uint8_t *corpus, size_t nbytes, int world, uint64_t *cuts) {
  return guard([&] {
    if (!cx || !cuts || world < 1 || (!corpus && nbytes)) throw sme::Error(SME_EINVAL, "bad argument");
    set_device(cx);
    hipStream_t st = cx->own_stream;
    sme::DevBuf buf;
    uint8_t *d = buf.as<uint8_t>(nbytes + 16);
    if (nbytes) SME_HIP(hipMemcpyAsync(d, corpus, nbytes, hipMemcpyHostToDevice, st));
    sme::split_points(cx, d, nbytes, world, cuts, st);
  });
}

int sme_split_points_device(sme_ctx *cx, const void *d_corpus, size_t nbytes, int world, void *stream,
                            uint64_t *cuts) {
  return guard([&] {
    if (!cx || !cuts || world < 1 || (!d_corpus && nbytes)) throw sme::Error(SME_EINVAL, "bad argument");
    set_device(cx);
    sme::split_points(cx, (const uint8_t *)d_corpus, nbytes, world, cuts, stream_of(cx, stream));
  });
}

int sme_build_index_device(sme_ctx *cx, const void *d_corpus, size_t nbytes, void *stream, sme_index **out) {
  return guard([&] {
    if (!cx || !out || (!d_corpus && nbytes)) throw sme::Error(SME_EINVAL, "null argument");
    set_device(cx);
    hipStream_t st = stream_of(cx, stream);
    sme_index *ix = sme::build_index(cx, (const uint8_t *)d_corpus, nbytes, st);
    cx->last_profile = ix->profile;
    *out = ix;
  });
}

int sme_build_chargram_device(sme_ctx *cx, const void *d_corpus, size_t nbytes, void *stream, sme_index **out) {
  return guard([&] {
    if (!cx || !out || (!d_corpus && nbytes)) throw sme::Error(SME_EINVAL, "null argument");
    set_device(cx);
    hipStream_t st = stream_of(cx, stream);
    sme_index *ix = sme::build_index(cx, (const uint8_t *)d_corpus, nbytes, st, 1);
    cx->last_profile = ix->profile;
    *out = ix;
  });
}

int sme_build_chargram(sme_ctx *cx, const uint8_t *corpus, size_t nbytes, sme_index **out) {
  return guard([&] {
    if (!cx || !out || (!corpus && nbytes)) throw sme::Error(SME_EINVAL, "null argument");
    set_device(cx);
    hipStream_t st = cx->own_stream;
    sme::DevBuf buf;
    uint8_t *d = buf.as<uint8_t>(nbytes + 16);
    if (nbytes) SME_HIP(hipMemcpyAsync(d, corpus, nbytes, hipMemcpyHostToDevice, st));
    sme_index *ix = sme::build_index(cx, d, nbytes, st, 1);
    SME_HIP(hipStreamSynchronize(st));
    cx->last_profile = ix->profile;
    *out = ix;
  });
}

int sme_chargram_stats(const sme_index *ix, uint64_t *ngrams, uint64_t *npairs) {
  return guard([&] {
    if (!ix || !ngrams || !npairs) throw sme::Error(SME_EINVAL, "null argument");
    if (ix->job != 1) throw sme::Error(SME_EINVAL, "not a CharKGramTermIndexer output");
    *ngrams = (uint64_t)ix->cg_ngrams;
    *npairs = (uint64_t)ix->cg_pairs;
  });
}

int sme_chargram_partition_text(sme_index *ix, int part, const uint8_t **buf, size_t *n) {
  if (ix && ix->job != 1) return fail(SME_EINVAL, "not a CharKGramTermIndexer output");
  return sme_index_partition_records(ix, part, buf, n);
}

int sme_build_index(sme_ctx *cx, const uint8_t *corpus, size_t nbytes, sme_index **out) {
  return guard([&] {
    if (!cx || !out || (!corpus && nbytes)) throw sme::Error(SME_EINVAL, "null argument");
    set_device(cx);
    hipStream_t st = cx->own_stream;
    // the corpus's device copy is kept in the context (no hipMalloc per build);
    // a pinned host corpus is copied at DMA rate
    uint8_t *d = cx->h_corpus_dev.as<uint8_t>(nbytes + 16);
    if (nbytes) SME_HIP(hipMemcpyAsync(d, corpus, nbytes, hipMemcpyHostToDevice, st));
    sme_index *ix = sme::build_index(cx, d, nbytes, st);
    SME_HIP(hipStreamSynchronize(st));
    // a large copy is not held for the context's lifetime: it would also shrink
    // the HBM that sme_index_prepare_queries sizes its heavy rows from
    if ((int64_t)nbytes > cx->opt_corpus_keep) cx->h_corpus_dev.release();
    cx->last_profile = ix->profile;
    *out = ix;
  });
}

int sme_index_from_records_device(sme_ctx *cx, const void *d_records, const uint64_t *part_offsets, int nparts,
                                  void *stream, sme_index **out) {
  return guard([&] {
    if (!cx || !out || nparts < 0 || (nparts > 0 && !part_offsets)) throw sme::Error(SME_EINVAL, "bad argument");
    set_device(cx);
    hipStream_t st = stream_of(cx, stream);
    sme_index *ix = sme::load_records(cx, (const uint8_t *)d_records, part_offsets, nparts, st);
    cx->last_profile = ix->profile;
    *out = ix;
  });
}

int sme_index_from_records(sme_ctx *cx, const uint8_t *records, const uint64_t *part_offsets, int nparts,
                           sme_index **out) {
  return guard([&] {
    if (!cx || !out || nparts < 0 || (nparts > 0 && !part_offsets)) throw sme::Error(SME_EINVAL, "bad argument");
    const size_t nbytes = nparts > 0 ? (size_t)part_offsets[nparts] : 0;
    if (!records && nbytes) throw sme::Error(SME_EINVAL, "null argument");
    set_device(cx);
    hipStream_t st = cx->own_stream;
    // the stream's device copy lives for this call only (a pooled block)
    sme::DevBuf buf;
    buf.pool = &cx->pool;
    uint8_t *d = buf.as<uint8_t>(nbytes + 16);
    if (nbytes) SME_HIP(hipMemcpyAsync(d, records, nbytes, hipMemcpyHostToDevice, st));
    sme_index *ix = nullptr;
    try {
      ix = sme::load_records(cx, d, part_offsets, nparts, st);
    } catch (...) {
      (void)hipStreamSynchronize(st);  // kernels may still read the copy
      throw;
    }
    SME_HIP(hipStreamSynchronize(st));
    cx->last_profile = ix->profile;
    *out = ix;
  });
}

void sme_index_free(sme_index *ix) {
  if (!ix) return;
  sme_ctx *cx = ix->ctx;
  (void)hipSetDevice(cx->device);
  (void)hipDeviceSynchronize();
  delete ix;  // buffers go back to the context's pool
  if (cx->live_indexes == 0 && cx->destroyed) ctx_release(cx);
}

int sme_index_stats(const sme_index *ix, uint64_t *N, uint64_t *V, uint64_t *P) {
  return guard([&] {
    if (!ix) throw sme::Error(SME_EINVAL, "null index");
    if (N) *N = (uint64_t)ix->N;
    if (V) *V = (uint64_t)ix->V;
    if (P) *P = (uint64_t)ix->P;
  });
}

int sme_index_partition_records(sme_index *ix, int part, const uint8_t **buf, size_t *n) {
  return guard([&] {
    if (!ix || !buf || !n) throw sme::Error(SME_EINVAL, "null argument");
    if (part < 0 || part >= ix->R) throw sme::Error(SME_EINVAL, "partition out of range");
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::serialize_index(ix, st);
    const int64_t a = ix->part_start[part], b = ix->part_start[part + 1];
    if (!ix->h_parts_ready[part]) {
      // default-initialised (not zero-filled) host storage, filled straight from HBM
      ix->h_parts[part].reset(new uint8_t[(size_t)(b - a) + 1]);
      copy_d2h(ix->ctx, ix->h_parts[part].get(), (const uint8_t *)ix->d_ser.p + a, (size_t)(b - a), st);
      ix->h_parts_ready[part] = 1;
    }
    *buf = ix->h_parts[part].get();
    *n = (size_t)(b - a);
  });
}

int sme_index_serialize(sme_index *ix, uint64_t *part_offsets, float *device_ms) {
  return guard([&] {
    if (!ix) throw sme::Error(SME_EINVAL, "null index");
    set_device(ix->ctx);
    sme::serialize_index(ix, ix->ctx->own_stream);
    if (part_offsets)
      for (int p = 0; p <= ix->R; p++) part_offsets[p] = (uint64_t)ix->part_start[p];
    if (device_ms) *device_ms = ix->ser_ms;
  });
}

int sme_index_copy_records(sme_index *ix, int part, void *dst, size_t cap, size_t *n) {
  return guard([&] {
    if (!ix || !n || (!dst && cap)) throw sme::Error(SME_EINVAL, "null argument");
    if (part < -1 || part >= ix->R) throw sme::Error(SME_EINVAL, "partition out of range");
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::serialize_index(ix, st);
    const int64_t a = part < 0 ? 0 : ix->part_start[part], b = part < 0 ? ix->part_start[ix->R] : ix->part_start[part + 1];
    if ((size_t)(b - a) > cap) throw sme::Error(SME_EINVAL, "destination smaller than the records");
    copy_d2h(ix->ctx, dst, (const uint8_t *)ix->d_ser.p + a, (size_t)(b - a), st);
    *n = (size_t)(b - a);
  });
}

int sme_index_csr(sme_index *ix, const int64_t **offsets, const int32_t **docno, const int32_t **tf,
                  const int32_t **true_df) {
  return guard([&] {
    if (!ix) throw sme::Error(SME_EINVAL, "null index");
    set_device(ix->ctx);
    if (!ix->h_csr_ready) {
      ix->h_off.resize(ix->V + 1);
      ix->h_docno.resize(ix->P);
      ix->h_tf.resize(ix->P);
      ix->h_df.resize(ix->V);
      SME_HIP(hipMemcpy(ix->h_off.data(), ix->d_off.p, (ix->V + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
      if (ix->P) {
        SME_HIP(hipMemcpy(ix->h_docno.data(), ix->d_docno_o.p, ix->P * sizeof(int32_t), hipMemcpyDeviceToHost));
        SME_HIP(hipMemcpy(ix->h_tf.data(), ix->d_tf_o.p, ix->P * sizeof(int32_t), hipMemcpyDeviceToHost));
      }
      for (int64_t t = 0; t < ix->V; t++) ix->h_df[t] = (int32_t)(ix->h_off[t + 1] - ix->h_off[t]);
      ix->h_csr_ready = true;
    }
    if (offsets) *offsets = ix->h_off.data();
    if (docno) *docno = ix->h_docno.data();
    if (tf) *tf = ix->h_tf.data();
    if (true_df) *true_df = ix->h_df.data();
  });
}

int sme_index_device_arrays(sme_index *ix, const int64_t **d_offsets, const int32_t **d_docno,
                            const double **d_weight) {
  return guard([&] {
    if (!ix) throw sme::Error(SME_EINVAL, "null index");
    need_query_side(ix);
    if (d_offsets) *d_offsets = (const int64_t *)ix->d_off.p;
    if (d_docno) *d_docno = (const int32_t *)ix->d_docno_d.p;
    if (d_weight) *d_weight = (const double *)ix->d_w.p;
  });
}

int sme_index_term(sme_index *ix, int64_t t, const uint8_t **utf8, size_t *n) {
  return guard([&] {
    if (!ix || !utf8 || !n) throw sme::Error(SME_EINVAL, "null argument");
    if (t < 0 || t >= ix->V) throw sme::Error(SME_EINVAL, "term id out of range");
    set_device(ix->ctx);
    ensure_host_terms(ix);
    ix->h_term_tmp.clear();
    const bool joined = ix->K > 1 && ix->h_gram.empty();  // merged pieces: components joined by U+0000
    const int64_t c = (ix->K > 1 && !joined) ? (int64_t)ix->h_gram[(size_t)(t * ix->K)] : t;  // k_gram[0] of a k-gram
    const uint16_t *u = ix->h_term_chars.data() + ix->h_term_off[c];
    size_t len = (size_t)(ix->h_term_off[c + 1] - ix->h_term_off[c]);
    if (joined)
      for (size_t i = 0; i < len; i++)
        if (u[i] == 0) {
          len = i;
          break;
        }
    u16_to_mutf8(u, len, ix->h_term_tmp);
    *utf8 = ix->h_term_tmp.data();
    *n = ix->h_term_tmp.size();
  });
}

int sme_tokenize(sme_ctx *cx, const uint8_t *utf8, size_t n, uint8_t *buf, size_t cap, int64_t *offs, int cap_tok,
                 int *ntok) {
  return guard([&] {
    if (!cx || !buf || !offs || !ntok || (!utf8 && n)) throw sme::Error(SME_EINVAL, "null argument");
    set_device(cx);
    std::vector<std::vector<uint16_t>> toks;
    sme::tokenize_string(cx, utf8, n, toks, cx->own_stream);
    if ((int)toks.size() > cap_tok) throw sme::Error(SME_ELIMIT, "more tokens than cap_tok");
    std::vector<uint8_t> o;
    offs[0] = 0;
    for (size_t i = 0; i < toks.size(); i++) {
      u16_to_mutf8(toks[i].data(), toks[i].size(), o);
      offs[i + 1] = (int64_t)o.size();
    }
    if (o.size() > cap) throw sme::Error(SME_ELIMIT, "token buffer too small");
    if (!o.empty()) memcpy(buf, o.data(), o.size());
    *ntok = (int)toks.size();
  });
}

int sme_lookup_terms(sme_index *ix, const uint8_t *terms, const int64_t *offs, int n, int32_t *term_ids) {
  return guard([&] {
    if (!ix || !offs || !term_ids || n < 0) throw sme::Error(SME_EINVAL, "null argument");
    set_device(ix->ctx);
    std::vector<std::vector<uint16_t>> q(n);
    for (int i = 0; i < n; i++) q[i] = utf8_to_u16(terms + offs[i], (size_t)(offs[i + 1] - offs[i]));
    sme::lookup_terms(ix, q, term_ids, ix->ctx->own_stream);
  });
}

// ---- the batched query features ---------------------------------------------
// Each leaves a sme::ResultSet on the index (sme_result.hpp).  A _device entry
// hands out its device arrays, a host entry fetches them into its mirrors and
// hands those out; either way the arrays are the index's until the same feature's
// next call.
void sme::ResultSet::fetch(hipStream_t st) {
  const size_t tot = (size_t)total;
  h_off.resize((size_t)n + 1);
  for (Column &c : col) c.h.resize((tot + 1) * c.esize);  // (never an empty vector: data() stays a valid pointer)
  SME_HIP(hipMemcpyAsync(h_off.data(), off.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (tot)
    for (Column &c : col)
      if (c.esize) SME_HIP(hipMemcpyAsync(c.h.data(), c.d.p, tot * c.esize, hipMemcpyDeviceToHost, st));
  SME_HIP(hipStreamSynchronize(st));
}

// a batch of n UTF-8 strings: text may be NULL only while every string is empty
static bool bad_text_batch(const sme_index *ix, const uint8_t *text, const int64_t *offs, int n) {
  return !ix || n < 0 || (n > 0 && !offs) || (n > 0 && !text && offs[n] > offs[0]);
}

// wildcard expansion and spelling suggestions run over the vocabulary of a K = 1
// term index (`shards`: what the feature tells the holder of merged pieces to do)
static void need_vocabulary(const sme_index *ix, const std::string &what, const char *shards) {
  if (ix->job != 0) throw sme::Error(SME_EINVAL, what + ": a CharKGramTermIndexer output has no term vocabulary");
  if (ix->records_only)
    throw sme::Error(SME_EINVAL, what + ": records-only index (merged shard pieces): " + shards);
  if (ix->K != 1) throw sme::Error(SME_EINVAL, what + ": K = " + std::to_string(ix->K) + " index (K = 1 only)");
}

static void need_wildcard_index(const sme_index *ix) {
  need_vocabulary(ix, "wildcards", "expand on the shard indexes");
}

int sme_index_prepare_wildcards(sme_index *ix, void *stream, float *ms) {
  return guard([&] {
    if (!ix) throw sme::Error(SME_EINVAL, "null index");
    need_wildcard_index(ix);
    set_device(ix->ctx);
    sme::prepare_wildcards(ix, stream_of(ix->ctx, stream));
    if (ms) *ms = ix->wild_ms;
  });
}

int sme_index_wildcard_stats(sme_index *ix, uint64_t *ngrams, uint64_t *npairs) {
  return guard([&] {
    if (!ix || !ngrams || !npairs) throw sme::Error(SME_EINVAL, "null argument");
    need_wildcard_index(ix);
    set_device(ix->ctx);
    sme::prepare_wildcards(ix, ix->ctx->own_stream);
    *ngrams = (uint64_t)ix->wild_G;
    *npairs = (uint64_t)ix->wild_pairs;
  });
}

int sme_index_expand_wildcards_device(sme_index *ix, const uint8_t *patterns, const int64_t *offs, int n, void *stream,
                                      const int64_t **d_match_off, const int32_t **d_term_ids, int64_t *total) {
  return guard([&] {
    if (!d_match_off || !d_term_ids || bad_text_batch(ix, patterns, offs, n))
      throw sme::Error(SME_EINVAL, "bad argument");
    need_wildcard_index(ix);
    set_device(ix->ctx);
    sme::expand_wildcards(ix, patterns, offs, n, stream_of(ix->ctx, stream));
    const sme::TermIds &r = ix->wx;
    *d_match_off = r.dev_offsets();
    *d_term_ids = r.dev<sme::TermIds::ids>();
    if (total) *total = r.total;
  });
}

int sme_index_expand_wildcards(sme_index *ix, const uint8_t *patterns, const int64_t *offs, int n,
                               const int64_t **match_off, const int32_t **term_ids) {
  return guard([&] {
    if (!match_off || !term_ids || bad_text_batch(ix, patterns, offs, n)) throw sme::Error(SME_EINVAL, "bad argument");
    need_wildcard_index(ix);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::expand_wildcards(ix, patterns, offs, n, st);
    sme::TermIds &r = ix->wx;
    r.fetch(st);
    *match_off = r.h_off.data();
    *term_ids = r.host<sme::TermIds::ids>();
  });
}

static void need_suggest_args(const sme_index *ix, const uint8_t *words, const int64_t *offs, int n, int max_dist,
                              int m) {
  if (bad_text_batch(ix, words, offs, n)) throw sme::Error(SME_EINVAL, "bad argument");
  if (max_dist < 0 || max_dist > 3) throw sme::Error(SME_EINVAL, "suggestions: max_dist must be 0..3");
  if (m < 0) throw sme::Error(SME_EINVAL, "suggestions: m must be >= 0");
  need_vocabulary(ix, "suggestions", "ask the shard indexes");
}

int sme_index_suggest_terms_device(sme_index *ix, const uint8_t *words, const int64_t *offs, int n, int max_dist, int m,
                                   void *stream, const int64_t **d_sug_off, const int32_t **d_term_ids,
                                   const uint8_t **d_dist, int64_t *total) {
  return guard([&] {
    if (!d_sug_off || !d_term_ids || !d_dist) throw sme::Error(SME_EINVAL, "null argument");
    need_suggest_args(ix, words, offs, n, max_dist, m);
    set_device(ix->ctx);
    sme::suggest_terms(ix, words, offs, n, max_dist, m, stream_of(ix->ctx, stream));
    const sme::TermDists &r = ix->fz;
    *d_sug_off = r.dev_offsets();
    *d_term_ids = r.dev<sme::TermDists::ids>();
    *d_dist = r.dev<sme::TermDists::dist>();
    if (total) *total = r.total;
  });
}

int sme_index_suggest_terms(sme_index *ix, const uint8_t *words, const int64_t *offs, int n, int max_dist, int m,
                            const int64_t **sug_off, const int32_t **term_ids, const uint8_t **dist) {
  return guard([&] {
    if (!sug_off || !term_ids || !dist) throw sme::Error(SME_EINVAL, "null argument");
    need_suggest_args(ix, words, offs, n, max_dist, m);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::suggest_terms(ix, words, offs, n, max_dist, m, st);
    sme::TermDists &r = ix->fz;
    r.fetch(st);
    *sug_off = r.h_off.data();
    *term_ids = r.host<sme::TermDists::ids>();
    *dist = r.host<sme::TermDists::dist>();
  });
}

int sme_index_suggest_stats(const sme_index *ix, uint64_t *scanned_words, uint64_t *candidates) {
  return guard([&] {
    if (!ix || !scanned_words || !candidates) throw sme::Error(SME_EINVAL, "null argument");
    *scanned_words = ix->fz_scanned;
    *candidates = ix->fz.cands;
  });
}

// Boolean retrieval and structured queries run over the query side of a
// TermKGramDocIndexer index.  Which arrays a batch without entries may leave NULL
// is each feature's own rule, checked after this.
static void need_group_args(const sme_index *ix, const std::string &what, const int64_t *q_offsets, int nq, int order,
                            int m) {
  if (!ix || nq < 0 || (nq > 0 && !q_offsets)) throw sme::Error(SME_EINVAL, "bad argument");
  if (ix->job != 0) throw sme::Error(SME_EINVAL, what + ": not a TermKGramDocIndexer index");
  need_query_side(ix);
  if (m < 0) throw sme::Error(SME_EINVAL, what + ": m must be >= 0");
  if (order != 0 && order != 1) throw sme::Error(SME_EINVAL, what + ": order must be 0 (docno) or 1 (score)");
}

// the result of a Boolean or a structured call
static void device_arrays(const sme::DocScores &r, const int64_t **d_res_off, const int32_t **d_docno,
                          const double **d_score, int64_t *total) {
  *d_res_off = r.dev_offsets();
  *d_docno = r.dev<sme::DocScores::docno>();
  *d_score = r.dev<sme::DocScores::score>();
  if (total) *total = r.total;
}
static void host_arrays(sme::DocScores &r, hipStream_t st, const int64_t **res_off, const int32_t **docno,
                        const double **score) {
  r.fetch(st);
  *res_off = r.h_off.data();
  *docno = r.host<sme::DocScores::docno>();
  *score = r.host<sme::DocScores::score>();
}

static void need_boolean_args(const sme_index *ix, const int32_t *term_ids, const int64_t *g_offsets,
                              const uint8_t *g_flags, const int64_t *q_offsets, int nq, int order, int m) {
  need_group_args(ix, "boolean", q_offsets, nq, order, m);
  // g_offsets always holds an entry; only a batch without a group may leave
  // g_flags and term_ids NULL (sme::query_boolean validates the offsets
  // themselves before anything is read through them)
  if (nq > 0 && (!g_offsets || (q_offsets[nq] != 0 && (!g_flags || !term_ids))))
    throw sme::Error(SME_EINVAL, "bad argument");
}

int sme_query_boolean_device(sme_index *ix, const int32_t *term_ids, const int64_t *g_offsets, const uint8_t *g_flags,
                             const int64_t *q_offsets, int nq, int order, int m, void *stream,
                             const int64_t **d_res_off, const int32_t **d_docno, const double **d_score,
                             int64_t *total) {
  return guard([&] {
    if (!d_res_off || !d_docno || !d_score) throw sme::Error(SME_EINVAL, "null argument");
    need_boolean_args(ix, term_ids, g_offsets, g_flags, q_offsets, nq, order, m);
    set_device(ix->ctx);
    sme::query_boolean(ix, term_ids, g_offsets, g_flags, q_offsets, nq, order, m, stream_of(ix->ctx, stream));
    device_arrays(ix->bq, d_res_off, d_docno, d_score, total);
  });
}

int sme_query_boolean(sme_index *ix, const int32_t *term_ids, const int64_t *g_offsets, const uint8_t *g_flags,
                      const int64_t *q_offsets, int nq, int order, int m, const int64_t **res_off,
                      const int32_t **docno, const double **score) {
  return guard([&] {
    if (!res_off || !docno || !score) throw sme::Error(SME_EINVAL, "null argument");
    need_boolean_args(ix, term_ids, g_offsets, g_flags, q_offsets, nq, order, m);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::query_boolean(ix, term_ids, g_offsets, g_flags, q_offsets, nq, order, m, st);
    host_arrays(ix->bq, st, res_off, docno, score);
  });
}

int sme_query_boolean_stats(const sme_index *ix, uint64_t *candidates, uint64_t *matches) {
  return guard([&] {
    if (!ix || !candidates || !matches) throw sme::Error(SME_EINVAL, "null argument");
    *candidates = ix->bq.cands;
    *matches = ix->bq.matches;
  });
}

// Phrase and proximity queries run over the query side and the positions of a
// K = 1 index.  term_ids may be NULL only in a batch without a term (the feature
// validates the offsets themselves before anything is read through them).
static void need_positions_args(const sme_index *ix, const std::string &what, const int32_t *term_ids,
                                const int64_t *offsets, int n, int order, int m) {
  if (!ix || n < 0 || (n > 0 && !offsets)) throw sme::Error(SME_EINVAL, "bad argument");
  if (ix->job != 0) throw sme::Error(SME_EINVAL, what + ": not a TermKGramDocIndexer index");
  if (ix->records_only) throw sme::Error(SME_EINVAL, what + ": the index has no query side (merged shard pieces)");
  if (ix->K != 1) throw sme::Error(SME_EINVAL, what + ": the index holds k-grams (K != 1), not terms");
  if (!ix->has_positions)
    throw sme::Error(SME_EINVAL, what + ": the index keeps no positions (build it with option \"positions\" 1)");
  if (m < 0) throw sme::Error(SME_EINVAL, what + ": m must be >= 0");
  if (order != 0 && order != 1) throw sme::Error(SME_EINVAL, what + ": order must be 0 (docno) or 1 (score)");
  if (n > 0 && offsets[n] != 0 && !term_ids) throw sme::Error(SME_EINVAL, "bad argument");
}

// the result of a phrase or a proximity call
static void device_arrays(const sme::DocFreqScores &r, const int64_t **d_res_off, const int32_t **d_docno,
                          const int32_t **d_freq, const double **d_score, int64_t *total) {
  *d_res_off = r.dev_offsets();
  *d_docno = r.dev<sme::DocFreqScores::docno>();
  *d_freq = r.dev<sme::DocFreqScores::freq>();
  *d_score = r.dev<sme::DocFreqScores::score>();
  if (total) *total = r.total;
}
static void host_arrays(sme::DocFreqScores &r, hipStream_t st, const int64_t **res_off, const int32_t **docno,
                        const int32_t **freq, const double **score) {
  r.fetch(st);
  *res_off = r.h_off.data();
  *docno = r.host<sme::DocFreqScores::docno>();
  *freq = r.host<sme::DocFreqScores::freq>();
  *score = r.host<sme::DocFreqScores::score>();
}
static void pass_stats(const sme::DocFreqScores &r, uint64_t *candidates, uint64_t *verified, uint64_t *matches) {
  *candidates = r.cands;
  *verified = r.verified;
  *matches = r.matches;
}

int sme_query_phrase_device(sme_index *ix, const int32_t *term_ids, const int64_t *p_offsets, int np, int order, int m,
                            void *stream, const int64_t **d_res_off, const int32_t **d_docno, const int32_t **d_freq,
                            const double **d_score, int64_t *total) {
  return guard([&] {
    if (!d_res_off || !d_docno || !d_freq || !d_score) throw sme::Error(SME_EINVAL, "null argument");
    need_positions_args(ix, "phrase query", term_ids, p_offsets, np, order, m);
    set_device(ix->ctx);
    sme::query_phrase(ix, term_ids, p_offsets, np, order, m, stream_of(ix->ctx, stream));
    device_arrays(ix->pq, d_res_off, d_docno, d_freq, d_score, total);
  });
}

int sme_query_phrase(sme_index *ix, const int32_t *term_ids, const int64_t *p_offsets, int np, int order, int m,
                     const int64_t **res_off, const int32_t **docno, const int32_t **freq, const double **score) {
  return guard([&] {
    if (!res_off || !docno || !freq || !score) throw sme::Error(SME_EINVAL, "null argument");
    need_positions_args(ix, "phrase query", term_ids, p_offsets, np, order, m);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::query_phrase(ix, term_ids, p_offsets, np, order, m, st);
    host_arrays(ix->pq, st, res_off, docno, freq, score);
  });
}

int sme_query_phrase_stats(const sme_index *ix, uint64_t *candidates, uint64_t *verified, uint64_t *matches) {
  return guard([&] {
    if (!ix || !candidates || !verified || !matches) throw sme::Error(SME_EINVAL, "null argument");
    pass_stats(ix->pq, candidates, verified, matches);
  });
}

// (a proximity batch with queries also has a width and a kind for each)
static void need_near_args(const sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets,
                           const int32_t *widths, const uint8_t *kinds, int nq, int order, int m) {
  if (nq > 0 && (!widths || !kinds)) throw sme::Error(SME_EINVAL, "bad argument");
  need_positions_args(ix, "proximity query", term_ids, q_offsets, nq, order, m);
}

int sme_query_near_device(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *widths,
                          const uint8_t *kinds, int nq, int order, int m, void *stream, const int64_t **d_res_off,
                          const int32_t **d_docno, const int32_t **d_freq, const double **d_score, int64_t *total) {
  return guard([&] {
    if (!d_res_off || !d_docno || !d_freq || !d_score) throw sme::Error(SME_EINVAL, "null argument");
    need_near_args(ix, term_ids, q_offsets, widths, kinds, nq, order, m);
    set_device(ix->ctx);
    sme::query_near(ix, term_ids, q_offsets, widths, kinds, nq, order, m, stream_of(ix->ctx, stream));
    device_arrays(ix->nq, d_res_off, d_docno, d_freq, d_score, total);
  });
}

int sme_query_near(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *widths,
                   const uint8_t *kinds, int nq, int order, int m, const int64_t **res_off, const int32_t **docno,
                   const int32_t **freq, const double **score) {
  return guard([&] {
    if (!res_off || !docno || !freq || !score) throw sme::Error(SME_EINVAL, "null argument");
    need_near_args(ix, term_ids, q_offsets, widths, kinds, nq, order, m);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::query_near(ix, term_ids, q_offsets, widths, kinds, nq, order, m, st);
    host_arrays(ix->nq, st, res_off, docno, freq, score);
  });
}

int sme_query_near_stats(const sme_index *ix, uint64_t *candidates, uint64_t *verified, uint64_t *matches) {
  return guard([&] {
    if (!ix || !candidates || !verified || !matches) throw sme::Error(SME_EINVAL, "null argument");
    pass_stats(ix->nq, candidates, verified, matches);
  });
}

// Relevance feedback reads the positions of a K = 1 index as phrase queries do, and
// the query side's document frequencies and idfs.  docnos may be NULL only in a
// batch without an entry (sme::feedback_terms validates the offsets themselves
// before anything is read through them).
static void need_feedback_args(const sme_index *ix, const int32_t *docnos, const int64_t *f_offsets, int nq, int m,
                               int min_docs, int min_df, int max_df) {
  need_positions_args(ix, "feedback terms", nullptr, nullptr, 0, 0, 0);
  if (nq < 0 || (nq > 0 && !f_offsets)) throw sme::Error(SME_EINVAL, "bad argument");
  if (m < 0) throw sme::Error(SME_EINVAL, "feedback terms: m must be >= 0");
  if (min_docs < 0) throw sme::Error(SME_EINVAL, "feedback terms: min_docs must be >= 0");
  if (min_df < 0) throw sme::Error(SME_EINVAL, "feedback terms: min_df must be >= 0");
  if (max_df < 0) throw sme::Error(SME_EINVAL, "feedback terms: max_df must be >= 0 (0: no upper bound)");
  if (nq > 0 && f_offsets[nq] > 0 && !docnos) throw sme::Error(SME_EINVAL, "bad argument");
}

int sme_index_feedback_terms_device(sme_index *ix, const int32_t *d_docnos, const int64_t *f_offsets, int nq,
                                    const int32_t *x_ids, const int64_t *x_offsets, int m, int min_docs, int min_df,
                                    int max_df, void *stream, const int64_t **d_res_off, const int32_t **d_term,
                                    const int32_t **d_freq, const int32_t **d_docs, const double **d_score,
                                    int64_t *total) {
  return guard([&] {
    if (!d_res_off || !d_term || !d_freq || !d_docs || !d_score) throw sme::Error(SME_EINVAL, "null argument");
    need_feedback_args(ix, d_docnos, f_offsets, nq, m, min_docs, min_df, max_df);
    set_device(ix->ctx);
    sme::feedback_terms(ix, d_docnos, true, f_offsets, nq, x_ids, x_offsets, m, min_docs, min_df, max_df,
                        stream_of(ix->ctx, stream));
    const sme::TermFreqDocsScores &r = ix->fb;
    *d_res_off = r.dev_offsets();
    *d_term = r.dev<sme::TermFreqDocsScores::term>();
    *d_freq = r.dev<sme::TermFreqDocsScores::freq>();
    *d_docs = r.dev<sme::TermFreqDocsScores::docs>();
    *d_score = r.dev<sme::TermFreqDocsScores::score>();
    if (total) *total = r.total;
  });
}

int sme_index_feedback_terms(sme_index *ix, const int32_t *docnos, const int64_t *f_offsets, int nq,
                             const int32_t *x_ids, const int64_t *x_offsets, int m, int min_docs, int min_df,
                             int max_df, const int64_t **res_off, const int32_t **term, const int32_t **freq,
                             const int32_t **docs, const double **score) {
  return guard([&] {
    if (!res_off || !term || !freq || !docs || !score) throw sme::Error(SME_EINVAL, "null argument");
    need_feedback_args(ix, docnos, f_offsets, nq, m, min_docs, min_df, max_df);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::feedback_terms(ix, docnos, false, f_offsets, nq, x_ids, x_offsets, m, min_docs, min_df, max_df, st);
    sme::TermFreqDocsScores &r = ix->fb;
    r.fetch(st);
    *res_off = r.h_off.data();
    *term = r.host<sme::TermFreqDocsScores::term>();
    *freq = r.host<sme::TermFreqDocsScores::freq>();
    *docs = r.host<sme::TermFreqDocsScores::docs>();
    *score = r.host<sme::TermFreqDocsScores::score>();
  });
}

int sme_index_feedback_stats(const sme_index *ix, uint64_t *positions, uint64_t *pairs, uint64_t *kept,
                             uint64_t *missing, uint64_t *spilled) {
  return guard([&] {
    if (!ix || !positions || !pairs || !kept || !missing || !spilled) throw sme::Error(SME_EINVAL, "null argument");
    *positions = ix->fb_positions;
    *pairs = ix->fb_pairs;
    *kept = ix->fb_kept;
    *missing = ix->fb_missing;
    *spilled = ix->fb_spilled;
  });
}

// A structured batch with an operator leaf also needs what proximity queries need
// (sme::query_structured says so once it has validated the batch and knows its leaves)
static void need_structured_args(const sme_index *ix, const int32_t *term_ids, const int64_t *l_offsets,
                                 const uint8_t *l_kinds, const int32_t *l_widths, const int64_t *g_offsets,
                                 const uint8_t *g_flags, const int64_t *q_offsets, int nq, int order, int m) {
  need_group_args(ix, "structured query", q_offsets, nq, order, m);
  // g_offsets and l_offsets always hold an entry; only a batch without a group may
  // leave the other arrays NULL (sme::query_structured validates the offsets
  // themselves before anything is read through them)
  if (nq > 0 && (!g_offsets || !l_offsets ||
                 (q_offsets[nq] != 0 && (!g_flags || !term_ids || !l_kinds || !l_widths))))
    throw sme::Error(SME_EINVAL, "bad argument");
}

int sme_query_structured_device(sme_index *ix, const int32_t *term_ids, const int64_t *l_offsets,
                                const uint8_t *l_kinds, const int32_t *l_widths, const int64_t *g_offsets,
                                const uint8_t *g_flags, const int64_t *q_offsets, int nq, int order, int m,
                                void *stream, const int64_t **d_res_off, const int32_t **d_docno,
                                const double **d_score, int64_t *total) {
  return guard([&] {
    if (!d_res_off || !d_docno || !d_score) throw sme::Error(SME_EINVAL, "null argument");
    need_structured_args(ix, term_ids, l_offsets, l_kinds, l_widths, g_offsets, g_flags, q_offsets, nq, order, m);
    set_device(ix->ctx);
    sme::query_structured(ix, term_ids, l_offsets, l_kinds, l_widths, g_offsets, g_flags, q_offsets, nq, order, m,
                          stream_of(ix->ctx, stream));
    device_arrays(ix->sq, d_res_off, d_docno, d_score, total);
  });
}

int sme_query_structured(sme_index *ix, const int32_t *term_ids, const int64_t *l_offsets, const uint8_t *l_kinds,
                         const int32_t *l_widths, const int64_t *g_offsets, const uint8_t *g_flags,
                         const int64_t *q_offsets, int nq, int order, int m, const int64_t **res_off,
                         const int32_t **docno, const double **score) {
  return guard([&] {
    if (!res_off || !docno || !score) throw sme::Error(SME_EINVAL, "null argument");
    need_structured_args(ix, term_ids, l_offsets, l_kinds, l_widths, g_offsets, g_flags, q_offsets, nq, order, m);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::query_structured(ix, term_ids, l_offsets, l_kinds, l_widths, g_offsets, g_flags, q_offsets, nq, order, m, st);
    host_arrays(ix->sq, st, res_off, docno, score);
  });
}

int sme_query_structured_stats(const sme_index *ix, uint64_t *leaves, uint64_t *verified, uint64_t *candidates,
                               uint64_t *matches) {
  return guard([&] {
    if (!ix || !leaves || !verified || !candidates || !matches) throw sme::Error(SME_EINVAL, "null argument");
    *leaves = ix->sq_leaves;
    *verified = ix->sq.verified;
    *candidates = ix->sq.cands;
    *matches = ix->sq.matches;
  });
}

int sme_index_positions(const sme_index *ix, uint64_t *records, uint64_t *positions, uint64_t *bytes) {
  return guard([&] {
    if (!ix || !records || !positions || !bytes) throw sme::Error(SME_EINVAL, "null argument");
    *records = *positions = *bytes = 0;
    if (!ix->has_positions) return;
    *records = (uint64_t)ix->ps_records;
    *positions = (uint64_t)ix->ps_terms;
    *bytes = (uint64_t)(ix->ps_records + 1) * sizeof(int64_t) + (uint64_t)ix->ps_terms * sizeof(int32_t) +
             (uint64_t)ix->ps_records * sizeof(int32_t);
  });
}

int sme_index_prepare_queries(sme_index *ix, void *stream, float *ms) {
  return guard([&] {
    if (!ix) throw sme::Error(SME_EINVAL, "null index");
    need_query_side(ix);
    if (ix->job != 0) throw sme::Error(SME_EINVAL, "not a TermKGramDocIndexer index");
    set_device(ix->ctx);
    sme::prepare_queries(ix, stream_of(ix->ctx, stream));
    if (ms) *ms = ix->q_prep_ms;
  });
}

int sme_query_topk_device(sme_index *ix, const int32_t *d_term_ids, const int64_t *d_q_offsets, int nq, int k,
                          int32_t *d_out_docno, double *d_out_score, void *stream) {
  return guard([&] {
    if (!ix || (nq > 0 && (!d_term_ids || !d_q_offsets || !d_out_docno || !d_out_score)))
      throw sme::Error(SME_EINVAL, "null argument");
    need_query_side(ix);
    set_device(ix->ctx);
    sme::query_topk(ix, d_term_ids, d_q_offsets, nq, k, d_out_docno, d_out_score, nullptr,
                    stream_of(ix->ctx, stream));
  });
}

int sme_query_topk_device_tie(sme_index *ix, const int32_t *d_term_ids, const int64_t *d_q_offsets, int nq, int k,
                              int32_t *d_out_docno, double *d_out_score, uint32_t *d_out_tie, void *stream) {
  return guard([&] {
    if (!ix || (nq > 0 && (!d_term_ids || !d_q_offsets || !d_out_docno || !d_out_score || !d_out_tie)))
      throw sme::Error(SME_EINVAL, "null argument");
    need_query_side(ix);
    set_device(ix->ctx);
    sme::query_topk(ix, d_term_ids, d_q_offsets, nq, k, d_out_docno, d_out_score, d_out_tie,
                    stream_of(ix->ctx, stream));
  });
}

static int query_topk_host(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, int nq, int k,
                           int32_t *out_docno, double *out_score, uint32_t *out_tie) {
  return guard([&] {
    if (!ix || (nq > 0 && (!term_ids || !q_offsets || !out_docno || !out_score)))
      throw sme::Error(SME_EINVAL, "null argument");
    need_query_side(ix);
    if (nq <= 0) return;
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    const int64_t nt = q_offsets[nq];
    for (int q = 0; q < nq; q++)
      if (q_offsets[q + 1] < q_offsets[q] || q_offsets[q] < 0) throw sme::Error(SME_EINVAL, "q_offsets not ascending");
    for (int64_t i = 0; i < nt; i++)
      if (term_ids[i] < -1 || term_ids[i] >= ix->V)
        throw sme::Error(SME_EINVAL, "term id " + std::to_string(term_ids[i]) + " outside [-1, V)");
    sme::DevBuf a, b, c, d, e;
    int32_t *dt = a.as<int32_t>(nt + 1);
    int64_t *dq = b.as<int64_t>(nq + 1);
    int32_t *dd = c.as<int32_t>((size_t)nq * k);
    double *ds = d.as<double>((size_t)nq * k);
    uint32_t *dtie = out_tie ? e.as<uint32_t>((size_t)nq * k) : nullptr;
    if (nt) SME_HIP(hipMemcpyAsync(dt, term_ids, nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SME_HIP(hipMemcpyAsync(dq, q_offsets, (nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    sme::query_topk(ix, dt, dq, nq, k, dd, ds, dtie, st);
    SME_HIP(hipMemcpyAsync(out_docno, dd, (size_t)nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipMemcpyAsync(out_score, ds, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_tie)
      SME_HIP(hipMemcpyAsync(out_tie, dtie, (size_t)nq * k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
  });
}

int sme_query_topk(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, int nq, int k,
                   int32_t *out_docno, double *out_score) {
  return query_topk_host(ix, term_ids, q_offsets, nq, k, out_docno, out_score, nullptr);
}

int sme_query_topk_tie(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, int nq, int k,
                       int32_t *out_docno, double *out_score, uint32_t *out_tie) {
  if (nq > 0 && !out_tie) return fail(SME_EINVAL, "null argument");
  return query_topk_host(ix, term_ids, q_offsets, nq, k, out_docno, out_score, out_tie);
}

// BM25 ranking runs over the query side of a TermKGramDocIndexer index
static void need_bm25_index(const sme_index *ix) {
  if (!ix) throw sme::Error(SME_EINVAL, "null index");
  if (ix->job != 0) throw sme::Error(SME_EINVAL, "bm25: a CharKGramTermIndexer output has no postings by document");
  if (ix->records_only)
    throw sme::Error(SME_EINVAL, "bm25: records-only index (merged shard pieces): query the shard indexes");
}

int sme_index_prepare_bm25(sme_index *ix, void *stream, float *ms) {
  return guard([&] {
    need_bm25_index(ix);
    set_device(ix->ctx);
    sme::prepare_bm25(ix, stream_of(ix->ctx, stream));
    if (ms) *ms = ix->bm_ms;
  });
}

int sme_index_doc_lengths(sme_index *ix, void *stream, const int32_t **d_len, int64_t *dmin, int64_t *span) {
  return guard([&] {
    need_bm25_index(ix);
    if (!d_len || !dmin || !span) throw sme::Error(SME_EINVAL, "null argument");
    set_device(ix->ctx);
    sme::prepare_bm25(ix, stream_of(ix->ctx, stream));
    *d_len = (const int32_t *)ix->d_bm_dl.p;
    *dmin = ix->dmin;
    *span = ix->bm_span;
  });
}

int sme_index_bm25_stats(const sme_index *ix, uint64_t *docs, uint64_t *total_len, uint64_t *max_len, uint64_t *window) {
  return guard([&] {
    need_bm25_index(ix);
    if (!docs || !total_len || !max_len || !window) throw sme::Error(SME_EINVAL, "null argument");
    set_device(ix->ctx);
    sme::prepare_bm25(const_cast<sme_index *>(ix), ix->ctx->own_stream);  // (the tables are a cache of the postings)
    *docs = ix->bm_docs;
    *total_len = ix->bm_total_len;
    *max_len = ix->bm_max_len;
    *window = (uint64_t)sme::bm25::kWindow;
  });
}

// the checks of a BM25 call that need no device; offs: the offsets on the host
static void need_bm25_args(const sme_index *ix, const int32_t *ids, const int64_t *offs, int nq, int k, double k1,
                           double b) {
  if (nq < 0) throw sme::Error(SME_EINVAL, "bm25: nq must be >= 0");
  if (k < 1) throw sme::Error(SME_EINVAL, "bm25: k must be >= 1");
  if (!sme::bm25::legal_params(k1, b))
    throw sme::Error(SME_EINVAL, "bm25: k1 must be finite and >= 0, b in [0, 1]");
  if (k > sme::bm25::kMaxK) throw sme::Error(SME_ELIMIT, "bm25: k > " + std::to_string(sme::bm25::kMaxK));
  int bad = -1;
  const int rc = sme::bm25::validate(ids, -1, offs, nq, ix->V, &bad);
  const std::string at = bad >= 0 ? " (query " + std::to_string(bad) + ")" : "";
  if (rc == sme::bm25::M_OFFSETS) throw sme::Error(SME_EINVAL, "bm25: q_offsets do not ascend from 0" + at);
  if (rc == sme::bm25::M_SLOTS)
    throw sme::Error(SME_ELIMIT, "bm25: more than " + std::to_string(sme::bm25::kMaxSlots) + " term slots" + at);
  if (rc == sme::bm25::M_TERM) throw sme::Error(SME_EINVAL, "bm25: a term id outside [-1, V)" + at);
}

int sme_query_topk_bm25_device(sme_index *ix, const int32_t *d_term_ids, const int64_t *d_q_offsets, int nq, int k,
                               double k1, double b, int32_t *d_out_docno, double *d_out_score, void *stream) {
  return guard([&] {
    need_bm25_index(ix);
    if (nq > 0 && (!d_term_ids || !d_q_offsets || !d_out_docno || !d_out_score))
      throw sme::Error(SME_EINVAL, "null argument");
    set_device(ix->ctx);
    hipStream_t st = stream_of(ix->ctx, stream);
    // the offsets come to the host: the slot limit is checked before a launch, the ids
    // by the scorer (an id outside [0, V) is skipped like -1)
    std::vector<int64_t> offs((size_t)std::max(nq, 0) + 1, 0);
    if (nq > 0) {
      SME_HIP(hipMemcpyAsync(offs.data(), d_q_offsets, offs.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
    }
    need_bm25_args(ix, nullptr, offs.data(), nq, k, k1, b);
    sme::query_topk_bm25(ix, d_term_ids, d_q_offsets, offs.data(), nq, k, k1, b, d_out_docno, d_out_score, st);
  });
}

int sme_query_topk_bm25(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, int nq, int k, double k1,
                        double b, int32_t *out_docno, double *out_score) {
  return guard([&] {
    need_bm25_index(ix);
    if (nq > 0 && (!term_ids || !q_offsets || !out_docno || !out_score)) throw sme::Error(SME_EINVAL, "null argument");
    need_bm25_args(ix, term_ids, q_offsets, nq, k, k1, b);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    const int64_t nt = nq > 0 ? q_offsets[nq] : 0;
    sme::DevBuf a, c, d, e;
    int32_t *dt = a.as<int32_t>((size_t)nt + 1);
    int64_t *dq = c.as<int64_t>((size_t)nq + 1);
    int32_t *dd = d.as<int32_t>((size_t)nq * k);
    double *ds = e.as<double>((size_t)nq * k);
    if (nt) SME_HIP(hipMemcpyAsync(dt, term_ids, (size_t)nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (nq > 0) SME_HIP(hipMemcpyAsync(dq, q_offsets, ((size_t)nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    sme::query_topk_bm25(ix, dt, dq, q_offsets, nq, k, k1, b, dd, ds, st);
    if (nq > 0) {
      SME_HIP(hipMemcpyAsync(out_docno, dd, (size_t)nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipMemcpyAsync(out_score, ds, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    SME_HIP(hipStreamSynchronize(st));
  });
}

int sme_query_bm25_stats(const sme_index *ix, uint64_t *windows, uint64_t *skipped, uint64_t *postings) {
  return guard([&] {
    if (!ix || !windows || !skipped || !postings) throw sme::Error(SME_EINVAL, "null argument");
    unsigned long long h[3] = {0, 0, 0};
    if (ix->bm_called) {
      set_device(ix->ctx);
      SME_HIP(hipMemcpyAsync(h, ix->d_bm_stat.p, sizeof h, hipMemcpyDeviceToHost, ix->bm_stream));
      SME_HIP(hipStreamSynchronize(ix->bm_stream));
    }
    *windows = h[0];
    *skipped = h[1];
    *postings = h[2];
  });
}

// Scoring given documents runs over the query side of a TermKGramDocIndexer index.
// The checks of a call that need no device; the batch itself is validated by
// sme::rescore_docs.  term_ids / docnos may be NULL only in a batch without a slot /
// a candidate (offs: the host copies of the offsets).
static void need_rescore_index(const sme_index *ix) {
  if (!ix) throw sme::Error(SME_EINVAL, "null index");
  if (ix->job != 0) throw sme::Error(SME_EINVAL, "rescore: a CharKGramTermIndexer output has no postings by document");
  if (ix->records_only)
    throw sme::Error(SME_EINVAL, "rescore: records-only index (merged shard pieces): query the shard indexes");
}
static void need_rescore_args(const sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets,
                              const int32_t *docnos, const int64_t *d_offsets, int nq, int model, double k1, double b,
                              int min_hits, int order, int m) {
  need_rescore_index(ix);
  if (nq < 0) throw sme::Error(SME_EINVAL, "rescore: nq must be >= 0");
  if (nq > 0 && (!q_offsets || !d_offsets)) throw sme::Error(SME_EINVAL, "null argument");
  if (!sme::rescore::legal_model(model)) throw sme::Error(SME_EINVAL, "rescore: model must be 0 (TF-IDF) or 1 (BM25)");
  if (order != 0 && order != 1) throw sme::Error(SME_EINVAL, "rescore: order must be 0 (as given) or 1 (score)");
  if (m < 0) throw sme::Error(SME_EINVAL, "rescore: m must be >= 0");
  if (min_hits < 0) throw sme::Error(SME_EINVAL, "rescore: min_hits must be >= 0");
  if (model == sme::rescore::MODEL_BM25 && !sme::bm25::legal_params(k1, b))
    throw sme::Error(SME_EINVAL, "rescore: k1 must be finite and >= 0, b in [0, 1]");
  // (offsets that do not start at 0 are refused by the validator before these arrays are read)
  if (nq > 0 && q_offsets[0] == 0 && q_offsets[nq] > 0 && !term_ids) throw sme::Error(SME_EINVAL, "null argument");
  if (nq > 0 && d_offsets[0] == 0 && d_offsets[nq] > 0 && !docnos) throw sme::Error(SME_EINVAL, "null argument");
}

int sme_query_rescore_device(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *d_docnos,
                             const int64_t *d_doc_offsets, int nq, int model, double k1, double b, int min_hits,
                             int order, int m, void *stream, const int64_t **d_res_off, const int32_t **d_docno,
                             const int32_t **d_hits, const double **d_score, int64_t *total) {
  return guard([&] {
    if (!d_res_off || !d_docno || !d_hits || !d_score) throw sme::Error(SME_EINVAL, "null argument");
    need_rescore_index(ix);  // (before anything is copied for it)
    if (nq > 0 && !d_doc_offsets) throw sme::Error(SME_EINVAL, "null argument");
    set_device(ix->ctx);
    hipStream_t st = stream_of(ix->ctx, stream);
    // the candidates' offsets come to the host, where they are validated
    std::vector<int64_t> offs((size_t)std::max(nq, 0) + 1, 0);
    if (nq > 0) {
      SME_HIP(hipMemcpyAsync(offs.data(), d_doc_offsets, offs.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
    }
    // (a device array of candidates is not read here: any non-null value stands for it)
    need_rescore_args(ix, term_ids, q_offsets, d_docnos, offs.data(), nq, model, k1, b, min_hits, order, m);
    sme::rescore_docs(ix, term_ids, q_offsets, d_docnos, true, offs.data(), d_doc_offsets, nq, model, k1, b, min_hits,
                      order, m, st);
    device_arrays(ix->rs, d_res_off, d_docno, d_hits, d_score, total);
  });
}

int sme_query_rescore(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *docnos,
                      const int64_t *d_offsets, int nq, int model, double k1, double b, int min_hits, int order, int m,
                      const int64_t **res_off, const int32_t **docno, const int32_t **hits, const double **score) {
  return guard([&] {
    if (!res_off || !docno || !hits || !score) throw sme::Error(SME_EINVAL, "null argument");
    need_rescore_args(ix, term_ids, q_offsets, docnos, d_offsets, nq, model, k1, b, min_hits, order, m);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::rescore_docs(ix, term_ids, q_offsets, docnos, false, d_offsets, nullptr, nq, model, k1, b, min_hits, order, m,
                      st);
    host_arrays(ix->rs, st, res_off, docno, hits, score);
  });
}

int sme_query_rescore_stats(const sme_index *ix, uint64_t *candidates, uint64_t *found, uint64_t *matches,
                            uint64_t *tile) {
  return guard([&] {
    if (!ix || !candidates || !found || !matches || !tile) throw sme::Error(SME_EINVAL, "null argument");
    pass_stats(ix->rs, candidates, found, matches);
    *tile = (uint64_t)sme::rescore::kTile;
  });
}

// Best passages read the term streams of a K = 1 index and the idfs of its query
// side.  A call empties both of its results first, so whatever refuses it -- here or
// in sme::query_passages, which validates the batch -- leaves them empty.
static void need_passages_index(sme_index *ix) {
  if (!ix) throw sme::Error(SME_EINVAL, "null index");
  ix->pw.reset();
  ix->pwt.reset();
  ix->pw_with_record = ix->pw_positions = 0;
  if (ix->job != 0) throw sme::Error(SME_EINVAL, "passages: a CharKGramTermIndexer output has no term streams");
  if (ix->records_only)
    throw sme::Error(SME_EINVAL, "passages: records-only index (merged shard pieces) has no query side");
  if (ix->K != 1) throw sme::Error(SME_EINVAL, "passages: the index holds k-grams (K != 1), not terms");
  if (!ix->has_positions)
    throw sme::Error(SME_EINVAL, "passages: the index keeps no positions (build it with option \"positions\" 1)");
}
static void need_passages_args(const int32_t *term_ids, const int64_t *q_offsets, const int32_t *docnos,
                               const int64_t *d_offsets, int nq, int min_cover, int order, int m, int with_terms) {
  if (nq < 0) throw sme::Error(SME_EINVAL, "passages: nq must be >= 0");
  if (nq > 0 && (!q_offsets || !d_offsets)) throw sme::Error(SME_EINVAL, "null argument");
  if (order != 0 && order != 1) throw sme::Error(SME_EINVAL, "passages: order must be 0 (as given) or 1 (score)");
  if (with_terms != 0 && with_terms != 1) throw sme::Error(SME_EINVAL, "passages: with_terms must be 0 or 1");
  if (m < 0) throw sme::Error(SME_EINVAL, "passages: m must be >= 0");
  if (min_cover < 0) throw sme::Error(SME_EINVAL, "passages: min_cover must be >= 0");
  // (offsets that do not start at 0 are refused by the validator before these arrays are read)
  if (nq > 0 && q_offsets[0] == 0 && q_offsets[nq] > 0 && !term_ids) throw sme::Error(SME_EINVAL, "null argument");
  if (nq > 0 && d_offsets[0] == 0 && d_offsets[nq] > 0 && !docnos) throw sme::Error(SME_EINVAL, "null argument");
}
static void passages_device_arrays(const sme_index *ix, sme_passages *out) {
  const sme::PassageRows &r = ix->pw;
  const sme::WindowTerms &w = ix->pwt;
  *out = sme_passages{r.dev_offsets(),
                      r.dev<sme::PassageRows::docno>(),
                      r.dev<sme::PassageRows::rec>(),
                      r.dev<sme::PassageRows::start>(),
                      r.dev<sme::PassageRows::len>(),
                      r.dev<sme::PassageRows::hits>(),
                      r.dev<sme::PassageRows::mask>(),
                      r.dev<sme::PassageRows::score>(),
                      r.total,
                      w.dev_offsets(),
                      w.dev<sme::WindowTerms::term>(),
                      w.dev<sme::WindowTerms::slot>(),
                      w.total};
}

int sme_query_passages_device(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets,
                              const int32_t *d_docnos, const int64_t *d_doc_offsets, int nq, int width, int min_cover,
                              int order, int m, int with_terms, void *stream, sme_passages *out) {
  return guard([&] {
    if (!out) throw sme::Error(SME_EINVAL, "null argument");
    need_passages_index(ix);  // (before anything is copied for it)
    if (nq > 0 && !d_doc_offsets) throw sme::Error(SME_EINVAL, "null argument");
    set_device(ix->ctx);
    hipStream_t st = stream_of(ix->ctx, stream);
    // the candidates' offsets come to the host, where they are validated
    std::vector<int64_t> offs((size_t)std::max(nq, 0) + 1, 0);
    if (nq > 0) {
      SME_HIP(hipMemcpyAsync(offs.data(), d_doc_offsets, offs.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
      SME_HIP(hipStreamSynchronize(st));
    }
    // (a device array of candidates is not read here: any non-null value stands for it)
    need_passages_args(term_ids, q_offsets, d_docnos, offs.data(), nq, min_cover, order, m, with_terms);
    sme::query_passages(ix, term_ids, q_offsets, d_docnos, true, offs.data(), d_doc_offsets, nq, width, min_cover, order,
                        m, with_terms, st);
    passages_device_arrays(ix, out);
  });
}

int sme_query_passages(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *docnos,
                       const int64_t *d_offsets, int nq, int width, int min_cover, int order, int m, int with_terms,
                       sme_passages *out) {
  return guard([&] {
    if (!out) throw sme::Error(SME_EINVAL, "null argument");
    need_passages_index(ix);
    need_passages_args(term_ids, q_offsets, docnos, d_offsets, nq, min_cover, order, m, with_terms);
    set_device(ix->ctx);
    hipStream_t st = ix->ctx->own_stream;
    sme::query_passages(ix, term_ids, q_offsets, docnos, false, d_offsets, nullptr, nq, width, min_cover, order, m,
                        with_terms, st);
    sme::PassageRows &r = ix->pw;
    sme::WindowTerms &w = ix->pwt;
    r.fetch(st);
    w.fetch(st);
    *out = sme_passages{r.h_off.data(),
                        r.host<sme::PassageRows::docno>(),
                        r.host<sme::PassageRows::rec>(),
                        r.host<sme::PassageRows::start>(),
                        r.host<sme::PassageRows::len>(),
                        r.host<sme::PassageRows::hits>(),
                        r.host<sme::PassageRows::mask>(),
                        r.host<sme::PassageRows::score>(),
                        r.total,
                        w.h_off.data(),
                        w.host<sme::WindowTerms::term>(),
                        w.host<sme::WindowTerms::slot>(),
                        w.total};
  });
}

int sme_query_passages_stats(const sme_index *ix, uint64_t *candidates, uint64_t *with_record, uint64_t *positions,
                             uint64_t *kept, uint64_t *chunk) {
  return guard([&] {
    if (!ix || !candidates || !with_record || !positions || !kept || !chunk)
      throw sme::Error(SME_EINVAL, "null argument");
    *candidates = ix->pw.cands;
    *with_record = ix->pw_with_record;
    *positions = ix->pw_positions;
    *kept = ix->pw.matches;
    *chunk = (uint64_t)sme::passage::kChunk;
  });
}

int sme_index_term_fingerprints(sme_index *ix, uint64_t *d_out, void *stream) {
  return guard([&] {
    if (!ix || (!d_out && ix->V > 0)) throw sme::Error(SME_EINVAL, "null argument");
    if (ix->job != 0) throw sme::Error(SME_EINVAL, "not a TermKGramDocIndexer index");
    set_device(ix->ctx);
    hipStream_t st = stream_of(ix->ctx, stream);
    sme::term_fingerprints(ix, d_out, st);
    SME_HIP(hipStreamSynchronize(st));
  });
}

int sme_df_owner_pack(sme_ctx *ctx, const uint64_t *d_fp, const int64_t *d_df, int64_t n, int world,
                      uint64_t *d_send_fp, int64_t *d_send_df, int64_t *d_pos, int64_t *counts, void *stream) {
  return guard([&] {
    if (!ctx || !counts || n < 0 || (n > 0 && (!d_fp || !d_df || !d_send_fp || !d_send_df || !d_pos)))
      throw sme::Error(SME_EINVAL, "bad argument");
    set_device(ctx);
    sme::dfx_pack(ctx, d_fp, d_df, n, world, d_send_fp, d_send_df, d_pos, counts, stream_of(ctx, stream));
  });
}

int sme_df_owner_sum(sme_ctx *ctx, const uint64_t *d_fp, const int64_t *d_df, int64_t n, int64_t *d_out,
                     int64_t *distinct, void *stream) {
  return guard([&] {
    if (!ctx || !distinct || n < 0 || (n > 0 && (!d_fp || !d_df || !d_out)))
      throw sme::Error(SME_EINVAL, "bad argument");
    set_device(ctx);
    sme::dfx_sum(ctx, d_fp, d_df, n, d_out, distinct, stream_of(ctx, stream));
  });
}

int sme_df_owner_unpack(sme_ctx *ctx, const int64_t *d_ret, const int64_t *d_pos, int64_t n, int64_t *d_out,
                        void *stream) {
  return guard([&] {
    if (!ctx || n < 0 || (n > 0 && (!d_ret || !d_pos || !d_out))) throw sme::Error(SME_EINVAL, "bad argument");
    set_device(ctx);
    hipStream_t st = stream_of(ctx, stream);
    sme::dfx_unpack(d_ret, d_pos, n, d_out, st);
    SME_HIP(hipStreamSynchronize(st));
  });
}

int sme_topk_merge_rows(sme_ctx *ctx, const double *d_score, const int32_t *d_docno, const uint32_t *d_tie,
                        int64_t rows, int m, int k, int32_t *d_out_docno, double *d_out_score, uint32_t *d_out_tie,
                        void *stream) {
  return guard([&] {
    if (!ctx || rows < 0 || m < 0 || k < 1 || (rows > 0 && (!d_out_docno || !d_out_score || (m > 0 && (!d_score || !d_docno)))))
      throw sme::Error(SME_EINVAL, "bad argument");
    set_device(ctx);
    hipStream_t st = stream_of(ctx, stream);
    sme::merge_rows(d_score, d_docno, d_tie, rows, m, k, d_out_docno, d_out_score, d_out_tie, st);
    SME_HIP(hipStreamSynchronize(st));
  });
}

int sme_count_shared_keys(sme_ctx *ctx, const uint64_t *d_rows, int64_t n, int64_t *count, void *stream) {
  return guard([&] {
    if (!ctx || !count || n < 0 || (n > 0 && !d_rows)) throw sme::Error(SME_EINVAL, "bad argument");
    set_device(ctx);
    *count = sme::count_shared_keys(ctx, d_rows, n, stream_of(ctx, stream));
  });
}

int sme_index_reweight(sme_index *ix, int64_t n_global, const int64_t *d_df_global, void *stream) {
  return guard([&] {
    if (!ix || n_global < 0) throw sme::Error(SME_EINVAL, "bad argument");
    need_query_side(ix);
    set_device(ix->ctx);
    sme::reweight_index(ix, n_global, d_df_global, stream_of(ix->ctx, stream));
  });
}

int sme_index_record_docnos(sme_index *ix, const int32_t **d_docno, int64_t *n) {
  return guard([&] {
    if (!ix || !d_docno || !n) throw sme::Error(SME_EINVAL, "null argument");
    if (ix->job != 0) throw sme::Error(SME_EINVAL, "not a TermKGramDocIndexer index");
    need_record_docnos(ix);
    *d_docno = (const int32_t *)ix->d_rec_docno.p;
    *n = ix->N;
  });
}

int sme_index_pack_pieces(sme_index *ix, int world, void *d_out, uint64_t *sizes, void *stream) {
  return guard([&] {
    if (!ix || !sizes) throw sme::Error(SME_EINVAL, "null argument");
    need_query_side(ix);
    need_record_docnos(ix);
    set_device(ix->ctx);
    hipStream_t st = stream_of(ix->ctx, stream);
    sme::pack_pieces(ix, world, (uint8_t *)d_out, sizes, st);
    SME_HIP(hipStreamSynchronize(st));
  });
}

int sme_merge_pieces(sme_ctx *cx, const void *d_blobs, const uint64_t *sizes, int n, void *stream, sme_index **out) {
  return guard([&] {
    if (!cx || !d_blobs || !sizes || !out || n < 1) throw sme::Error(SME_EINVAL, "bad argument");
    set_device(cx);
    *out = sme::merge_pieces(cx, (const uint8_t *)d_blobs, sizes, n, stream_of(cx, stream));
  });
}

int sme_index_merge(sme_ctx *cx, sme_index *const *indexes, int n, void *stream, sme_index **out) {
  return guard([&] {
    if (!cx || !out) throw sme::Error(SME_EINVAL, "null argument");
    if (!indexes) throw sme::Error(SME_EINVAL, "index merge: a null input list");
    set_device(cx);
    hipStream_t st = stream_of(cx, stream);
    sme_index *ix = nullptr;
    try {
      ix = sme::merge_indexes(cx, indexes, n, st);
    } catch (...) {
      (void)hipStreamSynchronize(st);  // kernels may still use the scratch that went back to the pool
      throw;
    }
    cx->last_profile = ix->profile;
    *out = ix;
  });
}

int sme_index_merge_stats(const sme_index *ix, uint64_t *inputs, uint64_t *shared_terms, uint64_t *merged_postings,
                          uint64_t *appended) {
  return guard([&] {
    if (!ix || !inputs || !shared_terms || !merged_postings || !appended)
      throw sme::Error(SME_EINVAL, "null argument");
    *inputs = ix->mg_inputs;
    *shared_terms = ix->mg_shared;
    *merged_postings = ix->mg_merged;
    *appended = ix->mg_appended;
  });
}

namespace {
int delete_docnos_entry(sme_index *ix, const int32_t *list, int64_t n, bool on_device, void *stream, sme_index **out) {
  return guard([&] {
    hipStream_t st = nullptr;
    if (ix && out) {  // (a null argument is the validator's to refuse, before anything else)
      set_device(ix->ctx);
      st = stream_of(ix->ctx, stream);
    }
    sme_index *res = nullptr;
    try {
      res = sme::delete_docnos(ix, list, n, on_device, out != nullptr, st);
    } catch (...) {
      if (ix && out) (void)hipStreamSynchronize(st);  // kernels may still use the scratch that went back to the pool
      throw;
    }
    ix->ctx->last_profile = res->profile;
    *out = res;
  });
}
}  // namespace

int sme_index_delete_docnos(sme_index *ix, const int32_t *docnos, int64_t n, void *stream, sme_index **out) {
  return delete_docnos_entry(ix, docnos, n, false, stream, out);
}

int sme_index_delete_docnos_device(sme_index *ix, const int32_t *d_docnos, int64_t n, void *stream, sme_index **out) {
  return delete_docnos_entry(ix, d_docnos, n, true, stream, out);
}

int sme_index_delete_stats(const sme_index *ix, uint64_t *docnos, uint64_t *records, uint64_t *postings,
                           uint64_t *terms) {
  return guard([&] {
    if (!ix || !docnos || !records || !postings || !terms) throw sme::Error(SME_EINVAL, "null argument");
    *docnos = ix->dl_docnos;
    *records = ix->dl_records;
    *postings = ix->dl_postings;
    *terms = ix->dl_terms;
  });
}

int sme_index_positions_file_device(sme_index *ix, int bits, void *stream, const void **d_buf, size_t *n) {
  return guard([&] {
    sme::check_positions_file_call(ix, d_buf && n, bits);
    set_device(ix->ctx);
    hipStream_t st = stream_of(ix->ctx, stream);
    try {
      sme::positions_file(ix, bits, st);
    } catch (...) {
      (void)hipStreamSynchronize(st);  // kernels may still use the scratch that went back to the pool
      throw;
    }
    *d_buf = ix->d_pf_file.p;
    *n = (size_t)ix->pf_bytes;
  });
}

int sme_index_positions_file(sme_index *ix, int bits, void *stream, const uint8_t **buf, size_t *n) {
  return guard([&] {
    sme::check_positions_file_call(ix, buf && n, bits);
    const void *d = nullptr;
    size_t bytes = 0;
    const int rc = sme_index_positions_file_device(ix, bits, stream, &d, &bytes);
    if (rc != SME_OK) throw sme::Error(rc, g_err);
    ix->h_pf_file.resize(std::max<size_t>(bytes, 1));
    hipStream_t st = stream_of(ix->ctx, stream);
    SME_HIP(hipMemcpyAsync(ix->h_pf_file.data(), d, bytes, hipMemcpyDeviceToHost, st));
    SME_HIP(hipStreamSynchronize(st));
    *buf = ix->h_pf_file.data();
    *n = bytes;
  });
}

namespace {
int attach_positions_entry(sme_index *ix, const uint8_t *h_file, const void *d_file, size_t n, int flags, void *stream) {
  return guard([&] {
    hipStream_t st = nullptr;
    if (ix) {  // (a null argument is the validator's to refuse, before anything else)
      set_device(ix->ctx);
      st = stream_of(ix->ctx, stream);
    }
    try {
      sme::attach_positions(ix, h_file, d_file, n, flags, true, st);
    } catch (...) {
      if (ix) (void)hipStreamSynchronize(st);  // kernels may still use the scratch that went back to the pool
      throw;
    }
  });
}
}  // namespace

int sme_index_attach_positions(sme_index *ix, const uint8_t *file, size_t n, int flags, void *stream) {
  return attach_positions_entry(ix, file, nullptr, n, flags, stream);
}

int sme_index_attach_positions_device(sme_index *ix, const void *d_file, size_t n, int flags, void *stream) {
  return attach_positions_entry(ix, nullptr, d_file, n, flags, stream);
}

int sme_index_posfile_stats(const sme_index *ix, uint64_t *file_bytes, uint64_t *bits, uint64_t *checked_postings,
                            float *encode_ms, float *decode_ms, float *crosscheck_ms) {
  return guard([&] {
    if (!ix || !file_bytes || !bits || !checked_postings) throw sme::Error(SME_EINVAL, "null argument");
    *file_bytes = ix->pf_bytes;
    *bits = ix->pf_bits;
    *checked_postings = ix->pf_checked;
    if (encode_ms) *encode_ms = ix->pf_encode_ms;
    if (decode_ms) *decode_ms = ix->pf_decode_ms;
    if (crosscheck_ms) *crosscheck_ms = ix->pf_crosscheck_ms;
  });
}

int sme_last_build_profile(const sme_ctx *cx, const char **json) {
  return guard([&] {
    if (!cx || !json) throw sme::Error(SME_EINVAL, "null argument");
    std::ostringstream os;
    os << "{";
    for (size_t i = 0; i < cx->last_profile.size(); i++)
      os << (i ? "," : "") << "\"" << cx->last_profile[i].first << "\":" << cx->last_profile[i].second;
    if (cx->last_query_ms >= 0) os << (cx->last_profile.empty() ? "" : ",") << "\"query_kernel\":" << cx->last_query_ms;
    if (cx->last_query_ms >= 0) os << ",\"query_prep\":" << cx->last_query_prep_ms;
    if (cx->last_query_ms >= 0) os << ",\"query_index\":" << cx->last_query_index_ms;
    if (cx->last_query_ms >= 0) os << ",\"query_kernel_name\":\"" << cx->last_query_name << "\"";
    if (cx->last_query_ms >= 0 && cx->last_query_name == std::string("k_query_win"))
      os << ",\"query_seed\":" << cx->last_query_seed_ms << ",\"query_final\":" << cx->last_query_final_ms
         << ",\"query_overflow\":" << cx->last_query_overflow << ",\"query_fallback\":" << cx->last_query_fallback << ",\"query_stages\":" << cx->last_query_stages << ",\"query_slices\":" << cx->last_query_slices
         << ",\"query_split\":" << (cx->last_query_split ? 1 : 0) << ",\"query_total\":" << cx->last_query_total_ms;
    os << "}";
    const_cast<sme_ctx *>(cx)->profile_json = os.str();
    *json = cx->profile_json.c_str();
  });
}

}  // extern "C"
