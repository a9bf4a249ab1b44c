// sme_internal.hpp -- context and index objects behind the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "sme_common.hpp"
#include "sme_result.hpp"

struct sme_ctx {
  sme::BufPool pool;  // declared first: destroyed after every DevBuf below
  sme_config cfg{};
  int device = 0;
  hipStream_t own_stream = nullptr;
  // a second stream for independent kernels of one build stage (the tf-desc
  // sort's segment classes), joined back by events
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  std::vector<hipEvent_t> prof_events;  // Prof's reusable stage events
  // docno mapping: {"", docids...} as UTF-16 (TrecDocnoMapping.readDocnoData)
  sme::DevBuf map_chars, map_off;
  int64_t map_n = 0;  // entries including the "" sentinel
  bool has_map = false;
  sme::DevBuf map_slots;  // docid hash table (entry index + 1), see k_docno
  uint64_t map_mask = 0;
  bool map_hash_ok = false;  // built, and the mapping's docids are distinct
  // build workspace, reused across builds (see DevBuf)
  sme::DevBuf ws[128];  // 48..63 query / serializer / tokenizer / reweight, 64..127 build
  sme::DevBuf cub_tmp;
  sme::DevBuf q_gates;  // k_query_win: per-query gate of the current thresholds (k_gates)
  uint64_t vocab_long_cap = 0, vocab_ovf_cap = 0, raw_cap_hint = 0, lt_cap_hint = 0;  // learned across builds
  std::string profile_json;
  std::vector<std::pair<std::string, float>> last_profile;
  std::vector<uint8_t> mapping_out;  // last sme_number_documents result
  std::vector<int32_t> h_wlist;      // k_query_win window order of the last batch (source of an async copy)
  float last_query_ms = -1.0f;  // device time of the last query kernel launch
  float last_query_prep_ms = -1.0f;  // per-batch tables before it (skip / impact tables, query order)
  float last_query_index_ms = -1.0f;  // one-time heavy-row build of the index it ran on (prepare_queries)
  bool last_query_tiled = false;  // tiled path (k_query_win / k_query_bm) or the streaming k_query
  const char *last_query_name = "k_query";  // the scoring kernel that ran
  float last_query_seed_ms = 0.0f, last_query_final_ms = 0.0f, last_query_total_ms = 0.0f;
  int64_t last_query_overflow = 0;  // k_query_win queries whose first candidate list overflowed
  int64_t last_query_fallback = 0;  // of those, queries finally scored by k_query_bm
  int64_t last_query_stages = 0;    // k_query_win launches of the first round (1: unstaged)
  int64_t last_query_slices = 0;    // query slices per window of that round's launches
  bool last_query_split = false;     // the batch was split by query range (table budget)
  // Path options (sme_set_option).  Every setting gives identical results; they
  // exist so tests can hold each path to the others and benches can sweep them.
  int64_t opt_query_kernel = 0;   // "query_kernel": 0 window-major (auto), 1 streaming k_query, 2 block-max sweep
  int64_t opt_heavy_div = 128;    // "heavy_div": heavy rows for terms with df >= span / div (0: none)
  int64_t opt_seed_tiles = 4;     // "seed_tiles": best-bound tiles scored before the sweep (0..8)
  int64_t opt_query_order = 1;    // "query_order": 1 heaviest-term query order, 0 batch order
  int64_t opt_agg_two_pass = 0;   // "agg_two_pass": 1 = count + emit aggregation passes
  int64_t opt_agg_grid = 0;      // "agg_grid": aggregation workgroups (0 = auto)
  int64_t opt_tok_grid = 5120;    // "tok_grid": tokenizer workgroups (>= 1): four rounds of 5 per CU x 256 CUs
  int64_t opt_raw_load_pct = 40;  // "raw_load_pct": raw-vocabulary table load of the next build (10..90)
  int64_t opt_docid_terms = 1;    // "docid_terms": docid terms beside the word vocabulary (K4b; 0 = general path)
  int64_t opt_sort_bits = 0;      // "sort_digit_bits": most bits per digit of the term sort's LSD passes (6..11; 0 auto)
  int64_t opt_term_off_tables = 1;  // "term_off_tables": 1 = CSR offsets from the term sort's tables (sorted keys only when read), 0 = from the sorted keys
  int64_t opt_docid_split = 1;    // "docid_split": docid pairs beside the term sort (K6b): 1 past 22 merged id bits, 2 whenever the words need fewer, 0 never
  int64_t opt_cand_cap = 1024;    // "cand_cap": candidate list per query of k_query_win (1..2048; >= 1024: at least 16 k)
  int64_t opt_seed_m = 64;        // "seed_m": seed postings per term (k_query_seed; 0 = no seed)
  int64_t opt_kgram_rank = 0;     // "kgram_rank": 1 = K >= 2 gram keys by iterated ranking even when packed ids fit
  int64_t opt_win_slice = 0;      // "win_slice": queries per k_query_win workgroup slice (0 = auto: 128, 256 from 1024 windows)
  int64_t opt_win_sample = 1;     // "win_sample": 1 = every 8th window first, thresholds raised, then the rest
  int64_t opt_win_stage_min = 0;   // "win_stage_min": windows of the first stage (at least; the stage count follows; 0 = auto)
  int64_t opt_query_budget = 0;  // "query_table_budget": per-batch skip-table bytes (0: a quarter of free HBM)
  int64_t opt_wild_scan = 0;      // "wild_scan": 1 = every wildcard pattern takes the whole vocabulary as candidates
  int64_t opt_wild_chunk = 1024;  // "wild_chunk": wildcard candidates per workgroup (64..4096, multiples of 64)
  int64_t opt_fuzzy_scan = 0;      // "fuzzy_scan": 1 = every suggestion word takes the whole vocabulary as candidates
  int64_t opt_bool_chunk = 1024;  // "bool_chunk": Boolean-query candidates per workgroup (64..4096, multiples of 64)
  int64_t opt_bool_driver = 0;    // "bool_driver": 0 = the required group with the fewest postings drives, 1 = the first
  int64_t opt_positions = 0;      // "positions": 1 = a K = 1 build keeps every record's term stream (phrase queries)
  int64_t opt_struct_narrow = 1;  // "struct_narrow": 1 = a structured query's term groups cut its operator leaves' candidates
  int64_t opt_fb_slots = 4096;    // "fb_slots": entries of relevance feedback's on-chip table (16..4096, a power of two)
  int64_t opt_merge_tile = 1024;  // "merge_tile": postings per tile of the index merger (64..2048, multiples of 64)
  int64_t opt_merge_append = 1;   // "merge_append": 1 = inputs of disjoint docno ranges are laid end to end, 0 = always merged
  int64_t opt_bm25_split = 0;     // "bm25_split": BM25 scorer workgroups per query (0 = auto; capped at the window count)
  int64_t opt_rescore_path = 0;   // "rescore_path": a rescore slot's form: 0 by its cost, 1 always search, 2 always scan
  int64_t opt_delete_tile = 16384; // "delete_tile": postings per tile of the index deletion pass (256..65536, multiples of 256)
  int64_t opt_corpus_keep = int64_t(16) << 30;  // "corpus_keep_bytes": host-corpus builds keep their device copy
                                                // (no hipMalloc next build) only up to this size
  // pinned host staging of device -> host record copies into pageable caller
  // memory (sme_index_copy_records): two buffers, DMA into one while the host
  // copies out of the other
  void *h_stage[2] = {nullptr, nullptr};
  size_t h_stage_cap = 0;
  // device copy of a host corpus (sme_build_index), kept across builds
  sme::DevBuf h_corpus_dev;
  // indexes borrow the context (its pool, workspace, stream): sme_destroy defers
  // the delete until the last index is freed, whatever order a host frees them in
  int live_indexes = 0;
  bool destroyed = false;
};

struct sme_index {
  sme_ctx *ctx = nullptr;
  int K = 1, R = 1, idf_mode = 0;
  int job = 0;               // 0 TermKGramDocIndexer index, 1 CharKGramTermIndexer output
  int64_t cg_ngrams = 0, cg_pairs = 0;  // job 1: distinct char k-grams, (gram, term) set entries
  int64_t N = 0, V = 0, P = 0;
  int64_t Vt = 0;  // term vocabulary size (V counts k-grams when K > 1)
  int32_t max_tf = 0;
  int64_t dmin = 0, dmax = -1;  // docno range of the records (query doc tiles)
  // sorted vocabulary (rank order): UTF-16 units
  sme::DevBuf d_term_off;    // int64 [V+1]
  sme::DevBuf d_term_chars;  // uint16
  // query-side CSR: postings per term in docno-ascending order, fp64 TF-IDF weights
  sme::DevBuf d_off;      // int64 [V+1]
  sme::DevBuf d_docno_d;  // int32 [P]
  sme::DevBuf d_tf_d;     // int32 [P]
  sme::DevBuf d_w;        // double [P]
  sme::DevBuf d_idf;      // double [V]   idf of every term (query side: w = lut[tf] * idf)
  sme::DevBuf d_gram;     // int32 [V * K]  term ids of every k-gram (K > 1)
  sme::DevBuf d_lut;      // double [max_tf + 1]  1 + ln(tf)
  // reduce-output CSR: (tf desc, docno asc) per term (MyReducer.reduce order)
  sme::DevBuf d_docno_o;  // int32 [P]
  sme::DevBuf d_tf_o;     // int32 [P]
  // docno of every record in input order (for the " " doc-counter postings)
  sme::DevBuf d_rec_docno;  // int32 [N]
  sme::DevBuf d_rec_first;  // u8 [N]: record starts a map task (split) -- merged shard pieces only
  bool records_only = false;  // merged shard pieces (sme_merge_pieces): reduce-order CSR + records, no query side
  // loaded from record streams (sme_index_from_records): d_rec_docno lacks every map task's last docno
  bool from_records = false;
  // every entry of d_rec_docno is the record's real docno: a build, a merge of such
  // inputs, a deletion from one -- not an index opened from part files (sme_load.hip)
  bool rec_complete = true;
  // serialized partitions (lazily built)
  sme::DevBuf d_ser;
  std::vector<int64_t> part_start;  // R+1
  bool ser_ready = false;
  float ser_ms = 0.0f;  // device time of the k_ser_* pass (serialize_index)
  // host copies of the partitions (sme_index_partition_records), not zero-filled
  std::vector<std::unique_ptr<uint8_t[]>> h_parts;
  std::vector<char> h_parts_ready;
  // host copies (lazily)
  std::vector<int64_t> h_off;
  std::vector<int32_t> h_docno, h_tf, h_df;
  bool h_csr_ready = false;
  std::vector<int64_t> h_term_off;
  std::vector<uint16_t> h_term_chars;
  std::vector<int32_t> h_gram;
  std::vector<uint8_t> h_term_tmp;
  bool h_terms_ready = false;
  // query-side heavy rows (prepare_queries, sme_query.hip): tf byte rows, 16-doc
  // and 1024-doc block maxima of the terms covering >= 1/div of the docno span
  sme::DevBuf d_hrow_of;  // int32 [V] heavy row or -1
  // u8 [H][T * 1024] tf | imp | [H][T * 64] bm16 | [H][T] bm1k | [H][T * 256] sbq
  sme::DevBuf d_heavy;
  const uint8_t *q_tfrow = nullptr, *q_bm16 = nullptr, *q_bm1k = nullptr, *q_imp = nullptr;
  const uint8_t *q_sbq = nullptr;  // impact maxima of 4-document sub-blocks (k_query_win's second level)
  // k_query_win's sparse postings, one word per docno-order posting of a term
  // without a heavy row: (docno - dmin) mod 4096 | q(tf) << 12 | min(tf, 4095) << 20
  sme::DevBuf d_spk;
  const uint32_t *q_spk = nullptr;
  double q_alpha = 1.0;                 // impact scale 253.5 / (largest weight of any term)
  unsigned long long q_wmax_bits = 0;   // that weight's bits
  int64_t q_T = 0, q_H = 0, q_div = -1;
  bool q_ready = false;
  float q_prep_ms = 0.0f;
  // wildcard expansion (sme_wild.hip): the vocabulary's character-trigram table,
  // built on first use and kept (it depends on the term strings only) ...
  sme::DevBuf d_wkeys;   // uint64 [G]      distinct trigram keys, ascending
  sme::DevBuf d_wgoff;   // int32 [G + 1]   CSR offsets into d_wgterm
  sme::DevBuf d_wgterm;  // int32 [pairs]   term ids per key, ascending
  int64_t wild_G = 0, wild_pairs = 0;
  bool wild_ready = false;
  float wild_ms = 0.0f;
  // ... and the last expansion (its result: sme_result.hpp), with the uploaded
  // batch and scratch per pattern and per candidate chunk
  sme::TermIds wx;
  sme::DevBuf d_wx_in, d_wx_plan, d_wx_choff, d_wx_moff, d_wx_scan;
  // spelling suggestions (sme_fuzzy.hip): the last call's result; cands counts the
  // (word, term) pairs length-tested, fz_scanned the words that took the whole vocabulary
  sme::TermDists fz;
  uint64_t fz_scanned = 0;
  // Boolean retrieval (sme_bool.hip): the last call's result; cands counts the
  // driver postings examined
  sme::DocScores bq;
  // positions (a K = 1 build with the "positions" option; sme_phrase.hip): the
  // records' term streams in docno-ascending record order -- a forward index.
  // Empty buffers (ps_records == 0 and nothing allocated) when the index keeps none.
  sme::DevBuf d_ps_off;    // int64 [ps_records + 1]  stream offsets
  sme::DevBuf d_ps_terms;  // int32 [ps_terms]        term ids in token order
  sme::DevBuf d_ps_docno;  // int32 [ps_records]      docno of each stream record, ascending
  int64_t ps_records = 0, ps_terms = 0;
  bool has_positions = false;
  int64_t idf_N = 0;  // the N the weights were last computed with (build, sme_index_reweight)
  // phrase queries: the last call's result (freq: occurrences of the phrase);
  // cands counts the driver postings, verified the filter's survivors
  sme::DocFreqScores pq;
  // proximity queries (sme_near.hip): the last call's result, as for phrases, and
  // the scorer table 1 + ln(f) for f < nq_lut_n -- d_lut's bits continued past
  // max_tf (an unordered freq can pass it); filled on first use, it only grows
  sme::DocFreqScores nq;
  sme::DevBuf d_nq_lut;  // double [nq_lut_n]
  int64_t nq_lut_n = 0;
  int64_t nq_max_span = -1;  // the most stream positions of one docno (-1: not yet found), a bound on any freq
  // structured queries (sme_structq.hip): the last call's result (verified: (leaf,
  // document) pairs scanned; cands: driver entries examined) and the operator
  // leaves evaluated, and in sv the virtual posting lists of those leaves -- leaf
  // i's documents (docno ascending) and values at its offsets i, i + 1 -- written by
  // the proximity pass with that pass's counts.  sv is no alias of nq: a structured
  // call leaves a proximity result alone.
  sme::DocScores sq;
  uint64_t sq_leaves = 0;
  sme::DocFreqScores sv;
  // relevance feedback (sme_feedback.hip): the last call's result and its counts --
  // stream positions of the sets, (set, term) pairs before the filters, pairs kept
  // before the cut, set docnos without a record, sets that took the large path
  sme::TermFreqDocsScores fb;
  uint64_t fb_positions = 0, fb_pairs = 0, fb_kept = 0, fb_missing = 0, fb_spilled = 0;
  // a merged index (sme_index_merge, sme_ixmerge.hip): its inputs, the terms two or
  // more of them held, the postings that equal docnos merged away, and whether
  // the concatenation path ran
  uint64_t mg_inputs = 0, mg_shared = 0, mg_merged = 0, mg_appended = 0;
  // an index sme_index_delete_docnos made (sme_ixdelete.hip): the listed docnos some
  // record had, and the records, postings and terms that went
  uint64_t dl_made = 0, dl_docnos = 0, dl_records = 0, dl_postings = 0, dl_terms = 0;
  // the positions file (sme_posfile.hip): the last file written (device bytes, and the
  // host copy the host entry hands out), and the last posfile call's counts and times
  sme::DevBuf d_pf_file;
  std::vector<uint8_t> h_pf_file;
  uint64_t pf_bytes = 0, pf_bits = 0, pf_checked = 0;
  float pf_encode_ms = 0.0f, pf_decode_ms = 0.0f, pf_crosscheck_ms = 0.0f;
  // BM25 ranking (sme_bm25.hip): the collection tables, built once per index (they
  // depend on the postings only), the last call's norm table and its counts
  sme::DevBuf d_bm_dl;     // int32 [bm_span]   dl[docno - dmin], 0 for a docno without postings
  sme::DevBuf d_bm_idf;    // double [V]        host-libm idf by true df
  sme::DevBuf d_bm_maxtf;  // int32 [V]         largest tf of every term
  sme::DevBuf d_bm_mindl;  // int32 [bm_nwin]   smallest non-zero dl of every window
  sme::DevBuf d_bm_norm;   // double [bm_span]  the last call's norm_d
  sme::DevBuf d_bm_stat;   // u64 [3]           the last call's windows, skipped, postings
  int64_t bm_span = 0, bm_nwin = 0;
  uint64_t bm_docs = 0, bm_total_len = 0, bm_max_len = 0;
  bool bm_ready = false, bm_called = false;
  float bm_ms = 0.0f;
  hipStream_t bm_stream = nullptr;  // the last call's stream (the counts are read behind it)
  // scoring given documents (sme_rescore.hip): the last call's result (freq: the
  // slots whose list holds the document; cands: the batch's candidates, verified:
  // the sum of those hits)
  sme::DocFreqScores rs;
  // best passages (sme_passage.hip): the last call's rows (cands: the batch's
  // candidates, matches: the rows before the cut) and, if it asked for them, the
  // rows' window terms; the candidates with a record and their stream positions
  sme::PassageRows pw;
  sme::WindowTerms pwt;
  uint64_t pw_with_record = 0, pw_positions = 0;
  // stage timings of the build that produced this index (ms)
  std::vector<std::pair<std::string, float>> profile;
  ~sme_index() { ctx->live_indexes--; }  // members (pooled buffers) are released after this body
  explicit sme_index(sme_ctx *c) : ctx(c) {
    c->live_indexes++;
    for (sme::DevBuf *b : {&d_term_off, &d_term_chars, &d_off, &d_docno_d, &d_tf_d, &d_w, &d_idf, &d_lut, &d_gram, &d_docno_o,
                           &d_tf_o, &d_rec_docno, &d_rec_first, &d_ser, &d_hrow_of, &d_heavy, &d_spk, &d_wkeys, &d_wgoff,
                           &d_wgterm, &d_wx_in, &d_wx_plan, &d_wx_choff, &d_wx_moff, &d_wx_scan, &d_ps_off, &d_ps_terms,
                           &d_ps_docno, &d_nq_lut, &d_pf_file, &d_bm_dl, &d_bm_idf, &d_bm_maxtf, &d_bm_mindl, &d_bm_norm,
                           &d_bm_stat})
      b->pool = &c->pool;
    for (sme::ResultSet *r : std::initializer_list<sme::ResultSet *>{&wx, &fz, &bq, &pq, &nq, &sq, &sv, &fb, &rs, &pw,
                                                                     &pwt})
      r->bind(&c->pool);
  }
};

namespace sme {
// per-stage device-event timer of a build
struct Prof {
  // stage events come from a pool kept by the context (hipEventCreate per mark
  // cost host time between a build's launches); events of an abandoned Prof
  // (an exception) go back to the pool in the destructor
  hipStream_t st;
  std::vector<hipEvent_t> *pool;
  std::vector<std::pair<std::string, hipEvent_t>> ev;
  Prof(hipStream_t s, std::vector<hipEvent_t> *p) : st(s), pool(p) { mark("start"); }
  ~Prof() {
    for (auto &e : ev) pool->push_back(e.second);
  }
  void mark(const char *name) {
    hipEvent_t e;
    if (!pool->empty()) {
      e = pool->back();
      pool->pop_back();
    } else {
      SME_HIP(hipEventCreate(&e));
    }
    ev.emplace_back(name, e);
    last_stage() = name;
    SME_HIP(hipEventRecord(e, st));
  }
  std::vector<std::pair<std::string, float>> finish() {
    SME_HIP(hipEventSynchronize(ev.back().second));
    std::vector<std::pair<std::string, float>> out;
    for (size_t i = 1; i < ev.size(); i++) {
      float ms = 0;
      SME_HIP(hipEventElapsedTime(&ms, ev[i - 1].second, ev[i].second));
      out.emplace_back(ev[i].first, ms);
    }
    float tot = 0;
    SME_HIP(hipEventElapsedTime(&tot, ev.front().second, ev.back().second));
    out.emplace_back("total", tot);
    for (auto &p : ev) pool->push_back(p.second);
    ev.clear();
    return out;
  }
};

struct RecordSpans {
  uint64_t *rs, *re;  // record [rs, re) byte spans, in reader order
  int64_t nR;
  uint64_t *C;        // sorted positions of '<' whose markup is not "simple"
  int64_t nC;
  int lt_attempts;   // passes of the '<' list loop (1: the first capacity held)
};
void build_docid_hash(sme_ctx *cx, bool distinct, hipStream_t st);
RecordSpans find_records(sme_ctx *cx, const uint8_t *d_text, uint64_t n, hipStream_t st, Prof *prof);
void split_points(sme_ctx *cx, const uint8_t *d_text, uint64_t n, int world, uint64_t *h_cuts, hipStream_t st);
void number_documents(sme_ctx *cx, const uint8_t *d_text, uint64_t n, hipStream_t st, std::vector<uint8_t> &out);
sme_index *build_index(sme_ctx *cx, const uint8_t *d_text, uint64_t n, hipStream_t st, int job = 0);
// CharKGramTermIndexer stage over the file-order term stream (sme_chargram.hip)
void chargram_stage(sme_ctx *cx, sme_index *ix, const int32_t *tstream, int64_t M, int64_t V, const int64_t *term_off,
                    const uint16_t *term_chars, hipStream_t st, Prof *prof);
// stable LSD radix sort of (term id, packed posting) pairs (sme_sort.hip)
// (reg != nullptr: the first pass reads pair x from reg[i] + x - xoff[i], record i
// holding it -- the single-pass aggregation's layout)
// (xw != nullptr: K6b -- the keys are word ranks; the last pass writes word i's
// postings shifted by xw[i].x and keyed xw[i].y into Pout slots keyed 0xFFFFFFFF)
uint32_t *term_sort(uint32_t *k0, uint32_t *v0, uint32_t *k1, uint32_t *v1, int64_t nrec, const int64_t *reg,
                    const int64_t *xoff, int64_t P, int bits, int64_t dmin, uint32_t F, int32_t *docno, int32_t *tf,
                    uint32_t *counts, hipStream_t st, const double *lut = nullptr, double idf = 0.0,
                    double *w = nullptr, int maxbits = 11, const uint2 *xw = nullptr, int64_t Pout = 0,
                    const uint32_t *rec_val = nullptr, int tf_shift = 0, int64_t *off_out = nullptr, int64_t V = 0,
                    int64_t vend = 0, bool write_keys = true);
// (off_out != nullptr: the first slot of every term id < V that has pairs, read
// from the last pass's offset table, and off_out[vend ? vend : V] = the pair count;
// write_keys false: the sorted keys are not stored)
// (rec_val != nullptr, gather mode: the regions hold one packed word per pair,
// term | tf << tf_shift, and rec_val[i] = record i's base value; v0 is then read
// by no pass, and written only when there are three passes or more)
int term_sort_passes(int bits, int maxbits);
size_t term_sort_scratch(int64_t P);
// stable LSD radix sort of (key, u32 value) pairs by the key's low `bits` bits
// (sme_sort.hip; K = uint32_t or uint64_t); ping-pongs between (k0, v0) and
// (k1, v1) and returns the sorted values' buffer (keys beside it if keys_out)
template <typename K>
uint32_t *kv_sort(K *k0, uint32_t *v0, K *k1, uint32_t *v1, int64_t n, int bits, uint32_t *scratch, hipStream_t st,
                  bool keys_out = false);
size_t kv_sort_scratch(int64_t n);
// device-wide exclusive scan out[i] = sum in[0..i) (in == out allowed; scratch:
// one T per 4096 items), and flag compaction (ascending indices of the nonzero
// flags, their count to *d_count) -- hand-written, sme_sort.hip
template <typename T>
void excl_scan(const T *in, T *out, int64_t n, DevBuf &scratch, hipStream_t st);
void select_flagged(const uint8_t *flag, int64_t n, int32_t *out, int32_t *d_count, DevBuf &s1, DevBuf &s2,
                    hipStream_t st);
// SortPairs-shaped wrappers of kv_sort (separate in / out arrays; the inputs are
// clobbered): u32 values, or 64-bit values through a sorted index + gather
template <typename K>
void sort_pairs(K *keys_in, K *keys_out, uint32_t *vals_in, uint32_t *vals_out, int64_t n, int bits, DevBuf &radix,
                hipStream_t st);
template <typename K>
void sort_pairs_v64(K *keys_in, K *keys_out, const uint64_t *vals_in, uint64_t *vals_out, int64_t n, int bits,
                    DevBuf &ia, DevBuf &ib, DevBuf &radix, hipStream_t st);
// *d_max = the largest of n >= 1 values (non-negative integers)
template <typename T>
void reduce_max(const T *in, int64_t n, T *d_max, hipStream_t st);
// runs of equal keys (sorted input) -> (key, sum of vals) per run, *d_runs = count
void reduce_by_key_sum(const uint64_t *keys, const int32_t *vals, int64_t n, uint64_t *ukeys, int32_t *sums,
                       int64_t *d_runs, DevBuf &flags, DevBuf &pos, DevBuf &scan, hipStream_t st);
// K8, the reducer's output order (sme_tfsort.hip): per segment [off[s], off[s + 1])
// of the term CSR, s < V, P = off[V], a stable sort by tf descending of (docno_d, tf_d) into
// (docno_o, tf_o); the inputs stay as they are.  A segmented counting sort for
// 1 <= max_tf <= kTfSortMaxTf (every tf in 0..max_tf); tf_d is 16-byte aligned.
// Scratch: lists (3 (V + 1) int64), tiles (V + 1 int64), tcnt (one u32 per tile of
// 4096 postings and tf value + one per tile), scan (excl_scan's) and the four
// device counters nseg.  The shorter segment classes run on aux_stream between
// the two events; on every exit, a throw included, st waits for aux_stream.
constexpr int kTfSortMaxTf = 1023;  // LDS counters (max_tf + 1) x 16 x 4 B <= 64 KiB
void tf_sort_segments(const int64_t *off, int64_t V, int64_t P, const int32_t *docno_d, const int32_t *tf_d,
                      int max_tf, int32_t *docno_o, int32_t *tf_o, DevBuf &lists, DevBuf &tiles, DevBuf &tcnt, DevBuf &scan,
                      unsigned long long *nseg, hipStream_t st, hipStream_t aux_stream, hipEvent_t ev_fork,
                      hipEvent_t ev_join);
void serialize_index(sme_index *ix, hipStream_t st);
// reference-layout output from doc shards (sme_merge.hip): per-owner blobs of a
// shard's terms and postings, and the owner's merge of the received blobs
void pack_pieces(sme_index *ix, int world, uint8_t *d_out, uint64_t *sizes, hipStream_t st);
sme_index *merge_pieces(sme_ctx *cx, const uint8_t *d_blobs, const uint64_t *sizes, int np, hipStream_t st);
// the vocabulary union of n sources (sme_vunion.hip; merge_pieces and merge_indexes
// stand on it).  Every source term is ranked among the other sources' sorted term
// lists by String.compareTo: equal strings are adjacent in rank order, sources in
// the order ord gives them.  A rank position is a SEGMENT, one source's posting list
// of one term; a scan of the first-occurrence flags numbers the merged terms, whose
// strings come from their first source.  Writes V, Vt, d_term_off and d_term_chars
// of ix (V == 0: one zero offset).  d_tbase: n + 1 term bases, Vt = d_tbase[n] < 2^31;
// d_shared: a zeroed counter of the terms two or more sources hold, or null.  The
// caller owns the scratch; st is synchronised on return.
struct TermSource {  // device pointers of one source
  const int64_t *toff;
  const uint16_t *tch;
  int64_t n;  // terms
  const int64_t *off;
  const int32_t *dn, *tf;  // its postings, by term
};
struct UnionScratch {
  DevBuf &pos, &at_pos, &first_at, &cnt_at, &pstart, &excl, &seg_key, &seg_val, &gid, &tmap, &gstart, &glen, &scan;
};
struct VocabUnion {
  int64_t V;                        // merged terms
  const int64_t *pos;               // [Vt] rank position of flat source term j
  const int64_t *at_pos;            // [Vt] its inverse
  const uint8_t *first_at;          // [Vt] the segment is its term's first
  const int32_t *gid;               // [Vt] merged term of a segment
  const int64_t *gstart;            // [V + 1] first segment of a merged term
  const int32_t *tmap;              // [Vt] merged term of flat source term j
  const int64_t *pstart;            // [Vt + 1] the segments' lists laid end to end
  const int32_t *const *seg_key;    // [Vt] a segment's docnos
  const int32_t *const *seg_val;    // [Vt] and tfs
};
VocabUnion union_vocab(const TermSource *d_src, int n, const int64_t *d_tbase, const int32_t *d_ord, int64_t Vt,
                       sme_index *ix, unsigned long long *d_shared, UnionScratch s, hipStream_t st);
// off[g] = pstart[gstart[g]], g < V: the term offsets when the segments laid end to
// end are the postings
void segment_term_offsets(const int64_t *pstart, const int64_t *gstart, int64_t V, int64_t *off, hipStream_t st);
// the reducer's final order (sme_vunion.hip): P postings (dn, tf) grouped by term,
// term[i] < V their term ids, stably sorted by (term, tf desc) into (odn, otf) --
// keys term << tfb | (max_tf - tf) of the items in perm order (null: as they lie)
// through kv_sort<uint64_t>, then a gather.  The caller owns the scratch.
void sort_term_tf(const uint32_t *term, const int32_t *dn, const int32_t *tf, const uint32_t *perm, int64_t P,
                  int64_t V, int max_tf, int32_t *odn, int32_t *otf, DevBuf &q0, DevBuf &q1, DevBuf &v0, DevBuf &v1,
                  DevBuf &radix, hipStream_t st);
// (d_term_of: the term id of every docno-order posting, if the caller has it --
// the weights are then written by one flat pass over the postings)
void reweight_index(sme_index *ix, int64_t N, const int64_t *d_gdf, hipStream_t st,
                    const uint32_t *d_term_of = nullptr);
// n indexes of cx into one full index (sme_ixmerge.hip): vocabulary union, postings
// merged by docno with equal docnos summed, both orders, weights, kept streams
sme_index *merge_indexes(sme_ctx *cx, sme_index *const *ins, int n, hipStream_t st);
// in without the records whose docno is in the list, as a new full index
// (sme_ixdelete.hip): both posting orders compacted in place of order, the
// vocabulary, weights, doc counter and kept streams of the survivors
sme_index *delete_docnos(sme_index *in, const int32_t *list, int64_t n, bool list_on_device, bool has_out,
                         hipStream_t st);
// the term streams as a file (sme_posfile.hip): written into ix->d_pf_file from an
// index that keeps positions (bits 0: the narrowest width), and attached -- decoded,
// checked against the header, the vocabulary and, unless flags says not to, the
// postings -- to one that keeps none, from host (h_file) or device (d_file) bytes.
// The two validators of a call throw SME_EINVAL before anything else happens.
void check_positions_file_call(const sme_index *ix, bool has_args, int bits);
void positions_file(sme_index *ix, int bits, hipStream_t st);
void attach_positions(sme_index *ix, const uint8_t *h_file, const void *d_file, size_t n, int flags, bool has_args,
                      hipStream_t st);
// an index from np partition record streams laid back to back in device memory
// (sme_load.hip; part_offsets: np + 1 host entries)
sme_index *load_records(sme_ctx *cx, const uint8_t *d_records, const uint64_t *part_offsets, int np, hipStream_t st);
void prepare_queries(sme_index *ix, hipStream_t st);
// tie_bits: the reference tie word's tf width (24, or 22 when a query of the
// batch has > 256 terms); 0 = decided by this batch.  Only the nested calls of
// one batch (query-range splits, overflow subsets) pass it, so every query of a
// batch -- on every doc shard answering it -- gets the same tie words.
void query_topk(sme_index *ix, const int32_t *d_terms, const int64_t *d_qoff, int nq, int k,
                int32_t *d_out_docno, double *d_out_score, uint32_t *d_out_tie, hipStream_t st, int tie_bits = 0);
// SME_TIE_JAVA7 (sme_timsort.hip): every query's whole first-encounter list and
// the JDK 7 ComparableTimSort over it, one thread per query
void query_topk_java7(sme_index *ix, const int32_t *d_terms, const int64_t *d_qoff, int nq, int k,
                      int32_t *d_out_docno, double *d_out_score, uint32_t *d_out_tie, hipStream_t st);
void tokenize_string(sme_ctx *cx, const uint8_t *h_utf8, size_t n, std::vector<std::vector<uint16_t>> &out,
                     hipStream_t st);
void term_fingerprints(sme_index *ix, uint64_t *d_out, hipStream_t st);
// multi-GPU df exchange steps (sme_dfx.hip): owner grouping, owner sums, return gather
void dfx_pack(sme_ctx *cx, const uint64_t *fp, const int64_t *df, int64_t n, int world, uint64_t *sfp, int64_t *sdf,
              int64_t *pos, int64_t *h_counts, hipStream_t st);
void dfx_sum(sme_ctx *cx, const uint64_t *fp, const int64_t *df, int64_t n, int64_t *out, int64_t *h_distinct,
             hipStream_t st);
void dfx_unpack(const int64_t *ret, const int64_t *pos, int64_t n, int64_t *out, hipStream_t st);
// owner-side steps of the N > 1 query path (sme_owner.hip): merge of the shards'
// top-k rows, and the count of keys that arrive from two or more ranks
void merge_rows(const double *s, const int32_t *d, const uint32_t *t, int64_t rows, int m, int k, int32_t *od,
                double *os, uint32_t *ot, hipStream_t st);
int64_t count_shared_keys(sme_ctx *cx, const uint64_t *rows, int64_t n, hipStream_t st);
void lookup_terms(sme_index *ix, const std::vector<std::vector<uint16_t>> &terms, int32_t *ids,
                  hipStream_t st);
// wildcard expansion (sme_wild.hip): the vocabulary's trigram table (built once),
// and a batch of n UTF-8 patterns -> ix->wx
void prepare_wildcards(sme_index *ix, hipStream_t st);
void expand_wildcards(sme_index *ix, const uint8_t *patterns, const int64_t *offs, int n, hipStream_t st);
// spelling suggestions (sme_fuzzy.hip): a batch of n UTF-8 words -> per word the
// terms within max_dist edits, ordered and cut to m: ix->fz, and ix->fz_scanned
void suggest_terms(sme_index *ix, const uint8_t *words, const int64_t *offs, int n, int max_dist, int m,
                   hipStream_t st);
// Boolean retrieval (sme_bool.hip): nq queries of required / excluded term groups
// (host arrays, validated here) -> per query the matching documents and scores,
// ordered (0 docno asc, 1 score desc then docno asc) and cut to m: ix->bq
void query_boolean(sme_index *ix, const int32_t *term_ids, const int64_t *g_offsets, const uint8_t *g_flags,
                   const int64_t *q_offsets, int nq, int order, int m, hipStream_t st);
// phrase queries (sme_phrase.hip): np phrases of term ids (host arrays, validated
// here) over the positions a K = 1 build kept -> per phrase the matching documents
// with the phrase's frequency and score, ordered (0 docno asc, 1 score desc then
// docno asc) and cut to m: ix->pq
void query_phrase(sme_index *ix, const int32_t *term_ids, const int64_t *p_offsets, int np, int order, int m,
                  hipStream_t st);
// proximity queries (sme_near.hip): nq queries of term ids with a width and a kind
// each (0 ordered window, 1 unordered; host arrays, validated here) over the same
// positions, through the same pass -> ix->nq
void query_near(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *widths,
                const uint8_t *kinds, int nq, int order, int m, hipStream_t st);
// What narrows a proximity pass (structured queries): pass query i cannot be a
// result outside any of the groups [qgoff[owner[i]], qgoff[owner[i] + 1]), group g
// being the union of the posting lists of terms[goff[g] .. goff[g + 1]) (-1: an
// empty list).  Host arrays; at most kNarrowGroups groups and kNarrowSlots slots
// per owner (what the filter stages in LDS).
constexpr int kNarrowGroups = 16, kNarrowSlots = 256;
struct NarrowSpec {
  std::vector<int32_t> owner;   // [nq]
  std::vector<int64_t> qgoff;   // [owners + 1]
  std::vector<int64_t> goff;    // [groups + 1]
  std::vector<int32_t> terms;   // [slots]
};
// query_near behind its validation: the batch through the pass into `out`, the
// candidate filter narrowed by `narrow` if given (sme_near.hip)
void near_pass(sme_index *ix, DocFreqScores &out, const int32_t *term_ids, const int64_t *q_offsets,
               const int32_t *widths, const uint8_t *kinds, int nq, int order, int m, const NarrowSpec *narrow,
               hipStream_t st);
// the index's scorer table 1 + ln(f) (d_nq_lut) grown to n entries at least, by the
// build's own expression (sme_near.hip); `st` is synchronised when it grows
void grow_score_lut(sme_index *ix, int64_t n, hipStream_t st);
// relevance feedback (sme_feedback.hip): n sets of docnos (device memory if
// on_device, else a host array; the offsets and the optional exclusion lists: host
// arrays, validated here) over the positions a K = 1 build kept -> per set its kept
// terms with freq, docs and score, by score descending then term ascending, cut to
// m: ix->fb and the fb_ counts
void feedback_terms(sme_index *ix, const int32_t *docnos, bool on_device, const int64_t *f_offsets, int n,
                    const int32_t *x_ids, const int64_t *x_offsets, int m, int min_docs, int min_df, int max_df,
                    hipStream_t st);
// structured queries (sme_structq.hip): nq queries of required / excluded groups of
// leaves -- a term, or an ordered / unordered window over terms (host arrays,
// validated here) -> per query the matching documents and scores, ordered and cut
// as query_boolean's: ix->sq, and ix->sq_leaves
void query_structured(sme_index *ix, const int32_t *term_ids, const int64_t *l_offsets, const uint8_t *l_kinds,
                      const int32_t *l_widths, const int64_t *g_offsets, const uint8_t *g_flags,
                      const int64_t *q_offsets, int nq, int order, int m, hipStream_t st);
// BM25 ranking (sme_bm25.hip): the index's collection tables (document lengths, idf
// by true df, the bound tables), built once; and nq queries of term ids in device
// memory -> per query the k best documents by BM25 score, laid out as query_topk's.
// h_qoff: the offsets' host copy, validated by the caller.
void prepare_bm25(sme_index *ix, hipStream_t st);
void query_topk_bm25(sme_index *ix, const int32_t *d_terms, const int64_t *d_qoff, const int64_t *h_qoff, int nq, int k,
                     double k1, double b, int32_t *d_out_docno, double *d_out_score, hipStream_t st);
// scoring given documents (sme_rescore.hip): nq queries of term slots and strictly
// ascending candidate docnos (the slots and both offset arrays: host arrays,
// validated here; the candidates: device memory with their offsets' device copy if
// on_device, where a kernel checks their order, else a host array) -> per query the
// candidates with hits >= min_hits, their hits and scores (model 0 TF-IDF, 1 BM25),
// ordered (0 as given, 1 score desc then docno asc) and cut to m: ix->rs
void rescore_docs(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *docnos,
                  bool on_device, const int64_t *d_offsets, const int64_t *d_offsets_dev, int nq, int model, double k1,
                  double b, int min_hits, int order, int m, hipStream_t st);
// best passages (sme_passage.hip): nq queries of term ids and strictly ascending
// candidate docnos, given as rescore_docs takes them -> per candidate the best window
// of at most `width` positions of one of its records' streams; the candidates whose
// window covers min_cover distinct query terms or more kept, ordered (0 as given, 1
// score desc then docno asc) and cut to m: ix->pw; with_terms: the kept windows'
// term ids and slots: ix->pwt
void query_passages(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *docnos,
                    bool on_device, const int64_t *d_offsets, const int64_t *d_offsets_dev, int nq, int width,
                    int min_cover, int order, int m, int with_terms, hipStream_t st);
// The idf of a term with document frequency df among N documents, the one
// expression behind the build's idf tables (idf_by_df[df] = idf_value(N, df),
// idf_by_q[q] = idf_value(q, 1) read at q = N / df: log10 of the integer quotient)
// and a phrase's score.  Host only: the
// tables exist because the platform libm's log10 is the reference's.
inline double idf_value(int64_t N, int64_t df) { return log10((double)(N / df)); }
}  // namespace sme
