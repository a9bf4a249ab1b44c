/*
 * sme.h -- C-ABI of the MI355X-native index-build / TF-IDF / query hot path.
 *
 * "sme" = Simple MapReduce Engine.  This library replaces, as one batch call,
 * the reference's whole TermKGramDocIndexer job (map -> shuffle/sort ->
 * combine/reduce) and IntDocVectorsForwardIndex.rank():
 *
 *   sme_build_index*      <- TermKGramDocIndexer.run / MyMapper.map / MyReducer.reduce
 *                            C/sa/edu/kaust/indexing/TermKGramDocIndexer.java:119-160,168-213,227-283
 *   sme_load_docno_mapping<- MyMapper.configure -> TrecDocnoMapping.loadMapping/readDocnoData
 *                            TermKGramDocIndexer.java:93-117; C/edu/umd/cloud9/collection/trec/TrecDocnoMapping.java:75-77,137-155
 *   sme_index_partition_records <- SequenceFileOutputFormat part-NNNNN record stream
 *                            (TermDF.write TermDF.java:50-56, ArrayListWritable.write ArrayListWritable.java:90-105)
 *   sme_tokenize          <- GalagoTokenizer.processContent  C/ivory/tokenize/GalagoTokenizer.java:139-183
 *   sme_lookup_terms      <- IntDocVectorsForwardIndex.getValue(String[]) term lookup
 *                            C/sa/edu/kaust/fwindex/IntDocVectorsForwardIndex.java:131-184
 *   sme_query_topk        <- IntDocVectorsForwardIndex.rank()  IntDocVectorsForwardIndex.java:192-223
 * (C/ = ABDURRAHMAN-PA2-3-code/src/ of the reference; U+2010 hyphens in the real path.)
 *
 * Conventions: every int-returning function returns 0 (SME_OK) on success and
 * a negative SME_E* code on failure; sme_last_error() returns a thread-local
 * message for the last failure.  Inputs are borrowed for the duration of the
 * call; outputs returned through pointers are owned by the library until the
 * owning object is freed.  One sme_ctx per device; calls on one context must
 * be serialized by the caller (the reference's query class is not thread-safe
 * either: IntDocVectorsForwardIndex.java:63-65).
 */
#ifndef SME_H
#define SME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SME_OK 0
#define SME_EINVAL -1    /* bad argument */
#define SME_EHIP -2      /* HIP runtime error */
#define SME_ENOMEM -3    /* device allocation failed */
#define SME_EPARSE -4    /* input the reference rejects (e.g. <DOCNO> without </DOCNO>: getDocid throws) */
#define SME_ENOMAP -5    /* no docno mapping loaded */
#define SME_ELIMIT -6    /* an implementation limit was hit (message says which) */
#define SME_ENOTIMPL -7  /* feature not built yet (message says which) */

/* idf_mode */
#define SME_IDF_REFERENCE 0 /* log10(N / stored_df); stored df of every real term is 1 */
#define SME_IDF_TRUE_DF 1   /* log10(N / df) with df = postings length, int division as the reference */

/* tiebreak */
#define SME_TIE_DOCNO 0     /* score desc, then docno asc (north-star contract) */
#define SME_TIE_REFERENCE 1 /* score desc, then the reference's printed order: rank() appends
                               candidates in first-encounter order (query token order, each term's
                               postings tf desc / docno asc) and Collections.sort over DocScore
                               (IntDocVectorsForwardIndex.java:195-215,363-365) is a stable sort by
                               score desc (its merge sort only asks compareTo <= 0 / > 0, which is
                               score order for finite scores), so equal scores keep that order */
#define SME_TIE_JAVA7 2     /* rank()'s list as a Java 7 JVM leaves it: Collections.sort is then
                               ComparableTimSort, and DocScore.compareTo = (int)Math.ceil(o.score -
                               score) -- 0 for score gaps in (-1, 0] -- is not a total order, so the
                               whole first-encounter list is sorted by the JDK 7 GA algorithm on the
                               device (one thread per query; a compatibility mode, not the serving
                               path).  A query whose sort Java aborts with IllegalArgumentException
                               ("Comparison method violates its general contract!") gets docno -2
                               in all k slots; tie words are 0xFFFFFFFF (no shard merge) */

typedef struct sme_ctx sme_ctx;
typedef struct sme_index sme_index;

typedef struct {
  int k;              /* K of the K-gram index (TermKGramDocIndexer args[0]); 1 = term index */
  int num_partitions; /* R reducers (conf.setNumReduceTasks(10) on the cluster, 1 in local mode) */
  int idf_mode;       /* SME_IDF_* used by the TF-IDF weight pass and sme_query_topk */
  int tiebreak;       /* SME_TIE_* */
  int device;         /* HIP device ordinal */
  int reserved[11];   /* must be zero */
} sme_config;

const char *sme_last_error(void);
const char *sme_version(void);

/* Device-memory plumbing for hosts without a HIP binding of their own (a JNI /
 * ctypes host passing d_df_global to sme_index_reweight, or reading a device
 * corpus back): allocation on `device`, and a copy in any direction
 * (hipMemcpyDefault; stream NULL = synchronous).  They run on the library's own
 * HIP runtime, so pointers from it and to it always agree. */
int sme_device_alloc(int device, size_t n, void **d);
void sme_device_free(void *d);
int sme_memcpy(void *dst, const void *src, size_t n, void *stream);

int sme_create(const sme_config *cfg, sme_ctx **out);
void sme_destroy(sme_ctx *ctx);

/* Path options of a context (no reference counterpart: the reference has one
 * code path).  Every value gives bit-identical results; the options exist so
 * tests can hold each device path to the others and benches can sweep them.
 *   "query_kernel"  0 window-major scoring with seeded thresholds (default), 1 streaming
 *                   k_query, 2 per-query block-max sweep k_query_bm
 *   "heavy_div"     heavy tf / impact rows for terms with df >= docno span / div (default 128; 0 none)
 *   "seed_m"        seed postings per term for the window path's threshold, 0..4096 (default 64)
 *   "cand_cap"      candidate list per query of the window path, 1..2048 (default 1024; >= 1024:
 *                   at least 16 k)
 *   "win_sample"    1 (default): sample windows first, thresholds raised, then the rest
 *   "win_stage_min" windows of the first sampled stage, at least (default 0 = auto: 16, or 8
 *                   for indexes of >= 1024 windows of 4096 documents; the stage count
 *                   follows, at most 9)
 *   "win_slice"     queries per window-path workgroup slice (default 0 = auto: 128, or 256 for
 *                   indexes of >= 1024 windows)
 *   "seed_tiles"    k_query_bm: best-bound tiles scored before the sweep, 0..8 (default 4)
 *   "query_order"   1 heaviest-term query order (default), 0 batch order
 *   "agg_two_pass"  1 count + emit aggregation passes (default 0: single pass)
 *   "kgram_rank"    1: K >= 2 gram keys by iterated ranking (the path of K * ceil(log2 V) > 63)
 *                   even when the packed term ids fit 64 bits (default 0: automatic)
 *   "agg_grid"      aggregation workgroups, 0 = auto (default 0)
 *   "tok_grid"      tokenizer workgroups, >= 1 (default 5120)
 *   "raw_load_pct"  raw-vocabulary table load of the next build, 10..90 (default 40)
 *   "docid_terms"   1 (default): a record's DOCNO token that is its own term (ASCII letters and
 *                   digits ending in a digit, unchanged by the stemmer) skips the per-distinct
 *                   vocabulary work and is ranked by a merge with the sorted word terms when the
 *                   docids ascend in file order; 0: every raw token through the general path
 *   "sort_digit_bits"  most bits per digit of the term sort's LSD passes, 6..11, or 0 (default:
 *                   11 -- two passes for up to 2^22 terms -- and 8 past 2^30 pairs)
 *   "term_off_tables"  1 (default): the CSR offsets are read out of the term sort's own offset
 *                   tables, and its last pass stores the sorted keys only when a later step reads
 *                   them (the df idf modes, a tf above 1023); 0: the keys are always stored and the
 *                   offsets found by a pass over them
 *   "docid_split"   1 (default): with docid terms (K4b) that push the term ids past 22 bits
 *                   while the word terms need fewer, each record's docid pair is kept beside
 *                   the sort of word-rank keys and merged into the CSR after it; 2: whenever
 *                   the word ranks need fewer bits than the merged ids; 0: one sort of all
 *                   pairs by merged id
 *   "query_table_budget"  bytes a batch's skip table may take (default 0 =
 *                   a quarter of the free HBM); a batch over it is split by
 *                   query range, and queries still overflowing their
 *                   candidate lists whose tile table does not fit run as their
 *                   own compact batch -- every batch of queries of <= 64 terms
 *                   is answered by the window-major scorer, for any k <= 448
 *   "corpus_keep_bytes"  sme_build_index keeps its device copy of the host
 *                   corpus for the next build (no hipMalloc) only up to this
 *                   many bytes (default 16 GiB); larger copies are freed after
 *                   the build, since HBM held there also shrinks the heavy-row
 *                   budget of sme_index_prepare_queries (1/4 of free HBM)
 *   "wild_scan"     wildcard expansion: 0 (default) candidates from the trigram table, 1 every
 *                   pattern takes the whole vocabulary as candidates
 *   "wild_chunk"    wildcard candidates per workgroup, 64..4096 in multiples of 64 (default 1024);
 *                   spelling suggestions cut their candidates by the same option
 *   "fuzzy_scan"    spelling suggestions: 0 (default) candidates from the trigram table, 1 every
 *                   word takes the whole vocabulary as candidates
 *   "bool_chunk"    Boolean-query candidates per workgroup, 64..4096 in multiples of 64 (default 1024)
 *   "bool_driver"   Boolean queries: 0 (default) the required group with the fewest postings
 *                   supplies the candidates, 1 the first required group
 *   "positions"     0 (default): nothing is kept; 1: a K = 1 sme_build_index* also keeps every
 *                   record's term stream with the index (sme_index_positions), which phrase
 *                   queries (sme_query_phrase) need.  Every other output of the build is the
 *                   same bytes; "bool_chunk" also cuts a phrase query's candidates
 *   "struct_narrow" structured queries (sme_query_structured): 1 (default) a query's required
 *                   term-only groups cut its operator leaves' candidates before their records
 *                   are scanned, 0 every leaf is evaluated whole.  Results are the same
 *   "fb_slots"      relevance feedback (sme_index_feedback_terms): entries of the on-chip term
 *                   table of one document set, a power of two in 16..4096 (default 4096, 48 KiB
 *                   of LDS: two workgroups fit a CU); a set with more than 3/4 of that many
 *                   distinct terms takes the large path.  Results are the same
 *   "merge_tile"    sme_index_merge: docno-order postings per tile of its n-way merge, a multiple
 *                   of 64 in 64..2048 (default 1024: 26 KiB of LDS per workgroup).  Results are
 *                   the same
 *   "delete_tile"   sme_index_delete_docnos: postings per tile of its compaction of the two posting
 *                   orders, a multiple of 256 in 256..65536 (default 16384; a workgroup takes 12 KiB
 *                   of LDS whatever the tile).  Results are the same
 *   "merge_append"  sme_index_merge: 1 (default) inputs whose docno ranges are pairwise disjoint
 *                   are laid end to end without merging, 0 every call takes the general merge.
 *                   Results are the same
 *   "bm25_split"    sme_query_topk_bm25*: scorer workgroups per query, 0 (default) automatic,
 *                   >= 1 that many (capped at the window count and at 4096).  Results are the same
 *   "rescore_path"  sme_query_rescore*: how a term slot meets a tile of candidates, 0 (default)
 *                   the cheaper form by the two lengths, 1 always a search of the term's list
 *                   per candidate, 2 always a scan of the list against the tile.  Results are the same
 * Unknown names and out-of-range values are SME_EINVAL. */
int sme_set_option(sme_ctx *ctx, const char *name, int64_t value);

/* Docno mapping file bytes: int32 N, then N x writeUTF(docid), docids sorted
 * (TrecDocnoMapping.writeDocnoData format).  Uploaded once; docno lookup is
 * Arrays.binarySearch over {"", docids...} on the device. */
int sme_load_docno_mapping(sme_ctx *ctx, const uint8_t *mapping_file, size_t n);

/* Docno assignment (NumberTrecDocuments.run + TrecDocnoMapping.writeDocnoData,
 * C/edu/umd/cloud9/collection/trec/NumberTrecDocuments.java:82-168,
 * TrecDocnoMapping.java:92-125): the distinct docids of the corpus's records in
 * UTF-8 byte order, numbered 1.., as the mapping FILE BYTES (int32 N, N x
 * writeUTF(docid)) that sme_load_docno_mapping takes.  *mapping is owned by ctx
 * until its next call. */
int sme_number_documents(sme_ctx *ctx, const uint8_t *corpus, size_t nbytes, const uint8_t **mapping, size_t *n);

/* Doc-shard cut points for `world` shards: cuts[0] = 0, cuts[world] =
 * nbytes, and cuts[g] = the first record start at or after nbytes * g / world,
 * i.e. shard g holds the records a Hadoop split [n g/W, n (g+1)/W) owns
 * (XMLInputFormat.java:110-143,173-198: a record belongs to the split its <DOC>
 * match begins in), found by one record-reader pass over the whole input so a
 * shard built from [cuts[g], cuts[g+1]) has exactly the single reader's records.
 * cuts: world + 1 host entries. */
int sme_split_points(sme_ctx *ctx, const uint8_t *corpus, size_t nbytes, int world, uint64_t *cuts);
int sme_split_points_device(sme_ctx *ctx, const void *d_corpus, size_t nbytes, int world, void *stream,
                            uint64_t *cuts);

/* Build from a host corpus (TREC <DOC>..</DOC> records, one split). Copies to HBM. */
int sme_build_index(sme_ctx *ctx, const uint8_t *corpus, size_t nbytes, sme_index **out);

/* Build from a corpus already resident in device memory (d_corpus on ctx's
 * device, nbytes long); stream may be NULL (default stream).  No host copies
 * of the corpus are made; this is the timed path of bench.py. */
int sme_build_index_device(sme_ctx *ctx, const void *d_corpus, size_t nbytes, void *stream,
                           sme_index **out);

/* CharKGramTermIndexer (C/sa/edu/kaust/indexing/CharKGramTermIndexer.java:74-211, the
 * other PA2-3 job): k = cfg.k (1..5) character k-grams of every '$'+token+'$', each
 * mapped to the set of tokens containing it (JDK 6 HashSet iteration order), written
 * as TextOutputFormat lines "gram\t[t1, t2, ...]\n" into cfg.num_partitions
 * HashPartitioner partitions in Text key order.  One split (one map task); no docno
 * mapping is needed (the job's mapper never reads docids).  The result is an
 * sme_index whose only accessors are the two below and sme_index_free. */
int sme_build_chargram(sme_ctx *ctx, const uint8_t *corpus, size_t nbytes, sme_index **out);
int sme_build_chargram_device(sme_ctx *ctx, const void *d_corpus, size_t nbytes, void *stream,
                              sme_index **out);
/* part-NNNNN text bytes of reduce partition `part` (host buffer owned by the index) */
int sme_chargram_partition_text(sme_index *ix, int part, const uint8_t **buf, size_t *n);
/* distinct k-grams (output lines) and (k-gram, token) set entries */
int sme_chargram_stats(const sme_index *ix, uint64_t *ngrams, uint64_t *npairs);

/* Open an index from its reduce-output record streams -- the step between the
 * reference's two programs: TermKGramDocIndexer writes part-NNNNN SequenceFiles,
 * IntDocVectorsForwardIndex opens them later (C/sa/edu/kaust/fwindex/
 * BuildIntDocVectorsForwardIndex.java:84-158, IntDocVectorsForwardIndex.java:93-184).
 * records = nparts partition streams laid back to back, part_offsets = nparts + 1
 * host entries from 0, non-decreasing, the last one the byte count.  A stream
 * is what sme_index_partition_records returns (int32 recLen, int32 keyLen,
 * TermDF bytes, ArrayListWritable<PostingWritable> bytes; big-endian), and where
 * a record would start, recLen == -1 followed by 16 bytes is a SequenceFile sync
 * escape and is skipped: the bytes of a part file after its header load as they
 * are (seqfile.read_part_body), with no per-record work on the host.
 * nparts need not be cfg.num_partitions: the terms are merged into one TermDF
 * order and the index serializes into cfg.num_partitions partitions.
 * The result is the index sme_build_index returns for the corpus behind the
 * records (vocabulary, both posting orders, fp64 weights, query side), with two
 * differences: the " " doc counter never holds a map task's last docno
 * (TermKGramDocIndexer.java:84-90,126), so the record is kept as its postings --
 * serialization gives it back byte for byte -- and sme_index_record_docnos /
 * sme_index_pack_pieces return SME_EINVAL.
 * K = 1 only: cfg.k != 1, or a key whose component count is not 1, is
 * SME_ENOTIMPL ("loading K >= 2 record streams"), decided before any per-term
 * work.  Nothing in the input is trusted: every length is checked against its
 * partition's end before a dependent read, and a malformed stream is SME_EPARSE
 * with a message naming the first problem and its place (a record past its
 * partition's end, keyLen or recLen inconsistent, a value class other than
 * sa.edu.kaust.io.PostingWritable, key bytes writeUTF does not write, keys not
 * strictly ascending in a partition or held by two, a stored df other than 1 /
 * the " " posting count, no or several " " records, tf <= 0, postings out of
 * (tf desc, docno asc) order, a docno twice in a term, " " postings other than
 * (0,0) / (docno,1) lists); a term frequency >= 2^24 is SME_ELIMIT.
 * sme_last_build_profile then holds the loader's stages (scan_candidates,
 * scan_records, keys, merge_terms, postings, docno_order, weights, total).
 * The host entry copies to HBM and calls the device entry (stream NULL =
 * default stream; d_records on ctx's device). */
int sme_index_from_records(sme_ctx *ctx, const uint8_t *records, const uint64_t *part_offsets, int nparts,
                           sme_index **out);
int sme_index_from_records_device(sme_ctx *ctx, const void *d_records, const uint64_t *part_offsets, int nparts,
                                  void *stream, sme_index **out);

void sme_index_free(sme_index *ix);

/* N = records mapped (= df of the " " doc-counter key), V = distinct terms
 * (K-grams when K > 1) excluding the doc counter, P = postings (distinct
 * (term, docno)).  K > 1 needs K * ceil(log2(distinct terms)) <= 63. */
int sme_index_stats(const sme_index *ix, uint64_t *N, uint64_t *V, uint64_t *P);

/* Serialized records of reduce partition `part` in key order, framed as in a
 * SequenceFile body: int32 recLen(key+value), int32 keyLen, TermDF bytes,
 * ArrayListWritable<PostingWritable> bytes (all big-endian).  The buffer lives
 * on the host and is owned by ix. */
int sme_index_partition_records(sme_index *ix, int part, const uint8_t **buf, size_t *n);

/* The device half of the same output (the serializer kernels k_ser_*, run once
 * per index): part_offsets (R+1 host entries, may be NULL) gets the byte offset
 * of every partition in the concatenated record stream (partition order), and
 * *device_ms (may be NULL) the serializer's device time.  Replaces the reduce
 * tasks' record writes, TermKGramDocIndexer.java:275 (SequenceFileOutputFormat)
 * + TermDF.java:50-56 + ArrayListWritable.java:90-105. */
int sme_index_serialize(sme_index *ix, uint64_t *part_offsets, float *device_ms);

/* Copy the record bytes of partition `part` (part = -1: every partition, back
 * to back in partition order) from HBM into caller memory dst of cap bytes;
 * *n gets the bytes written.  Pinned dst (hipHostMalloc / hipHostRegister,
 * e.g. a pinned direct ByteBuffer) is one DMA; pageable dst goes through the
 * context's pinned staging buffers.  No intermediate host copy is kept. */
int sme_index_copy_records(sme_index *ix, int part, void *dst, size_t cap, size_t *n);

/* Host copies of the CSR in reduce-output order (tf desc, docno asc) over
 * terms in TermDF key order.  offsets has V+1 entries; true_df has V. */
int sme_index_csr(sme_index *ix, const int64_t **offsets, const int32_t **docno,
                  const int32_t **tf, const int32_t **true_df);

/* Device pointers of the query-side arrays (docno-ascending postings per term
 * and their fp64 TF-IDF weights), for callers that keep data in HBM. */
int sme_index_device_arrays(sme_index *ix, const int64_t **d_offsets, const int32_t **d_docno,
                            const double **d_weight);

/* Term string of index term t (modified-UTF-8 bytes as written by writeUTF);
 * for K > 1 (t is a k-gram) its first element k_gram[0], the forward-index key. */
int sme_index_term(sme_index *ix, int64_t t, const uint8_t **utf8, size_t *n);

/* GalagoTokenizer.processContent on one UTF-8 string, run through the same
 * device kernels as the build.  Tokens (modified UTF-8) are written back to back
 * into buf; offs[i]..offs[i+1] delimits token i (offs has cap_tok+1 entries). */
int sme_tokenize(sme_ctx *ctx, const uint8_t *utf8, size_t n, uint8_t *buf, size_t cap,
                 int64_t *offs, int cap_tok, int *ntok);

/* Map processed terms (UTF-8, offs delimits n terms) to index term ids; -1 if
 * absent (getValue skips unknown terms silently).  For K > 1 a term maps to the
 * LAST k-gram (TermDF order) starting with it, as the forward index's Hashtable
 * keeps it (IntDocVectorsForwardIndex.java:107-120). */
int sme_lookup_terms(sme_index *ix, const uint8_t *terms, const int64_t *offs, int n,
                     int32_t *term_ids);

/* Wildcard term expansion (no reference counterpart: the reference's character
 * k-gram job, CharKGramTermIndexer, writes its gram -> term sets to text and no
 * program reads them).  A pattern is matched against whole term strings, UTF-16
 * unit by unit as String.compareTo sees them: '*' matches any run of units,
 * none included; '?' exactly one unit (a supplementary character needs "??");
 * every other unit itself.  No escape syntax and no case folding.  patterns /
 * offs delimit n UTF-8 patterns on the host as sme_lookup_terms takes terms;
 * malformed UTF-8 is SME_EINVAL (the message names the pattern's index), a
 * pattern of more than 255 units SME_ELIMIT.  Pattern i's matches are
 * term_ids[match_off[i] .. match_off[i + 1]), ascending (TermDF order); n + 1
 * offsets, ids back to back, owned by the index until the next expansion on it
 * (host memory from the host entry; device memory from the device entry, ready
 * to be spliced into a sme_query_topk_device batch, with *total = match_off[n],
 * total may be NULL).  n == 0 is valid; 2^31 or more matches in a batch are
 * SME_ELIMIT.  Candidates come from a character-trigram table of the vocabulary
 * (windows of three over START + units + END; a pattern's windows lie inside its
 * literal runs) and every candidate is verified against the term's own units, so
 * a pattern without a trigram ("*a*", "?b", "*", "") scans the vocabulary.  The
 * table is built once per index, on first use or by sme_index_prepare_wildcards
 * (*ms, may be NULL: its device time); it depends on the vocabulary only, so
 * sme_index_reweight leaves it alone, and its HBM (8 B per distinct trigram, 4 B
 * per (trigram, term) pair) stays held until the index is freed, so it counts
 * against the heavy-row budget of sme_index_prepare_queries.
 * sme_index_wildcard_stats (builds the table if needed): distinct trigram keys
 * and distinct (key, term) pairs.  K = 1 term indexes only: a chargram output, a
 * records-only merged index or K != 1 is SME_EINVAL (the message says which). */
int sme_index_prepare_wildcards(sme_index *ix, void *stream, float *ms);
int sme_index_wildcard_stats(sme_index *ix, uint64_t *ngrams, uint64_t *npairs);
int sme_index_expand_wildcards(sme_index *ix, const uint8_t *patterns, const int64_t *offs, int n,
                               const int64_t **match_off, const int32_t **term_ids);
int sme_index_expand_wildcards_device(sme_index *ix, const uint8_t *patterns, const int64_t *offs, int n,
                                      void *stream, const int64_t **d_match_off, const int32_t **d_term_ids,
                                      int64_t *total);

/* Spelling suggestions (no reference counterpart: a word sme_lookup_terms does
 * not know comes back -1 and getValue drops it silently).  words / offs delimit n
 * UTF-8 words on the host as sme_index_expand_wildcards takes patterns, decoded
 * by the same strict decoder: malformed UTF-8 is SME_EINVAL (the message names
 * the word's index).  No unit is a metacharacter here ('*' and '?' are ordinary
 * units) and there is no case folding.  A word has at most 64 UTF-16 units; more
 * is SME_ELIMIT (the message names the word).  The distance is Levenshtein's over
 * UTF-16 units as String sees them: insert, delete, substitute one unit at cost 1
 * each, no transposition; a supplementary character is two units.  max_dist is
 * 0..3 and m >= 0, anything else SME_EINVAL; max_dist == 0 agrees with
 * sme_lookup_terms.  Word i's result is the terms t with dist(word i, t) <=
 * max_dist, ordered by (distance asc, df desc, term id asc) -- df the term's
 * posting count (true_df of sme_index_csr) -- and cut to its first m entries
 * (m == 0: no cut): term_ids[sug_off[i] .. sug_off[i + 1]), dist[] parallel to
 * term_ids[], n + 1 offsets, owned by the index until the next suggestion call on
 * it (host memory from the host entry; device memory from the device entry, with
 * *total = sug_off[n], total may be NULL).  n == 0 is valid; 2^31 or more matches
 * in a batch BEFORE the cut are SME_ELIMIT.  Candidates come from the wildcard
 * trigram table (built on first use by this call or by
 * sme_index_prepare_wildcards; sme_index_reweight leaves it alone): a term within
 * distance d of a word misses at most 3d of the word's distinct windows, so the
 * union of the posting lists of the 3d + 1 distinct windows with the shortest
 * lists holds every match, and a word with fewer distinct windows (short words,
 * the empty word) takes the whole vocabulary; every candidate is verified by a
 * bit-parallel edit distance, so the candidate source never changes a result.  A
 * suggestion call leaves the buffers of the last wildcard expansion alone, and
 * the other way round.  sme_index_suggest_stats reports on the last suggestion
 * call on the index: the words that took the whole vocabulary as candidates, and
 * the (word, term) pairs that reached the length test.  K = 1 term indexes only,
 * refused as the wildcard entry points refuse (SME_EINVAL, the message says
 * which); indexes opened with sme_index_from_records work. */
int sme_index_suggest_terms(sme_index *ix, const uint8_t *words, const int64_t *offs, int n, int max_dist, int m,
                            const int64_t **sug_off, const int32_t **term_ids, const uint8_t **dist);
int sme_index_suggest_terms_device(sme_index *ix, const uint8_t *words, const int64_t *offs, int n, int max_dist,
                                   int m, void *stream, const int64_t **d_sug_off, const int32_t **d_term_ids,
                                   const uint8_t **d_dist, int64_t *total);
int sme_index_suggest_stats(const sme_index *ix, uint64_t *scanned_words, uint64_t *candidates);

/* Boolean retrieval (no reference counterpart: rank() is one disjunctive sum over
 * a flat term list).  A query is a list of groups, a group a list of term ids
 * plus one flag: query i's groups are [q_offsets[i], q_offsets[i + 1]) (nq + 1
 * entries from 0), group g's term slots term_ids[g_offsets[g] .. g_offsets[g + 1])
 * (ngroups + 1 entries from 0, ngroups = q_offsets[nq]) and its flag g_flags[g];
 * all host arrays.  A document matches a query when
 *   - for every REQUIRED group (flag 0) it lies in at least one of the group's
 *     posting lists: OR inside a group, AND across groups;
 *   - for every EXCLUDED group (flag 1) it lies in none of them.
 * Term id -1 is an unknown term, an empty list, as in sme_query_topk; an id
 * outside [-1, V) is SME_EINVAL (the message names the query).  A required group
 * without a posting therefore matches nothing, and so does a query without a
 * required group -- the empty query, or exclusions only: pure negation is not
 * offered.  A term in both a required and an excluded group contributes nothing
 * to the result.  For K >= 2 the ids are k-gram ids.
 * The score of a matching document is the fp64 sum, starting from 0.0, of its
 * weight (sme_index_device_arrays' d_weight at the document's posting) over
 * every term slot of every required group in listed order -- groups in order,
 * slots in order within a group; a slot whose list does not hold the document
 * adds nothing, a term listed twice counts twice, excluded slots add nothing.
 * That is the sum rank() forms for the flat list of the required slots, so the
 * score has the bits sme_query_topk gives the same document for that list.  The
 * weights are read at call time (a call after sme_index_reweight uses the new
 * ones).  order 0: a query's results by docno ascending (signed int32 order, as
 * the postings are kept); order 1: by score descending, then docno ascending;
 * both then cut to the first m entries (m == 0: no cut).  Query i's results are
 * docno[] / score[] at [res_off[i], res_off[i + 1]); nq + 1 offsets, owned by the
 * index until the next Boolean call on it (host memory from the host entry;
 * device memory from the device entry, with *total = res_off[nq], total may be
 * NULL).  A Boolean call leaves the buffers of the last wildcard expansion and
 * suggestion call alone, and the other way round.  nq == 0 is valid.
 * Limits: more than 64 groups or more than 1024 term slots in a query are
 * SME_ELIMIT (the message names the query), as are 2^31 or more term slots in
 * a batch and 2^31 or more matches in a batch BEFORE the cut.  q_offsets and
 * g_offsets are never NULL when nq > 0; g_flags and term_ids may be NULL only
 * in a batch without a group (q_offsets[nq] == 0) -- a NULL array otherwise is
 * SME_EINVAL, also when every group of the batch is empty.  m < 0, an order other than 0 / 1, offsets that do not
 * ascend from 0 or do not agree with each other, and a flag other than 0 / 1
 * are SME_EINVAL.  An index without a query side (a chargram output, a
 * records-only merged index) is SME_EINVAL, as the query entry points refuse.
 * Candidates come from one required group, the driver: the one with the fewest
 * postings, ties to the first ("bool_driver" 1: the first required group); every
 * candidate is tested against all other groups by binary searches, so the
 * driver never changes a result.  sme_query_boolean_stats reports on the last
 * Boolean call on the index: the driver postings examined over all queries that
 * could match (a query that matches nothing by the rules above adds none), and
 * the matches before the cut. */
int sme_query_boolean(sme_index *ix, const int32_t *term_ids, const int64_t *g_offsets, const uint8_t *g_flags,
                      const int64_t *q_offsets, int nq, int order, int m, const int64_t **res_off,
                      const int32_t **docno, const double **score);
int sme_query_boolean_device(sme_index *ix, const int32_t *term_ids, const int64_t *g_offsets,
                             const uint8_t *g_flags, const int64_t *q_offsets, int nq, int order, int m, void *stream,
                             const int64_t **d_res_off, const int32_t **d_docno, const double **d_score,
                             int64_t *total);
int sme_query_boolean_stats(const sme_index *ix, uint64_t *candidates, uint64_t *matches);

/* Positions: what a K = 1 index built with option "positions" 1 keeps beside its
 * postings -- per record, in docno-ascending record order, the term ids
 * (sme_lookup_terms' ids) of its tokens in token order, after stop-wording,
 * stemming and the expansion of tokens that give several terms, the DOCNO's
 * tokens included: a forward index.  Records that share a docno (duplicate
 * docids, docno 0 of records without DOCNO, the negative docnos of docids missing
 * from the mapping) stay separate records.  *records = stream records, *positions
 * = term positions over all of them, *bytes = device memory they take; all three
 * 0 for an index that keeps none: one built without the option or with K >= 2, a
 * chargram output, and every index from sme_index_from_records* or
 * sme_merge_pieces.  A K = 1 index with a query side that keeps none gets them
 * from a positions file (sme_index_attach_positions, below); sme_index_merge
 * carries its inputs' over, sme_index_delete_docnos those of the surviving records. */
int sme_index_positions(const sme_index *ix, uint64_t *records, uint64_t *positions, uint64_t *bytes);

/* Phrase queries (no reference counterpart; the reference answers a phrase of m
 * terms from a second index built with K = m).  Phrase i is the term ids
 * term_ids[p_offsets[i] .. p_offsets[i + 1]) (np + 1 entries from 0), L of them;
 * host arrays.  Document d matches with freq = the number of pairs (record r with
 * docno d, start s) such that s + L <= the length of r's term stream and
 * stream_r[s + j] == phrase[j] for every j < L.  Overlapping occurrences all
 * count ("a a" in "a a a": 2), an occurrence never crosses a record's end, and
 * freq sums over all records of the docno.  That is the posting (d, freq) of the
 * gram in the reference's K = L index of the same corpus.  A phrase holding id
 * -1 (an unknown term) and an empty phrase have no result; an id outside [-1, V)
 * is SME_EINVAL, more than 32 terms SME_ELIMIT (both messages name the phrase).
 * score = (1 + ln freq) * idf(df), one fp64 product, with df = the phrase's
 * matching documents BEFORE the cut and idf the expression of the index's weights
 * (log10(N / 1) in SME_IDF_REFERENCE, log10(N / df) with the integer quotient
 * otherwise; N as of the last sme_index_reweight, the df always this index's
 * own): the bits of d_weight at the gram's posting in a K = L index built by a
 * context with the same settings.  order 0: a phrase's results by docno ascending
 * (signed int32 order); order 1: by score descending, then docno ascending; both
 * then cut to the first m entries (m == 0: no cut).  Phrase i's results are
 * docno[] / freq[] / score[] at [res_off[i], res_off[i + 1]); np + 1 offsets,
 * owned by the index until the next phrase call on it (host memory from the host
 * entry; device memory from the device entry, with *total = res_off[np], total
 * may be NULL).  A phrase call leaves the buffers of the last wildcard, suggestion
 * and Boolean call alone, and the other way round.  np == 0 is valid.
 * Limits: 2^31 or more term slots in a batch, and 2^31 or more documents holding
 * all terms of their phrase over a batch (BEFORE positions are looked at and
 * before the cut) are SME_ELIMIT.  p_offsets is never NULL when np > 0; term_ids
 * may be NULL only in a batch without a term.  m < 0, an order other than 0 / 1
 * and offsets that do not ascend from 0 are SME_EINVAL.  SME_EINVAL, with a
 * message that says which, is also: an index without positions (see
 * sme_index_positions), one with K != 1, one without a query side, a chargram
 * output.
 * Candidates come from the phrase's term with the fewest postings; each is tested
 * against the posting lists of the phrase's other distinct terms, and the
 * survivors' records are scanned.  sme_query_phrase_stats reports on the last
 * phrase call on the index: *candidates = the driver postings examined,
 * *verified = the (phrase, document) pairs that hold all the phrase's terms and
 * had their records scanned, *matches = those with freq > 0, the matches before
 * the cut. */
int sme_query_phrase(sme_index *ix, const int32_t *term_ids, const int64_t *p_offsets, int np, int order, int m,
                     const int64_t **res_off, const int32_t **docno, const int32_t **freq, const double **score);
int sme_query_phrase_device(sme_index *ix, const int32_t *term_ids, const int64_t *p_offsets, int np, int order,
                            int m, void *stream, const int64_t **d_res_off, const int32_t **d_docno,
                            const int32_t **d_freq, const double **d_score, int64_t *total);
int sme_query_phrase_stats(const sme_index *ix, uint64_t *candidates, uint64_t *verified, uint64_t *matches);

/* Proximity queries: "these terms near each other" (Galago's #od:N and #uw:N; no
 * reference counterpart, a K-gram index only knows adjacency).  Query i is the term
 * ids term_ids[q_offsets[i] .. q_offsets[i + 1]) (nq + 1 entries from 0; at most
 * 32, sme_lookup_terms' ids, -1 = unknown), a width N = widths[i] (1 <= N <=
 * 2^31 - 1) and a kind kinds[i]; host arrays.  Everything is evaluated inside one
 * record's term stream (sme_index_positions): nothing crosses a record's end, and
 * freq of a document sums over all records of its docno, as for phrases.
 *
 * Kind 0, the ordered window (#od:N).  For terms t_0 .. t_{L-1} define over the
 * positions p of a record:
 *   R_0[p]      iff stream[p] == t_0;
 *   R_{j+1}[p]  iff stream[p] == t_{j+1} and R_j[q] for some q in [p - N, p - 1].
 * freq = the number of positions p with R_{L-1}[p]: the distinct END positions of
 * chains in which every next term follows the previous one by at most N
 * positions.  This is existence over all chains, not a greedy match: in
 * "a b b x c" with N = 2 the chain through the second b reaches c (the one through
 * the first does not), in "a b c b" with N = 3 the chain through the first b
 * reaches c (the one through the last does not); both match.  Repeated terms are
 * ordinary ("a a").  N = 1 is the exact phrase with sme_query_phrase's freq (ends
 * and starts correspond one to one); L = 1 gives the term's tf.
 *
 * Kind 1, the unordered window (#uw:N).  The query is the SET T of its distinct
 * terms (a term listed twice counts once).  freq = the number of positions e with
 * stream[e] in T and every term of T occurring in [max(0, e - N + 1), e]: the
 * window of N positions ending at a query term holds all of them.  N < |T|
 * matches nothing; a window is clipped at the record's start, never continued into
 * the previous record.
 *
 * Both kinds: an empty query and a query holding -1 have no result.  score =
 * (1 + ln freq) * idf(df), one fp64 product, with df = the query's matching
 * documents BEFORE the cut and idf and N_docs exactly as sme_query_phrase uses
 * them (log10(N / 1) in SME_IDF_REFERENCE, log10(N / df) with the integer quotient
 * otherwise; N as of the last sme_index_reweight).  1 + ln f comes from a table
 * kept with the index that continues the weights' own past the largest tf: an
 * unordered freq can reach the sum of the distinct terms' tfs.  order 0: a query's
 * results by docno ascending (signed int32 order); order 1: by score descending,
 * then docno ascending; both then cut to the first m entries (m == 0: no cut).
 * Query i's results are docno[] / freq[] / score[] at [res_off[i], res_off[i + 1]);
 * nq + 1 offsets, owned by the index until the next proximity call on it (host
 * memory from the host entry; device memory from the device entry, with *total =
 * res_off[nq], total may be NULL).  A proximity call leaves the buffers of the
 * last wildcard, suggestion, Boolean and phrase call alone, and the other way
 * round.  nq == 0 is valid.
 * Limits: more than 32 terms in a query is SME_ELIMIT, as are 2^31 or more term
 * slots in a batch and 2^31 or more documents holding all terms of their query
 * over a batch (before positions are looked at).  A term id outside [-1, V), a
 * width below 1 and a kind other than 0 / 1 are SME_EINVAL; every one of these
 * messages names the query.  q_offsets, widths and kinds are never NULL when
 * nq > 0; term_ids may be NULL only in a batch without a term.  m < 0, an order
 * other than 0 / 1 and offsets that do not ascend from 0 are SME_EINVAL, as is,
 * with a message that says which: an index without positions, one with K != 1, one
 * without a query side, a chargram output.  A freq past the scorer table (the
 * index's tfs and its streams disagreeing) is SME_ELIMIT, never a read past it.
 * Candidates come from the query's term with the fewest postings and are filtered
 * as a phrase's are ("bool_chunk" cuts them); the survivors' records are scanned,
 * every stream word read once whatever the query's length.
 * sme_query_near_stats reports on the last proximity call on the index:
 * *candidates = the driver postings examined, *verified = the (query, document)
 * pairs that hold all the query's terms and had their records scanned, *matches =
 * those with freq > 0, the matches before the cut. */
int sme_query_near(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *widths,
                   const uint8_t *kinds, int nq, int order, int m, const int64_t **res_off, const int32_t **docno,
                   const int32_t **freq, const double **score);
int sme_query_near_device(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *widths,
                          const uint8_t *kinds, int nq, int order, int m, void *stream, const int64_t **d_res_off,
                          const int32_t **d_docno, const int32_t **d_freq, const double **d_score, int64_t *total);
int sme_query_near_stats(const sme_index *ix, uint64_t *candidates, uint64_t *verified, uint64_t *matches);

/* Structured queries: Boolean retrieval whose group members are LEAVES -- a term,
 * or a phrase / window over terms -- so that one call answers and scores a query
 * such as `"new york" hotel* -"times square"` or `#uw:8(network protocol) tcp|udp`.
 * It is sme_query_boolean's three-level structure with one more level below the
 * slot.  Query i's groups are [q_offsets[i], q_offsets[i + 1]); group g's leaves
 * are [g_offsets[g], g_offsets[g + 1]) and its flag is g_flags[g] (0 required, 1
 * excluded); leaf l's term ids are term_ids[l_offsets[l] .. l_offsets[l + 1]), its
 * kind l_kinds[l] and its width l_widths[l].  All host arrays, every offset array
 * ascending from 0.
 *
 * Kind 0, a term: exactly one id.  The leaf's document list is the term's posting
 * list, its value at a document d_weight at that posting; its width is not read;
 * id -1 is an empty list, as in sme_query_boolean.
 * Kind 1, the ordered window #od:N, and kind 2, the unordered window #uw:N, with
 * N = l_widths[l], over 1 to 32 ids: the list is the documents sme_query_near
 * returns for that query (its kind 0 / 1) with its freq, the value the score
 * sme_query_near gives, bit for bit: (1 + ln freq) * idf(df), df the leaf's matching
 * documents over the whole index, idf as the weights form it in the index's idf
 * mode, N_docs as of the last sme_index_reweight.  A phrase is kind 1 with width
 * 1.  An operator leaf without ids, or holding -1, is an empty list.
 *
 * A document matches a query exactly by sme_query_boolean's rules with "posting
 * list" read as "leaf's document list": it lies in at least one list of every
 * required group and in no list of an excluded one; a query without a required
 * group and the empty query match nothing.  Its score is the fp64 sum from 0.0 of
 * the leaves' values at the document over every leaf of every required group in
 * listed order; a leaf listed twice counts twice, a leaf that does not hold the
 * document adds nothing, excluded leaves add nothing.  order 0 / 1 and the cut m
 * are sme_query_boolean's.  So a batch of term leaves only is sme_query_boolean,
 * one required group holding one operator leaf is sme_query_near, and an ordered
 * leaf of one term (any width) has the value of the term leaf.
 * Query i's results are docno[] / score[] at [res_off[i], res_off[i + 1]); nq + 1
 * offsets, owned by the index until the next structured call on it (host memory
 * from the host entry; device memory from the device entry, with *total =
 * res_off[nq], total may be NULL).  A structured call leaves the buffers of the
 * last wildcard, suggestion, Boolean, phrase and proximity call alone, and the
 * other way round.  nq == 0 is valid.
 *
 * A batch of term leaves only needs a query side and nothing else, as
 * sme_query_boolean (loaded indexes, K >= 2).  With any operator leaf in the batch
 * the index must keep positions and have K = 1: otherwise SME_EINVAL with
 * sme_query_near's message for the case.
 * Limits (SME_ELIMIT, the message names the query): more than 64 groups or more
 * than 1024 leaves in a query, more than 32 ids in an operator leaf; also 2^31 or
 * more ids or leaves in a batch, sme_query_near's 2^31 candidate documents over the
 * batch's operator leaves, and 2^31 or more matches in a batch before the cut.
 * SME_EINVAL (the message names the query): a term leaf with other than one id, a
 * kind outside 0 .. 2, an operator width below 1, an id outside [-1, V), a flag
 * other than 0 / 1, offsets at any level that do not ascend from 0 or do not agree
 * with the level above; also m < 0 and an order other than 0 / 1.  q_offsets,
 * g_offsets and l_offsets are never NULL when nq > 0; the other arrays may be NULL
 * only in a batch without a group -- a NULL array otherwise is SME_EINVAL.  Every
 * level's offsets are checked before anything is read through them.
 *
 * Evaluation: the batch's operator leaves go through sme_query_near's pass once
 * (docno order, uncut); the Boolean stage then reads them beside the posting
 * lists, its driver the required group with the fewest entries ("bool_driver",
 * "bool_chunk" as for sme_query_boolean).  Narrowing (option "struct_narrow", on
 * by default): a document outside any required group that holds term leaves only
 * cannot be a result, so an operator leaf of that query -- required or excluded,
 * alone or in an OR group -- is not verified there: its candidates are also tested
 * against those groups (the first 16 of them in listed order, skipping a group
 * that would take the slots past 256) before their records are scanned.  Only in
 * SME_IDF_REFERENCE: in the true-df mode a leaf's score needs its full df, leaves
 * are evaluated whole and the option is ignored.  The results never depend on the
 * option; only *verified does.
 * sme_query_structured_stats reports on the last structured call on the index:
 * *leaves = the operator leaves evaluated, *verified = the (leaf, document) pairs
 * whose records were scanned, *candidates = the Boolean stage's driver entries
 * examined, *matches = the matches before the cut. */
int sme_query_structured(sme_index *ix, const int32_t *term_ids, const int64_t *l_offsets, const uint8_t *l_kinds,
                         const int32_t *l_widths, const int64_t *g_offsets, const uint8_t *g_flags,
                         const int64_t *q_offsets, int nq, int order, int m, const int64_t **res_off,
                         const int32_t **docno, const double **score);
int sme_query_structured_device(sme_index *ix, const int32_t *term_ids, const int64_t *l_offsets,
                                const uint8_t *l_kinds, const int32_t *l_widths, const int64_t *g_offsets,
                                const uint8_t *g_flags, const int64_t *q_offsets, int nq, int order, int m,
                                void *stream, const int64_t **d_res_off, const int32_t **d_docno,
                                const double **d_score, int64_t *total);
int sme_query_structured_stats(const sme_index *ix, uint64_t *leaves, uint64_t *verified, uint64_t *candidates,
                               uint64_t *matches);

/* Relevance feedback: from documents to terms (no reference counterpart).  Given
 * sets of documents, the terms that characterise each set -- the expansion terms
 * of pseudo-relevance feedback (Rocchio), or the query of "more like this" -- from
 * the term streams a K = 1 index keeps (sme_index_positions).  sme_query_topk does
 * the rest.
 * Set i is the docnos docnos[f_offsets[i] .. f_offsets[i + 1]) (nq + 1 entries from
 * 0).  An entry equal to -1 is skipped (sme_query_topk's pad); a docno listed twice
 * counts once; a docno no stream record carries contributes nothing and is no
 * error; ALL records of a docno count (duplicate docids, docno 0 of records
 * without DOCNO, the negative docnos).  More than 1024 entries in a set is
 * SME_ELIMIT (the message names the set).
 * For a term t occurring in the set's records: freq(t) = its occurrences over all
 * of them, docs(t) = the set's distinct docnos whose records hold it -- the posting
 * list of t restricted to the set is {(d, tf)} with sum tf = freq and count = docs.
 * t is KEPT if docs(t) >= min_docs, and min_df <= df(t), and max_df == 0 or df(t) <=
 * max_df -- df(t) the index's own posting count of t -- and t is not among the
 * set's exclusion ids x_ids[x_offsets[i] .. x_offsets[i + 1]) (the original query's
 * terms; host arrays, both NULL for none; -1 excludes nothing; an id outside
 * [-1, V) is SME_EINVAL, the set named).  The streams hold the DOCNO's tokens, terms
 * of df 1 with the highest idf: min_df = 2 removes them.
 * score(t) = (1 + ln freq(t)) * idf(t), one fp64 product of the index's table of
 * 1 + ln f, continued past the largest tf as far as the batch's largest freq, and
 * the idf of t's weights: the weight the index would give t in one document that
 * is the concatenation of the set.  For a set of one docno d it is, bit for bit,
 * d_weight at the posting (t, d).
 * A set's kept terms are ordered by score descending, then term id ascending, and
 * cut to the first m (m == 0: no cut).  Set i's results are term[] / freq[] /
 * docs[] / score[] at [res_off[i], res_off[i + 1]); nq + 1 offsets, owned by the
 * index until the next feedback call on it (host memory from the host entry;
 * device memory from the device entry, with *total = res_off[nq], total may be
 * NULL).  A feedback call leaves the buffers of every other feature's last call
 * alone, and the other way round.  nq == 0 is valid.
 * The host entry takes docnos in host memory.  The device entry takes d_docnos in
 * DEVICE memory -- sme_query_topk_device's [nq, k] output as it stands, pads
 * included, with f_offsets[i] = i * k -- while the offsets and the exclusion lists
 * are host arrays as in the other device entries.
 * Limits (SME_ELIMIT): 2^31 or more entries in a batch; 2^31 or more stream
 * positions in one set (the set named); 2^31 or more (set, term) pairs in a batch --
 * counted as pair slots: min(positions, 3/4 "fb_slots") per set on the on-chip
 * path plus the pairs of the large path; 2^31 or more stream positions in the sets
 * that take the large path.  SME_EINVAL, with a message that says which: m,
 * min_docs, min_df or max_df below 0; offsets that do not ascend from 0; x_ids
 * without x_offsets; an index without positions, one with K != 1, one without a
 * query side, a chargram output.  f_offsets is never NULL when nq > 0; docnos may
 * be NULL only in a batch without an entry.
 * Evaluation: a docno's records are adjacent, so a document is one run of the
 * stream.  A workgroup per set counts the set's terms in an LDS hash table of
 * "fb_slots" entries, document after document; a set with more distinct terms than
 * 3/4 of the table is counted again by the large path -- one key per position, a
 * stable sort, a segmented reduce -- which has no size limit but the ones above.
 * sme_index_feedback_stats reports on the last feedback call on the index:
 * *positions = the stream positions of the sets' documents, *pairs = the (set,
 * term) pairs before the filters, *kept = the pairs after the filters and before
 * the cut, *missing = the distinct docnos of the sets (-1 aside) that no record
 * carries, *spilled = the sets that took the large path. */
int sme_index_feedback_terms(sme_index *ix, const int32_t *docnos, const int64_t *f_offsets, int nq,
                             const int32_t *x_ids, const int64_t *x_offsets, int m, int min_docs, int min_df,
                             int max_df, const int64_t **res_off, const int32_t **term, const int32_t **freq,
                             const int32_t **docs, const double **score);
int sme_index_feedback_terms_device(sme_index *ix, const int32_t *d_docnos, const int64_t *f_offsets, int nq,
                                    const int32_t *x_ids, const int64_t *x_offsets, int m, int min_docs, int min_df,
                                    int max_df, void *stream, const int64_t **d_res_off, const int32_t **d_term,
                                    const int32_t **d_freq, const int32_t **d_docs, const double **d_score,
                                    int64_t *total);
int sme_index_feedback_stats(const sme_index *ix, uint64_t *positions, uint64_t *pairs, uint64_t *kept,
                             uint64_t *missing, uint64_t *spilled);

/* Batched rank(): query q has term ids term_ids[q_offsets[q] .. q_offsets[q+1])
 * in query-token order (duplicates count twice, -1 entries are skipped; an id
 * outside [-1, V) is SME_EINVAL here and skipped like -1 by the device entry).
 * k <= 1792 (SME_ELIMIT above; k > 448 and queries of more than 64 terms take the
 * streaming kernel: up to 1024 terms, 256 in SME_TIE_REFERENCE order).
 * Writes k docnos / scores per query (score desc, docno asc), padded with
 * docno -1 / score 0 when fewer than k documents match. */
int sme_query_topk(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, int nq,
                   int k, int32_t *out_docno, double *out_score);
/* The same plus every result's tie word (see sme_query_topk_device_tie). */
int sme_query_topk_tie(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, int nq,
                       int k, int32_t *out_docno, double *out_score, uint32_t *out_tie);

/* Query-side structures of an index (the role the reference's forward index,
 * BuildIntDocVectorsForwardIndex.java:84-158, plays for rank()): heavy-term tf
 * and impact rows with their block maxima (at most a quarter of the free HBM --
 * counting the device blocks the context holds for reuse --, 64 GB), and one
 * 4-byte window-pass word per posting of the other terms (if 4 B per posting
 * fits a quarter of the free HBM; else the window-major scorer is
 * not used and batches take the block-max path).  Built once per index; the
 * impact rows and their scale depend on idf, so sme_index_reweight DROPS them:
 * call this after the last reweight (sme_query_topk* rebuilds them on first
 * use otherwise, inside that call).  *ms (may be NULL) gets the device time. */
int sme_index_prepare_queries(sme_index *ix, void *stream, float *ms);

/* Same with all arrays already in device memory (timed path). */
int sme_query_topk_device(sme_index *ix, const int32_t *d_term_ids, const int64_t *d_q_offsets,
                          int nq, int k, int32_t *d_out_docno, double *d_out_score, void *stream);

/* The same plus the tie word of every result (d_out_tie[nq * k], 0xFFFFFFFF
 * padding): 0 under SME_TIE_DOCNO; under SME_TIE_REFERENCE (first query token
 * holding the document) << 24 | (2^24 - 1 - its tf).  Results of doc shards
 * merge by (score desc, tie asc, docno asc) into the single index's order
 * (dist.py merge_topk_owner). */
int sme_query_topk_device_tie(sme_index *ix, const int32_t *d_term_ids, const int64_t *d_q_offsets,
                              int nq, int k, int32_t *d_out_docno, double *d_out_score, uint32_t *d_out_tie,
                              void *stream);

/* BM25 ranking.  For an index with a query side (a records-only merged index and
 * a chargram output are SME_EINVAL, as the other query entries refuse them).
 *
 * Collection statistics, from the docno-order postings alone (so a built, a loaded,
 * a merged and a deleted-from index have them alike, and sme_index_reweight does
 * not touch them):
 *   dl[d]   the sum of tf over all postings whose docno is d (an int64 sum stored as
 *           int32; a length that does not fit is SME_ELIMIT): for K = 1 the number of
 *           index terms in the document's records, DOCNO tokens included, for K >= 2
 *           the number of grams.  The " " doc-counter record is no posting list here.
 *   D       the docnos with at least one posting;  L = sum of dl;
 *   avgdl   (double)L / (double)D;
 *   df_t    the postings of term t: the true df, whatever the index's idf mode.
 * Weights, all fp64 in exactly this association (no fused multiply-add):
 *   idf_t   = log(1.0 + ((double)(D - df_t) + 0.5) / ((double)df_t + 0.5)), natural log
 *             with the bits of the HOST's libm (a table by df, gathered on the device)
 *   norm_d  = k1 * ((1.0 - b) + b * ((double)dl[d] / avgdl))
 *   w(t, d) = idf_t * (((double)tf * (k1 + 1.0)) / ((double)tf + norm_d))
 * A document's score starts at 0.0 and adds w over the query's term slots in listed
 * order: a slot whose list lacks the document adds nothing, a term listed twice
 * counts twice, -1 slots are skipped.  Results are laid out as sme_query_topk's: k
 * rows per query by score descending, then docno ascending (signed), padded with
 * docno -1 / score 0.0; a document holding none of the terms is never a result, and
 * D == 0, an empty query and a query of -1 slots only give pads.
 * k1 must be finite and >= 0 and b in [0, 1]: anything else, NaN included, is
 * SME_EINVAL.  Limits (SME_ELIMIT, the message names the query): k <= 1024, and at
 * most 1024 term slots per query.  An id outside [-1, V) is SME_EINVAL from the host
 * entry (the query named) and skipped like -1 by the device entry; offsets that do
 * not ascend from 0, k < 1 and nq < 0 are SME_EINVAL.
 *
 * The scorer is window-major over windows of 1024 docnos (sme_index_bm25_stats's
 * *window) and exhaustive inside a window; once k candidates stand, a window whose
 * bound -- every slot's weight at the term's largest tf in a document as short as
 * the window's shortest -- lies strictly below the k-th score is skipped.  Option
 * "bm25_split": workgroups per query, 0 (default) automatic, >= 1 that many, capped
 * at the window count and at 4096.  Results are the same for every value.
 *
 * sme_index_prepare_bm25 builds the index's tables (dl, idf, the bound tables) once;
 * nothing ever invalidates them, and the other entries build them on first use.
 * *ms (may be NULL) gets the device time.  sme_index_doc_lengths: the device pointer
 * of dl[docno - *dmin], *span entries, 0 for a docno without postings; the index's
 * own array.  sme_index_bm25_stats: D, L, the longest document, the window size.
 * sme_query_bm25_stats reports on the last BM25 call: the (query, window) pairs that
 * held a posting, those of them the bound skipped, and the postings scored (under a
 * split the workgroups of a query share the k-th score as they find it, so timing
 * may move the last two; it never moves a result). */
int sme_index_prepare_bm25(sme_index *ix, void *stream, float *ms);
int sme_index_doc_lengths(sme_index *ix, void *stream, const int32_t **d_len, int64_t *dmin, int64_t *span);
int sme_index_bm25_stats(const sme_index *ix, uint64_t *docs, uint64_t *total_len, uint64_t *max_len,
                         uint64_t *window);
int sme_query_topk_bm25(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, int nq, int k, double k1,
                        double b, int32_t *out_docno, double *out_score);
int sme_query_topk_bm25_device(sme_index *ix, const int32_t *d_term_ids, const int64_t *d_q_offsets, int nq, int k,
                               double k1, double b, int32_t *d_out_docno, double *d_out_score, void *stream);
int sme_query_bm25_stats(const sme_index *ix, uint64_t *windows, uint64_t *skipped, uint64_t *postings);

/* Scoring given documents: per query a list of term slots and a list of docnos ->
 * every listed document's score under TF-IDF or BM25.  What ranks the result of a
 * Boolean, phrase, proximity or structured query under either model, ranks "only
 * these documents" of a filter kept outside the index, and re-ranks one stage's
 * candidates with other parameters without another pass over the collection.  For
 * an index with a query side (a records-only merged index and a chargram output are
 * SME_EINVAL).
 *
 * Inputs.  Query i has the term slots term_ids[q_offsets[i] .. q_offsets[i+1]) --
 * host arrays in both entries, as in the other batched features -- and the
 * candidates docnos[d_offsets[i] .. d_offsets[i+1]), nq + 1 offsets from 0.  A
 * query's candidates are STRICTLY ASCENDING in signed int32 order: exactly what
 * order 0 of sme_query_boolean / _phrase / _near / _structured returns.  In the device
 * entry both candidate arrays are device memory, so the d_res_off / d_docno of
 * another feature's device call go in unchanged; the entry copies the nq + 1 offsets
 * to the host to check them (one synchronisation, as sme_query_topk_bm25_device
 * does) and a kernel checks the ascending rule before any score is written.
 *
 * model 0, TF-IDF: a document's score is the fp64 sum from 0.0, over the slots in
 * listed order, of the weight at the document's posting in the slot's list: a slot
 * whose list lacks the document adds nothing, a term listed twice counts twice, -1
 * slots are skipped.  Weights are read at call time (sme_index_reweight).  This is
 * the sum sme_query_boolean documents, and its bits are those sme_query_topk gives
 * that document for that term list.  k1 and b are not read.
 * model 1, BM25: exactly sme_query_topk_bm25's w(t, d) above, summed the same way,
 * from the tables of sme_index_prepare_bm25 (built on first use), under the same rule
 * for k1 and b.  The call leaves the last BM25 call's result and counts alone.
 *
 * Results.  hits = the slots, duplicates counted, whose list holds the document.
 * Every candidate with hits >= min_hits is a match: min_hits 0 keeps documents the
 * index has never seen (hits 0, score 0.0), min_hits 1 is "holds at least one term".
 * A candidate outside the index's docno range, or without a posting, is legal.
 * order 0: the matches in the given (docno) order; no sort runs on this path.
 * order 1: score descending, then docno ascending.  Both are then cut to the first m;
 * m == 0: no cut.  Query i's matches are docno / hits / score [res_off[i],
 * res_off[i+1]).  The arrays (host memory from the host entry, device memory from the
 * device entry) are owned by the index until its next rescore call; every other
 * feature's buffers are left alone, and no other feature touches these.
 *
 * SME_EINVAL (the message names the query where there is one): candidates not
 * strictly ascending -- the index's rescore result is then empty --, offsets of
 * either kind not ascending from 0, a term id outside [-1, V), a model or an order
 * other than 0 / 1, m < 0, min_hits < 0, nq < 0, illegal k1 / b under model 1.
 * SME_ELIMIT: more than 1024 slots in a query; 2^31 or more candidates, or slots, in
 * a batch.  nq == 0, a query without candidates and a query without slots are valid.
 *
 * One workgroup scores one tile of 1024 consecutive candidates of a query
 * (sme_query_rescore_stats's *tile).  Per slot it narrows the term's list to the
 * tile's docno range and then either scans that range against the tile or searches
 * it for every candidate.  Option "rescore_path": 0 (default) the cheaper form by the
 * two lengths, 1 always search, 2 always scan.  Results are the same for every value.
 *
 * sme_query_rescore_stats reports on the last rescore call: the batch's candidates,
 * the sum of hits, the matches before the cut, and the tile size. */
int sme_query_rescore(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *docnos,
                      const int64_t *d_offsets, int nq, int model, double k1, double b, int min_hits, int order, int m,
                      const int64_t **res_off, const int32_t **docno, const int32_t **hits, const double **score);
int sme_query_rescore_device(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *d_docnos,
                             const int64_t *d_doc_offsets, int nq, int model, double k1, double b, int min_hits,
                             int order, int m, void *stream, const int64_t **d_res_off, const int32_t **d_docno,
                             const int32_t **d_hits, const double **d_score, int64_t *total);
int sme_query_rescore_stats(const sme_index *ix, uint64_t *candidates, uint64_t *found, uint64_t *matches,
                            uint64_t *tile);

/* Best passages: where in a document the query matched.  Per query a list of term
 * ids and a list of docnos -> for every listed document the best window of at most
 * `width` consecutive positions of one of its records' term streams: what a result
 * list shows as a snippet, highlights as hits, or returns as the best passage of a
 * long document.  For a K = 1 index with a query side that keeps positions (built
 * with option "positions" 1, or after sme_index_attach_positions); any other index
 * is SME_EINVAL, and the message says which of the three it lacks.
 *
 * Inputs, as in sme_query_rescore.  Query i lists the term ids term_ids[q_offsets[i]
 * .. q_offsets[i+1]) -- host arrays in both entries -- and the candidates
 * docnos[d_offsets[i] .. d_offsets[i+1]), nq + 1 offsets from 0, STRICTLY ASCENDING
 * per query in signed int32 order: what order 0 of sme_query_boolean / _phrase / _near
 * / _structured returns.  In the device entry both candidate arrays are device
 * memory; the entry copies the nq + 1 offsets to the host to check them and a kernel
 * checks the ascending rule before anything is written.
 *
 * Slots.  Of a query's listed ids, -1 entries are dropped and a repeated id keeps its
 * first place; the j-th distinct id in listed order is slot j, bit j of a row's mask.
 * A query may list 1024 ids and hold 64 distinct ones.
 *
 * Windows.  The records of docno d are those of the index's term streams with that
 * docno, in the index's record order (equal docnos stay in file order); their ordinal
 * 0, 1, ... among the docno's records is rec.  A window never crosses a record's end:
 * a record of n positions has the starts 0 .. max(0, n - width), and the window at
 * start s is the positions [s, min(s + width, n)) -- an empty record has the one
 * window (0, 0).  Of a window, mask is the OR of the slots of the positions whose term
 * is a query term, cover the number of bits set in it, hits the number of such
 * positions, and score the fp64 sum from 0.0, over the set bits of mask in ascending
 * slot order, of the idf the index's weights use for the slot's term (additions only;
 * read at call time, so sme_index_reweight is honoured).
 * A candidate's best window is the first in the order: score descending, cover
 * descending (which decides where an idf is 0.0), hits descending, rec ascending,
 * start ascending.  A candidate without a record gets rec -1, start 0, len 0, mask 0,
 * hits 0, score 0.0.
 *
 * Result A, the rows.  A candidate is kept when cover >= min_cover (0 keeps every
 * candidate).  order 0: the kept candidates in the given (docno) order; no sort runs.
 * order 1: score descending, then docno ascending.  Both are cut to the first m; m ==
 * 0: no cut.  Query i's rows are [res_off[i], res_off[i+1]) of docno, rec, start, len,
 * hits, mask and score; `total` is their number.
 * Result B, the window terms, with with_terms 1: row r's window is [win_off[r],
 * win_off[r+1]) of win_term, the stream's term ids at the window's positions, and
 * win_slot, each position's slot or -1; win_off has total + 1 entries, the exclusive
 * scan of the rows' len, and win_total is its last.  With with_terms 0 no kernel runs
 * for it: win_off holds the one entry 0 and win_total is 0.
 * Both results (host memory from the host entry, device memory from the device entry)
 * are owned by the index until its next passages call; every other feature's buffers
 * are left alone, and no other feature touches these.  A call empties both before it
 * launches anything, and a refused call leaves them empty.
 *
 * SME_EINVAL (the message names the query where there is one): candidates not
 * strictly ascending, offsets of either kind not ascending from 0, a term id outside
 * [-1, V), width < 1, m < 0, min_cover < 0, an order or a with_terms other than 0 / 1,
 * nq < 0.  SME_ELIMIT: width > 256; more than 64 distinct or 1024 listed ids in a
 * query; 2^31 or more candidates, or listed ids, in a batch; 2^31 or more window term
 * entries.  nq == 0, a query without candidates and a query without ids are valid.
 *
 * sme_query_passages_stats reports on the last passages call: the batch's candidates,
 * those with at least one record, the stream positions of their records (each counted
 * once per candidate), the kept rows before the cut, and the window starts a wave of
 * the scan kernel takes at a time (its chunk length). */
typedef struct sme_passages {
  const int64_t *res_off; /* [nq + 1] */
  const int32_t *docno, *rec, *start, *len, *hits;
  const uint64_t *mask;
  const double *score;
  int64_t total;
  const int64_t *win_off; /* [total + 1], or the one entry 0 */
  const int32_t *win_term;
  const int8_t *win_slot;
  int64_t win_total;
} sme_passages;
int sme_query_passages(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets, const int32_t *docnos,
                       const int64_t *d_offsets, int nq, int width, int min_cover, int order, int m, int with_terms,
                       sme_passages *out);
int sme_query_passages_device(sme_index *ix, const int32_t *term_ids, const int64_t *q_offsets,
                              const int32_t *d_docnos, const int64_t *d_doc_offsets, int nq, int width, int min_cover,
                              int order, int m, int with_terms, void *stream, sme_passages *out);
int sme_query_passages_stats(const sme_index *ix, uint64_t *candidates, uint64_t *with_record, uint64_t *positions,
                             uint64_t *kept, uint64_t *chunk);

/* 128-bit fingerprint of every index term (two u64 per term into device memory
 * d_out[2 V]): equal term strings (k-grams) on different shards get equal
 * fingerprints, so a multi-GPU df exchange can key the all-reduce on them
 * without gathering and sorting term strings (dist.py global_df). */
int sme_index_term_fingerprints(sme_index *ix, uint64_t *d_out, void *stream);

/* Global df of a doc-sharded build by owner rank (the reducer's df =
 * postings length summed over the map outputs, TermKGramDocIndexer.java:175-183).
 * Rows are (fp[2i], fp[2i+1], df[i]) in device memory; a row's owner is
 * fp[2i] % world.
 *   pack:   rows grouped by owner into send_fp[2n] / send_df[n] (owner 0's rows
 *           first, ...), pos[i] = send slot of row i, counts[world] (host) = rows
 *           per owner -- the layout of one all_to_all
 *   sum:    for every received row, out[i] = the sum of df over all received rows
 *           with the same 128-bit fingerprint; *distinct = fingerprints seen
 *   unpack: out[i] = ret[pos[i]] (the owners' sums, returned in send order, back
 *           in local row order)
 * Replaces the Hadoop shuffle's grouping of the doc-counter / df by key. */
int sme_df_owner_pack(sme_ctx *ctx, const uint64_t *d_fp, const int64_t *d_df, int64_t n, int world,
                      uint64_t *d_send_fp, int64_t *d_send_df, int64_t *d_pos, int64_t *counts, void *stream);
int sme_df_owner_sum(sme_ctx *ctx, const uint64_t *d_fp, const int64_t *d_df, int64_t n, int64_t *d_out,
                     int64_t *distinct, void *stream);
int sme_df_owner_unpack(sme_ctx *ctx, const int64_t *d_ret, const int64_t *d_pos, int64_t n, int64_t *d_out,
                        void *stream);

/* Query-owner merge (dist.merge_topk_owner): rows x m candidates
 * (d_score / d_docno / optional d_tie, row-major, any order, docno -1 pads, e.g.
 * the W shards' top-k lists of the queries this rank owns) -> per row the best k
 * in (score desc, tie asc, docno asc) order, docno -1 / score 0 / tie ~0 pads.
 * The tie word is sme_query_topk_tie's (0 in the north-star docno order), so the
 * merged rows equal one index's top-k (IntDocVectorsForwardIndex.java:215-222:
 * Collections.sort over the candidates, first k).  k <= 2048.  Device memory;
 * synchronized on return. */
int sme_topk_merge_rows(sme_ctx *ctx, const double *d_score, const int32_t *d_docno, const uint32_t *d_tie,
                        int64_t rows, int m, int k, int32_t *d_out_docno, double *d_out_score, uint32_t *d_out_tie,
                        void *stream);

/* Owner side of the cross-shard duplicate-docid check (dist.docno_duplicates):
 * d_rows = n (key, source rank) pairs (u64, keys zero-extended 32-bit docnos)
 * received by the keys' owner rank (grouped with sme_df_owner_pack); *count =
 * distinct keys that arrive from two or more source ranks.  A docid held by two
 * shards is one posting with summed tf in the reference's single reducer
 * (TermKGramDocIndexer.java:202-210), so per-shard scoring must refuse it. */
int sme_count_shared_keys(sme_ctx *ctx, const uint64_t *d_rows, int64_t n, int64_t *count, void *stream);

/* Recompute the fp64 TF-IDF weights of a doc-sharded index with global
 * statistics: n_global = records over all shards (all-reduced doc counter),
 * d_df_global = per local term the all-reduced df (device int64[V]) or NULL to
 * keep the shard's own df (SME_IDF_TRUE_DF only; reference mode uses stored df 1). */
int sme_index_reweight(sme_index *ix, int64_t n_global, const int64_t *d_df_global, void *stream);

/* Synthetic Zipfian TREC corpus generated directly in HBM (bench / tests; same
 * bytes as synth.py).  vocab/vocab_off/cdf are host arrays (V words, V+1
 * offsets, V cumulative probabilities).  *d_corpus is freed with sme_synth_free. */
int sme_synth_corpus(int device, const uint8_t *vocab, const int64_t *vocab_off, int64_t V, const double *cdf,
                     int64_t n_docs, int64_t d0, uint64_t seed, int len_lo, int len_hi, void **d_corpus,
                     size_t *nbytes);
void sme_synth_free(void *d_corpus);

/* Calibration (bench.py): achievable HBM bandwidth of a streaming device copy of
 * `bytes` (x reps, after a warm-up); *gbps = read + write bytes / kernel time. */
int sme_hbm_copy_bench(int device, size_t bytes, int reps, double *gbps);

/* Reference-layout output from doc shards (the job's R part files,
 * TermKGramDocIndexer.java:189-211,246-275): partition p is reduced by rank
 * p % world.  pack: this shard's terms grouped by owner rank as `world` blobs
 * laid out back to back at d_out (device memory; NULL = only fill sizes[world],
 * each blob's bytes): the terms (String.compareTo order), their postings in
 * reduce order, and the shard's record docnos for the owner of the " " doc
 * counter's partition.  merge: the n blobs a rank received (one per shard, in
 * shard order, back to back at d_blobs) -> a records-only index whose
 * partitions p with p % world == rank hold exactly what the reference's single
 * reducer writes for the shards' map tasks (postings merged per term by
 * MyReducer.reduce, :189-211: docno sort, equal docnos summed, stable tf-desc
 * sort; one doc-counter list per map task).  Read it with sme_index_serialize /
 * sme_index_copy_records; it has no query side (query entry points: SME_EINVAL). */
int sme_index_pack_pieces(sme_index *ix, int world, void *d_out, uint64_t *sizes, void *stream);
/* Device pointer to the docnos of the index's records in input order (*n = N;
 * the map task's doc-counter postings, TermKGramDocIndexer.java:84-90,126). */
int sme_index_record_docnos(sme_index *ix, const int32_t **d_docno, int64_t *n);
int sme_merge_pieces(sme_ctx *ctx, const void *d_blobs, const uint64_t *sizes, int n, void *stream,
                     sme_index **out);

/* Merge n indexes of ctx (1 <= n <= 64) into one new, full index: what one build
 * of the inputs' corpora laid end to end gives, in every array.  The inputs are
 * read only and stay valid; they may be built, loaded from records or themselves
 * merged, in any mix, and are taken in the order given, as the map tasks of one
 * job in that order.  THEY MUST HAVE BEEN NUMBERED WITH ONE DOCNO MAPPING: docnos
 * are compared as they are, and nothing here can check where they came from.
 *   vocabulary  the union of the inputs' term strings in TermDF (String.compareTo)
 *               order, equal strings one term;
 *   postings    per term the inputs' lists merged by docno; a docno several inputs
 *               hold (a docid in two of them, docno 0, negative docnos of unmapped
 *               docids) is one posting with the tfs summed, as MyReducer.reduce and
 *               the build's duplicate-docno merge do (a sum >= 2^24 is SME_ELIMIT);
 *               the reduce order is that list stably sorted by tf descending;
 *   weights     N = the sum of the inputs' N, true df = the merged list's length,
 *               then the weights of sme_index_reweight(N) under ctx's idf mode.  An
 *               input's own earlier sme_index_reweight is NOT carried over;
 *   doc counter the inputs' lists back to back, every input's map-task starts kept
 *               (a built input is one task), so the " " record serializes as the
 *               reference job over those map tasks writes it.  As for a loaded
 *               index, sme_index_record_docnos / sme_index_pack_pieces on the
 *               result return SME_EINVAL;
 *   positions   kept if every input that has records keeps them ("positions"): the
 *               records' streams in docno-ascending order (equal docnos: input
 *               order, then the order inside the input), term ids rewritten to the
 *               merged ids; more than 2^31 - 1 stream positions is SME_ELIMIT.
 *               Otherwise the result keeps none and the position entry points
 *               refuse it as they refuse any index without them.
 * The query side and the wildcard table are built on first use, as for any index.
 * Refused before any per-term work, the message naming the input's place in the
 * list: n out of range, a null input, an input of another context, a records-only
 * input (sme_merge_pieces output), a chargram output (all SME_EINVAL); the context
 * or an input with K != 1 is SME_ENOTIMPL ("merging K >= 2 indexes").  n = 1 gives
 * a copy; inputs without records or terms are legal anywhere in the list.
 * sme_last_build_profile then holds the merger's stages (terms, postings,
 * tf_order, weights, positions, total).  stream NULL = the context's stream. */
int sme_index_merge(sme_ctx *ctx, sme_index *const *indexes, int n, void *stream, sme_index **out);
/* Of an index sme_index_merge made: its inputs, the terms two or more inputs held,
 * the postings that merging equal docnos removed (sum of the inputs' P - P), and 1
 * if the concatenation path ran (disjoint docno ranges, "merge_append").  All four
 * are 0 for any other index. */
int sme_index_merge_stats(const sme_index *ix, uint64_t *inputs, uint64_t *shared_terms, uint64_t *merged_postings,
                          uint64_t *appended);

/* Delete documents: a new, full index of ix's context that is, in every array, what
 * one build gives over ix's records in their order minus every record whose docno
 * is in the list (n docnos; host memory, or device memory for the _device entry,
 * which takes for instance the d_docno of sme_query_boolean_device as it is).  ix
 * is read only and stays valid, and so does its last result of every query
 * feature.  "Replace document d" is this call followed by sme_index_merge with a
 * build of the new document.
 *   the list    any order, duplicates allowed.  Docnos that no record has are
 *               ignored, values outside the index's docno range, INT32_MIN and
 *               INT32_MAX included (docno - dmin is taken in 64 bits).  Docno 0
 *               names every record without a DOCNO, a negative docno the records
 *               of that unmapped docid.  A docno several records hold (a docid
 *               occurring twice) removes all of them: the posting that summed
 *               their tfs goes whole.  n = 0 gives a copy;
 *   vocabulary  the terms that keep at least one posting, in the same TermDF
 *               order, ids renumbered densely;
 *   postings    both orders: ix's list of the term without the removed docnos, in
 *               ix's order (removing keeps an order, nothing is sorted); offsets
 *               and df from the surviving counts; P, V follow, N = the surviving
 *               records, max_tf is recomputed over the survivors (at least 1), and
 *               the docno range is that of the surviving records;
 *   weights     those of sme_index_reweight(N) with the new N and df under the
 *               context's idf mode.  ix's own earlier sme_index_reweight is NOT
 *               carried over;
 *   doc counter ix's record list without the removed records.  A surviving record
 *               starts a map task if and only if no survivor lies between it and
 *               the nearest task start at or before it: a task that loses its first
 *               record starts at its next survivor, one that loses every record
 *               disappears, so the " " record serializes as the reference job over
 *               the remaining records of those map tasks writes it.  As for a
 *               merged index, sme_index_record_docnos / sme_index_pack_pieces on
 *               the result return SME_EINVAL;
 *   positions   kept if and only if ix keeps them: the surviving records' streams
 *               in ix's record order, term ids rewritten to the new ids.
 * The query side and the wildcard table are built on first use, as for any index.
 * Refused before any per-posting work, with a message: a null ix or out, n < 0,
 * n > 0 with a null list, a records-only index (sme_merge_pieces output), a
 * chargram output (all SME_EINVAL); K != 1 is SME_ENOTIMPL ("deleting from K >= 2
 * indexes").  An index opened from part files (sme_index_from_records*), or merged
 * from one, is SME_EINVAL too: its doc counter never holds a map task's last
 * docno, so which record has a docno cannot be decided there.
 * sme_last_build_profile then holds the stages set, records, postings, terms,
 * tf_order, weights, positions, total.  stream NULL = the context's stream. */
int sme_index_delete_docnos(sme_index *ix, const int32_t *docnos, int64_t n, void *stream, sme_index **out);
int sme_index_delete_docnos_device(sme_index *ix, const int32_t *d_docnos, int64_t n, void *stream,
                                   sme_index **out);
/* Of an index sme_index_delete_docnos* made: the distinct listed docnos that at
 * least one record had, and the records, postings and terms removed.  All four
 * are 0 for any other index. */
int sme_index_delete_stats(const sme_index *ix, uint64_t *docnos, uint64_t *records, uint64_t *postings,
                           uint64_t *terms);

/* The positions file: the term streams (sme_index_positions) of an index in a file
 * form, written on the device from any index that keeps positions and attached on
 * the device to one that keeps none -- an index opened from its part files
 * (sme_index_from_records*) answers phrase, proximity, structured and feedback calls
 * again without the corpus.  The format is this library's own (no reference
 * counterpart); all integers are little-endian:
 *   offset 0   8 magic bytes 53 4D 45 50 4F 53 00 01 ("SMEPOS", 0, 1)
 *          8   u32 version = 1
 *         12   u32 bits b, need <= b <= 31, need = max(1, bit length of (V - 1))
 *         16   u64 records Rn (= the index's N, < 2^31)
 *         24   u64 positions T (< 2^31, the build's own limit)
 *         32   u64 V
 *         40   u64 vocabulary digest
 *         48   16 reserved bytes, zero
 *         64   int32 docno[Rn], ascending in signed order (equal values allowed),
 *              zero-padded to a multiple of 8 bytes
 *         then u32 len[Rn], padded likewise; their sum is T
 *         then u64 word[ceil(T b / 64)]: position p's id occupies bits [p b, (p + 1) b)
 *              of the words seen as one little-endian bit string (bit i = bit i mod 64
 *              of word i / 64); the unused high bits of the last word are zero.
 * The file ends exactly there.  Records are in the order of the streams: docno
 * ascending, records of equal docno in the order the index holds them.
 * digest = sum over t < V of h_t mod 2^64, h_t = FNV-1a-64 (offset basis
 * 0xcbf29ce484222325, prime 0x100000001b3) over the 8 bytes of t, little-endian,
 * followed by term t's UTF-16 code units, each low byte first.
 *
 * Writing.  bits = 0 writes the narrowest width, need; any b in [need, 31] is a
 * valid file; another value is SME_EINVAL.  *buf / *d_buf (n bytes; host memory from
 * the host entry, which is the device entry plus one copy; device memory from the
 * device entry) are owned by the index until its next posfile call and leave every
 * other feature's result buffers alone.  SME_EINVAL, with a message that says which:
 * an index without positions, one with K != 1, one without a query side, a chargram
 * output.  sme_last_build_profile then holds the stages digest, sections, encode,
 * total.
 *
 * Attaching fills the streams of an existing K = 1 TermKGramDocIndexer index that
 * has a query side and keeps no positions (loaded, built without the option, merged
 * or deleted without them) in place; d_file is 8-byte aligned.  flags: 0, or
 * SME_ATTACH_NO_CROSSCHECK.  SME_EINVAL, with a message that says which: an index
 * that already keeps positions, K != 1, a chargram output, a records-only index,
 * unknown flag bits.  Nothing in the file is trusted, and a refused file leaves the
 * index exactly as it was.  Checked, in this order:
 *   header      on the host (the device entry copies 64 bytes down first): magic,
 *               version, reserved bytes, bits, records == N, V == the index's V, the
 *               limits, and the exact file size, computed with overflow-checked
 *               arithmetic before any section offset is used.  SME_EPARSE with a
 *               message naming the field; positions >= 2^31 is SME_ELIMIT;
 *   digest      computed on the device over the index's term strings; a mismatch is
 *               SME_EPARSE, "written for another vocabulary";
 *   structure   on the device while decoding: docnos ascending, the lengths adding up
 *               to positions, every id < V, zero padding.  SME_EPARSE, the message
 *               naming the first offending record or position.  These checks keep
 *               every later kernel that indexes by a stream id in bounds and always run;
 *   cross-check (unless SME_ATTACH_NO_CROSSCHECK) every posting (t, d, tf) of the index
 *               has exactly tf positions holding t in the records of docno d, and
 *               every position's (id, docno) has a posting.  SME_EPARSE, the message
 *               naming the first (term id, then docno) that disagrees.  An index's own
 *               file passes.  Without it a file with the right structure and the
 *               wrong content is accepted: the flag is for files one wrote oneself.
 * Afterwards sme_index_positions reports the streams, and sme_query_phrase / _near /
 * _structured, sme_index_feedback_terms and sme_index_merge treat the index as a
 * built one.  sme_index_delete_docnos still refuses an index opened from part files.
 * sme_last_build_profile then holds the stages header, digest, records, decode,
 * crosscheck, total.  stream NULL = the context's stream.
 *
 * sme_index_posfile_stats reports on the last posfile call on the index: the file's
 * bytes and width, the postings the cross-check compared (P; 0 without it, and after
 * a write), and the device times of the encode kernel (a write), the decode kernel
 * and the cross-check (an attach); the time pointers may be NULL. */
#define SME_ATTACH_NO_CROSSCHECK 1
int sme_index_positions_file(sme_index *ix, int bits, void *stream, const uint8_t **buf, size_t *n);
int sme_index_positions_file_device(sme_index *ix, int bits, void *stream, const void **d_buf, size_t *n);
int sme_index_attach_positions(sme_index *ix, const uint8_t *file, size_t n, int flags, void *stream);
int sme_index_attach_positions_device(sme_index *ix, const void *d_file, size_t n, int flags, void *stream);
int sme_index_posfile_stats(const sme_index *ix, uint64_t *file_bytes, uint64_t *bits, uint64_t *checked_postings,
                            float *encode_ms, float *decode_ms, float *crosscheck_ms);

/* Timing of the last build, per stage, in milliseconds (device events on the
 * build stream), as a JSON object; "tok_kernel" brackets exactly the tokenizer
 * launch and "query_kernel" (if a query batch ran) the last scoring launch.
 * Beside the timings it carries integer path counters, so a caller (or a test)
 * can tell which path ran:
 *   tok_attempts, vocab_attempts, lt_attempts   passes of the build's capacity
 *     loops (raw-vocabulary table, k_vocab's long-token / multi-term lists, the
 *     '<' list): 1 each when the first capacity held;
 *   records_fast, records_slow   records the build tokenized with the
 *     byte-parallel k_tok_fast and with the sequential k_tok_slow (complex
 *     markup, or shorter than 48 bytes); their sum is the record count (like
 *     every value here they print with six significant digits);
 *   query_overflow   k_query_win queries whose first candidate list overflowed,
 *   query_fallback   of those, the queries finally scored by the block-max sweep,
 *   query_split      1 when the batch was split by query range (table budget),
 *   query_stages     k_query_win launches of the first round (1: not staged),
 *   query_slices     query slices per window of those launches
 * (the query_ counters only after a batch on the window kernel; of a split
 * batch, stages and slices are those of its last part). */
int sme_last_build_profile(const sme_ctx *ctx, const char **json);

#ifdef __cplusplus
}
#endif
#endif
