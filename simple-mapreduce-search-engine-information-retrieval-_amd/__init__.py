"""sme -- MI355X-native drop-in for the reference's index/TF-IDF/query hot path.

Host-side mirror of the reference operator surface (names follow the Java
classes; see include/sme.h for the C-ABI each call goes through):

  TermKGramDocIndexer    C/sa/edu/kaust/indexing/TermKGramDocIndexer.java:227-283 (run)
  TrecDocnoMapping       C/edu/umd/cloud9/collection/trec/TrecDocnoMapping.java:92-155
  GalagoTokenizer        C/ivory/tokenize/GalagoTokenizer.java:139-183 (processContent)
  IntDocVectorsForwardIndex  C/sa/edu/kaust/fwindex/IntDocVectorsForwardIndex.java:131-223
                         (getValue / rank), batched as Index.query_topk

Everything computes on the GPU through libsme.so.  There is no CPU fallback:
if the HIP library is missing or no GPU is visible, calls raise SmeError.
"""
import collections
import ctypes as C
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SME_LIB_PATH") or os.path.join(_HERE, "libsme.so")

SME_IDF_REFERENCE = 0
SME_TIE_DOCNO = 0      # score desc, docno asc (north star)
SME_TIE_REFERENCE = 1  # score desc, then rank()'s printed order (first encounter; include/sme.h)
SME_TIE_JAVA7 = 2      # rank()'s list as Java 7's Collections.sort (TimSort) leaves it; -2 rows: it throws
SME_IDF_TRUE_DF = 1


class SmeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sme error %d: %s" % (code, msg))
        self.code = code


class _Config(C.Structure):
    _fields_ = [("k", C.c_int), ("num_partitions", C.c_int), ("idf_mode", C.c_int), ("tiebreak", C.c_int),
                ("device", C.c_int), ("reserved", C.c_int * 11)]


class _Passages(C.Structure):
    """sme_passages (include/sme.h): the rows and the window terms of a passages call."""
    _fields_ = [("res_off", C.c_void_p), ("docno", C.c_void_p), ("rec", C.c_void_p), ("start", C.c_void_p),
                ("len", C.c_void_p), ("hits", C.c_void_p), ("mask", C.c_void_p), ("score", C.c_void_p),
                ("total", C.c_int64), ("win_off", C.c_void_p), ("win_term", C.c_void_p), ("win_slot", C.c_void_p),
                ("win_total", C.c_int64)]


_PASSAGE_FIELDS = ("res_off", "docno", "rec", "start", "len", "hits", "mask", "score", "win_off", "win_term",
                   "win_slot")
Passages = collections.namedtuple("Passages", _PASSAGE_FIELDS)
DevicePassages = collections.namedtuple("DevicePassages", _PASSAGE_FIELDS + ("total", "win_total"))


def snippet(vocabulary, win_term, win_slot):
    """A window as text: its term strings in stream order, the hits (slot >= 0) in
    square brackets.  vocabulary: Index.terms(), or anything indexed by term id."""
    return " ".join("[%s]" % vocabulary[int(t)] if s >= 0 else vocabulary[int(t)] for t, s in zip(win_term, win_slot))


_lib = None

EXPORTS = [
    "sme_last_error", "sme_version", "sme_device_alloc", "sme_device_free", "sme_memcpy", "sme_create", "sme_destroy", "sme_load_docno_mapping", "sme_build_index",
    "sme_build_index_device", "sme_index_free", "sme_index_stats", "sme_index_partition_records", "sme_index_serialize",
    "sme_index_copy_records", "sme_index_csr",
    "sme_index_device_arrays", "sme_index_term", "sme_tokenize", "sme_lookup_terms", "sme_query_topk",
    "sme_query_topk_device", "sme_query_topk_device_tie", "sme_query_topk_tie", "sme_last_build_profile", "sme_index_reweight", "sme_number_documents",
    "sme_build_chargram", "sme_build_chargram_device", "sme_chargram_partition_text", "sme_chargram_stats",
    "sme_split_points", "sme_split_points_device", "sme_index_term_fingerprints", "sme_set_option",
    "sme_index_prepare_queries", "sme_hbm_copy_bench", "sme_index_pack_pieces", "sme_merge_pieces",
    "sme_index_record_docnos", "sme_df_owner_pack", "sme_df_owner_sum", "sme_df_owner_unpack",
    "sme_topk_merge_rows", "sme_count_shared_keys", "sme_index_from_records", "sme_index_from_records_device",
    "sme_index_prepare_wildcards", "sme_index_wildcard_stats", "sme_index_expand_wildcards",
    "sme_index_expand_wildcards_device",
    "sme_index_suggest_terms", "sme_index_suggest_terms_device", "sme_index_suggest_stats",
    "sme_query_boolean", "sme_query_boolean_device", "sme_query_boolean_stats",
    "sme_index_positions", "sme_query_phrase", "sme_query_phrase_device", "sme_query_phrase_stats",
    "sme_query_near", "sme_query_near_device", "sme_query_near_stats",
    "sme_query_structured", "sme_query_structured_device", "sme_query_structured_stats",
    "sme_index_feedback_terms", "sme_index_feedback_terms_device", "sme_index_feedback_stats",
    "sme_index_merge", "sme_index_merge_stats",
    "sme_index_delete_docnos", "sme_index_delete_docnos_device", "sme_index_delete_stats",
    "sme_index_positions_file", "sme_index_positions_file_device", "sme_index_attach_positions",
    "sme_index_attach_positions_device", "sme_index_posfile_stats",
    "sme_index_prepare_bm25", "sme_index_doc_lengths", "sme_index_bm25_stats", "sme_query_topk_bm25",
    "sme_query_topk_bm25_device", "sme_query_bm25_stats",
    "sme_query_rescore", "sme_query_rescore_device", "sme_query_rescore_stats",
    "sme_query_passages", "sme_query_passages_device", "sme_query_passages_stats",
]


def lib():
    """Load libsme.so (fails loudly: the product has no CPU path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SmeError(-2, "libsme.so not built (run __graft_entry__.build() or make -C %s)" % _HERE)
    # a process that also drives the device through torch lets torch's HIP runtime
    # open it first (torch's lazy init fails once libsme's runtime holds the device)
    import sys
    t = sys.modules.get("torch")
    if t is not None and t.cuda.is_available():
        t.cuda.init()
    L = C.CDLL(LIB_PATH)
    vp, sz, i64p, i32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    L.sme_last_error.restype = C.c_char_p
    L.sme_device_alloc.argtypes = [C.c_int, sz, C.POINTER(vp)]
    L.sme_device_free.argtypes = [vp]
    L.sme_device_free.restype = None
    L.sme_memcpy.argtypes = [vp, vp, sz, vp]
    L.sme_version.restype = C.c_char_p
    L.sme_create.argtypes = [C.POINTER(_Config), C.POINTER(vp)]
    L.sme_destroy.argtypes = [vp]
    L.sme_destroy.restype = None
    L.sme_load_docno_mapping.argtypes = [vp, C.c_char_p, sz]
    L.sme_build_index.argtypes = [vp, C.c_char_p, sz, C.POINTER(vp)]
    L.sme_build_index_device.argtypes = [vp, vp, sz, vp, C.POINTER(vp)]
    L.sme_index_free.argtypes = [vp]
    L.sme_index_free.restype = None
    L.sme_index_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sme_index_partition_records.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    L.sme_index_serialize.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    L.sme_index_copy_records.argtypes = [vp, C.c_int, vp, sz, C.POINTER(sz)]
    L.sme_index_csr.argtypes = [vp, C.POINTER(i64p), C.POINTER(i32p), C.POINTER(i32p), C.POINTER(i32p)]
    L.sme_index_device_arrays.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.sme_index_term.argtypes = [vp, C.c_int64, C.POINTER(vp), C.POINTER(sz)]
    L.sme_tokenize.argtypes = [vp, C.c_char_p, sz, vp, sz, i64p, C.c_int, C.POINTER(C.c_int)]
    L.sme_lookup_terms.argtypes = [vp, C.c_char_p, i64p, C.c_int, i32p]
    L.sme_query_topk.argtypes = [vp, i32p, i64p, C.c_int, C.c_int, i32p, C.POINTER(C.c_double)]
    L.sme_query_topk_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.sme_query_topk_device_tie.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.sme_query_topk_tie.argtypes = [vp, i32p, i64p, C.c_int, C.c_int, i32p, C.POINTER(C.c_double),
                                     C.POINTER(C.c_uint32)]
    L.sme_last_build_profile.argtypes = [vp, C.POINTER(C.c_char_p)]
    L.sme_index_reweight.argtypes = [vp, C.c_int64, vp, vp]
    L.sme_number_documents.argtypes = [vp, C.c_char_p, sz, C.POINTER(vp), C.POINTER(sz)]
    L.sme_build_chargram.argtypes = [vp, C.c_char_p, sz, C.POINTER(vp)]
    L.sme_build_chargram_device.argtypes = [vp, vp, sz, vp, C.POINTER(vp)]
    L.sme_chargram_partition_text.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    L.sme_chargram_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sme_synth_corpus.argtypes = [C.c_int, C.c_char_p, vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_uint64, C.c_int,
                                   C.c_int, C.POINTER(vp), C.POINTER(sz)]
    L.sme_index_term_fingerprints.argtypes = [vp, vp, vp]
    L.sme_split_points.argtypes = [vp, C.c_char_p, sz, C.c_int, C.POINTER(C.c_uint64)]
    L.sme_split_points_device.argtypes = [vp, vp, sz, C.c_int, vp, C.POINTER(C.c_uint64)]
    L.sme_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.sme_index_prepare_queries.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.sme_synth_free.argtypes = [vp]
    L.sme_hbm_copy_bench.argtypes = [C.c_int, sz, C.c_int, C.POINTER(C.c_double)]
    L.sme_synth_free.restype = None
    L.sme_index_pack_pieces.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_uint64), vp]
    L.sme_merge_pieces.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.c_int, vp, C.POINTER(vp)]
    L.sme_index_record_docnos.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.sme_df_owner_pack.argtypes = [vp, vp, vp, C.c_int64, C.c_int, vp, vp, vp, i64p, vp]
    L.sme_df_owner_sum.argtypes = [vp, vp, vp, C.c_int64, vp, i64p, vp]
    L.sme_df_owner_unpack.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    L.sme_topk_merge_rows.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int, vp, vp, vp, vp]
    L.sme_count_shared_keys.argtypes = [vp, vp, C.c_int64, i64p, vp]
    L.sme_index_from_records.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.c_int, C.POINTER(vp)]
    L.sme_index_from_records_device.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.c_int, vp, C.POINTER(vp)]
    L.sme_index_prepare_wildcards.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.sme_index_wildcard_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sme_index_expand_wildcards.argtypes = [vp, C.c_char_p, i64p, C.c_int, C.POINTER(i64p), C.POINTER(i32p)]
    L.sme_index_expand_wildcards_device.argtypes = [vp, C.c_char_p, i64p, C.c_int, vp, C.POINTER(vp), C.POINTER(vp),
                                                    i64p]
    u8p = C.POINTER(C.c_uint8)
    L.sme_index_suggest_terms.argtypes = [vp, C.c_char_p, i64p, C.c_int, C.c_int, C.c_int, C.POINTER(i64p),
                                          C.POINTER(i32p), C.POINTER(u8p)]
    L.sme_index_suggest_terms_device.argtypes = [vp, C.c_char_p, i64p, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp),
                                                 C.POINTER(vp), C.POINTER(vp), i64p]
    L.sme_index_suggest_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    f64p = C.POINTER(C.c_double)
    L.sme_query_boolean.argtypes = [vp, i32p, i64p, u8p, i64p, C.c_int, C.c_int, C.c_int, C.POINTER(i64p),
                                    C.POINTER(i32p), C.POINTER(f64p)]
    L.sme_query_boolean_device.argtypes = [vp, i32p, i64p, u8p, i64p, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp),
                                           C.POINTER(vp), C.POINTER(vp), i64p]
    L.sme_query_boolean_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sme_index_positions.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sme_query_phrase.argtypes = [vp, i32p, i64p, C.c_int, C.c_int, C.c_int, C.POINTER(i64p), C.POINTER(i32p),
                                   C.POINTER(i32p), C.POINTER(f64p)]
    L.sme_query_phrase_device.argtypes = [vp, i32p, i64p, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp), C.POINTER(vp),
                                          C.POINTER(vp), C.POINTER(vp), i64p]
    L.sme_query_phrase_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sme_query_near.argtypes = [vp, i32p, i64p, i32p, u8p, C.c_int, C.c_int, C.c_int, C.POINTER(i64p), C.POINTER(i32p),
                                 C.POINTER(i32p), C.POINTER(f64p)]
    L.sme_query_near_device.argtypes = [vp, i32p, i64p, i32p, u8p, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp),
                                        C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i64p]
    L.sme_query_near_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sme_query_structured.argtypes = [vp, i32p, i64p, u8p, i32p, i64p, u8p, i64p, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(i64p), C.POINTER(i32p), C.POINTER(f64p)]
    L.sme_query_structured_device.argtypes = [vp, i32p, i64p, u8p, i32p, i64p, u8p, i64p, C.c_int, C.c_int, C.c_int,
                                              vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i64p]
    L.sme_query_structured_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint64)]
    L.sme_index_feedback_terms.argtypes = [vp, i32p, i64p, C.c_int, i32p, i64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(i64p), C.POINTER(i32p), C.POINTER(i32p), C.POINTER(i32p),
                                           C.POINTER(f64p)]
    L.sme_index_feedback_terms_device.argtypes = [vp, vp, i64p, C.c_int, i32p, i64p, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                  C.POINTER(vp), C.POINTER(vp), i64p]
    L.sme_index_feedback_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 5
    L.sme_index_merge.argtypes = [vp, C.POINTER(vp), C.c_int, vp, C.POINTER(vp)]
    L.sme_index_merge_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
    L.sme_index_delete_docnos.argtypes = [vp, i32p, C.c_int64, vp, C.POINTER(vp)]
    L.sme_index_delete_docnos_device.argtypes = [vp, vp, C.c_int64, vp, C.POINTER(vp)]
    L.sme_index_delete_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
    L.sme_index_positions_file.argtypes = [vp, C.c_int, vp, C.POINTER(vp), C.POINTER(sz)]
    L.sme_index_positions_file_device.argtypes = [vp, C.c_int, vp, C.POINTER(vp), C.POINTER(sz)]
    L.sme_index_attach_positions.argtypes = [vp, vp, sz, C.c_int, vp]
    L.sme_index_attach_positions_device.argtypes = [vp, vp, sz, C.c_int, vp]
    L.sme_index_posfile_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 3 + [C.POINTER(C.c_float)] * 3
    L.sme_index_prepare_bm25.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.sme_index_doc_lengths.argtypes = [vp, vp, C.POINTER(vp), i64p, i64p]
    L.sme_index_bm25_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
    L.sme_query_topk_bm25.argtypes = [vp, i32p, i64p, C.c_int, C.c_int, C.c_double, C.c_double, i32p,
                                      C.POINTER(C.c_double)]
    L.sme_query_topk_bm25_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, vp]
    L.sme_query_bm25_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 3
    L.sme_query_rescore.argtypes = [vp, i32p, i64p, i32p, i64p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                    C.c_int, C.c_int, C.POINTER(i64p), C.POINTER(i32p), C.POINTER(i32p),
                                    C.POINTER(f64p)]
    L.sme_query_rescore_device.argtypes = [vp, i32p, i64p, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                           C.c_int, C.c_int, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                           C.POINTER(vp), i64p]
    L.sme_query_rescore_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
    L.sme_query_passages.argtypes = [vp, i32p, i64p, i32p, i64p] + [C.c_int] * 6 + [C.POINTER(_Passages)]
    L.sme_query_passages_device.argtypes = [vp, i32p, i64p, vp, vp] + [C.c_int] * 6 + [vp, C.POINTER(_Passages)]
    L.sme_query_passages_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 5
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise SmeError(rc, lib().sme_last_error().decode("utf-8", "replace"))


def memcpy(dst, src, nbytes, stream=None):
    """Copy between host and device memory through libsme's HIP runtime
    (sme_memcpy; stream None = synchronous).  Python never loads a HIP runtime
    of its own: torch's bundled one and the library's could disagree."""
    _check(lib().sme_memcpy(C.c_void_p(dst), C.c_void_p(src), nbytes, C.c_void_p(stream or 0)))


def _d2h(arr, dptr, nbytes):
    """device -> host into a numpy array."""
    memcpy(arr.ctypes.data, dptr, nbytes)


def _host_bytes(p, n):
    """Copy n bytes at host address p (ctypes.string_at takes a C int size: < 2 GiB)."""
    if not n:
        return b""
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_ubyte)), shape=(n,)).tobytes()


def _mutf8_decode(b):
    """DataInput.readUTF body -> str (surrogates kept)."""
    out, i = [], 0
    while i < len(b):
        c = b[i]
        if c < 0x80:
            out.append(c)
            i += 1
        elif c & 0xE0 == 0xC0:
            out.append(((c & 0x1F) << 6) | (b[i + 1] & 0x3F))
            i += 2
        else:
            out.append(((c & 0x0F) << 12) | ((b[i + 1] & 0x3F) << 6) | (b[i + 2] & 0x3F))
            i += 3
    raw = b"".join(u.to_bytes(2, "little") for u in out)
    return raw.decode("utf-16-le", "surrogatepass")


# ---------------------------------------------------------------------------
class TrecDocnoMapping:
    """Docno mapping file: int32 N, N x writeUTF(docid), docids sorted (writeDocnoData)."""

    @staticmethod
    def write(docids):
        out = [struct.pack(">i", len(docids))]
        for d in docids:
            b = d.encode("utf-8")
            out.append(struct.pack(">H", len(b)) + b)
        return b"".join(out)


class Context:
    """One device context (sme_ctx): config + docno mapping + reusable HBM workspace."""

    def __init__(self, k=1, num_partitions=1, idf_mode=SME_IDF_REFERENCE, device=0, tiebreak=SME_TIE_DOCNO):
        cfg = _Config(k, num_partitions, idf_mode, tiebreak, device)
        h = C.c_void_p()
        _check(lib().sme_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.k, self.num_partitions, self.idf_mode, self.device = k, num_partitions, idf_mode, device
        self.tiebreak = tiebreak

    def close(self):
        if getattr(self, "_h", None):
            lib().sme_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_option(self, name, value):
        """sme_set_option: a result-preserving path option (include/sme.h)."""
        _check(lib().sme_set_option(self._h, name.encode(), int(value)))

    def load_docno_mapping(self, mapping_bytes):
        _check(lib().sme_load_docno_mapping(self._h, mapping_bytes, len(mapping_bytes)))

    def number_documents(self, corpus):
        """NumberTrecDocuments + writeDocnoData on the device: the mapping file bytes."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().sme_number_documents(self._h, corpus, len(corpus), C.byref(p), C.byref(n)))
        return C.string_at(p, n.value)

    def build(self, corpus):
        """Build from host bytes (copied to HBM)."""
        h = C.c_void_p()
        _check(lib().sme_build_index(self._h, corpus, len(corpus), C.byref(h)))
        return Index(h, self)

    def build_ptr(self, host_ptr, nbytes):
        """Build from nbytes of host memory at address host_ptr (pinned memory is
        copied to HBM at DMA rate)."""
        h = C.c_void_p()
        _check(lib().sme_build_index(self._h, C.cast(C.c_void_p(host_ptr), C.c_char_p), nbytes, C.byref(h)))
        return Index(h, self)

    def build_device(self, d_ptr, nbytes, stream=None):
        """Build from a corpus already in HBM (e.g. a torch uint8 tensor's data_ptr())."""
        h = C.c_void_p()
        _check(lib().sme_build_index_device(self._h, C.c_void_p(d_ptr), nbytes, C.c_void_p(stream or 0),
                                            C.byref(h)))
        return Index(h, self)

    def load_records(self, parts):
        """sme_index_from_records: an Index from its reduce-output record streams,
        one bytes-like per partition (the bytes of a part-NNNNN file after its
        SequenceFile header, sync escapes and all; seqfile.read_part_body).  The
        partition count need not be this context's: terms are merged into one
        order and the index serializes into num_partitions partitions."""
        views = [np.frombuffer(b, dtype=np.uint8) for b in parts]
        offs = (C.c_uint64 * (len(views) + 1))()
        for i, v in enumerate(views):
            offs[i + 1] = offs[i] + v.size
        buf = np.concatenate(views) if views else np.zeros(0, np.uint8)
        h = C.c_void_p()
        _check(lib().sme_index_from_records(self._h, C.c_void_p(buf.ctypes.data if buf.size else 0), offs, len(views),
                                            C.byref(h)))
        return Index(h, self)

    def load_records_device(self, d_ptr, part_offsets, stream=None):
        """sme_index_from_records_device: the same from streams laid back to back
        in HBM at d_ptr; part_offsets = len(parts) + 1 byte offsets from 0."""
        n = len(part_offsets) - 1
        offs = (C.c_uint64 * (n + 1))(*[int(x) for x in part_offsets])
        h = C.c_void_p()
        _check(lib().sme_index_from_records_device(self._h, C.c_void_p(d_ptr or 0), offs, n, C.c_void_p(stream or 0),
                                                   C.byref(h)))
        return Index(h, self)

    def df_owner_pack(self, d_fp, d_df, n, world, d_send_fp, d_send_df, d_pos, stream=None):
        """sme_df_owner_pack: rows grouped by owner rank (fp word 0 mod world) for
        one all_to_all; returns the rows per owner (list of `world` ints)."""
        counts = (C.c_int64 * max(world, 1))()
        _check(lib().sme_df_owner_pack(self._h, C.c_void_p(d_fp), C.c_void_p(d_df), n, world, C.c_void_p(d_send_fp),
                                       C.c_void_p(d_send_df), C.c_void_p(d_pos), counts, C.c_void_p(stream or 0)))
        return [int(c) for c in counts[:world]]

    def df_owner_sum(self, d_fp, d_df, n, d_out, stream=None):
        """sme_df_owner_sum: per received row, df summed over its fingerprint's
        rows; returns the number of distinct fingerprints."""
        dist = C.c_int64()
        _check(lib().sme_df_owner_sum(self._h, C.c_void_p(d_fp), C.c_void_p(d_df), n, C.c_void_p(d_out),
                                      C.byref(dist), C.c_void_p(stream or 0)))
        return dist.value

    def df_owner_unpack(self, d_ret, d_pos, n, d_out, stream=None):
        """sme_df_owner_unpack: out[i] = ret[pos[i]]."""
        _check(lib().sme_df_owner_unpack(self._h, C.c_void_p(d_ret), C.c_void_p(d_pos), n, C.c_void_p(d_out),
                                         C.c_void_p(stream or 0)))

    def topk_merge_rows(self, d_score, d_docno, d_tie, rows, m, k, d_out_docno, d_out_score, d_out_tie, stream=None):
        """sme_topk_merge_rows: rows x m candidates (device; d_tie may be 0) -> per
        row the best k by (score desc, tie asc, docno asc), docno -1 pads."""
        _check(lib().sme_topk_merge_rows(self._h, C.c_void_p(d_score), C.c_void_p(d_docno), C.c_void_p(d_tie or 0),
                                         rows, m, k, C.c_void_p(d_out_docno), C.c_void_p(d_out_score),
                                         C.c_void_p(d_out_tie or 0), C.c_void_p(stream or 0)))

    def count_shared_keys(self, d_rows, n, stream=None):
        """sme_count_shared_keys: (key, source rank) u64 pairs -> distinct keys
        that arrive from two or more sources."""
        cnt = C.c_int64()
        _check(lib().sme_count_shared_keys(self._h, C.c_void_p(d_rows), n, C.byref(cnt), C.c_void_p(stream or 0)))
        return cnt.value

    def merge_pieces(self, d_blobs, sizes):
        """sme_merge_pieces: the blobs one rank received from every shard (device
        memory at d_blobs, back to back, `sizes` bytes each, shard order) -> a
        records-only Index whose partitions p with p % world == rank are the
        reference's reduce output for those partitions (include/sme.h)."""
        n = len(sizes)
        arr = (C.c_uint64 * max(n, 1))(*[int(x) for x in sizes])
        h = C.c_void_p()
        _check(lib().sme_merge_pieces(self._h, C.c_void_p(d_blobs), arr, n, None, C.byref(h)))
        return Index(h, self)

    def merge(self, indexes, stream=None):
        """sme_index_merge: one full Index from 1..64 indexes of this context (built,
        loaded or merged, numbered with one docno mapping), taken in list order as
        the map tasks of one job: what one build of their corpora gives (include/sme.h).
        The inputs stay valid."""
        idx = list(indexes)
        arr = (C.c_void_p * max(len(idx), 1))(*[getattr(i, "_h", None) for i in idx])
        h = C.c_void_p()
        _check(lib().sme_index_merge(self._h, arr, len(idx), C.c_void_p(stream or 0), C.byref(h)))
        return Index(h, self)

    def build_chargram(self, corpus):
        """CharKGramTermIndexer over host bytes (k = this context's k, R = num_partitions)."""
        h = C.c_void_p()
        _check(lib().sme_build_chargram(self._h, corpus, len(corpus), C.byref(h)))
        return CharGramOutput(h, self)

    def build_chargram_device(self, d_ptr, nbytes, stream=None):
        h = C.c_void_p()
        _check(lib().sme_build_chargram_device(self._h, C.c_void_p(d_ptr), nbytes, C.c_void_p(stream or 0),
                                               C.byref(h)))
        return CharGramOutput(h, self)

    def last_build_profile(self):
        import json
        p = C.c_char_p()
        _check(lib().sme_last_build_profile(self._h, C.byref(p)))
        return json.loads(p.value.decode())

    def process_content(self, text):
        """GalagoTokenizer.processContent on the device."""
        b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        cap_tok = len(b) + 4
        buf = (C.c_ubyte * (3 * len(b) + 16))()
        offs = (C.c_int64 * (cap_tok + 1))()
        nt = C.c_int(0)
        _check(lib().sme_tokenize(self._h, b, len(b), buf, len(buf), offs, cap_tok, C.byref(nt)))
        raw = bytes(buf)
        return [_mutf8_decode(raw[offs[i]:offs[i + 1]]) for i in range(nt.value)]


class Index:
    """A built index (sme_index): reduce output + query-side CSR, resident in HBM."""

    def __init__(self, h, ctx):
        self._h, self.ctx = h, ctx
        n, v, p = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().sme_index_stats(h, C.byref(n), C.byref(v), C.byref(p)))
        self.N, self.V, self.P = n.value, v.value, p.value

    def close(self):
        if getattr(self, "_h", None):
            lib().sme_index_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def partition_records(self, part):
        """Record bytes of reduce partition `part`, always as a bytearray (one D2H
        copy into it; large partitions are not copied again into immutable bytes --
        wrap with bytes() where an immutable/hashable object is needed)."""
        offs, _ = self.serialize()
        out = bytearray(int(offs[part + 1] - offs[part]))
        self.copy_records(part, out)
        return out

    def record_docnos_ptr(self):
        """(device pointer, N): the docnos of the index's records in input order."""
        p, n = C.c_void_p(), C.c_int64()
        _check(lib().sme_index_record_docnos(self._h, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def pack_pieces(self, world, d_out=None):
        """sme_index_pack_pieces: sizes of this shard's `world` per-owner blobs
        (d_out None), or write them back to back at device address d_out."""
        arr = (C.c_uint64 * world)()
        _check(lib().sme_index_pack_pieces(self._h, int(world), C.c_void_p(d_out or 0), arr, None))
        return [int(x) for x in arr]

    def serialize(self):
        """Device serialization of every partition (once per index):
        (partition byte offsets [R+1] in the concatenated stream, k_ser_* device ms)."""
        R = self.ctx.num_partitions
        offs = (C.c_uint64 * (R + 1))()
        ms = C.c_float()
        _check(lib().sme_index_serialize(self._h, offs, C.byref(ms)))
        return np.array(offs[:], dtype=np.int64), float(ms.value)

    def copy_records(self, part, out):
        """Copy partition `part`'s records (part = -1: all partitions back to back)
        into `out` (a writable buffer: bytearray, numpy uint8 array, pinned torch
        tensor's numpy view ...) straight from HBM; returns the byte count."""
        n = C.c_size_t()
        if hasattr(out, "ctypes"):
            ptr, cap = out.ctypes.data, out.nbytes
        else:
            mv = memoryview(out)
            cap = mv.nbytes
            ptr = C.addressof((C.c_char * max(cap, 1)).from_buffer(out)) if cap else None
        _check(lib().sme_index_copy_records(self._h, part, ptr, cap, C.byref(n)))
        return n.value

    def csr(self):
        """(offsets[V+1], docno[P], tf[P], true_df[V]) in reduce-output order (tf desc, docno asc)."""
        o, d, t, f = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        _check(lib().sme_index_csr(self._h, C.byref(o), C.byref(d), C.byref(t), C.byref(f)))
        V, P = self.V, self.P

        def arr(ptr, n, dt):  # empty host vectors may hand out NULL
            return np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dt)
        return arr(o, V + 1, np.int64), arr(d, P, np.int32), arr(t, P, np.int32), arr(f, V, np.int32)

    def device_arrays(self):
        o, d, w = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().sme_index_device_arrays(self._h, C.byref(o), C.byref(d), C.byref(w)))
        return o.value, d.value, w.value

    def offsets(self):
        """int64 offsets[V+1] of the postings per term (df = np.diff)."""
        o, _, _ = self.device_arrays()
        off = np.zeros(self.V + 1, np.int64)
        _d2h(off, o, 8 * (self.V + 1))
        return off

    def term_fingerprints(self, d_out, stream=None):
        """128-bit fingerprint per term into device memory d_out (uint64 [V, 2])."""
        _check(lib().sme_index_term_fingerprints(self._h, C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def weights(self):
        """Host copies of the query-side CSR and the TF-IDF weight pass's output:
        (offsets[V+1], docno[P] docno-ascending per term, w[P] fp64)."""
        o, d, w = self.device_arrays()
        V, P = self.V, self.P
        off = np.zeros(V + 1, np.int64)
        dn = np.zeros(max(P, 1), np.int32)
        ws = np.zeros(max(P, 1), np.float64)
        _d2h(off, o, 8 * (V + 1))
        if P:
            _d2h(dn, d, 4 * P)
            _d2h(ws, w, 8 * P)
        return off, dn[:P], ws[:P]

    def term(self, t):
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().sme_index_term(self._h, t, C.byref(p), C.byref(n)))
        return _mutf8_decode(C.string_at(p, n.value))

    def terms(self):
        return [self.term(t) for t in range(self.V)]

    def lookup(self, terms):
        bs = [t.encode("utf-8", "surrogatepass") for t in terms]
        offs = np.zeros(len(bs) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(b) for b in bs]) if bs else []
        ids = np.zeros(max(len(bs), 1), dtype=np.int32)
        _check(lib().sme_lookup_terms(self._h, b"".join(bs), offs.ctypes.data_as(C.POINTER(C.c_int64)), len(bs),
                                      ids.ctypes.data_as(C.POINTER(C.c_int32))))
        return ids[:len(bs)]

    def query_topk(self, term_ids, q_offsets, k=10, with_tie=False):
        """Batched rank(): returns (docno[nq,k], score[nq,k]); docno -1 pads.
        with_tie: also the uint32 tie word of every result (sme_query_topk_tie),
        the key doc-shard merges need under SME_TIE_REFERENCE."""
        term_ids = np.ascontiguousarray(term_ids, dtype=np.int32)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64)
        nq = len(q_offsets) - 1
        dn = np.zeros((max(nq, 1), k), dtype=np.int32)
        sc = np.zeros((max(nq, 1), k), dtype=np.float64)
        args = [self._h, term_ids.ctypes.data_as(C.POINTER(C.c_int32)), q_offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                nq, k, dn.ctypes.data_as(C.POINTER(C.c_int32)), sc.ctypes.data_as(C.POINTER(C.c_double))]
        if not with_tie:
            _check(lib().sme_query_topk(*args))
            return dn[:nq], sc[:nq]
        tie = np.zeros((max(nq, 1), k), dtype=np.uint32)
        _check(lib().sme_query_topk_tie(*args, tie.ctypes.data_as(C.POINTER(C.c_uint32))))
        return dn[:nq], sc[:nq], tie[:nq]

    def prepare_queries(self, stream=None):
        """Build the query-side heavy rows now (else the first query batch does);
        returns their device build time in ms."""
        ms = C.c_float(0.0)
        _check(lib().sme_index_prepare_queries(self._h, C.c_void_p(stream or 0), C.byref(ms)))
        return ms.value

    def prepare_wildcards(self, stream=None):
        """Build the vocabulary's character-trigram table now (else the first
        expansion does); returns its device build time in ms."""
        ms = C.c_float(0.0)
        _check(lib().sme_index_prepare_wildcards(self._h, C.c_void_p(stream or 0), C.byref(ms)))
        return ms.value

    # ---- the batched query features: n queries in, n + 1 offsets and one to four
    # value columns out (include/sme.h).  The four patterns below are each written
    # once; a feature names its entry, its input dtypes and its column dtypes.
    _CT = {np.int32: C.c_int32, np.int64: C.c_int64, np.uint8: C.c_uint8, np.float64: C.c_double, np.int8: C.c_int8,
           np.uint64: C.c_uint64}

    @staticmethod
    def _typed_ptrs(arrays, dtypes):
        """(the arrays to keep alive, their ctypes pointers): contiguous, of the
        given dtypes, and never empty (an empty numpy array may hand out any
        pointer: one element is kept behind each)."""
        keep, ptrs = [], []
        for a, dt in zip(arrays, dtypes):
            a = np.ascontiguousarray(a, dtype=dt)
            a = a if a.size else np.zeros(1, dt)
            keep.append(a)
            ptrs.append(a.ctypes.data_as(C.POINTER(Index._CT[dt])))
        return keep, ptrs

    @staticmethod
    def _host_call(h, fn, args, n, cols):
        """fn(index, *args, &offsets, &column...) -> (offsets int64[n+1], one array
        per dtype of cols), copied at once: the library's arrays are the index's
        until the feature's next call.  An empty column is np.zeros(0, dt)."""
        outs = [C.POINTER(Index._CT[dt])() for dt in (np.int64,) + cols]
        _check(fn(h, *args, *[C.byref(o) for o in outs]))
        off = np.ctypeslib.as_array(outs[0], (n + 1,)).copy()
        total = int(off[n])
        return (off,) + tuple(np.ctypeslib.as_array(o, (total,)).copy() if total else np.zeros(0, dt)
                              for o, dt in zip(outs[1:], cols))

    @staticmethod
    def _device_call(h, fn, args, stream, cols):
        """fn(index, *args, stream, &offsets, &column..., &total) -> (device pointer
        of the offsets, of every column, total); a NULL pointer is 0."""
        outs = [C.c_void_p() for _ in range(len(cols) + 1)]
        tot = C.c_int64()
        _check(fn(h, *args, C.c_void_p(stream or 0), *[C.byref(o) for o in outs], C.byref(tot)))
        return tuple(o.value or 0 for o in outs) + (tot.value,)

    @staticmethod
    def _query_host(h, fn, arrays, dtypes, nq, order, m, cols):
        """_host_call over a batch of nq queries given as its arrays."""
        keep, ptrs = Index._typed_ptrs(arrays, dtypes)
        return Index._host_call(h, fn, ptrs + [nq, int(order), int(m)], nq, cols)

    @staticmethod
    def _query_device(h, fn, arrays, dtypes, nq, order, m, stream, cols):
        """_device_call over a batch of nq queries given as its arrays."""
        keep, ptrs = Index._typed_ptrs(arrays, dtypes)
        return Index._device_call(h, fn, ptrs + [nq, int(order), int(m)], stream, cols)

    @staticmethod
    def _stats(h, fn, count):
        """fn(index, &uint64...) -> the `count` values."""
        vals = [C.c_uint64() for _ in range(count)]
        _check(fn(h, *[C.byref(v) for v in vals]))
        return tuple(v.value for v in vals)

    _TERM_COLS, _SUGGEST_COLS = (np.int32,), (np.int32, np.uint8)
    _DOC_COLS, _PASS_COLS = (np.int32, np.float64), (np.int32, np.int32, np.float64)
    _BOOLEAN_IN = (np.int32, np.int64, np.uint8, np.int64)
    _PHRASE_IN = (np.int32, np.int64)
    _NEAR_IN = (np.int32, np.int64, np.int32, np.uint8)
    _STRUCTURED_IN = (np.int32, np.int64, np.uint8, np.int32, np.int64, np.uint8, np.int64)

    def wildcard_stats(self):
        """(distinct trigram keys, distinct (key, term) pairs) of the wildcard table."""
        return Index._stats(self._h, lib().sme_index_wildcard_stats, 2)

    @staticmethod
    def _pattern_args(patterns):
        """(the offsets array to keep alive, (blob, offsets pointer, n)) of str / bytes patterns."""
        bs = [p if isinstance(p, (bytes, bytearray)) else p.encode("utf-8", "surrogatepass") for p in patterns]
        offs = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            offs[1:] = np.cumsum([len(b) for b in bs])
        return offs, (b"".join(bs), offs.ctypes.data_as(C.POINTER(C.c_int64)), len(bs))

    def expand_wildcards(self, patterns):
        """sme_index_expand_wildcards: patterns (str, or bytes of UTF-8) -> (match_off
        int64[n+1], term_ids int32); pattern i matches term_ids[match_off[i]:
        match_off[i+1]], ascending.  '*' = any run of UTF-16 units, '?' = one unit;
        no case folding (include/sme.h)."""
        keep, args = Index._pattern_args(patterns)
        return Index._host_call(self._h, lib().sme_index_expand_wildcards, args, args[2], Index._TERM_COLS)

    def expand_wildcards_device(self, patterns, stream=None):
        """sme_index_expand_wildcards_device: (device pointer of match_off int64[n+1],
        device pointer of term_ids int32[total], total); the arrays belong to the
        index until its next expansion."""
        keep, args = Index._pattern_args(patterns)
        return Index._device_call(self._h, lib().sme_index_expand_wildcards_device, args, stream, Index._TERM_COLS)

    def suggest_terms(self, words, max_dist=2, m=10):
        """sme_index_suggest_terms: words (str, or bytes of UTF-8) -> (sug_off
        int64[n+1], term_ids int32, dist uint8); word i's suggestions are
        term_ids[sug_off[i]:sug_off[i+1]], the terms within max_dist (0..3) unit
        edits of it ordered by (distance asc, df desc, term id asc) and cut to the
        first m (0: no cut); dist runs parallel to term_ids (include/sme.h)."""
        keep, args = Index._pattern_args(words)
        return Index._host_call(self._h, lib().sme_index_suggest_terms, args + (int(max_dist), int(m)), args[2],
                               Index._SUGGEST_COLS)

    def suggest_terms_device(self, words, max_dist=2, m=10, stream=None):
        """sme_index_suggest_terms_device: (device pointer of sug_off int64[n+1],
        of term_ids int32[total], of dist uint8[total], total); the arrays belong
        to the index until its next suggestion call."""
        keep, args = Index._pattern_args(words)
        return Index._device_call(self._h, lib().sme_index_suggest_terms_device, args + (int(max_dist), int(m)), stream,
                                 Index._SUGGEST_COLS)

    def suggest_stats(self):
        """(scanned_words, candidates) of the last suggestion call: the words that
        took the whole vocabulary as candidates, and the (word, term) pairs that
        reached the length test."""
        return Index._stats(self._h, lib().sme_index_suggest_stats, 2)

    @staticmethod
    def boolean_arrays(queries):
        """The C-ABI's three-level structure of a list of queries, each a list of
        (term_ids, excluded) groups: (term_ids int32, g_offsets int64[ngroups+1],
        g_flags uint8[ngroups], q_offsets int64[nq+1])."""
        terms, goff, flags, qoff = [], [0], [], [0]
        for groups in queries:
            for ids, excluded in groups:
                terms.extend(int(t) for t in ids)
                goff.append(len(terms))
                flags.append(int(excluded))
            qoff.append(len(flags))
        return (np.array(terms, np.int32), np.array(goff, np.int64), np.array(flags, np.uint8),
                np.array(qoff, np.int64))

    def query_boolean(self, queries, order=0, m=0, arrays=None):
        """sme_query_boolean: queries = a list of queries, each a list of
        (term_ids, excluded) groups -- a document matches when it lies in at least
        one posting list of every required group and in none of an excluded one;
        term id -1 is an empty list.  Returns (res_off int64[nq+1], docno int32,
        score float64): query i's matches are [res_off[i], res_off[i+1]), the
        score the fp64 sum of the weights over the required slots in listed order,
        ordered by docno ascending (order 0) or score descending then docno
        ascending (order 1) and cut to the first m (0: no cut) (include/sme.h).
        arrays: the structure as boolean_arrays returns it, instead of queries."""
        a = arrays if arrays is not None else Index.boolean_arrays(queries)
        return Index._query_host(self._h, lib().sme_query_boolean, a, Index._BOOLEAN_IN, len(a[3]) - 1,
                                 order, m, Index._DOC_COLS)

    def query_boolean_device(self, queries, order=0, m=0, stream=None, arrays=None):
        """sme_query_boolean_device: (device pointer of res_off int64[nq+1], of
        docno int32[total], of score float64[total], total); the arrays belong to
        the index until its next Boolean call."""
        a = arrays if arrays is not None else Index.boolean_arrays(queries)
        return Index._query_device(self._h, lib().sme_query_boolean_device, a, Index._BOOLEAN_IN, len(a[3]) - 1,
                                   order, m, stream, Index._DOC_COLS)

    def boolean_stats(self):
        """(candidates, matches) of the last Boolean call: the driver postings
        examined, and the matches before the cut."""
        return Index._stats(self._h, lib().sme_query_boolean_stats, 2)

    def positions(self):
        """sme_index_positions: (records, positions, bytes) of the term streams the
        index keeps for phrase queries -- all zero unless it is a K = 1 index built
        with Context.set_option("positions", 1)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().sme_index_positions(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    @staticmethod
    def phrase_arrays(phrases):
        """The C-ABI's structure of a list of phrases, each a list of term ids:
        (term_ids int32, p_offsets int64[np+1])."""
        terms, poff = [], [0]
        for ph in phrases:
            terms.extend(int(t) for t in ph)
            poff.append(len(terms))
        return np.array(terms, np.int32), np.array(poff, np.int64)

    def query_phrase(self, phrases, order=0, m=0, arrays=None):
        """sme_query_phrase: phrases = a list of phrases, each a list of term ids
        (Index.lookup's; -1 = unknown, the phrase then has no result).  A document
        matches a phrase when a record of it holds the terms at consecutive
        positions; freq counts those places (overlaps included, summed over the
        docno's records), score = (1 + ln freq) * idf(matching documents), the
        weight a K = len(phrase) index gives that gram.  Returns (res_off
        int64[np+1], docno int32, freq int32, score float64): phrase i's matches
        are [res_off[i], res_off[i+1]), by docno ascending (order 0) or score
        descending then docno ascending (order 1), cut to the first m (0: no cut)
        (include/sme.h).  The index must keep positions (Index.positions).
        arrays: the structure as phrase_arrays returns it, instead of phrases."""
        a = arrays if arrays is not None else Index.phrase_arrays(phrases)
        return Index._query_host(self._h, lib().sme_query_phrase, a, Index._PHRASE_IN, len(a[1]) - 1,
                                 order, m, Index._PASS_COLS)

    def query_phrase_device(self, phrases, order=0, m=0, stream=None, arrays=None):
        """sme_query_phrase_device: (device pointer of res_off int64[np+1], of docno
        int32[total], of freq int32[total], of score float64[total], total); the
        arrays belong to the index until its next phrase call."""
        a = arrays if arrays is not None else Index.phrase_arrays(phrases)
        return Index._query_device(self._h, lib().sme_query_phrase_device, a, Index._PHRASE_IN, len(a[1]) - 1,
                                   order, m, stream, Index._PASS_COLS)

    def phrase_stats(self):
        """(candidates, verified, matches) of the last phrase call: the driver
        postings examined, the (phrase, document) pairs whose records were
        scanned, and the matches before the cut."""
        return Index._stats(self._h, lib().sme_query_phrase_stats, 3)

    @staticmethod
    def near_arrays(queries):
        """The C-ABI's structure of a list of proximity queries, each (term_ids,
        width, ordered): (term_ids int32, q_offsets int64[nq+1], widths int32[nq],
        kinds uint8[nq]; kind 0 = ordered window, 1 = unordered)."""
        terms, qoff, widths, kinds = [], [0], [], []
        for ids, width, ordered in queries:
            terms.extend(int(t) for t in ids)
            qoff.append(len(terms))
            widths.append(int(width))
            kinds.append(0 if ordered else 1)
        return (np.array(terms, np.int32), np.array(qoff, np.int64), np.array(widths, np.int32),
                np.array(kinds, np.uint8))

    def query_near(self, queries, order=0, m=0, arrays=None):
        """sme_query_near: queries = a list of (term_ids, width, ordered), the ids
        Index.lookup's (-1 = unknown, the query then has no result), at most 32.
        ordered: every next term stands at most `width` positions after the
        previous one (#od:width; width 1 is the exact phrase), freq = the distinct
        end positions of such chains.  Not ordered: the set of the distinct terms
        within `width` positions (#uw:width), freq = the positions of a query term
        whose window of `width` positions ending there holds them all.  Within
        one record, summed over the docno's records; score = (1 + ln freq) *
        idf(matching documents).  Returns (res_off int64[nq+1], docno int32, freq
        int32, score float64), ordered and cut as query_phrase's (include/sme.h).
        The index must keep positions (Index.positions).
        arrays: the structure as near_arrays returns it, instead of queries."""
        a = arrays if arrays is not None else Index.near_arrays(queries)
        return Index._query_host(self._h, lib().sme_query_near, a, Index._NEAR_IN, len(a[1]) - 1,
                                 order, m, Index._PASS_COLS)

    def query_near_device(self, queries, order=0, m=0, stream=None, arrays=None):
        """sme_query_near_device: (device pointer of res_off int64[nq+1], of docno
        int32[total], of freq int32[total], of score float64[total], total); the
        arrays belong to the index until its next proximity call."""
        a = arrays if arrays is not None else Index.near_arrays(queries)
        return Index._query_device(self._h, lib().sme_query_near_device, a, Index._NEAR_IN, len(a[1]) - 1,
                                   order, m, stream, Index._PASS_COLS)

    def near_stats(self):
        """(candidates, verified, matches) of the last proximity call: the driver
        postings examined, the (query, document) pairs whose records were
        scanned, and the matches before the cut."""
        return Index._stats(self._h, lib().sme_query_near_stats, 3)

    @staticmethod
    def structured_arrays(queries):
        """The C-ABI's four-level structure of a list of queries, each a list of
        (leaves, excluded) groups, a leaf being (term_ids, kind, width) -- kind 0 a
        term (one id; the width is not read), 1 the ordered window #od:width, 2 the
        unordered window #uw:width: (term_ids int32, l_offsets int64[nleaves+1],
        l_kinds uint8[nleaves], l_widths int32[nleaves], g_offsets
        int64[ngroups+1], g_flags uint8[ngroups], q_offsets int64[nq+1])."""
        terms, loff, kinds, widths, goff, flags, qoff = [], [0], [], [], [0], [], [0]
        for groups in queries:
            for leaves, excluded in groups:
                for ids, kind, width in leaves:
                    terms.extend(int(t) for t in ids)
                    loff.append(len(terms))
                    kinds.append(int(kind))
                    widths.append(int(width))
                goff.append(len(kinds))
                flags.append(int(excluded))
            qoff.append(len(flags))
        return (np.array(terms, np.int32), np.array(loff, np.int64), np.array(kinds, np.uint8),
                np.array(widths, np.int32), np.array(goff, np.int64), np.array(flags, np.uint8),
                np.array(qoff, np.int64))

    def query_structured(self, queries, order=0, m=0, arrays=None):
        """sme_query_structured: queries = a list of queries, each a list of
        (leaves, excluded) groups; a leaf is (term_ids, kind, width): kind 0 a term
        (one id, -1 = an empty list), kind 1 the ordered window #od:width (width 1:
        the phrase), kind 2 the unordered window #uw:width, over at most 32 ids.
        A leaf's document list is the term's postings, or what query_near returns
        for the window; a document matches by query_boolean's rules over those
        lists, and its score is the fp64 sum, in listed order, of the required
        leaves' values -- the term's weight, the window's query_near score.
        Returns (res_off int64[nq+1], docno int32, score float64), ordered and
        cut as query_boolean's (include/sme.h).  A batch with a window needs an
        index that keeps positions (Index.positions).
        arrays: the structure as structured_arrays returns it, instead of queries."""
        a = arrays if arrays is not None else Index.structured_arrays(queries)
        return Index._query_host(self._h, lib().sme_query_structured, a, Index._STRUCTURED_IN, len(a[6]) - 1,
                                 order, m, Index._DOC_COLS)

    def query_structured_device(self, queries, order=0, m=0, stream=None, arrays=None):
        """sme_query_structured_device: (device pointer of res_off int64[nq+1], of
        docno int32[total], of score float64[total], total); the arrays belong to
        the index until its next structured call."""
        a = arrays if arrays is not None else Index.structured_arrays(queries)
        return Index._query_device(self._h, lib().sme_query_structured_device, a, Index._STRUCTURED_IN, len(a[6]) - 1,
                                   order, m, stream, Index._DOC_COLS)

    def structured_stats(self):
        """(leaves, verified, candidates, matches) of the last structured call: the
        operator leaves evaluated, the (leaf, document) pairs whose records were
        scanned, the Boolean stage's driver entries examined, and the matches
        before the cut."""
        return Index._stats(self._h, lib().sme_query_structured_stats, 4)

    _FEEDBACK_COLS = (np.int32, np.int32, np.int32, np.float64)

    @staticmethod
    def _feedback_args(f_offsets, exclude, m, min_docs, min_df, max_df):
        """(arrays to keep alive, the C-ABI's arguments after the docnos): the set
        offsets, and the exclusion lists -- None, a list of id lists (one per set)
        or (x_ids, x_offsets) arrays -- as NULL or typed pointers."""
        nq = len(f_offsets) - 1
        keep, (foff,) = Index._typed_ptrs([f_offsets], (np.int64,))
        xid = xoff = None
        if exclude is not None:
            a = exclude if isinstance(exclude, tuple) else Index.phrase_arrays(exclude)
            k2, (xid, xoff) = Index._typed_ptrs(a, (np.int32, np.int64))
            keep += k2
        return keep, [foff, nq, xid, xoff, int(m), int(min_docs), int(min_df), int(max_df)]

    def feedback_terms(self, doc_sets, m=20, min_docs=1, min_df=2, max_df=0, exclude=None, arrays=None):
        """sme_index_feedback_terms: doc_sets = a list of docno lists.  Per set,
        the terms of those documents' kept streams with freq (occurrences over
        the set) and docs (the set's documents holding the term), kept if docs >=
        min_docs, min_df <= df <= max_df (the index's own df; max_df 0: no upper
        bound) and not among the set's `exclude` ids, scored (1 + ln freq) * idf,
        ordered by score descending then term id ascending and cut to the first m
        (0: no cut).  A docno of -1 is skipped, a repeated one counts once, one
        without a record contributes nothing (include/sme.h).  Returns (res_off
        int64[n+1], term int32, freq int32, docs int32, score float64).  The
        index must keep positions (Index.positions).
        exclude: a list of term id lists, one per set, or (x_ids, x_offsets).
        arrays: (docnos int32, f_offsets int64[n+1]) instead of doc_sets."""
        docnos, foff = arrays if arrays is not None else Index.phrase_arrays(doc_sets)
        keep, (dn,) = Index._typed_ptrs([docnos], (np.int32,))
        keep2, rest = Index._feedback_args(foff, exclude, m, min_docs, min_df, max_df)
        return Index._host_call(self._h, lib().sme_index_feedback_terms, [dn] + rest, len(foff) - 1,
                                Index._FEEDBACK_COLS)

    def feedback_terms_device(self, d_docnos, f_offsets, m=20, min_docs=1, min_df=2, max_df=0, exclude=None,
                              stream=None):
        """sme_index_feedback_terms_device: d_docnos = a device pointer of int32
        docnos, or a contiguous int32 device tensor (anything with data_ptr()) --
        query_topk_device's output as it stands --, f_offsets the host
        int64[n+1] offsets of the sets in it.  Returns (device pointer of res_off
        int64[n+1], of term, freq, docs int32[total], of score float64[total],
        total); the arrays belong to the index until its next feedback call."""
        keep, rest = Index._feedback_args(f_offsets, exclude, m, min_docs, min_df, max_df)
        if hasattr(d_docnos, "data_ptr"):  # a contiguous int32 device tensor
            d_docnos = d_docnos.data_ptr()
        return Index._device_call(self._h, lib().sme_index_feedback_terms_device, [C.c_void_p(d_docnos or 0)] + rest,
                                  stream, Index._FEEDBACK_COLS)

    def feedback_stats(self):
        """(positions, pairs, kept, missing, spilled) of the last feedback call: the
        stream positions of the sets' documents, the (set, term) pairs before the
        filters, the pairs kept before the cut, the sets' docnos without a
        record, and the sets that took the large path ("fb_slots")."""
        return Index._stats(self._h, lib().sme_index_feedback_stats, 5)

    def query_feedback(self, term_ids, q_offsets, k=10, fb_docs=10, fb_terms=20, **filters):
        """Pseudo-relevance feedback: query_topk with k = fb_docs, on the device;
        feedback_terms_device over those documents, each query's own terms
        excluded (m = fb_terms; filters: min_docs, min_df, max_df); the expansion
        terms appended to each query; query_topk of the expanded queries with the
        original k.  Returns (docno[nq,k], score[nq,k], expanded_term_ids,
        expanded_offsets).  fb_terms = 0 expands nothing: plain query_topk."""
        term_ids = np.ascontiguousarray(term_ids, dtype=np.int32)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64)
        nq = len(q_offsets) - 1
        if nq == 0 or fb_terms <= 0 or fb_docs <= 0:
            dn, sc = self.query_topk(term_ids, q_offsets, k)
            return dn, sc, term_ids, q_offsets
        L, dev = lib(), self.ctx.device
        bufs = []

        def dalloc(nbytes):
            p = C.c_void_p()
            _check(L.sme_device_alloc(dev, max(nbytes, 16), C.byref(p)))
            bufs.append(p)
            return p.value
        try:
            d_t, d_q = dalloc(term_ids.nbytes), dalloc(q_offsets.nbytes)
            d_dn, d_sc = dalloc(4 * nq * fb_docs), dalloc(8 * nq * fb_docs)
            if term_ids.size:
                memcpy(d_t, term_ids.ctypes.data, term_ids.nbytes)
            memcpy(d_q, q_offsets.ctypes.data, q_offsets.nbytes)
            self.query_topk_device(d_t, d_q, nq, fb_docs, d_dn, d_sc)
            foff = np.arange(nq + 1, dtype=np.int64) * fb_docs
            d_off, d_term, _, _, _, total = self.feedback_terms_device(d_dn, foff, m=fb_terms,
                                                                       exclude=(term_ids, q_offsets), **filters)
            off, terms = np.zeros(nq + 1, np.int64), np.zeros(max(total, 1), np.int32)
            _d2h(off, d_off, off.nbytes)
            if total:
                _d2h(terms, d_term, 4 * total)
        finally:
            for p in bufs:
                L.sme_device_free(p)
        parts, xoff = [], [0]
        for i in range(nq):
            parts += [term_ids[q_offsets[i]:q_offsets[i + 1]], terms[off[i]:off[i + 1]]]
            xoff.append(xoff[-1] + len(parts[-2]) + len(parts[-1]))
        expanded, xoff = np.concatenate(parts).astype(np.int32), np.array(xoff, np.int64)
        dn, sc = self.query_topk(expanded, xoff, k)
        return dn, sc, expanded, xoff

    def merge_stats(self):
        """sme_index_merge_stats: of a merged index its inputs, the terms two or more
        inputs held, the postings equal docnos merged away and whether the
        concatenation path ran; zeros for any other index."""
        i, s, m, a = self._stats(self._h, lib().sme_index_merge_stats, 4)
        return {"inputs": i, "shared_terms": s, "merged_postings": m, "appended": a}

    def delete_docnos(self, docnos, stream=None):
        """sme_index_delete_docnos: a new full Index without the records whose docno
        is in `docnos` (any order, duplicates and absent docnos allowed) -- in every
        array what one build of the remaining documents gives (include/sme.h).  This
        index stays valid."""
        d = np.ascontiguousarray(np.asarray(docnos, dtype=np.int32).reshape(-1))
        ptr = d.ctypes.data_as(C.POINTER(C.c_int32)) if d.size else None
        h = C.c_void_p()
        _check(lib().sme_index_delete_docnos(self._h, ptr, d.size, C.c_void_p(stream or 0), C.byref(h)))
        return Index(h, self.ctx)

    def delete_docnos_device(self, d_docnos, n, stream=None):
        """sme_index_delete_docnos_device: as delete_docnos, the n int32 docnos in device
        memory at d_docnos -- a device result (query_boolean_device's docnos, say)
        without a round trip."""
        h = C.c_void_p()
        _check(lib().sme_index_delete_docnos_device(self._h, C.c_void_p(d_docnos or 0), int(n), C.c_void_p(stream or 0),
                                                    C.byref(h)))
        return Index(h, self.ctx)

    def delete_stats(self):
        """sme_index_delete_stats: of an index delete_docnos made the distinct listed
        docnos some record had, and the records, postings and terms removed; zeros
        for any other index."""
        d, r, p, t = self._stats(self._h, lib().sme_index_delete_stats, 4)
        return {"docnos": d, "records": r, "postings": p, "terms": t}

    ATTACH_NO_CROSSCHECK = 1  # SME_ATTACH_NO_CROSSCHECK

    def positions_file(self, bits=0, stream=None):
        """sme_index_positions_file: the term streams this index keeps (positions) as
        the bytes of a positions file (include/sme.h has the format), written on the
        device; bits 0 = the narrowest id width, else a width up to 31.  Another
        index of the same documents and vocabulary -- one opened from its part
        files, say -- takes them back with attach_positions."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().sme_index_positions_file(self._h, int(bits), C.c_void_p(stream or 0), C.byref(p), C.byref(n)))
        return _host_bytes(p.value, n.value)

    def positions_file_device(self, bits=0, stream=None):
        """sme_index_positions_file_device: (device pointer, byte count) of the same
        file, left in HBM; it belongs to the index until its next posfile call."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().sme_index_positions_file_device(self._h, int(bits), C.c_void_p(stream or 0), C.byref(p),
                                                     C.byref(n)))
        return p.value, n.value

    def attach_positions(self, data, crosscheck=True, stream=None):
        """sme_index_attach_positions: give this K = 1 index, which keeps no positions,
        the term streams of a positions file (bytes-like).  The file is checked against
        its header, this index's vocabulary and, with crosscheck, every posting's tf; a
        refused file (SmeError, code -4) leaves the index as it was.  Afterwards phrase,
        proximity, structured and feedback calls and merges treat it as built with
        positions."""
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(0, np.uint8)
        keep = np.ascontiguousarray(buf) if buf.size else np.zeros(1, np.uint8)
        _check(lib().sme_index_attach_positions(self._h, C.c_void_p(keep.ctypes.data), buf.size,
                                                0 if crosscheck else Index.ATTACH_NO_CROSSCHECK,
                                                C.c_void_p(stream or 0)))

    def attach_positions_device(self, d_file, nbytes, crosscheck=True, stream=None):
        """sme_index_attach_positions_device: as attach_positions, the file's nbytes in
        device memory at d_file (8-byte aligned)."""
        _check(lib().sme_index_attach_positions_device(self._h, C.c_void_p(d_file or 0), int(nbytes),
                                                       0 if crosscheck else Index.ATTACH_NO_CROSSCHECK,
                                                       C.c_void_p(stream or 0)))

    def posfile_stats(self):
        """sme_index_posfile_stats: of the last positions_file / attach_positions call
        on this index the file's bytes and id width, the postings the cross-check
        compared, and the device times of the encode kernel, the decode kernel and the
        cross-check (ms; zero for what the call did not run)."""
        u = [C.c_uint64() for _ in range(3)]
        f = [C.c_float() for _ in range(3)]
        _check(lib().sme_index_posfile_stats(self._h, *[C.byref(x) for x in u + f]))
        return {"file_bytes": u[0].value, "bits": u[1].value, "checked_postings": u[2].value,
                "encode_ms": f[0].value, "decode_ms": f[1].value, "crosscheck_ms": f[2].value}

    # ---- BM25 ranking (include/sme.h, sme_query_topk_bm25)
    def prepare_bm25(self, stream=None):
        """Build the BM25 tables (document lengths, idf by true df, the bound tables)
        now (else the first BM25 call does); returns their device build time in ms."""
        ms = C.c_float(0.0)
        _check(lib().sme_index_prepare_bm25(self._h, C.c_void_p(stream or 0), C.byref(ms)))
        return ms.value

    def doc_lengths_device(self, stream=None):
        """(device pointer of int32 dl[docno - dmin], dmin, span): the index's own array."""
        p, dmin, span = C.c_void_p(), C.c_int64(), C.c_int64()
        _check(lib().sme_index_doc_lengths(self._h, C.c_void_p(stream or 0), C.byref(p), C.byref(dmin), C.byref(span)))
        return p.value or 0, dmin.value, span.value

    def doc_lengths(self):
        """(dmin, np.int32[span]): dl[docno - dmin], the sum of tf over the document's
        postings, 0 for a docno without postings."""
        p, dmin, span = self.doc_lengths_device()
        dl = np.zeros(span, np.int32)
        if span:
            _d2h(dl, p, 4 * span)
        return dmin, dl

    def bm25_stats(self):
        """{"docs": D, "total_len": L, "max_len", "window": documents per scorer window}."""
        d, t, m, w = Index._stats(self._h, lib().sme_index_bm25_stats, 4)
        return {"docs": d, "total_len": t, "max_len": m, "window": w}

    def query_bm25(self, term_ids, q_offsets, k=10, k1=1.2, b=0.75):
        """Batched BM25 ranking, laid out as query_topk: (docno[nq,k], score[nq,k]) by
        score descending then docno ascending; docno -1 / score 0.0 pad."""
        term_ids = np.ascontiguousarray(term_ids, dtype=np.int32)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64)
        nq = len(q_offsets) - 1
        rows = max(nq, 1) * max(int(k), 1)
        dn = np.zeros(rows, dtype=np.int32)
        sc = np.zeros(rows, dtype=np.float64)
        keep, ptrs = Index._typed_ptrs([term_ids, q_offsets], (np.int32, np.int64))
        _check(lib().sme_query_topk_bm25(self._h, ptrs[0], ptrs[1], nq, int(k), float(k1), float(b),
                                         dn.ctypes.data_as(C.POINTER(C.c_int32)),
                                         sc.ctypes.data_as(C.POINTER(C.c_double))))
        return dn[:nq * k].reshape(nq, k), sc[:nq * k].reshape(nq, k)

    def query_bm25_device(self, d_terms, d_qoff, nq, k, d_out_docno, d_out_score, k1=1.2, b=0.75, stream=None):
        """query_bm25 with every array in device memory (query_topk_device's layout)."""
        _check(lib().sme_query_topk_bm25_device(self._h, C.c_void_p(d_terms), C.c_void_p(d_qoff), nq, int(k),
                                                float(k1), float(b), C.c_void_p(d_out_docno),
                                                C.c_void_p(d_out_score), C.c_void_p(stream or 0)))

    def query_bm25_stats(self):
        """The last BM25 call: {"windows": (query, window) pairs that held a posting,
        "skipped": those the bound skipped, "postings": postings scored}."""
        w, s, p = Index._stats(self._h, lib().sme_query_bm25_stats, 3)
        return {"windows": w, "skipped": s, "postings": p}

    # ---- scoring given documents (include/sme.h, sme_query_rescore)
    _MODELS = {"tfidf": 0, "bm25": 1, 0: 0, 1: 1}

    @staticmethod
    def _rescore_tail(model, k1, b, min_hits, order, m):
        if model not in Index._MODELS:
            raise ValueError("model must be \"tfidf\" or \"bm25\" (or 0 / 1), not %r" % (model,))
        return [Index._MODELS[model], float(k1), float(b), int(min_hits), int(order), int(m)]

    def rescore(self, term_ids, q_offsets, docnos, d_offsets, model="bm25", order=1, m=0, min_hits=0, k1=1.2,
                b=0.75):
        """sme_query_rescore: query i's term slots term_ids[q_offsets[i]:q_offsets[i+1]]
        over its candidates docnos[d_offsets[i]:d_offsets[i+1]], strictly ascending --
        what order 0 of query_boolean / _phrase / _near / _structured returns.  Every
        candidate gets its score under `model` ("tfidf": the sum query_boolean
        documents; "bm25": query_bm25's weights with k1, b) and hits, the slots whose
        posting list holds it; those with hits >= min_hits are the matches, in the
        given order (order 0) or by score descending then docno ascending (order
        1), cut to the first m (0: no cut).  Returns (res_off int64[nq+1], docno
        int32, hits int32, score float64) (include/sme.h)."""
        a = [term_ids, q_offsets, docnos, d_offsets]
        keep, ptrs = Index._typed_ptrs(a, (np.int32, np.int64, np.int32, np.int64))
        nq = len(keep[1]) - 1
        return Index._host_call(self._h, lib().sme_query_rescore,
                                ptrs + [nq] + Index._rescore_tail(model, k1, b, min_hits, order, m), nq,
                                Index._PASS_COLS)

    def rescore_device(self, term_ids, q_offsets, d_docnos, d_doc_offsets, model="bm25", order=1, m=0, min_hits=0,
                       k1=1.2, b=0.75, stream=None):
        """sme_query_rescore_device: the candidates and their nq + 1 offsets in device
        memory (pointers, or contiguous int32 / int64 device tensors) -- the docno
        and res_off pointers of another feature's device call as they stand; the
        term slots and their offsets are host arrays.  Returns (device pointer of
        res_off int64[nq+1], of docno, hits int32[total], of score float64[total],
        total); the arrays belong to the index until its next rescore call."""
        keep, ptrs = Index._typed_ptrs([term_ids, q_offsets], (np.int32, np.int64))
        nq = len(keep[1]) - 1
        dev = [C.c_void_p((x.data_ptr() if hasattr(x, "data_ptr") else x) or 0) for x in (d_docnos, d_doc_offsets)]
        return Index._device_call(self._h, lib().sme_query_rescore_device,
                                  ptrs + dev + [nq] + Index._rescore_tail(model, k1, b, min_hits, order, m), stream,
                                  Index._PASS_COLS)

    def rescore_stats(self):
        """The last rescore call: {"candidates": the batch's candidates, "found": the
        sum of hits, "matches": the matches before the cut, "tile": candidates per
        workgroup of the scorer}."""
        c, f, mt, t = Index._stats(self._h, lib().sme_query_rescore_stats, 4)
        return {"candidates": c, "found": f, "matches": mt, "tile": t}

    # ---- best passages (include/sme.h, sme_query_passages)
    _PASSAGE_DTYPES = (np.int64, np.int32, np.int32, np.int32, np.int32, np.int32, np.uint64, np.float64, np.int64,
                       np.int32, np.int8)

    def passages(self, term_ids, q_offsets, docnos, d_offsets, width, min_cover=0, order=0, m=0, with_terms=False):
        """sme_query_passages: for query i's term ids term_ids[q_offsets[i]:q_offsets[i+1]]
        and each of its candidates docnos[d_offsets[i]:d_offsets[i+1]], strictly
        ascending, the best window of at most `width` (1..256) consecutive positions of
        one of the document's records: -1 dropped and repeats folded, the j-th distinct
        id is slot j; a window's mask ORs the slots it holds, hits counts the matching
        positions, score sums the covered slots' idfs; the best is the first by score,
        cover, hits descending, then rec, start ascending.  Candidates covering
        min_cover slots or more are kept, in the given order (order 0) or by score
        descending then docno ascending (order 1), cut to the first m (0: no cut).
        Returns Passages(res_off int64[nq+1], docno, rec, start, len, hits int32, mask
        uint64, score float64, win_off, win_term, win_slot): with_terms, row r's
        window is win_term / win_slot[win_off[r]:win_off[r+1]], the stream's term ids
        and each one's slot or -1 (snippet() renders it); else win_off is [0] and both
        are empty.  The index must keep positions (Index.positions)."""
        keep, ptrs = Index._typed_ptrs([term_ids, q_offsets, docnos, d_offsets], (np.int32, np.int64, np.int32, np.int64))
        nq = len(keep[1]) - 1
        r = _Passages()
        _check(lib().sme_query_passages(self._h, *ptrs, nq, int(width), int(min_cover), int(order), int(m),
                                        int(with_terms), C.byref(r)))
        counts = [nq + 1] + [r.total] * 7 + [r.total + 1 if with_terms else 1] + [r.win_total] * 2

        def arr(name, n, dt):
            ptr = getattr(r, name)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(Index._CT[dt])), (n,)).copy() if n else np.zeros(0, dt)
        return Passages(*[arr(f, n, dt) for f, n, dt in zip(_PASSAGE_FIELDS, counts, Index._PASSAGE_DTYPES)])

    def passages_device(self, term_ids, q_offsets, d_docnos, d_doc_offsets, width, min_cover=0, order=0, m=0,
                        with_terms=False, stream=None):
        """sme_query_passages_device: the candidates and their nq + 1 offsets in device
        memory (pointers, or contiguous int32 / int64 device tensors) -- the docno
        and res_off pointers of another feature's order 0 device call as they stand;
        the term ids and their offsets are host arrays.  Returns DevicePassages: the
        device pointers of Passages' arrays (0 for an empty one), total (the rows)
        and win_total; they belong to the index until its next passages call."""
        keep, ptrs = Index._typed_ptrs([term_ids, q_offsets], (np.int32, np.int64))
        nq = len(keep[1]) - 1
        dev = [C.c_void_p((x.data_ptr() if hasattr(x, "data_ptr") else x) or 0) for x in (d_docnos, d_doc_offsets)]
        r = _Passages()
        _check(lib().sme_query_passages_device(self._h, *ptrs, *dev, nq, int(width), int(min_cover), int(order),
                                               int(m), int(with_terms), C.c_void_p(stream or 0), C.byref(r)))
        return DevicePassages(*[getattr(r, f) or 0 for f in _PASSAGE_FIELDS], r.total, r.win_total)

    def passages_stats(self):
        """The last passages call: {"candidates": the batch's candidates, "with_record":
        those with at least one record, "positions": the stream positions of their
        records, "kept": the rows before the cut, "chunk": the window starts a wave of
        the scan takes at a time}."""
        c, w, p, k, ch = Index._stats(self._h, lib().sme_query_passages_stats, 5)
        return {"candidates": c, "with_record": w, "positions": p, "kept": k, "chunk": ch}

    def snippet(self, passages, row, vocabulary=None):
        """Row `row` of a with_terms Passages result as text, hits bracketed (snippet())."""
        a, e = int(passages.win_off[row]), int(passages.win_off[row + 1])
        return snippet(vocabulary if vocabulary is not None else self.terms(), passages.win_term[a:e],
                       passages.win_slot[a:e])

    def reweight(self, n_global, d_df_global=None, stream=None):
        """TF-IDF weights with all-reduced N (and df) of a doc-sharded index."""
        _check(lib().sme_index_reweight(self._h, n_global, C.c_void_p(d_df_global or 0), C.c_void_p(stream or 0)))

    def query_topk_device(self, d_terms, d_qoff, nq, k, d_out_docno, d_out_score, stream=None, d_out_tie=None):
        if d_out_tie is None:
            _check(lib().sme_query_topk_device(self._h, C.c_void_p(d_terms), C.c_void_p(d_qoff), nq, k,
                                               C.c_void_p(d_out_docno), C.c_void_p(d_out_score),
                                               C.c_void_p(stream or 0)))
        else:
            _check(lib().sme_query_topk_device_tie(self._h, C.c_void_p(d_terms), C.c_void_p(d_qoff), nq, k,
                                                   C.c_void_p(d_out_docno), C.c_void_p(d_out_score),
                                                   C.c_void_p(d_out_tie), C.c_void_p(stream or 0)))


class DeviceCorpus:
    """A synthetic Zipfian TREC corpus generated directly in HBM (sme_synth_corpus;
    the same bytes as synth.gen_corpus): docs d0 .. d0+n_docs-1."""

    def __init__(self, n_docs, V=1 << 20, seed=42, len_lo=400, len_hi=600, d0=0, device=0):
        from . import synth
        blob, voff = synth.make_vocab(V, seed)
        cdf = synth.zipf_cdf(V, 1.0)
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().sme_synth_corpus(device, blob, voff.ctypes.data, V, cdf.ctypes.data, n_docs, d0, seed, len_lo,
                                      len_hi, C.byref(p), C.byref(n)))
        self.ptr, self.nbytes = p.value, n.value

    def to_host(self):
        """Copy the corpus bytes back (hipMemcpy device -> host)."""
        out = np.zeros(max(self.nbytes, 1), np.uint8)
        _d2h(out, self.ptr, self.nbytes)
        return out[:self.nbytes].tobytes()

    def close(self):
        if getattr(self, "ptr", None):
            lib().sme_synth_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        self.close()


# ---------------------------------------------------------------------------
class CharGramOutput:
    """Output of the CharKGramTermIndexer job: the text of every reduce partition."""

    def __init__(self, h, ctx):
        self._h, self.ctx = h, ctx
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().sme_chargram_stats(h, C.byref(a), C.byref(b)))
        self.ngrams, self.npairs = a.value, b.value

    def close(self):
        if getattr(self, "_h", None):
            lib().sme_index_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def partition_text(self, part):
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().sme_chargram_partition_text(self._h, part, C.byref(p), C.byref(n)))
        return _host_bytes(p, n.value)


# reference-shaped facades
class GalagoTokenizer:
    """GalagoTokenizer.processContent, evaluated by the device tokenizer."""

    def __init__(self, ctx=None):
        self.ctx = ctx or Context()

    def processContent(self, text):  # noqa: N802 (reference name)
        return self.ctx.process_content(text)


class NumberTrecDocuments:
    """NumberTrecDocuments.run(input, output, mappingFile, nMappers) as one device
    call: returns (and optionally writes) the docno mapping file."""

    def __init__(self, device=0):
        self.ctx = Context(device=device)

    def run(self, corpus, mapping_file=None):
        corpus = open(corpus, "rb").read() if isinstance(corpus, str) else corpus
        m = self.ctx.number_documents(corpus)
        if mapping_file is not None:
            with open(mapping_file, "wb") as f:
                f.write(m)
        return m


class TermKGramDocIndexer:
    """TermKGramDocIndexer.run(K, input, output, mapping) as one device call.

    run() returns the Index; if output_dir is given, the reduce partitions are
    written as part-NNNNN files (SequenceFile v6 container, see seqfile.py).
    """

    def __init__(self, k=1, num_reduce_tasks=10, idf_mode=SME_IDF_REFERENCE, device=0):
        self.ctx = Context(k, num_reduce_tasks, idf_mode, device)

    def run(self, corpus, mapping, output_dir=None):
        corpus = open(corpus, "rb").read() if isinstance(corpus, str) else corpus
        mapping = open(mapping, "rb").read() if isinstance(mapping, str) else mapping
        self.ctx.load_docno_mapping(mapping)
        ix = self.ctx.build(corpus)
        if output_dir is not None:
            from . import seqfile
            seqfile.write_index_dir(ix, output_dir)
        return ix


class CharKGramTermIndexer:
    """CharKGramTermIndexer.run(K, input, output) as one device call (R = 10 reducers
    as the reference's run() sets); writes part-NNNNN text files if output_dir is given."""

    def __init__(self, k=2, num_reduce_tasks=10, device=0):
        self.ctx = Context(k, num_reduce_tasks, SME_IDF_REFERENCE, device)

    def run(self, corpus, output_dir=None):
        corpus = open(corpus, "rb").read() if isinstance(corpus, str) else corpus
        out = self.ctx.build_chargram(corpus)
        if output_dir is not None:
            os.makedirs(output_dir, exist_ok=True)
            for p in range(self.ctx.num_partitions):
                with open(os.path.join(output_dir, "part-%05d" % p), "wb") as f:
                    f.write(out.partition_text(p))
        return out


def _split_outside(text, seps, what):
    """text cut at the characters of seps (None: whitespace) that stand outside
    "..." and (...); unbalanced quotes or parentheses are a ValueError."""
    parts, cur, quoted, depth = [], [], False, 0
    for ch in text:
        if ch == '"':
            quoted = not quoted
        elif not quoted and ch == "(":
            depth += 1
        elif not quoted and ch == ")":
            depth -= 1
            if depth < 0:
                raise ValueError("structured query: ')' without '(' in %r" % what)
        if not quoted and depth == 0 and (ch.isspace() if seps is None else ch in seps):
            parts.append("".join(cur))
            cur = []
        else:
            cur.append(ch)
    if quoted:
        raise ValueError("structured query: unbalanced '\"' in %r" % what)
    if depth:
        raise ValueError("structured query: unbalanced '(' in %r" % what)
    parts.append("".join(cur))
    return parts


def parse_structured(text):
    """The structure of a query text, no index needed: a list of groups (leaves,
    excluded), every leaf a (kind, text, width) of strings -- ("term", word, 0),
    ("od", words, N) or ("uw", words, N).

    The text is split on whitespace outside quotes and parentheses; every piece is
    one group:
      -piece          a leading '-' excludes the group
      a|b|"c d"       '|' without spaces joins alternatives into one OR group
      "new york"      a phrase: the ordered window of width 1, ("od", "new york", 1)
      #od:N(a b c)    the ordered window: each next term at most N positions on
      #uw:N(a b c)    the unordered window: all the terms within N positions
      word            anything else, wildcards ('*', '?') included: ("term", word, 0)
    Unbalanced quotes or parentheses, an empty alternative, a window without a
    width of at least 1 and quotes or parentheses inside a word are a ValueError.
    IntDocVectorsForwardIndex.get_structured turns the strings into term ids."""
    import re
    groups = []
    for piece in _split_outside(text, None, text):
        if not piece:
            continue
        excluded = piece.startswith("-")
        leaves = []
        for alt in _split_outside(piece[1:] if excluded else piece, "|", piece):
            if not alt:
                raise ValueError("structured query: an empty alternative in %r" % piece)
            win = re.match(r"^#(od|uw):(\d+)\((.*)\)$", alt, re.S)
            if alt.startswith('"'):
                if len(alt) < 2 or not alt.endswith('"') or '"' in alt[1:-1]:
                    raise ValueError("structured query: text beside a quoted phrase in %r" % piece)
                leaves.append(("od", alt[1:-1], 1))
            elif win:
                if int(win.group(2)) < 1 or "(" in win.group(3) or ")" in win.group(3) or '"' in win.group(3):
                    raise ValueError("structured query: a malformed window in %r" % piece)
                leaves.append((win.group(1), win.group(3), int(win.group(2))))
            elif alt.startswith("#") or any(c in alt for c in '"()'):
                raise ValueError("structured query: a malformed leaf in %r" % piece)
            else:
                leaves.append(("term", alt, 0))
        groups.append((leaves, excluded))
    return groups


class IntDocVectorsForwardIndex:
    """Query side: getValue(terms) then rank() -> up to 10 docnos (score desc,
    docno asc), plus the REPL contract of IntDocVectorsForwardIndex.main
    (C/sa/edu/kaust/fwindex/IntDocVectorsForwardIndex.java:243-322) in query_line."""

    def __init__(self, index, mapping=None):
        self.index = index
        self._terms = []
        self._docids = None
        if mapping is not None:  # TrecDocnoMapping.loadMapping: {"", docids...}
            n = struct.unpack_from(">i", mapping, 0)[0]
            p, ids = 4, [""]
            for _ in range(n):
                ln = struct.unpack_from(">H", mapping, p)[0]
                ids.append(_mutf8_decode(mapping[p + 2:p + 2 + ln]))
                p += 2 + ln
            self._docids = ids

    @classmethod
    def from_dir(cls, ctx, index_dir, mapping=None, positions=False):
        """The reference's second program: open a reduce output directory
        (part-00000 ...) written earlier -- by TermKGramDocIndexer.run here or by
        the Hadoop job -- and answer queries from it (IntDocVectorsForwardIndex
        ctor, IntDocVectorsForwardIndex.java:93-122).  positions: also attach the
        term streams of the directory's positions file (seqfile.write_positions),
        so phrase and proximity queries work; FileNotFoundError if it is missing."""
        from . import seqfile
        ix = seqfile.load_index_dir(ctx, index_dir)
        if positions:
            seqfile.attach_positions(ix, index_dir)
        return cls(ix, mapping)

    def merged(self, other, *more):
        """A forward index over the merge (Context.merge) of this one's index and the
        others' -- IntDocVectorsForwardIndex or Index objects of the same context,
        numbered with the same docno mapping, which the result keeps.  "Add these
        documents" without rebuilding; this index stays as it is."""
        idx = [self.index] + [getattr(o, "index", o) for o in (other,) + more]
        out = IntDocVectorsForwardIndex(self.index.ctx.merge(idx))
        out._docids = self._docids
        return out

    def without(self, docs):
        """A forward index over this one's index without the given documents
        (Index.delete_docnos): `docs` holds docnos (ints) and/or docid strings, the
        strings resolved through the docno mapping this object holds -- an unknown
        docid, or a docid without a mapping, raises ValueError.  The result keeps the
        mapping; this index stays as it is.  Replacing a document is a deletion and a
        merge with a build of its new text:

            fresh = fwd.without(["FT911-3"]).merged(ctx.build(new_text_of_ft911_3))
        """
        docnos, by_id = [], None
        for d in docs:
            if isinstance(d, str):
                if self._docids is None:
                    raise ValueError("docid %r: this forward index holds no docno mapping" % d)
                if by_id is None:
                    by_id = {s: i for i, s in enumerate(self._docids) if i > 0}
                if d not in by_id:
                    raise ValueError("docid %r is not in the docno mapping" % d)
                docnos.append(by_id[d])
            else:
                docnos.append(int(d))
        out = IntDocVectorsForwardIndex(self.index.delete_docnos(docnos))
        out._docids = self._docids
        return out

    def getValue(self, terms):  # noqa: N802
        ids = self.index.lookup(list(terms))
        self._terms = [int(t) for t in ids if t >= 0]  # unknown terms are skipped silently

    def get_wildcard(self, words):
        """getValue with wildcard words: a word holding '*' or '?' is lower-cased
        (str.lower) and expanded against the vocabulary (Index.expand_wildcards);
        the other words go through processContent and the term lookup as
        getValue's callers send them.  The query becomes the plain terms in order,
        then each pattern's matches in order; a term reached twice counts twice, as
        duplicates do in sme_query_topk.  rank() then works unchanged -- an
        expansion past the query side's limit of 1024 terms per query surfaces
        there, as the SmeError (SME_ELIMIT) query_topk raises."""
        words = list(words)
        pats = [w.lower() for w in words if "*" in w or "?" in w]
        plain = [w for w in words if not ("*" in w or "?" in w)]
        toks = []
        for w in plain:
            toks.extend(self.index.ctx.process_content(w))
        self._terms = [int(t) for t in self.index.lookup(toks) if t >= 0]
        if pats:
            _, ids = self.index.expand_wildcards(pats)
            self._terms.extend(int(t) for t in ids)

    def get_corrected(self, words, max_dist=2):
        """getValue with spelling correction: every word goes through
        processContent; a token the lookup knows is kept, an unknown one is
        replaced by its best suggestion (Index.suggest_terms with m = 1: the
        nearest term within max_dist unit edits, the most frequent among equals)
        if there is one and skipped as getValue skips it otherwise.  Sets the
        query terms for rank() and returns the replacements made, a list of
        (token, replacement term string)."""
        toks = []
        for w in words:
            toks.extend(self.index.ctx.process_content(w))
        ids = [int(t) for t in self.index.lookup(toks)]
        unknown = [i for i, t in enumerate(ids) if t < 0]
        made = []
        if unknown:
            off, sug, _ = self.index.suggest_terms([toks[i] for i in unknown], max_dist, 1)
            for j, i in enumerate(unknown):
                if off[j + 1] > off[j]:
                    ids[i] = int(sug[off[j]])
                    made.append((toks[i], self.index.term(ids[i])))
        self._terms = [t for t in ids if t >= 0]
        return made

    def get_boolean(self, words):
        """A Boolean query from whitespace-separated words: every word is one
        group, excluded if it starts with '-'.  A word holding '*' or '?' is
        lower-cased and expanded (Index.expand_wildcards) into one OR-group; any
        other word goes through processContent and each resulting token is a
        group of its own -- a word that yields no token (a stopword) is dropped,
        an unknown token is a group holding -1, so a required unknown word gives
        no results.  Sets the groups for rank_boolean() and returns them, a list
        of (term_ids, excluded).  A query holds at most 1024 term ids over all
        its groups and at most 64 groups (include/sme.h): a wildcard word whose
        expansion, with the other words' terms, passes that is not cut short --
        rank_boolean() then raises the SmeError (SME_ELIMIT) query_boolean
        raises, as rank() does after get_wildcard."""
        groups = []
        for w in words:
            excluded = w.startswith("-")
            if excluded:
                w = w[1:]
            if "*" in w or "?" in w:
                _, ids = self.index.expand_wildcards([w.lower()])
                groups.append(([int(t) for t in ids], excluded))
            else:
                toks = self.index.ctx.process_content(w)
                if toks:
                    groups.extend(([int(t)], excluded) for t in self.index.lookup(toks))
        self._groups = groups
        return groups

    def _scorer(self, scorer):
        """The scorer's name checked before a query runs for it."""
        if scorer not in ("bm25", "tfidf"):
            raise ValueError("scorer must be None, \"bm25\" or \"tfidf\", not %r" % (scorer,))
        return scorer

    def _rescored(self, device_result, slots, scorer, k, k1, b):
        """The one query of a feature's order 0, m 0 device result (res_off, docno,
        ..., total) ranked by `scorer` over `slots`: the first k docnos."""
        slots = np.array(slots, np.int32)
        off, dn = device_result[0], device_result[1]
        r = self.index.rescore_device(slots, np.array([0, len(slots)], np.int64), dn, off, model=scorer, order=1, m=k,
                                      min_hits=0, k1=k1, b=b)
        total = r[4]
        out = np.zeros(max(total, 1), np.int32)
        if total:
            _d2h(out, r[1], 4 * total)
        return [int(d) for d in out[:total]]

    def rank_boolean(self, k=10, scorer=None, k1=1.2, b=0.75):
        """The first k documents (score desc, docno asc) matching get_boolean's groups.
        scorer "bm25" or "tfidf": the matches ranked by that model over the required
        groups' terms in listed order (Index.rescore_device over the device result;
        k1, b: BM25's parameters); None: by the Boolean score."""
        groups = getattr(self, "_groups", [])
        if scorer is None:
            _, dn, _ = self.index.query_boolean([groups], order=1, m=k)
            return [int(d) for d in dn]
        self._scorer(scorer)
        slots = [int(t) for ids, excluded in groups if not excluded for t in ids]
        return self._rescored(self.index.query_boolean_device([groups], order=0, m=0), slots, scorer, k, k1, b)

    def get_phrase(self, text):
        """An exact phrase from a text: processContent (stop words are dropped as
        the indexer drops them, so the phrase is what the indexer saw of the
        text) -> the term lookup -> one phrase for rank_phrase(); an unknown
        token stays as -1, so the phrase then has no results.  Returns the term
        ids.  The index must keep positions (Index.positions)."""
        toks = self.index.ctx.process_content(text)
        self._phrase = [int(t) for t in self.index.lookup(toks)] if toks else []
        return self._phrase

    def rank_phrase(self, k=10, scorer=None, k1=1.2, b=0.75):
        """The first k documents (score desc, docno asc) holding get_phrase's phrase.
        scorer "bm25" or "tfidf": the matches ranked by that model over the phrase's
        terms (Index.rescore_device); None: by the phrase score."""
        phrase = getattr(self, "_phrase", [])
        if scorer is None:
            _, dn, _, _ = self.index.query_phrase([phrase], order=1, m=k)
            return [int(d) for d in dn]
        self._scorer(scorer)
        return self._rescored(self.index.query_phrase_device([phrase], order=0, m=0), phrase, scorer, k, k1, b)

    def get_near(self, text, width, ordered=False):
        """A proximity query from a text: processContent -> the term lookup, as
        get_phrase (an unknown token stays as -1: no results), with the width and
        whether the terms must stand in the text's order (#od:width) or only
        within `width` positions of each other (#uw:width).  Sets the query for
        rank_near() and returns it, (term_ids, width, ordered)."""
        toks = self.index.ctx.process_content(text)
        ids = [int(t) for t in self.index.lookup(toks)] if toks else []
        self._near = (ids, int(width), bool(ordered))
        return self._near

    def rank_near(self, k=10, scorer=None, k1=1.2, b=0.75):
        """The first k documents (score desc, docno asc) matching get_near's query.
        scorer "bm25" or "tfidf": the matches ranked by that model over the window's
        terms (Index.rescore_device); None: by the proximity score."""
        near = getattr(self, "_near", ([], 1, False))
        if scorer is None:
            _, dn, _, _ = self.index.query_near([near], order=1, m=k)
            return [int(d) for d in dn]
        self._scorer(scorer)
        return self._rescored(self.index.query_near_device([near], order=0, m=0), near[0], scorer, k, k1, b)

    def get_passages(self, query, docnos, width=32):
        """Where the query matched in the given documents: the text goes through
        processContent and the term lookup (unknown tokens skipped), the docnos are
        sorted and repeats dropped, and every document's best window of at most
        `width` positions comes back (Index.passages, every candidate kept, in docno
        order) as a list of dicts: docno, rec, start, len, hits, cover (the distinct
        query terms in the window), score and snippet, the window's terms with the
        hits in square brackets.  A docno without a record has rec -1 and an empty
        snippet.  The index must keep positions (Index.positions)."""
        ids = [int(t) for t in self.index.lookup(self.index.ctx.process_content(query)) if t >= 0]
        cands = sorted(set(int(d) for d in docnos))
        r = self.index.passages(ids, [0, len(ids)], cands, [0, len(cands)], width, with_terms=True)
        if getattr(self, "_vocabulary", None) is None:
            self._vocabulary = self.index.terms()
        return [{"docno": int(r.docno[i]), "rec": int(r.rec[i]), "start": int(r.start[i]), "len": int(r.len[i]),
                 "hits": int(r.hits[i]), "cover": bin(int(r.mask[i])).count("1"), "score": float(r.score[i]),
                 "snippet": self.index.snippet(r, i, self._vocabulary)} for i in range(len(r.docno))]

    def get_similar(self, docno, terms=25):
        """More like this: the `terms` best feedback terms of the one document
        `docno` (Index.feedback_terms with its defaults, so the DOCNO's own tokens
        are left out) become the query for rank_similar().  Returns the term ids,
        best first; none if no record carries the docno."""
        _, ids, _, _, _ = self.index.feedback_terms([[int(docno)]], m=terms)
        self._similar = (int(docno), [int(t) for t in ids])
        return self._similar[1]

    def rank_similar(self, k=10):
        """The first k documents (score desc, docno asc) for get_similar's terms,
        the source document itself removed."""
        docno, ids = getattr(self, "_similar", (-1, []))
        if not ids:
            return []
        dn, _ = self.index.query_topk(np.array(ids, np.int32), np.array([0, len(ids)], np.int64), k + 1)
        return [int(d) for d in dn[0] if d >= 0 and d != docno][:k]

    def rank_feedback(self, text, k=10, fb_docs=10, fb_terms=20):
        """One query with pseudo-relevance feedback: processContent -> the term
        lookup (unknown tokens skipped, as getValue skips them) ->
        Index.query_feedback.  Returns the first k docnos."""
        ids = [int(t) for t in self.index.lookup(self.index.ctx.process_content(text)) if t >= 0]
        if not ids:
            return []
        dn, _, _, _ = self.index.query_feedback(np.array(ids, np.int32), np.array([0, len(ids)], np.int64), k, fb_docs,
                                                fb_terms)
        return [int(d) for d in dn[0] if d >= 0]

    def get_structured(self, text):
        """A structured query from a text in parse_structured's syntax:
        `"new york" hotel* -"times square"`, `#uw:8(network protocol) tcp|udp`.
        A word holding '*' or '?' is lower-cased and expanded
        (Index.expand_wildcards) into term leaves of its group; any other word
        goes through processContent -- standing alone, every token it yields is a
        group of its own (a word that yields none, a stop word, is dropped; an
        unknown token is -1), in an OR group its tokens join the group, all as
        get_boolean does.  Phrase and window texts go through processContent and
        the lookup as get_phrase's (an unknown token stays -1: the leaf is empty).
        Sets the query for rank_structured() and returns it, a list of (leaves,
        excluded) with leaves (term_ids, kind, width) as Index.query_structured
        takes them.  A window needs an index that keeps positions."""
        kinds = {"od": 1, "uw": 2}
        groups = []
        for leaves, excluded in parse_structured(text):
            out, had_other = [], False
            for kind, body, width in leaves:
                if kind != "term":
                    toks = self.index.ctx.process_content(body)
                    ids = [int(t) for t in self.index.lookup(toks)] if toks else []
                    out.append((ids, kinds[kind], width))
                    had_other = True
                elif "*" in body or "?" in body:
                    _, ids = self.index.expand_wildcards([body.lower()])
                    out.extend(([int(t)], 0, 0) for t in ids)
                    had_other = True
                else:
                    toks = self.index.ctx.process_content(body)
                    ids = [int(t) for t in self.index.lookup(toks)] if toks else []
                    if len(leaves) == 1:  # a word alone: a group per token
                        groups.extend(([([t], 0, 0)], excluded) for t in ids)
                    else:
                        out.extend(([t], 0, 0) for t in ids)
            if out or had_other:
                groups.append((out, excluded))
        self._structured = groups
        return groups

    def rank_structured(self, k=10, scorer=None, k1=1.2, b=0.75):
        """The first k documents (score desc, docno asc) matching get_structured's query.
        scorer "bm25" or "tfidf": the matches ranked by that model over the term ids
        of all leaves of the required groups, in listed order (Index.rescore_device);
        None: by the structured score."""
        groups = getattr(self, "_structured", [])
        if scorer is None:
            _, dn, _ = self.index.query_structured([groups], order=1, m=k)
            return [int(d) for d in dn]
        self._scorer(scorer)
        slots = [int(t) for leaves, excluded in groups if not excluded for ids, _, _ in leaves for t in ids]
        return self._rescored(self.index.query_structured_device([groups], order=0, m=0), slots, scorer, k, k1, b)

    def rank(self, k=10):
        if not self._terms:
            return []
        dn, _ = self.index.query_topk(np.array(self._terms, np.int32), np.array([0, len(self._terms)], np.int64), k)
        return [int(d) for d in dn[0] if d >= 0]

    def rank_bm25(self, k=10, k1=1.2, b=0.75):
        """rank() by BM25 score (Index.query_bm25) over the terms getValue set."""
        if not self._terms:
            return []
        dn, _ = self.index.query_bm25(np.array(self._terms, np.int32), np.array([0, len(self._terms)], np.int64), k,
                                      k1, b)
        return [int(d) for d in dn[0] if d >= 0]

    def query_line(self, line, tokenizer=None):
        """One REPL turn (:284-320): trim; an empty line, or one that is not 1-2
        raw words (String.split("\\s+")), ends the session (returns None);
        otherwise processContent -> getValue -> rank, printed as main prints it:
        Arrays.toString of the docnos, or the docids each followed by a space
        (mapping given), or "No results ..."."""
        import re
        term = line
        b, e = 0, len(term)
        while b < e and ord(term[b]) <= 0x20:  # String.trim
            b += 1
        while e > b and ord(term[e - 1]) <= 0x20:
            e -= 1
        term = term[b:e]
        if not term:
            return None
        orig = re.split(r"[ \t\n\x0b\f\r]+", term)
        if len(orig) not in (1, 2):
            return None
        ctx = tokenizer or self.index.ctx
        self.getValue(ctx.process_content(term))
        res = self.rank()
        if self._docids is None:
            body = ("[" + ", ".join(str(d) for d in res) + "]") if res else "No results ..."
        else:
            body = "".join(self._docids[d] + " " for d in res) if res else "No results ..."
        return term + ": " + body
