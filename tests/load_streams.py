"""Record streams written in Python for the loader tests (sme_index_from_records):
the reduce output's framing (include/sme.h, sme_index_partition_records), valid
and malformed.  Shared by test_gpu_load.py and test_recparse_host.py, so the host
sanitizer check and the device loader see exactly the same bytes."""
import struct

import numpy as np

POSTING_CLASS = b"sa.edu.kaust.io.PostingWritable"

# csrc/sme_recparse.hpp codes
RP_OK, RP_TRUNC, RP_PAST_END, RP_KEYLEN, RP_KGRAM, RP_CLASS, RP_MUTF8 = 0, 2, 4, 5, 6, 9, 10
RP_KEY_ORDER, RP_KEY_DUP, RP_POST_ORDER, RP_DOCNO_DUP = 11, 12, 18, 19
SME_EINVAL, SME_EPARSE, SME_ENOTIMPL = -1, -4, -7


def record(term, posts, df=1, cls=POSTING_CLASS, more=(), rec_len_add=0, key_len_add=0):
    """One framed record; term / more: writeUTF bodies (bytes), posts: [(docno, tf)]
    or an (n, 2) integer array."""
    key = struct.pack(">i", 1 + len(more)) + struct.pack(">H", len(term)) + term
    for m in more:
        key += struct.pack(">H", len(m)) + m
    key += struct.pack(">i", df)
    n = len(posts)
    val = struct.pack(">i", n)
    if n:
        val += struct.pack(">H", len(cls)) + cls + np.asarray(posts, dtype=">i4").reshape(n, 2).tobytes()
    return struct.pack(">ii", len(key) + len(val) + rec_len_add, len(key) + key_len_add) + key + val


def counter(posts, df=None):
    """The " " doc-counter record."""
    return record(b" ", posts, df=len(posts) if df is None else df)


def counter_posts(docnos):
    """One map task's list: (0,0), then every record's docno but the last."""
    return [(0, 0)] + [(int(d), 1) for d in docnos[:-1]]


def java_partition(term_utf16_units, R):
    """HashPartitioner over TermDF.hashCode = Arrays.hashCode({term}) (TermDF.java:79-81)."""
    h = 0
    for u in term_utf16_units:
        h = (31 * h + u) & 0xFFFFFFFF
    return ((31 + h) & 0x7FFFFFFF) % R


SP = counter([(0, 0), (7, 1), (9, 1)])
APPLE = record(b"apple", [(9, 3), (7, 1), (12, 1)])
BERRY = record(b"berry", [])
CAFE = record("café€".encode("utf-8"), [(7, 2)])  # 2- and 3-byte units (as modified UTF-8 writes them)
VALID = [SP + APPLE + BERRY, CAFE]  # two partitions


def refused():
    """[(name, partitions, recparse code, sme code)]: every stream has one defect."""
    return [
        ("truncated_tail", [(SP + APPLE)[:-5]], RP_PAST_END, SME_EPARSE),
        ("stray_tail", [SP + APPLE + b"\x00\x00"], RP_TRUNC, SME_EPARSE),
        ("reclen_past_end", [SP + record(b"apple", [(9, 3)], rec_len_add=4096)], RP_PAST_END, SME_EPARSE),
        ("bad_keylen", [SP + record(b"apple", [(9, 3)], key_len_add=1)], RP_KEYLEN, SME_EPARSE),
        ("unsorted_keys", [SP + BERRY + APPLE], RP_KEY_ORDER, SME_EPARSE),
        ("key_in_two_partitions", [SP + APPLE, APPLE + BERRY], RP_KEY_DUP, SME_EPARSE),
        ("tf_order", [SP + record(b"apple", [(9, 1), (7, 3)])], RP_POST_ORDER, SME_EPARSE),
        ("docno_order", [SP + record(b"apple", [(9, 2), (7, 2)])], RP_POST_ORDER, SME_EPARSE),
        ("duplicate_docno", [SP + record(b"apple", [(9, 3), (7, 1), (9, 1)])], RP_DOCNO_DUP, SME_EPARSE),
        ("wrong_class", [SP + record(b"apple", [(9, 3)], cls=b"sa.edu.kaust.io.PostingWritablf")], RP_CLASS,
         SME_EPARSE),
        ("bad_mutf8", [SP + record(b"a\x80z", [(9, 1)])], RP_MUTF8, SME_EPARSE),
        ("k2_key", [SP + record(b"apple", [(9, 1)], more=(b"pie",))], RP_KGRAM, SME_ENOTIMPL),
    ]


def walk(body):
    """Framed records of a part file body, sync escapes skipped."""
    out, i = [], 0
    while i < len(body):
        rl = struct.unpack_from(">i", body, i)[0]
        if rl == -1:
            i += 20
            continue
        out.append(bytes(body[i:i + 8 + rl]))
        i += 8 + rl
    return out
