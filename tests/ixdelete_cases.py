"""Generated corpora for the index deletion tests (tests/test_gpu_ixdelete.py), in
the style of ixmerge_cases.py, whose document form they share: docids are "D%06d"
over the mapping D000001 .. D{NMAP}, so docno = the number in the docid, and a
document is (docid spec, text) with a spec an int (that docno), None (no DOCNO:
docno 0) or a string (a literal docid; outside the mapping: a negative docno).  The
expected index of a deletion is simply the build of the documents whose docno is
not deleted (`remaining`).

The edge cases are laid out for "delete_tile" 256, the smallest: the docid of
every document is a term of its own ("d000123"), so a case's own terms start with
a letter before "d" and come first in the vocabulary -- their postings then sit
where the case says in the flat docno-order array."""
import bisect
import random

import common
from ixmerge_cases import NMAP, corpus_bytes, doc_bytes, mapping_ids  # noqa: F401  (shared document form)

T = 256  # the tile the layouts are made for


def docno_of(spec, ids=None):
    """The docno TrecDocnoMapping gives a docid spec (ids: the sorted mapping;
    default this module's): Arrays.binarySearch over {"", ids...}."""
    if spec is None:
        return 0
    if isinstance(spec, int):
        return spec
    arr = [""] + list(mapping_ids() if ids is None else ids)
    i = bisect.bisect_left(arr, spec)
    return i if i < len(arr) and arr[i] == spec else -i - 1


def remaining(docs, deleted, ids=None):
    gone = set(int(d) for d in deleted)
    return [(s, t) for s, t in docs if docno_of(s, ids) not in gone]


# ---- the fuzz corpus, document by document ------------------------------------------
def fuzz_documents(seed, n_docs):
    """common.fuzz_corpus's documents with its docid quirks (no DOCNO, a docid twice,
    a docid outside the mapping) but without its junk before and after, so record i
    is document i: ([(docid or None, the document's bytes)], sorted mapping ids)."""
    rng = random.Random(seed)
    ids = ["FZ%06d-%02d" % (i, rng.randint(0, 99)) for i in range(n_docs)]
    docs = []
    for i, d in enumerate(ids):
        choice = rng.random()
        docid = d
        if choice < 0.03:
            docid = None
        elif choice < 0.06:
            docid = ids[rng.randrange(max(i, 1))]
        elif choice < 0.08:
            docid = "MISSING%d" % i
        docs.append((docid, common.fuzz_doc(rng, docid, rng.randint(0, 80)).encode("utf-8")))
    return docs, sorted(set(ids))


# ---- edge cases: (documents, docnos to delete) ------------------------------------------
def _docs(by_docno):
    return [(d, " ".join(w)) for d, w in sorted(by_docno.items())]


SURVIVE = (0, 1, 63, 64, 65, 255, 256)


def survivors_case():
    """Seven terms of exactly one tile each (term j is tile j): 0, 1, 63, 64, 65, 255
    and all of the tile's postings survive."""
    docs, gone = {}, []
    for j, k in enumerate(SURVIVE):
        base = 1 + 300 * j
        for i in range(T):
            docs.setdefault(base + i, []).append("a%02dk%d" % (j, k))
        gone += [base + i for i in range(k, T)]
    return _docs(docs), gone


def long_list_case():
    """One list of three tiles + 1: the last posting of tile 0 and the first of tile 1
    go, and tile 2 is left without a survivor."""
    docs = {1 + i: ["b0long"] for i in range(3 * T + 1)}
    gone = [T, T + 1] + [2 * T + 1 + i for i in range(T)]
    return _docs(docs), gone


def vanishing_terms_case():
    """Terms held only by deleted documents vanish: the first term of the vocabulary
    (at a tile's start), one at a tile's end, one spanning whole tiles, runs of 1, 2,
    64 and 65 consecutive vanishing terms between kept ones, and the last term of
    the vocabulary.  (The deleted documents' docid terms are one more long run.)"""
    plan = [(10, True), (T - 20, False), (10, True), (2 * T + 88, True), (5, False)]
    for run in (1, 2, 64, 65):
        plan += [(1, True)] * run + [(3, False)]
    docs, names = {}, []
    for i, (n, vanish) in enumerate(plan):
        name = "c%04dv%d" % (i, 1 if vanish else 0)
        names.append(name)
        for x in range(n):
            docs.setdefault((1 if vanish else 5001) + x, []).append(name)
    docs[1].append("zz9")  # after every docid term
    gone = [d for d in docs if d < 5001]
    return _docs(docs), gone, names


def stream_len_case():
    """Records of 0, 1, 63, 64, 65 stream positions besides the docid's, alternately
    deleted and kept; every length on either side."""
    docs, gone = [], []
    for i, k in enumerate((0, 1, 63, 64, 65) * 2):
        docs.append((100 + i, " ".join("w%d" % (x % 7) for x in range(k))))
        if i % 2:
            gone.append(100 + i)
    return docs, gone


def duplicate_case():
    """A docid held by two records and by three, two records without DOCNO, and two
    different docids outside the mapping (MISSING7 sorts after every mapped docid,
    AMISSING before: two negative docnos)."""
    return [(39, "plain before"), (40, "intwo twice"), (41, "inthree inthree"), (None, "nodocno zero"),
            ("MISSING7", "unmapped neg"), (40, "intwo again shared"), (41, "inthree"), ("AMISSING", "unmapped other"),
            (None, "nodocno again"), (41, "inthree third shared"), ("MISSING7", "unmapped more"), (50, "plain shared")]


def large_tf_case(stays):
    """A document with tf 1200 is deleted: max_tf falls to 600, under kTfSortMaxTf =
    1023 -- or, `stays`, another document keeps it at 1100."""
    docs = [(7, " ".join(["big"] * 1200) + " tail"), (8, " ".join(["big"] * 600)), (9, "big small")]
    if stays:
        docs.append((10, " ".join(["big"] * 1100)))
    return docs, [7]
